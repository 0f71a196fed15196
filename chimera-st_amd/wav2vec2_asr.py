"""CTC fine-tuning of wav2vec2 — mirror of fairseq/models/wav2vec/wav2vec2_asr.py: add_common_args (:19-143), Wav2VecCtc (:146-181),
Wav2VecEncoder (:304-415) and the wav2vec_ctc architecture (:630-653).  wav2vec_seq2seq is not built.

State-dict keys are the reference's: w2v_encoder.w2v_model.* (the wav2vec2 model WITHOUT its pre-training heads,
remove_pretraining_modules) and w2v_encoder.proj.*.  The projection runs through CF.linear and the criterion takes the raw logits
(criterions.CtcCriterion -> CF.ctc_loss): no log-probability tensor is built on the training path."""
import contextlib
import copy

import torch

from . import functional as CF
from .distributed import notify_unused_parameters
from .fairseq_model import BaseFairseqModel, FairseqEncoder
from .modules import Linear, to_time_major_view
from .registry import register_model, register_model_architecture
from .wav2vec2 import Wav2Vec2Model
from .wav2vec2 import base_architecture as w2v_base_architecture


def add_common_args(parser):
    """:19-143."""
    parser.add_argument("--w2v-path", help="path to wav2vec 2.0 model (or synthetic:<name>)")
    parser.add_argument("--no-pretrained-weights", action="store_true")
    parser.add_argument("--dropout-input", type=float, metavar="D")
    parser.add_argument("--final-dropout", type=float, metavar="D")
    parser.add_argument("--apply-mask", action="store_true")
    parser.add_argument("--dropout", type=float, metavar="D")
    parser.add_argument("--attention-dropout", type=float, metavar="D")
    parser.add_argument("--activation-dropout", "--relu-dropout", type=float, metavar="D")
    parser.add_argument("--mask-length", type=int)
    parser.add_argument("--mask-prob", type=float)
    parser.add_argument("--mask-selection", type=str, choices=["static", "uniform", "normal", "poisson"])
    parser.add_argument("--mask-other", type=float)
    parser.add_argument("--no-mask-overlap", action="store_true")
    parser.add_argument("--mask-channel-length", type=int)
    parser.add_argument("--mask-channel-prob", type=float)
    parser.add_argument("--mask-channel-selection", type=str, choices=["static", "uniform", "normal", "poisson"])
    parser.add_argument("--mask-channel-other", type=float)
    parser.add_argument("--no-mask-channel-overlap", action="store_true")
    parser.add_argument("--freeze-finetune-updates", default=0, type=int)
    parser.add_argument("--feature-grad-mult", type=float)  # (no default: the architecture function supplies 0)
    parser.add_argument("--layerdrop", default=0.0, type=float)


@register_model("wav2vec_ctc")
class Wav2VecCtc(BaseFairseqModel):
    single_use_parameters = True  # one forward pass uses every parameter once (trainer.py: deferred reductions)

    @staticmethod
    def add_args(parser):
        add_common_args(parser)

    def __init__(self, w2v_encoder, args):
        super().__init__()
        self.w2v_encoder = w2v_encoder
        self.args = args

    @classmethod
    def build_model(cls, args, task):
        base_architecture(args)
        return cls(Wav2VecEncoder(args, task.target_dictionary), args)

    def get_normalized_probs(self, net_output, log_probs, sample=None):
        """:169-176 — for interop; the criterion here reads net_output["encoder_out"] directly."""
        logits = net_output["encoder_out"]
        return torch.log_softmax(logits.float(), dim=-1) if log_probs else torch.softmax(logits.float(), dim=-1)

    def get_logits(self, net_output):
        return net_output["encoder_out"]

    def forward(self, **kwargs):
        return self.w2v_encoder(**kwargs)

    def set_num_updates(self, num_updates):
        self.w2v_encoder.set_num_updates(num_updates)

    def max_positions(self):
        return None


class Wav2VecEncoder(FairseqEncoder):
    def __init__(self, args, tgt_dict=None):
        super().__init__(None)
        from .w2v2_transformer import load_w2v_checkpoint
        self.apply_mask = args.apply_mask
        overrides = {
            "dropout": args.dropout, "activation_dropout": args.activation_dropout, "dropout_input": args.dropout_input,
            "attention_dropout": args.attention_dropout, "mask_length": args.mask_length, "mask_prob": args.mask_prob,
            "mask_selection": args.mask_selection, "mask_other": args.mask_other, "no_mask_overlap": args.no_mask_overlap,
            "mask_channel_length": args.mask_channel_length, "mask_channel_prob": args.mask_channel_prob,
            "mask_channel_selection": args.mask_channel_selection, "mask_channel_other": args.mask_channel_other,
            "no_mask_channel_overlap": args.no_mask_channel_overlap, "encoder_layerdrop": args.layerdrop,
            "feature_grad_mult": args.feature_grad_mult,
        }
        if getattr(args, "w2v_args", None) is None:
            # (:327-331: the pre-trained checkpoint's arguments with this model's overrides; kept in args.w2v_args so that a
            #  checkpoint of THIS model can be rebuilt without the pre-trained file)
            state = load_w2v_checkpoint(args.w2v_path)
            w2v_args = copy.deepcopy(state["args"])
            for k, v in overrides.items():
                setattr(w2v_args, k, v)
            args.w2v_args = w2v_args
            model = Wav2Vec2Model.build_model(w2v_args, task=None)  # with the heads: the pre-trained file carries them
            if state["model"] is not None and not args.no_pretrained_weights:
                model.load_state_dict(state["model"], strict=True)
            model.remove_pretraining_modules()
        else:
            w2v_args = args.w2v_args
            w2v_base_architecture(w2v_args)
            model = Wav2Vec2Model(w2v_args, pretraining_heads=False)
        assert getattr(args, "normalize", False) == getattr(w2v_args, "normalize", False), \
            "Fine-tuning works best when data normalization is the same"
        # the loss reads no frame at or past an utterance's end (cst_ctc_fwd): the padding rows of the layer stack are never consumed
        model.encoder.padding_rows_consumed = False
        model.encoder.padding_rows_read = 0
        self.w2v_model = model
        self.final_dropout_p = float(args.final_dropout)
        self.freeze_finetune_updates = args.freeze_finetune_updates
        self.num_updates = 0
        d = w2v_args.encoder_embed_dim
        if tgt_dict is not None:
            self.proj = Linear(d, len(tgt_dict))
        elif getattr(args, "decoder_embed_dim", d) != d:
            self.proj = Linear(d, args.decoder_embed_dim)
        else:
            self.proj = None

    def set_num_updates(self, num_updates):
        self.num_updates = num_updates

    def forward(self, source, padding_mask, tbc=True, **kwargs):
        """:371-397."""
        masking = bool(self.apply_mask and self.training)
        ft = self.freeze_finetune_updates <= self.num_updates
        if not ft and self.training and torch.is_grad_enabled():
            # the frozen stack fires no gradient hook (the model itself reports mask_emb where it is not used)
            reported = masking and self.w2v_model.mask_prob > 0
            notify_unused_parameters([p for p in self.w2v_model.parameters() if reported or p is not self.w2v_model.mask_emb])
        with torch.no_grad() if not ft else contextlib.ExitStack():
            x, padding_mask = self.w2v_model.extract_features(source, padding_mask, mask=masking)
        if self.training and self.final_dropout_p > 0:
            x = CF.dropout(x, self.final_dropout_p)
        if self.proj is not None:
            x = self.proj(x)
        if tbc:
            x = to_time_major_view(x)  # B x T x C -> T x B x C without a copy: the CTC kernels read this view
        return {"encoder_out": x, "encoder_padding_mask": padding_mask, "padding_mask": padding_mask}

    def reorder_encoder_out(self, encoder_out, new_order):
        if encoder_out["encoder_out"] is not None:
            encoder_out["encoder_out"] = encoder_out["encoder_out"].index_select(1, new_order)
        if encoder_out["encoder_padding_mask"] is not None:
            encoder_out["encoder_padding_mask"] = encoder_out["encoder_padding_mask"].index_select(0, new_order)
            encoder_out["padding_mask"] = encoder_out["encoder_padding_mask"]
        return encoder_out

    def max_positions(self):
        return None


@register_model_architecture("wav2vec_ctc", "wav2vec_ctc")
def base_architecture(args):
    """:630-653."""
    d = dict(no_pretrained_weights=False, dropout_input=0, final_dropout=0, apply_mask=False, dropout=0, attention_dropout=0,
             activation_dropout=0, mask_length=10, mask_prob=0.5, mask_selection="static", mask_other=0, no_mask_overlap=False,
             mask_channel_length=10, mask_channel_prob=0.5, mask_channel_selection="static", mask_channel_other=0,
             no_mask_channel_overlap=False, freeze_finetune_updates=0, feature_grad_mult=0, layerdrop=0.0)
    for k, v in d.items():
        # (a flag the parser leaves at None — the reference declares --feature-grad-mult with default=None — takes the default too:
        #  the override would otherwise write None into the wav2vec2 arguments)
        setattr(args, k, v if getattr(args, k, None) is None else getattr(args, k))
