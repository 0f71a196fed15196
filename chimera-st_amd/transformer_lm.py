"""Target-side Transformer language model: trained by the `language_modeling` task (tasks.py, criterion `cross_entropy`), scored by
fairseq_eval_lm.py and used for shallow fusion in decoding (`--lm-path`, `--lm-weight`) — mirror of
fairseq/models/transformer_lm.py (TransformerLanguageModel :165-246, base_lm_architecture :250-306 and the named architectures)
and fairseq/models/fairseq_model.py FairseqLanguageModel: a TransformerDecoder WITHOUT encoder attention over the target dictionary.

The state_dict keys are the reference's (`decoder.embed_tokens.weight`, `decoder.layers.<i>.self_attn.*`, `decoder.layers.<i>.fc1.*`,
`decoder.layer_norm.*`, `decoder.output_projection.weight`, ...), so a reference LM checkpoint loads strictly, and one written here
loads in the reference.  In decoding, sequence_generator.py adds lm_weight x its next-token log-softmax to the translation model's
log-probabilities (reference sequence_generator.py:318-324); on the device engine it is one more decoder of the step
(decode_engine.py).  Adaptive input / softmax, character embeddings and learned positions are refused by name."""
from .fairseq_model import BaseFairseqModel
from .registry import register_model, register_model_architecture
from .s2t_transformer import TransformerDecoder, build_embedding

DEFAULT_MAX_TARGET_POSITIONS = 1024

# what the reference's LM can be built with and this mirror cannot: (args attribute, the flag to name)
_REFUSED = (("character_embeddings", "--character-embeddings"), ("adaptive_input", "--adaptive-input"),
            ("adaptive_softmax_cutoff", "--adaptive-softmax-cutoff"), ("tie_adaptive_weights", "--tie-adaptive-weights"),
            ("decoder_learned_pos", "--decoder-learned-pos"), ("layernorm_embedding", "--layernorm-embedding"),
            ("decoder_layers_to_keep", "--decoder-layers-to-keep"))


@register_model("transformer_lm")
class TransformerLanguageModel(BaseFairseqModel):
    """transformer_lm.py:165-246 / fairseq_model.py FairseqLanguageModel (:456-513)."""

    def __init__(self, decoder):
        super().__init__()
        self.decoder = decoder

    @staticmethod
    def add_args(parser):
        parser.add_argument("--activation-fn", type=str)
        parser.add_argument("--dropout", type=float)
        parser.add_argument("--attention-dropout", type=float)
        parser.add_argument("--activation-dropout", type=float)
        parser.add_argument("--decoder-embed-dim", type=int)
        parser.add_argument("--decoder-ffn-embed-dim", type=int)
        parser.add_argument("--decoder-layers", type=int)
        parser.add_argument("--decoder-attention-heads", type=int)
        parser.add_argument("--no-decoder-final-norm", action="store_true")
        parser.add_argument("--no-token-positional-embeddings", action="store_true")
        parser.add_argument("--share-decoder-input-output-embed", action="store_true")
        parser.add_argument("--no-scale-embedding", action="store_true")
        # (--tokens-per-sample and --max-target-positions are the language_modeling task's flags, as in the reference, where the
        # model reads them from the task's configuration; build_model below takes the position limit from them)

    @classmethod
    def build_model(cls, args, task):
        base_lm_architecture(args)
        for attr, flag in _REFUSED:
            if getattr(args, attr, None):
                raise NotImplementedError("transformer_lm: %s is not supported by this build (the language model must use a plain "
                                          "embedding table, sinusoidal positions and a full softmax)" % flag)
        if args.decoder_input_dim != args.decoder_embed_dim or args.decoder_output_dim != args.decoder_embed_dim:
            raise NotImplementedError("transformer_lm: --decoder-input-dim / --decoder-output-dim other than --decoder-embed-dim are not "
                                      "supported by this build")
        if getattr(args, "max_target_positions", None) is None:
            args.max_target_positions = getattr(args, "tokens_per_sample", DEFAULT_MAX_TARGET_POSITIONS)
        embed_tokens = build_embedding(task.target_dictionary, args.decoder_input_dim)  # (an LM's source dictionary IS its target's)
        return cls(TransformerDecoder(args, task.target_dictionary, embed_tokens, no_encoder_attn=True))

    def forward(self, src_tokens, **kwargs):
        """fairseq_model.py:470-488: (logits [B, T, V], extra) of the next-token distributions after each prefix of src_tokens."""
        return self.decoder(src_tokens, **kwargs)

    def get_normalized_probs(self, net_output, log_probs, sample=None):
        return self.decoder.get_normalized_probs(net_output, log_probs, sample)

    def extract_features(self, src_tokens, **kwargs):
        return self.decoder.extract_features(src_tokens, **kwargs)

    def output_layer(self, features, **kwargs):
        return self.decoder.output_layer(features, **kwargs)

    def max_positions(self):
        return self.decoder.max_positions()

    def max_decoder_positions(self):
        return self.decoder.max_positions()

    @property
    def supported_targets(self):
        return {"future"}


# the reference's defaults (transformer_lm.py:250-306), in its order; output / input width default to the embedding width
_BASE_DEFAULTS = dict(
    dropout=0.1, attention_dropout=0.0, decoder_embed_dim=512, decoder_ffn_embed_dim=2048, decoder_layers=6, decoder_attention_heads=8,
    adaptive_softmax_cutoff=None, adaptive_softmax_dropout=0, adaptive_softmax_factor=4, decoder_learned_pos=False, activation_fn="relu",
    decoder_layerdrop=0, decoder_layers_to_keep=None, add_bos_token=False, no_token_positional_embeddings=False,
    share_decoder_input_output_embed=False, character_embeddings=False, no_decoder_final_norm=False, adaptive_input=False,
    adaptive_input_factor=4, adaptive_input_cutoff=None, tie_adaptive_weights=False, tie_adaptive_proj=False, no_scale_embedding=False,
    layernorm_embedding=False)


def _fill(args, **defaults):
    for k, v in defaults.items():
        if not hasattr(args, k):
            setattr(args, k, v)


def base_lm_architecture(args):
    if hasattr(args, "no_tie_adaptive_proj"):  # the mark of an old checkpoint: those never had a final norm
        args.no_decoder_final_norm = True
        if args.no_tie_adaptive_proj is False:
            args.tie_adaptive_proj = True
    if hasattr(args, "decoder_final_norm"):
        args.no_decoder_final_norm = not args.decoder_final_norm
    _fill(args, **_BASE_DEFAULTS)
    _fill(args, decoder_output_dim=args.decoder_embed_dim, decoder_input_dim=args.decoder_embed_dim)
    args.decoder_normalize_before = True  # always pre-norm, whatever the checkpoint says


register_model_architecture("transformer_lm", "transformer_lm")(base_lm_architecture)


@register_model_architecture("transformer_lm", "transformer_lm_big")
def transformer_lm_big(args):
    _fill(args, decoder_layers=12, decoder_embed_dim=1024, decoder_ffn_embed_dim=4096, decoder_attention_heads=16)
    base_lm_architecture(args)


@register_model_architecture("transformer_lm", "transformer_lm_gpt")
def transformer_lm_gpt(args):
    _fill(args, decoder_embed_dim=768, decoder_ffn_embed_dim=3072, decoder_layers=12, decoder_attention_heads=12, dropout=0.1,
          attention_dropout=0.1, activation_fn="gelu")
    base_lm_architecture(args)


@register_model_architecture("transformer_lm", "transformer_lm_gpt2_small")
def transformer_lm_gpt2_small(args):
    _fill(args, decoder_embed_dim=1024, decoder_ffn_embed_dim=4096, decoder_layers=24, decoder_attention_heads=16, dropout=0.1,
          attention_dropout=0.1, activation_fn="gelu")
    base_lm_architecture(args)
