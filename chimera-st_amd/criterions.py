"""Mirror of fairseq/criterions/label_smoothed_cross_entropy.py (:33-160) and
fairseq/criterions/triplet_st_mt_contrastive.py (:18-212).  The log-softmax + NLL + smoothing runs in the fused
cst_ls_ce kernels (logits read once each way; no fp32 [B*U,V] log-prob tensor)."""
import math
from copy import deepcopy

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import functional as CF
from .dictionary import post_process  # noqa: F401  (data/data_utils.py:340-351; the ctc criterion's WER and its tests use it from here)
from .distributed import notify_unused_parameters
from .registry import register_criterion


class FairseqCriterion(nn.Module):
    def __init__(self, task):
        super().__init__()
        self.task = task
        self.padding_idx = task.target_dictionary.pad() if hasattr(task, "target_dictionary") and task.target_dictionary else -100

    @staticmethod
    def add_args(parser):
        pass

    @classmethod
    def build_criterion(cls, args, task):
        raise NotImplementedError

    @staticmethod
    def logging_outputs_can_be_summed() -> bool:
        return False


@register_criterion("label_smoothed_cross_entropy")
class LabelSmoothedCrossEntropyCriterion(FairseqCriterion):
    single_pass = True  # one forward pass per sample: every parameter receives one gradient per backward pass (trainer.py)

    def __init__(self, task, sentence_avg, label_smoothing, ignore_prefix_size=0, report_accuracy=False):
        super().__init__(task)
        self.sentence_avg = sentence_avg
        self.eps = label_smoothing
        self.ignore_prefix_size = ignore_prefix_size
        self.report_accuracy = report_accuracy
        assert ignore_prefix_size == 0

    @staticmethod
    def add_args(parser):
        parser.add_argument("--label-smoothing", default=0.0, type=float, metavar="D")
        parser.add_argument("--report-accuracy", action="store_true")
        parser.add_argument("--ignore-prefix-size", default=0, type=int)

    @classmethod
    def build_criterion(cls, args, task):
        return cls(task, getattr(args, "sentence_avg", False), args.label_smoothing,
                   getattr(args, "ignore_prefix_size", 0), getattr(args, "report_accuracy", False))

    def forward(self, model, sample, reduce=True):
        """:56-86.  Note Q6: net_input carries the collater's `mask`; the models here swallow it."""
        src = sample["net_input"].get("src_tokens")
        if torch.is_tensor(src) and not src.dtype.is_floating_point and model.training and torch.is_grad_enabled():
            # a text-only update (the MT pre-training recipe, chimera/scripts/train-en2any-MT.sh:38-60, runs this criterion over
            # token ids on the Chimera arch): the audio front end takes no part, its ~96 M parameters never fire a gradient hook and
            # are all-reduced as zeros (legacy_distributed_data_parallel.py:155-156).  Reported here — where it is known that NO
            # pass of this micro-batch is an audio pass — their buckets leave during backward instead of at finish().
            enc = getattr(model, "encoder", None)
            unused = [p for name in ("wav2vec_model", "subsample") if getattr(enc, name, None) is not None
                      for p in getattr(enc, name).parameters()]
            if unused:
                notify_unused_parameters(unused)
        net_output = model(**sample["net_input"])
        loss, nll_loss = self.compute_loss(model, net_output, sample, reduce=reduce)
        sample_size = sample["target"].size(0) if self.sentence_avg else sample["ntokens"]
        logging_output = {"loss": loss.data, "nll_loss": nll_loss.data, "ntokens": sample["ntokens"],
                          "nsentences": sample["target"].size(0), "sample_size": sample_size}
        return loss, sample_size, logging_output

    def compute_loss(self, model, net_output, sample, reduce=True):
        assert reduce, "reduce=False (kd_ratio path) is not on the chimera/scripts path"
        logits = net_output[0]
        target = model.get_targets(sample, net_output)
        return CF.label_smoothed_nll_loss(logits, target, self.eps, self.padding_idx)

    @staticmethod
    def logging_outputs_can_be_summed() -> bool:
        return True

    @staticmethod
    def logging_keys():
        """The keys of logging_output, known without running a batch: a rank that runs out of memory in its FIRST update still has to
        build the all-reduced statistics vector in the other ranks' layout (trainer.py:564-570)."""
        return ("loss", "nll_loss", "ntokens", "nsentences", "sample_size")


@register_criterion("triplet_st_mt_contrastive")
class TripletSTMTContrastiveCriterion(LabelSmoothedCrossEntropyCriterion):
    single_pass = False  # an audio pass and a text pass per sample: the shared layers receive two gradients per backward pass

    def __init__(self, task, sentence_avg, label_smoothing, loss_ratio, contrastive_temp=0.1, ignore_prefix_size=0,
                 report_accuracy=False, contrastive_increase_until=None, kd_ratio=None):
        super().__init__(task, sentence_avg, label_smoothing, ignore_prefix_size, report_accuracy)
        self.loss_ratio = list(loss_ratio)
        self.contrastive_temp = contrastive_temp
        self.contrastive_increase_until = contrastive_increase_until
        self.kd_ratio = kd_ratio if kd_ratio is not None else [None, None]
        self.num_updates = 0
        assert list(self.kd_ratio) == [None, None], "kd_ratio is not used by chimera/scripts"

    @staticmethod
    def add_args(parser):
        """:47-66."""
        parser.add_argument("--label-smoothing", default=0.0, type=float, metavar="D")
        parser.add_argument("--report-accuracy", action="store_true")
        parser.add_argument("--ignore-prefix-size", default=0, type=int)
        parser.add_argument("--loss-ratio", default=[1, 1, 1], type=float, nargs=3)
        parser.add_argument("--contrastive-temp", default=0.1, type=float)
        parser.add_argument("--contrastive-increase-until", type=int, default=None)
        parser.add_argument("--kd-ratio", default=[None, None], type=float, nargs=2)

    @classmethod
    def build_criterion(cls, args, task):
        return cls(task, getattr(args, "sentence_avg", False), args.label_smoothing, args.loss_ratio,
                   args.contrastive_temp, getattr(args, "ignore_prefix_size", 0), getattr(args, "report_accuracy", False),
                   args.contrastive_increase_until, list(args.kd_ratio))

    def set_num_updates(self, n):
        """The reference reads metrics.get_smoothed_values("train")["num_updates"] (:43-45); the trainer pushes it here."""
        self.num_updates = n

    @staticmethod
    def one_decoder_pass(model):
        """Can the audio pass and the text pass share ONE decoder call?  Both feed the decoder the same prev_output_tokens and an
        M-slot memory of the same shape (w2v2_transformer_interlingua.py:137-146, :301-304: no padding in the memory), and every
        decoder row depends on its own batch element only — so decoder(cat(prev, prev), cat(memory_audio, memory_text)) yields the
        two passes' logits as its two batch halves: half the decoder launches at twice the rows, and every decoder parameter
        receives one gradient per backward pass instead of two."""
        import os
        return (not os.environ.get("CST_NO_PAIR_DECODER") and hasattr(model, "encoder") and hasattr(model, "decoder")
                and hasattr(model, "forward_with_internal") and not getattr(getattr(model, "encoder", None), "no_interlingua", True))

    @staticmethod
    def twice_used(model):
        """The parameters BOTH passes of an update run through when the decoder is shared (one_decoder_pass): the encoder layers behind
        the modality-specific front ends and the memory module.  They receive two gradients per backward pass (trainer.py marks them:
        their reductions are not deferred); everything else — wav2vec2, subsampler, text embedding, decoder — receives one."""
        if not TripletSTMTContrastiveCriterion.one_decoder_pass(model):
            return None
        import os
        if not hasattr(model.encoder, "forward_pair") or os.environ.get("CST_NO_PAIR_ENCODER") or os.environ.get("CST_NO_PACK"):
            return [p for n, p in model.encoder.named_parameters() if not n.startswith(("wav2vec_model.", "subsample.", "text_embed_tokens."))]
        if os.environ.get("CST_NO_PAIR_MEMORY"):  # forward_pair walks the shared encoder layers once, the memory layers per modality
            return [p for n, p in model.encoder.named_parameters() if n.startswith(("interlingua_layers.", "interlingua_embedding."))]
        return []  # ... and, by default, the memory layers once as well: every parameter receives one gradient per backward pass

    def _two_passes_one_decoder(self, model, sample, reduce):
        from .fairseq_model import EncoderOut
        from .modules import to_batch_major, to_time_major_view
        ni = sample["net_input"]
        import os
        if hasattr(model.encoder, "forward_pair") and not os.environ.get("CST_NO_PAIR_ENCODER") and not os.environ.get("CST_NO_PACK"):
            # ... and ONE walk through the shared encoder layers (S2T_W2V2_TransformerInterlinguaEncoder.forward_pair)
            enc_a, enc_t, enc_both = model.encoder.forward_pair(ni["src_tokens"], ni["src_lengths"], sample["src_text"], sample["src_text_lengths"])
        else:
            enc_a = model.encoder(src_tokens=ni["src_tokens"], src_lengths=ni["src_lengths"])
            enc_t = model.encoder(src_tokens=sample["src_text"], src_lengths=sample["src_text_lengths"])
            enc_both = None
        if enc_both is None:
            mem = to_time_major_view(torch.cat((to_batch_major(enc_a.encoder_out), to_batch_major(enc_t.encoder_out)), 0))  # [M, 2B, C]
            pm = torch.cat((enc_a.encoder_padding_mask, enc_t.encoder_padding_mask), 0)
            enc_both = EncoderOut(encoder_out=mem, encoder_padding_mask=pm, encoder_embedding=None, encoder_states=None, src_tokens=None,
                                  src_lengths=None)
        prev = ni["prev_output_tokens"]
        logits, extra = model.decoder(prev_output_tokens=torch.cat((prev, prev), 0), encoder_out=enc_both)
        B = prev.size(0)
        st_loss, st_nll_loss = self.compute_loss(model, (logits[:B], extra), sample, reduce=reduce)
        mt_loss, mt_nll_loss = self.compute_loss(model, (logits[B:], extra), sample, reduce=reduce)
        return st_loss, st_nll_loss, mt_loss, mt_nll_loss, enc_a.encoder_out, enc_t.encoder_out

    def forward(self, model, sample, reduce=True):
        """:68-146 — audio pass, text pass, contrastive term."""
        if self.loss_ratio[1] != 0 and self.one_decoder_pass(model):
            st_loss, st_nll_loss, mt_loss, mt_nll_loss, audio_internal, text_internal = self._two_passes_one_decoder(model, sample, reduce)
        else:
            st_net_output, audio_internal = model.forward_with_internal(**sample["net_input"])
            st_loss, st_nll_loss = self.compute_loss(model, st_net_output, sample, reduce=reduce)
            if self.loss_ratio[1] != 0:
                mt_input = {"src_tokens": sample["src_text"], "src_lengths": sample["src_text_lengths"],
                            "prev_output_tokens": sample["net_input"]["prev_output_tokens"], "mask": sample["net_input"]["mask"]}
                mt_net_output, text_internal = model.forward_with_internal(**mt_input)
                mt_loss, mt_nll_loss = self.compute_loss(model, mt_net_output, sample, reduce=reduce)
            else:
                mt_loss, mt_nll_loss = 0, 0
        if self.loss_ratio[2] != 0:
            contrastive_loss = self.compute_contrastive(audio_internal, text_internal, reduce)
        else:
            contrastive_loss = 0
        loss_ratio = deepcopy(self.loss_ratio)
        if self.contrastive_increase_until is not None:
            loss_ratio[2] *= min(1, (self.num_updates or 0) / self.contrastive_increase_until)
        loss = sum(loss_ratio[i] * l for i, l in enumerate((st_loss, mt_loss, contrastive_loss)))
        nll_loss = sum(loss_ratio[i] * l for i, l in enumerate((st_nll_loss, mt_nll_loss)))
        sample_size = sample["target"].size(0) if self.sentence_avg else sample["ntokens"]
        logging_output = {
            "loss": loss.data, "nll_loss": nll_loss.data, "st_loss": st_loss.data, "st_nll_loss": st_nll_loss.data,
            "mt_loss": mt_loss.data if self.loss_ratio[1] != 0 else 0,
            "mt_nll_loss": mt_nll_loss.data if self.loss_ratio[1] != 0 else 0,
            "contrastive_loss": contrastive_loss.data if self.loss_ratio[2] != 0 else 0,
            "ntokens": sample["ntokens"], "nsentences": sample["target"].size(0), "sample_size": sample_size,
        }
        return loss, sample_size, logging_output

    def compute_contrastive(self, input1, input2, reduce):
        """:154-169 — per-utterance M x M cosine-similarity CE (class dim = audio slot): cst_contrastive_fwd/bwd."""
        assert input1.shape == input2.shape
        if not reduce:
            raise NotImplementedError("compute_contrastive(reduce=False) is not on the training path")
        from . import functional as CF
        return CF.contrastive_loss(input1.transpose(0, 1), input2.transpose(0, 1), self.contrastive_temp)

    @staticmethod
    def logging_outputs_can_be_summed() -> bool:
        return True

    @staticmethod
    def logging_keys():
        return ("loss", "nll_loss", "st_loss", "st_nll_loss", "mt_loss", "mt_nll_loss", "contrastive_loss", "ntokens", "nsentences",
                "sample_size")


@register_criterion("ctc")
class CtcCriterion(FairseqCriterion):
    """fairseq/criterions/ctc.py:18-253.  The loss runs on the model's RAW logits in the fused cst_ctc kernels (no fp32 [T, B, V]
    log-probability tensor, csrc/ctc.hip); validation decodes the best path on the device (cst_ctc_greedy) and brings B*T + B int32
    values to the host instead of the log-probabilities; the edit distances are cst_edit_distance (the reference imports
    `editdistance`).  A training step adds no host synchronisation: the input lengths are computed from the padding mask on the device
    and handed to the kernel as a device tensor."""
    single_pass = True

    def __init__(self, task, sentence_avg=False, zero_infinity=False, post_process="letter", wer_args=None):
        super().__init__(task)
        d = task.target_dictionary
        self.blank_idx, self.pad_idx, self.eos_idx = d.bos(), d.pad(), d.eos()
        self.post_process = post_process if post_process else "letter"
        if wer_args is not None:
            raise NotImplementedError("--wer-args (KenLM / lexicon decoding of the validation set, examples/speech_recognition/"
                                      "w2l_decoder.py) is not built: validation reports the best-path uer / wer / raw_wer only")
        self.zero_infinity = bool(zero_infinity)
        self.sentence_avg = bool(sentence_avg)

    @staticmethod
    def add_args(parser):
        """:52-73."""
        parser.add_argument("--zero-infinity", action="store_true", help="zero inf loss")
        parser.add_argument("--post-process", "--remove-bpe", default="letter")
        parser.add_argument("--wer-args", type=str, default=None)

    @classmethod
    def build_criterion(cls, args, task):
        return cls(task, getattr(args, "sentence_avg", False), getattr(args, "zero_infinity", False),
                   getattr(args, "post_process", "letter"), getattr(args, "wer_args", None))

    def _targets(self, sample):
        """The sample's target with pad and eos removed, left-packed [B, Lmax] (the reference's masked_select keeps the same order),
        on the device without a synchronisation."""
        t = sample["target"]
        keep = (t != self.pad_idx) & (t != self.eos_idx)
        Lmax = t.size(1)
        dst = torch.where(keep, keep.cumsum(1) - 1, torch.full_like(t, Lmax))
        packed = t.new_zeros(t.size(0), Lmax + 1).scatter_(1, dst, t)
        return packed[:, :Lmax].contiguous(), sample["target_lengths"].to(torch.int64)

    def forward(self, model, sample, reduce=True):
        """:75-183."""
        net_output = model(**sample["net_input"])
        logits = net_output["encoder_out"]  # [T, B, V] raw (model.get_logits): the log-softmax is fused into the loss
        T, B = logits.shape[0], logits.shape[1]
        if "src_lengths" in sample["net_input"]:
            input_lengths = sample["net_input"]["src_lengths"].to(torch.int64)
        elif net_output.get("padding_mask") is not None:
            input_lengths = (~net_output["padding_mask"]).long().sum(-1)
        else:
            input_lengths = torch.full((B,), T, dtype=torch.int64, device=logits.device)
        targets, target_lengths = self._targets(sample)
        loss, _ = CF.ctc_loss(logits, targets, target_lengths, input_lengths, self.blank_idx, self.zero_infinity)
        ntokens = sample["ntokens"] if "ntokens" in sample else int(target_lengths.sum())
        sample_size = sample["target"].size(0) if self.sentence_avg else ntokens
        logging_output = {"loss": loss.data, "ntokens": ntokens, "nsentences": sample["id"].numel() if "id" in sample else B,
                          "sample_size": sample_size}
        if not model.training:
            logging_output.update(self.error_counts(logits, input_lengths, sample))
        return loss, sample_size, logging_output

    @torch.no_grad()
    def error_counts(self, logits, input_lengths, sample):
        """:116-181 without a decoder: unit and word errors of the best path."""
        from . import kernels as K
        d = self.task.target_dictionary
        T, B = logits.shape[0], logits.shape[1]
        host = CF.ctc_greedy(logits, input_lengths, self.blank_idx)[2].cpu()
        ids, counts = host[:B * T].view(B, T), host[B * T:]
        tgt = (sample["target_label"] if "target_label" in sample else sample["target"]).cpu()
        c_err = c_len = w_errs = w_len = 0
        for b in range(B):
            t = tgt[b]
            targ_units_arr = t[(t != self.pad_idx) & (t != self.eos_idx)].tolist()
            pred_units_arr = ids[b, :int(counts[b])].tolist()
            c_err += K.edit_distance(pred_units_arr, targ_units_arr)
            c_len += len(targ_units_arr)
            targ_words = post_process(d.string(targ_units_arr), self.post_process).split()
            pred_words = post_process(d.string(pred_units_arr), self.post_process).split()
            word_ids = {}
            enc = lambda ws: [word_ids.setdefault(w, len(word_ids)) for w in ws]
            w_errs += K.edit_distance(enc(pred_words), enc(targ_words))
            w_len += len(targ_words)
        return {"wv_errors": w_errs, "w_errors": w_errs, "w_total": w_len, "c_errors": c_err, "c_total": c_len}

    @staticmethod
    def derived_metrics(out):
        """reduce_metrics :208-244: uer / wer / raw_wer in per cent from the summed counts (only where the counts exist)."""
        d = {}
        if out.get("c_total", 0) > 0:
            d["uer"] = round(out["c_errors"] * 100.0 / out["c_total"], 3)
        if out.get("w_total", 0) > 0:
            d["wer"] = round(out["w_errors"] * 100.0 / out["w_total"], 3)
            d["raw_wer"] = round(out["wv_errors"] * 100.0 / out["w_total"], 3)
        return d

    @staticmethod
    def logging_outputs_can_be_summed() -> bool:
        return True

    @staticmethod
    def logging_keys():
        return ("loss", "ntokens", "nsentences", "sample_size")


@register_criterion("wav2vec")
class Wav2vecCriterion(FairseqCriterion):
    """fairseq/criterions/wav2vec_criterion.py, the InfoNCE form.  The contrastive loss is functional.infonce_loss on the model's
    x / y / negative indices (csrc/w2v_pretrain.hip): no [K + 1, B M, D] targets and no logits tensor; `correct` / `count` come out of
    the same kernel as two device integers.  Every logged quantity stays on the device — the trainer's one small read brings them to
    the host together; there is no .item() here."""
    single_pass = True

    def __init__(self, task, infonce=False, loss_weights=None, log_keys=None):
        super().__init__(task)
        if not infonce:
            raise NotImplementedError("criterion wav2vec without --infonce (the binary cross entropy form) is not built")
        self.infonce = True
        self.loss_weights = None if loss_weights is None else [float(w) for w in (eval(loss_weights) if isinstance(loss_weights, str) else loss_weights)]
        self.log_keys = [] if log_keys is None else list(eval(log_keys) if isinstance(log_keys, str) else log_keys)

    @staticmethod
    def add_args(parser):
        parser.add_argument("--infonce", action="store_true", help="cross entropy over the positive and the negatives (InfoNCE)")
        parser.add_argument("--loss-weights", type=str, default=None, help="weights for additional loss terms (not first one)")
        parser.add_argument("--log-keys", type=str, default=None, help="output keys to log")

    @classmethod
    def build_criterion(cls, args, task):
        return cls(task, getattr(args, "infonce", False), getattr(args, "loss_weights", None), getattr(args, "log_keys", None))

    def forward(self, model, sample, reduce=True):
        net_output = model(**sample["net_input"])
        x, y = net_output["x"], net_output["y"]
        D = x.shape[-1]
        loss, _, counters = CF.infonce_loss(x.reshape(-1, D), y.reshape(-1, D), net_output["neg_idx"], model.logit_temp)
        sample_size = x.shape[0] * x.shape[1]  # the masked positions: a host number (the masks are drawn on the host)
        losses = [loss.detach().clone()]
        if self.loss_weights is not None:
            extra = model.get_extra_losses(net_output)
            weights = self.loss_weights
            if len(weights) == 1 and len(extra) != 1:
                weights = [weights[0]] * len(extra)
            assert len(extra) == len(weights), "%d extra losses, %d --loss-weights" % (len(extra), len(weights))
            for p, coef in zip(extra, weights):
                if coef != 0 and p is not None:
                    p = coef * p.float() * sample_size
                    loss = loss + p
                    losses.append(p.detach())
        logging_output = {"loss": loss.detach(), "ntokens": sample_size, "nsentences": sample["id"].numel() if "id" in sample else x.shape[0],
                          "sample_size": sample_size, "correct": counters[0], "count": counters[1]}
        for lk in self.log_keys:
            if lk in net_output:
                logging_output[lk] = net_output[lk].detach() if torch.is_tensor(net_output[lk]) else float(net_output[lk])
        if len(losses) > 1:
            for i, l in enumerate(losses):
                logging_output["loss_%d" % i] = l
        return loss, sample_size, logging_output

    def logging_keys(self):
        keys = ["loss", "ntokens", "nsentences", "sample_size", "correct", "count"] + list(self.log_keys)
        if self.loss_weights is not None:
            keys += ["loss_%d" % i for i in range(1 + len(self.loss_weights))]
        return tuple(keys)

    @staticmethod
    def reduce_metrics(logging_outputs):
        """wav2vec_criterion.py:125-175 as a dictionary: loss (and loss_i) per sample in bits, accuracy = correct / count, the other
        keys averaged over the logging outputs."""
        import math
        tot = lambda k: float(sum(float(log.get(k, 0)) for log in logging_outputs))
        sample_size = tot("sample_size")
        out = {"loss": tot("loss") / sample_size / math.log(2), "ntokens": tot("ntokens"), "nsentences": tot("nsentences"),
               "sample_size": sample_size, "_correct": tot("correct"), "_total": tot("count")}
        if out["_total"] > 0:
            out["accuracy"] = round(out["_correct"] / out["_total"], 5)
        for k in logging_outputs[0]:
            if k not in ("loss", "ntokens", "nsentences", "sample_size", "correct", "count"):
                val = tot(k) / len(logging_outputs)
                out[k] = val / sample_size / math.log(2) if k.startswith("loss") else round(val, 3)
        return out

    @staticmethod
    def derived_metrics(out):
        """What the training log derives from one update's summed scalars: the accuracy and the loss terms per sample in bits."""
        import math
        d = {}
        if out.get("count", 0) > 0:
            d["accuracy"] = round(out["correct"] / out["count"], 5)
        ss = max(out.get("sample_size", 1.0), 1.0)
        for k, v in out.items():
            if k.startswith("loss_"):
                d[k] = v / ss / math.log(2)
        return d

    @staticmethod
    def logging_outputs_can_be_summed() -> bool:
        return False


@register_criterion("cross_entropy")
class CrossEntropyCriterion(FairseqCriterion):
    """criterions/cross_entropy.py:21-89 — the language_modeling task's loss: the summed negative log-likelihood of the non-pad
    targets.  The log-softmax and the gather run in the fused cst_ls_ce kernels at smoothing 0 (no fp32 [B*T, V] log-prob tensor)."""
    single_pass = True  # one forward pass per sample (trainer.py)
    derives_from_train_log = True  # derived_metrics reads only keys of the training log: the epoch's train line carries `ppl` too

    def __init__(self, task, sentence_avg):
        super().__init__(task)
        self.sentence_avg = sentence_avg

    @classmethod
    def build_criterion(cls, args, task):
        return cls(task, getattr(args, "sentence_avg", False))

    def forward(self, model, sample, reduce=True):
        """:27-46."""
        net_output = model(**sample["net_input"])
        loss, _ = self.compute_loss(model, net_output, sample, reduce=reduce)
        sample_size = sample["target"].size(0) if self.sentence_avg else sample["ntokens"]
        logging_output = {"loss": loss.data, "ntokens": sample["ntokens"], "nsentences": sample["target"].size(0), "sample_size": sample_size}
        return loss, sample_size, logging_output

    def compute_loss(self, model, net_output, sample, reduce=True):
        assert reduce, "reduce=False is not built"
        loss, _ = CF.label_smoothed_nll_loss(net_output[0], model.get_targets(sample, net_output), 0.0, self.padding_idx)
        return loss, loss

    @staticmethod
    def derived_metrics(summed):
        """:60-80: ppl = 2^(the base-2 loss per token) — of nll_loss = loss / ntokens under --sentence-avg, else of loss."""
        ntokens, ss = summed.get("ntokens", 0.0), summed.get("sample_size", 0.0)
        if "loss" not in summed or ntokens <= 0:
            return {}
        out = {}
        if ss != ntokens:
            out["nll_loss"] = summed["loss"] / ntokens / math.log(2)
        try:
            out["ppl"] = round(2 ** (summed["loss"] / ntokens / math.log(2)), 2)
        except OverflowError:
            out["ppl"] = float("inf")
        return out

    @staticmethod
    def logging_outputs_can_be_summed() -> bool:
        return True

    @staticmethod
    def logging_keys():
        return ("loss", "ntokens", "nsentences", "sample_size")
