"""Scoring of given translations — mirror of fairseq/sequence_scorer.py (SequenceScorer.generate :34-153), which
`fairseq-generate --score-reference` selects in place of a search (tasks/fairseq_task.py:313-320): how probable does a model, or a
checkpoint ensemble, find THIS target?  The teacher-forced forward is the training forward in eval mode; what is new is the step from
the members' [B, T, V] logits to per-token scores, which cst_score_tokens (include/cst.h, ABI 13) does in one pass without the
float32 [B, T, V] probability tensor the reference builds per member.

An ensemble averages the members' probabilities of the target token: score = logsumexp_m(log p_m) - log N.  The reference adds the
probabilities and takes the log (:96-111) — the same number wherever that is finite; the log-domain form does not turn into -inf when
every member's probability underflows fp32.

A language model is scored the same way (fairseq_eval_lm.py: its net_input is src_tokens / src_lengths, its logits the next-token
distributions).  Not built: `softmax_batch` (chunked softmax — nothing of size [B, T, V] is materialised in fp32 here, so there is
nothing to chunk) and `sample["start_indices"]` (--context-window).  The speech decoders return no attention (TransformerDecoderScriptable.extract_features returns x, None), so
`attention` and `alignment` are None, as they are from SequenceGenerator."""
import math

import torch


def score_tokens_torch(logits_list, target, pad):
    """The readable restatement of cst_score_tokens in plain torch (works on CPU tensors): per member the float log-softmax and the
    gather of the target column, over the members logsumexp - log N, 0 at pad positions; per sentence the number of non-pad targets
    and the mean of their scores (no targets: 0 / 0 = NaN).  -> (pos fp32 [B, T], score fp32 [B], len int32 [B])."""
    live = target.ne(pad)
    index = target.clamp(0, logits_list[0].size(-1) - 1).unsqueeze(-1)
    lps = [torch.log_softmax(x.float(), dim=-1).gather(2, index).squeeze(-1) for x in logits_list]
    pos = lps[0] if len(lps) == 1 else torch.logsumexp(torch.stack(lps, dim=0), dim=0) - math.log(len(lps))
    pos = torch.where(live, pos, torch.zeros_like(pos))
    length = live.sum(dim=1)
    return pos, pos.sum(dim=1) / length.to(pos.dtype), length.to(torch.int32)


class SequenceScorer:
    """tgt_dict: the target dictionary; eos: as in the reference (kept; the tokens of a result are the target without pad, eos
    included).  fused=True: cst_score_tokens and ONE transfer of (positional scores, scores, lengths) to the host per batch — the
    wrapper's range check of the target ids reads two more integers; fused=False: score_tokens_torch on the same logits, the
    cross-check (as the host loop is SequenceGenerator's)."""

    def __init__(self, tgt_dict, eos=None, fused=True):
        self.tgt_dict = tgt_dict
        self.pad = tgt_dict.pad()
        self.eos = tgt_dict.eos() if eos is None else eos
        self.vocab_size = len(tgt_dict)
        self.fused = bool(fused)

    @torch.no_grad()
    def generate(self, models, sample, **kwargs):
        """Score a batch of translations: sample["net_input"] = src_tokens, src_lengths, prev_output_tokens; sample["target"] [B, T].
        Returns per sentence a list with one dict: tokens, score, attention None, alignment None, positional_scores."""
        target = sample.get("target")
        if target is None:
            raise ValueError("SequenceScorer needs sample['target']: there is nothing to score")
        models = list(models) if isinstance(models, (list, tuple)) else [models]
        logits = []
        for i, model in enumerate(models):
            model.eval()
            x = model(**sample["net_input"])[0]
            if x.size(-1) != self.vocab_size:
                raise ValueError("ensemble member %d has a target vocabulary of %d symbols, the dictionary has %d: the members of an "
                                 "ensemble must share the target dictionary" % (i, x.size(-1), self.vocab_size))
            logits.append(x)
        target = target.to(logits[0].device)
        B, T = target.shape
        if self.fused:
            from . import kernels
            packed = kernels.score_tokens(logits, target, self.pad)[3].cpu()
            pos, score, length = packed[:B * T].view(B, T), packed[B * T:B * T + B], packed[B * T + B:].view(torch.int32)
        else:
            pos, score, length = (t.cpu() for t in score_tokens_torch(logits, target, self.pad))
        # targets are right-padded (the collater's layout; the reference's slice of the positional scores, :126, assumes the same):
        # sentence i is its first len[i] columns
        return [[{"tokens": target[i, :n], "score": score[i], "attention": None, "alignment": None, "positional_scores": pos[i, :n]}]
                for i, n in enumerate(length.tolist())]
