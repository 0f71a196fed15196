"""BLEU for --eval-bleu (fairseq/tasks/translation.py:364-417, 433-469): the per-batch statistics that are SUMMED over batches and
ranks, and the score from the summed statistics.

The reference computes both with sacrebleu (corpus_bleu / compute_bleu).  sacrebleu is not a dependency of this build: the statistics
are counted on whitespace tokens — what the reference does under --eval-tokenized-bleu (tokenize="none") — and the score is written
out from the published definition below.  It has NOT been compared with sacrebleu."""
import math
from collections import Counter

ORDER = 4  # translation.py:28 EVAL_BLEU_ORDER


def sentence_stats(hyp, ref):
    """(counts[4], totals[4], sys_len, ref_len) of one hypothesis / reference pair of whitespace-tokenised strings: counts[n-1] the
    hypothesis n-grams also in the reference, clipped to the reference's multiplicity; totals[n-1] the hypothesis n-grams."""
    h, r = hyp.split(), ref.split()
    counts, totals = [0] * ORDER, [0] * ORDER
    for n in range(1, ORDER + 1):
        hc = Counter(tuple(h[i:i + n]) for i in range(len(h) - n + 1))
        rc = Counter(tuple(r[i:i + n]) for i in range(len(r) - n + 1))
        counts[n - 1] = sum(min(c, rc[g]) for g, c in hc.items())
        totals[n - 1] = max(len(h) - n + 1, 0)
    return counts, totals, len(h), len(r)


def corpus_stats(hyps, refs):
    """The statistics of a batch as the logging keys of TranslationTask.valid_step (:367-375)."""
    out = {"_bleu_sys_len": 0, "_bleu_ref_len": 0}
    for i in range(ORDER):
        out["_bleu_counts_%d" % i] = 0
        out["_bleu_totals_%d" % i] = 0
    for h, r in zip(hyps, refs):
        c, t, sl, rl = sentence_stats(h, r)
        out["_bleu_sys_len"] += sl
        out["_bleu_ref_len"] += rl
        for i in range(ORDER):
            out["_bleu_counts_%d" % i] += c[i]
            out["_bleu_totals_%d" % i] += t[i]
    return out


def bleu_from_stats(counts, totals, sys_len, ref_len):
    """BLEU in [0, 100] from summed statistics: brevity penalty min(1, exp(1 - ref_len / sys_len)) times the geometric mean of the four
    n-gram precisions; `exp` smoothing: the k-th order (k = 1, 2, ...) whose count is zero takes the numerator 1 / 2^k.  0 when any
    total is 0 (a system output shorter than four tokens in all, the empty output included)."""
    if sys_len <= 0 or any(t <= 0 for t in totals):
        return 0.0
    log_p, k = 0.0, 0
    for c, t in zip(counts, totals):
        if c <= 0:
            k += 1
            c = 1.0 / 2 ** k
        log_p += math.log(c / t)
    bp = min(1.0, math.exp(1.0 - ref_len / sys_len))
    return 100.0 * bp * math.exp(log_p / ORDER)


def derived_bleu(summed):
    """{"bleu": score} from a dict of summed logging values (the keys of corpus_stats), or {} when no BLEU statistics are in it.
    Rounded to two decimals as the reference logs it (translation.py:415)."""
    if "_bleu_sys_len" not in summed:
        return {}
    counts = [summed.get("_bleu_counts_%d" % i, 0) for i in range(ORDER)]
    totals = [summed.get("_bleu_totals_%d" % i, 0) for i in range(ORDER)]
    return {"bleu": round(bleu_from_stats(counts, totals, summed["_bleu_sys_len"], summed["_bleu_ref_len"]), 2)}


# ---- detokenisers of --eval-bleu-detok (fairseq/data/encoders) -----------------------------------------------------------------
_noted = set()


def note_once(logger, key, msg):
    if key not in _noted:
        _noted.add(key)
        logger.warning(msg)


class SpaceTokenizer:
    """encoders/space_tokenizer.py: decode is the identity."""

    def decode(self, x):
        return x


class MosesDetokenizer:
    """encoders/moses_tokenizer.py decode: sacremoses' detokeniser over the whitespace tokens."""

    def __init__(self, target_lang="en", **unused):
        from sacremoses import MosesDetokenizer as M
        self.detok = M(target_lang)

    def decode(self, x):
        return self.detok.detokenize(x.split())


def build_detokenizer(name, logger, **kw):
    if name in (None, "space"):
        return SpaceTokenizer()
    if name == "moses":
        try:
            return MosesDetokenizer(**kw)
        except ImportError:
            note_once(logger, "moses", "--eval-bleu-detok moses: sacremoses is not installed; falling back to `space` (no detokenisation)")
            return SpaceTokenizer()
    raise NotImplementedError("--eval-bleu-detok %s is not built (space, moses)" % name)
