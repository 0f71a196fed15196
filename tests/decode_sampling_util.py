"""Shared by tests/test_decode_sampling_cpu.py and tests/test_decode_sampling_gpu.py: an fp64 restatement of ONE sampling step of
cst_beam_step (include/cst.h, ABI 11; search.py Sampling.step :676-742 inside sequence_generator.py's loop) — the masks, the kept set
of top-p / top-k, the counter-based inverse-CDF draw and the bookkeeping over K = beam candidates — on the synthetic per-step logits
of tests/decode_constraints_util.py.

For every draw the restatement also says whether the draw is DECIDABLE: the kernel forms its sums in fp32 in its own fixed order, so
where a decision hangs on less than the rounding of such a sum, two correct evaluations may differ.  With
    DELTA = (longest addition chain stated in the kernel comment of csrc/beam_search.hip + 8) * 2^-24 = (64 + 8) * 2^-24 = 4.3e-6
a draw is decidable when no exclusive prefix mass of the descending order lies within DELTA * (the row's mass) of p (top-p), and
u * Z is not within DELTA * Z of an edge of the kept CDF.  (The 8 covers what is not an addition: the fp32 log-softmax the kernel's
q = exp(x) starts from — x carries about an ulp of a number below 16, 1e-6, which scales q by 1 +- 1e-6 — and expf itself.)
DELTA is derived from the kernel's stated chain, not tuned."""
import math

import numpy as np
import torch

from decode_constraints_util import BEAM, BSZ, EOS, HOT, MAX_LEN, PAD, PREFIX, UNK, banned_tokens  # noqa: F401

CHAIN = 64  # csrc/beam_search.hip, comment of beam_row_sample_tail: "LONGEST ADDITION CHAIN ... 64"
DELTA = (CHAIN + 8) * 2.0 ** -24
_M32 = 0xFFFFFFFF

# (dtype name, vocabulary, members): fp32 vectors hold 4 elements, bf16 vectors 8, 512 threads -> NV = 1 / 3 / 5 vectors per thread;
# 10001 is no multiple of 8 (nor of 4)
CASES = [(dt, V, members) for dt, Vs in (("fp32", (60, 6000, 10001)), ("bf16", (60, 10001, 20001))) for V in Vs for members in (1, 2)]
# name -> (top-k, top-p, temperature, n-gram, prefix, min_len)
VARIANTS = {"plain": (0, 0.0, 1.0, 0, False, 1), "topk1": (1, 0.0, 1.0, 0, False, 1), "topk8": (8, 0.0, 1.0, 0, False, 1),
            "topp0.9": (0, 0.9, 1.0, 0, False, 1), "temp0.7": (0, 0.0, 0.7, 0, False, 1),
            "topp0.9_prefix_ngram2_minlen4": (0, 0.9, 1.0, 2, True, 4)}


TIED = (20, 21, 22)  # three tokens with one and the same logit in the middle of the HOT ladder: cuts fall on ties


def step_logits(dtype_name, V, members, step):
    """Fresh logits [members][BSZ * BEAM, V] of one step, peaked like decode_constraints_util.step_logits (the HOT tokens 14 .. 9, eos
    rising with the step), with two changes for sampling.  The noise sits 6 lower: where the n-gram ban removes the top of the ladder
    a draw would otherwise land in a tail of thousands of tokens whose CDF edges lie closer together than DELTA, and a fifth of such
    draws would be undecidable.  And the TIED tokens share the logit 10 exactly (in fp32 and bf16, in every member), so that the
    top-k cut (and at times the nucleus cut) falls between equal values and the kept set hangs on the token order."""
    g = torch.Generator().manual_seed(100003 * step + 17 * V + members + (7 if dtype_name == "bf16" else 0))
    rows = BSZ * BEAM
    out = []
    for _ in range(members):
        x = torch.randn(rows, V, generator=g) - 6.0
        x[:, list(HOT)] = 14.0 - torch.arange(len(HOT), dtype=torch.float32) + torch.randn(rows, len(HOT), generator=g)
        x[:, EOS] = 8.0 + 0.7 * step + torch.randn(rows, generator=g)
        x[:, list(TIED)] = 10.0
        out.append(x.to(torch.bfloat16 if dtype_name == "bf16" else torch.float32))
    return out


def family(dtype_name, V):
    vec = 8 if dtype_name == "bf16" else 4
    nv = -(-(-(-V // vec)) // 512)
    return "wide" if nv > 5 else "NV%d" % (1 if nv <= 1 else 3 if nv <= 3 else 5)


def uniforms(key, idx):
    """numpy twin of the device's u: (cst_drop_bits32(key, cst_drop_key2(key), idx) >> 8) * 2^-24 (csrc/cst_common.h), float64."""
    u64 = np.uint64
    key = int(key) & _M32
    key2 = (key * 0x2C1B3C6D + 0x297A2D39) & _M32
    idx = np.asarray(idx, dtype=np.uint64) & u64(_M32)
    x = ((idx ^ u64(key)) * u64(0x9E3779B1)) & u64(_M32)
    x = ((x ^ (x >> u64(15))) + u64(key2)) & u64(_M32)
    x = (x * u64(0x85EBCA77)) & u64(_M32)
    x = x ^ (x >> u64(13))
    return (x >> u64(8)).astype(np.float64) * 2.0 ** -24


def kept_set(lp, topk=0, topp=0.0, widen=0.0):
    """lp: float64 [V] masked log-probabilities.  Returns (kept bool [V], order, before): the descending order (value, then token)
    and the exclusive prefix masses along it.  widen: keeps the top-p elements with less than p + widen in front of them."""
    V = lp.shape[0]
    order = np.lexsort((np.arange(V), -lp))  # value descending, token ascending (-inf last, in token order)
    q = np.exp(lp[order])
    before = np.cumsum(q) - q
    kept = np.zeros(V, dtype=bool)
    if topp > 0:
        kept[order[before < topp + widen]] = True
    elif topk > 0:
        kept[order[:topk]] = True
    else:
        kept[:] = True
    return kept, order, before


def new_state():
    bbsz, L1, LT = BSZ * BEAM, MAX_LEN + 1, MAX_LEN + 2
    tokens = torch.full((bbsz, LT), PAD, dtype=torch.long)
    tokens[:, 0] = EOS
    anc = torch.zeros(bbsz, L1, dtype=torch.int32)
    anc[:, 0] = torch.arange(bbsz, dtype=torch.int32)
    return dict(tokens=tokens, scores=torch.zeros(bbsz, L1, dtype=torch.float64), anc=anc,
                ignore=torch.zeros(BSZ, BEAM, dtype=torch.uint8), finished=torch.zeros(BSZ, dtype=torch.uint8),
                nfinal=torch.zeros(BSZ, dtype=torch.int32), fin_tokens=torch.zeros(BSZ, BEAM, L1, dtype=torch.long),
                fin_score=torch.zeros(BSZ, BEAM, dtype=torch.float64), fin_len=torch.zeros(BSZ, BEAM, dtype=torch.int32))


def masked_lprobs(st, logits, s, temperature=1.0, ngram=0, prefix=None, min_len=1, unk_penalty=0.0):
    """float64 [bbsz, V]: log-softmax (ensemble: log of the mean distribution) and the masks in the generator's order.  Where the prefix
    holds eos the sentence's first row is copied over its rows in st (tokens, scores, ancestry), as the reference does."""
    beam = BEAM
    lps = [torch.log_softmax(x.double() / temperature, dim=-1) for x in logits]
    lp = lps[0] if len(lps) == 1 else torch.logsumexp(torch.stack(lps, 0), 0) - math.log(len(lps))
    lp[lp != lp] = -math.inf
    lp[:, PAD] = -math.inf
    lp[:, UNK] -= unk_penalty
    if s >= MAX_LEN:
        lp[:, :EOS] = -math.inf
        lp[:, EOS + 1:] = -math.inf
    if prefix is not None and s < prefix.size(1) and s < MAX_LEN:
        for b in range(BSZ):
            t = int(prefix[b, s])
            rows = slice(b * beam, (b + 1) * beam)
            if t != PAD:
                keep = lp[rows, t].clone()
                lp[rows] = -math.inf
                lp[rows, t] = keep
            if t == EOS:
                lp[rows] = lp[b * beam].clone()
                for name in ("tokens", "scores", "anc"):
                    st[name][rows] = st[name][b * beam].clone()
    elif s < min_len:
        lp[:, EOS] = -math.inf
    if ngram:
        tk_all = st["tokens"].tolist()
        for h in range(lp.size(0)):
            ban = sorted(set(banned_tokens(tk_all[h], s, ngram)))
            if ban:
                lp[h, torch.tensor(ban)] = -math.inf
    return lp


def draw(lp_row, u, topk=0, topp=0.0):
    """One draw from a row: dict(tok, lprob, decidable, kept, wide) — tok PAD / lprob -inf for a row without mass; `wide` = the
    DELTA-widened kept set (what an undecidable draw may still choose from)."""
    lp = lp_row.numpy() if torch.is_tensor(lp_row) else lp_row
    V = lp.shape[0]
    kept, order, before = kept_set(lp, topk, topp)
    mass = float(np.exp(lp).sum())
    wide = kept_set(lp, topk, topp, widen=DELTA * mass)[0] if topp > 0 else kept
    decidable = True
    if topp > 0:  # no exclusive prefix mass (nor the whole mass) within DELTA * mass of p
        edges = np.concatenate([before, [mass]])
        decidable = bool(np.abs(edges - topp).min() > DELTA * mass)
    q = np.where(kept, np.exp(lp), 0.0)
    cdf = np.cumsum(q)
    Z = float(cdf[-1])
    if not Z > 0.0:
        return dict(tok=PAD, lprob=-math.inf, decidable=decidable, kept=kept, wide=wide)
    target = u * Z
    live = q > 0
    decidable = decidable and bool(np.abs(cdf[live] - target).min() > DELTA * Z)
    hit = np.nonzero(live & (cdf > target))[0]
    tok = int(hit[0]) if len(hit) else int(np.nonzero(live)[0][-1])
    return dict(tok=tok, lprob=float(lp[tok]), decidable=decidable, kept=kept, wide=wide & (np.exp(lp) > 0))


def step_draws(st, lp, s, key, topk=0, topp=0.0, prefix=None):
    """The `beam` candidates of every sentence at step s: list over (sentence * beam + slot) of draw() dicts with `row` (the parent)
    and `score` (lprob + the parent's cumulative score) added."""
    beam, L1 = BEAM, MAX_LEN + 1
    out = []
    for b in range(BSZ):
        first = prefix is not None and s < prefix.size(1) and s < MAX_LEN and int(prefix[b, s]) == EOS
        for k in range(beam):
            row = b * beam + (0 if (s == 0 or first) else k)
            u = float(uniforms(key, [(b * beam + k) * L1 + s])[0])
            d = draw(lp[row], u, topk, topp)
            d["row"], d["lp_row"] = row, lp[row]
            d["score"] = d["lprob"] + (float(st["scores"][row, s - 1]) if s > 0 else 0.0)
            out.append(d)
    return out


def adopt(st, d, tok, s):
    """An undecidable draw takes the device's token (the caller has checked that it is in d["wide"])."""
    d["tok"], d["lprob"] = int(tok), float(d["lp_row"][tok])
    d["score"] = d["lprob"] + (float(st["scores"][d["row"], s - 1]) if s > 0 else 0.0)


def bookkeeping(st, cands, s):
    """sequence_generator.py:340-499 over K = beam candidates per sentence (finalisation, cands_to_ignore, the next rows)."""
    beam = BEAM
    tokens, scores, anc = st["tokens"], st["scores"], st["anc"]
    new_tokens, new_scores, new_anc = tokens.clone(), scores.clone(), anc.clone()
    for b in range(BSZ):
        c = cands[b * beam:(b + 1) * beam]
        ign = st["ignore"][b].tolist()
        was_finished, nf = bool(st["finished"][b]), int(st["nfinal"][b])
        em, any_eos = [], False
        for k in range(beam):
            e = c[k]["tok"] == EOS and c[k]["score"] != -math.inf and not ign[k]
            em.append(e)
            if e:
                any_eos = True
                if not was_finished and nf < beam:
                    bi = c[k]["row"]
                    st["fin_tokens"][b, nf, :s] = tokens[bi, 1:s + 1]
                    st["fin_tokens"][b, nf, s] = EOS
                    st["fin_len"][b, nf] = s + 1
                    st["fin_score"][b, nf] = c[k]["score"] / float(s + 1)  # normalize_scores, len_penalty 1
                    nf += 1
        st["nfinal"][b] = nf
        if any_eos and not was_finished and (nf == beam or s == MAX_LEN):
            st["finished"][b] = 1
        dead = [em[k] or bool(ign[k]) for k in range(beam)]
        live = [k for k in range(beam) if not dead[k]]
        act = live + [k for k in range(beam) if dead[k]]
        st["ignore"][b] = torch.tensor([1 if i >= len(live) else 0 for i in range(beam)], dtype=torch.uint8)
        if s < MAX_LEN:
            for i, k in enumerate(act):
                src, dst = c[k]["row"], b * beam + i
                new_tokens[dst, :s + 1] = tokens[src, :s + 1]
                new_tokens[dst, s + 1] = c[k]["tok"]
                new_scores[dst, :s] = scores[src, :s]
                new_scores[dst, s] = c[k]["score"]
                new_anc[dst, :s + 1] = anc[src, :s + 1]
                new_anc[dst, s + 1] = dst
    if s < MAX_LEN:
        st["tokens"], st["scores"], st["anc"] = new_tokens, new_scores, new_anc


def case_key(dtype_name, V, members, variant):
    return (0x9E3779B1 * (V + 13 * members + (7 if dtype_name == "bf16" else 0)) + 0x85EBCA77 * sorted(VARIANTS).index(variant) + 1) & _M32


def run_restatement(dtype_name, V, members, variant):
    """The whole search by the restatement alone: (state, draws, undecidable draws)."""
    topk, topp, temperature, ngram, with_prefix, min_len = VARIANTS[variant]
    prefix = torch.tensor(PREFIX) if with_prefix else None
    key = case_key(dtype_name, V, members, variant)
    st = new_state()
    n = bad = 0
    for s in range(MAX_LEN + 1):
        logits = step_logits(dtype_name, V, members, s)
        lp = masked_lprobs(st, logits, s, temperature, ngram, prefix, min_len)
        cands = step_draws(st, lp, s, key, topk, topp, prefix)
        n += len(cands)
        bad += sum(not d["decidable"] for d in cands)
        bookkeeping(st, cands, s)
    return st, n, bad
