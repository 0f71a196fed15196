"""fp64 restatement, brute-force enumeration and counted error bounds for the kernels in csrc/ctc_decode.hip: cst_ctc_topn and
cst_ctc_beam (CTC prefix beam search; Graves 2006 §7.5.3, Hannun et al. 2014 Alg. 1).  Plain numpy on the CPU; shared by
test_ctc_beam_ref_cpu.py (the restatement equals the enumeration, every listed defect does not) and test_ctc_beam_gpu.py (the kernels
under the same bounds).  The conventions are those of ctc_ref.py.

Rules restated (include/cst.h has them in full).  A beam entry is (prefix, p_b, p_nb); (+) is logaddexp.  Per frame with log-probabilities
lp and the list = the N most probable non-blank classes by (lp descending, id ascending), for every entry l, tot = p_b (+) p_nb:
    stay    p_b'(l) = tot + lp[blank];  p_nb'(l) = p_nb + lp[last(l)] (l not empty; the exact lp, listed or not)
    extend  c in the list:  v = (p_b if c == last(l) else tot) + lp[c];  where l + c is a beam entry l', p_nb'(l') (+)= v, else (l + c, -inf, v)
    select  score = p_b' (+) p_nb';  drop -inf and scores below best - theta;  keep the best K by (score descending, source rank, stay
            before extension, token id).
A prefix is identified by an interned id (parent id, token) — exact, never a hash of the string.

How the bounds are built.  Every fp32 operation returns (x op y)(1 + d), |d| <= u = 2^-24; expf and logf count 2u relative.  The logits
rounded to the storage type are the exact inputs.  All errors are ABSOLUTE errors of log-domain numbers.
    row:    l = mx + logf(se) carries dl_t = u (CHAIN + 2 + sum_v softmax_v |x_v - mx| + 2 |log se| + |l|) (ctc_ref.py, row stage), and
            lp_c = x_c - l carries dl_t + u |lp_c|                                                                        =: dlp_t(c)
    a (+) b = m + logf(1 + expf(n - m)), m >= n:  the argument's rounding weighs (m - n) e^-(m - n) <= 1/e on the term, expf 2u on a term
            <= 1/2 of the sum, the add 1u: the sum is off by (0.37 + 1 + 1) u relatively, its log by the same absolutely; logf adds
            2u log 2 < 1.4u; the last add u |a (+) b|.  In all u (3.8 + |a (+) b|), and (+) passes its inputs' errors on unamplified
            (1-Lipschitz in the sup norm).
    step, the beam's (p_b, p_nb) taken as exact inputs, A_t = the largest finite magnitude among tot, p_b', p_nb', v and the scores,
            P_t = the largest |lp| the step reads:  tot: u (3.8 + A);  + lp: dlp + u A;  the merge's (+): u (3.8 + A);  the score's (+):
            u (3.8 + A).  Every number the step produces is within
                step_bound_t = dl_t + u (P_t + 11.4 + 4 A_t)
    run:    errors of the inputs pass through a step unamplified, so after frame t every beam number is within D_t = sum_{s <= t}
            step_bound_s, and a final score within D_T + u (3.8 + |score|).
SLACK = 1 + 2^-10 covers the second-order products.  No constant here was fitted to an output of the kernels."""
import itertools
import math

import numpy as np
import torch

from ctc_ref import SLACK, U32, row_chain

NINF = float("-inf")
DEFECTS = ("repeat_from_tot", "no_merge", "no_repeat_stay", "wrong_blank", "threshold_before_merge", "stay_from_list_only")


def lae(a, b):
    m, n = (a, b) if a >= b else (b, a)
    if m == NINF:
        return NINF
    return m + math.log1p(math.exp(n - m))


def row_terms(x, dtype=torch.float32):
    """x [T, V]: the stored logits as float64 (exact inputs) -> (lp [T, V] fp64 log-softmax, dl [T] the counted bound of the frame's
    log-sum-exp as the kernels compute it)."""
    x = np.asarray(x, dtype=np.float64)
    mx = x.max(axis=1, keepdims=True)
    ex = np.exp(x - mx)
    se = ex.sum(axis=1, keepdims=True)
    l = mx + np.log(se)
    cse = row_chain(x.shape[1], dtype) + 2 + (ex / se * np.abs(x - mx)).sum(axis=1)
    dl = U32 * (cse + 2 * np.abs(np.log(se[:, 0])) + np.abs(l[:, 0]))
    return x - l, dl


def top_list(lp_row, blank, N):
    """ids of the N most probable non-blank classes by (lp descending, id ascending)."""
    ids = [v for v in range(len(lp_row)) if v != blank]
    ids.sort(key=lambda v: (-lp_row[v], v))
    return ids[:N]


def brute(lp, blank):
    """{labelling (tuple): log-probability}: all V^T alignments summed per collapsed labelling, in fp64."""
    T, V = lp.shape
    acc = {}
    for path in itertools.product(range(V), repeat=T):
        s = 0.0
        for t, c in enumerate(path):
            s += lp[t, c]
        lab = tuple(c for i, c in enumerate(path) if c != blank and (i == 0 or c != path[i - 1]))
        acc.setdefault(lab, []).append(s)
    out = {}
    for lab, terms in acc.items():
        m = max(terms)
        out[lab] = m + math.log(sum(math.exp(s - m) for s in terms)) if m > NINF else NINF
    return out


class Trie:
    """Interned prefixes: id 0 is the empty prefix; child(p, c) is THE id of p + c."""

    def __init__(self):
        self.par, self.tok, self.kids = [-1], [-1], {}

    def child(self, p, c):
        k = (p, c)
        i = self.kids.get(k)
        if i is None:
            i = self.kids[k] = len(self.par)
            self.par.append(p)
            self.tok.append(c)
        return i

    def prefix(self, i):
        out = []
        while i > 0:
            out.append(self.tok[i])
            i = self.par[i]
        return tuple(reversed(out))


def step(trie, beam, lp_row, blank, K, N, theta, defect=None):
    """One frame in fp64.  beam: list of (id, p_b, p_nb) in rank order.  Returns (cands, cut, A, P): cands = every candidate after merging
    as (score, key, id, p_b', p_nb') sorted by the selection order (not yet cut or pruned), cut = best - theta, A / P = the magnitudes of
    the module docstring."""
    V = len(lp_row)
    eblank = (blank + 1) % V if defect == "wrong_blank" else blank
    lst = top_list(lp_row, eblank, N)
    inlist = {c: n for n, c in enumerate(lst)}
    pos = {e[0]: i for i, e in enumerate(beam)}
    A, P = 0.0, abs(lp_row[eblank])

    def mag(*vs):
        nonlocal A
        for v in vs:
            if v != NINF and abs(v) > A:
                A = abs(v)
    tots, spb, spnb = [], [], []
    for (pid, pb, pnb) in beam:
        tt = lae(pb, pnb)
        last = trie.tok[pid]
        rep = NINF
        if pid != 0 and defect != "no_repeat_stay" and not (defect == "stay_from_list_only" and last not in inlist):
            rep = pnb + lp_row[last]
            P = max(P, abs(lp_row[last]))
        tots.append(tt)
        spb.append(tt + lp_row[eblank])
        spnb.append(rep)
        mag(tt, spb[-1], rep)
    lpl = np.array([lp_row[c] for c in lst], dtype=np.float64)
    if len(lst):
        P = max(P, float(np.abs(lpl[np.isfinite(lpl)]).max()) if np.isfinite(lpl).any() else 0.0)
    ext = {}  # (i, n) -> v
    vals = np.empty((len(beam), len(lst)), dtype=np.float64)
    for i, (pid, pb, pnb) in enumerate(beam):
        vals[i] = tots[i] + lpl
        last = trie.tok[pid]
        if last in inlist and defect != "repeat_from_tot":
            vals[i, inlist[last]] = pb + lp_row[last]
    fin = vals[np.isfinite(vals)]
    if fin.size:
        mag(float(np.abs(fin).max()))
    dead = np.zeros(vals.shape, dtype=bool)
    if defect == "threshold_before_merge" and vals.size:
        pre = max([lae(a, b) for a, b in zip(spb, spnb)] + [float(vals.max())])
        dead = vals < pre - theta
    merged = np.zeros(vals.shape, dtype=bool)
    if defect != "no_merge":
        for j, (pid, _, _) in enumerate(beam):
            if pid == 0:
                continue
            i, n = pos.get(trie.par[pid]), inlist.get(trie.tok[pid])
            if i is not None and n is not None:
                merged[i, n] = True
                if not dead[i, n]:
                    spnb[j] = lae(spnb[j], float(vals[i, n]))
                    mag(spnb[j])
    cands = []
    for i, (pid, _, _) in enumerate(beam):
        sc = lae(spb[i], spnb[i])
        mag(sc)
        cands.append((sc, (i, 0, -1), pid, spb[i], spnb[i]))
    for i, n in zip(*np.nonzero(~merged & ~dead & (vals > NINF))):
        c = lst[n]
        cands.append((float(vals[i, n]), (int(i), 1, c), trie.child(beam[i][0], c), NINF, float(vals[i, n])))
    cands.sort(key=lambda r: (-r[0], r[1]))
    best = cands[0][0] if cands else NINF
    return cands, best - theta, A, P


def select(cands, cut, K):
    """(the next beam [(id, p_b, p_nb)], the smallest decision gap of this frame: K / K+1 boundary and threshold boundary)."""
    live = [r for r in cands if r[0] > NINF and r[0] >= cut]
    gap = math.inf
    if len(live) > K:
        gap = min(gap, live[K - 1][0] - live[K][0])
    if cut > NINF:
        for r in cands:
            if r[0] > NINF:
                gap = min(gap, abs(r[0] - cut))
    return [(r[2], r[3], r[4]) for r in live[:K]], gap


def step_bound(dl_t, A, P):
    return (dl_t + U32 * (P + 11.4 + 4 * A)) * SLACK


def prefix_beam_search(lp, blank, K, N, theta, defect=None, dl=None, keep=False):
    """The whole search in fp64 on log-probabilities lp [T, V].  Returns dict(hyps = [(labelling, score)] best first (the whole final
    beam), gap = the smallest decision gap met (every frame's K / K+1 and threshold boundaries, adjacent final hypotheses), bound = the
    counted bound D_T + u (3.8 + max |score|) on a final score (needs dl from row_terms), beams = per frame [(labelling, p_b, p_nb)]
    with keep)."""
    trie = Trie()
    beam = [(0, 0.0, NINF)]
    gap, D, beams = math.inf, 0.0, []
    for t in range(lp.shape[0]):
        cands, cut, A, P = step(trie, beam, lp[t], blank, K, N, theta, defect)
        beam, g = select(cands, cut, K)
        gap = min(gap, g)
        if dl is not None:
            D += step_bound(dl[t], A, P)
        if keep:
            beams.append([(trie.prefix(i), pb, pnb) for i, pb, pnb in beam])
        if not beam:
            break
    hyps = [(trie.prefix(i), lae(pb, pnb)) for i, pb, pnb in beam]
    for a, b in zip(hyps, hyps[1:]):
        gap = min(gap, a[1] - b[1])
    smax = max([abs(s) for _, s in hyps] + [0.0])
    return dict(hyps=hyps, gap=gap, bound=(D + U32 * (3.8 + smax) * SLACK) if dl is not None else None, beams=beams)


def check_step(prev_beam, frame, next_beam, bound=None):
    """prev_beam / next_beam: lists of (labelling tuple, p_b, p_nb) in rank order — prev_beam's numbers are taken as exact inputs.  frame:
    dict(lp = the frame's fp64 log-probabilities [V], dl = its counted row bound, blank, K, N, theta, defect (optional: the step is then
    computed WITH the defect — never used to judge)).  bound: None = the counted step bound.  Returns (ok, reason, bound).  Accepted only
    if BOTH hold: every number of next_beam lies within `bound` of the fp64 step's, and next_beam is a legal selection — no duplicate, at
    most K, in descending order, nothing included that the threshold excludes and no excluded candidate that beats an included one, each
    by more than 2 * bound."""
    trie = Trie()

    def intern(lab):
        i = 0
        for c in lab:
            i = trie.child(i, c)
        return i
    beam = [(intern(lab), float(pb), float(pnb)) for lab, pb, pnb in prev_beam]
    cands, cut, A, P = step(trie, beam, frame["lp"], frame["blank"], frame["K"], frame["N"], frame["theta"])
    if bound is None:
        bound = step_bound(frame["dl"], A, P)
    by_id = {r[2]: r for r in cands}
    got, seen = [], set()
    for lab, pb, pnb in next_beam:
        i = intern(lab)
        r = by_id.get(i)
        if r is None or r[0] == NINF:
            return False, "prefix %s is no candidate of this frame" % (lab,), bound
        if i in seen:
            return False, "prefix %s twice in the beam" % (lab,), bound
        seen.add(i)
        for g, w, what in ((float(pb), r[3], "p_b"), (float(pnb), r[4], "p_nb")):
            if (w == NINF) != (g == NINF) or (w != NINF and not abs(g - w) <= bound):
                return False, "%s of %s: %r against %r, bound %.3g" % (what, lab, g, w, bound), bound
        got.append(r)
    if len(got) > frame["K"]:
        return False, "more than K entries", bound
    for a, b in zip(got, got[1:]):
        if b[0] > a[0] + 2 * bound:
            return False, "not in descending order", bound
    for r in got:
        if r[0] < cut - 2 * bound:
            return False, "an entry below the threshold was kept", bound
    low = min([r[0] for r in got] + [math.inf])
    full = len(got) == frame["K"]
    for r in cands:
        if r[2] in seen or r[0] == NINF or r[0] < cut + 2 * bound:
            continue
        if not full or r[0] > low + 2 * bound:
            return False, "candidate %s (%.9g) left out, the beam's lowest is %.9g" % (trie.prefix(r[2]), r[0], low), bound
    return True, "", bound


def make_logits(T, V, seed, std=2.0, dtype=torch.float32, classes=None):
    """default_rng(seed).normal(0, std) logits [T, V] rounded to the storage type; classes: only these columns stay probable (the others
    are lowered by 30), which forces repeated labels and merges."""
    x = np.random.default_rng(seed).normal(0.0, std, size=(T, V))
    if classes is not None:
        low = np.ones(V, dtype=bool)
        low[list(classes)] = False
        x[:, low] -= 30.0
    x = torch.from_numpy(x).to(dtype)
    if dtype == torch.bfloat16:
        # bf16 has few values: equal logits in a row are exact ties, which no gap condition can hold.  The 128 largest values of a row
        # (no list is longer) are made strictly decreasing, each at least one bf16 step below the one before it; the others stay below.
        bits = x.view(torch.int16).numpy().view(np.uint16).copy()
        val = x.float().numpy()

        def below(b):  # the bits of the next bf16 value below the value of bits b
            if b & 0x7FFF == 0:
                return 0x8001
            return b - 1 if b < 0x8000 else b + 1

        def value(b):
            return float(np.array([int(b) << 16], dtype=np.uint32).view(np.float32)[0])
        for t in range(T):
            order = sorted(range(V), key=lambda v: (-val[t, v], v))
            top = min(V, 128)
            for r in range(1, top):
                a, c = order[r - 1], order[r]
                if not val[t, c] < val[t, a]:
                    bits[t, c] = below(int(bits[t, a]))
                    val[t, c] = value(bits[t, c])
            floor = order[top - 1]
            for c in order[top:]:
                if not val[t, c] < val[t, floor]:
                    bits[t, c] = below(int(bits[t, floor]))
                    val[t, c] = value(bits[t, c])
        x = torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16)
    return x


# name -> dict(T, V, K, N, theta, seed, std, blank, classes).  Committed only where the restatement's smallest decision gap is at least
# 4 x the counted bound on a score (asserted in test_ctc_beam_ref_cpu.py for fp32 and bf16 logits alike).
# seeds: one utterance each; in_len: their input lengths (default T).  The seeds were found by search on the CPU; where T = 140 left the
# counted bound above a quarter of the gap, T was shortened.
EXACT_CASES = {
    "wave": dict(T=40, V=32, K=8, N=31, seeds=(13,)),
    "wide1000": dict(T=8, V=1000, K=8, N=20, std=4.0, seeds=(2,)),
    "short_list": dict(T=32, V=32, K=8, N=4, std=1.0, seeds=(7,)),
    "threshold3": dict(T=24, V=32, K=8, N=31, theta=3.0, seeds=(32,)),
    "nbest_all": dict(T=24, V=32, K=8, N=31, theta=3.0, seeds=(32,), nbest=8),
    "brute6": dict(T=6, V=4, K=128, N=3, seeds=(3,)),
    "brute4": dict(T=4, V=4, K=128, N=3, seeds=(0,)),             # unpruned: all 64 labellings fit the beam
    "merges": dict(T=30, V=8, K=8, N=7, classes=(0, 1, 2), seeds=(1,)),  # low entropy over 3 classes: repeats and forced merges
    "few_candidates": dict(T=3, V=4, K=64, N=3, seeds=(0,)),      # K larger than the number of candidates
    "lengths": dict(T=20, V=32, K=8, N=31, seeds=(5, 100, 108), in_len=(0, 1, 20)),
    "blank_last": dict(T=20, V=32, K=8, N=31, seeds=(108,), blank=0, roll=True),  # the blank is class V - 1: columns rolled by one
}


def exact_case(name, dtype):
    """(x [T, B, V] in dtype, in_len, blank, params, per-utterance fp64 results with bound) of a committed exact case."""
    c = EXACT_CASES[name]
    T, V = c["T"], c["V"]
    xs = [make_logits(T, V, s, c.get("std", 2.0), dtype, c.get("classes")) for s in c["seeds"]]
    blank = c.get("blank", 0)
    if c.get("roll"):
        xs = [torch.roll(x, -1, dims=1) for x in xs]
        blank = V - 1
    in_len = c.get("in_len", (T,) * len(xs))
    res = []
    for x, n in zip(xs, in_len):
        lp, dl = row_terms(x[:n].double().numpy(), dtype) if n else (np.zeros((0, V)), np.zeros(0))
        res.append(prefix_beam_search(lp, blank, c["K"], c["N"], c.get("theta", math.inf), dl=dl))
    return torch.stack(xs, dim=1), in_len, blank, c, res
