"""fp64 restatement, derived forward-error bounds and an fp32 op-by-op evaluation of the kernels in csrc/ctc.hip: cst_ctc_fwd,
cst_ctc_bwd, cst_ctc_greedy.  Plain torch / numpy on the CPU; shared by test_ctc_ref_cpu.py (the restatement equals torch's
F.ctc_loss on fp64 log_softmax with autograd; the bounds hold for a faithful fp32 evaluation and reject every listed defect) and
test_ctc_gpu.py (the kernels under the same bounds).

How the bounds are built (the conventions of loss_optim_ref.py).  Every fp32 operation returns (x op y)(1 + d), |d| <= u = 2^-24;
expf and logf are libm-accurate: 1 ulp, counted as 2u relative.  A bf16 store rounds to nearest even, |d| <= 2^-8.  The logits ROUNDED
to the storage type are the exact inputs.  All errors below are ABSOLUTE errors of log-domain numbers unless said otherwise.

Row stage, frame t (mx = the row maximum, exact):
    se = sum_v exp(x_v - mx):  a term's argument is rounded (|x_v - mx| u, relative on the term after the exponential) and expf adds 2u;
         the adds: one per element of a thread's chain, 6 wave-shuffle adds, (waves - 1) adds.  Relative error of se:
         Cse_t u,  Cse_t = CHAIN(V) + 2 + sum_v softmax_v |x_v - mx|          [CHAIN: row_chain()]
    l = mx + logf(se):  Cse_t u (conditioning of log) + 2u |log se| (logf) + u |l| (the add)          =: dl_t
    e_t(s) = x[l'_s] - l:  dl_t + u |e_t(s)|
Recursion step (alpha; beta alike).  logsumexp is 1-Lipschitz in the sup norm, so the inputs' errors D_{t-1} pass through unamplified.
    m = max (exact);  exp(a_i - m): argument rounding weighted by the term, sum_i w_i |a_i - m| u <= 2/e u < 1u, expf 2u, two adds 2u:
    the sum's relative error 5u;  logf: 2u log 3 < 2.2u;  m + log: u |lse3|;  + e: u |alpha_t(s)|;  the emission's own error.
    D_t = D_{t-1} + u (7.2 + max_s (|alpha_t(s) - e_t(s)| + |alpha_t(s)| + |e_t(s)|)) + dl_t        (max over the finite states)
    D_0 = max_s (dl_0 + u |e_0(s)|).
So D_t = u (c1 t + c2 M) with M the running sum of the log-domain magnitudes READ OFF THE fp64 RECURSION: the error grows with
|alpha|, |beta| (hundreds to thousands at the longer cases), not with the gradient.  That is a worst-case count (every rounding in one
direction along the whole chain); observed errors are far inside it at large T, which the GPU test prints.
    nll = -lse3(alpha_T(S-1), alpha_T(S-2)):  Dalpha_{T-1} + u (7.2 + |nll|)
    loss = (float) sum in double:  sum_b dnll_b + u |loss|
Gradient at a live frame, class c with n_c states:  ab(s) = alpha + beta: Dalpha_t + Dbeta_t + u |ab(s)|;
    lsec = logsumexp over the class's states: relative error of the sum (2 + max(n_c, 10) + 0.37 n_c) u (chain of at most n_c adds — the
    blank's tree is shorter than 10 + ceil(n_c / 64) —, expf, weighted argument roundings n_c / e), logf 2u log n_c, the add u |lsec|;
    z = (lsec + nll) - lp:  the three inputs' errors + u |lsec + nll| + u |z|;   lp = x_c - l: dl_t + u |lp|
    occ = expf(z): occ (exp(dz) - 1) + 2u occ  (dz is NOT small at the long cases, so not linearised);   p = expf(lp): p (dlp + 2u)
    out = g (p - occ): 2u |out|;  a bf16 store: 2^-8 |out| on top.  A class outside the target: g p only.
Frames at or past the input length, and every frame of an infeasible utterance under zero_infinity: bound 0 (exact zeros).
SLACK = 1 + 2^-10 covers the second-order products; FLUSH: expf may return 0 below the smallest normal.
No constant here was fitted to an output of the kernels or of the evaluation below."""
import functools
import math

import numpy as np
import torch

U32 = 2.0 ** -24
UBF = 2.0 ** -8
FLUSH = 2.0 ** -126
SLACK = 1.0 + 2.0 ** -10

DEFECTS = ("skip_equal", "skip_blank", "no_last_blank", "wrong_blank", "grad_past_len", "no_softmax", "zero_inf_grad_kept")
GREEDY_DEFECTS = ("no_collapse", "collapse_after_blank")
RECURSION_DEFECTS = ("beta_skip_lost_past_1024",)  # judged on alpha / beta themselves (alpha_beta_bounds)

# name -> dict(T, B, V, L, in_len, blank, std, zero_infinity, targets (explicit, optional))
CASES = {
    "edge": dict(T=12, B=3, V=5, L=(0, 1, 4), in_len=(12, 7, 9)),
    "edge_blank_last": dict(T=12, B=3, V=5, L=(0, 1, 4), in_len=(12, 7, 9), blank=4),
    "repeats_inf": dict(T=9, B=2, V=6, L=(4, 4), in_len=(6, 5), targets=((2, 2, 3, 3), (4, 4, 1, 1))),
    "repeats_zero_inf": dict(T=9, B=2, V=6, L=(4, 4), in_len=(6, 5), targets=((2, 2, 3, 3), (4, 4, 1, 1)), zero_infinity=True),
    "wave": dict(T=140, B=2, V=32, L=(32, 33), in_len=(140, 100)),
    "workgroup": dict(T=640, B=2, V=32, L=(600, 300), in_len=(640, 640)),
    "longest": dict(T=1499, B=2, V=32, L=(400, 10), in_len=(1499, 1200)),
    "wide1000": dict(T=64, B=2, V=1000, L=(20, 7), in_len=(64, 50), std=8.0),
    "wide10000": dict(T=16, B=2, V=10000, L=(6, 3), in_len=(16, 11)),
}


def make_case(name, dtype=torch.float32):
    """(logits [T, B, V] in dtype, targets int64 [B, Lmax], target_len, input_len, blank, zero_infinity) of a named case; labels are
    random non-blank classes, with adjacent repeats kept wherever the input length leaves room for them."""
    c = CASES[name]
    T, B, V = c["T"], c["B"], c["V"]
    blank = c.get("blank", 0)
    g = torch.Generator(device="cpu")
    g.manual_seed(1000 + sorted(CASES).index(name))
    x = (torch.randn(T, B, V, generator=g) * c.get("std", 3.0)).to(dtype)
    Lmax = max(c["L"])
    targets = torch.zeros(B, max(Lmax, 0), dtype=torch.int64)
    classes = [v for v in range(V) if v != blank]
    for b, L in enumerate(c["L"]):
        if "targets" in c:
            row = list(c["targets"][b])
        else:
            row = [classes[i] for i in torch.randint(len(classes), (L,), generator=g).tolist()]
            for j in range(1, L):  # take out adjacent repeats while the utterance would be infeasible
                if L + sum(row[i] == row[i - 1] for i in range(1, L)) <= c["in_len"][b]:
                    break
                while row[j] == row[j - 1]:
                    row[j] = classes[(classes.index(row[j]) + 1) % len(classes)]
        targets[b, :L] = torch.tensor(row, dtype=torch.int64)
    return (x, targets, torch.tensor(c["L"], dtype=torch.int64), torch.tensor(c["in_len"], dtype=torch.int64), blank,
            c.get("zero_infinity", False))


def row_chain(V, dtype):
    """Adds on the longest chain of a row sum in ctc_rows_kernel: 64 threads up to 512 classes, else 256; a thread adds its groups of
    VEC (4 fp32 / 8 bf16) elements in turn; then 6 shuffle adds and one add per further wave."""
    nt = 64 if V <= 512 else 256
    vec = 8 if dtype == torch.bfloat16 else 4
    return vec * math.ceil(V / (vec * nt)) + 6 + (nt // 64 - 1)


def _lse3(a, b, c):
    """m + log(exp(a - m) + exp(b - m) + exp(c - m)), -inf where all three are (the kernel's ctc_lse3), in the operands' dtype."""
    m = torch.maximum(a, torch.maximum(b, c))
    ms = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    r = ms + torch.log((torch.exp(a - ms) + torch.exp(b - ms)) + torch.exp(c - ms))
    return torch.where(torch.isinf(m) & (m < 0), m, r)


def _lse_cols(ab, idx):
    """logsumexp over the columns idx of ab [T, S], the maximum taken out, terms added in increasing s; -inf where all are."""
    sub = ab[:, idx]
    m = sub.max(dim=1).values
    ms = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    s = torch.zeros_like(m)
    for j in range(sub.shape[1]):
        s = s + torch.exp(sub[:, j] - ms)
    return torch.where(torch.isinf(m) & (m < 0), m, ms + torch.log(s))


def ctc_eval(x, targets, target_len, input_len, blank, zero_infinity=False, gscale=1.0, dt=torch.float64, defect=None):
    """The operation sequence of cst_ctc_fwd / cst_ctc_bwd in the arithmetic `dt` (fp64: the reference; fp32: a faithful evaluation;
    `defect`: one of DEFECTS).  x [T, B, V] (its values are the exact inputs).  Returns dict(nll [B], loss, grad [T, B, V]) and the
    terms the bounds are stated in."""
    T, B, V = x.shape
    ninf = float("-inf")
    eblank = (blank + 1) % V if defect == "wrong_blank" else blank
    nll = torch.zeros(B, dtype=dt)
    grad = torch.zeros(T, B, V, dtype=dt)
    terms = []
    for b in range(B):
        Tb, L = int(input_len[b]), int(target_len[b])
        S = 2 * L + 1
        ext = torch.full((S,), eblank, dtype=torch.int64)
        ext[1::2] = targets[b, :L]
        xb = x[:Tb, b].to(dt)
        mx = xb.max(dim=1, keepdim=True).values
        se = torch.exp(xb - mx).sum(dim=1, keepdim=True)
        l = mx + torch.log(se)
        e = xb[:, ext] - l
        s_idx = torch.arange(S)
        skip = torch.zeros(S, dtype=torch.bool)
        if S > 2:
            skip[2:] = (ext[2:] != eblank) & (ext[2:] != ext[:-2])
            if defect == "skip_equal":
                skip[2:] = ext[2:] != eblank
            if defect == "skip_blank":
                skip[2:] = True
        skipb = torch.zeros(S, dtype=torch.bool)
        skipb[:-2] = skip[2:]
        if defect == "beta_skip_lost_past_1024":  # what a second-pass (k > 0) state of the 1024-thread recursion would do on a striding slip
            skipb[1024:] = False
        alpha = torch.full((Tb, S), ninf, dtype=dt)
        beta = torch.full((Tb, S), ninf, dtype=dt)
        pad = torch.full((2,), ninf, dtype=dt)
        alpha[0, :2] = e[0, :2]
        beta[Tb - 1, max(S - 2, 0):] = e[Tb - 1, max(S - 2, 0):]
        for t in range(1, Tb):
            a = torch.cat([pad, alpha[t - 1]])
            alpha[t] = _lse3(a[2:], a[1:-1], torch.where(skip, a[:-2], pad[0])) + e[t]
        for t in range(Tb - 2, -1, -1):
            a = torch.cat([beta[t + 1], pad])
            beta[t] = _lse3(a[:-2], a[1:-1], torch.where(skipb, a[2:], pad[0])) + e[t]
        last2 = alpha[Tb - 1, S - 2] if S > 1 else pad[0]
        last1 = pad[0] if (defect == "no_last_blank" and S > 1) else alpha[Tb - 1, S - 1]
        nl = -_lse3(last1.reshape(1), last2.reshape(1), pad[:1])[0]
        nll[b] = nl
        p = torch.exp(xb - l)
        gb = torch.zeros_like(p) if defect == "no_softmax" else p.clone()
        ab = alpha + beta
        occ_info = {}
        for c in sorted(set(ext.tolist())):
            idx = s_idx[ext == c]
            lsec = _lse_cols(ab, idx)
            lp = xb[:, c] - l[:, 0]
            z = (lsec + nl) - lp
            occ = torch.exp(z)
            gb[:, c] = (torch.zeros_like(occ) if defect == "no_softmax" else torch.exp(lp)) - occ
            occ_info[c] = (len(idx), lsec, z, occ)
        if zero_infinity and bool(torch.isinf(nl)) and defect != "zero_inf_grad_kept":
            gb = torch.zeros_like(gb)
        grad[:Tb, b] = gscale * gb
        if defect == "grad_past_len" and Tb < T:
            xd = x[Tb:, b].to(dt)
            grad[Tb:, b] = gscale * torch.softmax(xd, dim=1)
        terms.append(dict(Tb=Tb, L=L, S=S, ext=ext, xb=xb, mx=mx, se=se, l=l, e=e, alpha=alpha, beta=beta, p=p, occ=occ_info, nll=nl))
    contrib = torch.where(torch.isinf(nll), torch.zeros_like(nll), nll) if zero_infinity else nll
    return dict(nll=nll, loss=contrib.double().sum().to(dt), grad=grad, terms=terms)  # (the kernel adds the nll in double)


def _finite_max(t, dim):
    return torch.where(torch.isfinite(t), t, torch.zeros_like(t)).max(dim=dim).values


def recursion_bounds(tm, chain):
    """(dl [Tb], Dalpha [Tb], its magnitudes, Dbeta [Tb], its magnitudes) of one utterance's terms: the absolute log-domain error bounds
    of the frame log-sum-exp and of alpha_t(.) / beta_t(.) (sup over the finite states), as derived in the module docstring."""
    u, Tb = U32, tm["Tb"]
    cse = chain + 2 + (tm["p"] * (tm["xb"] - tm["mx"]).abs()).sum(dim=1)
    dl = u * (cse + 2 * tm["se"][:, 0].log().abs() + tm["l"][:, 0].abs())  # [Tb]

    def run(var, order):
        D = torch.zeros(Tb, dtype=torch.float64)
        mags = torch.zeros(Tb, dtype=torch.float64)
        prev = None
        for t in order:
            fin = torch.isfinite(var[t])
            ea = torch.where(fin, tm["e"][t].abs(), torch.zeros_like(var[t]))
            va = torch.where(fin, var[t].abs(), torch.zeros_like(var[t]))
            if prev is None:
                D[t] = dl[t] + u * ea.max()
                mags[t] = ea.max()
            else:
                lse_a = torch.where(fin, (var[t] - tm["e"][t]).abs(), torch.zeros_like(var[t]))
                mags[t] = (lse_a + va + ea).max()
                D[t] = D[prev] + u * (7.2 + mags[t]) + dl[t]
            prev = t
        return D, mags
    Da, ma = run(tm["alpha"], range(Tb))
    Db, mb = run(tm["beta"], range(Tb - 1, -1, -1))
    return dl, Da, ma, Db, mb


def alpha_beta_bounds(r, x, dtype):
    """Per utterance (alpha fp64 [Tb, S], beta, Dalpha [Tb] * SLACK, Dbeta [Tb] * SLACK): the forward / backward variables themselves
    under their log-domain bounds — orders of magnitude tighter, relative to |alpha| ~ 10^3, than what the occupancy term of the gradient
    allows at the long cases, so a state that reads a wrong neighbour cannot hide."""
    chain = row_chain(x.shape[2], dtype)
    out = []
    for tm in r["terms"]:
        _, Da, _, Db, _ = recursion_bounds(tm, chain)
        out.append((tm["alpha"], tm["beta"], Da * SLACK, Db * SLACK))
    return out


def ctc_bounds(r, x, input_len, dtype, gscale=1.0, zero_infinity=False):
    """Per-element bounds (nll [B], loss, grad [T, B, V]) for the kernels at the fp64 result r = ctc_eval(...); also M [B], the sum of
    the log-domain magnitudes the recursion's bound is proportional to (printed by the tests).  An utterance whose nll is +inf gets
    bound 0 on nll (the kernel must return +inf exactly) and, under zero_infinity, 0 on its gradient."""
    T, B, V = x.shape
    u = U32
    chain = row_chain(V, dtype)
    bn = torch.zeros(B, dtype=torch.float64)
    bg = torch.zeros(T, B, V, dtype=torch.float64)
    M = torch.zeros(B, dtype=torch.float64)
    for b, tm in enumerate(r["terms"]):
        Tb = tm["Tb"]
        if Tb == 0:
            continue
        soft = tm["p"]
        dl, Da, ma, Db, mb = recursion_bounds(tm, chain)
        M[b] = ma.sum() + mb.sum()
        nl = tm["nll"]
        infeasible = bool(torch.isinf(nl))
        dnll = float(Da[Tb - 1]) + u * (7.2 + (0.0 if infeasible else abs(float(nl))))
        bn[b] = 0.0 if infeasible else dnll * SLACK
        if infeasible:
            if not zero_infinity:
                bg[:Tb, b] = float("inf")  # any value: the test asks for a non-finite element there
            continue
        # classes outside the target: g * p
        dlp_all = dl[:, None] + u * (tm["xb"] - tm["l"]).abs()
        bcls = soft * (dlp_all + 2 * u) + 2 * u * soft
        for c, (n_c, lsec, z, occ) in tm["occ"].items():
            ab = tm["alpha"] + tm["beta"]
            abm = _finite_max(ab[:, tm["ext"] == c].abs(), 1)
            d_ab = Da + Db + u * abm
            lf = torch.where(torch.isfinite(lsec), lsec.abs(), torch.zeros_like(lsec))
            d_lsec = d_ab + u * ((2 + max(n_c, 10) + 0.37 * n_c) + 2 * math.log(max(n_c, 2)) + lf)
            lp = tm["xb"][:, c] - tm["l"][:, 0]
            d_lp = dl + u * lp.abs()
            zf = torch.where(torch.isfinite(z), z.abs(), torch.zeros_like(z))
            dz = d_lsec + dnll + u * (lf + abs(float(nl))) + d_lp + u * zf
            pc = soft[:, c]
            out = (pc - occ).abs()
            bcls[:, c] = pc * (d_lp + 2 * u) + occ * torch.expm1(dz) + 2 * u * occ + 2 * u * out
        val = r["grad"][:Tb, b].abs()
        bg[:Tb, b] = (abs(gscale) * bcls * SLACK + FLUSH) * (1 + (UBF if dtype == torch.bfloat16 else 0.0)) \
            + (UBF * val if dtype == torch.bfloat16 else 0.0)
    fin = torch.where(torch.isinf(r["nll"]), torch.zeros_like(r["nll"]), r["nll"]) if zero_infinity else r["nll"]
    bl = float((bn.sum() + u * fin.abs().sum()) * SLACK)
    return bn, bl, bg, M


def worst_ratio(got, ref, bound):
    """(max |got - ref| / bound, elements over the bound).  A zero bound demands the exact value; an infinite bound accepts anything;
    where the reference is infinite the result must be the same infinity."""
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    bound = bound.double().reshape(-1).expand_as(ref)
    same_inf = torch.isinf(ref) & (got == ref)
    err = torch.where(same_inf, torch.zeros_like(ref), (got - ref).abs())
    free = torch.isinf(bound)
    bad = ~(err <= bound) & ~free
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    ratio = torch.where(free | torch.isnan(ratio), torch.zeros_like(ratio), ratio)
    return (float(ratio.max()) if ratio.numel() else 0.0), int(bad.sum())


def greedy_ref(x, input_len, blank, defect=None):
    """Best path per utterance: argmax over classes (numpy: the first of equal maxima) of the live frames, runs collapsed, blanks dropped.
    Returns a list of B lists of ids."""
    T, B, V = x.shape
    out = []
    for b in range(B):
        am = np.argmax(x[:int(input_len[b]), b].float().numpy(), axis=1).tolist()
        if defect == "collapse_after_blank":
            am = [a for a in am if a != blank]
        if defect != "no_collapse":
            am = [a for i, a in enumerate(am) if i == 0 or a != am[i - 1]]
        out.append([a for a in am if a != blank])
    return out


@functools.lru_cache(maxsize=None)
def reference(name, dtype):
    """(inputs, fp64 result, bounds) of a named case at a storage type, computed once per process and shared; do not modify."""
    x, tg, tl, il, blank, zi = make_case(name, dtype)
    r = ctc_eval(x, tg, tl, il, blank, zi)
    return (x, tg, tl, il, blank, zi), r, ctc_bounds(r, x, il, dtype, 1.0, zi)


def judge(name, dtype, got):
    """Elements of (nll, loss, grad) outside the bounds, with the worst ratios."""
    (x, tg, tl, il, blank, zi), r, (bn, bl, bg, M) = reference(name, dtype)
    rn, badn = worst_ratio(got["nll"], r["nll"], bn)
    rl, badl = worst_ratio(got["loss"].reshape(1), r["loss"].reshape(1), torch.tensor([bl]))
    rg, badg = worst_ratio(got["grad"], r["grad"], bg)
    if not zi:  # an infeasible utterance without zero_infinity: a non-finite gradient element is required
        for b in range(x.shape[1]):
            if torch.isinf(r["nll"][b]) and bool(torch.isfinite(got["grad"][:int(il[b]), b].float()).all()):
                badg += 1
    return (rn, rl, rg), badn + badl + badg, M


def greedy_logits():
    """[T = 20, B = 4, V = 7] with exact ties, a run that continues across the input-length boundary, an all-blank utterance and an
    utterance whose last run ends at its last live frame; (logits, input_len, blank)."""
    g = torch.Generator(device="cpu")
    g.manual_seed(7)
    T, B, V, blank = 20, 4, 7, 0
    x = torch.randn(T, B, V, generator=g)
    il = torch.tensor([20, 13, 16, 9], dtype=torch.int64)
    for t, c in enumerate([3, 3, 0, 3, 5, 5, 5, 0, 0, 2, 2, 6, 6, 6, 6, 1, 0, 4, 4, 4]):
        x[t, 0, c] = 9.0
    x[4, 0, 2] = 9.0          # a tie of classes 2 and 5: the lower wins, the run of 5 starts a frame later
    x[10, 0, 6] = 9.0         # a tie of 2 and 6: 2 continues its run
    for t in range(T):
        x[t, 1, 4 if t < 6 else 2] = 8.0   # the run of 2 goes on past input_len = 13
    x[:, 2, blank] = 7.0      # all blank
    for t in range(T):
        x[t, 3, [1, 1, 0, 0, 1, 3, 3, 0, 5][t % 9]] = 8.0  # the last run (5) is the last live frame
    x[3, 3, 0] = 8.0
    x[3, 3, 6] = 8.0          # a tie of blank and 6 inside a blank run: blank
    return x, il, blank


def judge_alpha_beta(name, dtype, alphas, betas):
    """alphas / betas: per utterance [Tb, S] tensors.  (worst err / bound, elements outside) against the fp64 variables; -inf states
    must be -inf."""
    (x, tg, tl, il, blank, zi), r, _ = reference(name, dtype)
    worst, bad = 0.0, 0
    for b, (a64, b64, Da, Db) in enumerate(alpha_beta_bounds(r, x, dtype)):
        for got, ref, D in ((alphas[b], a64, Da), (betas[b], b64, Db)):
            ratio, nbad = worst_ratio(got, ref, D[:, None].expand_as(ref))
            worst, bad = max(worst, ratio), bad + nbad
    return worst, bad
