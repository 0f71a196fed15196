"""fp64 restatement of cst_score_tokens (csrc/score.hip, include/cst.h), a per-element forward-error bound for an fp32 evaluation of
it, and fp32 emulations of the defects the bound has to reject.  Plain torch on the CPU; shared by test_decode_score_cpu.py (the
bound holds for the plain-torch scorer and rejects every listed defect) and test_decode_score_gpu.py (the kernel under the same bound).

The bound is built as tests/loss_optim_ref.py builds lsce_bounds: every fp32 operation returns (x op y)(1 + d), |d| <= U32; a
term's coefficient COUNTS the roundings it passes through in the kernel's operation sequence; __expf(a) carries EXP(a) = 2 + 3|a|
units of U32 (1 ulp of v_exp_f32 plus three relative errors of its argument: the subtraction, log2e, their product), __logf 2 units;
an exponential below 2^-126 may be flushed; bf16 logits are taken as the exact values they hold.  No constant here was fitted to an
output of the kernel or of an emulation.

The kernel's sequence, per non-pad position (256 threads) and member m:
    mx   = max_v x_v                                             exact
    se   = sum_v __expf(x_v - mx)    per thread: a head element, ceil(vectors / 256) vectors of VEC elements, a tail element,
                                     then 6 butterfly levels and 3 additions of the waves' sums
    lse  = fl(mx + __logf(se))
    l_m  = fl(x_target - lse)
    N = 1: pos = l_1
    N > 1: M = max_m l_m;  s = sum_m __expf(l_m - M) in member order;  pos = fl(fl(M + __logf(s)) - fl(log N))
per sentence: the non-pad pos are added in double, rounded to fp32 once and divided by fl(len)."""
import math

import torch

from loss_optim_ref import BLOCK_SUM_ADDS, ETA, FLUSH, NT, SLACK, U32, lsce_logits, worst_ratio

SCORE_DEFECTS = ("no_max_subtraction", "mean_of_logprobs", "divide_by_T", "pad_counted")


def score_ref64(logits_list, target, pad):
    """The definition in fp64: dict with pos [B, T] (0 at pad), score [B] (NaN without targets), len [B], and the terms the bound is
    stated in."""
    N = len(logits_list)
    live = target.ne(pad)
    idx = target.clamp(0, logits_list[0].size(-1) - 1).unsqueeze(-1)
    mem = []
    for x in logits_list:
        x = x.double()
        mx = x.max(-1).values
        e = (x - mx.unsqueeze(-1)).exp()
        se = e.sum(-1)
        lse = mx + se.log()
        mem.append(dict(x=x, mx=mx, se=se, lse=lse, l=x.gather(2, idx).squeeze(-1) - lse, w=e / se.unsqueeze(-1)))
    ls = torch.stack([m["l"] for m in mem], 0)
    pos = ls[0] if N == 1 else torch.logsumexp(ls, 0) - math.log(N)
    pos = torch.where(live, pos, torch.zeros_like(pos))
    length = live.sum(1)
    return dict(pos=pos, score=pos.sum(1) / length.double(), len=length.to(torch.int32), live=live, mem=mem, ls=ls, N=N)


def _c_sum(V, vec):
    """Additions on the longest path of the block-wide sum over a row of V elements read as 16-byte vectors of `vec` elements."""
    nvec = (V + vec - 1) // vec
    return 2 + vec * ((nvec + NT - 1) // NT) + BLOCK_SUM_ADDS


def score_bounds(r, dtype):
    """(bound of pos [B, T], bound of score [B]) for the sequence in the module docstring; `dtype` = the logits' storage type (it sets
    the vector width).  Pad positions and their sentences' empty sums demand exact results (0; NaN compares as bad in worst_ratio, so
    the callers compare NaN scores separately)."""
    u = U32
    vec = 8 if dtype == torch.bfloat16 else 4
    N, live = r["N"], r["live"].double()
    b_l = []
    for m in r["mem"]:
        V = m["x"].size(-1)
        a = (m["x"] - m["mx"].unsqueeze(-1)).abs()
        rel_se = u * (_c_sum(V, vec) + (m["w"] * (2 + 3 * a)).sum(-1)) + V * FLUSH
        b_lse = SLACK * (rel_se + 2 * u * m["se"].log().abs() + u * m["lse"].abs()) + ETA
        b_l.append(b_lse + u * m["l"].abs())
    b_l = torch.stack(b_l, 0)
    if N == 1:
        b_pos = b_l[0]
    else:
        # logsumexp is 1-Lipschitz with weights q_m: the members' errors enter as sum_m q_m b_l[m]; then the roundings of the
        # combination itself: the exponentials (their arguments' subtraction inside EXP), N - 1 additions, the logarithm, the sum with
        # M, fl(log N) and the final subtraction
        M = r["ls"].max(0).values
        a = (r["ls"] - M).abs()
        q = torch.softmax(r["ls"], 0)
        s = (r["ls"] - M).exp().sum(0)
        full = M + s.log()
        b_pos = SLACK * ((q * b_l).sum(0) + u * (q * (2 + 3 * a)).sum(0) + (N - 1) * u + N * FLUSH + 2 * u * s.log().abs()
                         + u * full.abs() + u * math.log(N) + u * (full - math.log(N)).abs()) + ETA
    b_pos = b_pos * live
    n = live.sum(1).clamp_min(1.0)
    b_score = SLACK * (b_pos.sum(1) / n + 2 * u * r["score"].abs().nan_to_num(0.0)) + ETA
    return b_pos, b_score


def score_check(pos, score, length, r, dtype):
    """((worst ratio, elements over the bound) of pos, the same of the scores of sentences with targets, whether len is exact and the
    sentences without targets score NaN)."""
    b_pos, b_score = score_bounds(r, dtype)
    has = r["len"] > 0
    score = score.double().cpu()
    exact = torch.equal(length.cpu().to(torch.int32), r["len"]) and bool(torch.isnan(score[~has]).all())
    return worst_ratio(pos.cpu(), r["pos"], b_pos), worst_ratio(score[has], r["score"][has], b_score[has]), exact


def score_inputs(B, T, V, N, dtype, pad=1, offsets=(0.0, 80.0, -80.0), seed=90):
    """N members' logits [B, T, V] in `dtype` and a target [B, T]: 2 N(0, 1) logits (lsce_logits' scale), member m offset by
    offsets[m % len(offsets)] (+80 and -80: the same softmax at another magnitude — only a maximum subtraction keeps the
    exponentials in range); right-padded targets with index 0 and V - 1 present, and — from three sentences on — sentence 1 fully
    padded."""
    g = torch.Generator().manual_seed(seed)
    xs = []
    for m in range(N):
        # (member 0: the logits the loss kernel's parity tests use)
        x = lsce_logits(B * T, V, torch.float32).view(B, T, V) if m == 0 else torch.randn(B, T, V, generator=g) * 2.0
        x = x + offsets[m % len(offsets)]
        xs.append(x.to(dtype))
    t = torch.randint(0, V, (B, T), generator=g)
    t[0, 0], t[-1, 0] = 0, V - 1
    if V > pad:
        t[t == pad] = 0  # (pad only where the layout below puts it)
        for b in range(B):
            keep = T if b == 0 else 1 + (b * 3) % max(T - 1, 1)  # (shorter than T wherever T > 1)
            t[b, keep:] = pad
        if B >= 3:
            t[1, :] = pad
    return xs, t


def score_emulate32(logits_list, target, pad, defect=None):
    """The kernel's formula in fp32 with plain torch operations (torch.exp / torch.log stand in for the device intrinsics), with one
    of SCORE_DEFECTS built in.  -> (pos, score, len)."""
    assert defect is None or defect in SCORE_DEFECTS
    N, (B, T) = len(logits_list), target.shape
    live = target.ne(pad)
    idx = target.clamp(0, logits_list[0].size(-1) - 1).unsqueeze(-1)
    ls = []
    for x in logits_list:
        x = x.float()
        mx = torch.zeros(B, T) if defect == "no_max_subtraction" else x.max(-1).values
        lse = mx + (x - mx.unsqueeze(-1)).exp().sum(-1).log()
        ls.append(x.gather(2, idx).squeeze(-1) - lse)
    ls = torch.stack(ls, 0)
    if N == 1:
        pos = ls[0]
    elif defect == "mean_of_logprobs":
        pos = ls.mean(0)
    else:
        M = ls.max(0).values
        pos = (M + (ls - M).exp().sum(0).log()) - torch.tensor(math.log(N), dtype=torch.float32)
    if defect != "pad_counted":
        pos = torch.where(live, pos, torch.zeros_like(pos))
    length = live.sum(1)
    den = torch.full((B,), float(T)) if defect == "divide_by_T" else length.float()
    return pos, pos.double().sum(1).float() / den, length.to(torch.int32)
