"""fp64 restatements, derived forward-error bounds and fp32 op-by-op emulations of the kernels in csrc/loss_optim.hip:
cst_adam_step, cst_sumsq, cst_ls_ce_fwd / cst_ls_ce_bwd.  Plain torch on the CPU; shared by test_loss_optim_ref_cpu.py (the bounds hold
for a faithful fp32 evaluation and reject every listed defect) and test_loss_optim_gpu.py (the kernels under the same bounds).

How the bounds are built.  Every fp32 operation of a kernel returns (x op y)(1 + d) + e with |d| <= u32 = 2^-24 and |e| <= 2^-150
(gradual underflow); a bf16 store rounds to nearest even, |d| <= ubf = 2^-8.  An error bound is then
    sum over the terms that are added of  c_term * u * |term|,
where c_term COUNTS the roundings that term passes through in the kernel's operation sequence (the count is written next to every
constant below).  The first-order sums are multiplied by SLACK = 1 + 2^-10 for the products of two roundings that a first-order count
leaves out (the largest count used here is below 2^7, so c*u < 2^-17 and the neglected part is below 2^-16 of the bound).
No constant here was fitted to an output of the kernels or of the emulations.

The scalar arguments travel through a C ABI as `float`: the references take lr, betas, eps and weight decay ROUNDED TO fp32 as the
exact inputs of the operation (the kernel never sees the double), and everything after that in fp64."""
import math

import torch

U32 = 2.0 ** -24      # unit roundoff of fp32 (24 significant bits)
UBF = 2.0 ** -8       # unit roundoff of a bf16 store (8 significant bits)
ETA = 2.0 ** -149     # one fp32 underflow (smallest subnormal; covers the 2^-150 of a rounded subnormal with margin)
FLUSH = 2.0 ** -126   # v_exp_f32 does not return subnormals: a result below the smallest normal may come back as 0
SLACK = 1.0 + 2.0 ** -10
NT = 256              # threads per workgroup of every kernel here

ADAM_DEFECTS = ("no_weight_decay", "eps_inside_sqrt", "no_bias_correction", "l2_decay")
LSCE_DEFECTS = ("no_smoothing", "target_coef_one", "pad_grad")


def f32(x):
    """The double value of x rounded to fp32 (what a `float` argument of the C ABI holds)."""
    return float(torch.tensor(float(x), dtype=torch.float32))


def _t(x):
    return torch.tensor(float(x), dtype=torch.float32)


def out_u(dtype):
    return UBF if dtype == torch.bfloat16 else 0.0


def worst_ratio(got, ref, bound):
    """(max over elements of |got - ref| / bound, number of elements over the bound).  A zero bound demands an exact result."""
    err = (got.double().reshape(-1) - ref.double().reshape(-1)).abs()
    bound = bound.double().reshape(-1).expand_as(err)
    bad = ~(err <= bound)  # NaN counts as bad
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return (float(ratio.max()) if err.numel() else 0.0), int(bad.sum())


# ------------------------------------------------------------------------------------------------------------------------------------
# Adam
# ------------------------------------------------------------------------------------------------------------------------------------
ADAM_BIG = 4 * 256 * 4096 + 4 * 256 + 3   # one full grid of float4 items, a second grid-stride iteration, and a scalar tail of 3
F, B = torch.float32, torch.bfloat16
# (n, grad dtype, param dtype, weight decay, step, grad_scale, small_v): a covering set — every n, every dtype pair, both wd, every
# step and both grad_scale forms appear, every dtype pair at the size of a real tensor; not the full product
ADAM_CASES = [
    (1, F, F, 0.01, 1, 0.25, False),
    (3, B, B, 0.0, 3, None, False),
    (4, F, B, 0.01, 150000, None, False),
    (1027, B, F, 0.01, 3, 0.25, False),
    (1027, F, F, 0.0, 150000, 0.25, False),
    (100003, F, F, 0.01, 3, 0.25, False),
    (100003, B, B, 0.01, 3, 0.25, False),
    (100003, F, B, 0.0, 1, None, False),
    (100003, B, F, 0.01, 150000, None, False),
    (100003, B, B, 0.01, 3, 0.25, True),      # v near eps^2: the regime in which "eps inside the square root" shows on every element
    (ADAM_BIG, B, B, 0.01, 3, 0.25, False),
    (ADAM_BIG, F, F, 0.0, 150000, None, False),
]
ADAM_HP = dict(lr=1e-3, b1=0.9, b2=0.98, eps=1e-8)


def adam_case_id(c):
    n, gdt, pdt, wd, step, gs, small = c
    nm = {F: "f32", B: "bf16"}
    return "n%d-g%s-p%s-wd%g-t%d-gs%s%s" % (n, nm[gdt], nm[pdt], wd, step, "none" if gs is None else "%g" % gs, "-smallv" if small else "")


def _randn(n, seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return torch.randn(n, generator=g)


def adam_inputs(n, gdt, small_v=False):
    """(master, m, v fp32; g in gdt) on the CPU.  small_v: second moments and gradients so small that sqrt(v') is of the size of eps."""
    master = _randn(n, 70)
    if small_v:
        return master, _randn(n, 71) * 1e-8, _randn(n, 72).abs() * 1e-16, (_randn(n, 73) * 4e-8).to(gdt)
    return master, _randn(n, 71) * 0.1, _randn(n, 72).abs() * 0.01, _randn(n, 73).to(gdt)


def adam_step_size64(lr, b1, b2, step):
    lr, b1, b2 = f32(lr), f32(b1), f32(b2)
    return lr * math.sqrt(1.0 - b2 ** step) / (1.0 - b1 ** step)


def adam_ref64(master, m, v, g, gs, lr, b1, b2, eps, wd, step):
    """The update of cst_adam_step in fp64: gradient scaled first, decoupled weight decay p -= wd*lr*p, bias corrections folded into
    step_size = lr * sqrt(1 - b2^t) / (1 - b1^t).  Returns a dict: master, m, v, and the terms the bounds are stated in."""
    lr, b1, b2, eps, wd = f32(lr), f32(b1), f32(b2), f32(eps), f32(wd)
    p, m, v = master.double(), m.double(), v.double()
    gg = g.double() * (1.0 if gs is None else float(gs))
    t_m, t_g = b1 * m, (1.0 - b1) * gg
    m1 = t_m + t_g
    t_v, t_gg = b2 * v, (1.0 - b2) * gg * gg
    v1 = t_v + t_gg
    decay = wd * lr * p
    step_size = adam_step_size64(lr, b1, b2, step)
    den = v1.sqrt() + eps
    delta = step_size * m1 / den
    return dict(master=p - decay - delta, m=m1, v=v1, p=p, decay=decay, delta=delta, den=den, step_size=step_size,
                t_m=t_m.abs(), t_g=t_g.abs(), t_v=t_v, t_gg=t_gg)


def adam_bounds(r, kg=1):
    """Per-element bounds (master, m, v) for the sequence of adam_one.  kg = roundings in the scaled gradient g*gs (1: the product).

    m' = fl(fl(m*b1) + fl(fl(1-b1)*g)):
        b1*m     : product, sum                                  -> 2
        (1-b1)*g : g (kg), fl(1-b1), product, sum                -> 3 + kg
      stated on |b1*m| + |(1-b1)*g|, not on |m'|: where the two cancel, the error relative to m' is unbounded.
    v' = fl(fl(v*b2) + fl(fl(fl(1-b2)*g)*g)):
        b2*v       : product, sum                                -> 2
        (1-b2)*g*g : g twice (2kg), fl(1-b2), two products, sum  -> 4 + 2kg
    master: p1 = fl(p - fl(fl(wd*lr)*p)),  p2 = fl(p1 - fl(fl(step_size*m') / fl(fl(sqrt(v')) + eps)))
        |p|       : rounding of p1, rounding of p2               -> 2
        |wd*lr*p| : fl(wd*lr), product, p1, p2                   -> 4
        delta     : error of m' times step_size/den, plus |delta| times
                    fl(step_size) 1, product 1, division 1, p2 1,
                    den: half the relative error of v' (square root), sqrt 1, sum with eps 1   -> 6 + rel(v')/2
    """
    u = U32
    bm = SLACK * u * (2 * r["t_m"] + (3 + kg) * r["t_g"]) + 2 * ETA
    bv = SLACK * u * (2 * r["t_v"] + (4 + 2 * kg) * r["t_gg"]) + 3 * ETA
    rel_v = torch.where(r["v"] > 0, bv / r["v"].clamp_min(1e-300), torch.zeros_like(bv))
    bp = SLACK * (u * (2 * r["p"].abs() + 4 * r["decay"].abs()) + (r["step_size"] / r["den"]) * bm
                  + r["delta"].abs() * (6 * u + 0.5 * rel_v)) + 4 * ETA
    return bp, bm, bv


def param_bound(r, bp, pdt):
    """The model parameter is the master stored in pdt: for bf16 one more rounding, of the COMPUTED master."""
    uo = out_u(pdt)
    return bp * (1.0 + uo) + uo * r["master"].abs()


def adam_emulate32(master, m, v, g, gs, lr, b1, b2, eps, wd, step, defect=None):
    """adam_one in fp32, one torch op per device operation (`fp contract(off)`: no product is fused into a sum)."""
    assert defect is None or defect in ADAM_DEFECTS
    lr_, b1_, b2_, eps_, wd_ = _t(lr), _t(b1), _t(b2), _t(eps), _t(wd)
    step_size = _t(adam_step_size64(lr, b1, b2, step))
    if defect == "no_bias_correction":
        step_size = lr_
    p, mi, vi = master.float().clone(), m.float().clone(), v.float().clone()
    gg = g.float() * _t(1.0 if gs is None else float(gs))
    if defect == "l2_decay":
        gg = gg + wd_ * p
    mi = mi * b1_ + (_t(1.0) - b1_) * gg
    vi = vi * b2_ + ((_t(1.0) - b2_) * gg) * gg
    if f32(wd) != 0.0 and defect not in ("no_weight_decay", "l2_decay"):
        p = p - (wd_ * lr_) * p
    den = (vi + eps_).sqrt() if defect == "eps_inside_sqrt" else vi.sqrt() + eps_
    p = p - (step_size * mi) / den
    return p, mi, vi


# ------------------------------------------------------------------------------------------------------------------------------------
# the block reduction both reductions share (block_sum in the source): 6 butterfly levels in a wave, then 4 waves added in order
# ------------------------------------------------------------------------------------------------------------------------------------
_LANE = torch.arange(64)


def _block_sum32(acc):
    """[..., 256] fp32 per-thread values -> [...] : wave_sum (v += shfl_xor(v, o), o = 32..1), then t = 0 + w0 + w1 + w2 + w3."""
    w = acc.reshape(*acc.shape[:-1], NT // 64, 64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[..., _LANE ^ o]
    w = w[..., 0]
    t = torch.zeros_like(w[..., 0])
    for k in range(NT // 64):
        t = t + w[..., k]
    return t


BLOCK_SUM_ADDS = 6 + 4


# ------------------------------------------------------------------------------------------------------------------------------------
# sumsq
# ------------------------------------------------------------------------------------------------------------------------------------
SUMSQ_BIG = 8 * 256 * 2048 * 2 + 8 * 256 * 3 + 5   # two full grids of 8-element items, a partial third, and a tail of 5 for block 0
SUMSQ_SIZES = [1, 7, 8, 2055, 100003, SUMSQ_BIG]


def sumsq_inputs(n, dt):
    """The last element is 64: a tail that is dropped (or read twice) moves the sum by far more than the bound at every size."""
    x = _randn(n, 80)
    x[-1] = 64.0
    return x.to(dt)


def sumsq_ref64(x):
    return (x.double() ** 2).sum()


def _sumsq_grid(n):
    blocks = min((n + NT * 8 - 1) // (NT * 8), 2048)
    nth = blocks * NT
    n8 = n // 8
    return blocks, nth, n8, (n8 + nth - 1) // nth


def sumsq_chain(n):
    """Roundings on the longest path from one x*x to out[0]:
    the square 1, the thread's additions 8 * (grid-stride iterations), one tail element 1, block_sum 10, the final kernel's per-thread
    additions ceil(blocks / 256), its block_sum 10, out[0] += acc 1."""
    blocks, _, _, iters = _sumsq_grid(n)
    return 1 + 8 * iters + 1 + BLOCK_SUM_ADDS + (blocks + NT - 1) // NT + BLOCK_SUM_ADDS + 1


def sumsq_bound(ref, n, extra=0):
    """All terms are squares: the error is relative to the sum.  `extra`: further additions of non-negative terms by the caller."""
    return SLACK * (sumsq_chain(n) + extra) * U32 * abs(float(ref)) + ETA * n


def sumsq_emulate32(x, out0=0.0):
    """sumsq_kernel + sumsq_final_kernel, thread by thread, every square and sum rounded to fp32 on its own."""
    n = x.numel()
    xf = x.float().reshape(-1)
    blocks, nth, n8, iters = _sumsq_grid(n)
    acc = torch.zeros(nth, dtype=torch.float32)
    if iters:
        body = torch.zeros(iters * nth * 8, dtype=torch.float32)  # (zero padding: 0*0 and acc + 0 are exact)
        body[:n8 * 8] = xf[:n8 * 8]
        body = body.view(iters, nth, 8)
        for it in range(iters):
            for e in range(8):
                acc = acc + body[it, :, e] * body[it, :, e]
    tail = xf[n8 * 8:]
    if tail.numel():
        acc = acc.clone()
        acc[:tail.numel()] = acc[:tail.numel()] + tail * tail
    part = _block_sum32(acc.view(blocks, NT))
    steps = (blocks + NT - 1) // NT
    pp = torch.zeros(steps * NT, dtype=torch.float32)
    pp[:blocks] = part
    pp = pp.view(steps, NT)
    acc2 = torch.zeros(NT, dtype=torch.float32)
    for s in range(steps):
        acc2 = acc2 + pp[s]
    return _t(out0) + _block_sum32(acc2)


# ------------------------------------------------------------------------------------------------------------------------------------
# label-smoothed cross entropy
# ------------------------------------------------------------------------------------------------------------------------------------
LSCE_SHAPES = [(1, 1), (5, 255), (37, 257), (33, 10001)]   # below / above one pass of the 256 threads, odd V, V of a real vocabulary
LSCE_EPS, LSCE_PAD, LSCE_G = 0.1, 1, 0.37
LSCE_SHIFT = {F: 80.0, B: 60.0}


def lsce_targets(rows, V):
    """Index 0 in the first row, V-1 in the last, the pad index in every fifth row from row 2 (and wherever the draw gives it)."""
    t = torch.randint(0, V, (rows,), generator=torch.Generator().manual_seed(61))
    if V > LSCE_PAD:
        t[2::5] = LSCE_PAD
    t[-1] = V - 1
    t[0] = 0
    return t


def lsce_logits(rows, V, dt, kind="plain"):
    """plain: 2 * N(0, 1).  shift: (unshifted, shifted) with shifted = unshifted + LSCE_SHIFT[dt] EXACTLY (the shifted tensor is drawn
    and rounded first; subtracting the shift from it is exact in both dtypes), so both describe the same softmax.
    peaked: in every non-pad row one logit is raised, by 40 in even rows (p elsewhere ~ 1e-18) and by 100 in odd rows (the fp32
    exponential underflows to zero elsewhere)."""
    g = torch.Generator(device="cpu")
    g.manual_seed(60)
    base = torch.randn(rows, V, generator=g) * 2.0
    if kind == "plain":
        return base.to(dt)
    if kind == "shift":
        s = LSCE_SHIFT[dt]
        hi = (base + s).to(dt)
        lo = (hi.float() - s).to(dt)
        assert torch.equal(lo.double() + s, hi.double())
        return lo, hi
    assert kind == "peaked"
    x = base.clone()
    for r in range(rows):
        x[r, (7 * r + 3) % V] += 40.0 if r % 2 == 0 else 100.0
    return x.to(dt)


def _c_sum(V):
    """Additions on the longest path of a block-wide sum over V: the thread's ceil(V / 256) terms, then block_sum."""
    return (V + NT - 1) // NT + BLOCK_SUM_ADDS


def lsce_ref64(logits, target, eps, pad, gscale=1.0):
    """loss = sum over non-pad rows of (1-eps) * nll_row + (eps/V) * sum_v (lse - x_v), nll_row = lse - x_t;
    dlogits = g * (softmax - (1-eps) * onehot(t) - eps/V), zero in pad rows.  eps and gscale as their fp32 values, all else fp64."""
    eps, g = f32(eps), f32(gscale)
    x = logits.double()
    rows, V = x.shape
    mx = x.max(1).values
    se = (x - mx[:, None]).exp().sum(1)
    lse = mx + se.log()
    live = target.ne(pad)
    xt = x.gather(1, target[:, None]).squeeze(1)
    nll_row = torch.where(live, lse - xt, torch.zeros_like(lse))
    smooth = V * lse - x.sum(1)
    loss_row = torch.where(live, (1.0 - eps) * (lse - xt) + (eps / V) * smooth, torch.zeros_like(lse))
    p = (x - lse[:, None]).exp()
    onehot = torch.zeros_like(x).scatter_(1, target[:, None], 1.0)
    d = g * (p - (1.0 - eps) * onehot - eps / V) * live[:, None].double()
    return dict(loss=loss_row.sum(), nll=nll_row.sum(), lse=lse, dlogits=d, x=x, mx=mx, se=se, p=p, live=live, onehot=onehot,
                nll_row=nll_row, smooth=smooth, loss_row=loss_row, eps=eps, g=g, V=V)


def lsce_bounds(r, out_dtype):
    """Bounds for lse [rows], loss, nll (scalars) and dlogits [rows, V].

    __expf(a) is v_exp_f32(fl(log2e_f32 * a)): the argument of the base-2 exponential carries the rounding of log2e and of the product,
    and a itself the rounding of the subtraction that formed it — three relative errors of the ARGUMENT, i.e. 3*|a|*u relative in the
    result; v_exp_f32 is specified to 1 ulp <= 2u.  EXP(a) = 2 + 3|a| in units of u32.   __logf is the accurate logf, 1 ulp <= 2u.
      se  = sum_v __expf(x_v - mx): positive terms, relative error  c_sum(V) + sum_v p_v EXP(x_v - mx);  a term below 2^-126 may be flushed
      lse = fl(mx + __logf(se)):    rel(se)  +  2u |log se|  +  u |lse|
      row:  nll = fl(lse - x_t) 1;  sx = sum_v x_v: c_sum(V) * u * sum|x_v|;  fl(V*lse) 1;  smooth = fl(V*lse - sx) 1;
            l = fl(fl(fl(1-eps)*nll) + fl(fl(eps/V)*smooth)): 2 per product, 1 for the sum
      loss, nll: the rows are added in double; one rounding to fp32 at the end
      dlogits_v = out(fl(g * t)),  t = fl(fl(__expf(fl(x_v - lse')) - ev) - [v == target] fl(1-eps)),  ev = fl(eps/V), lse' the kernel's lse:
            p_v * (bound(lse) + EXP(x_v - lse) u)      the exponential
            u (|p_v - ev| + ev)                         the subtraction of ev and the rounding of ev
            u (|t| + (1-eps))  at the target entry      the cancellation there: both of size u, times g
            u |d|                                       the product with g — for an fp32 output this is the store
            ubf |d|                                     a bf16 store
    """
    u = U32
    x, V, eps, g = r["x"], r["V"], r["eps"], abs(r["g"])
    cs = _c_sum(V)
    a_mx = (x - r["mx"][:, None]).abs()
    w = (x - r["mx"][:, None]).exp() / r["se"][:, None]
    rel_se = u * (cs + (w * (2 + 3 * a_mx)).sum(1)) + V * FLUSH
    b_lse = SLACK * (rel_se + 2 * u * r["se"].log().abs() + u * r["lse"].abs()) + ETA
    live = r["live"].double()
    nll_row = r["nll_row"].abs()
    b_nll_row = (b_lse + u * nll_row) * live
    b_smooth = V * b_lse + u * (V * r["lse"]).abs() + cs * u * x.abs().sum(1) + u * r["smooth"].abs()
    t1, t2 = (1.0 - eps) * nll_row, (eps / V) * r["smooth"].abs()
    b_row = ((1.0 - eps) * (b_nll_row + 2 * u * nll_row) + (eps / V) * (b_smooth + 2 * u * r["smooth"].abs()) + u * (t1 + t2)) * live
    b_loss = SLACK * (float(b_row.sum()) + u * abs(float(r["loss"]))) + ETA
    b_nll = SLACK * (float(b_nll_row.sum()) + u * abs(float(r["nll"]))) + ETA
    ev = eps / V
    p = r["p"]
    a_l = (x - r["lse"][:, None]).abs()
    t = p - ev - (1.0 - eps) * r["onehot"]
    et = p * (b_lse[:, None] + u * (2 + 3 * a_l)) + FLUSH + u * ((p - ev).abs() + ev) + r["onehot"] * u * (t.abs() + (1.0 - eps))
    uo = out_u(out_dtype)
    d = r["dlogits"].abs()
    b_d = (SLACK * (g * et + u * d) * (1.0 + uo) + uo * d + ETA) * live[:, None]
    return dict(lse=b_lse, loss=b_loss, nll=b_nll, dlogits=b_d)


def lsce_emulate32(logits, target, eps, pad, gscale=1.0, defect=None):
    """ls_ce_fwd_kernel + sum_pairs_kernel + ls_ce_bwd_kernel in fp32, thread by thread; torch.exp / torch.log stand in for the device
    intrinsics (whose own error the bounds carry).  Returns loss, nll (fp32 scalars), lse fp32 [rows], dlogits in the logits' dtype."""
    assert defect is None or defect in LSCE_DEFECTS
    x = logits.float()
    rows, V = x.shape
    steps = (V + NT - 1) // NT
    mx = x.max(1).values
    xp = torch.zeros(rows, steps * NT, dtype=torch.float32)
    ep = torch.zeros(rows, steps * NT, dtype=torch.float32)
    xp[:, :V] = x
    ep[:, :V] = (x - mx[:, None]).exp()
    xp, ep = xp.view(rows, steps, NT), ep.view(rows, steps, NT)
    se_t, sx_t = torch.zeros(rows, NT), torch.zeros(rows, NT)
    for s in range(steps):
        se_t = se_t + ep[:, s]
        sx_t = sx_t + xp[:, s]
    se, sx = _block_sum32(se_t), _block_sum32(sx_t)
    lse = mx + se.log()
    eps_, one = _t(eps), _t(1.0)
    live = target.ne(pad)
    nll_row = lse - x.gather(1, target[:, None]).squeeze(1)
    smooth = _t(V) * lse - sx
    coef = one if defect == "target_coef_one" else one - eps_
    l_row = coef * nll_row if defect == "no_smoothing" else coef * nll_row + (eps_ / _t(V)) * smooth
    if defect != "pad_grad":
        l_row, nll_row = torch.where(live, l_row, torch.zeros_like(l_row)), torch.where(live, nll_row, torch.zeros_like(nll_row))
    loss, nll = l_row.double().sum().float(), nll_row.double().sum().float()
    ev = _t(0.0) if defect == "no_smoothing" else eps_ / _t(V)
    p = (x - lse[:, None]).exp() - ev
    rr = torch.arange(rows)
    p[rr, target] = p[rr, target] - coef
    g = torch.full((rows,), f32(gscale), dtype=torch.float32)
    if defect != "pad_grad":
        g = torch.where(live, g, torch.zeros_like(g))
    return loss, nll, lse, (g[:, None] * p).to(logits.dtype)
