"""fp64 restatements, derived forward-error bounds and fp32 op-by-op emulations of the normalisation kernels in csrc/layernorm.hip and
csrc/ln_gelu.hip: cst_layernorm_fwd / _bwd, cst_ln_gelu_fwd / _bwd, cst_conv0_ln_gelu_fwd / _bwd.  Plain torch on the CPU; shared by
test_norm_ref_cpu.py (the bounds hold for a faithful fp32 evaluation and reject every listed defect) and test_norm_gpu.py (the kernels
under the same bounds).  Built like loss_optim_ref.py, whose U32, UBF, SLACK and worst_ratio are used here.

How the bounds are built.  Every fp32 operation returns (x op y)(1 + d), |d| <= u32; a bf16 store adds |d| <= ubf.  A bound is
    sum over the terms that are added of  c_term * u32 * |term|   (+ the propagated bounds of the inputs times their condition terms),
and c_term COUNTS the roundings the term passes through in the kernel's operation sequence.  The counts that recur:
    C_ROW(cols) = 8 NV + 6   a row sum: a lane adds its 8 NV elements in a chain (NV = 1, 2, 4 vectors of 8 for cols <= 512, <= 1024,
                             <= 2048), then wave_sum adds across the 64 lanes in 6 butterfly levels
    kdiv                     turning the sum into a mean: 1 in layernorm.hip (a division by (float)cols), 2 in ln_gelu.hip (fl(1 / C),
                             then a product)
    BLOCK = 4                the four waves of a block, added in wave order
    column sums over rows    (a wave's chain over its grid-stride iterations) + BLOCK + (the reduce kernel's chain, *_red_chain below)
    device intrinsics        rsqrtf, __expf, __frcp_rn: 2 roundings each
An fmaf (written in ln_gelu.hip, or contracted by the compiler in layernorm.hip) rounds once where the count below assumes a product
and a sum: the count is an upper bound for either code.  The bound of a sum is stated in the sum of the ABSOLUTE terms, never in the
result.  First-order sums are multiplied by SLACK.  No constant here was fitted to an output of a kernel or of an emulation.

Two constants cannot be counted: the absolute errors of the GELU approximations, taken from csrc/cst_common.h (A_GELU, A_DGELU; the
CPU test checks the fp32 restatements of the formulas against them on a grid over [-6, 6]).  Outside [-6, 6]:
    erf forms       the tail term P(t) E is below 6 * 1e-9: the result is x (or 0, or 1) to that; the constant holds everywhere
    bf16 GELU       the argument is clamped to |x| <= 4: gelu_poly(x) = x c4 with |c4 - Phi(4)| <= A / 4 (from the error at 4), and
                    Phi(x) - Phi(4) <= 3.2e-5: error <= |x| (A / 4 + 3.2e-5)
    bf16 GELU'      constant beyond 4, while GELU' moves from 1.000503 to 1: error <= A' + 5.1e-4

Inputs (norm_rows): rows of six kinds in ONE tensor, by row index modulo 8 — see KINDS."""
import functools
import math

import torch

from loss_optim_ref import ETA, SLACK, U32, UBF, f32, out_u, worst_ratio  # noqa: F401  (worst_ratio: re-exported to the tests)

F, B = torch.float32, torch.bfloat16
NAME = {F: "f32", B: "bf16"}
WAVES = 4                     # rows per block iteration in every row kernel
BLOCK = 4                     # additions of the block partial
LN_FWD_CAP, LN_BWD_CAP = 2048, 1024      # ln_blocks(rows, 2048) in cst_layernorm_fwd, LN_BWD_BLOCKS
LG_FWD_CAP, LG_BWD_CAP = 4096, 1024      # LG_FWD_BLOCKS, LG_BWD_BLOCKS
C0_BWD_TB = 2048                         # frames per backward block of layer 0
INTRIN = 2                    # roundings counted for one device intrinsic

# absolute errors of the GELU approximations of csrc/cst_common.h: TWICE the worst error measured on an MI355X through cst_act_fwd /
# cst_act_bwd against fp64 (the factor covers the grid spacing); test_norm_gpu.py::test_gelu_on_the_device repeats the measurement
#   erf forms, 2.4 M fp32 points over [-6, 6]:  GELU 3.317e-7 (at 3.0956), GELU' 3.020e-7 (at 0.0491)
#   polynomials: the stored bf16 result equals the rounded fp32 restatement below on every one of the 33152 bf16 arguments in [-6, 6],
#   so the restatement is the device function; on 1.2 M fp32 arguments it errs by 3.3016e-4 (GELU, at -3.9104) and 3.1031e-4 (GELU')
A_GELU = {F: 6.64e-7, B: 6.61e-4}
A_DGELU = {F: 6.05e-7, B: 6.21e-4}
# the erf forms feed two intrinsics (__frcp_rn, __expf) into a tail term of size <= 0.17 (GELU: max x (1 - Phi(x))) / <= 0.5 (the cdf
# half of GELU'), and __expf into the density term |x| phi(x) <= 0.25
I_GELU = {F: 2 * INTRIN * U32 * 0.17, B: 0.0}
I_DGELU = {F: 2 * INTRIN * U32 * 0.5 + INTRIN * U32 * 0.25, B: 0.0}

LN_FWD_DEFECTS = ("eps_outside_sqrt", "unbiased_variance", "one_pass_variance", "stats_of_rounded_sum", "residual_missing_from_sum_out")
LN_BWD_DEFECTS = ("no_xhat_term", "no_mean_term", "dres_not_added", "dgamma_from_g", "last_row_dropped", "second_stride_iteration_dropped")
LG_FWD_DEFECTS = ("eps_outside_sqrt", "unbiased_variance", "one_pass_variance", "limit_row_not_zeroed")
LG_BWD_DEFECTS = ("no_xhat_term", "no_mean_term", "dgamma_from_g", "last_row_dropped", "second_stride_iteration_dropped",
                  "gelu_prime_is_cdf", "limit_row_not_zeroed")
C0_DEFECTS = ("bias_missing", "tap_k_minus_1_dropped", "dbias_from_dz")

_LANE = torch.arange(64)


def nv_of(cols):
    return 1 if cols <= 512 else (2 if cols <= 1024 else 4)


def c_row(cols):
    """Roundings on the longest path of one row sum: the lane's chain of 8 NV additions, then 6 butterfly levels."""
    return 8 * nv_of(cols) + 6


def blocks_of(rows, cap):
    return min((rows + WAVES - 1) // WAVES, cap)


def ln_red_chain(nb):
    """ln_bwd_reduce_kernel: 64 row groups, group g adds partials g, g + 64, ... (ceil(nb / 64) additions), then group 0 adds the other
    groups' sums in order (an empty group adds an exact zero: min(nb, 64) - 1 additions that round)."""
    return (nb + 63) // 64 + min(nb, 64) - 1


def lg_red_chain(n):
    """lg_reduce_kernel: four interleaved chains of ceil(n / 4) additions, then (a0 + a1) + (a2 + a3): 2 more."""
    return (n + 3) // 4 + 2


def ln_bwd_chain(rows):
    nb = blocks_of(rows, LN_BWD_CAP)
    return (rows + WAVES * nb - 1) // (WAVES * nb) + BLOCK + ln_red_chain(nb)


def lg_bwd_chain(rows):
    nb = blocks_of(rows, LG_BWD_CAP)
    return (rows + WAVES * nb - 1) // (WAVES * nb) + BLOCK + lg_red_chain(nb)


def c0_bwd_chain(Bn, L):
    nblk = (L + C0_BWD_TB - 1) // C0_BWD_TB
    return (min(L, C0_BWD_TB) + WAVES - 1) // WAVES + BLOCK + lg_red_chain(Bn * nblk)


# ------------------------------------------------------------------------------------------------------------------------------------
# GELU: fp64, and the kernels' formulas restated in fp32 from csrc/cst_common.h
# ------------------------------------------------------------------------------------------------------------------------------------
def pdf64(z):
    return torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def gelu64(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def dgelu64(z):
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * pdf64(z)


def d2gelu64(z):
    return pdf64(z) * (2.0 - z * z)


D3GELU_MAX = 1.0   # |GELU'''| = phi(z) |z^3 - 4 z| <= 0.78


def _c(x):
    return torch.tensor(x, dtype=F)


def _fma(a, b, c):
    """fmaf: one rounding (the fp64 product of two fp32 values is exact; the double rounding of the sum is immaterial to the bounds)."""
    a, b, c = (t if torch.is_tensor(t) else _c(t) for t in (a, b, c))
    return (a.double() * b.double() + c.double()).float()


def _gelu_tail32(x):
    u = x.abs() * _c(0.70710678118654752)
    t = _c(1.0) / _fma(0.3275911, u, 1.0)
    E = torch.exp((_c(-0.5) * x) * x)
    pl = _fma(1.061405429, t, -1.453152027)
    pl = _fma(pl, t, 1.421413741)
    pl = _fma(pl, t, -0.284496736)
    pl = _fma(pl, t, 0.254829592)
    return pl * t * E, E


def gelu_erf32(x):
    q = _c(0.5) * x * _gelu_tail32(x)[0]
    return torch.where(x >= 0, x - q, q)


def dgelu_erf32(x, defect=None):
    tail, E = _gelu_tail32(x)
    q = _c(0.5) * tail
    cdf = torch.where(x >= 0, _c(1.0) - q, q)
    return cdf if defect == "gelu_prime_is_cdf" else _fma(x * _c(0.39894228040143268), E, cdf)


def _poly32(t, coef):
    p = _fma(coef[0], t, coef[1])
    for c in coef[2:]:
        p = _fma(p, t, c)
    return p


_P13 = (2.6867663649454698e-08, -1.824730247790285e-06, 5.28495256730821e-05, -0.0008661365136504173, 0.009053179994225502,
        -0.06526926904916763, 0.39845922589302063)
_Q15 = (-1.5577683143419563e-08, 1.1633505891950335e-06, -3.7250658351695165e-05, 0.0006728997686877847, -0.0075911665335297585,
        0.0555923730134964, -0.26155415177345276, 0.7965189218521118)


def gelu_poly32(x):
    xc = x.clamp(-4.0, 4.0)
    return x * _fma(_poly32(xc * xc, _P13), xc, 0.5)


def dgelu_poly32(x, defect=None):
    xc = x.clamp(-4.0, 4.0)
    if defect == "gelu_prime_is_cdf":   # the cdf half alone, in the same polynomial form
        return _fma(_poly32(xc * xc, _P13), xc, 0.5)
    return _fma(_poly32(xc * xc, _Q15), xc, 0.5)


def gelu32(x, dt):
    return gelu_poly32(x) if dt == B else gelu_erf32(x)


def dgelu32(x, dt, defect=None):
    return dgelu_poly32(x, defect) if dt == B else dgelu_erf32(x, defect)


def a_gelu(z, dt):
    """Absolute error allowed to the kernel's GELU at the exact argument z (module docstring)."""
    a = A_GELU[dt] + I_GELU[dt]
    if dt == B:
        return torch.where(z.abs() <= 6.0, torch.full_like(z, a), z.abs() * (a / 4.0 + 3.2e-5))
    return torch.full_like(z, a)


def a_dgelu(z, dt):
    a = A_DGELU[dt] + I_DGELU[dt]
    if dt == B:
        return torch.where(z.abs() <= 6.0, torch.full_like(z, a), torch.full_like(z, a + 5.1e-4))
    return torch.full_like(z, a)


# ------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------------
# row r is of kind KINDS[r % 8]
KINDS = ("const", "spike", "randn", "offset", "tiny", "randn", "randn", "dy0")
CONST, SPIKE, OFFSET, TINY, DY0 = 0, 1, 3, 4, 7


def _gen(seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return g


def kind_of(rows):
    return torch.arange(rows) % 8


def is_plain(kd):
    return (kd == 2) | (kd == 5) | (kd == 6)


def norm_rows(rows, cols, dt, seed=11, with_res=False):
    """[rows, cols] in dt (and a residual of the same shape).  By row index modulo 8:
      0        a constant row: variance exactly 0, rstd = eps^-1/2, y = beta
      1        N(0, 1) with one element 1e4
      2, 5, 6  N(0, 1)
      3        mean 100, standard deviation 0.1: x - mean cancels 10 bits (one_pass_variance)
      4        standard deviation 3e-3: the variance is of the size of eps (eps_outside_sqrt)
      7        N(0, 1); the backward tests give this row dy = 0 exactly
    (the last row of every shape used, and the last row below every limit, is of kind 2, 4, 5 or 6: last_row_dropped drops a row whose
    terms are of ordinary size)
    The residual is 0.3 N(0, 1) scaled like its row (a constant 0.25 in the constant row), so x + res is of the same kind."""
    g = _gen(seed)
    x = torch.randn(rows, cols, generator=g)
    r = 0.3 * torch.randn(rows, cols, generator=g)
    kd = kind_of(rows)
    x[kd == OFFSET] = 100.0 + 0.1 * x[kd == OFFSET]
    r[kd == OFFSET] *= 0.1
    x[kd == TINY] *= 3e-3
    r[kd == TINY] *= 3e-3
    x[kd == CONST] = 0.75
    r[kd == CONST] = 0.25
    sp = torch.nonzero(kd == SPIKE).reshape(-1)
    x[sp, (5 * sp + 1) % cols] = 1e4
    return (x.to(dt), r.to(dt)) if with_res else x.to(dt)


def norm_dy(rows, cols, dt, seed=12):
    g = _gen(seed)
    dy = torch.randn(rows, cols, generator=g)
    dres = torch.randn(rows, cols, generator=g)
    dy[kind_of(rows) == DY0] = 0.0
    return dy.to(dt), dres.to(dt)


def norm_params(cols, dt, seed=13):
    """gamma of both signs with exact zeros (every 7th from 3), beta 0.1 N(0, 1)."""
    g = _gen(seed)
    gamma = 0.3 + torch.randn(cols, generator=g)
    beta = 0.1 * torch.randn(cols, generator=g)
    gamma[3::7] = 0.0
    return gamma.to(dt), beta.to(dt)


def conv0_inputs(Bn, S, C, k, dt, seed=14):
    """Raw samples [Bn, S] fp32 in segments of 64 samples, by segment index modulo 8 as KINDS: exactly zero (the frame is the bias: the
    smallest variance a frame can have here), 0.1 N with one sample 1e4, 0.1 N(0, 1), 100 + 0.1 N, 3e-3 N, 0.1 N (three).  The frame
    statistics follow from the convolution; a constant frame over the channels cannot be made from the samples.
    w [C, k] 0.5 N, bias 0.25 + 0.1 N."""
    g = _gen(seed)
    wav = 0.1 * torch.randn(Bn, S, generator=g)
    seg = (torch.arange(S) // 64) % 8
    wav[:, seg == OFFSET] = 100.0 + wav[:, seg == OFFSET]
    wav[:, seg == TINY] *= 3e-2
    wav[:, seg == CONST] = 0.0
    first = torch.nonzero((seg == SPIKE) & (torch.arange(S) % 64 == 17)).reshape(-1)
    wav[:, first] = 1e4
    w = (0.5 * torch.randn(C, k, generator=g)).to(dt)
    bias = (0.25 + 0.1 * torch.randn(C, generator=g)).to(dt)
    return wav, w, bias


# ------------------------------------------------------------------------------------------------------------------------------------
# shared pieces of the bounds
# ------------------------------------------------------------------------------------------------------------------------------------
def _stats64(v, eps):
    mean = v.mean(1)
    D = v - mean[:, None]
    var = (D * D).mean(1)
    return mean, D, var, (var + eps) ** -0.5


def _stat_bounds(v, ev, mean, D, var, rstd, eps, kdiv):
    """Bounds of the kernel's mean and rstd [rows].  v: the exact values the statistics are defined on; ev >= |kernel's fp32 v - v|.
      mean = fl(sum / C):     every term carries ev and the C_ROW roundings of the sum; the mean itself kdiv
      d_j = fl(v_j - mean):   ev, the subtraction 1 (relative to |D_j|), and the error of the mean, which is SHARED by all j:
                              sum_j D_j = 0, so it enters q = sum d_j^2 only in second order — written out as a square, not dropped
      q / C:                  per term 2 |D_j| e_j, the square 1, the sum C_ROW, the mean kdiv
      t = fl(q / C + eps) 1;  rstd = rsqrtf(t): half the relative error of t (its exact form (1 - r)^-1/2 - 1), the intrinsic 2."""
    u, cr = U32, c_row(v.shape[1])
    b_mean = SLACK * (ev.mean(1) + u * (cr * v.abs().mean(1) + kdiv * mean.abs())) + ETA
    ed = ev + u * D.abs()
    t = var + eps
    b_t = SLACK * ((2.0 * D.abs() * ed).mean(1) + u * (1 + cr + kdiv) * var + u * t) + (b_mean + ed.max(1).values) ** 2 + ETA
    rel = (1.0 - (b_t / t).clamp_max(0.5)) ** -0.5 - 1.0
    b_rstd = SLACK * rstd * (rel + INTRIN * u)
    return b_mean, b_rstd


def _affine_bound(D, ev, b_mean, rstd, b_rstd, gamma, z):
    """z = fl(fl(fl(fl(v - mean) * rstd) * gamma) + beta): the errors of v and mean times rstd |gamma|, that of rstd times |D gamma|,
    subtraction + two products = 3 on |xhat gamma|, the sum 1 on |z|."""
    ga = gamma.abs()[None]
    return SLACK * (ga * rstd[:, None] * (ev + b_mean[:, None]) + D.abs() * ga * b_rstd[:, None]
                    + U32 * (3.0 * (D * rstd[:, None]).abs() * ga + z.abs())) + ETA


def _gelu_arg_bound(z, b_z, dt):
    """GELU(z') against GELU(z), |z' - z| <= b_z, BEFORE any store: (|GELU'(z)| + max|GELU''| b_z) b_z and the approximation."""
    return (dgelu64(z).abs() + 0.8 * b_z) * b_z + a_gelu(z, dt)


def _gelu_out_bound(z, b_z, dt):
    """_gelu_arg_bound and the bf16 store."""
    y = gelu64(z)
    b = _gelu_arg_bound(z, b_z, dt)
    uo = out_u(dt)
    return b * (1.0 + uo) + uo * y.abs() + ETA


def _dx_bound(g, b_g, xh, b_xh, rstd, kdiv):
    """rstd * (g - s1 - xhat s2), s1 = mean(g), s2 = mean(g xhat), before any store.  b_g, b_xh: bounds of the kernel's g and xhat.
      s1: b_g, the row sum C_ROW, the mean kdiv                        s2: b_g |xhat| + |g| b_xh, the product 1, C_ROW, kdiv
      g - s1 - xhat s2, times rstd: every one of the three terms passes two subtractions (or the product and one) and the product with
      rstd: 3 each; xhat s2 carries b_xh again because the kernel forms xhat a second time."""
    u, cr = U32, c_row(g.shape[1])
    s1, s2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    b_s1 = b_g.mean(1, keepdim=True) + u * (cr + kdiv) * g.abs().mean(1, keepdim=True)
    b_s2 = (b_g * xh.abs() + g.abs() * b_xh).mean(1, keepdim=True) + u * (1 + cr + kdiv) * (g * xh).abs().mean(1, keepdim=True)
    r = rstd[:, None]
    return SLACK * r * (b_g + b_s1 + xh.abs() * b_s2 + s2.abs() * b_xh + 3.0 * u * (g.abs() + s1.abs() + (xh * s2).abs())) + ETA


def _colsum_bound(terms_abs, b_terms, chain):
    """A column sum over rows: the bounds of the terms, and `chain` roundings on the sum of the ABSOLUTE terms."""
    return SLACK * (b_terms.sum(0) + chain * U32 * terms_abs.sum(0)) + ETA * terms_abs.shape[0]


def _store(b, val, dt):
    uo = out_u(dt)
    return b * (1.0 + uo) + uo * val.abs()


# ------------------------------------------------------------------------------------------------------------------------------------
# the kernels' summation shapes, in fp32
# ------------------------------------------------------------------------------------------------------------------------------------
def _wave_sum32(a, b=None, fma=False):
    """Row sums of a (or of a * b) [rows, cols] as one wave forms them: lane l holds the vectors l, l + 64, ... of 8 elements and adds
    them in order (`fma`: s = fmaf(a, b, s)), then v += shfl_xor(v, o), o = 32 .. 1."""
    rows, cols = a.shape
    nv = nv_of(cols)

    def lay(t):
        p = torch.zeros(rows, nv * 512, dtype=F)
        p[:, :cols] = t
        return p.view(rows, nv, 64, 8)
    pa, pb = lay(a), (lay(b) if b is not None else None)
    s = torch.zeros(rows, 64, dtype=F)
    for i in range(nv):
        for e in range(8):
            if pb is None:
                s = s + pa[:, i, :, e]
            elif fma:
                s = _fma(pa[:, i, :, e], pb[:, i, :, e], s)
            else:
                s = s + pa[:, i, :, e] * pb[:, i, :, e]
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, _LANE ^ o]
    return s[:, 0]


def _grid_slots(rows, cap):
    """(slot, iteration) of every row in a grid-stride row kernel: slot = block * 4 + wave."""
    n = blocks_of(rows, cap) * WAVES
    r = torch.arange(rows)
    return r % n, r // n, n


def _col_accum32(a, b, slot, it, nslots, fma=False, skip_it=None, keep=None):
    """Per-wave accumulators over the rows of a slot in iteration order (acc += a [* b], or fmaf), then the block partial
    0 + w0 + w1 + w2 + w3.  -> [nslots / 4, cols].  skip_it: an iteration that is left out (a defect); keep: rows that take part."""
    cols = a.shape[1]
    acc = torch.zeros(nslots, cols, dtype=F)
    for i in range(int(it.max()) + 1 if it.numel() else 0):
        if i == skip_it:
            continue
        sel = it == i
        if keep is not None:
            sel = sel & keep
        if not bool(sel.any()):
            continue
        sl = slot[sel]
        if b is None:
            acc[sl] = acc[sl] + a[sel]
        elif fma:
            acc[sl] = _fma(a[sel], b[sel], acc[sl])
        else:
            acc[sl] = acc[sl] + a[sel] * b[sel]
    w = acc.view(nslots // WAVES, WAVES, cols)
    p = torch.zeros(nslots // WAVES, cols, dtype=F)
    for k in range(WAVES):
        p = p + w[:, k]
    return p


def _ln_reduce32(part):
    """ln_bwd_reduce_kernel over [nb, cols]."""
    nb, cols = part.shape
    steps = (nb + 63) // 64
    pp = torch.zeros(steps * 64, cols, dtype=F)
    pp[:nb] = part
    pp = pp.view(steps, 64, cols)
    grp = torch.zeros(64, cols, dtype=F)
    for s in range(steps):
        grp = grp + pp[s]
    a = grp[0]
    for k in range(1, 64):
        a = a + grp[k]
    return a


def _lg_reduce32(part):
    """lg_reduce_kernel over [n, cols]."""
    n, cols = part.shape
    steps = (n + 3) // 4
    pp = torch.zeros(steps * 4, cols, dtype=F)
    pp[:n] = part
    pp = pp.view(steps, 4, cols)
    a = torch.zeros(4, cols, dtype=F)
    for s in range(steps):
        a = a + pp[s]
    return (a[0] + a[1]) + (a[2] + a[3])


def _stats32(v, eps, kdiv, fma, defect=None):
    """mean and rstd of the rows of v as the forward kernels form them."""
    cols = v.shape[1]
    eps_ = _c(f32(eps))
    if kdiv == 1:
        def mean_of(s, n=cols):
            return s / _c(float(n))
    else:
        def mean_of(s, n=cols):
            return s * (_c(1.0) / _c(float(n)))
    mu = mean_of(_wave_sum32(v))
    if defect == "one_pass_variance":
        var = mean_of(_wave_sum32(v, v, fma)) - mu * mu
        var = var.clamp_min(0.0)
    else:
        d = v - mu[:, None]
        var = mean_of(_wave_sum32(d, d, fma), cols - 1 if defect == "unbiased_variance" else cols)
    rs = _c(1.0) / (var.sqrt() + eps_) if defect == "eps_outside_sqrt" else torch.rsqrt(var + eps_)
    return mu, rs


# ------------------------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ------------------------------------------------------------------------------------------------------------------------------------
def ln_fwd64(x, res, gamma, beta, eps):
    """sum = x + res (exact), mean and rstd of THAT sum, y = (sum - mean) rstd gamma + beta."""
    eps = f32(eps)
    s = x.double() + (res.double() if res is not None else 0.0)
    mean, D, var, rstd = _stats64(s, eps)
    g, b = gamma.double(), beta.double()
    y = D * rstd[:, None] * g[None] + b[None]
    return dict(sum=s, mean=mean, rstd=rstd, y=y, D=D, var=var, eps=eps, gamma=g, kv=0 if res is None else 1)


def ln_fwd_bounds(r, dt):
    """v = fl(x + res): 1 rounding when there is a residual (kv), none otherwise; kdiv = 1.
    sum_out: v stored; y: _affine_bound, stored."""
    ev = r["kv"] * U32 * r["sum"].abs()
    b_mean, b_rstd = _stat_bounds(r["sum"], ev, r["mean"], r["D"], r["var"], r["rstd"], r["eps"], kdiv=1)
    b_z = _affine_bound(r["D"], ev, b_mean, r["rstd"], b_rstd, r["gamma"], r["y"])
    return dict(mean=b_mean, rstd=b_rstd, y=_store(b_z, r["y"], dt), sum=_store(ev, r["sum"], dt))


def ln_fwd_emulate32(x, res, gamma, beta, eps, defect=None):
    assert defect is None or defect in LN_FWD_DEFECTS
    dt = x.dtype
    v = x.float() + res.float() if res is not None else x.float()
    so = (x if defect == "residual_missing_from_sum_out" else v.to(dt)) if res is not None else None
    if defect == "stats_of_rounded_sum":
        v = v.to(dt).float()
    mu, rs = _stats32(v, eps, 1, False, defect)
    y = ((v - mu[:, None]) * rs[:, None]) * gamma.float()[None] + beta.float()[None]
    return y.to(dt), so, mu, rs


def ln_bwd64(dy, s, gamma, mean, rstd, dres):
    """A function of what the kernel receives: xhat = (s - mean) rstd from the STORED s and the fp32 mean / rstd handed in."""
    d, x, ga, mu, rs = dy.double(), s.double(), gamma.double(), mean.double(), rstd.double()
    xh = (x - mu[:, None]) * rs[:, None]
    g = d * ga[None]
    s1, s2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    inner = rs[:, None] * (g - s1 - xh * s2)
    dx = inner + (dres.double() if dres is not None else 0.0)
    return dict(dx=dx, dgamma=(d * xh).sum(0), dbeta=d.sum(0), d=d, xh=xh, g=g, rstd=rs, inner=inner, has_dres=dres is not None)


def ln_bwd_bounds(r, dt):
    """xhat = fl(fl(s - mean) * rstd): 2.  g = fl(dy gamma): 1.  dx: _dx_bound with kdiv = 1, the sum with dres 1 (on |dx|), the store.
    dgamma: terms dy xhat (xhat 2, product 1), dbeta: terms dy (exact); chain = ln_bwd_chain(rows)."""
    u = U32
    xh, g, d = r["xh"], r["g"], r["d"]
    b_xh = 2 * u * xh.abs()
    b = _dx_bound(g, u * g.abs(), xh, b_xh, r["rstd"], kdiv=1)
    if r["has_dres"]:
        b = b + u * r["dx"].abs()
    chain = ln_bwd_chain(d.shape[0])
    t = (d * xh).abs()
    return dict(dx=_store(b, r["dx"], dt), dgamma=_colsum_bound(t, 3 * u * t, chain), dbeta=_colsum_bound(d.abs(), 0 * d, chain))


def ln_bwd_emulate32(dy, s, gamma, mean, rstd, dres, defect=None, cap=LN_BWD_CAP):
    """-> dx (dtype of s), dgamma, dbeta fp32."""
    assert defect is None or defect in LN_BWD_DEFECTS
    dt = s.dtype
    d, x, ga = dy.float(), s.float(), gamma.float()[None]
    rows, cols = x.shape
    C_ = _c(float(cols))
    mu, rs = mean[:, None], rstd[:, None]
    xh = (x - mu) * rs
    g = d * ga
    s1 = (_wave_sum32(g) / C_)[:, None]
    s2 = (_wave_sum32(g, xh) / C_)[:, None]
    if defect == "no_mean_term":
        s1 = torch.zeros_like(s1)
    if defect == "no_xhat_term":
        s2 = torch.zeros_like(s2)
    o = rs * (g - s1 - xh * s2)
    if dres is not None and defect != "dres_not_added":
        o = o + dres.float()
    slot, it, n = _grid_slots(rows, cap)
    keep = (torch.arange(rows) < rows - 1) if defect == "last_row_dropped" else None
    skip = 1 if defect == "second_stride_iteration_dropped" else None
    pg = _col_accum32(g if defect == "dgamma_from_g" else d, xh, slot, it, n, skip_it=skip, keep=keep)
    pb = _col_accum32(d, None, slot, it, n, skip_it=skip, keep=keep)
    return o.to(dt), _ln_reduce32(pg), _ln_reduce32(pb)


# ------------------------------------------------------------------------------------------------------------------------------------
# ln_gelu (layers 1..): rows [B, L, C]
# ------------------------------------------------------------------------------------------------------------------------------------
def _live(Bn, L, row_limit):
    if row_limit is None:
        return torch.ones(Bn, L, dtype=torch.bool)
    return torch.arange(L)[None] < row_limit.long().reshape(Bn, 1)


def ln_gelu_fwd64(u, gamma, beta, eps, row_limit=None):
    """y = GELU(LayerNorm_C(u)) with the erf GELU; y, mean, rstd are zero in rows t >= row_limit[b]."""
    eps = f32(eps)
    Bn, L, C = u.shape
    v = u.double().reshape(Bn * L, C)
    mean, D, var, rstd = _stats64(v, eps)
    g, b = gamma.double(), beta.double()
    z = D * rstd[:, None] * g[None] + b[None]
    lv = _live(Bn, L, row_limit).reshape(-1)
    m = lv.double()
    return dict(y=(gelu64(z) * m[:, None]).view(Bn, L, C), mean=(mean * m).view(Bn, L), rstd=(rstd * m).view(Bn, L), z=z, v=v, D=D,
                var=var, eps=eps, gamma=g, live=lv, mean_all=mean, rstd_all=rstd)


def ln_gelu_fwd_bounds(r, dt, ev=None):
    """No residual (ev = 0; layer 0 passes the error of its convolution), kdiv = 2; z as _affine_bound; y = GELU(z) stored.  Zero from the limit on."""
    Bn, L, C = r["y"].shape
    ev = torch.zeros_like(r["v"]) if ev is None else ev
    b_mean, b_rstd = _stat_bounds(r["v"], ev, r["mean_all"], r["D"], r["var"], r["rstd_all"], r["eps"], kdiv=2)
    b_z = _affine_bound(r["D"], ev, b_mean, r["rstd_all"], b_rstd, r["gamma"], r["z"])
    m = r["live"].double()
    return dict(mean=(b_mean * m).view(Bn, L), rstd=(b_rstd * m).view(Bn, L), y=(_gelu_out_bound(r["z"], b_z, dt) * m[:, None]).view(Bn, L, C))


def ln_gelu_fwd_emulate32(u, gamma, beta, eps, row_limit=None, defect=None):
    assert defect is None or defect in LG_FWD_DEFECTS
    dt = u.dtype
    Bn, L, C = u.shape
    v = u.float().reshape(Bn * L, C)
    mu, rs = _stats32(v, eps, 2, True, defect)
    z = _fma((v - mu[:, None]) * rs[:, None], gamma.float()[None], beta.float()[None])
    y = gelu32(z, dt)
    if defect != "limit_row_not_zeroed":
        lv = _live(Bn, L, row_limit).reshape(-1)
        y, mu, rs = y * lv[:, None], mu * lv, rs * lv
    return y.to(dt).view(Bn, L, C), mu.view(Bn, L), rs.view(Bn, L)


def _gelu_bwd_core64(d, xh, ga, be, rs, lv):
    z = xh * ga[None] + be[None]
    dz = d * dgelu64(z)
    g = dz * ga[None]
    s1, s2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    du = rs[:, None] * (g - s1 - xh * s2) * lv[:, None]
    return z, dz, g, du


def _gelu_bwd_core_bounds(r, b_xh, dt, kdiv=2):
    """z = fmaf(xhat, gamma, beta): b_xh |gamma|, product and sum 2.
    dz = fl(dy GELU'(z')): |dy| (the approximation A', (|GELU''| + max|GELU'''| b_z) b_z, the product 1 on |GELU'|)
    g = fl(dz gamma): |gamma| b_dz + 1.   du (before the store): _dx_bound.
    terms of dgamma: fmaf(dz, xhat, .) -> b_dz |xhat| + |dz| b_xh;  of dbeta: dz -> b_dz;  of colsum(du): du -> its bound."""
    u = U32
    d, xh, z, ga = r["d"], r["xh"], r["z"], r["gamma"].abs()[None]
    b_z = ga * b_xh + u * ((xh.abs() * ga) + z.abs())
    b_dz = d.abs() * (a_dgelu(z, dt) + (d2gelu64(z).abs() + D3GELU_MAX * b_z) * b_z + u * dgelu64(z).abs())
    b_g = ga * b_dz + u * r["g"].abs()
    m = r["live"].double()[:, None]
    b_du = _dx_bound(r["g"], b_g, xh, b_xh, r["rstd"], kdiv) * m
    return b_dz * m, b_du


def ln_gelu_bwd64(dy, u, gamma, beta, mean, rstd, row_limit=None):
    """du, dgamma, dbeta, colsum(du) from the stored u and the fp32 mean / rstd handed in; rows from the limit on give du = 0 and add nothing."""
    Bn, L, C = u.shape
    lv = _live(Bn, L, row_limit).reshape(-1).double()
    d = dy.double().reshape(-1, C) * lv[:, None]
    mu, rs = mean.double().reshape(-1), rstd.double().reshape(-1)
    xh = (u.double().reshape(-1, C) - mu[:, None]) * rs[:, None] * lv[:, None]
    ga, be = gamma.double(), beta.double()
    z, dz, g, du = _gelu_bwd_core64(d, xh, ga, be, rs, lv)
    return dict(du=du.view(Bn, L, C), dgamma=(dz * xh).sum(0), dbeta=dz.sum(0), colsum=du.sum(0), d=d, xh=xh, z=z, dz=dz, g=g,
                gamma=ga, rstd=rs, live=lv.bool())


def ln_gelu_bwd_bounds(r, dt):
    """xhat = fl(fl(u - mean) rstd): 2.  chain = lg_bwd_chain(rows).  colsum(du) adds the UNSTORED du."""
    u = U32
    xh, dz = r["xh"], r["dz"]
    b_xh = 2 * u * xh.abs()
    b_dz, b_du = _gelu_bwd_core_bounds(r, b_xh, dt)
    chain = lg_bwd_chain(xh.shape[0])
    du = r["du"].reshape(xh.shape)
    return dict(du=_store(b_du, du, dt).view(r["du"].shape),
                dgamma=_colsum_bound((dz * xh).abs(), b_dz * xh.abs() + dz.abs() * b_xh, chain),
                dbeta=_colsum_bound(dz.abs(), b_dz, chain), colsum=_colsum_bound(du.abs(), b_du, chain))


def ln_gelu_bwd_emulate32(dy, u, gamma, beta, mean, rstd, row_limit=None, defect=None, cap=LG_BWD_CAP):
    """-> du (dtype of u), dgamma, dbeta, colsum(du) fp32."""
    assert defect is None or defect in LG_BWD_DEFECTS
    dt = u.dtype
    Bn, L, C = u.shape
    rows = Bn * L
    lv = _live(Bn, L, row_limit).reshape(-1)
    if defect == "limit_row_not_zeroed":
        lv = torch.ones_like(lv)
    d, x, ga, be = dy.float().reshape(rows, C), u.float().reshape(rows, C), gamma.float()[None], beta.float()[None]
    mu, rs = mean.reshape(rows, 1), rstd.reshape(rows, 1)
    inv_c = _c(1.0) / _c(float(C))
    xh = (x - mu) * rs
    dz = d * dgelu32(_fma(xh, ga, be), dt, defect)
    g = dz * ga
    s1 = (_wave_sum32(g) * inv_c)[:, None]
    s2 = (_wave_sum32(g, xh, True) * inv_c)[:, None]
    if defect == "no_mean_term":
        s1 = torch.zeros_like(s1)
    if defect == "no_xhat_term":
        s2 = torch.zeros_like(s2)
    o = rs * (g - s1 - xh * s2)
    o = torch.where(lv[:, None], o, torch.zeros_like(o))
    slot, it, n = _grid_slots(rows, cap)
    keep = lv.clone()
    if defect == "last_row_dropped":
        keep[int(torch.nonzero(lv).max())] = False
    skip = 1 if defect == "second_stride_iteration_dropped" else None
    pg = _col_accum32(g if defect == "dgamma_from_g" else dz, xh, slot, it, n, fma=True, skip_it=skip, keep=keep)
    pb = _col_accum32(dz, None, slot, it, n, skip_it=skip, keep=keep)
    pc = _col_accum32(o, None, slot, it, n, skip_it=skip, keep=keep)
    return o.to(dt).view(Bn, L, C), _lg_reduce32(pg), _lg_reduce32(pb), _lg_reduce32(pc)


# ------------------------------------------------------------------------------------------------------------------------------------
# layer 0: Conv1d(1 -> C, k, stride, bias) + LayerNorm(C) + GELU from the raw samples
# ------------------------------------------------------------------------------------------------------------------------------------
def _frames(wav, k, stride):
    return wav.unfold(1, k, stride)   # [B, L, k]


def _conv64(wav, w, bias, k, stride):
    """u [B L, C], and the bound of the kernel's u: bias, then k fmaf in tap order — k roundings, each of a partial sum that is at most
    |bias| + sum |w x| (the zero-padded taps of the generic kernel add exact zeros)."""
    X = _frames(wav.double(), k, stride)
    Bn, L, _ = X.shape
    X = X.reshape(Bn * L, k)
    W, bi = w.double(), bias.double()
    u = X @ W.t() + bi[None]
    b_u = k * U32 * (X.abs() @ W.abs().t() + bi.abs()[None])
    return X, u, b_u, Bn, L


def conv0_ln_fwd64(wav, w, bias, gamma, beta, k, stride, eps, frame_limit=None):
    """As ln_gelu_fwd64 on u = conv(wav) + bias; frames from frame_limit[b] on are not written by the kernel and not compared."""
    X, u, b_u, Bn, L = _conv64(wav, w, bias, k, stride)
    r = ln_gelu_fwd64(u.view(Bn, L, -1), gamma, beta, eps, frame_limit)
    r["b_u"] = b_u
    return r


def conv0_ln_fwd_bounds(r, dt):
    return ln_gelu_fwd_bounds(r, dt, ev=r["b_u"])


def _conv32(wav, w, bias, k, stride, defect=None):
    X = _frames(wav.float(), k, stride)
    Bn, L, _ = X.shape
    X = X.reshape(Bn * L, k)
    W = w.float()
    u = torch.zeros(Bn * L, W.shape[0], dtype=F) if defect == "bias_missing" else bias.float()[None].expand(Bn * L, -1).clone()
    for j in range(k - 1 if defect == "tap_k_minus_1_dropped" else k):
        u = _fma(W[None, :, j], X[:, j:j + 1], u)
    return X, u, Bn, L


def conv0_ln_fwd_emulate32(wav, w, bias, gamma, beta, k, stride, eps, frame_limit=None, defect=None):
    assert defect is None or defect in C0_DEFECTS
    dt = w.dtype
    X, u, Bn, L = _conv32(wav, w, bias, k, stride, defect)
    mu, rs = _stats32(u, eps, 2, True)
    y = gelu32(_fma((u - mu[:, None]) * rs[:, None], gamma.float()[None], beta.float()[None]), dt)
    return y.to(dt).view(Bn, L, -1), mu.view(Bn, L), rs.view(Bn, L)


def conv0_ln_bwd64(dy, wav, w, bias, gamma, beta, mean, rstd, k, stride, frame_limit=None):
    """dW [C, k], dbias, dgamma, dbeta from the raw samples and the fp32 mean / rstd handed in; frames from the limit on add nothing."""
    X, u, b_u, Bn, L = _conv64(wav, w, bias, k, stride)
    C = u.shape[1]
    lvb = _live(Bn, L, frame_limit).reshape(-1)
    lv = lvb.double()
    d = dy.double().reshape(-1, C) * lv[:, None]
    zero = torch.zeros(Bn * L, dtype=torch.float64)   # (from the limit on the kernel has written no statistics: whatever is there is not read)
    mu, rs = torch.where(lvb, mean.double().reshape(-1), zero), torch.where(lvb, rstd.double().reshape(-1), zero)
    xh = (u - mu[:, None]) * rs[:, None]
    ga, be = gamma.double(), beta.double()
    z, dz, g, du = _gelu_bwd_core64(d, xh, ga, be, rs, lv)
    return dict(dW=du.t() @ X, dbias=du.sum(0), dgamma=(dz * xh).sum(0), dbeta=dz.sum(0), d=d, xh=xh, z=z, dz=dz, g=g, gamma=ga,
                rstd=rs, live=lv.bool(), du=du, X=X, b_u=b_u, Bn=Bn, L=L)


def conv0_ln_bwd_bounds(r, dt):
    """xhat = fl(fl(u' - mean) rstd) with the recomputed u': rstd b_u + 2.  chain = c0_bwd_chain(B, L) (a wave adds up to 512 frames).
    dW[c, j]: terms fmaf(du, x_j, .): b_du |x_j| (the fmaf's rounding is the chain's)."""
    u = U32
    xh, dz, du, X = r["xh"], r["dz"], r["du"], r["X"].abs()
    b_xh = r["rstd"][:, None] * r["b_u"] * r["live"].double()[:, None] + 2 * u * xh.abs()
    b_dz, b_du = _gelu_bwd_core_bounds(r, b_xh, dt)
    chain = c0_bwd_chain(r["Bn"], r["L"])
    n = xh.shape[0]
    b_dw = SLACK * (b_du.t() @ X + chain * u * (du.abs().t() @ X)) + ETA * n
    return dict(dW=b_dw, dbias=_colsum_bound(du.abs(), b_du, chain),
                dgamma=_colsum_bound((dz * xh).abs(), b_dz * xh.abs() + dz.abs() * b_xh, chain), dbeta=_colsum_bound(dz.abs(), b_dz, chain))


def conv0_ln_bwd_emulate32(dy, wav, w, bias, gamma, beta, mean, rstd, k, stride, frame_limit=None, defect=None):
    """-> dW [C, k], dbias, dgamma, dbeta fp32."""
    assert defect is None or defect in C0_DEFECTS
    dt = w.dtype
    X, u, Bn, L = _conv32(wav, w, bias, k, stride, defect)
    n, C = u.shape
    lv = _live(Bn, L, frame_limit).reshape(-1)
    d, ga, be = dy.float().reshape(n, C), gamma.float()[None], beta.float()[None]
    mu, rs = mean.reshape(n, 1), rstd.reshape(n, 1)
    inv_c = _c(1.0) / _c(float(C))
    xh = (u - mu) * rs
    dz = d * dgelu32(_fma(xh, ga, be), dt)
    g = dz * ga
    s1 = (_wave_sum32(g) * inv_c)[:, None]
    s2 = (_wave_sum32(g, xh, True) * inv_c)[:, None]
    du = rs * (g - s1 - xh * s2)
    # frame (b, t): block t // 2048 of utterance b, wave (t % 2048) % 4, iteration (t % 2048) // 4; partial index b * nblk + block
    nblk = (L + C0_BWD_TB - 1) // C0_BWD_TB
    t = torch.arange(L).repeat(Bn)
    b = torch.arange(Bn).repeat_interleave(L)
    tl = t % C0_BWD_TB
    slot = ((b * nblk + t // C0_BWD_TB) * WAVES) + tl % WAVES
    it = tl // WAVES
    ns = Bn * nblk * WAVES
    pg = _col_accum32(dz, xh, slot, it, ns, fma=True, keep=lv)
    pb = _col_accum32(dz, None, slot, it, ns, keep=lv)
    pbi = _col_accum32(dz if defect == "dbias_from_dz" else du, None, slot, it, ns, keep=lv)
    dw = torch.stack([_lg_reduce32(_col_accum32(du, X[:, j:j + 1].expand(n, C), slot, it, ns, fma=True, keep=lv)) for j in range(k)], 1)
    return dw, _lg_reduce32(pbi), _lg_reduce32(pg), _lg_reduce32(pb)


# ------------------------------------------------------------------------------------------------------------------------------------
# cases shared by the CPU and the GPU tests (the CPU test runs every one of them)
# ------------------------------------------------------------------------------------------------------------------------------------
LN_COLS = [8, 72, 512, 520, 768, 1024, 1032, 2048]
LN_ROWS = 37
LN_FWD_BIG = 2 * 8192 + 5     # above ln_blocks(rows, 2048) * 4 twice over: the prefetch branch runs, and a third, partial iteration
LN_BWD_BIG = 2 * 4096 + 3
BIG_COLS = [64, 1032]
LG_COLS = [8, 72, 512, 520, 1024, 1032, 2048]
LG_B, LG_L = 3, 13
LG_BIG_L = 5471               # 3 * 5471 = 16413 rows: above 4 * 4096 and 4 * 1024; 5471 divides neither block stride
# (k, stride, C, S): L = (S - k) // stride + 1 is above 2048 and no multiple of 128
C0_KS = [(10, 5, 10400), (3, 2, 4200), (16, 7, 14500), (1, 1, 2100), (2, 2, 4200)]
C0_CASES = [(k, st, C, S) for (k, st, S) in C0_KS for C in (8, 72, 512)]
C0_B = 2
C0_LIMITS = (None, "L", 700)
EPS = 1e-5


def c0_L(k, stride, S):
    return (S - k) // stride + 1


@functools.lru_cache(maxsize=None)
def ln_case(rows, cols, dt, with_res=True):
    x, res = norm_rows(rows, cols, dt, with_res=True)
    gamma, beta = norm_params(cols, dt)
    dy, dres = norm_dy(rows, cols, dt)
    return x, (res if with_res else None), gamma, beta, dy, dres


@functools.lru_cache(maxsize=None)
def lg_case(Bn, L, C, dt):
    u = norm_rows(Bn * L, C, dt).view(Bn, L, C)
    gamma, beta = norm_params(C, dt)
    dy = norm_dy(Bn * L, C, dt)[0].view(Bn, L, C)
    return u, gamma, beta, dy


def lg_limit(Bn, L, which):
    """row_limit cases of the issue: every utterance L, L / 3, or 0; None: no limit vector."""
    return None if which is None else torch.full((Bn,), {"L": L, "L/3": L // 3, "0": 0}[which], dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def c0_case(k, stride, C, S, dt):
    wav, w, bias = conv0_inputs(C0_B, S, C, k, dt)
    gamma, beta = norm_params(C, dt)
    L = c0_L(k, stride, S)
    dy = norm_dy(C0_B * L, C, dt)[0].view(C0_B, L, C)
    return wav, w, bias, gamma, beta, dy


def c0_limit(L, which):
    return None if which is None else torch.full((C0_B,), L if which == "L" else which, dtype=torch.int32)
