"""fp64 restatements, counted forward-error bounds and fp32 op-by-op emulations of the HBM-bound helpers in csrc/elementwise.hip
(cst_glu_fwd / _bwd, cst_act_fwd / _bwd, cst_colsum, cst_colsum_typed, cst_colsum_typed_live, cst_dropout_colsum, cst_col2im1d, cst_mask_rows,
cst_dropout, cst_rows_pack / _unpack, cst_weight_norm_fwd / _bwd), the embedding kernels in csrc/embed.hip (cst_embed_pos_fwd,
cst_embed_bwd, cst_dropout_scale) and the contrastive term in csrc/loss_optim.hip (cst_contrastive_fwd / _bwd).  Plain torch (and
numpy for the dropout hash); no GPU and no import of the package.  Shared by
test_helper_ref_cpu.py (a faithful fp32 evaluation stays inside every bound and every listed defect leaves it) and test_helper_gpu.py
(the kernels under the same bounds).  Built like norm_ref.py; U32, UBF, ETA, FLUSH, SLACK and worst_ratio are loss_optim_ref.py's,
INTRIN, the GELU constants and the fp64 / fp32 GELU restatements norm_ref.py's.

How the bounds are counted.  Every fp32 add, multiply or fma returns (x op y)(1 + d), |d| <= u = 2^-24, on the magnitude it produced;
a sum is charged (chain length) u on the sum of the ABSOLUTE terms, the chain length read from the kernel; __expf, sqrtf, / and
__frcp_rn count INTRIN = 2 each (csrc/Makefile passes no divide / sqrt flag: hipcc's default is the correctly rounded pair, which
INTRIN covers, as it covers the fast pair); an error of the ARGUMENT of __expf (the rounded log2 e and its product: 2 |a| u) is a
relative error of the result; a bf16 store adds 2^-8.  An exponential below 2^-126 may come back as 0 (FLUSH); one above the fp32
range comes back as Inf, after which 1 / (1 + Inf) = 0 where the exact value is below 2^-128: the same FLUSH term covers it.
The compiler may contract a product into the following sum (one rounding where the count assumes two): the count is an upper bound for
either code.  First-order sums are multiplied by SLACK.  No constant here was fitted to an output of a kernel or of an emulation; the
only measured constants are the four GELU figures of norm_ref.py.

Scalars the launchers form on the host (the dropout factor 1.0f / (1.0f - p), the threshold) are IEEE fp32 operations on the CPU and
are restated bit for bit (drop_scale, drop_thr): the references take them as exact inputs, as loss_optim_ref.py takes its `float`
arguments.  The dropout mask is the counter hash of csrc/cst_common.h restated in numpy (keep_mask); test_helper_gpu.py checks it
against the package's own numpy statement."""
import functools
import math

import numpy as np
import torch

from loss_optim_ref import BLOCK_SUM_ADDS, ETA, FLUSH, SLACK, U32, UBF, _block_sum32, f32, out_u, worst_ratio  # noqa: F401  (re-exported)
from norm_ref import INTRIN, NAME, _c, _fma, _ln_reduce32, _store, a_dgelu, a_gelu, dgelu32, dgelu64, gelu32, gelu64  # noqa: F401

F, B = torch.float32, torch.bfloat16
EW_THREADS = 4096 * 256               # ew_blocks caps an elementwise grid at 4096 blocks of 256 threads, 8 elements per thread
EW_BIG = 8 * (EW_THREADS + 3)         # 8 388 632 elements: every thread runs once, three run a second grid-stride iteration
PAD = 1


def _gen(seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return g


def _cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------------------------------------------
# dropout: the counter hash, the launcher's scalars
# ------------------------------------------------------------------------------------------------------------------------------------
_M32 = 0xFFFFFFFF


def drop_thr(p):
    """cst_drop_thr16: (uint32)(p * 65536.0f + 0.5f) in fp32."""
    return int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))


def drop_scale(p):
    """The launchers' 1.0f / (1.0f - p) in fp32 (1 for p = 0), as a double."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def keep_mask(key, n, p, idx=None):
    """keep decisions of the elements idx (default 0 .. n - 1) of site `key`: cst_drop_bits / cst_drop8 / cst_drop1 of csrc/cst_common.h."""
    u = np.uint64
    idx = np.arange(n, dtype=np.uint64) if idx is None else np.asarray(idx).astype(np.uint64)
    pair = idx >> u(1)
    key2 = (int(key) * 0x2C1B3C6D + 0x297A2D39) & _M32
    x = (((pair & u(_M32)) ^ u(int(key) & _M32)) + (pair >> u(32)) * u(0x9E3779B1)) & u(_M32)
    x = (x * u(0x9E3779B1)) & u(_M32)
    x = ((x ^ (x >> u(15))) + u(key2)) & u(_M32)
    x = (x * u(0x85EBCA77)) & u(_M32)
    x ^= x >> u(13)
    half = np.where((idx & u(1)) == 1, x >> u(16), x & u(0xFFFF))
    return torch.from_numpy(half >= u(drop_thr(p)))


def _factor(keep, p, dtype=torch.float64):
    return keep.to(dtype) * drop_scale(p)


# ------------------------------------------------------------------------------------------------------------------------------------
# GLU: y = a sigma(g);  da = dy sigma,  dg = dy a sigma (1 - sigma)
# ------------------------------------------------------------------------------------------------------------------------------------
GLU_SHAPES = [(1, 8), (77, 64)]
GLU_BIG = (4099, 2056)            # 8 427 544 gate / value pairs: the second grid-stride iteration
GLU_DEFECTS = ("halves_swapped", "dg_without_one_minus_sigma", "da_from_sigma_of_a")
GLU_PLANTS = (30.0, -30.0, 100.0, -100.0)


def glu_inputs(rows, C, dt, seed=21):
    """z [rows, 2 C] N(0, 1) (value half, gate half), dy [rows, C].  Four gates are planted: +-30 saturate the sigmoid (1 - sigma =
    9e-14), at +100 __expf(-g) is flushed to 0, at -100 it overflows to Inf."""
    g = _gen(seed)
    z = torch.randn(rows, 2 * C, generator=g)
    dy = torch.randn(rows, C, generator=g)
    n = rows * C
    for k, val in enumerate(GLU_PLANTS):
        i = (k * (n // 4) + 1) % n
        z[i // C, C + i % C] = val
    return z.to(dt), dy.to(dt)


def glu64(z, dy):
    C = z.shape[1] // 2
    a, g, d = z[:, :C].double(), z[:, C:].double(), dy.double()
    s = torch.sigmoid(g)
    return dict(y=a * s, da=d * s, dg=d * a * s * (1.0 - s), a=a, g=g, d=d, s=s)


def _sigma_rel(g, s):
    """Relative error of 1 / (1 + __expf(-g)) (and of a / (1 + __expf(-g)), the same operations): E = __expf(-g) carries INTRIN + 2 |g|,
    it enters 1 + E with weight E / (1 + E) = 1 - sigma; the sum 1; the division INTRIN."""
    return U32 * ((1.0 - s) * (INTRIN + 2.0 * g.abs()) + 1.0 + INTRIN)


def glu_bounds(r, dt):
    """y: _sigma_rel on |y|, and |a| FLUSH.   da = fl(dy sg): _sigma_rel + 1.
    dg = fl(fl(fl(dy a) sg) fl(1 - sg)): the products 3 and _sigma_rel on |dg|; 1 - sg has the ABSOLUTE error sigma rel + u (1 - sigma)
    (at sigma = 1 - 9e-14 the fp32 value is 0: the error is all of 1 - sigma, and the bound says so)."""
    a, d, s = r["a"].abs(), r["d"].abs(), r["s"]
    rs = _sigma_rel(r["g"], s)
    by = SLACK * r["y"].abs() * rs + a * FLUSH + ETA
    bda = SLACK * r["da"].abs() * (rs + U32) + d * FLUSH + ETA
    bdg = SLACK * (r["dg"].abs() * (rs + 3.0 * U32) + d * a * s * (s * rs + U32 * (1.0 - s))) + d * a * FLUSH + ETA
    return dict(y=_store(by, r["y"], dt), dz=torch.cat([_store(bda, r["da"], dt), _store(bdg, r["dg"], dt)], 1))


def glu_emulate32(z, dy, defect=None):
    """-> y, dz in the dtype of z.  torch.exp stands in for __expf (whose own error the bound carries)."""
    assert defect is None or defect in GLU_DEFECTS
    dt = z.dtype
    C = z.shape[1] // 2
    a, g, d = z[:, :C].float(), z[:, C:].float(), dy.float()
    if defect == "halves_swapped":
        a, g = g, a
    one = _c(1.0)
    y = a / (one + torch.exp(-g))
    sg = one / (one + torch.exp(-g))
    da = d * (one / (one + torch.exp(-a)) if defect == "da_from_sigma_of_a" else sg)
    dg = d * a * sg
    if defect != "dg_without_one_minus_sigma":
        dg = dg * (one - sg)
    return y.to(dt), torch.cat([da, dg], 1).to(dt)


# ------------------------------------------------------------------------------------------------------------------------------------
# activations
# ------------------------------------------------------------------------------------------------------------------------------------
ACT_SIZES = [8, EW_BIG]
ACT_DEFECTS = ("relu_prime_at_zero_is_one",)


def act_inputs(n, dt, seed=22):
    """x N(0, 1) with +0, -0, the smallest subnormal of dt and minus the smallest normal in the first four places; dy N(0, 1)."""
    g = _gen(seed)
    x = torch.randn(n, generator=g).to(dt)
    dy = torch.randn(n, generator=g).to(dt)
    sub = 2.0 ** -149 if dt == F else 2.0 ** -133
    x[:4] = torch.tensor([0.0, -0.0, sub, -torch.finfo(dt).tiny], dtype=torch.float64).to(dt)
    assert float(x[2]) == sub and bool(torch.signbit(x[1])) and float(x[1]) == 0.0
    return x, dy


def relu_ref(x, dy):
    """Exact, in the storage dtype: max(x, 0); dy where x > 0, else 0 (the derivative at +-0 is 0, torch's and the oracle's convention)."""
    return torch.relu(x), torch.where(x > 0, dy, torch.zeros_like(dy))


def relu_emulate(x, dy, defect=None):
    assert defect is None or defect in ACT_DEFECTS
    on = (x >= 0) if defect == "relu_prime_at_zero_is_one" else (x > 0)
    return torch.relu(x), (dy.float() * on.float()).to(x.dtype)


def gelu_act64(x, dy):
    z = x.double()
    return dict(y=gelu64(z), dx=dy.double() * dgelu64(z), z=z, d=dy.double())


def gelu_act_bounds(r, dt):
    """y: the approximation (A_GELU, with the intrinsics' share), the store.  dx = fl(dy GELU'(z)): |dy| (A_DGELU + u |GELU'|), the store."""
    z, d = r["z"], r["d"].abs()
    return dict(y=_store(a_gelu(z, dt) + ETA, r["y"], dt), dx=_store(d * (a_dgelu(z, dt) + U32 * dgelu64(z).abs()) + ETA, r["dx"], dt))


def gelu_act_emulate32(x, dy):
    dt = x.dtype
    return gelu32(x.float(), dt).to(dt), (dy.float() * dgelu32(x.float(), dt)).to(dt)


# ------------------------------------------------------------------------------------------------------------------------------------
# mask_rows, dropout, dropout_scale
# ------------------------------------------------------------------------------------------------------------------------------------
MASK_SHAPES = [(7, 8), (1234, 72)]
MASK_BIG = (4099 * 8 + 1, 256)     # 8 395 008 elements
DROP_SIZES = [1, 7, 8, 4099, EW_BIG + 5]      # the last: a second iteration and a scalar tail of 5
DROP_SCALE_SIZES = [8, 4104, EW_BIG]           # cst_dropout_scale takes multiples of 8
DROP_PS = [0.1, 0.5]
DROP_KEY = 0x1234ABCD
ALPHA = math.sqrt(512.0)
MASK_DEFECTS = ("masked_by_product",)
DROP_DEFECTS = ("pair_halves_swapped", "scalar_tail_dropped", "scale_missing")


def mask_inputs(rows, cols, dt, seed=23):
    """x N(0, 1); every third row is masked, and masked rows hold NaN, +Inf and -Inf."""
    x = torch.randn(rows, cols, generator=_gen(seed)).to(dt)
    mask = (torch.arange(rows) % 3 == 0)
    x[0, 0], x[0, cols - 1], x[3 % rows if rows > 3 else 0, 1] = float("nan"), float("inf"), float("-inf")
    if rows > 6:
        x[(rows - 1) // 3 * 3] = float("nan")
    assert bool(torch.isfinite(x[~mask].float()).all())
    return x, mask.to(torch.uint8)


def mask_ref(x, mask):
    return torch.where(mask.bool()[:, None], torch.zeros_like(x), x)


def mask_emulate(x, mask, defect=None):
    assert defect is None or defect in MASK_DEFECTS
    if defect == "masked_by_product":
        return (x.float() * (1.0 - mask.float())[:, None]).to(x.dtype)
    return mask_ref(x, mask)


def drop_inputs(n, dt, seed=24):
    x = torch.randn(n, generator=_gen(seed))
    x[x == 0] = 1.0                 # (a kept element must not be zero: the kept set is read off the output)
    x = x.to(dt)
    assert bool((x != 0).all())
    return x


def dropout64(x, keep, p, alpha=None):
    """y = x keep s [alpha], s the launcher's fp32 factor, alpha as its fp32 value.  Bound: the product with s one rounding (none at
    p = 0, where s = 1), the product with alpha one more, the store."""
    y = x.double() * _factor(keep.to(x.device), p)
    k = 0 if p == 0 else 1
    if alpha is not None:
        y = y * f32(alpha)
        k += 1
    return y, _store(SLACK * k * U32 * y.abs() + (ETA if k else 0.0), y, x.dtype)


def dropout_emulate32(x, key, p, alpha=None, defect=None):
    assert defect is None or defect in DROP_DEFECTS
    n = x.numel()
    idx = np.arange(n, dtype=np.uint64)
    keep = keep_mask(key, n, p, idx ^ np.uint64(1) if defect == "pair_halves_swapped" else idx)
    s = 1.0 if defect == "scale_missing" else drop_scale(p)
    y = x.float().reshape(-1) * (keep.float() * _c(s))
    if alpha is not None:
        y = y * _c(f32(alpha))
    if defect == "scalar_tail_dropped":
        y[n // 8 * 8:] = 0.0
    return y.to(x.dtype).view(x.shape)


# ------------------------------------------------------------------------------------------------------------------------------------
# col2im1d: dx[b, l, :] = dact(z[b, l, :]) * sum_j dcol[b, t, j, :],  l + pad - j = t stride, 0 <= t < Lout, j ascending
# ------------------------------------------------------------------------------------------------------------------------------------
C2I_TRIPLES = [(3, 2, 0), (2, 2, 0), (5, 2, 2), (10, 5, 0), (3, 1, 1), (1, 1, 0), (3, 2, 2)]
C2I_B = 2
C2I_BIG = (2, 4099 * 128, 8, 3, 2, 0)      # B, Lin, C, k, stride, pad: 8 394 752 output elements
C2I_DEFECTS = ("tap_k_minus_1_dropped", "t_guard_missing", "pad_ignored", "stride_parity_missing", "dact_from_row_l_plus_1")


def c2i_lins(k, stride, pad):
    """Two input lengths from 41 on: one with (Lin + 2 pad - k) divisible by the stride, one without (trailing positions that receive
    nothing) — at stride 1 both are divisible."""
    div = next(L for L in range(41, 60) if (L + 2 * pad - k) % stride == 0)
    non = next((L for L in range(41, 60) if (L + 2 * pad - k) % stride), div + 1)
    return sorted((div, non))


C2I_CASES = [(k, s, p, Lin, C) for (k, s, p) in C2I_TRIPLES for Lin in c2i_lins(k, s, p) for C in (8, 16)]


def c2i_lout(Lin, k, stride, pad):
    return (Lin + 2 * pad - k) // stride + 1


def c2i_inputs(Bn, Lin, C, k, stride, pad, dt, seed=25):
    g = _gen(seed)
    Lout = c2i_lout(Lin, k, stride, pad)
    dcol = torch.randn(Bn, Lout, k * C, generator=g).to(dt)
    z = torch.randn(Bn, Lin, C, generator=g).to(dt)
    return dcol, z


def _c2i_gather(dcol, Bn, Lin, Lout, C, k, stride, pad, acc_dtype, defect=None):
    """-> (sum, sum of |terms|, number of taps) [Bn, Lin, C] / [Lin]; the taps are added in the order j = 0 .. k - 1, as the kernel does.
    A contribution is addressed as the kernel addresses it, by the flat frame b Lout + t: without the t < Lout guard (a defect) that
    is a frame of the next utterance (beyond the tensor: nothing)."""
    dev = dcol.device
    d = dcol.reshape(Bn * Lout, k, C).to(acc_dtype)
    acc = torch.zeros(Bn, Lin, C, dtype=acc_dtype, device=dev)
    ab = torch.zeros_like(acc)
    cnt = torch.zeros(Lin, dtype=torch.int64, device=dev)
    l_all = torch.arange(Lin, device=dev)
    for j in range(k - 1 if defect == "tap_k_minus_1_dropped" else k):
        num = l_all + (0 if defect == "pad_ignored" else pad) - j
        ok = num >= 0
        if defect != "stride_parity_missing":
            ok = ok & (num % stride == 0)
        t = torch.div(num.clamp_min(0), stride, rounding_mode="floor")
        if defect != "t_guard_missing":
            ok = ok & (t < Lout)
        li, ti = l_all[ok], t[ok]
        fr = torch.arange(Bn, device=dev)[:, None] * Lout + ti[None]
        inside = fr < Bn * Lout
        v = d[fr.clamp_max(Bn * Lout - 1).reshape(-1), j].view(Bn, -1, C) * inside[:, :, None].to(acc_dtype)
        acc[:, li] = acc[:, li] + v
        ab[:, li] = ab[:, li] + v.abs()
        cnt[li] += 1
    return acc, ab, cnt


def col2im64(dcol, z, Bn, Lin, C, k, stride, pad, dact):
    Lout = c2i_lout(Lin, k, stride, pad)
    acc, ab, cnt = _c2i_gather(dcol, Bn, Lin, Lout, C, k, stride, pad, torch.float64)
    zz = z.double() if dact else None
    da = dgelu64(zz) if dact == "gelu" else ((zz > 0).double() if dact == "relu" else None)
    return dict(dx=acc if da is None else acc * da, acc=acc, ab=ab, cnt=cnt, da=da, z=zz, dact=dact)


def col2im_bounds(r, dt):
    """The sum of n taps: n - 1 roundings (0 + v is exact) on sum |terms|.  GELU': |GELU'| b_sum + |sum| (A_DGELU + u |GELU'|); ReLU'
    is an exact factor.  The store."""
    b = SLACK * (r["cnt"] - 1).clamp_min(0).double()[None, :, None] * U32 * r["ab"]
    if r["dact"] == "gelu":
        b = r["da"].abs() * b + r["acc"].abs() * (a_dgelu(r["z"], dt) + U32 * r["da"].abs()) + ETA
    elif r["dact"] == "relu":
        b = b * r["da"]
    return _store(b, r["dx"], dt)


def col2im_emulate32(dcol, z, Bn, Lin, C, k, stride, pad, dact, defect=None):
    assert defect is None or defect in C2I_DEFECTS
    dt = dcol.dtype
    acc, _, _ = _c2i_gather(dcol, Bn, Lin, c2i_lout(Lin, k, stride, pad), C, k, stride, pad, F, defect)
    if dact:
        zz = z.float()
        if defect == "dact_from_row_l_plus_1":
            zz = torch.roll(zz.reshape(Bn * Lin, C), -1, 0).view(Bn, Lin, C)
        acc = acc * (dgelu32(zz, dt) if dact == "gelu" else (zz > 0).float())
    return acc.to(dt)


# ------------------------------------------------------------------------------------------------------------------------------------
# rows_pack (tail_sum) / rows_unpack
# ------------------------------------------------------------------------------------------------------------------------------------
RP_T = 77
RP_LENS = [77, 76, 70, 69, 33, 1]      # tail lengths 1, 2, 8, 9, 45, 77: both sides of the 8-row unroll
RP_COLS = [8, 136, 520]                # 520: a second lane stride of 512 columns
RP_DEFECTS = ("row_T_minus_1_dropped", "group_boundary_row_added_twice", "columns_from_512_dropped")


def rp_inputs(C, dt, seed=26):
    x = torch.randn(len(RP_LENS), RP_T, C, generator=_gen(seed)).to(dt)
    off = torch.zeros(len(RP_LENS) + 1, dtype=torch.int32)
    off[1:] = torch.cumsum(torch.tensor(RP_LENS), 0)
    return x, off


def rows_pack64(x, off):
    """-> (packed [N, C] fp64, bound [N, C]).  Rows t < n_b - 1 are copies (bound 0: exact); the last packed row of sequence b is the
    sum of rows n_b - 1 .. T - 1 in index order: T - n_b roundings on sum |terms|, then the store (a single row is a copy)."""
    Bn, T, C = x.shape
    N = int(off[-1])
    ref = torch.zeros(N, C, dtype=torch.float64)
    bound = torch.zeros(N, C, dtype=torch.float64)
    for b in range(Bn):
        o, n = int(off[b]), int(off[b + 1] - off[b])
        ref[o:o + n - 1] = x[b, :n - 1].double()
        tail = x[b, n - 1:].double()
        ref[o + n - 1] = tail.sum(0)
        if T - n > 0:
            bound[o + n - 1] = _store(SLACK * (T - n) * U32 * tail.abs().sum(0), ref[o + n - 1], x.dtype)
    return ref, bound


def rows_pack_emulate32(x, off, defect=None):
    assert defect is None or defect in RP_DEFECTS
    Bn, T, C = x.shape
    out = torch.zeros(int(off[-1]), C, dtype=x.dtype)
    for b in range(Bn):
        o, n = int(off[b]), int(off[b + 1] - off[b])
        out[o:o + n - 1] = x[b, :n - 1]
        a = torch.zeros(C, dtype=F)
        groups = (T - (n - 1)) // 8
        for r in range(n - 1, T - 1 if defect == "row_T_minus_1_dropped" else T):
            a = a + x[b, r].float()
            if defect == "group_boundary_row_added_twice" and groups and r == n - 1 + 8 * groups - 1:
                a = a + x[b, r].float()
        if defect == "columns_from_512_dropped":
            a[512:] = 0.0
        out[o + n - 1] = a.to(x.dtype)
    return out


def rows_unpack_ref(packed, off, Bn, T, tail):
    """Exact: dst[b, t] = packed[off[b] + min(t, n_b - 1)] (tail) or 0 beyond the sequence."""
    out = torch.zeros(Bn, T, packed.shape[1], dtype=packed.dtype)
    for b in range(Bn):
        o, n = int(off[b]), int(off[b + 1] - off[b])
        out[b, :n] = packed[o:o + n]
        if tail:
            out[b, n:] = packed[o + n - 1]
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# weight normalisation along the last dimension
# ------------------------------------------------------------------------------------------------------------------------------------
WN_COLS = [8, 16, 32, 64, 128, 256]
WN_ROWS = [1, 33, 256, 257, 256 * 3 + 5]
WN_MODEL = (768 * 48, 128)
WN_CASES = [(R, C) for C in WN_COLS for R in WN_ROWS] + [WN_MODEL]
WN_CHUNK = 256
WN_FWD_DEFECTS = ("norm_per_row", "last_row_chunk_dropped", "norm_of_rounded_w")
WN_BWD_DEFECTS = ("dv_without_projection", "dg_is_dot", "last_row_chunk_dropped")
WN_G0, WN_SMALL, WN_LARGE, WN_ORTH = 1, 2, 3, 4   # columns: g = 0; |v| ~ 1e-3; |v| ~ 1e3; dw orthogonal to v


def wn_inputs(R, C, dt, seed=27):
    """v [R, C] N(0, 1) with column 2 of norm ~ 1e-3 and column 3 of norm ~ 1e3; g N(0, 1) of both signs with g[1] = 0 exactly;
    dw N(0, 1), its column 4 made orthogonal to v's (in fp64, then stored): dot ~ 0 against sum |dw v| ~ R."""
    g_ = _gen(seed)
    v = torch.randn(R, C, generator=g_)
    g = torch.randn(C, generator=g_)
    dw = torch.randn(R, C, generator=g_)
    g[0], g[WN_G0], g[5] = 0.7, 0.0, -1.3
    v[:, WN_SMALL] *= 1e-3 / float(v[:, WN_SMALL].norm())
    v[:, WN_LARGE] *= 1e3 / float(v[:, WN_LARGE].norm())
    v = v.to(dt)
    vo, do = v[:, WN_ORTH].double(), dw[:, WN_ORTH].double()
    dw[:, WN_ORTH] = (do - vo * (do @ vo) / (vo @ vo)).float()
    return v, g.to(dt), dw.to(dt)


def wn_chain(R, C):
    """Roundings on the longest path of a column sum of products: the product (or the fma) 1, a row lane's C / 8 steps, the 2048 / C
    lanes added in order, the row chunks added in order."""
    gpr = C // 8
    return 1 + gpr + 256 // gpr + _cdiv(R, WN_CHUNK)


def wn_fwd64(v, g):
    V, G = v.double(), g.double()
    n = (V * V).sum(0).sqrt()
    return dict(w=V * (G / n)[None], norm=n, R=v.shape[0], C=v.shape[1])


def wn_fwd_bounds(r, dt):
    """s = sum v^2 (all terms positive: relative wn_chain u); n = sqrtf(s): half of that, INTRIN; scale = g / n: INTRIN; w = fl(v scale): 1;
    the store."""
    cs = wn_chain(r["R"], r["C"])
    rel_n = U32 * (0.5 * cs + INTRIN)
    return dict(norm=SLACK * r["norm"] * rel_n + ETA, w=_store(SLACK * r["w"].abs() * (rel_n + (INTRIN + 1) * U32) + ETA, r["w"], dt))


def _wn_colsum32(a, b, drop_last=False):
    """wn_partial_kernel + the chunk-order sum of the apply kernels: column sums of a * b over the rows."""
    R, C = a.shape
    gpr = C // 8
    rpp = 256 // gpr
    nch = _cdiv(R, WN_CHUNK)
    pa, pb = torch.zeros(nch * WN_CHUNK, C, dtype=F), torch.zeros(nch * WN_CHUNK, C, dtype=F)
    pa[:R], pb[:R] = a, b
    pa, pb = pa.view(nch, gpr, rpp, C), pb.view(nch, gpr, rpp, C)    # row r0 + lane + rpp * step
    acc = torch.zeros(nch, rpp, C, dtype=F)
    for i in range(gpr):
        acc = _fma(pa[:, i], pb[:, i], acc)
    part = torch.zeros(nch, C, dtype=F)
    for lane in range(rpp):
        part = part + acc[:, lane]
    s = torch.zeros(C, dtype=F)
    for k in range(nch - 1 if drop_last else nch):
        s = s + part[k]
    return s


def wn_fwd_emulate32(v, g, defect=None):
    """-> w (dtype of v), norm fp32."""
    assert defect is None or defect in WN_FWD_DEFECTS
    dt = v.dtype
    vf = v.float()
    if defect == "norm_per_row":
        n = (vf * vf).sum(1, keepdim=True).sqrt()
        return (vf * (g.float()[None] / n)).to(dt), n.reshape(-1)[:v.shape[1]]
    n = _wn_colsum32(vf, vf, defect == "last_row_chunk_dropped").sqrt()
    w = (vf * (g.float() / n)[None]).to(dt)
    if defect == "norm_of_rounded_w":
        n = n.to(B).float()
    return w, n


def wn_bwd64(v, g, dw, norm):
    """A function of what the kernel receives: the fp32 norm handed in.  dv = (g / n)(dw - v dot / n^2), dg = dot / n."""
    V, G, D, n = v.double(), g.double(), dw.double(), norm.double()
    dot = (D * V).sum(0)
    co, sc = dot / (n * n), G / n
    inner = D - V * co[None]
    return dict(dv=sc[None] * inner, dg=dot / n, dot=dot, adot=(D * V).abs().sum(0), co=co, sc=sc, inner=inner, V=V, n=n, R=v.shape[0], C=v.shape[1])


def wn_bwd_bounds(r, dt):
    """dot: wn_chain on sum |dw v|.  dg = dot / n: b_dot / n, INTRIN, the store.  co = dot / fl(n n): b_dot / n^2, the product 1, INTRIN.
    sc = g / n: INTRIN.  dv = fl(sc fl(dw - fl(v co))): |v| b_co, the product 1 on |v co|, the difference 1 on |inner|; times |sc|; the
    error of sc on |inner|; the last product 1 on |dv|; the store."""
    u, n = U32, r["n"]
    b_dot = SLACK * wn_chain(r["R"], r["C"]) * u * r["adot"] + ETA * r["R"]
    b_dg = b_dot / n + INTRIN * u * r["dg"].abs() + ETA
    b_co = b_dot / (n * n) + (1 + INTRIN) * u * r["co"].abs()
    V, inner, sc = r["V"].abs(), r["inner"].abs(), r["sc"].abs()
    b_inner = V * b_co[None] + u * V * r["co"].abs()[None] + u * inner
    b_dv = SLACK * (sc[None] * b_inner + (INTRIN * u * sc)[None] * inner + u * r["dv"].abs()) + ETA * (sc[None] > 0)
    return dict(dv=_store(b_dv, r["dv"], dt), dg=_store(b_dg, r["dg"], dt))


def wn_bwd_emulate32(v, g, dw, norm, defect=None):
    """-> dv, dg in the dtype of v."""
    assert defect is None or defect in WN_BWD_DEFECTS
    dt = v.dtype
    vf, df, gf = v.float(), dw.float(), g.float()
    dot = _wn_colsum32(vf, df, defect == "last_row_chunk_dropped")
    sc, co = gf / norm, dot / (norm * norm)
    dg = dot if defect == "dg_is_dot" else dot / norm
    dv = sc[None] * df if defect == "dv_without_projection" else sc[None] * (df - vf * co[None])
    return dv.to(dt), dg.to(dt)


# ------------------------------------------------------------------------------------------------------------------------------------
# column sums: cst_colsum (atomics), cst_colsum_typed / _live, cst_dropout_colsum
# ------------------------------------------------------------------------------------------------------------------------------------
CS_ROWS = [1, 15, 17, 64, 113, 127, 64 * 65 + 49]
CS_COLS = [8, 128, 136, 264]
CS_KEY, CS_P, CS_EPOCH = 0x1234567, 0.1, 7
CS_DEFECTS = ("tail_rows_dropped", "chunks_from_64_dropped", "stamp_off_by_one_tile", "sums_of_unrounded_product", "last_column_block_dropped")
CS_STAMPS = (None, "alternate", "last_dead", "last_live")


def cs_inputs(rows, cols, dt, seed=28):
    """N(0, 1); column 1 is 100 +- 0.1 (no cancellation: the sum is of the size of sum |terms|); one 1e4 spike in column 3."""
    x = torch.randn(rows, cols, generator=_gen(seed))
    x[:, 1] = 100.0 + 0.1 * x[:, 1]
    x[(rows - 1) // 2, 3] = 1e4
    return x.to(dt)


def cs_stamps(rows, which):
    """(stamps int32 [ceil(rows / 64)], row mask of the dead tiles).  alternate: every second tile dead (from tile 1); last_dead: the
    last tile (partial when rows % 64) dead; last_live: tile 0 dead (when there is another), the last live."""
    nt = _cdiv(rows, 64)
    st = torch.full((nt,), CS_EPOCH, dtype=torch.int32)
    if which == "alternate":
        st[1::2] = 0
    elif which == "last_dead":
        st[-1] = 3
    elif which == "last_live" and nt > 1:
        st[0] = CS_EPOCH - 1
    dead = (st != CS_EPOCH)[torch.arange(rows) // 64]
    return st, dead


def cs_grid(rows, cols, typed):
    """(rows per chunk, chunks) of cst_colsum (atomics) and of colsum_grid (typed: whole 64-row tiles per chunk)."""
    cblocks = _cdiv(cols // 8, 16)
    chunks = max(1, min(_cdiv(1536, cblocks), _cdiv(rows, 64)))
    rows_per = _cdiv(rows, chunks)
    if typed:
        rows_per = _cdiv(rows_per, 64) * 64
    return rows_per, _cdiv(rows, rows_per)


def _lane_steps(n_c, g):
    main = max(0, _cdiv(n_c - 48 - g, 64))
    return main, max(0, _cdiv(n_c - (g + 64 * main), 16))


def cs_chain(rows, cols, typed):
    """Roundings on the longest path of one column: a row lane's main-loop steps, three per four rows ((v0 + v1) + (v2 + v3), then the
    accumulator), plus its tail steps — the largest over lanes and chunks; the 16-term LDS combine; then the reduce kernel's
    ceil(chunks / 64) + 63, or for the atomics one rounding per chunk in an order nobody fixes."""
    rows_per, nch = cs_grid(rows, cols, typed)
    lane = 0
    for n_c in {min(rows_per, rows - c * rows_per) for c in (0, nch - 1)}:
        lane = max(lane, max(3 * m + t for m, t in (_lane_steps(n_c, g) for g in range(16))))
    return lane + 16 + (_cdiv(nch, 64) + 63 if typed else nch)


def colsum64(x, rows, cols, typed, out_dt=F, b_terms=None):
    """Column sums of the stored x [rows, cols] and their bound; b_terms: bounds of the terms themselves (none: they are inputs)."""
    X = x.double()
    s = X.sum(0)
    b = SLACK * cs_chain(rows, cols, typed) * U32 * X.abs().sum(0) + ETA * rows
    if b_terms is not None:
        b = b + b_terms.sum(0)
    return s, _store(b, s, out_dt)


def _cs_kernel32(x, rows_per, nch, stamps=None, defect=None):
    """colsum_kernel over fp32 values x [rows, cols] -> partials [nch, cols]: 16 row lanes per block, the main loop over 64 rows (four
    loads, (v0 + v1) + (v2 + v3), one addition into the accumulator; a dead tile skipped), the tail 16 rows at a time, then the lanes
    added in order."""
    rows, cols = x.shape
    S = _cdiv(rows_per, 64)
    xp = torch.zeros(nch, S * 64, cols, dtype=F)
    n_c = torch.zeros(nch, dtype=torch.int64)
    for c in range(nch):
        r0, r1 = c * rows_per, min(rows, (c + 1) * rows_per)
        xp[c, :r1 - r0] = x[r0:r1]
        n_c[c] = r1 - r0
    xp = xp.view(nch, S, 4, 16, cols)          # chunk, step, quarter, lane: row 64 s + 16 q + lane
    g = torch.arange(16)
    acc = torch.zeros(nch, 16, cols, dtype=F)
    for s in range(S):
        main = (g[None] + 64 * s + 48) < n_c[:, None]                      # [nch, 16]
        v = xp[:, s]
        four = (v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3])
        live = torch.ones(nch, dtype=torch.bool)
        if stamps is not None:
            tile = torch.arange(nch) * (rows_per // 64) + s
            if defect == "stamp_off_by_one_tile":
                tile = tile + 1
            live = stamps[tile.clamp_max(stamps.numel() - 1)] == CS_EPOCH
        acc = torch.where((main & live[:, None])[:, :, None], acc + four, acc)
        if defect != "tail_rows_dropped":
            for q in range(4):                                               # (rows beyond the chunk are zero padding: a + 0 is exact)
                acc = torch.where((~main)[:, :, None], acc + v[:, q], acc)
    part = torch.zeros(nch, cols, dtype=F)
    for k in range(16):
        part = part + acc[:, k]
    if defect == "last_column_block_dropped":
        part[:, (_cdiv(cols, 128) - 1) * 128:] = 0.0
    return part


def colsum_emulate32(x, typed, out_dt=F, stamps=None, defect=None, drop=None):
    """-> sums in out_dt (fp32 for the atomics, whose chunks are added here in chunk order), and with drop = (key, p) the masked x in
    its dtype first: the sums are then taken over the STORED values."""
    assert defect is None or defect in CS_DEFECTS
    rows, cols = x.shape
    xf, xd = x.float(), None
    if drop is not None:
        key, p = drop
        prod = xf * (keep_mask(key, rows * cols, p).view(rows, cols).float() * _c(drop_scale(p)))
        xd = prod.to(x.dtype)
        xf = prod if defect == "sums_of_unrounded_product" else xd.float()
    rows_per, nch = cs_grid(rows, cols, typed)
    part = _cs_kernel32(xf, rows_per, nch, stamps, defect)
    if typed:
        out = _ln_reduce32(part[:64] if defect == "chunks_from_64_dropped" else part).to(out_dt)   # colsum_reduce_kernel: ln_bwd_reduce_kernel's order
    else:
        out = torch.zeros(cols, dtype=F)
        for c in range(nch):
            out = out + part[c]
    return out if drop is None else (xd, out)


# ------------------------------------------------------------------------------------------------------------------------------------
# embedding forward: out = dropout(scale * src + pos_table[position])
# ------------------------------------------------------------------------------------------------------------------------------------
EF_T = [7, 64, 65, 130]            # the count loop j += 64 runs one, two and three rounds
EF_COLS = [8, 520]
EF_V = 20
EF_PS = [0.0, 0.1]
EF_KEY = 0xBEEF01
EF_FORMS = ("tokens", "mask", "ids+mask", "dense", "dense_no_table")
EF_DEFECTS = ("positions_count_pads", "pos_without_pad_idx", "pad_symbol_given_a_position", "scale_on_position_term", "count_truncated_at_64",
              "dropout_index_per_row")


def sinusoidal_table(num, dim, pad):
    """modules/sinusoidal_positional_embedding.py:36-58 (sin || cos, row `pad` zero), as oracle.sinusoidal_table states it."""
    half = dim // 2
    e = math.log(10000) / (half - 1)
    e = torch.exp(torch.arange(half, dtype=torch.float) * -e)
    e = torch.arange(num, dtype=torch.float).unsqueeze(1) * e.unsqueeze(0)
    e = torch.cat([torch.sin(e), torch.cos(e)], dim=1).view(num, -1)
    e[pad, :] = 0
    return e


def ef_tokens(T, seed=29):
    """[4, T] ids in [2, EF_V): row 0 has pads inside the sequence, row 1 is left-padded, row 2 is all pad, row 3 has no pad."""
    tok = torch.randint(2, EF_V, (4, T), generator=_gen(seed))
    tok[0, 3], tok[0, T // 2] = PAD, PAD
    tok[1, :T // 3 + 1] = PAD
    tok[2] = PAD
    return tok


def make_positions(nonpad, pad):
    """utils.make_positions: pad + (number of non-pad symbols up to and including t) for a non-pad symbol, pad for a pad."""
    m = nonpad.long()
    return torch.cumsum(m, 1) * m + pad


def ef_inputs(T, C, dt, seed=30):
    g = _gen(seed)
    tok = ef_tokens(T)
    E = (torch.randn(EF_V, C, generator=g) * C ** -0.5).to(dt)
    E[PAD] = 0
    x = torch.randn(4, T, C, generator=g).to(dt)
    return tok, E, x, sinusoidal_table(PAD + 1 + T, C, PAD)


def ef_args(form, tok, E, x, table):
    """(tokens, pad_mask, embed, x, table) of a form; the mask is uint8 with 1 at pads (it is compared with pad_idx = 1)."""
    mask = tok.eq(PAD).to(torch.uint8)
    return {"tokens": (tok, None, E, None, table), "mask": (None, mask, None, x, table), "ids+mask": (tok, mask, E, None, table),
            "dense": (tok, None, None, x, table), "dense_no_table": (None, None, None, x, None)}[form]


def _ef_pos(tokens, mask, pad, T, defect=None):
    nonpad = mask.ne(pad) if mask is not None else tokens.ne(pad)
    if defect == "positions_count_pads":
        return torch.where(nonpad, pad + 1 + torch.arange(T)[None].expand_as(nonpad), torch.full_like(nonpad, pad, dtype=torch.int64))
    if defect == "count_truncated_at_64":      # one round of the 64 lanes: symbols 0 .. min(t, 63)
        c = torch.cumsum(nonpad.long(), 1)
        c = torch.where(torch.arange(T)[None] > 63, c[:, min(63, T - 1):min(63, T - 1) + 1], c)
        return c * nonpad.long() + pad
    if defect == "pos_without_pad_idx":
        return torch.where(nonpad, torch.cumsum(nonpad.long(), 1), torch.full_like(nonpad, pad, dtype=torch.int64))
    if defect == "pad_symbol_given_a_position":
        return torch.cumsum(nonpad.long(), 1) + pad
    return make_positions(nonpad, pad)


def embed_fwd64(tokens, mask, E, x, table, scale, p, key):
    """-> (out fp64 [B, T, C], bound).  v = fmaf(scale, src, pe): one rounding on |v| (without a table the product: one); the dropout
    factor one more at p > 0; the store."""
    src = (E[tokens] if E is not None else x).double()
    Bn, T, C = src.shape
    v = f32(scale) * src
    if table is not None:
        v = v + table.double()[_ef_pos(tokens, mask, PAD, T)]
    dt = (E if E is not None else x).dtype
    keep = keep_mask(key, Bn * T * C, p).view(Bn, T, C) if p > 0 else torch.ones(Bn, T, C, dtype=torch.bool)
    y = v * _factor(keep, p)
    return y, _store(SLACK * U32 * ((drop_scale(p) if p > 0 else 1.0) * v.abs() * keep + (y.abs() if p > 0 else 0.0)) + ETA * keep, y, dt)


def embed_fwd_emulate32(tokens, mask, E, x, table, scale, p, key, defect=None):
    assert defect is None or defect in EF_DEFECTS
    src = (E[tokens] if E is not None else x)
    dt = src.dtype
    src = src.float()
    Bn, T, C = src.shape
    s = _c(f32(scale))
    if table is not None:
        pe = table[_ef_pos(tokens, mask, PAD, T, defect)]
        v = s * (src + pe) if defect == "scale_on_position_term" else _fma(s, src, pe)
    else:
        v = s * src
    if p > 0:
        idx = np.arange(Bn * T * C, dtype=np.uint64)
        if defect == "dropout_index_per_row":
            idx = idx // np.uint64(C) + idx % np.uint64(C)
        v = v * (keep_mask(key, Bn * T * C, p, idx).view(Bn, T, C).float() * _c(drop_scale(p)))
    return v.to(dt)


# ------------------------------------------------------------------------------------------------------------------------------------
# embedding backward: dE[v] = scale * sum over the occurrences j of v (index order) of keep_j dy[j]
# ------------------------------------------------------------------------------------------------------------------------------------
EB_CASES = [(21, 8, 12), (700, 64, 40), (300, 2056, 50), (64, 8192, 9)]     # (n, C, V): vector slots 1, 1, 2, 4
EB_PS = [0.0, 0.1]
EB_KEY = 0xBEEF02
EB_DEFECTS = ("occurrences_after_first_pass_dropped", "owner_search_truncated_at_256", "vector_slots_from_1_dropped", "gradient_on_pad_row",
              "scale_missing", "mask_of_wrong_row")


def eb_tokens(n, V, seed=31):
    """ids in [2, V - 2) (rows 0, V - 2, V - 1 stay unused), pads at every 7th place from 4.  n = 700: symbols recur more than 256
    places apart; symbol V - 5 first occurs at 300 and again at 650, V - 4 at 260 and 699 — first occurrences behind the first
    pass of 256 ids of the owner search, with other symbols before them."""
    hi = V - 5 if n == 700 else V - 2
    tok = torch.randint(2, hi, (n,), generator=_gen(seed))
    tok[4::7] = PAD
    if n == 700:
        tok[300], tok[650], tok[260], tok[699] = V - 5, V - 5, V - 4, V - 4
    return tok


def eb_inputs(n, C, V, dt, seed=32):
    return torch.randn(n, C, generator=_gen(seed)).to(dt), eb_tokens(n, V)


def embed_bwd64(dy, tok, V, scale, p, key, grad_dt):
    """-> (dE fp64 [V, C], bound).  A row with m occurrences: m - 1 additions that round, the dropout factor (p > 0) and the product
    with scale one each, on scale * sum |terms|; the store in the gradient dtype.  The pad row and unused rows: exactly 0."""
    n, C = dy.shape
    g = dy.double()
    if p > 0:
        g = g * _factor(keep_mask(key, n * C, p).view(n, C), p)
    live = tok.ne(PAD)
    s = f32(scale)
    dE = torch.zeros(V, C, dtype=torch.float64).index_add_(0, tok[live], g[live]) * s
    ab = torch.zeros(V, C, dtype=torch.float64).index_add_(0, tok[live], g[live].abs()) * s
    occ = torch.bincount(tok[live], minlength=V)
    k = ((occ - 1).clamp_min(0) + (1 if p > 0 else 0) + 1).double()[:, None]
    return dE, _store(SLACK * k * U32 * ab + ETA * (occ > 0)[:, None], dE, grad_dt)


def embed_bwd_emulate32(dy, tok, V, scale, p, key, grad_dt, defect=None):
    assert defect is None or defect in EB_DEFECTS
    n, C = dy.shape
    g = dy.float()
    if p > 0:
        idx = np.arange(n * C, dtype=np.uint64)
        if defect == "mask_of_wrong_row":
            idx = idx + np.uint64(C)
        g = g * (keep_mask(key, n * C, p, idx).view(n, C).float() * _c(drop_scale(p)))
    acc = torch.zeros(V, C, dtype=F)
    first = {}
    for j in range(n):
        t = int(tok[j])
        if t == PAD and defect != "gradient_on_pad_row":
            continue
        first.setdefault(t, j)
        if defect == "occurrences_after_first_pass_dropped" and j >= first[t] + 256:
            continue
        if defect == "owner_search_truncated_at_256" and j >= 256 and j > first[t] >= 256:
            acc[t] = 0.0          # this occurrence finds no earlier one among the first 256 ids, takes the row and writes it last
        acc[t] = acc[t] + g[j]
    if defect != "scale_missing":
        acc = acc * _c(f32(scale))
    if defect == "vector_slots_from_1_dropped":
        acc[:, 2048:] = 0.0
    return acc.to(grad_dt)


# ------------------------------------------------------------------------------------------------------------------------------------
# contrastive term (csrc/loss_optim.hip): c[i][j] = a_i . t_j / max(|a_i| |t_j|, 1e-8), L = c / temp,
#   loss = sum_b sum_j (logsumexp_i L[i][j] - L[j][j]);  G = g (softmax_i L - I),  W = G / max(|a||t|, 1e-8),
#   da_i = sum_j W[i][j] t_j - r_a[i] a_i / |a_i|^2,  r_a[i] = sum_j G c;   dt_j = sum_i W[i][j] a_i - r_t[j] t_j / |t_j|^2
# ------------------------------------------------------------------------------------------------------------------------------------
CT_SHAPES = [(1, 1, 8), (2, 8, 64), (1, 33, 72), (3, 64, 512), (2, 63, 40)]
CT_TEMPS = [0.1, 0.05]
CT_GSCALES = [1.0, 0.7]
CT_FWD_DEFECTS = ("softmax_over_text", "target_j_plus_1", "channel_tail_dropped")
CT_BWD_DEFECTS = ("softmax_over_text", "da_without_projection", "no_inv_temp", "target_j_plus_1", "second_channel_slice_dropped")


def ct_inputs(Bn, M, C, dt, seed=33, zero_row=False):
    """a N(0, 1), t = 0.5 a + N(0, 1).  In utterance 0: slot 0 nearly parallel (cos ~ 1 - 1e-6), slot 1 nearly antiparallel, audio slot 2
    scaled by 1e3, text slot 3 by 1e-3 (where M has them).  zero_row: audio slot M - 1 and text slot 0 of the last utterance all zero."""
    g = _gen(seed)
    a = torch.randn(Bn, M, C, generator=g)
    t = 0.5 * a + torch.randn(Bn, M, C, generator=g)
    n = torch.randn(2, C, generator=g)
    t[0, 0] = a[0, 0] + 1.4e-3 * n[0] * float(a[0, 0].norm()) / float(n[0].norm())
    if M > 1:
        t[0, 1] = -a[0, 1] + 1.4e-3 * n[1] * float(a[0, 1].norm()) / float(n[1].norm())
    if M > 3:
        a[0, 2] *= 1e3
        t[0, 3] *= 1e-3
    if zero_row:
        a[-1, M - 1] = 0.0
        t[-1, 0] = 0.0
    return a.to(dt), t.to(dt)


def inv_temp32(temp):
    """The launcher's 1.0f / temp."""
    return float(np.float32(1.0) / np.float32(temp))


def ct_fwd64(a, t, temp):
    A, T = a.double(), t.double()
    it = inv_temp32(temp)
    dot = A @ T.transpose(1, 2)
    adot = A.abs() @ T.abs().transpose(1, 2)
    na, nt = (A * A).sum(2).sqrt(), (T * T).sum(2).sqrt()
    den = (na[:, :, None] * nt[:, None, :]).clamp_min(1e-8)
    sim = dot / den
    L = sim * it
    lse = torch.logsumexp(L, 1)                       # over the audio slot i, per text slot j
    l = lse - torch.diagonal(L, dim1=1, dim2=2)
    rows = l.sum(1)
    return dict(sim=sim, na=na, nt=nt, rows=rows, loss=rows.sum(), L=L, lse=lse, l=l, adot=adot, den=den, it=it, C=a.shape[2],
                clamped=(na[:, :, None] * nt[:, None, :]) < 1e-8)


def ct_fwd_bounds(r):
    """q = sum x^2 and the dot products: chains of C fmaf (zero padding to 32 channels adds exact zeros).  |x| = sqrtf(q): C / 2 +
    INTRIN.  den = fl(|a| |t|): both, 1 (a clamped den is the constant).  c = dot / den: C u sum |a t| / den, the error of den and
    INTRIN on |c|.  L = fl(c / temp): 1.  Per text slot j, with p the softmax over i and x_i = L_i - max: errors of the L enter lse
    with weights p; every exponential carries INTRIN + 3 |x_i| (the difference, the rounded log2 e and its product), the sum M, __logf
    INTRIN on |log se|, max + log 1 on |lse|, minus L_jj: its error, 1 on |l|.  A row: block_sum's 10 on sum |l|; the loss: the rows added
    in double, one rounding."""
    u, C, it = U32, r["C"], r["it"]
    M = r["sim"].shape[1]
    rel_n = (0.5 * C + INTRIN) * u
    b_na, b_nt = SLACK * r["na"] * rel_n + ETA, SLACK * r["nt"] * rel_n + ETA
    rel_den = torch.where(r["clamped"], torch.zeros_like(r["den"]), torch.full_like(r["den"], 2 * rel_n + u))
    b_c = SLACK * (C * u * r["adot"] / r["den"] + r["sim"].abs() * (rel_den + INTRIN * u)) + ETA
    L = r["L"]
    b_L = it * b_c + u * L.abs()
    p = torch.softmax(L, 1)
    x = (L - L.max(1, keepdim=True).values).abs()
    se = torch.exp(r["lse"] - L.max(1).values)
    b_l = SLACK * ((p * b_L).sum(1) + u * (p * (INTRIN + 3.0 * x)).sum(1) + M * u + INTRIN * u * se.log().abs() + u * r["lse"].abs()
                   + torch.diagonal(b_L, dim1=1, dim2=2) + u * r["l"].abs()) + ETA
    b_rows = b_l.sum(1) + SLACK * BLOCK_SUM_ADDS * u * r["l"].abs().sum(1)
    return dict(sim=b_c, na=b_na, nt=b_nt, rows=b_rows, loss=b_rows.sum() + u * r["loss"].abs() + ETA)


def _block_sum_rows32(l):
    """block_sum over 256 threads of which the first M hold a value: wave_sum, then the four waves in order."""
    Bn, M = l.shape
    v = torch.zeros(Bn, 256, dtype=F)
    v[:, :M] = l
    return _block_sum32(v)


def _ct_logits32(S, it, transpose):
    """Per column j: L, max and the sum of exponentials in the order i = 0 .. M - 1."""
    L = S * it
    if transpose:
        L = L.transpose(1, 2)
    mx = L.max(1, keepdim=True).values
    E = torch.exp(L - mx)
    se = torch.zeros_like(E[:, 0])
    for i in range(E.shape[1]):
        se = se + E[:, i]
    return L, mx.squeeze(1), E, se


def ct_fwd_emulate32(a, t, temp, defect=None):
    """-> loss (fp32 scalar), loss_rows, sim, na, nt."""
    assert defect is None or defect in CT_FWD_DEFECTS
    A, T = a.float(), t.float()
    Bn, M, C = A.shape
    Cu = C // 32 * 32 if defect == "channel_tail_dropped" else C
    acc, qa, qt = torch.zeros(Bn, M, M, dtype=F), torch.zeros(Bn, M, dtype=F), torch.zeros(Bn, M, dtype=F)
    for c in range(Cu):
        x, y = A[:, :, c], T[:, :, c]
        qa, qt = _fma(x, x, qa), _fma(y, y, qt)
        acc = _fma(x[:, :, None], y[:, None, :], acc)
    na, nt = qa.sqrt(), qt.sqrt()
    S = acc / (na[:, :, None] * nt[:, None, :]).clamp_min(1e-8)
    it = _c(inv_temp32(temp))
    L, mx, _, se = _ct_logits32(S, it, defect == "softmax_over_text")
    j = torch.arange(M)
    diag = S[:, (j + 1) % M, j] if defect == "target_j_plus_1" else S[:, j, j]
    l = mx + se.log() - diag * it
    rows = _block_sum_rows32(l)
    return rows.double().sum().float(), rows, S, na, nt


def ct_bwd64(a, t, sim, na, nt, gscale, temp):
    """A function of what the kernel receives: the fp32 sim, |a|, |t| of the forward, the fp32 gscale."""
    A, T, S = a.double(), t.double(), sim.double()
    it = inv_temp32(temp)
    g = f32(gscale) * it
    Na, Nt = na.double().clamp_min(1e-12), nt.double().clamp_min(1e-12)
    den = (Na[:, :, None] * Nt[:, None, :]).clamp_min(1e-8)
    L = S * it
    P = torch.softmax(L, 1)
    eye = torch.eye(S.shape[1], dtype=torch.float64)[None]
    G = g * (P - eye)
    ra, rt = (G * S).sum(2), (G * S).sum(1)
    W = G / den
    da = W @ T - (ra / (Na * Na))[:, :, None] * A
    dt_ = W.transpose(1, 2) @ A - (rt / (Nt * Nt))[:, :, None] * T
    return dict(da=da, dt=dt_, A=A, T=T, S=S, L=L, P=P, G=G, W=W, ra=ra, rt=rt, Na=Na, Nt=Nt, den=den, g=g, eye=eye)


def ct_bwd_bounds(r, dt):
    """L = fl(S / temp) 1.  E_i = __expf(fl(L_i - max)): the two L, the difference, log2 e and its product — |L_i| + |max| + 3 |x_i| —
    and INTRIN.  se: the terms' errors weighted by p, M for the chain.  P = E / se: INTRIN.  G = fl(g fl(P - [i = j])): g = fl(gscale /
    temp) 1, the difference 1, the product 1.  r_a, r_t = sum G c: the product and M additions on sum |G c|.  W = G / max(fl(|a||t|),
    1e-8): 1 + INTRIN.  x = sum_j W t_j: M fmaf on sum |W t|.  The projection r a / fl(|a|^2): the error of r, products 2, INTRIN;
    the difference 1 on the result; the store."""
    u = U32
    S, L, P, G, W = r["S"].abs(), r["L"], r["P"], r["G"].abs(), r["W"].abs()
    M = S.shape[1]
    mx = L.max(1, keepdim=True).values
    rho = u * (L.abs() + mx.abs() + 3.0 * (L - mx).abs() + INTRIN)
    rel_P = rho + (P * rho).sum(1, keepdim=True) + (M + INTRIN) * u
    b_G = SLACK * (abs(r["g"]) * P * rel_P + 3.0 * u * G)
    GS = G * S
    b_ra = b_G.mul(S).sum(2) + (M + 1) * u * GS.sum(2)
    b_rt = b_G.mul(S).sum(1) + (M + 1) * u * GS.sum(1)
    b_W = b_G / r["den"] + (1 + INTRIN) * u * W
    out = {}
    for name, X, Y, Wm, bW, rr, b_r, N in (("da", r["A"], r["T"], W, b_W, r["ra"], b_ra, r["Na"]),
                                           ("dt", r["T"], r["A"], W.transpose(1, 2), b_W.transpose(1, 2), r["rt"], b_rt, r["Nt"])):
        proj = (rr / (N * N))[:, :, None] * X
        b_x = bW @ Y.abs() + M * u * (Wm @ Y.abs())
        b_p = (b_r / (N * N))[:, :, None] * X.abs() + (2 + INTRIN) * u * proj.abs()
        out[name] = _store(SLACK * (b_x + b_p + u * r[name].abs()) + ETA, r[name], dt)
    return out


def ct_bwd_emulate32(a, t, sim, na, nt, gscale, temp, defect=None):
    """-> da, dt in the dtype of a."""
    assert defect is None or defect in CT_BWD_DEFECTS
    dtp = a.dtype
    A, T, S = a.float(), t.float(), sim
    Bn, M, C = A.shape
    it = _c(inv_temp32(temp))
    g = _c(f32(gscale)) if defect == "no_inv_temp" else _c(f32(gscale)) * it
    Na, Nt = na.clamp_min(1e-12), nt.clamp_min(1e-12)
    tr = defect == "softmax_over_text"
    _, _, E, se = _ct_logits32(S, it, tr)
    P = E / se[:, None, :]
    if tr:
        P = P.transpose(1, 2)
    j = torch.arange(M)
    tgt = torch.zeros(M, M, dtype=F)
    tgt[(j + 1) % M if defect == "target_j_plus_1" else j, j] = 1.0
    G = g * (P - tgt[None])
    rt, ra = torch.zeros(Bn, M, dtype=F), torch.zeros(Bn, M, dtype=F)
    for i in range(M):
        rt = rt + G[:, i, :] * S[:, i, :]
    for k in range(M):
        ra = ra + G[:, :, k] * S[:, :, k]
    W = G / (Na[:, :, None] * Nt[:, None, :]).clamp_min(1e-8)
    xa, xt = torch.zeros(Bn, M, C, dtype=F), torch.zeros(Bn, M, C, dtype=F)
    for k in range(M):
        xa = _fma(W[:, :, k][:, :, None], T[:, k][:, None, :], xa)
        xt = _fma(W[:, k, :][:, :, None], A[:, k][:, None, :], xt)
    da = xa if defect == "da_without_projection" else xa - ra[:, :, None] * A / (Na * Na)[:, :, None]
    dt_ = xt - rt[:, :, None] * T / (Nt * Nt)[:, :, None]
    if defect == "second_channel_slice_dropped":
        da[:, :, 64:128] = 0.0
        dt_[:, :, 64:128] = 0.0
    return da.to(dtp), dt_.to(dtp)


# ------------------------------------------------------------------------------------------------------------------------------------
# cached cases (the CPU and the GPU tests use the same tensors)
# ------------------------------------------------------------------------------------------------------------------------------------
glu_case = functools.lru_cache(maxsize=None)(glu_inputs)
wn_case = functools.lru_cache(maxsize=None)(wn_inputs)
cs_case = functools.lru_cache(maxsize=None)(cs_inputs)
