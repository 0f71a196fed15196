"""fp64 reference, exact expected bits, counted bounds, fp32 emulations and index-level defects of cst_gemm (csrc/gemm.hip, gemm8p.hip,
gemm4w.hip) on every launch arm gemm_route can return without the experiment hook.  Plain torch on the CPU; shared by
test_gemm_ref_cpu.py (routes, launcher arithmetic, the premise of exactness, the bounds, every defect leaves its case) and
test_gemm_parity_gpu.py (the kernels).  Built like posconv_ref.py, whose norm_ref pieces are used here; nothing about the GELU is restated.

A case is a row in the notation of test_gemm_route_cpu.py plus what that notation does not carry (act kind, drop p, dead blocks, per-batch
limits), the route text it exists to reach, and its kind:

  exact    A and B hold signed non-zero small integers (bf16-exact).  Their products are exact, every partial sum stays below 2^24 and is
           therefore exact in fp32 in ANY order, tree or split; alpha is a power of two, bias / residual are integers, ReLU, ReLU' and
           dropout at p = 0.5 (scale 2) are exact.  The only rounding is the one store — on gemm8p's fast path and gemm4w also the
           documented bf16 rounding of the pre-activation, see "image" below — a round-to-nearest-even of a known number: the
           expected BITS follow from an fp64 matmul.  The magnitude sets shrink with K (magnitudes()) so that at most 2 % of the bf16
           outputs reach 256, where the bf16 spacing exceeds 1 and the store could hide a unit error; both conditions are asserted.
  bounded  random normal operands (B scaled by K^-1/2), GELU / GELU' / a general alpha, some with full-mantissa fp32 operands.  Bounds:
             v = alpha acc + bias   the accumulator in ANY order: a sum of n terms passes at most n - 1 roundings per term.  n = K products,
                                    + 1 with a bias (gemm8p's fast epilogue seeds the accumulators with the bias row; counting the bias as a
                                    term of the sum covers that order and the add-afterwards of epilogue_store), + 1 rounding per term for
                                    the product of fp32 operands, + 1 per K slice (the reduce kernel's additions); the product with an alpha
                                    that is no power of two 1 on |alpha acc|; the bias add 1 on |v|
             aux_out                the store of v
             image                  gemm8p's fast epilogue and gemm4w only (o["image"]): the bf16 rounding of v into the LDS image, which
                                    the steps below then act on (their headers: "one bf16 rounding (this is the pre-activation z)")
             act                    GELU: norm_ref._gelu_arg_bound; ReLU: 1-Lipschitz, no rounding
             dropout                the product 1 (scale 2 is exact, still counted)
             act'(aux_in)           aux_in is an exact input: a_dgelu on |y|, the product 1
             resid                  1 on the sum;  C: the store
             colsum                 ORDER-FREE: (K - 1 + slices) u32 sum |a| — no chain length is read from a kernel — and the store
           No constant is fitted to a kernel's or an emulation's output.

Storage: operands are flat buffers read through strided views, exactly as include/cst.h states the addressing (overlapping rows, segments,
batch strides).  aux_out / aux_in / resid share C's geometry (leading dimension ldc, the batch offsets of C).  C, aux_out and colsum are
prefilled with NaN where the launch must write and with SENT where it must not (columns N .. ldc - 1, the gaps between strided batches)."""
import functools
import zlib

import torch

from norm_ref import ETA, SLACK, U32, _colsum_bound, _gelu_arg_bound, _store, a_dgelu, dgelu32, dgelu64, gelu32, gelu64, worst_ratio  # noqa: F401
from test_gemm_route_cpu import parse

BF, F32 = torch.bfloat16, torch.float32
SENT = 777.0
NONE, RELU, GELU = 0, 1, 2      # lib.ACT_*
EPOCH = 0x5A17C3E1              # the stamps of a live block; dead blocks hold EPOCH - 1, "the epoch of another launch"
DROP_KEY = 0x1234ABCD
GROUP_M = 4                     # gemm_switches(): m tiles per group of the persistent walk


def _c(name, row, route, kind="exact", **extra):
    return dict(name=name, row=row, route=route, kind=kind, **extra)


R128, R256, RN = "128x128 nt256", "256x256 nt1024", "64x128 nt256"
_8P = "3592 3608 72 "           # 15 x 15 = 225 tiles of 256 x 256: one round on 256 CUs
# (variant, flags, 8p epilogue mode)
_8P_VARIANTS = [("plain", "", 1), ("bias_act_aux", "bias act aux_out", 1), ("bias_act_aux_alpha", "bias act aux_out alpha=0.5", 0), ("resid", "resid", 2), ("dact", "dact", 2), ("cf32", "cf32", 0),
                ("biasrow", "biasrow", 0), ("bias_alpha", "bias alpha=0.5", 0), ("drop", "drop", 1), ("split2", "split=2", 0),
                ("ldc", "ldc=3616", 1)]

CASES = [
    # ---- register-staged kernel ----
    _c("reg_mm", "136 136 200 mm", "reg bf16 mm %s split1" % R128),
    _c("reg_km", "136 136 200 km", "reg bf16 km %s split1" % R128),
    _c("reg_mk", "136 136 200 mk", "reg bf16 mk %s split1" % R128),
    _c("reg_mm_colsum", "136 136 200 mm colsum", "reg bf16 mm %s colsum split1" % R128),
    _c("reg_mm_colsum_split8", "136 264 4104 mm colsum", "reg bf16 mm %s colsum split8" % R128),   # fused sums through the reduce kernel
    _c("reg_mm_split8", "520 520 4104 mm", "reg bf16 mm %s split8" % R128),                        # unbatched split: split_order walk
    _c("reg_mm_split8_epi", "520 520 4104 mm bias act resid", "reg bf16 mm %s split8" % R128),       # the reduce kernel's epilogue
    _c("reg_km_alpha", "136 136 200 km bias act alpha=-2", "reg bf16 km %s split1" % R128),          # a negative alpha
    _c("reg_klen_split1", "136 136 4104 mm b0=4 k_len cf32 split=1", "reg bf16 mm %s split1" % R128, k_len=(4104, 1000, 1, 0)),
    _c("reg_klen_split2", "136 136 4104 mm b0=4 k_len cf32 split=2", "reg bf16 mm %s split2" % R128, k_len=(4104, 1000, 1, 0)),
    _c("narrowm", "64 264 136 mm", "reg bf16 mm %s split1" % RN),
    _c("narrowm_colsum", "64 264 136 mm colsum", "reg bf16 mm %s colsum split1" % RN),
    _c("narrowm_klive", "48 264 4104 mm b1=2 cf32 split=1 colsum k_live", "reg bf16 mm %s colsum split1" % RN, dead_k=(1, 2, 7, 30, 64)),
    _c("reg_km_mlive", "520 264 200 km m_live", "reg bf16 km %s split1" % R128, dead_m=(0, 1, 4, 5, 8)),   # m tile 0 wholly dead
    _c("reg_km_mlen", "520 264 200 km b0=2 m_len split=1 bias resid", "reg bf16 km %s split1" % R128, m_len=(300, 0)),   # tiles behind the limit: epilogue(0)
    _c("reg_seg", "264 136 128 kk a_seg=64 a_seg_stride=256", "reg bf16 kk seg %s split1" % R128),
    _c("large_mm", "3592 3608 72 mm", "reg bf16 mm %s split1" % R256),
    _c("large_mk", "3592 3608 72 mk", "reg bf16 mk %s split1" % R256),
    _c("large_split3", "3592 3608 200 mm split=3", "reg bf16 mm %s split3" % R256),
    _c("large_split3_colsum", "3592 3608 200 mm colsum split=3", "reg bf16 mm %s split3" % R256),   # the SEPARATE column sum
    _c("large_colsum", "3592 3608 72 mm colsum", "reg bf16 mm %s split1" % R256),
    _c("large_colsum_klive", "3592 3608 200 mm colsum split=3 k_live", "reg bf16 mm %s split3" % R256, dead_k=(0, 2)),
    _c("large_auto3", "2056 2056 3080 mm", "reg bf16 mm %s split3" % R256),
    _c("f32_mm", "136 136 100 mm f32", "reg f32 mm %s split1" % R128),
    _c("f32_km", "136 132 100 km f32", "reg f32 km %s split1" % R128),                              # N % 8 != 0: the scalar epilogue_store
    _c("f32_km_drop", "136 132 100 km f32 bias drop", "reg f32 km %s split1" % R128),               # cst_drop1 in the scalar epilogue_store
    _c("f32_mm_colsum_split8", "136 136 2056 mm f32 colsum", "reg f32 mm %s colsum split8" % R128),
    _c("f32_large_km", "3592 3608 40 km f32", "reg f32 km %s split1" % R256),
    # ---- DMA ring ----
    _c("glds_skinny4", "136 136 200 kk", "glds bf16 kk 64x64 nt256 ns4 split1"),
    _c("glds_conv", "300 136 192 kk lda=128", "glds bf16 kk 64x64 nt256 ns4 split1"),              # overlapping rows: the implicit conv
    _c("glds_skinny2", "1544 1416 72 kk", "glds bf16 kk 64x64 nt256 ns2 split1"),
    _c("glds_skinny2_epi", "1544 1416 72 kk bias act aux_out resid", "glds bf16 kk 64x64 nt256 ns2 split1"),
    _c("glds_mlive", "1544 1416 72 kk m_live resid", "glds bf16 kk 64x64 nt256 ns2 split1", dead_m=(0, 3, 4, 5, 24)),
    _c("glds_skinny2_drop", "1544 1416 72 kk bias act resid drop", "glds bf16 kk 64x64 nt256 ns2 split1"),   # cst_drop8 in epilogue_store8
    _c("glds_biasrow", "136 136 200 kk biasrow", "glds bf16 kk 64x64 nt256 ns4 split1"),                     # the row bias in epilogue_store8
    _c("glds_small", "2056 2056 72 kk", "glds bf16 kk %s ns2 split1" % R128),
    _c("glds_batched", "70 40 72 kk b0=3 b1=2 bias", "glds bf16 kk %s ns2 split1" % R128, shared_b=True),   # B and bias per batch1 only
    _c("glds_narrown", "264 48 136 kk b0=3 b1=2 lda=48 ldc=768 bias act aux_out resid split=1 m_len", "glds bf16 kk 128x64 nt256 ns2 split1",
       m_len=(264, 130, 0)),
    _c("glds_large", "3592 3608 72 kk dact resid", "glds bf16 kk %s ns2 split1" % R256),
    _c("glds_f32_skinny", "136 136 100 kk f32", "glds f32 kk 64x64 nt256 ns4 split1"),
    _c("glds_f32_split2", "1000 768 512 kk f32", "glds f32 kk %s ns2 split2" % R128),
    _c("glds_f32_large", "3592 3608 40 kk f32", "glds f32 kk %s ns2 split1" % R256),
]
for _lay in ("kk", "km"):
    for _v, _fl, _mode in _8P_VARIANTS:
        CASES.append(_c("8p_%s_%s" % (_lay, _v), (_8P + _lay + " " + _fl).strip(), "8p " + _lay, mode=_mode,
                        state=dict(tiles=450, half_from=None, claims=True) if "split" in _fl else dict(tiles=225)))
CASES += [
    _c("8p_kk_drop_ldc", _8P + "kk drop ldc=3616", "8p kk", mode=1),      # the mask index is row N + col, not row ldc + col
    # 17 x 16 = 272 tiles: on 256 CUs the 16 tiles of the second round run as 32 half items, every item after the first is claimed
    _c("8p_kk_tail", "4300 4096 72 kk", "8p kk", mode=1, state=dict(tiles=272, half_from=256, nitems=288, claims=True)),
    _c("8p_km_tail", "4300 4096 72 km", "8p km", mode=1, state=dict(tiles=272, half_from=256, nitems=288, claims=True)),
    _c("8p_kk_tail_mlive", "4300 4096 72 kk m_live", "8p kk", mode=1, dead_m=tuple(range(4, 13)) + (20, 22, 60, 66, 67),
       state=dict(tiles=272, half_from=256, nitems=288, claims=True)),
    # a skipped K loop through the image epilogue (not the zero-store shortcut): the residual / the bias seed on zero accumulators
    _c("8p_kk_mlive_resid", _8P + "kk m_live resid", "8p kk", mode=2, dead_m=tuple(range(4, 13)) + (20, 55, 56), state=dict(tiles=225)),
    _c("8p_kk_mlive_bias", _8P + "kk m_live bias", "8p kk", mode=1, dead_m=tuple(range(4, 13)) + (20, 55, 56), state=dict(tiles=225)),
    _c("8p_kk_scalar_epi", "4300 4100 72 kk", "8p kk", mode=0, state=dict(tiles=289)),              # N % 8 != 0: the scalar epilogue
    _c("8p_mrot", "1100 2568 192 kk b0=4 lda=128 m_len split=1", "8p kk", mode=1, m_len=(1100, 700, 256, 0),
       state=dict(tiles=220, gperm_full=0, mrot=6)),
    _c("8p_gperm", "16400 264 192 kk b0=2 lda=128 m_len split=1", "8p kk", mode=1, m_len=(16400, 9000), state=dict(tiles=260, gperm_full=16, mrot=0)),
    _c("8p_gperm_epi", "16400 264 192 kk b0=2 lda=128 m_len split=1 act aux_out", "8p kk", mode=1, m_len=(16400, 9000),
       state=dict(tiles=260, gperm_full=16, mrot=0)),
    # ---- four-wave kernel: 64 x 4 = 256 tiles of 256 x 192 exactly, ragged last m tile ----
    _c("4w_bias_resid", "16284 768 1536 kk bias resid", "4w"),
    _c("4w_bias_resid_drop", "16284 768 1536 kk bias resid drop", "4w"),
    _c("4w_mlive_resid", "16284 768 1536 kk m_live resid", "4w", dead_m=tuple(range(8, 20)) + (33, 100, 254)),
    _c("4w_k1600", "16284 768 1600 kk", "4w"),
    _c("4w_two_rounds", "24100 768 1536 kk resid", "4w"),                                           # 380 tiles: a second round, 124 full
    _c("8p_not_4w_alpha", "16284 768 1536 kk bias alpha=0.5", "8p kk", mode=0),                      # the conditions that turn 4w down
    _c("8p_not_4w_act", "16284 768 1536 kk act", "8p kk", mode=1),
    # mode 2 at a K whose sums reach 256: the image rounding of z and the residual's second rounding both show
    _c("8p_not_4w_act_resid", "16284 768 1536 kk act resid", "8p kk", mode=2),
    # ---- bounded: one per epilogue code path ----
    _c("b_scalar_epi_f32", "136 132 100 km f32 bias act aux_out resid", "reg f32 km %s split1" % R128, "bounded", act=GELU),
    _c("b_store8", "1544 1416 72 kk bias act aux_out resid", "glds bf16 kk 64x64 nt256 ns2 split1", "bounded", act=GELU),
    _c("b_reduce", "520 520 4104 mm bias act alpha=0.3", "reg bf16 mm %s split8" % R128, "bounded", act=GELU),
    _c("b_reduce_colsum", "136 264 4104 mm colsum", "reg bf16 mm %s colsum split8" % R128, "bounded"),
    _c("b_f32_split2", "1000 768 512 kk f32", "glds f32 kk %s ns2 split2" % R128, "bounded"),
    _c("b_f32_colsum_split8", "136 136 2056 mm f32 colsum", "reg f32 mm %s colsum split8" % R128, "bounded"),
    _c("b_8p_mode0", _8P + "kk bias act aux_out alpha=0.3", "8p kk", "bounded", act=GELU, mode=0),
    _c("b_8p_mode1_epi", _8P + "kk bias act aux_out", "8p kk", "bounded", act=GELU, mode=1),      # the bias row seeds the accumulators
    _c("b_8p_mode1", _8P + "kk", "8p kk", "bounded", mode=1),
    _c("b_8p_mode2", _8P + "kk dact", "8p kk", "bounded", dact=GELU, mode=2),
    _c("b_8p_alpha", _8P + "km bias alpha=0.3", "8p km", "bounded", mode=0),
    _c("b_4w_resid", "16284 768 1536 kk resid", "4w", "bounded"),
]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def arm_of(route):
    """The launch arm of a route text: the text without storage dtype, ' colsum' and the split count."""
    return " ".join(w for w in route.split() if w not in ("bf16", "f32", "colsum") and not w.startswith("split"))


def tile_of(route):
    """(BM, BN, half height or 0) of the arm: what the mismatch map is drawn in."""
    if route.startswith("8p"):
        return 256, 256, 128
    if route == "4w":
        return 256, 192, 0
    bm, bn = next(w for w in route.split() if "x" in w and w[0].isdigit()).split("x")
    return int(bm), int(bn), 0


def launch8p_state(M, N, nbatch, splits, has_m_len, ncu=256, reserved=0, no_halves=False):
    """gemm8p.hip: launch8p's arithmetic, restated from its rules."""
    tiles_m, tiles_n = -(-M // 256), -(-N // 256)
    nz = nbatch * splits
    total = tiles_m * tiles_n * nz
    ntl = tiles_m * tiles_n
    gfull = tiles_m // GROUP_M
    gperm_full = gfull if (has_m_len and gfull >= 16) else 0
    mrot = (max(ntl // 8, 1) if (has_m_len and gperm_full == 0 and ntl >= 2) else 0)
    avail = max(ncu - reserved, 8)
    nitems, half_from = total, None
    if not no_halves and nz == 1 and total > avail:
        r = total % avail
        if r > 0 and 2 * r <= avail:
            half_from, nitems = total - r, total + r
    grid = min(nitems, avail)
    return dict(tiles=total, avail=avail, half_from=half_from, nitems=nitems, grid=grid, claims=nitems > avail and grid % 8 == 0,
                gperm_full=gperm_full, mrot=mrot)


def tile_of_item8p(v, st, tiles_m, tiles_n):
    """gemm8p.hip: setup()'s work item -> (m tile, n tile, half or -1) of an unbatched launch without row limits: item v of the grid-stride
    walk belongs to XCD v % 8, which owns a contiguous run of the grouped order (groups of GROUP_M m tiles, m fastest inside a group)."""
    assert st["mrot"] == 0 and st["gperm_full"] == 0 and st["tiles"] == tiles_m * tiles_n
    half, vt = -1, v
    if st["half_from"] is not None and v >= st["half_from"]:
        half, vt = (v - st["half_from"]) & 1, st["half_from"] + ((v - st["half_from"]) >> 1)
    ntiles = tiles_m * tiles_n
    q, r, xcd, loc = ntiles >> 3, ntiles & 7, vt & 7, vt >> 3
    i = (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + loc
    per_group = GROUP_M * tiles_n
    grp, rem = divmod(i, per_group)
    gm0 = grp * GROUP_M
    gsz = min(tiles_m - gm0, GROUP_M)
    return (gm0 + rem % gsz, rem // gsz, half)


def fast8p(o):
    """gemm8p.hip: fast_epi, the bf16 path through the LDS image, restated from cst_gemm8p_launch (a comment there points here: the route
    text does not carry the mode, so a change of the launcher's conditions has to be repeated in this function).  The first, fourth and
    last terms are gemm.hip: fill_params' vec_epi for the operands of these cases (16-byte aligned, leading dimension ldc)."""
    return (o["cdt"] == BF and o["splits"] == 1 and o["ldc"] % 8 == 0 and o["N"] % 8 == 0 and o["bias_mode"] != 2
            and (o["bias_mode"] == 0 or o["alpha"] == 1.0) and (o["drop_p"] == 0 or o["N"] % 2 == 0))


def mode8p(o):
    """cst_gemm8p_launch: the epilogue instantiation."""
    fast = fast8p(o)
    if fast and not o["aux_out"] and ((o["dact"] != 0) != (o["resid"] is not None)):
        return 2
    return 1 if fast and not o["dact"] and o["resid"] is None else 0


# ------------------------------------------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------------------------------------------
def magnitudes(K, dt, cdt, gain=1.0, colsum=False):
    """The magnitude sets of A and B of an exact case (module docstring).  Two refinements keep the share of bf16 outputs at 256 or above
    under 2 %: dropout at p = 0.5 and alpha = -2 double the values (gain), i.e. quadruple the variance, so such a case takes the set of
    gain^2 K; and the
    column sums of a bf16 A are bf16 whatever C is, so a case with column sums takes the bf16 rule even with an fp32 C."""
    K = int(K * max(gain, 1.0) ** 2)
    if ((cdt == F32 and not colsum) or dt == F32) or K <= 264:
        return (1, 2, 3), (1, 2, 3)
    if K <= 1600:
        return (1, 2), (1,)
    assert K <= 8200
    return (1,), (1,)


def _ints(gen, n, mags):
    m = torch.tensor(mags, dtype=torch.float32)[torch.randint(0, len(mags), (n,), generator=gen)]
    return m * (2.0 * torch.randint(0, 2, (n,), generator=gen) - 1.0)


def _r8(n):
    return (n + 7) // 8 * 8


def a_view(o, z, buf=None, lda=None, seg_stride=None):
    """Aop [M, K] of batch z as a strided view of the flat buffer (include/cst.h's addressing)."""
    M, K, lda = o["M"], o["K"], o["lda"] if lda is None else lda
    buf = o["a"] if buf is None else buf
    off = o["a_off"][z]
    if o["a_seg"]:
        s, ss = o["a_seg"], o["a_seg_stride"] if seg_stride is None else seg_stride
        assert o["ak"] and K % s == 0
        return buf.as_strided((M, K // s, s), (lda, ss, 1), off)
    return buf.as_strided((M, K), (lda, 1) if o["ak"] else (1, lda), off)


def b_view(o, z, buf=None):
    buf = o["b"] if buf is None else buf
    return buf.as_strided((o["K"], o["N"]), (1, o["ldb"]) if o["bk"] else (o["ldb"], 1), o["b_off"][z])


def c_view(o, flat, z):
    return flat.as_strided((o["M"], o["N"]), (o["ldc"], 1), o["c_off"][z])


def c_stack(o, flat):
    return torch.stack([c_view(o, flat, z) for z in range(o["nb"])])


@functools.lru_cache(maxsize=2)
def operands(name):
    """Everything a launch of the case reads, on the CPU, deterministic per name."""
    c = BY_NAME[name]
    M, N, K, lay, flags, kv = parse(c["row"])
    exact = c["kind"] == "exact"
    gen = torch.Generator(device="cpu")
    gen.manual_seed(zlib.crc32(name.encode()))
    dt = F32 if "f32" in flags else BF
    cdt = F32 if "cf32" in flags else dt
    ak, bk = lay[0] == "k", lay[1] == "k"
    b0, b1 = kv.get("b0", 1), kv.get("b1", 1)
    nb = b0 * b1
    o = dict(name=name, kind=c["kind"], M=M, N=N, K=K, ak=ak, bk=bk, dt=dt, cdt=cdt, b0=b0, b1=b1, nb=nb, flags=flags,
             lda=kv.get("lda", K if ak else M), ldb=kv.get("ldb", K if bk else N), ldc=kv.get("ldc", N), a_seg=kv.get("a_seg", 0),
             a_seg_stride=kv.get("a_seg_stride", 0), alpha=kv.get("alpha", 1.0), split_k=kv.get("split", -1))
    assert not kv.get("b_seg")
    if o["a_seg"]:
        a_sz = (M - 1) * o["lda"] + (K // o["a_seg"] - 1) * o["a_seg_stride"] + o["a_seg"]
    else:
        a_sz = (M - 1) * o["lda"] + K if ak else (K - 1) * o["lda"] + M
    b_sz = (N - 1) * o["ldb"] + K if bk else (K - 1) * o["ldb"] + N
    a_sz, b_sz = _r8(a_sz), _r8(b_sz)
    o["sa"] = (b1 * a_sz, a_sz) if nb > 1 else (0, 0)
    o["sb"] = ((0, b_sz) if c.get("shared_b") else (b1 * b_sz, b_sz)) if nb > 1 else (0, 0)
    zs = [(i, j) for i in range(b0) for j in range(b1)]
    o["a_off"] = [i * o["sa"][0] + j * o["sa"][1] for i, j in zs]
    o["b_off"] = [i * o["sb"][0] + j * o["sb"][1] for i, j in zs]
    nA, nB = max(o["a_off"]) + a_sz, max(o["b_off"]) + b_sz
    if exact:
        ma, mb = magnitudes(K, dt, cdt, (2.0 if "drop" in flags else 1.0) * abs(o["alpha"]), "colsum" in flags)
        o["a"], o["b"] = _ints(gen, nA, ma), _ints(gen, nB, mb)
    else:
        o["a"], o["b"] = torch.randn(nA, generator=gen), torch.randn(nB, generator=gen) * K ** -0.5
    if dt == BF:
        o["a"], o["b"] = o["a"].to(BF).float(), o["b"].to(BF).float()      # (held as fp32 on the CPU; values are bf16-exact)
    # ---- what the contracts declare zero in A ----
    o["k_len"], o["m_len"] = c.get("k_len"), c.get("m_len")
    o["dead_k"], o["dead_m"] = c.get("dead_k"), c.get("dead_m")
    assert ("k_len" in flags) == (o["k_len"] is not None) and ("m_len" in flags) == (o["m_len"] is not None)
    assert ("k_live" in flags) == (o["dead_k"] is not None) and ("m_live" in flags) == (o["dead_m"] is not None)
    for z, (i, _) in enumerate(zs):
        av = a_view(o, z)
        if o["a_seg"]:
            continue
        if o["k_len"] is not None:
            av[:, o["k_len"][i]:] = 0
        if o["m_len"] is not None:
            av[o["m_len"][i]:] = 0
        for blk in o["dead_k"] or ():
            av[:, 64 * blk:64 * blk + 64] = 0
        for blk in o["dead_m"] or ():
            av[64 * blk:64 * blk + 64] = 0
    # ---- C's geometry, shared by aux_out / aux_in / resid ----
    ldc = o["ldc"]
    if nb > 1 and ldc > N:
        o["sc"] = (M * ldc, N)                    # batch1 = channel groups writing neighbouring column blocks (the pos-conv layout)
        assert b1 * N <= ldc
    else:
        o["sc"] = (b1 * M * ldc, M * ldc) if nb > 1 else (0, 0)
    o["c_off"] = [i * o["sc"][0] + j * o["sc"][1] for i, j in zs]
    o["c_size"] = _r8(max(o["c_off"]) + (M - 1) * ldc + N) + (ldc - N)
    o["bias_mode"] = 2 if "biasrow" in flags else 1 if "bias" in flags else 0
    o["bias"], o["sbias"], o["bias_off"] = None, (0, 0), [0] * nb
    blen = M if o["bias_mode"] == 2 else N

    def small(n):
        if exact:
            return torch.randint(-32, 33, (n,), generator=gen).float()
        v = torch.randn(n, generator=gen)
        return v.to(BF).float() if dt == BF else v
    if o["bias_mode"]:
        o["sbias"] = (0, _r8(blen)) if c.get("shared_b") else (b1 * _r8(blen), _r8(blen)) if nb > 1 else (0, 0)
        o["bias_off"] = [i * o["sbias"][0] + j * o["sbias"][1] for i, j in zs]
        o["bias"] = small(max(o["bias_off"]) + _r8(blen))
    o["act"] = c.get("act", RELU) if "act" in flags else NONE
    o["dact"] = c.get("dact", RELU) if "dact" in flags else NONE
    o["aux_out"] = "aux_out" in flags
    o["resid"] = small(o["c_size"]) if "resid" in flags else None
    o["aux_in"] = small(o["c_size"]) if "dact" in flags else None
    o["drop_p"] = c.get("drop_p", 0.5) if "drop" in flags else 0.0
    o["keep"] = None
    if o["drop_p"]:
        from conftest import load_pkg
        import importlib
        load_pkg()
        rng = importlib.import_module("chimera-st_amd.rng")
        o["keep"] = torch.from_numpy(rng.keep_mask_numpy(DROP_KEY, M * _r8(max(N, ldc)), o["drop_p"]))
    o["colsum"] = "colsum" in flags
    o["splits"] = int(c["route"].rsplit("split", 1)[1]) if "split" in c["route"] else max(o["split_k"], 1)
    # gemm8p's fast epilogue and gemm4w round the pre-activation z = alpha acc + bias to bf16 ONCE (the bf16 image in LDS; the reference
    # model's bf16 F.linear output) before activation, dropout, act' and the residual act on it: gemm8p.hip / gemm4w.hip headers
    o["image"] = c["route"] == "4w" or (c["route"].startswith("8p") and fast8p(o))
    return o


def prefill(o, dtype):
    """A flat output before the launch: NaN where the launch must write, SENT everywhere else."""
    flat = torch.full((o["c_size"],), SENT, dtype=dtype)
    for z in range(o["nb"]):
        c_view(o, flat, z).fill_(float("nan"))
    return flat


def expected_all_dead(name):
    """The outputs of the launch whose A is entirely zero (every block dead, every limit 0): exactly the epilogue of zero."""
    o = operands(name)
    aux, v = epilogue(o, torch.zeros(o["nb"], o["M"], o["N"], dtype=torch.float64))
    out = {"C": _flat(o, v, o["cdt"])}
    if aux is not None:
        out["aux_out"] = _flat(o, aux, o["dt"])
    if o["colsum"]:
        out["colsum"] = torch.zeros(o["nb"], o["M"], dtype=o["dt"])
    return out


def stamps(dead, extent):
    """int32 stamps over `extent` in blocks of 64, as the live-tile tests build them: EPOCH where live, another launch's epoch where dead."""
    n = (extent + 63) // 64
    s = torch.full((n,), EPOCH, dtype=torch.int32)
    s[list(dead)] = EPOCH - 1
    return s


# ------------------------------------------------------------------------------------------------------------------------------------
# the fp64 reference
# ------------------------------------------------------------------------------------------------------------------------------------
def _bk(o):
    return 64 if o["dt"] == BF else 32


def _krange(o, z, defect):
    """The K range [0, hi) batch z sums over."""
    K, bk = o["K"], _bk(o)
    hi = K
    if o["k_len"] is not None:
        hi = min(K, o["k_len"][z // o["b1"]])
        if defect == "k_len_rounded_down":
            hi = hi // bk * bk
    if defect == "last_k_tile_dropped":
        hi = (-(-K // bk) - 1) * bk
    if defect == "k_tail_dropped":
        hi = K // bk * bk
    return hi


def _padded(buf, extra):
    return torch.cat([buf, torch.zeros(extra, dtype=buf.dtype)])


def products(o, defect=None, absolute=False, rows=None):
    """acc [nb, M (or len(rows)), N] in fp64 — or sum |a| |b| with absolute."""
    out = []
    for z in range(o["nb"]):
        A, Bm = a_view(o, z), b_view(o, z)
        if defect == "seg_stride_ignored":
            A = a_view(o, z, _padded(o["a"], o["K"]), seg_stride=o["a_seg"])
        if defect == "overlap_read_with_lda_K":
            A = a_view(o, z, _padded(o["a"], o["M"] * o["K"]), lda=o["K"])
        A = A.reshape(o["M"], o["K"])
        hi = _krange(o, z, defect)
        if rows is not None:
            A = A[rows]
        A, Bm = A.double(), Bm.double()
        if absolute:
            A, Bm = A.abs(), Bm.abs()
        acc = A[:, :hi] @ Bm[:hi]
        if defect == "k_tail_not_zero_filled":
            # the last K tile reads k in [K, ceil) of every row: in k-major storage the first elements of the next row
            assert o["ak"] and o["bk"] and rows is None
            t = -(-o["K"] // _bk(o)) * _bk(o) - o["K"]
            Ax = _padded(o["a"], t).as_strided((o["M"], t), (o["lda"], 1), o["a_off"][z] + o["K"]).double()
            Bx = _padded(o["b"], t).as_strided((t, o["N"]), (1, o["ldb"]), o["b_off"][z] + o["K"]).double()
            acc = acc + Ax @ Bx
        if defect == "k_tile_in_two_splits":
            per = -(-(-(-o["K"] // _bk(o))) // o["splits"]) * _bk(o)     # K elements per slice: its first tile is also the previous slice's last
            acc = acc + A[:, per:per + _bk(o)] @ Bm[per:per + _bk(o)]
        if defect == "empty_split_slab_uninitialised" and hi <= _bk(o):   # at most one live K tile: every later slice is empty
            acc = acc + 3.0
        out.append(acc)
    return torch.stack(out)


def _gather(o, flat, rows):
    v = c_stack(o, flat)
    return v if rows is None else v[:, rows]


def epilogue(o, acc, defect=None, rows=None):
    """gemm_common.h: epilogue_store's order — alpha, bias, aux_out, act, dropout, act'(aux_in), resid — in acc's precision (fp64: the
    reference; fp32: the emulation, with norm_ref's restatements of the device GELU).  -> (aux or None, v)."""
    M, N = o["M"], o["N"]
    f64 = acc.dtype == torch.float64
    cast = (lambda t: t.double()) if f64 else (lambda t: t.float())
    ridx = torch.arange(M) if rows is None else rows
    bias = None
    if o["bias_mode"]:
        offs = [0] * o["nb"] if defect == "bias_batch_stride_ignored" else o["bias_off"]
        by_row = (o["bias_mode"] == 2) != (defect == "bias_by_row_instead_of_column")
        if by_row:
            n = M if o["bias_mode"] == 2 else N
            bias = torch.stack([cast(o["bias"][f:f + n])[ridx % n][:, None] for f in offs])
        else:
            bias = torch.stack([cast(o["bias"][f:f + N])[None, :] for f in offs])
    alpha = o["alpha"] if f64 else torch.tensor(o["alpha"], dtype=torch.float32)
    if defect == "alpha_after_bias":
        v = (acc + bias) * alpha
    else:
        v = acc * alpha
        if bias is not None:
            v = v + bias

    def act(x, kind):
        if kind == RELU:
            return x.clamp_min(0.0)
        if kind == GELU:
            return gelu64(x) if f64 else gelu32(x, o["dt"])
        return x
    if o["image"] and (not f64 or o["kind"] == "exact"):
        v = v.to(BF).to(v.dtype)          # (fp64: only where the value is an exact small number; the bounded reference stays unrounded)
    resid = None if o["resid"] is None else cast(_gather(o, o["resid"], rows))
    aux = v if o["aux_out"] else None
    if defect == "residual_before_act":
        v = v + resid
    v = act(v, o["act"])
    if defect == "aux_out_after_act":
        aux = v
    if o["drop_p"]:
        ld = o["ldc"] if defect == "dropout_index_with_ldc" else N
        keep = o["keep"].as_strided((M, N), (ld, 1))[ridx]
        v = v * cast(keep) * (1.0 / (1.0 - o["drop_p"]) if f64 else torch.tensor(1.0, dtype=torch.float32) / torch.tensor(1.0 - o["drop_p"], dtype=torch.float32))
    if o["dact"]:
        zin = cast(_gather(o, o["aux_in"], rows))
        if o["dact"] == RELU:
            v = v * (zin > 0).to(v.dtype)
        else:
            v = v * (dgelu64(zin) if f64 else dgelu32(zin, o["dt"]))
    if resid is not None and defect != "residual_before_act":
        v = v + resid
    return aux, v


def colsums64(o, defect=None):
    """[nb, M] in fp64: the sums of A over k."""
    out = []
    for z in range(o["nb"]):
        A = a_view(o, z).double()
        hi = o["K"]
        if defect == "colsum_last_k_block_dropped":
            hi = (-(-hi // 64) - 1) * 64
        s = A[:, :hi].sum(1)
        if defect == "colsum_one_slice_missing":
            per = -(-(-(-o["K"] // _bk(o))) // o["splits"]) * _bk(o)
            s = s - A[:, per:2 * per].sum(1)
        out.append(s)
    return torch.stack(out)


def _flat(o, vals, dtype):
    flat = torch.full((o["c_size"],), SENT, dtype=dtype)
    for z in range(o["nb"]):
        c_view(o, flat, z).copy_(vals[z])
    return flat


def expected(name, defect=None):
    """Every output of the launch.  -> dict(C=flat [c_size] in C's dtype, aux_out=flat (storage dtype), colsum=[nb, M] (storage dtype)) with
    SENT wherever the launch must not write, and under "v64" the fp64 values {C, aux_out, colsum} ([nb, M, N] / [nb, M]) the bounds are
    drawn around.  For exact cases the flat tensors hold THE bits; for bounded ones the rounded reference."""
    o = operands(name)
    acc = products(o, defect)
    aux, v = epilogue(o, acc, defect)
    out, v64 = {}, {"C": v, "acc": acc}
    if defect == "tile_twice_and_one_never":
        bm, bn, _ = tile_of(BY_NAME[name]["route"])
        v = v.clone()
        v[:, bm:2 * bm, bn:2 * bn] = float("nan")            # tile (1, 1) keeps its prefill
    if defect == "second_half_reads_first_half_rows":
        st = launch8p_state(o["M"], o["N"], o["nb"], o["splits"], o["m_len"] is not None)
        v = v.clone()
        for t in range(st["half_from"], st["nitems"], 2):           # the first half item of every tail tile
            tm, tn, _ = tile_of_item8p(t, st, -(-o["M"] // 256), -(-o["N"] // 256))
            m0, n0 = tm * 256, tn * 256
            h = v[:, m0 + 128:m0 + 256, n0:n0 + 256]
            h.copy_(v[:, m0:m0 + h.shape[1], n0:n0 + 256])
    out["C"] = _flat(o, v, o["cdt"])
    if defect == "trailing_rows_clamped_and_stored":
        bm = tile_of(BY_NAME[name]["route"])[0]
        for z in range(o["nb"]):
            for r in range(o["M"], -(-o["M"] // bm) * bm):    # row M - 1 again, into what follows at C's strides
                at = o["c_off"][z] + r * o["ldc"]
                if at + o["N"] <= o["c_size"]:
                    out["C"][at:at + o["N"]] = v[z, o["M"] - 1].to(o["cdt"])
    if defect == "columns_past_N_written":
        for z in range(o["nb"]):
            g = out["C"].as_strided((o["M"], o["ldc"] - o["N"]), (o["ldc"], 1), o["c_off"][z] + o["N"])
            g.copy_(v[z, :, -1:].to(o["cdt"]).expand_as(g))
    if aux is not None:
        out["aux_out"], v64["aux_out"] = _flat(o, aux, o["dt"]), aux
    if o["colsum"]:
        v64["colsum"] = colsums64(o, defect)
        out["colsum"] = v64["colsum"].to(o["dt"])
    out["v64"] = v64
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# conditions of the exact cases, bounds of the bounded ones
# ------------------------------------------------------------------------------------------------------------------------------------
def headroom(o):
    """K max|a| max|b| |alpha| + max|bias| + max|resid|: below 2^24 every partial sum of every order is an exact fp32 number."""
    mx = lambda t: 0.0 if t is None else float(t.abs().max())  # noqa: E731
    return o["K"] * mx(o["a"]) * mx(o["b"]) * abs(o["alpha"]) + mx(o["bias"]) + mx(o["resid"])


def share_ge_256(ex, o):
    """{output: share of its bf16 elements with magnitude >= 256} (fp32 outputs hold every integer below 2^24: no share to bound)."""
    out = {}
    for k in ("C", "aux_out", "colsum"):
        if k in ex and ex[k].dtype == BF:
            v = ex["v64"][k]
            out[k] = float((v.abs() >= 256).double().mean())
    return out


def bounds(name, ex):
    """{output: bound [nb, M, N] / [nb, M]} of a bounded case (module docstring)."""
    o = operands(name)
    u = U32
    acc = ex["v64"]["acc"]
    S = products(o, absolute=True)
    n = o["K"] + (1 if o["bias_mode"] else 0)
    per_term = (n - 1) + o["splits"] + (1 if o["dt"] == F32 else 0)
    al = abs(o["alpha"])
    pow2 = al in (0.25, 0.5, 1.0, 2.0, 4.0)
    bias_abs = 0.0
    v = acc * o["alpha"]
    if o["bias_mode"]:
        b = torch.stack([o["bias"][f:f + o["N"]].double()[None, :] for f in o["bias_off"]])
        assert o["bias_mode"] == 1
        bias_abs, v = b.abs(), v + b
    b_v = SLACK * (per_term * u * (al * S + bias_abs) + (0.0 if pow2 else u) * (al * acc).abs() + (u * v.abs() if o["bias_mode"] else 0.0)) + ETA
    out = {}
    if o["aux_out"]:
        out["aux_out"] = _store(b_v, v, o["dt"])
    if o["image"]:
        b_v = _store(b_v, v, BF)
    y, b_y = v, b_v
    if o["act"] == GELU:
        y = gelu64(v)
        b_y = _gelu_arg_bound(v, b_v, o["dt"])
    elif o["act"] == RELU:
        y = v.clamp_min(0.0)
    assert not o["drop_p"]
    if o["dact"]:
        zin = c_stack(o, o["aux_in"]).double()
        assert o["dact"] == GELU
        dg, a_dg = dgelu64(zin), a_dgelu(zin, o["dt"])
        y2 = y * dg
        b_y = b_y * (dg.abs() + a_dg) + y.abs() * a_dg + u * y2.abs() + ETA
        y = y2
    if o["resid"] is not None:
        y = y + c_stack(o, o["resid"]).double()
        b_y = b_y + u * y.abs() + ETA
    assert torch.equal(y, ex["v64"]["C"])
    out["C"] = _store(b_y, y, o["cdt"])
    if o["colsum"]:
        bs = []
        for z in range(o["nb"]):
            At = a_view(o, z).double().abs().t()              # [K, M]
            bs.append(_colsum_bound(At, torch.zeros_like(At), o["K"] - 1 + o["splits"]))
        out["colsum"] = _store(torch.stack(bs), ex["v64"]["colsum"], o["dt"])
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# fp32 emulations: the premise of the exact cases shown, the bounds of the others exercised
# ------------------------------------------------------------------------------------------------------------------------------------
SHAPES = ("seq", "chunk16perm")


def sample_rows(M, n=24):
    """The rows an emulation evaluates: the first, the last and a middle run (whole cases up to 3 n rows)."""
    if M <= 3 * n:
        return torch.arange(M)
    return torch.cat([torch.arange(n), torch.arange(M // 2, M // 2 + n), torch.arange(M - n, M)])


def emulate32(name, shape, rows):
    """-> dict(C [nb, R, N], aux_out, colsum [nb, M]) as fp32 arithmetic forms them, rounded by the store:
    seq          one sequential chain in K
    chunk16perm  chunks of 16 consecutive k summed first (one rounding per chunk), the chunks chained in a permuted order"""
    o = operands(name)
    K = o["K"]
    if shape == "seq":
        order = [(k, k + 1) for k in range(K)]
    else:
        ch = [(k, min(k + 16, K)) for k in range(0, K, 16)]
        g = torch.Generator().manual_seed(K)
        order = [ch[i] for i in torch.randperm(len(ch), generator=g).tolist()]
    accs, cs = [], []
    for z in range(o["nb"]):
        A = a_view(o, z).reshape(o["M"], K)
        Ar, Bm = A[rows].float().contiguous(), b_view(o, z).float().contiguous()
        hi = _krange(o, z, None)
        acc = torch.zeros(len(rows), o["N"], dtype=torch.float32)
        col = torch.zeros(o["M"], dtype=torch.float32)
        for lo, up in order:
            up = min(up, hi)
            if up <= lo:
                continue
            if up - lo == 1:
                acc = acc + Ar[:, lo, None] * Bm[lo][None]        # (fp32 operands: the product rounds, then the sum)
            else:
                part = (Ar[:, lo:up, None] * Bm[lo:up][None]).sum(1, dtype=torch.float32) if o["dt"] == F32 else (Ar[:, lo:up].double() @ Bm[lo:up].double()).float()
                acc = acc + part
            if o["colsum"]:
                col = col + (A[:, lo].float() if up - lo == 1 else A[:, lo:up].double().sum(1).float())
        accs.append(acc)
        cs.append(col)
    aux, v = epilogue(o, torch.stack(accs), rows=rows)
    out = {"C": v.to(o["cdt"])}
    if aux is not None:
        out["aux_out"] = aux.to(o["dt"])
    if o["colsum"]:
        out["colsum"] = torch.stack(cs).to(o["dt"])
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# defects: name -> the case in which the wrong output an index-level mistake would produce must show.  expected(case, defect) computes it
# from the same fp64 pieces.  Not listed because no output can show them: a dead k_live block whose stamp is the epoch of another launch
# being visited (the block is zero in A by contract — the dead stamps of stamps() do hold such an epoch, EPOCH - 1), and a dropout index
# without drop_row0 (fill_params sets it to 0 and no caller changes it).
# ------------------------------------------------------------------------------------------------------------------------------------
DEFECTS = {
    "last_k_tile_dropped": "reg_mm",
    "k_tail_dropped": "glds_skinny4",
    "k_tail_not_zero_filled": "glds_skinny4",
    "k_tile_in_two_splits": "reg_mm_split8",
    "empty_split_slab_uninitialised": "reg_klen_split2",          # k_len = 1 and 0: the second slice of those batches is empty
    "trailing_rows_clamped_and_stored": "glds_batched",
    "columns_past_N_written": "8p_kk_ldc",
    "second_half_reads_first_half_rows": "8p_kk_tail",
    "tile_twice_and_one_never": "8p_km_tail",
    "bias_by_row_instead_of_column": "glds_skinny2_epi",
    "bias_batch_stride_ignored": "glds_batched",
    "alpha_after_bias": "8p_kk_bias_alpha",
    "aux_out_after_act": "glds_skinny2_epi",
    "residual_before_act": "glds_skinny2_epi",
    "dropout_index_with_ldc": "8p_kk_drop_ldc",
    "colsum_last_k_block_dropped": "reg_mm_colsum",
    "colsum_one_slice_missing": "reg_mm_colsum_split8",
    "k_len_rounded_down": "reg_klen_split1",
    "seg_stride_ignored": "reg_seg",
    "overlap_read_with_lda_K": "glds_conv",
}


def mismatch_report(got, want, o, route, limit=6):
    """Count, the first few (batch, row, col, got, want) and the set of (m tile, n tile[, half]) the mismatches of a flat output fall in."""
    bm, bn, half = tile_of(route)
    g, w = c_stack(o, got.cpu()).double(), c_stack(o, want.cpu()).double()
    bad = ~((g == w) | (torch.isnan(g) & torch.isnan(w)))
    idx = bad.nonzero()
    first = [(int(z), int(r), int(c), float(g[z, r, c]), float(w[z, r, c])) for z, r, c in idx[:limit]]
    if half:
        tiles = sorted({(int(r) // bm, int(c) // bn, int(r) % bm // half) for _, r, c in idx[::max(1, len(idx) // 20000)]})
    else:
        tiles = sorted({(int(r) // bm, int(c) // bn) for _, r, c in idx[::max(1, len(idx) // 20000)]})
    gaps = int((~((got.cpu().double() == want.cpu().double()))).sum()) - int(bad.sum())
    return "%d of %d differ (+ %d outside the written region); first %s; tiles %s" % (int(bad.sum()), bad.numel(), gaps, first, tiles[:64])
