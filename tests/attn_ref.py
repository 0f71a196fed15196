"""fp64 restatements, counted forward-error bounds and fp32 op-by-op emulations of the fused attention TRAINING kernels: the generic
attn_fwd_kernel / attn_delta_kernel / attn_bwd_dq_kernel / attn_bwd_dkv_kernel of csrc/attention.hip ("generic" route: f32 or bf16,
head dim 32 or 64, causal or not) and the LDS-DMA kernels fa_fwd_kernel / fa_dq_kernel / fa_dkv_kernel of csrc/attention_fast.inc
("fast" route: bf16, head dim 64, not causal).  Plain torch on the CPU; no GPU and no import of the package.  Shared by
test_attn_ref_cpu.py (a faithful fp32 evaluation stays inside every bound, every listed defect leaves it on its named case) and
test_attn_gpu.py (the kernels under the same bounds).  Built like decode_ref.py, whose constants and helpers are imported, not restated.

What is restated bit for bit (a deterministic rounding of an input is part of the reference, not of the bound):
  * fast route: c2 = fl32(fl32(scale) * 1.4426950408889634f); the forward and the dQ kernel score with q^ = bf16(fl32(q c2))
    (decode_ref.mc_qhat), t = q^ . k in log2 units.  The dK / dV kernel scores with q . k^, k^ = bf16(fl32(k c2)): the reference stays at
    t, and |q^ . k - q . k^| is charged per score at its exact fp64 size;
  * generic route: t = (q . k) c2, the fp32 accumulator scaled afterwards;
  * the dropout scale is the launcher's fp32 1 / (1 - p), scale the fp32 argument.
Outputs: o, lse (natural log), dQ, dK, dV.  The gradients are the reference module's formulas in fp64 at the restated scores:
dV = P~^T dO, dP = dO V^T, delta = rowsum(dO o O), dS = P o (dP - delta), dQ = scale dS K, dK = scale dS^T Q, with P~ = P o keep / (1 - p)
and dP masked and scaled alike; dropped probabilities stay in the normaliser.  A row without a visible key has o = 0, lse = -inf and
contributes zero to every gradient.

What is charged (u = 2^-24 per fp32 operation on the magnitude produced, a sum costs its chain length times u on the sum of absolute
terms, an intrinsic INTRIN, an exponential's argument error is a relative error expm1 of it, FLUSH per exponential):
  o      decode_ref.attn_ref_bound.  fast: base 2, the 64-long chain of an MFMA that starts at -m (m_in_chain), P rounded to bf16 (UBF), the
         rescales exact powers of two (n_rescale 0), the P V chain 64 per tile + the l pair sums.  generic: the chain starts at 0 (D
         links), fma(s, c2, -m) rounds once on |t - m|, one exp2 rescale per tile, P rounded to bf16 for bf16 inputs only.
  lse    relative error of l = sum_j w_j rel_j (the same per-key relative errors as o) + its chain (16 + 2 per tile and half-wave, + 2);
         log2 / log: INTRIN on |log2 l| <= |lse2| + |m| and an absolute unit (the mantissa part), the sum with m and the product with
         ln 2 (a rounded constant): u each on the same magnitude.
  backward, on top:  the RECEIVED lse and O carry the forward's bounds: P inherits expm1 of (bound(lse) log2 e + the product with log2 e),
         delta inherits sum_d |dO| bound(O);  delta's own chain (fast: 32 fma per half row + the exchange + the product with 1 / dropout
         scale; generic: 8 fma + a butterfly over D / 8 lanes);  dP: a D-long chain (fast: it starts at -delta / dropout scale, one more
         link of that size);  P: the score chain (fast: it starts at -lse2, every link as large as |lse2| + A) and, generic, the fma
         rounding on |t - lse2|;  in the dK / dV kernel of the fast route |q^ . k - q . k^| in the argument;  dS = P (dP - delta): two
         roundings, then bf16 (UBF on |dS|; dV: UBF on |P~|) for bf16 inputs;  the final chains: 64 per key tile for dQ, 64 per query tile
         for dK / dV;  the scale product (three roundings) and the store.
No constant here was fitted to an output of a kernel or of an emulation."""
import math
import zlib

import torch

from decode_ref import (B, ETA, F, FLUSH, INTRIN, LN2, LOG2E, NAME, NINF, SLACK, U32, UB, _c, _cdiv, _fma, _gen, _store,  # noqa: F401
                        attn_ref_bound, bf, f32, mc_qhat, worst_ratio)
from helper_ref import drop_scale

KT = 64                 # keys (queries in dK / dV) per tile, both routes
FA_THR = 8.0            # the fast route raises its integer maximum when a tile exceeds it by more than this (log2 units)
PERM16 = (0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15)   # k-slot order of a 16-row MFMA step: half-wave 0's rows, then half-wave 1's
CLIMB_Q, CLIMB_KEY = 4.0, 32.0    # planted rows carry CLIMB_Q, the keys of tile i carry i CLIMB_KEY along 1 / sqrt(D): 23 log2 units per tile (D = 64)
ONE_HOT_KEY = 10.0                # every component of the dominant key: 57 log2 units above the rest
SHIFT_KEY = 17.25                 # every component of every key: all scores of a row near +-100 log2 units
OUTS = ("o", "lse", "dq", "dk", "dv")
GARBAGE = 7.0                     # what an unwritten output row holds


def _reg_keys(hi):
    """Keys of a 64-key tile in the order of half-wave hi's accumulator registers (block ks, register r)."""
    return [ks * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi for ks in range(2) for r in range(16)]


# ------------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------------
def _case(name, Tq, Tk, Bn=2, H=2, dt=B, D=64, mask="none", marg=None, kv_len=False, kind="normal", causal=False, drop=0.0, layout="bt",
          slices=False, do_zero=False):
    return dict(name=name, Tq=Tq, Tk=Tk, Bn=Bn, H=H, dt=dt, D=D, mask=mask, marg=marg, kv_len=kv_len, kind=kind, causal=causal, drop=drop,
                layout=layout, slices=slices, do_zero=do_zero)


_LIST = [
    # geometry, N(0, 1), no mask.  B H = 9: one (batch, head) group wraps onto XCD 0 and the padded grid has dead blocks
    _case("geo-1x1", 1, 1),
    _case("geo-33x64", 33, 64, Bn=3, H=3),
    _case("geo-128x65", 128, 65),
    _case("geo-129x192", 129, 192, Bn=3, H=3),
    _case("geo-200x257", 200, 257),
    _case("geo-64x449", 64, 449),
    # masks
    _case("suffix-129x192", 129, 192, Bn=3, mask="suffix", marg=(1, 64, 65)),
    _case("suffix-129x192-kvlen", 129, 192, Bn=3, mask="suffix", marg=(1, 64, 65), kv_len=True),
    _case("suffix-200x257", 200, 257, Bn=3, mask="suffix", marg=(257, 130, 65)),
    _case("suffix-200x257-kvlen", 200, 257, Bn=3, mask="suffix", marg=(257, 130, 65), kv_len=True),
    _case("self-200x200-suffix", 200, 200, Bn=3, mask="suffix", marg=(200, 131, 64), slices=True),       # also run packed (seq=)
    _case("self-200x200-suffix-kvlen", 200, 200, Bn=3, mask="suffix", marg=(200, 131, 64), kv_len=True),
    _case("prefix-129x192", 129, 192, Bn=3, mask="prefix", marg=(1, 64, 130)),
    _case("prefix-64x449", 64, 449, Bn=3, mask="prefix", marg=(0, 200, 385)),
    _case("scattered-200x257", 200, 257, mask="scattered"),
    _case("allmasked-129x192", 129, 192, Bn=3, mask="suffix", marg=(192, 0, 100)),
    _case("allmasked-129x192-kvlen", 129, 192, Bn=3, mask="suffix", marg=(192, 0, 100), kv_len=True),
    # score kinds
    _case("climb-200x449", 200, 449, Bn=3, H=3, kind="climb"),
    _case("descend-64x449", 64, 449, kind="descend"),
    _case("onehot-129x192", 129, 192, Bn=3, mask="suffix", marg=(192, 192, 150), kind="onehot"),
    _case("shift-128x65", 128, 65, kind="shift"),
    # variants
    _case("dropout-129x192", 129, 192, Bn=3, mask="suffix", marg=(192, 100, 65), drop=0.25),
    _case("tb-129x192", 129, 192, Bn=3, mask="suffix", marg=(192, 100, 65), layout="tb"),
    _case("dozero-200x257", 200, 257, do_zero=True),
    # generic only
    _case("f32-D32-100x131", 100, 131, dt=F, D=32, mask="suffix", marg=(131, 70)),
    _case("f32-D64-100x131", 100, 131, dt=F, D=64, mask="suffix", marg=(131, 70)),
    _case("bf16-D32-100x131", 100, 131, dt=B, D=32, mask="suffix", marg=(131, 70)),
    _case("causal-150x150-bf16-D64", 150, 150, causal=True),
    _case("causal-150x150-f32-D32", 150, 150, dt=F, D=32, causal=True),
    _case("causal-40x100-bf16-D32", 40, 100, D=32, causal=True),
    _case("causal-40x100-f32-D64", 40, 100, dt=F, causal=True),
    _case("causal-100x40-bf16-D64", 100, 40, causal=True),              # 60 rows see no key
    _case("causal-100x40-f32-D32", 100, 40, dt=F, D=32, causal=True),
    _case("causal-suffix-150x150", 150, 150, mask="suffix", marg=(150, 70), causal=True),
]
CASES = {c["name"]: c for c in _LIST}


def fast_eligible(c):
    """attn_fast_ok of csrc/attention.hip for the tensors the tests hand over."""
    return c["dt"] == B and c["D"] == 64 and not c["causal"]


def routes(c):
    return ("fast", "generic") if fast_eligible(c) else ("generic",)


RUNS = [(n, r) for n, c in CASES.items() for r in routes(c)]


def dozero_rows(Tq):
    """dO is zero on the leading 128-query block and on the trailing query tile(s): rows outside [128, 192)."""
    i = torch.arange(Tq)
    return (i < 128) | (i >= 192)


def climb_rows(Tq):
    """The planted rows of a climb / descend case: one row in four, so every wave holds planted and plain rows."""
    return (torch.arange(Tq) % 4) == 1


def one_hot_keys(c):
    """Key 63 (last of tile 0), 64 (first of tile 1) and the last live key."""
    return (63, 64, c["marg"][2] - 1)


def case_mask(c):
    """-> bool [Bn, Tk] (True = padding) or None."""
    Bn, Tk = c["Bn"], c["Tk"]
    j = torch.arange(Tk)
    if c["mask"] == "none":
        return None
    if c["mask"] == "suffix":
        return j[None, :] >= torch.tensor(c["marg"])[:, None]
    if c["mask"] == "prefix":
        return j[None, :] < torch.tensor(c["marg"])[:, None]
    m = ((j >= 128) & (j < 192)) | (j == 64) | (j == 64 + 31) | (j == 64 + 32) | (j == 64 + 63)     # scattered
    return m[None, :].expand(Bn, Tk).clone()


def inputs(c):
    """-> dict(q, do [Bn, Tq, H D], k, v [Bn, Tk, H D] of the case's dtype, every value a bf16 value; masked bool [Bn, Tk] | None;
    kv_len int32 [Bn] | None; scale)."""
    Bn, H, D, Tq, Tk = c["Bn"], c["H"], c["D"], c["Tq"], c["Tk"]
    g = _gen(zlib.crc32(c["name"].encode()) & 0xFFFF)
    q = torch.randn(Bn, Tq, H, D, generator=g)
    k = torch.randn(Bn, Tk, H, D, generator=g)
    v = torch.randn(Bn, Tk, H, D, generator=g)
    do = torch.randn(Bn, Tq, H, D, generator=g)
    d = torch.full((D,), D ** -0.5)
    kind = c["kind"]
    if kind != "normal":
        q = q - (q @ d)[..., None] * d                      # no component along d: the planted one is the only one
    if kind in ("climb", "descend"):
        q[:, climb_rows(Tq)] += CLIMB_Q * d
        lvl = (torch.arange(Tk) // KT).float()
        if kind == "descend":
            lvl = float((Tk - 1) // KT) - lvl
        k = k + (lvl * CLIMB_KEY)[None, :, None, None] * d
    elif kind == "onehot":
        q = q + CLIMB_Q * d
        for b, jh in enumerate(one_hot_keys(c)):
            k[b, jh] = ONE_HOT_KEY
    elif kind == "shift":
        q = q + CLIMB_Q * d
        k[0] += SHIFT_KEY
        k[1] -= SHIFT_KEY
    if c["do_zero"]:
        do[:, dozero_rows(Tq)] = 0.0
    masked = case_mask(c)
    kv_len = torch.tensor(c["marg"], dtype=torch.int32) if c["kv_len"] else None
    fin = lambda x, T: x.reshape(Bn, T, H * D).to(B).to(c["dt"])
    return dict(q=fin(q, Tq), k=fin(k, Tk), v=fin(v, Tk), do=fin(do, Tq), masked=masked, kv_len=kv_len, scale=D ** -0.5)


def cpu_keep(c):
    """A keep mask for the CPU tests (the GPU test hands over the package's own)."""
    g = _gen(77)
    return torch.rand(c["Bn"], c["H"], c["Tq"], c["Tk"], generator=g) >= c["drop"]


def _heads(x, c):
    Bn, T = x.shape[0], x.shape[1]
    return x.view(Bn, T, c["H"], c["D"]).transpose(1, 2)        # [Bn, H, T, D]


def _flat(x):
    Bn, H, T, D = x.shape
    return x.transpose(1, 2).reshape(Bn, T, H * D)


def visible(c, masked, cshift=None):
    """-> bool [Bn, 1, Tq, Tk]: key j takes part in query i's row."""
    Bn, Tq, Tk = c["Bn"], c["Tq"], c["Tk"]
    ok = torch.ones(Bn, 1, Tq, Tk, dtype=torch.bool)
    if masked is not None:
        ok = ok & ~masked[:, None, None, :]
    if c["causal"]:
        cs = Tk - Tq if cshift is None else cshift
        ok = ok & (torch.arange(Tk)[None, :] <= torch.arange(Tq)[:, None] + cs)
    return ok


def _c2(scale):
    return _c(f32(scale)) * _c(LOG2E)


def scores64(c, inp, route):
    """-> t, A (the forward's and the dQ kernel's scores, log2 units, and sum_d |q_d k_d| in the same units), t2, A2 (the dK / dV kernel's)."""
    Q, K = _heads(inp["q"], c).float(), _heads(inp["k"], c).float()
    c2 = _c2(inp["scale"])
    dot = lambda a, b: torch.einsum("bhqd,bhjd->bhqj", a.double(), b.double())
    if route == "fast":
        qh, kh = mc_qhat(Q, inp["scale"]), bf(K * c2)
        return dot(qh, K), dot(qh.abs(), K.abs()), dot(Q, kh), dot(Q.abs(), kh.abs())
    t, A = dot(Q, K) * float(c2), dot(Q.abs(), K.abs()) * float(c2)
    return t, A, t, A


# ------------------------------------------------------------------------------------------------------------------------------------
# the fp64 reference and its bounds
# ------------------------------------------------------------------------------------------------------------------------------------
def ref64(c, inp, route, keep=None):
    """-> dict: o, lse, dq, dk, dv (fp64; o, dq [Bn, Tq, C], dk, dv [Bn, Tk, C], lse [Bn, H, Tq]), b_o .. b_dv (the bounds, same shapes),
    t (scores), ok (visibility), dead (rows without a key)."""
    dt, D, Tq, Tk, Bn, H = c["dt"], c["D"], c["Tq"], c["Tk"], c["Bn"], c["H"]
    fast = route == "fast"
    assert not fast or fast_eligible(c)
    p = c["drop"]
    assert (keep is not None) == (p > 0)
    dsc = drop_scale(p) if p > 0 else 1.0
    sc = f32(inp["scale"])
    Q, K, V, dO = (_heads(inp[n], c).double() for n in ("q", "k", "v", "do"))
    ok = visible(c, inp["masked"]).expand(Bn, H, Tq, Tk)
    t, A, t2, A2 = scores64(c, inp, route)
    dead = ~ok.any(-1)
    okf = ok | dead[..., None]                        # a dead row is evaluated over every key and zeroed below
    nt, nqt = _cdiv(Tk, KT), _cdiv(Tq, KT)
    ubf = UB if dt == B else 0.0
    if fast:
        kw = dict(base2=True, chain_t=64, chain_sum=KT * nt + 5, n_rescale=0, m_in_chain=True, p_bf16=True)
        chain_l = 18 * nt + 2
    else:
        kw = dict(base2=True, chain_t=D, chain_sum=(KT + 1) * nt + 3, n_rescale=nt, m_in_chain=False, p_bf16=dt == B)
        chain_l = 19 * nt + 2
    keepf = keep.double() * dsc if p > 0 else torch.ones(())
    Vx = V[:, :, None] * keepf[..., None] if p > 0 else V[:, :, None]
    o, b_o = attn_ref_bound(t, A, okf, Vx, dt, **kw)
    if p > 0:
        b_o = b_o + 2.0 * U32 * o.abs() * (1.0 + ubf)       # the dropout scale folded into 1 / l: one product, one rounded constant
    o = torch.where(dead[..., None], torch.zeros_like(o), o)
    b_o = torch.where(dead[..., None], torch.zeros_like(b_o), b_o)

    # lse
    tm = torch.where(okf, t, torch.full_like(t, NINF))
    lse2 = torch.logsumexp(tm * LN2, -1) / LN2
    w = torch.softmax(tm * LN2, -1)
    tmax = tm.max(-1, keepdim=True).values
    tmin = torch.where(okf, t, torch.full_like(t, float("inf"))).min(-1, keepdim=True).values
    tabs = torch.where(okf, t.abs(), torch.zeros_like(t)).max(-1, keepdim=True).values
    mlink = tabs + 1.0 if fast else 0.0
    arg = kw["chain_t"] * U32 * (A + mlink) + U32 * ((tmax - t).abs() + mlink)
    arg = torch.where(okf, arg, torch.zeros_like(arg))
    rel = SLACK * (torch.expm1(LN2 * arg) + U32 * (INTRIN + kw["n_rescale"] * (INTRIN + 2.0 + LN2 * (tmax - tmin).clamp_min(0.0))))
    rel_l = (w * rel).sum(-1) + SLACK * U32 * chain_l + Tk * 2.0 * FLUSH * 2.0     # l >= 1/2
    mag = lse2.abs() + tabs[..., 0] + 2.0
    b_lse2 = -torch.log1p(-rel_l) / LN2 + U32 * (INTRIN + 2.0) * mag
    lse = lse2 * LN2
    b_lse = SLACK * (LN2 * b_lse2 + 3.0 * U32 * lse.abs()) + ETA
    lse = torch.where(dead, torch.full_like(lse, NINF), lse)
    b_lse = torch.where(dead, torch.zeros_like(b_lse), b_lse)

    # backward
    lse2c = lse2[..., None]
    eps_l2 = torch.where(dead, torch.zeros_like(b_lse), b_lse / LN2 + 2.0 * U32 * lse2.abs())[..., None]
    P = torch.where(ok, torch.exp2(t - lse2c), torch.zeros_like(t))
    Pt = P * keepf
    dPraw = torch.einsum("bhqd,bhjd->bhqj", dO, V)
    AP = torch.einsum("bhqd,bhjd->bhqj", dO.abs(), V.abs())
    delta = (dO * o).sum(-1, keepdim=True)
    dSm = keepf * dPraw - delta
    dS = P * dSm
    dq = sc * torch.einsum("bhqj,bhjd->bhqd", dS, K)
    dk = sc * torch.einsum("bhqj,bhqd->bhjd", dS, Q)
    dv = torch.einsum("bhqj,bhqd->bhjd", Pt, dO)

    ndel = 65 if fast else 16 + int(math.log2(D // 8))
    e_delta = ((dO.abs() * b_o).sum(-1, keepdim=True) * (1.0 + U32 * ndel) + SLACK * U32 * (ndel + 2) * (dO * o).abs().sum(-1, keepdim=True))
    e_dp = keepf * SLACK * U32 * (D + 1) * (AP + (delta.abs() / dsc if fast else 0.0)) + e_delta + 2.0 * U32 * dSm.abs()
    if fast:
        argq = eps_l2 + U32 * ((D + 1) * (A + lse2c.abs()) + (t - lse2c).abs())
        argk = eps_l2 + U32 * ((D + 1) * (A2 + lse2c.abs()) + (t2 - lse2c).abs()) + (t - t2).abs()
    else:
        argq = argk = eps_l2 + U32 * (D * A + (t - lse2c).abs() + lse2c.abs())
    relq = SLACK * (torch.expm1(LN2 * argq) + U32 * INTRIN)
    relk = SLACK * (torch.expm1(LN2 * argk) + U32 * INTRIN)

    def e_ds(r):
        return dS.abs() * r + P * (1.0 + r) * e_dp + (2.0 * U32 + ubf) * dS.abs() + 2.0 * FLUSH * dSm.abs()

    Eq, Ek = e_ds(relq), e_ds(relk)
    b_dq = sc * (torch.einsum("bhqj,bhjd->bhqd", Eq, K.abs()) + SLACK * U32 * KT * nt * torch.einsum("bhqj,bhjd->bhqd", dS.abs(), K.abs()))
    b_dq = _store(b_dq + 3.0 * U32 * dq.abs() + ETA, dq, dt)
    b_dk = sc * (torch.einsum("bhqj,bhqd->bhjd", Ek, Q.abs()) + SLACK * U32 * KT * nqt * torch.einsum("bhqj,bhqd->bhjd", dS.abs(), Q.abs()))
    b_dk = _store(b_dk + 3.0 * U32 * dk.abs() + ETA, dk, dt)
    Ev = Pt * (relk + ubf + U32) + keepf * 2.0 * FLUSH
    b_dv = torch.einsum("bhqj,bhqd->bhjd", Ev, dO.abs()) + SLACK * U32 * KT * nqt * torch.einsum("bhqj,bhqd->bhjd", Pt, dO.abs())
    b_dv = _store(b_dv + 3.0 * U32 * dv.abs() + ETA, dv, dt)
    return dict(o=_flat(o), lse=lse, dq=_flat(dq), dk=_flat(dk), dv=_flat(dv), b_o=_flat(b_o), b_lse=b_lse, b_dq=_flat(b_dq), b_dk=_flat(b_dk),
                b_dv=_flat(b_dv), t=t, ok=ok, dead=dead)


def plain64(c, inp):
    """softmax(Q K^T scale) V in fp64, nothing restated (for the q^ perturbation test)."""
    Q, K, V = (_heads(inp[n], c).double() for n in ("q", "k", "v"))
    ok = visible(c, inp["masked"])
    s = torch.einsum("bhqd,bhjd->bhqj", Q, K) * inp["scale"]
    return _flat(torch.softmax(torch.where(ok, s, torch.full_like(s, NINF)), -1) @ V)


# ------------------------------------------------------------------------------------------------------------------------------------
# reachability, from the fp64 scores
# ------------------------------------------------------------------------------------------------------------------------------------
def raises64(t, ok):
    """How often fa_fwd_kernel raises a row's lazy integer maximum (the first set included), tile by tile -> long [Bn, H, Tq]."""
    Tk = t.shape[-1]
    tm = torch.where(ok, t, torch.full_like(t, NINF))
    m = torch.full(t.shape[:-1], NINF, dtype=t.dtype)
    n = torch.zeros(t.shape[:-1], dtype=torch.long)
    for j in range(_cdiv(Tk, KT)):
        mt = tm[..., KT * j:KT * (j + 1)].amax(-1)
        need = torch.where(m == NINF, mt > NINF, mt - m > FA_THR)
        m = torch.where(need, torch.ceil(mt), m)
        n = n + need.long()
    return n


def leading_masked_tiles(masked):
    """-> long [Bn]: how many leading 64-key tiles are wholly masked."""
    Bn, Tk = masked.shape
    nt = _cdiv(Tk, KT)
    full = torch.stack([masked[:, KT * j:KT * (j + 1)].all(1) for j in range(nt)], 1).long()
    return torch.cumprod(full, 1).sum(1)


# ------------------------------------------------------------------------------------------------------------------------------------
# fp32 op-by-op emulations
# ------------------------------------------------------------------------------------------------------------------------------------
DEFECTS = {
    # name: (case, route, the outputs of which at least one must leave its bound)
    "o_not_rescaled_at_second_raise": ("climb-200x449", "fast", ("o",)),
    "l_not_rescaled_at_second_raise": ("climb-200x449", "fast", ("o", "lse")),
    "negm_not_shifted_lse_stale": ("climb-200x449", "fast", ("lse",)),
    "raise_taken_only_once": ("climb-200x449", "fast", ("o", "lse")),
    "last_key_of_ragged_tile_dropped": ("geo-128x65", "fast", ("o", "lse")),
    "mask_bit_of_wrong_register": ("scattered-200x257", "fast", ("o", "lse")),
    "masked_first_tile_leaves_m_at_minus_inf": ("prefix-64x449", "fast", ("o", "lse")),
    "kv_len_off_by_one": ("suffix-129x192-kvlen", "fast", ("o", "lse")),
    "causal_cshift_ignored": ("causal-40x100-f32-D64", "generic", ("o", "lse")),
    "dropped_removed_from_normaliser": ("dropout-129x192", "fast", ("o", "lse")),
    "delta_without_dropout_factor": ("dropout-129x192", "fast", ("dq", "dk")),
    "dk_scaled_by_c2": ("geo-33x64", "fast", ("dk",)),
    "dead_tile_rows_not_zeroed": ("dozero-200x257", "fast", ("dq",)),
    "lse_in_log2_units": ("geo-33x64", "fast", ("lse",)),
    "generic_o_not_rescaled": ("climb-200x449", "generic", ("o",)),
    "generic_dv_without_dropout_scale": ("dropout-129x192", "generic", ("dv",)),
}


def _chain(a, b, start):
    """start [.., M, N] + sum_k a [.., M, k] b [.., N, k] as one k-ordered fmaf chain (an MFMA accumulation, decode_ref)."""
    s = start
    for k in range(a.shape[-1]):
        s = _fma(a[..., :, None, k], b[..., None, :, k], s)
    return s


def _padrows(x, n):
    pad = n - x.shape[2]
    return x if pad == 0 else torch.cat([x, x.new_zeros(x.shape[:2] + (pad,) + x.shape[3:])], 2)


def _tile_order(n):
    """Rows 0 .. n - 1 in the order an MFMA chain over 64-row tiles meets them."""
    return [KT * j + base + i for j in range(_cdiv(n, KT)) for base in (0, 16, 32, 48) for i in PERM16 if KT * j + base + i < n]


def _key_state(c, inp, defect):
    """-> masked bool [Bn, Tkp] over the tile-padded keys (mask, range, kv_len) with the mask defects planted, Tkp, leading tiles [Bn]."""
    Bn, Tk = c["Bn"], c["Tk"]
    Tkp = KT * _cdiv(Tk, KT)
    m = torch.ones(Bn, Tkp, dtype=torch.bool)
    m[:, :Tk] = inp["masked"] if inp["masked"] is not None else False
    ntl = torch.full((Bn,), _cdiv(Tk, KT))
    if inp["kv_len"] is not None:
        kend = inp["kv_len"].long() - (1 if defect == "kv_len_off_by_one" else 0)
        m = m | (torch.arange(Tkp)[None, :] >= kend[:, None])
        ntl = (kend + KT - 1) // KT
    if defect == "last_key_of_ragged_tile_dropped" and Tk % KT:
        m[:, Tk - 1] = True
    if defect == "mask_bit_of_wrong_register":      # the tile word not shifted by 4 hi: half-wave 1 tests the bits of half-wave 0's keys
        jj = torch.arange(Tkp)
        m = m[:, jj - 4 * ((jj >> 2) & 1)]
    return m, Tkp, ntl


def _vis_padded(c, inp, defect):
    """ok [Bn, 1, Tq, Tkp] for the generic kernels."""
    m, Tkp, _ = _key_state(c, inp, defect)
    ok = ~m[:, None, None, :].expand(c["Bn"], 1, c["Tq"], Tkp)
    if c["causal"]:
        cs = 0 if defect == "causal_cshift_ignored" else c["Tk"] - c["Tq"]
        ok = ok & (torch.arange(Tkp)[None, :] <= torch.arange(c["Tq"])[:, None] + cs)
    return ok, Tkp


def _keep_padded(keep, Tkp):
    if keep is None:
        return None
    pad = Tkp - keep.shape[-1]
    return keep if pad == 0 else torch.cat([keep, keep.new_ones(keep.shape[:-1] + (pad,))], -1)


def _pair_sums(p, l, alpha=None):
    """l [.., 2] (one partial sum per half-wave) takes a tile's probabilities p [.., 64]: even and odd registers in two chains."""
    out = []
    for hi in range(2):
        idx = _reg_keys(hi)
        e, od = torch.zeros_like(p[..., 0]), torch.zeros_like(p[..., 0])
        for i in range(0, 32, 2):
            e = e + p[..., idx[i]]
            od = od + p[..., idx[i + 1]]
        lh = l[..., hi] if alpha is None else l[..., hi] * alpha
        out.append(lh + (e + od))
    return torch.stack(out, -1)


def _pv(o, pb, Vt):
    """o [.., Tq, D] += pb [.., Tq, 64] Vt [.., 64, D]: four MFMA steps of 16 keys, slot order PERM16."""
    for base in (0, 16, 32, 48):
        for i in PERM16:
            o = _fma(pb[..., base + i, None], Vt[:, :, None, base + i, :], o)
    return o


def _dead_blocks(dO4, Tq):
    """-> bool [Bn, H, Tq]: the row's 128-query workgroup has no non-zero dO row."""
    nz = (dO4 != 0).any(-1)
    out = torch.zeros_like(nz)
    for q0 in range(0, Tq, 128):
        out[..., q0:q0 + 128] = ~nz[..., q0:q0 + 128].any(-1, keepdim=True)
    return out


def fast_fwd32(c, inp, keep=None, defect=None):
    """fa_fwd_kernel -> o [Bn, Tq, C] bf16, lse fp32 [Bn, H, Tq]."""
    Bn, H, Tq = c["Bn"], c["H"], c["Tq"]
    m, Tkp, ntl = _key_state(c, inp, defect)
    Q, K, V = (_heads(inp[n], c).float() for n in ("q", "k", "v"))
    K, V = _padrows(K, Tkp), _padrows(V, Tkp)
    keep = _keep_padded(keep, Tkp)
    dsc = _c(drop_scale(c["drop"]) if c["drop"] > 0 else 1.0)
    qh = mc_qhat(Q, inp["scale"])
    negm = torch.zeros(Bn, H, Tq)
    negm_lse = torch.zeros(Bn, H, Tq)
    raise_at = torch.full((Bn, H, Tq), NINF)
    l = torch.zeros(Bn, H, Tq, 2)
    o = torch.zeros(Bn, H, Tq, 64)
    one = torch.ones(Bn, H, Tq)
    for j in range(Tkp // KT):
        sl = slice(KT * j, KT * (j + 1))
        mk = m[:, None, None, sl].expand(Bn, H, Tq, KT)
        s = _chain(qh, K[:, :, sl], torch.where(mk, torch.full((Bn, H, Tq, KT), NINF), negm[..., None].expand(Bn, H, Tq, KT)))
        mt = s.amax(-1)
        first = raise_at < 0
        need = mt > raise_at
        if defect == "raise_taken_only_once":
            need = need & first
        dm = torch.where(need, torch.ceil(mt), torch.zeros_like(mt))
        alpha = torch.where(first, one, torch.exp2(-dm))
        second = need & ~first
        o = o * (torch.where(second, one, alpha) if defect == "o_not_rescaled_at_second_raise" else alpha)[..., None]
        l = l * (torch.where(second, one, alpha) if defect == "l_not_rescaled_at_second_raise" else alpha)[..., None]
        negm = negm - dm
        negm_lse = negm_lse - (torch.where(second, torch.zeros_like(dm), dm) if defect == "negm_not_shifted_lse_stale" else dm)
        s = s - dm[..., None]
        raise_at = torch.where(need, torch.full_like(raise_at, FA_THR), raise_at)
        if defect == "masked_first_tile_leaves_m_at_minus_inf":
            full = (mk.all(-1) & first & (j < ntl).view(Bn, 1, 1))
            negm = torch.where(full, torch.full_like(negm, float("inf")), negm)      # m = -inf taken as set
        p = torch.exp2(s)
        pl = torch.where(keep[..., sl], p, torch.zeros_like(p)) if (defect == "dropped_removed_from_normaliser" and keep is not None) else p
        l = _pair_sums(pl, l)
        pb = bf(p)
        if keep is not None:
            pb = torch.where(keep[..., sl], pb, torch.zeros_like(pb))
        o = _pv(o, pb, V[:, :, sl])
    lt = l[..., 0] + l[..., 1]
    inv = torch.where(lt > 0, dsc / lt, torch.zeros_like(lt))
    lse = torch.log2(lt) - negm_lse
    if defect != "lse_in_log2_units":
        lse = lse * _c(LN2)
    lse = torch.where(lt > 0, lse, torch.full_like(lt, NINF))
    return _flat(o * inv[..., None]).to(B), lse


def _fast_stats(c, inp, o, lse, defect):
    """The pre-pass inside fa_dq_kernel: -lse log2 e and -delta / dropout scale per query row."""
    O4, dO4 = _heads(o, c).float(), _heads(inp["do"], c).float()
    acc = []
    for hi in range(2):
        a = torch.zeros_like(O4[..., 0])
        for kk in range(4):
            for e in range(8):
                d = 16 * kk + 8 * hi + e
                a = _fma(O4[..., d], dO4[..., d], a)
        acc.append(a)
    acc = acc[0] + acc[1]
    nl = torch.where(lse == NINF, lse, -lse * _c(LOG2E))
    inv = _c(1.0) / _c(drop_scale(c["drop"]) if c["drop"] > 0 else 1.0)
    nd = -acc if defect == "delta_without_dropout_factor" else -acc * inv
    return nl, nd


def fast_dq32(c, inp, o, lse, keep=None, defect=None):
    """fa_dq_kernel -> dQ [Bn, Tq, C] bf16."""
    Bn, H, Tq = c["Bn"], c["H"], c["Tq"]
    m, Tkp, _ = _key_state(c, inp, defect)
    Q, K, V, dO = (_heads(inp[n], c).float() for n in ("q", "k", "v", "do"))
    K, V = _padrows(K, Tkp), _padrows(V, Tkp)
    keep = _keep_padded(keep, Tkp)
    qh = mc_qhat(Q, inp["scale"])
    nl, nd = _fast_stats(c, inp, o, lse, defect)
    mk = m[:, None, None, :].expand(Bn, H, Tq, Tkp)
    s = _chain(qh, K, torch.where(mk, torch.full((Bn, H, Tq, Tkp), NINF), nl[..., None].expand(Bn, H, Tq, Tkp)))
    dp = _chain(dO, V, nd[..., None].expand(Bn, H, Tq, Tkp))
    if keep is not None:
        dp = torch.where(keep, dp, nd[..., None].expand_as(dp))
    pr = torch.exp2(s)
    dsb = bf(pr * dp)
    dq = torch.zeros(Bn, H, Tq, 64)
    for kk in _tile_order(Tkp):
        dq = _fma(K[:, :, None, kk, :], dsb[..., kk, None], dq)
    mul = _c(f32(inp["scale"])) * _c(drop_scale(c["drop"]) if c["drop"] > 0 else 1.0)
    out = bf(dq * mul)
    if defect == "dead_tile_rows_not_zeroed":
        out = torch.where(_dead_blocks(dO, Tq)[..., None], torch.full_like(out, GARBAGE), out)
    return _flat(out).to(B)


def fast_dkv32(c, inp, o, lse, keep=None, defect=None):
    """fa_dkv_kernel -> dK, dV [Bn, Tk, C] bf16."""
    Bn, H, Tq, Tk = c["Bn"], c["H"], c["Tq"], c["Tk"]
    m, Tkp, _ = _key_state(c, inp, defect)
    Q, K, V, dO = (_heads(inp[n], c).float() for n in ("q", "k", "v", "do"))
    K, V = _padrows(K, Tkp), _padrows(V, Tkp)
    keep = _keep_padded(keep, Tkp)
    kh = bf(K * _c2(inp["scale"]))
    nl, nd = _fast_stats(c, inp, o, lse, defect)
    s = _chain(Q, kh, nl[..., None].expand(Bn, H, Tq, Tkp))
    ndx = nd[..., None].expand(Bn, H, Tq, Tkp)
    dp = _chain(dO, V, ndx)
    pr = torch.exp2(s)
    if keep is not None:
        ds_ = pr * torch.where(keep, dp, ndx)
        pr = torch.where(keep, pr, torch.zeros_like(pr))
    else:
        ds_ = pr * dp
    prb, dsb = bf(pr), bf(ds_)
    dk = torch.zeros(Bn, H, Tkp, 64)
    dv = torch.zeros(Bn, H, Tkp, 64)
    for q in _tile_order(Tq):
        dv = _fma(dO[:, :, q, None, :], prb[:, :, q, :, None], dv)
        dk = _fma(Q[:, :, q, None, :], dsb[:, :, q, :, None], dk)
    dsc = _c(drop_scale(c["drop"]) if c["drop"] > 0 else 1.0)
    mulk = (_c2(inp["scale"]) if defect == "dk_scaled_by_c2" else _c(f32(inp["scale"]))) * dsc
    z = m[:, None, :, None]
    dk = torch.where(z, torch.zeros_like(dk), dk * mulk)[:, :, :Tk]
    dv = torch.where(z, torch.zeros_like(dv), dv * dsc)[:, :, :Tk]
    return _flat(dk).to(B), _flat(dv).to(B)


def _rnd(c):
    return bf if c["dt"] == B else (lambda x: x)


def gen_scores32(c, inp, ok, Tkp):
    Q, K = _heads(inp["q"], c).float(), _padrows(_heads(inp["k"], c).float(), Tkp)
    return _chain(Q, K, torch.zeros(c["Bn"], c["H"], c["Tq"], Tkp))


def gen_fwd32(c, inp, keep=None, defect=None):
    """attn_fwd_kernel -> o [Bn, Tq, C], lse."""
    Bn, H, Tq, D = c["Bn"], c["H"], c["Tq"], c["D"]
    ok, Tkp = _vis_padded(c, inp, defect)
    ok = ok.expand(Bn, H, Tq, Tkp)
    V = _padrows(_heads(inp["v"], c).float(), Tkp)
    keep = _keep_padded(keep, Tkp)
    c2 = _c2(inp["scale"])
    dsc = _c(drop_scale(c["drop"]) if c["drop"] > 0 else 1.0)
    rnd = _rnd(c)
    s_all = gen_scores32(c, inp, ok, Tkp)
    s_all = torch.where(ok, s_all, torch.full_like(s_all, NINF))
    mrun = torch.full((Bn, H, Tq), -1.0e30)
    l = torch.zeros(Bn, H, Tq, 2)
    o = torch.zeros(Bn, H, Tq, D)
    for j in range(Tkp // KT):
        sl = slice(KT * j, KT * (j + 1))
        s = s_all[..., sl]
        mnew = torch.maximum(mrun, s.amax(-1) * c2)
        alpha = torch.exp2(mrun - mnew)
        e = torch.exp2(_fma(s, c2, -mnew[..., None]))
        if defect == "dropped_removed_from_normaliser" and keep is not None:
            e = torch.where(keep[..., sl], e, torch.zeros_like(e))
        l = _pair_sums(e, l, alpha)
        mrun = mnew
        if keep is not None:
            e = torch.where(keep[..., sl], e, torch.zeros_like(e))
        if not (defect == "generic_o_not_rescaled" and j >= 2):
            o = o * alpha[..., None]
        o = _pv(o, rnd(e), V[:, :, sl])
    lt = l[..., 0] + l[..., 1]
    inv = torch.where(lt > 0, dsc / lt, torch.zeros_like(lt))
    lse = torch.where(lt > 0, mrun * _c(LN2) + torch.log(lt), torch.full_like(lt, NINF))
    return _flat(o * inv[..., None]).to(c["dt"]), lse


def gen_delta32(c, inp, o):
    """attn_delta_kernel: 8 elements per lane, a butterfly over the D / 8 lanes of a row."""
    O4, dO4 = _heads(o, c).float(), _heads(inp["do"], c).float()
    lpr = c["D"] // 8
    x = torch.zeros(O4.shape[:-1] + (lpr,))
    O8, dO8 = O4.reshape(O4.shape[:-1] + (lpr, 8)), dO4.reshape(dO4.shape[:-1] + (lpr, 8))
    for e in range(8):
        x = _fma(O8[..., e], dO8[..., e], x)
    idx, off = torch.arange(lpr), 1
    while off < lpr:
        x = x + x[..., idx ^ off]
        off <<= 1
    return x[..., 0]


def _gen_bwd_common(c, inp, o, lse, keep, defect):
    Bn, H, Tq = c["Bn"], c["H"], c["Tq"]
    ok, Tkp = _vis_padded(c, inp, defect)
    ok = ok.expand(Bn, H, Tq, Tkp)
    V, dO = _padrows(_heads(inp["v"], c).float(), Tkp), _heads(inp["do"], c).float()
    keep = _keep_padded(keep, Tkp)
    dsc = _c(drop_scale(c["drop"]) if c["drop"] > 0 else 1.0)
    lse2 = torch.where(lse == NINF, torch.full_like(lse, float("inf")), lse * _c(LOG2E))
    s = gen_scores32(c, inp, ok, Tkp)
    e = torch.exp2(_fma(s, _c2(inp["scale"]), -lse2[..., None]))
    e = torch.where(ok, e, torch.zeros_like(e))
    dp = _chain(dO, V, torch.zeros_like(s))
    if keep is not None:
        dp = torch.where(keep, dp * dsc, torch.zeros_like(dp))
    dsv = e * (dp - gen_delta32(c, inp, o)[..., None])
    return ok, Tkp, keep, dsc, e, dsv, dO


def gen_dq32(c, inp, o, lse, keep=None, defect=None):
    ok, Tkp, keep, dsc, e, dsv, dO = _gen_bwd_common(c, inp, o, lse, keep, defect)
    K = _padrows(_heads(inp["k"], c).float(), Tkp)
    dsb = _rnd(c)(dsv)
    dq = torch.zeros(c["Bn"], c["H"], c["Tq"], c["D"])
    for kk in _tile_order(Tkp):
        dq = _fma(K[:, :, None, kk, :], dsb[..., kk, None], dq)
    out = dq * _c(f32(inp["scale"]))
    if defect == "dead_tile_rows_not_zeroed":
        out = torch.where(_dead_blocks(dO, c["Tq"])[..., None], torch.full_like(out, GARBAGE), out)
    return _flat(out).to(c["dt"])


def gen_dkv32(c, inp, o, lse, keep=None, defect=None):
    ok, Tkp, keep, dsc, e, dsv, dO = _gen_bwd_common(c, inp, o, lse, keep, defect)
    Q = _heads(inp["q"], c).float()
    rnd = _rnd(c)
    pr = e
    if keep is not None:
        pr = torch.where(keep, e if defect == "generic_dv_without_dropout_scale" else e * dsc, torch.zeros_like(e))
    prb, dsb = rnd(pr), rnd(dsv)
    dk = torch.zeros(c["Bn"], c["H"], Tkp, c["D"])
    dv = torch.zeros(c["Bn"], c["H"], Tkp, c["D"])
    for q in _tile_order(c["Tq"]):
        dv = _fma(dO[:, :, q, None, :], prb[:, :, q, :, None], dv)
        dk = _fma(Q[:, :, q, None, :], dsb[:, :, q, :, None], dk)
    m, _, _ = _key_state(c, inp, defect)
    z = m[:, None, :, None]
    dk = torch.where(z, torch.zeros_like(dk), dk * _c(f32(inp["scale"])))[:, :, :c["Tk"]]
    dv = torch.where(z, torch.zeros_like(dv), dv)[:, :, :c["Tk"]]
    return _flat(dk).to(c["dt"]), _flat(dv).to(c["dt"])


def emulate32(c, inp, route, keep=None, defect=None, want=OUTS):
    """Forward, then the backward on the emulated forward's own o and lse, as a training step chains the kernels -> dict of OUTS."""
    assert defect is None or defect in DEFECTS
    fwd, dqf, dkvf = (fast_fwd32, fast_dq32, fast_dkv32) if route == "fast" else (gen_fwd32, gen_dq32, gen_dkv32)
    o, lse = fwd(c, inp, keep, defect)
    out = dict(o=o, lse=lse)
    if "dq" in want:
        out["dq"] = dqf(c, inp, o, lse, keep, defect)
    if "dk" in want or "dv" in want:
        out["dk"], out["dv"] = dkvf(c, inp, o, lse, keep, defect)
    return out
