"""fp64 restatements, counted forward-error bounds and fp32 op-by-op emulations of the kernels that run once per generated token:
cst_dec_self_attn, cst_dec_cross_attn (the VALU kernel of csrc/decode.hip and the matrix-core fa_dec_cross_kernel of
csrc/attention_fast.inc), cst_dec_ln_q_cross_attn, cst_dec_linear / cst_dec_ln_linear and cst_dec_embed.  Plain torch and numpy; no GPU
and no import of the package.  Shared by test_decode_ref_cpu.py (a faithful fp32 evaluation stays inside every bound and every listed
defect leaves it on a named case) and test_decode_kernels_gpu.py (the kernels under the same bounds).  Built like helper_ref.py /
norm_ref.py, whose constants (U32, UBF, ETA, FLUSH, SLACK, INTRIN) and helpers are imported, not restated.

What is restated bit for bit (the references are functions of what a kernel RECEIVES; a deterministic rounding of an input is part of
the reference, not of the bound):
  * matrix-core cross attention: q^ = bf16(fl32(q c2)), c2 = fl32(scale * 1.4426950408889634f), as fa_row_frags forms it;
  * VALU cross attention: fl32(q scale);  self-attention: fl32(q scale), on the FAST path (bf16, head dim 64) times log2 e again;
  * Wg, sg, sb of the LayerNorm-folded kernels are taken as given.

What is charged.  An fp32 add, multiply or fma costs u = 2^-24 on the magnitude produced; a sum costs (chain length, read from the
kernel) u on the sum of the ABSOLUTE terms.  An MFMA is a k-ordered fp32 fmaf chain with one rounding per product (the programming
guide), and the emulations are written that way: the chain of QK^T is 64 (head dim 32: 32), of dec_linear K / NW plus the NW - 1 wave-order
adds.  expf, exp2, rsqrtf and / cost INTRIN each; the error of an exponential's argument is a relative error of its result (expm1 of it:
no linearisation); FLUSH is charged per exponential.  The softmax is invariant under a shift of all scores of a row, so the error of the
running maximum itself costs nothing: only the rounding of `score - max` (and, in the matrix-core kernel, of the chain that starts at
-m) does.  In the matrix-core kernel every probability is rounded to bf16 before P V: UBF = 2^-8 relative on sum_j p_j |v_j| (bf16 keeps 8
significant bits, so round-to-nearest errs by up to 2^-8 of a value just above a power of two, not 2^-9; on a one-hot row the whole
output is v_j bf16(p_j) / p_j and the error is reached, not averaged: with 2^-9 the faithful emulation leaves the bound, 1.018 at S = 97,
beam 32, left padding); its own sum l adds the fp32 values.  Rescaling there multiplies by exact powers of two.  A bf16 store goes through _store.  The LayerNorm-folded kernels
compute var = E[x^2] - mean^2 and v - mean sg in fp32: the bound carries the error of mean^2 against var + eps (as an interval of rstd,
not linearised: a constant row has var = 0) and of mean sg against v, so a row with a dominant mean gets the wider bound it is entitled
to and no more.  No constant here was fitted to an output of a kernel or of an emulation."""
import math

import torch

from helper_ref import ETA, FLUSH, INTRIN, NAME, SLACK, U32, UBF, _c, _fma, _store, a_gelu, f32, gelu32, gelu64, worst_ratio  # noqa: F401
from norm_ref import dgelu64

F, B = torch.float32, torch.bfloat16
BSZ = 3
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
UB = UBF                # round-to-nearest of a bf16 value inside a kernel (P, q, q^): 8 significant bits, unit roundoff 2^-8
NINF = float("-inf")


def _gen(seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return g


def _cdiv(a, b):
    return (a + b - 1) // b


def bf(x):
    """fp32 -> bf16 (round to nearest even) -> fp32."""
    return x.to(B).float()


def _exp32(x, base2):
    return torch.exp2(x) if base2 else torch.exp(x)


# ------------------------------------------------------------------------------------------------------------------------------------
# the shared bound of a single-query softmax attention row
# ------------------------------------------------------------------------------------------------------------------------------------
def attn_ref_bound(t, A, ok, V, dt, base2, chain_t, chain_sum, n_rescale, m_in_chain=False, p_bf16=False, dt_extra=None):
    """t [.., n]: exact scores in the kernel's units (log2 units if base2) of the rounded inputs; A [.., n] = sum_d |q_d k_jd|;
    ok [.., n]: key takes part; V [.., n, D] (fp64).  -> (out, bound) [.., D].
    argument of key j's exponential: chain_t u A_j (the dot product; with m_in_chain the chain starts at -m and every link may be as
    large as |m| + A_j, |m| <= max|t| + 1, and `s -= dm` rounds once more), u |t_j - max| for the subtraction, dt_extra (an absolute
    error of the score that the caller brings, e.g. of a query computed in the kernel).  Relative error of p_j: expm1 of that, INTRIN,
    and per rescale of the running state INTRIN + 2 and u (max - min) for its argument (VALU kernels; the matrix-core kernel rescales
    by exact powers of two).  p_j enters numerator and denominator: w_j rel_j (|v_j| + |out|).  The sums: chain_sum u on sum w |v| and
    on the denominator; the final division INTRIN + 1; FLUSH per exponential against a denominator >= 1/2."""
    ln = LN2 if base2 else 1.0
    tm = torch.where(ok, t, torch.full_like(t, NINF))
    tmax = tm.max(-1, keepdim=True).values
    tmin = torch.where(ok, t, torch.full_like(t, float("inf"))).min(-1, keepdim=True).values
    rng = (tmax - tmin).clamp_min(0.0)
    w = torch.softmax(tm * ln, -1)
    out = torch.einsum("...j,...jd->...d", w, V)
    tabs = torch.where(ok, t.abs(), torch.zeros_like(t)).max(-1, keepdim=True).values
    arg = chain_t * U32 * (A + (tabs + 1.0 if m_in_chain else 0.0)) + U32 * ((tmax - t).abs() + (tabs + 1.0 if m_in_chain else 0.0))
    if dt_extra is not None:
        arg = arg + dt_extra
    arg = torch.where(ok, arg, torch.zeros_like(arg))
    rel = SLACK * (torch.expm1(ln * arg) + U32 * (INTRIN + n_rescale * (INTRIN + 2.0 + ln * rng)))
    wv = torch.einsum("...j,...jd->...d", w, V.abs())
    e = torch.einsum("...j,...jd->...d", w * rel, V.abs()) + (w * rel).sum(-1, keepdim=True) * out.abs()
    e = e + (UB * wv if p_bf16 else 0.0) + SLACK * U32 * chain_sum * (wv + out.abs()) + U32 * (INTRIN + 1.0) * out.abs()
    e = e + t.shape[-1] * 2.0 * FLUSH * (V.abs().amax((-1, -2)).unsqueeze(-1) + out.abs()) + ETA
    return out, _store(e, out, dt)


# ------------------------------------------------------------------------------------------------------------------------------------
# the VALU streams (dec_cross_attn_kernel, dec_self_attn_kernel): per-slot online softmax, slot butterfly, wave merge
# ------------------------------------------------------------------------------------------------------------------------------------
def valu_geometry(dt, D, unr):
    vec = 8 if dt == B else 4
    lpk = D // vec
    kpi = 64 // lpk
    return vec, lpk, kpi, kpi * unr


def _valu_stream32(qs, K, V, ok, vec, lpk, kpi, unr, nw, base2, defect=None, first_batch_masked=None):
    """qs [B,H,Q,D] fp32 scaled queries; K, V [B,H,n,D] fp32; ok [B,1|H,1|Q,n] bool -> fp32 [B,H,Q,D] = o / l (0 where l = 0 and nw > 1)."""
    Bn, H, Q, D = qs.shape
    n = K.shape[2]
    bk = kpi * unr
    nb = _cdiv(n, bk)
    pad = nb * bk - n
    if pad:
        K = torch.cat([K, K.new_zeros(Bn, H, pad, D)], 2)
        V = torch.cat([V, V.new_zeros(Bn, H, pad, D)], 2)
        ok = torch.cat([ok, ok.new_zeros(ok.shape[:-1] + (pad,))], -1)
    ok = ok.expand(Bn, H, Q, nb * bk)
    qv = qs.view(Bn, H, Q, 1, 1, lpk, vec)
    ms, ls, os_ = [], [], []
    for w in range(nw):
        m = qs.new_full((Bn, H, Q), NINF)
        l = qs.new_zeros(Bn, H, Q, kpi)
        acc = qs.new_zeros(Bn, H, Q, kpi, D)
        raises = torch.zeros(Bn, H, Q, dtype=torch.long)
        for bi in range(w, nb, nw):
            Kb = K[:, :, bi * bk:(bi + 1) * bk].view(Bn, H, 1, unr, kpi, lpk, vec)
            Vb = V[:, :, bi * bk:(bi + 1) * bk].view(Bn, H, 1, unr, kpi, D)
            okb = ok[..., bi * bk:(bi + 1) * bk].reshape(Bn, H, Q, unr, kpi)
            part = qs.new_zeros(Bn, H, Q, unr, kpi, lpk)
            for e in range(vec):
                part = _fma(qv[..., e], Kb[..., e], part)
            o = lpk >> 1
            idx = torch.arange(lpk)
            while o:  # butterfly over the lanes of a key
                part = part + part[..., idx ^ o]
                o >>= 1
            part = torch.where(okb, part[..., 0], torch.full_like(part[..., 0], NINF))
            mn = torch.maximum(m, part.amax((-1, -2)))
            corr = torch.where(m == NINF, torch.zeros_like(m), _exp32(m - mn, base2))
            rose = mn > m
            if defect == "rescale_skipped_on_second_raise":
                corr = torch.where(rose & (raises == 1), torch.ones_like(corr), corr)
            raises = raises + rose.long()
            l = l * corr[..., None]
            acc = acc * corr[..., None, None]
            m = mn
            for u in range(unr):
                pe = torch.where(part[..., u, :] == NINF, torch.zeros_like(l), _exp32(part[..., u, :] - m[..., None], base2))
                l = l + pe
                acc = _fma(pe[..., None], Vb[:, :, :, u], acc)
        if defect == "slot_reduction_misses_last_slot":
            l[..., kpi - 1] = 0.0
            acc[..., kpi - 1, :] = 0.0
        o, idx = 1, torch.arange(kpi)
        while o < kpi:
            l = l + l[..., idx ^ o]
            acc = acc + acc[..., idx ^ o, :]
            o <<= 1
        if defect == "wave_with_masked_first_tile_keeps_minus_inf" and first_batch_masked is not None and w < len(first_batch_masked):
            m = torch.where(first_batch_masked[w].view(Bn, 1, 1), torch.full_like(m, NINF), m)
        ms.append(m), ls.append(l[..., 0]), os_.append(acc[..., 0, :])
    if nw == 1:
        return os_[0] / ls[0][..., None]
    M = torch.stack(ms).amax(0)
    l = qs.new_zeros(Bn, H, Q)
    o = qs.new_zeros(Bn, H, Q, D)
    for w in range(nw):
        if defect == "wave_3_state_not_merged" and w == 3:
            continue
        f = torch.where(ms[w] == NINF, torch.zeros_like(M), torch.exp(ms[w] - M))
        l = l + ls[w] * f
        o = o + os_[w] * f[..., None]
    return torch.where(l[..., None] > 0, o / l[..., None], torch.zeros_like(o))


# ------------------------------------------------------------------------------------------------------------------------------------
# cross attention
# ------------------------------------------------------------------------------------------------------------------------------------
CROSS_S = [1, 31, 32, 33, 97, 128, 129, 289]
VALU_BEAMS = [1, 2, 5, 6, 8, 9, 32, 33]
MC_BEAMS = [1, 5, 31, 32]
MASKS = ("none", "suffix", "prefix", "scattered")
CROSS_DEFECTS = ("last_key_of_ragged_tile_dropped", "mask_bit_of_wrong_register", "second_mask_word_of_ballot_lost", "wave_3_state_not_merged",
                 "rescale_skipped_on_second_raise", "wave_with_masked_first_tile_keeps_minus_inf", "query_row_beam_minus_1_from_row_0",
                 "scale_applied_after_rounding")
CLIMB_KEY, CLIMB_Q = 24.0, 4.0   # sentence 1: keys of a wave's i-th tile carry i * CLIMB_KEY along a unit direction, queries CLIMB_Q along it
ONE_HOT = 60.0                   # sentence 2, query row 0: one key this many log2 units above what the others reach


def _shape_list(beams, S_all, S_beams):
    out = [(S, 5) for S in S_all]
    out += [(S, b) for S in S_beams for b in beams if (S, b) not in out]
    return out


# (dtype, D, H, S, beam): the VALU kernel's cases and the matrix-core kernel's
VALU_CASES = ([(dt, 64, 2, S, b) for dt in (F, B) for (S, b) in _shape_list(VALU_BEAMS, CROSS_S, (33, 289))] +
              [(dt, 32, 3, S, b) for dt in (F, B) for S in (33, 289) for b in (1, 5, 9)])
MC_CASES = [(B, 64, 2 if S != 97 else 3, S, b) for (S, b) in _shape_list(MC_BEAMS, CROSS_S, (97, 289))]


def cross_id(c):
    return "%s-D%d-H%d-S%d-beam%d" % (NAME[c[0]], c[1], c[2], c[3], c[4])


def cross_route(dt, D, beam, valu_only=False):
    """The launcher's choice (cst_dec_cross_attn)."""
    return "mc" if (not valu_only and dt == B and D == 64 and beam <= 32) else "valu"


def one_hot_key(S):
    """The planted key of sentence 2: in the LAST tile of wave 3 (tiles 3, 7, ...), None if wave 3 has no tile."""
    nt = _cdiv(S, 32)
    if nt < 4:
        return None
    tile = 3 + 4 * ((nt - 4) // 4)
    return min(32 * tile + 5, S - 1)


def cross_mask(S, kind):
    """-> uint8 [BSZ, S] (1 = padding) or None.  suffix: the usual right padding; prefix: left padding (whole leading tiles of
    sentences 1 and 2 at S = 289: a wave whose first tile is wholly masked and whose second is not); scattered: the whole tile 5 (wave
    1's second tile) and the single keys 0, 31, 32, 63.  No sentence is left without a key, and sentence 2 keeps its planted key."""
    if kind == "none":
        return None
    j = torch.arange(S)
    if kind == "suffix":
        keep = torch.tensor([max(1, S - 3), max(1, S // 2), S])
        m = j[None, :] >= keep[:, None]
    elif kind == "prefix":
        padl = torch.tensor([0, min(S - 1, 40), min(S - 1, S // 3)])
        m = j[None, :] < padl[:, None]
    else:
        m1 = ((j >= 160) & (j < 192)) | (j == 0) | (j == 31) | (j == 32) | (j == 63)
        if bool(m1.all()):
            m1 = torch.zeros_like(m1)
        m = m1[None, :].expand(BSZ, S).clone()
    jh = one_hot_key(S)
    assert not bool(m.all(1).any()) and (jh is None or not bool(m[2, jh]))
    return m.to(torch.uint8).contiguous()


def cross_inputs(S, beam, H, D, dt, seed=31):
    """q [BSZ * beam, H D], kx, vx head-major [BSZ, H, S, D], scale.  Sentence 0: N(0, 1).  Sentence 1: planted logits that CLIMB — the
    keys of tiles 4 i .. 4 i + 3 carry i * CLIMB_KEY along the unit direction 1 / sqrt(D) and every query exactly CLIMB_Q along it, i.e.
    CLIMB_KEY CLIMB_Q scale log2 e = 17 (D = 64) log2 units per level against a spread of about +-4: the lazy maximum of a wave is raised
    at each of its tiles.  Sentence 2: the key one_hot_key(S) is a multiple of query row 0, ONE_HOT log2 units above its other scores."""
    g = _gen(seed + 1000 * S + 10 * beam + D)
    C = H * D
    q = torch.randn(BSZ, beam, H, D, generator=g)
    kx = torch.randn(BSZ, H, S, D, generator=g)
    vx = torch.randn(BSZ, H, S, D, generator=g)
    scale = D ** -0.5
    d = torch.full((D,), D ** -0.5)
    q[1] = q[1] - (q[1] @ d)[..., None] * d + CLIMB_Q * d
    lvl = (torch.arange(S) // 128).float()
    kx[1] = kx[1] + (lvl * CLIMB_KEY)[None, :, None] * d
    jh = one_hot_key(S)
    if jh is not None:
        q0 = q[2, 0]                                              # [H, D]
        c = scale * LOG2E
        others = (torch.einsum("hd,hjd->hj", q0, kx[2]) * c).amax(-1)   # what the other keys reach (log2 units)
        kx[2, :, jh] = q0 * ((ONE_HOT + others.clamp_min(0.0) + 8.0) / (c * (q0 * q0).sum(-1)))[:, None]
    return q.reshape(BSZ * beam, C).to(dt), kx.to(dt), vx.to(dt), scale


def _split(q, kx, beam):
    Bn, H, S, D = kx.shape
    return q.float().view(Bn, beam, H, D).transpose(1, 2)   # [B, H, Q, D]


def _ok(kpm, Bn, S):
    if kpm is None:
        return torch.ones(Bn, 1, 1, S, dtype=torch.bool)
    return (kpm == 0).view(Bn, 1, 1, S)


def mc_qhat(q, scale):
    """fa_row_frags: bf16(fl32(q c2)), c2 the fp32 product scale * 1.4426950408889634f."""
    c2 = _c(f32(scale)) * _c(LOG2E)
    return bf(q.float() * c2)


def cross64(q, kx, vx, kpm, scale, beam, route, nw=4):
    """-> dict(out, bound) [BSZ * beam, C] in fp64 for the route's kernel."""
    Bn, H, S, D = kx.shape
    dt = q.dtype
    ok = _ok(kpm, Bn, S).expand(Bn, H, beam, S)
    K, V = kx.double(), vx.double()
    if route == "mc":
        qh = mc_qhat(_split(q, kx, beam), scale).double()
        ntile = _cdiv(_cdiv(S, 32), 4)
        kw = dict(base2=True, chain_t=64, chain_sum=32 * ntile + 5, n_rescale=0, m_in_chain=True, p_bf16=True)
    else:
        qh = (_split(q, kx, beam) * _c(f32(scale))).double()
        vec, lpk, kpi, bk = valu_geometry(dt, D, 4)
        nb = _cdiv(_cdiv(S, bk), nw)
        kw = dict(base2=False, chain_t=vec + int(math.log2(lpk)), chain_sum=4 * nb + int(math.log2(kpi)) + nw + 1, n_rescale=nb + 1)
    t = torch.einsum("bhqd,bhjd->bhqj", qh, K)
    A = torch.einsum("bhqd,bhjd->bhqj", qh.abs(), K.abs())
    out, bound = attn_ref_bound(t, A, ok, V[:, :, None], dt, **kw)
    flat = lambda x: x.transpose(1, 2).reshape(Bn * beam, H * D)
    return dict(out=flat(out), bound=flat(bound), t=t, ok=ok)


def _tile_perm_wrong():
    """Key i of a 32-key tile sits in accumulator register r of half-wave hi with i = (r & 3) + 8 (r >> 2) + 4 hi; the planted mapping
    reads i = (r & 3) + 4 (r >> 2) + 16 hi instead."""
    p = torch.zeros(32, dtype=torch.long)
    for hi in range(2):
        for r in range(16):
            p[(r & 3) + 8 * (r >> 2) + 4 * hi] = (r & 3) + 4 * (r >> 2) + 16 * hi
    return p


def _cross_defect_inputs(q4, masked, S, defect):
    """The defects that act on the inputs alike for both kernels.  masked [B, Sp] (Sp = 32 * tiles; keys behind S are masked)."""
    Sp = masked.shape[1]
    if defect == "last_key_of_ragged_tile_dropped" and S % 32:
        masked = masked.clone()
        masked[:, S - 1] = True
    if defect == "mask_bit_of_wrong_register":
        masked = masked.view(-1, Sp // 32, 32)[:, :, _tile_perm_wrong()].reshape(-1, Sp)
    if defect == "second_mask_word_of_ballot_lost":
        masked = masked.clone().view(-1, Sp // 32, 32)
        masked[:, 1::2] = False
        masked = masked.view(-1, Sp)
    if defect == "query_row_beam_minus_1_from_row_0":
        q4 = q4.clone()
        q4[:, :, -1] = q4[:, :, 0]
    return q4, masked


def _padded(kx, vx, kpm):
    Bn, H, S, D = kx.shape
    Sp = 32 * _cdiv(S, 32)
    K = torch.cat([kx.float(), torch.zeros(Bn, H, Sp - S, D)], 2)
    V = torch.cat([vx.float(), torch.zeros(Bn, H, Sp - S, D)], 2)
    masked = torch.ones(Bn, Sp, dtype=torch.bool)
    masked[:, :S] = (kpm != 0) if kpm is not None else False
    return K, V, masked


def valu_cross_emulate32(q, kx, vx, kpm, scale, beam, nw=4, defect=None):
    """dec_cross_attn_kernel op by op (torch.exp stands in for expf).  The kernel tests `j < S` itself: a planted mask defect reaches
    only keys in range."""
    assert defect is None or defect in CROSS_DEFECTS
    Bn, H, S, D = kx.shape
    dt = q.dtype
    vec, lpk, kpi, bk = valu_geometry(dt, D, 4)
    K, V, masked = _padded(kx, vx, kpm)
    fbm = [masked[:, 32 * w:32 * w + 32].all(1) for w in range(4) if 32 * w < masked.shape[1]]
    q4, masked = _cross_defect_inputs(_split(q, kx, beam), masked, S, defect)
    masked = masked.clone()
    masked[:, S:] = True     # the kernel's own `j < S`
    qs = q4 * _c(f32(scale))
    o = _valu_stream32(qs, K, V, ~masked.view(Bn, 1, 1, -1), vec, lpk, kpi, 4, nw, False, defect, fbm)
    return o.transpose(1, 2).reshape(Bn * beam, H * D).to(dt)


def mc_cross_emulate32(q, kx, vx, kpm, scale, beam, defect=None, qhat=None):
    """fa_dec_cross_kernel op by op: 32-key tiles, wave w owns tiles w, w + 4, ..; S^T = K q^ as a 64-long fmaf chain that starts at
    -m (or -inf for a masked key); the integer lazy maximum (FA_THR = 8, ceilf, alpha = exp2(-dm)); P rounded to bf16 for P V, l from the
    fp32 values, per half-wave; the four states merged in wave order at the common integer maximum.  qhat: the query tile when the
    fused projection formed it ([B, H, Q, 64], bf16 values)."""
    assert defect is None or defect in CROSS_DEFECTS
    Bn, H, S, D = kx.shape
    assert D == 64 and q.dtype == B
    K, V, masked = _padded(kx, vx, kpm)
    nt = masked.shape[1] // 32
    first_masked = [masked[:, 32 * w:32 * w + 32].all(1) for w in range(min(4, nt))]
    if qhat is None:
        q4 = _split(q, kx, beam)
        qhat = mc_qhat(q4, scale) if defect != "scale_applied_after_rounding" else q4 * (_c(f32(scale)) * _c(LOG2E))
    qhat, masked = _cross_defect_inputs(qhat, masked, S, defect)
    Q = qhat.shape[2]
    half = ((torch.arange(32) >> 2) & 1).bool()   # keys of half-wave 1
    ms, ls, os_ = [], [], []
    for w in range(4):
        negm = torch.zeros(Bn, H, Q)
        raise_at = torch.full((Bn, H, Q), NINF)
        l = torch.zeros(Bn, H, Q, 2)
        o = torch.zeros(Bn, H, Q, 64)
        raises = torch.zeros(Bn, H, Q, dtype=torch.long)
        for tile in range(w, nt, 4):
            Kt, Vt = K[:, :, None, 32 * tile:32 * tile + 32], V[:, :, None, 32 * tile:32 * tile + 32]   # [B,H,1,32,64]
            mk = masked[:, None, None, 32 * tile:32 * tile + 32]
            s = torch.where(mk, torch.full((Bn, H, Q, 32), NINF), negm[..., None].expand(Bn, H, Q, 32))
            for k in range(64):
                s = _fma(Kt[..., k], qhat[..., None, k], s)
            mt = s.amax(-1)
            need = mt > raise_at
            first = raise_at < 0
            dm = torch.where(need, torch.ceil(mt), torch.zeros_like(mt))
            alpha = torch.where(first, torch.ones_like(dm), torch.exp2(-dm))
            if defect == "rescale_skipped_on_second_raise":
                alpha = torch.where(need & (raises == 1), torch.ones_like(alpha), alpha)
            raises = raises + need.long()
            o = o * alpha[..., None]
            l = l * alpha[..., None]
            negm = negm - dm
            s = s - dm[..., None]
            raise_at = torch.where(need, torch.full_like(raise_at, 8.0), raise_at)
            p = torch.exp2(s)
            for hi in range(2):
                ph = p[..., half == bool(hi)]          # this half-wave's 16 keys, register order
                for r in range(0, 16, 2):
                    l[..., hi] = l[..., hi] + (ph[..., r] + ph[..., r + 1])
            pb = bf(p)
            for j in range(32):
                o = _fma(pb[..., j, None], Vt[..., j, :].expand(Bn, H, Q, 64), o)
        mw = torch.where(raise_at < 0, torch.full_like(negm, NINF), -negm)
        if defect == "wave_with_masked_first_tile_keeps_minus_inf" and w < nt:
            mw = torch.where(first_masked[w].view(Bn, 1, 1), torch.full_like(mw, NINF), mw)
        ms.append(mw), ls.append(l), os_.append(o)
    M = torch.stack(ms).amax(0)
    l = torch.zeros(Bn, H, Q, 2)
    o = torch.zeros(Bn, H, Q, 64)
    for w in range(4):
        if defect == "wave_3_state_not_merged" and w == 3:
            continue
        f = torch.where(ms[w] == NINF, torch.zeros_like(M), torch.exp2(ms[w] - M))
        l = l + ls[w] * f[..., None]
        o = o + os_[w] * f[..., None]
    lt = l[..., 0] + l[..., 1]
    inv = torch.where(lt > 0, 1.0 / lt, torch.zeros_like(lt))
    return (o * inv[..., None]).transpose(1, 2).reshape(Bn * Q, H * 64).to(B)


def cross_emulate32(q, kx, vx, kpm, scale, beam, route, defect=None, nw=4):
    if route == "mc":
        return mc_cross_emulate32(q, kx, vx, kpm, scale, beam, defect)
    return valu_cross_emulate32(q, kx, vx, kpm, scale, beam, nw, defect)


# ------------------------------------------------------------------------------------------------------------------------------------
# self-attention
# ------------------------------------------------------------------------------------------------------------------------------------
SELF_ROWS, SELF_H, SELF_UNR = 5, 3, 8
SELF_CASES = [(dt, D) for dt in (F, B) for D in (32, 64)]
SELF_DEFECTS = ("ancestor_of_previous_parity", "position_s_read_from_cache", "batch_boundary_key_dropped", "slot_reduction_misses_last_slot")
DOMINANT = 6.0    # head 1: the key at position 1 is this multiple of the query (its score leads by tens of units)


def self_geometry(dt, D):
    """(KPI * UNR, max_len, steps): each configuration's own batch of keys."""
    bk = valu_geometry(dt, D, SELF_UNR)[3]
    max_len = 2 * bk + 3
    return bk, max_len, [0, 1, bk - 1, bk, bk + 1, 2 * bk, max_len]


def self_fast(dt, D):
    return dt == B and D == 64


def self_inputs(dt, D, s, seed=41):
    """qkv [rows, 3 C], caches kc, vc [rows, H, L1, D] (N(0, 1) everywhere: a stale slot s is visible if it is read), the ancestry
    table anc [2, rows, L1]: parity s & 1 a shuffle (own row at position s), the other parity DIFFERENT rows everywhere."""
    rows, H = SELF_ROWS, SELF_H
    bk, max_len, _ = self_geometry(dt, D)
    L1, C = max_len + 1, H * D
    g = _gen(seed + D)
    kc = torch.randn(rows, H, L1, D, generator=g)
    vc = torch.randn(rows, H, L1, D, generator=g)
    qkv = torch.randn(rows, 3 * C, generator=g)
    g2 = _gen(seed + 7 * s + D)
    a = torch.randint(0, rows, (rows, L1), generator=g2)
    a[:, s] = torch.arange(rows)
    anc = torch.stack([a, (a + 1 + torch.randint(0, rows - 1, (rows, L1), generator=g2)) % rows])
    if s & 1:
        anc = anc.flip(0)
    assert bool((anc[0] != anc[1]).all())
    if s >= 1:   # the dominant early key of head 1: position 1 of whichever row the ancestry names
        qh = qkv[:, D:2 * D]
        if s == 1:
            qkv[:, C + D:C + 2 * D] = DOMINANT * qh
        else:
            for r in range(rows):
                kc[anc[s & 1, r, 1], 1, 1] = DOMINANT * qh[r]   # (rows that share an ancestor share the key: the last writer's query)
    return qkv.to(dt), kc.to(dt), vc.to(dt), anc.int().contiguous(), D ** -0.5


def _self_gather(qkv, kc, vc, anc, s, defect=None):
    rows, H, L1, D = kc.shape
    C = H * D
    a = anc[(s & 1) ^ (1 if defect == "ancestor_of_previous_parity" else 0)].long()[:, :s + 1]
    pos = torch.arange(s + 1)
    K = kc[a, :, pos].transpose(1, 2).clone()     # [rows, H, s + 1, D]
    V = vc[a, :, pos].transpose(1, 2).clone()
    if defect == "position_s_read_from_cache":
        r = torch.arange(rows)
        K[:, :, s], V[:, :, s] = kc[r, :, s], vc[r, :, s]
    else:
        K[:, :, s] = qkv[:, C:2 * C].view(rows, H, D)
        V[:, :, s] = qkv[:, 2 * C:].view(rows, H, D)
    return qkv[:, :C].view(rows, H, 1, D), K, V


def _self_q(q, scale, fast):
    qs = q.float() * _c(f32(scale))
    return qs * _c(LOG2E) if fast else qs


def self64(qkv, kc, vc, anc, s, scale):
    """-> dict(out, bound [rows, C], kc, vc: the caches after the append)."""
    rows, H, L1, D = kc.shape
    dt = qkv.dtype
    fast = self_fast(dt, D)
    q, K, V = _self_gather(qkv, kc, vc, anc, s)
    qs = _self_q(q, scale, fast).double()
    vec, lpk, kpi, bk = valu_geometry(dt, D, SELF_UNR)
    nb = _cdiv(s + 1, bk)
    t = torch.einsum("rhqd,rhjd->rhqj", qs, K.double())
    A = torch.einsum("rhqd,rhjd->rhqj", qs.abs(), K.double().abs())
    out, bound = attn_ref_bound(t, A, torch.ones_like(t, dtype=torch.bool), V.double()[:, :, None], dt, base2=fast,
                                chain_t=vec + int(math.log2(lpk)), chain_sum=SELF_UNR * nb + int(math.log2(kpi)) + 1, n_rescale=nb)
    kc2, vc2 = kc.clone(), vc.clone()
    kc2[:, :, s], vc2[:, :, s] = K[:, :, s], V[:, :, s]
    return dict(out=out.reshape(rows, H * D), bound=bound.reshape(rows, H * D), kc=kc2, vc=vc2)


def self_emulate32(qkv, kc, vc, anc, s, scale, defect=None):
    assert defect is None or defect in SELF_DEFECTS
    rows, H, L1, D = kc.shape
    dt = qkv.dtype
    fast = self_fast(dt, D)
    q, K, V = _self_gather(qkv, kc, vc, anc, s, defect)
    vec, lpk, kpi, bk = valu_geometry(dt, D, SELF_UNR)
    ok = torch.ones(rows, 1, 1, s + 1, dtype=torch.bool)
    if defect == "batch_boundary_key_dropped" and s >= bk:
        ok[..., bk] = False
    o = _valu_stream32(_self_q(q, scale, fast), K.float(), V.float(), ok, vec, lpk, kpi, SELF_UNR, 1, fast, defect)
    return o.reshape(rows, H * D).to(dt)


# ------------------------------------------------------------------------------------------------------------------------------------
# Linear and LayerNorm-folded Linear
# ------------------------------------------------------------------------------------------------------------------------------------
LIN_CASES = [("NT1/UN4", 81, 40, 1024), ("NT1/UN2", 1, 17, 512), ("NT1/UN2", 80, 520, 1536), ("NT2/UN4", 81, 2576, 1024),
             ("NT2/UN2", 81, 2576, 1536), ("NT4/UN2", 161, 5472, 512), ("NT4/UN2", 161, 5472, 1024)]
LIN_DEFECTS = ("k_quarter_of_last_wave_dropped", "prefetched_step_used_twice", "row_80_from_row_79", "bias_of_column_n_minus_1", "resid_with_ldy",
               "activation_after_residual")
LN_DEFECTS = ("sg_of_wrong_head", "mean_over_kq", "variance_without_mean_square", "eps_outside_sqrt", "fragment_major_halves_swapped")
LN_EPS = 1e-5
LN_KINDS = ("mean0", "mean3", "mean30", "const", "tiny", "small")
ACTS = ("none", "relu", "gelu")


def lin_id(c):
    return "%s-M%d-N%d-K%d" % (c[0].replace("/", ""), c[1], c[2], c[3])


def lin_dispatch(M, N, K, env_nw=0):
    """dec_linear_impl's choice: (instantiation name, NT, UN, NW, k-steps per wave, loop iterations, workgroups of one column tile)."""
    wg1 = _cdiv(N, 16) * _cdiv(M, 80)
    nw = env_nw if env_nw in (4, 8, 16) else 8
    while nw > 4 and K % (nw * 64):
        nw >>= 1
    steps = K // nw // 32
    if wg1 <= 320:
        nt, un = 1, (4 if nw == 4 or steps % 4 == 0 else 2)
    elif wg1 <= 1024:
        nw = 8 if nw == 16 else nw
        steps = K // nw // 32
        nt, un = 2, (4 if nw == 4 or steps % 4 == 0 else 2)
    else:
        nt, un, nw = 4, 2, 4
        steps = K // nw // 32
    return dict(name="NT%d/UN%d" % (nt, un), nt=nt, un=un, nw=nw, steps=steps, iters=_cdiv(steps, un), wg1=wg1)


def ln_rows(M, K, seed):
    """Rows of mean 0, 3 sigma and 30 sigma, one constant row (2.0), one row of tiny spread (1e-3) around 5 and one of small elements
    (1e-3 N(0, 1): var = 1e-6 < eps without a mean to cancel, the row on which eps in the wrong place shows), cycled.  bf16 has a spacing
    of 2^-5 at 5: the tiny row would round to a second constant row, so every 7th element of it is moved one bf16 step up — the
    smallest spread the format can hold there."""
    g = _gen(seed)
    x = torch.randn(M, K, generator=g)
    for r in range(M):
        kd = LN_KINDS[r % len(LN_KINDS)]
        if kd == "mean3":
            x[r] += 3.0
        elif kd == "mean30":
            x[r] += 30.0
        elif kd == "const":
            x[r] = 2.0
        elif kd == "tiny":
            x[r] = 5.0 + 1e-3 * x[r]
        elif kd == "small":
            x[r] = 1e-3 * x[r]
    xb = x.to(B)
    for r in range(M):
        if LN_KINDS[r % len(LN_KINDS)] == "tiny":
            xb[r, ::7] = 5.03125
    return xb


def lin_inputs(M, N, K, ln, seed=51):
    """x [M, K + 8] (ldx > K; the tail holds 1000s that must not be read), W [N, K] N(0, 1 / K), bias [N], resid [M, N + 16], and for
    ln: Wg = W, sg = the fp32 row sums of Wg, sb N(0, 1) (fp32) — taken as given by the kernel."""
    g = _gen(seed + M + N + K)
    xs = torch.full((M, K + 8), 1000.0, dtype=B)
    xs[:, :K] = ln_rows(M, K, seed + K) if ln else torch.randn(M, K, generator=g).to(B)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(B)
    bias = torch.randn(N, generator=g).to(B)
    resid = torch.randn(M, N + 16, generator=g).to(B)
    sg = W.float().sum(1)
    sb = torch.randn(N, generator=g)
    return dict(x=xs, W=W, bias=bias, resid=resid, sg=sg, sb=sb, K=K)


def lnfold64(x, Wg, sg, sb, eps, chain_v, chain_s):
    """y = rstd (x Wg^T - mean sg) + sb in fp64 and its bound.  v: chain_v u on sum |x| |Wg|.  mean = fl(s1 / K): (chain_s + INTRIN) u
    on sum |x| / K.  var~ = max(fl(s2 / K) - mean~^2, 0): (chain_s + INTRIN) u E[x^2], 2 |mean| d_mean + d_mean^2, the product and the
    difference (2 u mean^2 + u E[x^2]).  rstd~ lies between the rsqrt of the two ends of var + eps -+ d_var (an interval: a constant
    row has var = 0 and d_var of the order of eps), INTRIN u on top.  t = v - mean sg: d_v + |sg| d_mean + u |mean sg| + u |t|.
    y = fma(rstd, t, sb): rstd (1 + rel) d_t + |rstd t| rel + u |y|."""
    x, Wg, sg, sb = x.double(), Wg.double(), sg.double()[None, :], sb.double()[None, :]
    K = x.shape[1]
    v = x @ Wg.t()
    d_v = SLACK * chain_v * U32 * (x.abs() @ Wg.abs().t())
    mean = x.mean(1, keepdim=True)
    ex2 = (x * x).mean(1, keepdim=True)
    var = (ex2 - mean * mean).clamp_min(0.0)
    d_mean = SLACK * (chain_s + INTRIN) * U32 * x.abs().mean(1, keepdim=True)
    d_var = SLACK * ((chain_s + INTRIN + 1.0) * U32 * ex2 + 2.0 * mean.abs() * d_mean + d_mean * d_mean + 2.0 * U32 * mean * mean)
    rstd = (var + eps).rsqrt()
    hi = ((var - d_var).clamp_min(0.0) + eps).rsqrt()
    lo = (var + d_var + eps).rsqrt()
    rel = torch.maximum(hi / rstd - 1.0, 1.0 - lo / rstd) * SLACK + (INTRIN + 1.0) * U32
    t = v - mean * sg
    d_t = d_v + sg.abs() * d_mean + U32 * (mean * sg).abs() + U32 * (t.abs() + d_v + sg.abs() * d_mean)
    y = rstd * t + sb
    d_y = SLACK * (rstd * (1.0 + rel) * d_t + (rstd * t).abs() * rel) + U32 * y.abs() + ETA
    return y, d_y


def lin64(p, ln, act, has_bias, has_resid, nw):
    """-> dict(y, bound) [M, N] of cst_dec_linear (ln False) / cst_dec_ln_linear on lin_inputs' tensors."""
    K = p["K"]
    x, W = p["x"][:, :K].double(), p["W"].double()
    chain = K // nw + nw - 1
    if ln:
        z, d_z = lnfold64(x, W, p["sg"], p["sb"], LN_EPS, chain, K // nw // 4 + 2 + nw)
    else:
        z = x @ W.t()
        d_z = SLACK * chain * U32 * (x.abs() @ W.abs().t())
        if has_bias:
            z = z + p["bias"].double()
            d_z = d_z + U32 * z.abs()
        d_z = d_z + ETA
    if act == "relu":
        y, d_y = torch.relu(z), d_z
    elif act == "gelu":
        y = gelu64(z)
        d_y = (dgelu64(z).abs() + 0.8 * d_z) * d_z + a_gelu(z, B)
    else:
        y, d_y = z, d_z
    if has_resid:
        y = y + p["resid"][:, :p["W"].shape[0]].double()
        d_y = d_y + U32 * y.abs()
    return dict(y=y, bound=_store(d_y, y, B))


def _mfma_chain32(x, Wt, k0, k1, acc=None):
    """acc[m, n] += x[m, k] W[n, k] for k = k0 .. k1 - 1 in k order, fp32, one rounding per product and per sum (Wt = W^T, [K, N])."""
    acc = torch.zeros(x.shape[0], Wt.shape[1]) if acc is None else acc
    for k in range(k0, k1):
        acc.addcmul_(x[:, k, None], Wt[k][None, :])
    return acc


def _ln_stats32(x, nw, defect=None):
    """sum(x), sum(x^2) of every row as the kernel gathers them: lane group c of wave w adds the elements 8 c .. 8 c + 7 of each 32-wide
    k-step of the wave's K range in order, the four groups meet by two shuffles, the waves in wave order."""
    M, K = x.shape
    kq = K // nw
    xs = x.view(M, nw, kq // 32, 4, 8).permute(0, 1, 3, 2, 4).reshape(M, nw, 4, kq // 4)
    s1 = torch.zeros(M, nw, 4)
    s2 = torch.zeros(M, nw, 4)
    for i in range(kq // 4):
        f = xs[..., i]
        s1 = s1 + f
        s2 = _fma(f, f, s2)
    s1 = (s1[..., 0] + s1[..., 1]) + (s1[..., 2] + s1[..., 3])
    s2 = (s2[..., 0] + s2[..., 1]) + (s2[..., 2] + s2[..., 3])
    a, b2 = s1[:, 0], s2[:, 0]
    for w in range(1, nw):
        a, b2 = a + s1[:, w], b2 + s2[:, w]
    div = _c(float(kq if defect == "mean_over_kq" else K))
    mean = a / div
    var = b2 / div if defect == "variance_without_mean_square" else b2 / div - mean * mean
    var = var.clamp_min(0.0)
    if defect == "eps_outside_sqrt":
        rstd = 1.0 / (var.sqrt() + _c(LN_EPS))
    else:
        rstd = 1.0 / (var + _c(LN_EPS)).sqrt()
    return mean[:, None], rstd[:, None]


def lin_emulate32(p, ln, act, has_bias, has_resid, nw, un, defect=None):
    """dec_linear_kernel op by op (without the workgroup tiling, which does not change a value): wave w's MFMA chain over its K range,
    the wave-order sum, LayerNorm fold or bias, activation, residual, bf16 store.  -> [M, N] bf16."""
    assert defect is None or defect in LIN_DEFECTS + LN_DEFECTS
    K = p["K"]
    N = p["W"].shape[0]
    x = p["x"][:, :K].float()
    M = x.shape[0]
    if defect == "row_80_from_row_79" and M > 80:
        x = x.clone()
        x[80] = x[79]
    Wt = p["W"].float().t().contiguous()
    kq = K // nw
    v = None
    for w in range(nw):
        k0, k1 = w * kq, (w + 1) * kq
        if defect == "k_quarter_of_last_wave_dropped" and w == nw - 1:
            k1 -= kq // 4
        if defect == "prefetched_step_used_twice" and kq > 32 * un:   # iteration 1 multiplies by the weights of iteration 0
            a = _mfma_chain32(x, Wt, k0, k0 + 32 * un)
            a = _mfma_chain32(x[:, 32 * un:], Wt, k0, k0 + 32 * un, a)
            a = _mfma_chain32(x, Wt, k0 + 64 * un, k1, a)
        else:
            a = _mfma_chain32(x, Wt, k0, k1)
        v = a if v is None else v + a
    if ln:
        mean, rstd = _ln_stats32(x, nw, defect)
        sg = p["sg"].roll(64) if defect == "sg_of_wrong_head" else p["sg"]
        o = _fma(rstd, v - mean * sg[None, :], p["sb"][None, :])
    else:
        o = v
        if has_bias:
            o = o + (p["bias"].roll(1) if defect == "bias_of_column_n_minus_1" else p["bias"]).float()[None, :]
    r = None
    if has_resid:
        r = p["resid"].float()
        r = r.reshape(-1)[:M * (N + 8)].view(M, N + 8)[:, :N] if defect == "resid_with_ldy" else r[:, :N]
    if defect == "activation_after_residual" and r is not None:
        o, r = o + r, None
    if act == "relu":
        o = torch.relu(o)
    elif act == "gelu":
        o = gelu32(o, B)
    if r is not None:
        o = o + r
    return o.to(B)


# ------------------------------------------------------------------------------------------------------------------------------------
# the fused LayerNorm + query projection + cross attention (cst_dec_ln_q_cross_attn)
# ------------------------------------------------------------------------------------------------------------------------------------
QX_CASES = [(4, 5, 289), (8, 5, 129), (4, 32, 97), (8, 1, 33)]    # (H, beam, S): H 64 = 256 / 512 -> one / two K iterations of a wave
QX_SPREAD = 2.5                                                  # target standard deviation of a row's scores (natural units)


def qx_id(c):
    return "H%d-beam%d-S%d" % c


def qx_inputs(H, beam, S, seed=61):
    """x [BSZ * beam, C + 8] (ldx > C) with rows of mean 0 / 0.3 / 3 and every fourth row of small elements (1e-3 N(0, 1)), Wg [C, C], sg, sb, and keys / values as cross_inputs builds them
    with the keys scaled so that a row's scores have a standard deviation of QX_SPREAD: LN(x) has unit elements, q = LN(x) Wg^T about unit
    elements, q . k / 8 a deviation of |k| elements -> keys N(0, QX_SPREAD^2)."""
    C = H * 64
    g = _gen(seed + H + beam + S)
    x = torch.full((BSZ * beam, C + 8), 1000.0, dtype=B)
    xf = torch.randn(BSZ * beam, C, generator=g) * 1.5 + torch.tensor([0.0, 0.3, 3.0])[torch.arange(BSZ * beam) % 3, None]
    xf[3::4] = 1e-3 * (xf[3::4] - torch.tensor([0.0, 0.3, 3.0])[torch.arange(3, BSZ * beam, 4) % 3, None])
    x[:, :C] = xf.to(B)
    Wg = (torch.randn(C, C, generator=g) / C ** 0.5).to(B)
    sg = Wg.float().sum(1)
    sb = 0.1 * torch.randn(C, generator=g)
    kx = (QX_SPREAD * torch.randn(BSZ, H, S, 64, generator=g)).to(B)
    vx = torch.randn(BSZ, H, S, 64, generator=g).to(B)
    return dict(x=x, Wg=Wg, sg=sg, sb=sb, kx=kx, vx=vx, C=C, scale=0.125)


def qx64(p, kpm, beam):
    """q = LN-folded projection (lnfold64 with the fused kernel's chains: K / 4 + 3 for v, K / 8 + 1 + 4 for the sums); the kernel rounds
    it to bf16, multiplies by c2 and rounds again: d_q^ = c2 (d_q (1 + UBF) + UBF |q|) + (u + UBF) |q c2|, which reaches the score of
    key j as sum_d |k_jd| d_q^_d."""
    C, H = p["C"], p["C"] // 64
    Bn, _, S, _ = p["kx"].shape
    q, d_q = lnfold64(p["x"][:, :C], p["Wg"], p["sg"], p["sb"], LN_EPS, C // 4 + 3, C // 8 + 5)
    c2 = float(_c(f32(p["scale"])) * _c(LOG2E))
    qh = q * c2
    d_qh = c2 * (d_q * (1.0 + UB) + UB * q.abs()) + (U32 + UB) * (qh.abs() + c2 * d_q)
    sp = lambda z: z.view(Bn, beam, H, 64).transpose(1, 2)
    K, V = p["kx"].double(), p["vx"].double()
    t = torch.einsum("bhqd,bhjd->bhqj", sp(qh), K)
    A = torch.einsum("bhqd,bhjd->bhqj", sp(qh).abs() + sp(d_qh), K.abs())
    extra = torch.einsum("bhqd,bhjd->bhqj", sp(d_qh), K.abs())
    ok = _ok(kpm, Bn, S).expand(Bn, H, beam, S)
    out, bound = attn_ref_bound(t, A, ok, V[:, :, None], B, base2=True, chain_t=64, chain_sum=32 * _cdiv(_cdiv(S, 32), 4) + 5, n_rescale=0,
                                m_in_chain=True, p_bf16=True, dt_extra=extra)
    flat = lambda z: z.transpose(1, 2).reshape(Bn * beam, C)
    return dict(out=flat(out), bound=flat(bound), q=q, t=t)


def frag_address(h, n, k, K):
    """Element offset of Wg[h * 64 + n][k] in the fragment-major packing (include/cst.h):
    [head][32-column block][k / 16][lane = 32 (k / 8 % 2) + column % 32][8]."""
    return (((h * 2 + n // 32) * (K // 16) + k // 16) * 64 + 32 * (k // 8 % 2) + n % 32) * 8 + k % 8


def qx_emulate32(p, kpm, beam, defect=None):
    assert defect is None or defect in LN_DEFECTS + CROSS_DEFECTS
    C, H = p["C"], p["C"] // 64
    Bn = p["kx"].shape[0]
    x = p["x"][:, :C].float()
    Wg = p["Wg"].float()
    if defect == "fragment_major_halves_swapped":   # the two 8-wide halves of every 16 k's change places
        Wg = Wg.view(C, C // 16, 2, 8).flip(2).reshape(C, C)
    Wt = Wg.t().contiguous()
    kq = C // 4
    a = None
    for w in range(4):
        aw = _mfma_chain32(x, Wt, w * kq, (w + 1) * kq)
        a = aw if a is None else a + aw
    # row sums: each half-wave adds its 8 of every 16 k's in order, the halves meet, then the waves
    M = x.shape[0]
    xs = x.view(M, 4, kq // 16, 2, 8).permute(0, 1, 3, 2, 4).reshape(M, 4, 2, kq // 2)
    s1, s2 = torch.zeros(M, 4, 2), torch.zeros(M, 4, 2)
    for i in range(kq // 2):
        s1 = s1 + xs[..., i]
        s2 = _fma(xs[..., i], xs[..., i], s2)
    s1, s2 = s1[..., 0] + s1[..., 1], s2[..., 0] + s2[..., 1]
    t1, t2 = torch.zeros(M), torch.zeros(M)
    for w in range(4):
        t1, t2 = t1 + s1[:, w], t2 + s2[:, w]
    div = _c(float(kq if defect == "mean_over_kq" else C))
    mean = t1 / div
    var = (t2 / div if defect == "variance_without_mean_square" else t2 / div - mean * mean).clamp_min(0.0)
    rstd = 1.0 / (var.sqrt() + _c(LN_EPS)) if defect == "eps_outside_sqrt" else 1.0 / (var + _c(LN_EPS)).sqrt()
    sg = p["sg"].roll(64) if defect == "sg_of_wrong_head" else p["sg"]
    ql = bf(_fma(rstd[:, None], a - mean[:, None] * sg[None, :], p["sb"][None, :]))
    qhat = bf(ql * (_c(f32(p["scale"])) * _c(LOG2E))).view(Bn, beam, H, 64).transpose(1, 2)
    cd = defect if defect in CROSS_DEFECTS else None
    return mc_cross_emulate32(torch.empty(0, dtype=B), p["kx"], p["vx"], kpm, p["scale"], beam, cd, qhat=qhat)


# ------------------------------------------------------------------------------------------------------------------------------------
# embed
# ------------------------------------------------------------------------------------------------------------------------------------
EMBED_CS = [8, 200, 520]      # C = 8, below and above one pass of the 256 threads, neither a multiple of 256


def embed_ref(tokens, s, E, P, scale, pad, max_len):
    """Exact: fl(fl(scale E[token]) + P[min(pad + 1 + s, rows - 1)]) in fp32, no fused multiply-add, stored in E's dtype."""
    pr = min(pad + 1 + s, P.shape[0] - 1)
    e = E[tokens[s & 1, :, s]].float()
    return ((e * torch.tensor(f32(scale), dtype=F, device=e.device)) + P[pr]).to(E.dtype)
