"""fp64 restatements, counted forward-error bounds and fp32 emulations of the sliding-window kernels of the positional convolution in
csrc/posconv.hip: cst_posconv_fwd, cst_posconv_dx, cst_posconv_dw.  Plain torch on the CPU; shared by test_posconv_ref_cpu.py (the
bounds hold for a faithful fp32 evaluation in two summation shapes and reject every listed defect) and test_posconv_gpu.py (the kernels,
and the implicit-GEMM route of functional._PosConvGemmFn, under the same bounds).  Built like norm_ref.py, whose constants and GELU pieces
are used here; nothing about the GELU is restated.

The operations (bf16 in, bf16 out, C = 48 G channels, k <= 128 taps, padl = k // 2):
    z[b, t, g co]  = bias[g co] + sum_j sum_ci x[b, t - padl + j, g ci] w[g co, ci, j]        (frames outside [0, T) are zero)
    y              = x + GELU(z)
    dx[b, m, g ci] = dy[b, m, g ci] + sum_j sum_co dz[b, m + padl - j, g co] w[g co, ci, j]
    dw[g co, ci, j] = sum_b sum_t dz[b, t, g co] x[b, t - padl + j, g ci]                      db[c] = sum_b sum_t dz[b, t, c]
For even k this is torch's conv1d with padding k / 2 on both sides and the LAST output frame dropped (SamePad).  The kernels write dx
as a window sum over dz with the flipped weight: tap j' = k - 1 - j reads frame m - left + j', left = k - 1 - k // 2.

How the bounds are built.  A product of two bf16 values is exact in fp32.  The accumulator of one output element is the sum of its n
NONZERO products (adding an exact zero rounds nothing: zero padding, zeroed frames and dead blocks do not count), formed by
v_mfma_f32_32x32x16_bf16 in an order and with an internal rounding this file does NOT assume — neither is documented, and nobody here
has measured them.  Whatever the order, a sum of n terms passes at most n - 1 roundings per term:
    |acc - exact| <= (n - 1) u32 sum |terms|
That is the worst case over all summation orders; it was chosen because it needs no assumption about the instruction (a chain in K
order meets it, and so does any tree).  It is far above a typical error, so a worst err / bound well below 1 for dw or dx is expected.
Then the epilogue is counted as gemm_common.h's epilogue_store8 performs it (alpha = 1 multiplies exactly):
    z    the bias add 1 (on |z|), the bf16 store
    y    gelu_t<bf16> of the UNROUNDED fp32 value (the first line of norm_ref._gelu_out_bound with the propagated bound; the store of
         that function comes later here), the residual add 1 (on |y|), the bf16 store
    dx   the accumulator, the residual add 1 (on |dx|), the bf16 store
    dw   the accumulator, the bf16 store
    db   posconv_dw_kernel: thread t adds rows t / 8 and 32 + t / 8 of every K block to its partial (2 nkb additions, the first to an
         exact zero: 2 nkb - 1 roundings), then 32 partials are added in row order (31): chain = 2 nkb + 30; the bf16 store
No constant here was fitted to an output of a kernel or of an emulation.

The emulations evaluate the same sums in fp32 in two shapes, both of which must stay inside the bounds:
    "seq"      a strictly sequential chain in the kernel's K order (forward / dX: tap-major, channel-minor; dW: ascending rows of the
               zero-padded [B, Tp] frame axis)
    "chunk16"  16 consecutive K values summed exactly (in fp64: 16 products of 16 significant bits), one fp32 rounding per chunk
Rows of the dW axis whose dz is entirely zero are skipped in both: they add exact zeros.

Inputs (case): deterministic per name, bf16-exact, no subnormals; the first and the last min(L, 4) live frames of every utterance are
four times larger in x, dy and dz, so that a frame leaking across an utterance boundary or into the padding is larger than any bound.
With limits, x, dy and dz are zero from the limit on, as the callers of functional.pos_conv_gelu_residual guarantee."""
import functools
import zlib

import torch

from norm_ref import ETA, SLACK, U32, _colsum_bound, _gelu_out_bound, _store, a_gelu, dgelu64, gelu32, gelu64, worst_ratio  # noqa: F401

BF = torch.bfloat16
CG, KMAX = 48, 128            # channels per group, taps (posconv.hip)
FBM, TAPS = 256, 4            # forward / dX: frames per workgroup, taps per weight stage
DTJ, DNS, DKLIST = 8, 6, 1024  # dW: taps per workgroup, ring stages, entries of the live-block list

FWD_DEFECTS = ("last_tap_dropped", "tail_stage_dropped", "window_one_frame_late", "even_k_keeps_last_frame_drops_first",
               "next_group_channels", "second_block_reads_first_window", "bias_after_gelu", "residual_missing", "limit_row_not_zeroed")
DX_DEFECTS = tuple(d for d in FWD_DEFECTS if d != "bias_after_gelu")   # (dX has no bias)
DW_DEFECTS = ("frames_leak_across_utterances", "last_k_block_dropped", "blocks_past_1024_dropped", "tap_block_offset_ignored",
              "lp_is_k_half", "db_rows_32_63_dropped", "db_from_every_tap_block")


# ------------------------------------------------------------------------------------------------------------------------------------
# cases: name -> (B, T, G, k).  Every path named in a comment is reached by that case; geometry() derives the counts the comments
# quote from the kernel's constants, and test_posconv_ref_cpu.py asserts them.
# ------------------------------------------------------------------------------------------------------------------------------------
CASES = {
    # forward / dX (all of these also run dW)
    "one": (1, 1, 1, 1),         # one item; k = 1, left = 0 in both directions, partial stage only; dW: Tp = 1 (magic wraps to 0), nkb = 1,
                                 # ntb = 1 with fewer than 8 taps, 1 item (n8 = 0)
    "tail3": (3, 5, 2, 3),       # k < 4: the partial-stage branch alone; dW: ntb = 1 with 3 taps, nkb = 1 (T < k: many_utts)
    "full4": (2, 70, 1, 4),      # k = 4: one full stage, no tail; even k: forward left = 2, dX left = 1; dW: even k, scalar store
    "full4p1": (2, 70, 3, 5),    # k = 5: a full stage + a 1-tap tail; G = 3
    "k126": (3, 256, 2, 126),    # even k, no multiple of 4: 2-tap tail; T = one frame block exactly; dW: even k with k % 8 != 0 (scalar
                                 # store with even-k offsets), last tap block holds 6 taps; G ntb = 32
    "k127": (3, 257, 2, 127),    # a second frame block that holds one row; 12 items (n8 = 1, r8 = 4)
    "k128": (1, 300, 1, 128),    # 2 items (n8 = 0); dW: 16 items
    "blocks3": (3, 600, 3, 128),  # three frame blocks, 27 items (n8 = 3, r8 = 3); dW: 48 items
    # dW only
    "nkb2": (2, 40, 1, 8),       # nkb = 2 < DNS - 1: the prologue is partly issued, pc_wait_vmcnt<0> from the first iteration; k = 8: one
                                 # full tap block on the 16-byte store8 path; one item
    "nkb5": (2, 150, 1, 9),      # nkb = 5 = DNS - 1 exactly; k = 9: a second tap block that holds one tap; 2 items; db == nullptr
                                 # (test_posconv_gpu.py calls it directly with and without db, as k126)
    "wrap": (2, 190, 3, 16),     # nkb = 7: stage 0 of the ring is used a second time; 6 items (n8 = 0, G ntb no multiple of 8); with
                                 # grad_rows = (0, 0) and dz = 0 every K block is dead (nk = 0): dw and db are written as zeros
    "remap9": (2, 50, 3, 24),    # 9 dW items (n8 = 1, r8 = 1): XCD 0 owns two items, the others one (not in the issue's table: added)
    "many_utts": (40, 1, 1, 3),  # Tp = 3 < 64: a K block spans 21 utterances, the `while (pp >= Tp)` loop runs many times
    "past_list": (2, 33000, 1, 8),  # nkb = 1032 > DKLIST: the live-block list is abandoned, every block runs, with and without stamps
}
FWD_CASES = ("one", "tail3", "full4", "full4p1", "k126", "k127", "k128", "blocks3")
DW_ONLY_CASES = ("nkb2", "nkb5", "wrap", "remap9", "many_utts", "past_list")
# lens = grad_rows.  k127: utterance 1's second frame block is dead behind a live first one (m0 = 256 >= m_len = 100 + left > 0), utterance 2
# has nothing live; dW: dead K blocks are dropped from the list
LIMITS = {"k127": (257, 100, 0), "blocks3": (600, 300, 0)}
PAST_LIST_ROWS = (200, 64)     # the second run of past_list: dz live on [0, 200) / [0, 64) only, stamps present and ignored
PAST_LIST_LIVE = (200, 100)    # the first: dz non-zero on frames [0, 200) and [T - 100, T) of each utterance

# the case in which each defect must leave the bounds (test_posconv_ref_cpu.py)
FWD_DEFECT_CASE = {
    "last_tap_dropped": ("k128", None),             # one tap of 128: ~0.07 in z against a bound of ~0.02
    "tail_stage_dropped": ("k126", None),           # taps 124, 125
    "window_one_frame_late": ("full4", None),       # left - 1 (even k: the off-by-one of the padding rule)
    "even_k_keeps_last_frame_drops_first": ("full4", None),
    "next_group_channels": ("tail3", None),
    "second_block_reads_first_window": ("k127", None),   # the one row of the second block
    "bias_after_gelu": ("tail3", None),
    "residual_missing": ("tail3", None),
    "limit_row_not_zeroed": ("k127", LIMITS["k127"]),
}
DW_DEFECT_CASE = {
    "frames_leak_across_utterances": ("many_utts", None),   # T = 1: taps 0 and 2 are exactly zero unless a neighbour leaks in
    "last_k_block_dropped": ("nkb2", None),
    "blocks_past_1024_dropped": ("past_list", None),
    "tap_block_offset_ignored": ("nkb5", None),
    "lp_is_k_half": ("nkb2", None),
    "db_rows_32_63_dropped": ("nkb2", None),
    "db_from_every_tap_block": ("nkb5", None),
}


def geometry(B, T, G, k):
    """The launch geometry of posconv.hip for a shape, from the constants above."""
    Tp = T + k - 1 + (1 if k % 2 == 0 else 0)
    padl = k // 2
    Kr = B * Tp - (k - 1)
    nblk = (T + FBM - 1) // FBM
    fwd_items, dw_items = G * B * nblk, G * ((k + DTJ - 1) // DTJ)
    return dict(Tp=Tp, padl=padl, lp=k - 1 - padl, Kr=Kr, nkb=(Kr + 63) // 64, ntb=(k + DTJ - 1) // DTJ, nblk=nblk,
                nst=(k + TAPS - 1) // TAPS, tail=k % TAPS, fwd_items=fwd_items, fwd_n8=fwd_items // 8, fwd_r8=fwd_items % 8,
                dw_items=dw_items, dw_n8=dw_items // 8, dw_r8=dw_items % 8, magic=((1 << 32) // Tp) & 0xFFFFFFFF)


def k_block_stamps(B, T, k, rows):
    """The K-block stamps functional.posconv_k_block_stamps builds from grad_rows (1 = live), restated: block kb covers rows [64 kb, 64 kb + 64) of
    the axis kappa = b Tp + t; it is live if it starts inside utterance b's live frames or runs into a live utterance b + 1."""
    g = geometry(B, T, 1, k)
    out = []
    for kb in range(g["nkb"]):
        b0, t0 = divmod(kb * 64, g["Tp"])
        out.append(int(t0 < rows[b0] or (t0 + 64 > g["Tp"] and b0 + 1 < B and rows[b0 + 1] > 0)))
    return torch.tensor(out, dtype=torch.int32)


def _edges(v, live):
    """Scale the first and the last min(L, 4) live frames of every utterance by 4 and zero the frames from the limit on."""
    B, T, _ = v.shape
    t = torch.arange(T)[None, :, None]
    L = torch.tensor(live).view(B, 1, 1)
    edge = (t < 4) | (t >= L - 4)
    return torch.where(t < L, torch.where(edge, 4.0 * v, v), torch.zeros_like(v))


@functools.lru_cache(maxsize=None)
def case(name, lens=None):
    """-> dict(x, w, bias, dy, dz [bf16, CPU], B, T, G, k, C, lens).  dz is a stand-in of the size of dy for the tests that call the
    gradient kernels directly; through the function the device's own dz is used."""
    B, T, G, k = CASES[name]
    C = CG * G
    gen = torch.Generator(device="cpu")
    gen.manual_seed(zlib.crc32(name.encode()))
    live = tuple(lens) if lens is not None else (T,) * B
    x = _edges(0.5 * torch.randn(B, T, C, generator=gen), live)
    w = (0.2 if k <= 16 else 0.02) * torch.randn(C, CG, k, generator=gen)
    bias = 0.1 * torch.randn(C, generator=gen)
    dy = _edges(torch.randn(B, T, C, generator=gen), live)
    dz = _edges(torch.randn(B, T, C, generator=gen), live)
    if name == "past_list" and lens is None:
        t = torch.arange(T)[None, :, None]
        keep = (t < PAST_LIST_LIVE[0]) | (t >= T - PAST_LIST_LIVE[1])
        dz, dy = dz * keep, dy * keep
    out = dict(x=x.to(BF), w=w.to(BF), bias=bias.to(BF), dy=dy.to(BF), dz=dz.to(BF), B=B, T=T, G=G, k=k, C=C, lens=lens)
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# windows and per-group products, shared by the fp64 restatements and the emulations
# ------------------------------------------------------------------------------------------------------------------------------------
def _windows(v, k, left):
    """v [B, T, C] -> a view [B, T, k, C]: entry (b, m, j) is frame m - left + j of utterance b, zero outside [0, T)."""
    B, T, C = v.shape
    p = torch.zeros(B, T + 2 * k, C, dtype=v.dtype)
    p[:, k:k + T] = v
    return p.unfold(1, k, 1)[:, k - left:k - left + T].permute(0, 1, 3, 2)


def _w_fwd(w, groups):
    """[C, C/G, k] -> [G, k cg, cg]: row j cg + ci, column co = w[g co, ci, j]."""
    k = w.shape[2]
    return w.view(groups, CG, CG, k).permute(0, 3, 2, 1).reshape(groups, k * CG, CG)


def _w_dx(w, groups):
    """[C, C/G, k] -> [G, k cg, cg]: row j' cg + co, column ci = w[g co, ci, k - 1 - j']."""
    k = w.shape[2]
    jr = torch.arange(k - 1, -1, -1)
    return w.view(groups, CG, CG, k)[:, :, :, jr].permute(0, 3, 1, 2).reshape(groups, k * CG, CG)


def _win_sums(v, Wm, groups, k, left):
    """Window sums [B, T, C] of v against Wm in fp64, the sums of the absolute products, and the number of nonzero products."""
    B, T, C = v.shape
    v = v.double()
    Wm = Wm.double()
    outs = []
    for a, m in ((v, Wm), (v.abs(), Wm.abs()), ((v != 0).double(), (Wm != 0).double())):
        win = _windows(a, k, left)
        o = torch.empty(B * T, C, dtype=torch.float64)
        for g in range(groups):
            o[:, g * CG:(g + 1) * CG] = win[..., g * CG:(g + 1) * CG].reshape(B * T, k * CG) @ m[g]
        outs.append(o.view(B, T, C))
    return outs


def _check_limit(v, lens):
    if lens is not None:
        for b, n in enumerate(lens):
            assert not bool(v[b, int(n):].any()), "frames from the limit on must be zero (the caller's guarantee)"


# ------------------------------------------------------------------------------------------------------------------------------------
# fp64 restatements and bounds
# ------------------------------------------------------------------------------------------------------------------------------------
def _fwd_all(x, w, bias, groups, lens=None):
    _check_limit(x, lens)
    k = w.shape[2]
    acc, S, n = _win_sums(x, _w_fwd(w, groups), groups, k, k // 2)
    z = acc + (bias.double()[None, None] if bias is not None else 0.0)
    return z, x.double() + gelu64(z), S, n


def fwd64(x, w, bias, groups, lens=None):
    """-> z, y in fp64.  lens: frames of x from lens[b] on are zero (checked); the values do not depend on it."""
    return _fwd_all(x, w, bias, groups, lens)[:2]


def _acc_bound(S, n):
    return SLACK * (n - 1.0).clamp_min(0.0) * U32 * S


def _gelu_bound(z, b_z):
    """gelu_t<bf16>(z') against GELU(z), |z' - z| <= b_z, BEFORE any store: the first line of norm_ref._gelu_out_bound."""
    return (dgelu64(z).abs() + 0.8 * b_z) * b_z + a_gelu(z, BF)


def fwd_bounds(x, w, bias, groups):
    z, y, S, n = _fwd_all(x, w, bias, groups)
    b_acc = _acc_bound(S, n)
    b_v = b_acc * (1.0 + U32) + U32 * z.abs() + ETA if bias is not None else b_acc
    b_y = _gelu_bound(z, b_v) * (1.0 + U32) + U32 * y.abs() + ETA
    return dict(z=_store(b_v, z, BF), y=_store(b_y, y, BF))


def _dx_all(dz, w, dy, groups):
    k = w.shape[2]
    acc, S, n = _win_sums(dz, _w_dx(w, groups), groups, k, k - 1 - k // 2)
    return dy.double() + acc, S, n


def dx64(dz, w, dy, groups):
    return _dx_all(dz, w, dy, groups)[0]


def dx_bounds(dz, w, dy, groups):
    dx, S, n = _dx_all(dz, w, dy, groups)
    return dict(dx=_store(_acc_bound(S, n) * (1.0 + U32) + U32 * dx.abs() + ETA, dx, BF))


def _dw_all(dz, x, groups, k):
    """dw [C, cg, k], its absolute sums and counts, db.  Frames whose dz is entirely zero add nothing and are left out."""
    B, T, C = dz.shape
    bi, ti = torch.nonzero((dz != 0).any(2), as_tuple=True)
    d = dz[bi, ti].double()                                       # [R, C]
    outs = []
    for a, m in ((d, x.double()), (d.abs(), x.double().abs()), ((d != 0).double(), (x != 0).double())):
        win = _windows(m, k, k // 2)[bi, ti]                      # [R, k, C]: frames t - padl + j
        o = torch.empty(C, CG, k, dtype=torch.float64)
        for g in range(groups):
            s = slice(g * CG, (g + 1) * CG)
            o[s] = (a[:, s].t() @ win[:, :, s].reshape(-1, k * CG)).view(CG, k, CG).permute(0, 2, 1)
        outs.append(o)
    return outs[0], outs[1], outs[2], dz.double().sum((0, 1))


def dw64(dz, x, groups, k):
    """-> dw [C, C/G, k], db [C]: sums over every frame of every utterance; no frame of utterance b meets a frame of b + 1."""
    r = _dw_all(dz, x, groups, k)
    return r[0], r[3]


def db_chain(nkb):
    return 2 * nkb - 1 + 31


def dw_bounds(dz, x, groups, k):
    B, T, C = dz.shape
    dw, S, n, db = _dw_all(dz, x, groups, k)
    t = dz.double().abs().reshape(B * T, C)
    t = t[(t != 0).any(1)]
    b_db = _colsum_bound(t, torch.zeros_like(t), db_chain(geometry(B, T, groups, k)["nkb"])) if t.numel() else torch.zeros(C, dtype=torch.float64)
    return dict(dw=_store(_acc_bound(S, n), dw, BF), db=_store(b_db, db, BF))


# ------------------------------------------------------------------------------------------------------------------------------------
# fp32 emulations
# ------------------------------------------------------------------------------------------------------------------------------------
SHAPES = ("seq", "chunk16")


def _chain32(At, W, shape, chunks=None):
    """fp32 accumulators [R, N] of sum_kk At[kk, :, None] W[kk, None, :] over the K axis in order.  At [K, R], W [K, N] fp32 holding bf16
    values (every product is exact in fp32).  chunks (chunk16): the chunk index of every K row, ascending; default kk // 16."""
    K, R = At.shape
    acc = torch.zeros(R, W.shape[1], dtype=torch.float32)
    if shape == "seq":
        for kk in range(K):
            acc.addcmul_(At[kk][:, None], W[kk][None])            # (exact product, one rounding of the sum)
        return acc
    assert shape == "chunk16"
    if chunks is None:
        bounds = list(range(0, K, 16)) + [K]
    else:
        ch = chunks.tolist()
        bounds = [0] + [i for i in range(1, K) if ch[i] != ch[i - 1]] + [K]
    for a, b in zip(bounds[:-1], bounds[1:]):
        if b > a:
            acc = (acc.double() + At[a:b].double().t() @ W[a:b].double()).float()
    return acc


def _win_acc32(v, Wm, groups, k, left, shape, defect, m_len):
    """The fp32 accumulators [B, T, C] of posconv_win_kernel: per (group, utterance, block of 256 frames) the window sum in K order
    tap-major / channel-minor; a block with m0 >= m_len[b] keeps zero accumulators."""
    B, T, C = v.shape
    if defect == "window_one_frame_late":
        left -= 1
    Wm = Wm.float().clone()
    if defect == "last_tap_dropped":
        Wm[:, (k - 1) * CG:] = 0.0
    if defect == "tail_stage_dropped":
        Wm[:, TAPS * (k // TAPS) * CG:] = 0.0
    win = _windows(v.float(), k, left)
    m = torch.arange(T)
    dead = torch.zeros(B, T, dtype=torch.bool)
    if m_len is not None:
        dead = (m // FBM * FBM)[None] >= torch.tensor(m_len).view(B, 1)
    acc = torch.empty(B, T, C, dtype=torch.float32)
    for g in range(groups):
        gs = (g + 1) % groups if defect == "next_group_channels" else g
        A = win[..., gs * CG:(gs + 1) * CG].reshape(B, T, k * CG)
        if defect == "second_block_reads_first_window":
            A = A[:, m % FBM]                                     # m0 ignored: row m of block > 0 reads the window of row m - m0
        if defect == "limit_row_not_zeroed":
            A = torch.where(dead[..., None], A[0, m % FBM][None], A)   # a dead block runs its K loop over what LDS held: utterance 0's first block
        else:
            A = A * (~dead)[..., None]
        acc[..., g * CG:(g + 1) * CG] = _chain32(A.reshape(B * T, k * CG).t().contiguous(), Wm[g], shape).view(B, T, CG)
    return acc


def _m_len(lens, T, left):
    return None if lens is None else [min(int(n) + left, T) for n in lens]


def fwd_emulate32(x, w, bias, groups, lens=None, shape="seq", defect=None):
    """-> z, y (bf16) as cst_posconv_fwd forms them."""
    assert defect is None or defect in FWD_DEFECTS
    k, T = w.shape[2], x.shape[1]
    left = k // 2
    if defect == "even_k_keeps_last_frame_drops_first":
        assert k % 2 == 0
        left -= 1                                                 # outputs 1 .. T of the T + 1 that the padding gives
    acc = _win_acc32(x, _w_fwd(w, groups), groups, k, left, shape, defect, _m_len(lens, T, k // 2))
    b = bias.float()[None, None] if bias is not None else None
    v = acc + b if b is not None else acc
    if defect == "bias_after_gelu":
        y = gelu32(acc, BF) + b
    else:
        y = gelu32(v, BF)
    if defect != "residual_missing":
        y = y + x.float()
    return v.to(BF), y.to(BF)


def dx_emulate32(dz, w, dy, groups, rows=None, shape="seq", defect=None):
    """-> dx (bf16) as cst_posconv_dx forms it from the flipped weight; rows = grad_rows."""
    assert defect is None or defect in DX_DEFECTS
    k, T = w.shape[2], dz.shape[1]
    left = k - 1 - k // 2
    if defect == "even_k_keeps_last_frame_drops_first":
        assert k % 2 == 0
        left += 1                                                 # the transpose of the forward that drops the first frame
    acc = _win_acc32(dz, _w_dx(w, groups), groups, k, left, shape, defect, _m_len(rows, T, k - 1 - k // 2))
    if defect != "residual_missing":
        acc = acc + dy.float()
    return acc.to(BF)


def dw_emulate32(dz, x, groups, k, shape="seq", defect=None):
    """-> dw [C, C/G, k], db [C] (bf16) as posconv_dw_kernel forms them: rows kappa = b Tp + p of the zero-padded frame axis in ascending
    order (x at p = padl + t, dz at p = lp + t, so that accumulator row kappa pairs dz row kappa + lp with x rows kappa + j)."""
    assert defect is None or defect in DW_DEFECTS
    B, T, C = dz.shape
    geo = geometry(B, T, groups, k)
    padl, lp, nkb, ntb = geo["padl"], geo["lp"], geo["nkb"], geo["ntb"]
    tail = torch.zeros(64 + 2 * k, C, dtype=torch.float32)
    if defect == "frames_leak_across_utterances":                 # B T contiguous frames, no zero rows between the utterances
        xa = torch.cat([torch.zeros(padl, C), x.float().reshape(B * T, C)])
        da = torch.cat([torch.zeros(lp, C), dz.float().reshape(B * T, C)])
        nkb = (B * T + 63) // 64
    else:
        xa = torch.zeros(B, geo["Tp"], C, dtype=torch.float32)
        da = torch.zeros(B, geo["Tp"], C, dtype=torch.float32)
        xa[:, padl:padl + T] = x.float()
        da[:, lp:lp + T] = dz.float()
        xa, da = xa.view(-1, C), da.view(-1, C)
    fill = torch.zeros(max(0, nkb * 64 + lp + 1 - da.shape[0]), C)
    xa, da = torch.cat([xa, fill, tail]), torch.cat([da, fill, tail])
    if defect == "lp_is_k_half":
        assert k % 2 == 0
        lp += 1
    img = da[lp:lp + nkb * 64]                                    # accumulator row kappa reads dz image row kappa
    if defect == "last_k_block_dropped":
        img = img[:(nkb - 1) * 64]
    if defect == "blocks_past_1024_dropped":
        img = img[:DKLIST * 64]
    rows = torch.nonzero((img != 0).any(1)).reshape(-1)
    dw = torch.zeros(C, CG, k, dtype=torch.float32)
    for g in range(groups):
        s = slice(g * CG, (g + 1) * CG)
        W = xa[:, s].unfold(0, k, 1)[rows].permute(0, 2, 1).reshape(-1, k * CG)   # [R, j cg + ci] = x row kappa + j
        acc = _chain32(img[rows][:, s].contiguous(), W, shape, chunks=rows // 16)
        dw[s] = acc.view(CG, k, CG).permute(0, 2, 1)
    if defect == "tap_block_offset_ignored":
        dw = dw[:, :, torch.arange(k) % DTJ]                      # tap block tb > 0 reads the windows of taps 0 .. 7
    # db: 32 partials per column, partial r adds rows r and 32 + r of every K block in block order; then the partials in row order
    blocks = img.view(-1, 2, 32, C)
    cs = torch.zeros(32, C, dtype=torch.float32)
    for kb in torch.nonzero((blocks != 0).flatten(1).any(1)).reshape(-1).tolist():
        cs = cs + blocks[kb, 0]
        if defect != "db_rows_32_63_dropped":
            cs = cs + blocks[kb, 1]
    db = torch.zeros(C, dtype=torch.float32)
    for r in range(32):
        db = db + cs[r]
    if defect == "db_from_every_tap_block":
        db = db * float(ntb)
    return dw.to(BF), db.to(BF)
