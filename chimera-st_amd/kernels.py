"""Raw (non-autograd) wrappers: torch tensors in, C-ABI calls out.  Torch only supplies device
memory and the current HIP stream here; every arithmetic op is a kernel of libcst_hip.so."""
import ctypes
import os

import torch

from . import lib as L

_ws = {}
STATS = {}  # light counters for tests / tools (e.g. how many GEMM launches carried live-tile stamps)


def workspace(nbytes: int, device) -> torch.Tensor:
    """Grow-only scratch buffer, stream-ordered reuse (all product kernels run on the current stream)."""
    key = (device.index, L.stream_ptr().value)  # (the raw-stream getter: torch.cuda.current_stream() costs ~20 us of Python per call)
    t = _ws.get(key)
    if t is None or t.numel() < nbytes:
        t = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _ws[key] = t
    return t


class _Deferred:
    """Second stages of fixed-order reductions (split-K slabs of the small weight-gradient GEMMs, bias-gradient slices, LayerNorm
    dgamma / dbeta partials) that are finished together by ONE cst_reduce_multi launch instead of a launch each.  The results
    are gradients of parameters: nothing reads them before the update gathers them, PROVIDED no second gradient of the same
    parameter arrives in the same backward pass (autograd would add the two at once) — so the mode is switched on only by a trainer
    whose criterion runs one pass over a model that uses each parameter once (trainer.py), parameters shared between modules are
    excluded at the call sites, and a gradient that is being accumulated into (p.grad is not None) takes the immediate route.
    CST_DEFER_POISON=1 (the test suite sets it) fills every deferred destination with NaN until the flush writes it: a read that
    comes too early cannot go unnoticed."""

    MAX_BYTES = 32 << 20  # slabs above this stay with their own reduce launch (they would have to be re-read cold from HBM)

    def __init__(self):
        self.on, self.items, self.keep, self.flushes = 0, [], [], 0
        self.main = None   # the stream the flush runs on (set when the mode is entered)
        self.side = None   # side stream of the small weight-gradient GEMMs (side_gemm), created on first use
        self.side_used = False
        self.poison = False

    def push(self, src_ptr, dst, stride, Lr, P, keep, order=0):
        if self.poison:
            dst.fill_(float("nan"))
        # (side-stream launches only — torch.cuda.current_stream() costs ~20 us of Python, 320 pushes per update: never in the default path)
        if self.side_used and torch.is_tensor(keep) and torch.cuda.current_stream() != self.main:
            keep.record_stream(self.main)  # allocated on the side stream's pool, read by the flush on the main stream
        self.items.append((src_ptr, dst.data_ptr(), stride, Lr, P, L.dtype_code(dst.dtype), order))
        # (an ALIAS of dst keeps its storage alive: holding dst itself would raise its reference count, and AccumulateGrad only adopts
        #  a gradient tensor nobody else holds — otherwise it clones it on the spot, i.e. reads it before the flush has written it)
        self.keep.append((keep, dst.detach()))

    def join(self):
        """The main stream waits for everything the side stream has been given (before anything reads a gradient)."""
        if self.side_used:
            torch.cuda.current_stream().wait_stream(self.side)
            self.side_used = False

    def flush(self):
        self.join()
        if self.items:
            reduce_multi(self.items)
            self.flushes += 1
            self.items, self.keep = [], []


DEFER = _Deferred()


def reduce_multi(items):
    """items: [(src_ptr, dst_ptr, stride, L, P, dst_dtype_code, order)] -> dst[i] = sum_p src[p * stride + i]: ONE launch (include/cst.h:
    order 0 = the split-K reduce's summation order, 1 = the LayerNorm second stage's)."""
    lib = L.load()
    for at in range(0, len(items), 64):
        chunk = items[at:at + 64]
        arr = (L.ReduceItem * len(chunk))()
        for a, (src, dst, stride, Lr, P, dt, order) in zip(arr, chunk):
            a.src, a.dst, a.stride, a.L, a.P, a.dst_dtype, a.order = src, dst, stride, Lr, P, dt, order
        L.check(lib.cst_reduce_multi(arr, len(chunk), L.stream_ptr()), "cst_reduce_multi")


class deferred_reductions:
    """with deferred_reductions(enabled): loss.backward()  — the flush runs on exit (and before any bucket all-reduce: distributed.py)."""

    def __init__(self, enabled=True):
        self.enabled = bool(enabled) and not os.environ.get("CST_NO_DEFER")

    def __enter__(self):
        if self.enabled:
            DEFER.on += 1
            DEFER.main = torch.cuda.current_stream()
            DEFER.poison = bool(os.environ.get("CST_DEFER_POISON"))
        return self

    def __exit__(self, *exc):
        if self.enabled:
            DEFER.on -= 1
            if DEFER.on == 0:
                DEFER.flush()
        return False


def side_gemm(big, reads, *args, **kw):
    """A weight-gradient GEMM of a SMALL layer (`big` False: the 4-wave configurations, a few hundred workgroups that leave most
    of every CU free) on a side stream, next to the dX chain of the backward pass it belongs to: the backward of the 512-wide
    encoder / decoder layers is a chain of 10-50 us kernels none of which fills the chip, and the weight gradients are off its
    critical path — nothing reads them before the update gathers them.  Only inside the trainer's backward context (DEFER.on: the
    same guarantee — the result is a parameter gradient nobody reads yet), joined before the deferred reductions are flushed.
    `reads`: the tensors the launch reads; they are handed to the side stream's allocator bookkeeping (record_stream) because
    autograd frees them as soon as the backward function returns."""
    # (measured on MI355X, same box, two runs each: 64.7 / 65.2 ms per update with the side stream, 64.9 / 65.0 without — the dX
    #  chain's own launches already take every CU's LDS, the side launches only slip into their tails.  Kept as a switch, off.)
    if big or not DEFER.on or DEFER.main is None or not os.environ.get("CST_SIDE_STREAM") or torch.cuda.current_stream() != DEFER.main:
        return gemm(*args, **kw)
    if DEFER.side is None:
        DEFER.side = torch.cuda.Stream()
    side = DEFER.side
    side.wait_stream(DEFER.main)  # the operands are the latest things queued on the main stream
    DEFER.side_used = True        # (before the launch: the pushes inside gemm() look at it)
    with torch.cuda.stream(side):
        out = gemm(*args, **kw)
    for t in reads:
        if t is not None:
            t.record_stream(side)
    STATS["side_gemm"] = STATS.get("side_gemm", 0) + 1
    return out


def _2d(t):
    assert t.dim() == 2 and t.stride(1) == 1, "expected a row-major 2-D tensor, got %s / %s" % (tuple(t.shape), t.stride())
    return t


def _stamps(live, extent, stat):
    """(pointer, epoch) of the live-tile stamps `live` = (stamps, epoch) over `extent` rows in 64-row tiles; (NULL, 0) without stamps."""
    if live is None:
        return None, 0
    assert live[0].numel() * 64 >= extent and live[0].dtype == torch.int32
    STATS[stat] = STATS.get(stat, 0) + 1
    return live[0].data_ptr(), live[1]


def _per_batch(v, batch0, stat):
    """Pointer of an int32 vector with one entry per batch0 index, or NULL."""
    if v is None:
        return None
    assert v.dtype == torch.int32 and v.numel() == batch0 and v.is_contiguous()
    STATS[stat] = STATS.get(stat, 0) + 1
    return v.data_ptr()


# ------------------------------------------------------------------------------------------------
def gemm(A, B, C, M, N, K, *, a_kmajor, b_kmajor, lda, ldb, ldc, bias=None, bias_mode=L.BIAS_COL, act=L.ACT_NONE,
         aux_out=None, ld_aux_out=0, dact=L.ACT_NONE, aux_in=None, ld_aux_in=0, resid=None, ld_resid=0, alpha=1.0,
         batch0=1, batch1=1, sa=(0, 0), sb=(0, 0), sc=(0, 0), sbias=(0, 0), a_seg=0, a_seg_stride=0, b_seg=0,
         b_seg_stride=0, split_k=-1, a_off=0, b_off=0, c_off=0, drop_p=0.0, drop_key=0, k_live=None, m_live=None, k_len=None, m_len=None,
         ws=None, colsum=None, defer=False, reduce_to=None):
    """C = epilogue(alpha * Aop @ Bop); see include/cst.h.  colsum (mn-major A): [batch, M] tensor of A's dtype that receives the
    column sums of A over k — the bias gradient next to a weight-gradient GEMM (cst_gemm_desc.colsum).
    defer: the caller allows the split-K reduce of this launch (C and colsum are parameter gradients nobody reads yet) to be left to
    the deferred-reduction flush (DEFER); ignored when the mode is off, the launch does not split, or the slabs are large.
    reduce_to (batched launches into an fp32 C [batch, M, N] with sc = (M * N, 0)): the sum over the batch — and over the K slices
    — goes to `reduce_to` [M, N] through cst_reduce_multi instead of a torch sum over C (which is then never written when K is split).  Offsets *_off are in elements.  k_live = (stamps, epoch): the 64-wide
    K blocks of A that are not all-zero (LiveTiles.pair()); dead blocks may be skipped; m_live: the same stamps for the rows of A of a
    row-wise GEMM (dX): output tiles without a live row skip their K loop.  ws: the caller's own split-K scratch (uint8; launches
    captured into a graph must not depend on the shared grow-only buffer)."""
    lib = L.load()
    d = L.GemmDesc()
    d.dtype = L.dtype_code(A.dtype)
    assert B.dtype == A.dtype, "A/B dtype mismatch"
    d.c_dtype = L.dtype_code(C.dtype)
    d.a_kmajor, d.b_kmajor = int(a_kmajor), int(b_kmajor)
    d.M, d.N, d.K = M, N, K
    es = A.element_size()
    d.A = A.data_ptr() + a_off * es
    d.lda, d.a_seg, d.a_seg_stride = lda, a_seg, a_seg_stride
    d.B = B.data_ptr() + b_off * es
    d.ldb, d.b_seg, d.b_seg_stride = ldb, b_seg, b_seg_stride
    d.C = C.data_ptr() + c_off * C.element_size()
    d.ldc = ldc
    if bias is not None:
        assert bias.dtype == A.dtype
        d.bias, d.bias_mode = bias.data_ptr(), bias_mode
    else:
        d.bias, d.bias_mode = None, L.BIAS_NONE
    d.sbias0, d.sbias1 = sbias
    d.act = act
    d.aux_out = None if aux_out is None else aux_out.data_ptr() + c_off * es
    d.ld_aux_out = ld_aux_out
    d.dact = dact
    d.aux_in = None if aux_in is None else aux_in.data_ptr() + c_off * es
    d.ld_aux_in = ld_aux_in
    d.resid = None if resid is None else resid.data_ptr() + c_off * es
    d.ld_resid = ld_resid
    d.alpha = alpha
    d.drop_p, d.drop_key = float(drop_p), int(drop_key) & 0xFFFFFFFF
    d.batch0, d.batch1 = batch0, batch1
    d.sa0, d.sa1 = sa
    d.sb0, d.sb1 = sb
    d.sc0, d.sc1 = sc
    d.split_k = split_k
    d.k_live, d.k_epoch = _stamps(k_live, K, "gemm_k_live")
    d.m_live, d.m_epoch = _stamps(m_live, M, "gemm_m_live")
    d.k_len = _per_batch(k_len, batch0, "gemm_k_len")
    d.m_len = _per_batch(m_len, batch0, "gemm_m_len")
    if colsum is not None:
        assert not a_kmajor and colsum.dtype == A.dtype and colsum.is_contiguous() and colsum.numel() == M * batch0 * batch1
        d.colsum = colsum.data_ptr()
    else:
        d.colsum = None
    d.defer_reduce = 0
    splits = 1
    need = lib.cst_gemm_workspace(ctypes.byref(d))
    nb = batch0 * batch1
    deferred = False
    if need > 0 and (reduce_to is not None or (defer and DEFER.on and nb == 1 and need <= DEFER.MAX_BYTES and ldc == N and N % 8 == 0)):
        splits = lib.cst_gemm_splits(ctypes.byref(d))
        if splits > 1:
            assert ws is None and bias is None and act == L.ACT_NONE and dact == L.ACT_NONE and resid is None and aux_out is None and alpha == 1.0
            ws = torch.empty(need, dtype=torch.uint8, device=A.device)  # private: it must outlive this call (slabs read by the flush)
            d.defer_reduce = 1
            deferred = True
    if need > 0:
        if ws is None:
            ws = workspace(need, A.device)
        assert ws.dtype == torch.uint8 and ws.numel() >= need, "split-K scratch too small: %d < %d" % (ws.numel(), need)
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    else:
        d.workspace, d.workspace_bytes = None, 0
    L.check(lib.cst_gemm(ctypes.byref(d), L.stream_ptr()), "cst_gemm")
    if reduce_to is not None:
        assert C.dtype == torch.float32 and sc == (M * N, 0) and ldc == N and reduce_to.numel() == M * N and reduce_to.is_contiguous() and colsum is None
        item = ((ws.data_ptr(), reduce_to, M * N, M * N, nb * splits, ws) if deferred else (C.data_ptr(), reduce_to, M * N, M * N, nb, C))
        if defer and DEFER.on:
            DEFER.push(*item)
        else:
            reduce_multi([(item[0], item[1].data_ptr(), item[2], item[3], item[4], L.dtype_code(reduce_to.dtype), 0)])
    elif deferred:
        DEFER.push(ws.data_ptr(), C, M * N, M * N, splits, ws)
        if colsum is not None:
            DEFER.push(ws.data_ptr() + 4 * splits * M * N, colsum, M, M, splits, ws)
    return C


_DW_FUSED = {}


def dw_colsum_is_fused(n_out, k_in, tokens, dtype):
    """Whether the weight-gradient GEMM dW[n_out, k_in] = dY^T X over `tokens` rows yields the bias gradient as a by-product of its
    own kernel (cst_gemm_colsum_is_fused) — the 4-wave configurations do, the 16-wave one runs a separate column sum."""
    key = (n_out, k_in, tokens, dtype)
    r = _DW_FUSED.get(key)
    if r is None:
        d = L.GemmDesc()
        d.dtype = d.c_dtype = L.dtype_code(dtype)
        d.a_kmajor = d.b_kmajor = 0
        d.M, d.N, d.K = n_out, k_in, tokens
        d.batch0 = d.batch1 = 1
        d.split_k = -1
        d.colsum = 1  # (any non-NULL value: the query reads no memory)
        r = _DW_FUSED[key] = bool(L.load().cst_gemm_colsum_is_fused(ctypes.byref(d)))
        if len(_DW_FUSED) > 4096:
            _DW_FUSED.clear()
    return r


def layernorm_fwd(x, res, gamma, beta, eps, want_sum=False):
    x = _2d(x)
    rows, cols = x.shape
    y = torch.empty_like(x)
    s = torch.empty_like(x) if (want_sum and res is not None) else None
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    L.check(L.load().cst_layernorm_fwd(L.ptr(x), L.ptr(res), L.ptr(gamma), L.ptr(beta), L.ptr(y), L.ptr(s), L.ptr(mean),
                                       L.ptr(rstd), rows, cols, eps, L.dtype_code(x.dtype), L.stream_ptr()), "cst_layernorm_fwd")
    return y, s, mean, rstd


_EPOCH = [0x3C6EF372]  # (not 0: the stamp buffers are never initialised, and recycled device memory is full of small integers — a dead
#                          tile whose stale word equals the epoch would be visited for nothing; harmless, but not what the stamps are for)


def next_epoch():
    """Unique non-zero 32-bit stamp per producer call (live-tile stamps are never initialised: a tile is live iff stamp == epoch)."""
    _EPOCH[0] = (_EPOCH[0] % 0xFFFFFFFE) + 1
    return _EPOCH[0]


def _two_stage(wbytes, outs, defer, launch):
    """A reduction whose kernel leaves fp32 partials [chunks][len(outs)][cols] in a scratch buffer and whose second stage sums them
    over the chunks into `outs` ([cols] each).  launch(ws, *output pointers) enqueues the kernel.  Normally the scratch is the shared
    workspace and the kernel runs the second stage itself; with `defer` inside the deferred mode the scratch is private (the flush
    reads it after this call has returned), the kernel gets NULL outputs and the second stage is handed to DEFER (order 1 of
    cst_reduce_multi = the summation order of these kernels' own second stages)."""
    deferred = bool(defer) and DEFER.on > 0
    dev = outs[0].device
    ws = torch.empty(wbytes, dtype=torch.uint8, device=dev) if deferred else workspace(wbytes, dev)
    launch(ws, *[None if deferred else L.ptr(o) for o in outs])
    if deferred:
        n, cols = len(outs), outs[0].numel()
        for i, o in enumerate(outs):
            DEFER.push(ws.data_ptr() + 4 * cols * i, o, n * cols, cols, wbytes // (4 * n * cols), ws, order=1)


def layernorm_bwd(dy, s, gamma, mean, rstd, dres=None, grad_dtype=torch.float32, want_tiles=False, defer=False):
    """dgamma / dbeta come back in `grad_dtype` (fp32, or the parameter dtype: accumulated in fp32, rounded once).
    want_tiles: also returns (stamps int32 [ceil(rows/64)], epoch) marking the 64-row tiles of dx that are not exactly zero.
    defer: the caller allows the second stage (row-block partials -> dgamma / dbeta) to be left to the deferred-reduction flush."""
    dy, s = _2d(dy), _2d(s)
    rows, cols = s.shape
    lib = L.load()
    dx = torch.empty_like(s)
    dg = torch.empty(cols, dtype=grad_dtype, device=s.device)
    db = torch.empty(cols, dtype=grad_dtype, device=s.device)
    stamps, epoch = (torch.empty((rows + 63) // 64, dtype=torch.int32, device=s.device), next_epoch()) if want_tiles else (None, 0)

    def launch(ws, pg, pb):
        if want_tiles:
            L.check(lib.cst_layernorm_bwd_tiles(L.ptr(dy), L.ptr(s), L.ptr(gamma), L.ptr(mean), L.ptr(rstd), L.ptr(dres), L.ptr(dx), pg,
                                                pb, L.ptr(ws), rows, cols, L.dtype_code(s.dtype), L.dtype_code(grad_dtype),
                                                L.ptr(stamps), epoch, L.stream_ptr()), "cst_layernorm_bwd_tiles")
        else:
            L.check(lib.cst_layernorm_bwd(L.ptr(dy), L.ptr(s), L.ptr(gamma), L.ptr(mean), L.ptr(rstd), L.ptr(dres), L.ptr(dx), pg,
                                          pb, L.ptr(ws), rows, cols, L.dtype_code(s.dtype), L.dtype_code(grad_dtype), L.stream_ptr()),
                    "cst_layernorm_bwd")

    _two_stage(lib.cst_layernorm_bwd_workspace(rows, cols), (dg, db), defer, launch)
    return (dx, dg, db, (stamps, epoch)) if want_tiles else (dx, dg, db)


def _bhtd_strides(t, layout):
    """Element strides (sb, sh, st) of a [B,T,H*D]-shaped ("bthd") or [T,B,H*D] ("tbhd") activation; d contiguous."""
    assert t.stride(-1) == 1
    if layout == "bt":  # tensor is [B, T, C]
        return t.stride(0), None, t.stride(1)
    return t.stride(1), None, t.stride(0)  # [T, B, C]


def attn_desc(q, k, v, o, lse, H, D, kpm, causal, scale, layout_q="bt", layout_kv="bt", drop_p=0.0, drop_key=0, kv_len=None, seq=None):
    """q,o: [B,Tq,H*D] (layout "bt") or [Tq,B,H*D] ("tb"); k,v likewise with Tk.  Head h at channel offset h*D.
    seq = (seq_offsets int32 [B+1], longest sequence): packed self-attention, q/k/v/o are [1, rows, H*D] (include/cst.h)."""
    d = L.AttnDesc()
    d.dtype = L.dtype_code(q.dtype)
    if layout_q == "bt":
        B, Tq = q.shape[0], q.shape[1]
    else:
        Tq, B = q.shape[0], q.shape[1]
    Tk = k.shape[1] if layout_kv == "bt" else k.shape[0]
    if seq is not None:
        assert layout_q == "bt" and layout_kv == "bt" and B == 1 and kpm is None
        assert seq[0].dtype == torch.int32 and seq[0].is_contiguous()
        B, Tq, Tk = seq[0].numel() - 1, int(seq[1]), int(seq[1])
        d.seq_offsets = seq[0].data_ptr()
        STATS["attn_packed"] = STATS.get("attn_packed", 0) + 1
    else:
        d.seq_offsets = None
    d.B, d.H, d.Tq, d.Tk, d.D = B, H, Tq, Tk, D

    def st(t, lay):
        sb, _, stt = _bhtd_strides(t, lay)
        return sb, D, stt

    d.Q = q.data_ptr(); d.q_sb, d.q_sh, d.q_st = st(q, layout_q)
    d.K = k.data_ptr(); d.k_sb, d.k_sh, d.k_st = st(k, layout_kv)
    d.V = v.data_ptr(); d.v_sb, d.v_sh, d.v_st = st(v, layout_kv)
    d.O = o.data_ptr(); d.o_sb, d.o_sh, d.o_st = st(o, layout_q)
    d.lse = lse.data_ptr()
    if kpm is not None:
        assert kpm.dtype == torch.uint8 and kpm.stride(1) == 1 and kpm.shape == (B, Tk)
        d.key_padding_mask, d.kpm_stride = kpm.data_ptr(), kpm.stride(0)
        bits = kpm_bits(kpm)
        d.kpm_bits = bits.data_ptr()
        d._kpm_bits_owner = bits
    else:
        d.key_padding_mask, d.kpm_stride = None, 0
        d.kpm_bits = None
    d.bwd_ws = None
    d.causal, d.scale = int(causal), scale
    if q.dtype == torch.bfloat16 and D == 64 and not causal and not os.environ.get("CST_ATTN_GENERIC"):
        STATS["attn_fast"] = STATS.get("attn_fast", 0) + 1  # (mirrors attn_fast_ok of csrc/attention.hip: the DMA-staged kernels)
    d.drop_p, d.drop_key = float(drop_p), int(drop_key) & 0xFFFFFFFF
    if kv_len is not None:
        assert (kpm is not None or seq is not None) and kv_len.dtype == torch.int32 and kv_len.numel() == B and kv_len.is_contiguous()
        d.kv_len = kv_len.data_ptr()
        STATS["attn_kv_len"] = STATS.get("attn_kv_len", 0) + 1
    else:
        d.kv_len = None
    return d


_KPM_BITS = []  # [(data_ptr, shape, version, uint8 mask (kept alive), int64 words)]: one padding mask serves every layer of a pass
_BIT_WEIGHTS = {}  # device -> int64 [64]: 1 << k (built on the device: a host list would be a pageable copy, i.e. a stream sync)


def kpm_bits(kpm):
    """uint8 [B, Tk] key padding mask -> int64 [B, ceil(Tk/64)]: bit k of word j = key 64 j + k is masked (bits of keys >= Tk set).
    cst_attn_desc.kpm_bits: the DMA-staged attention kernels read one mask word per key tile from scalar registers.
    Nothing here touches the host: the backward pass asks again with the tensor autograd saved (another Python object over the same
    storage), so the cache goes by storage address + shape + version."""
    key = (kpm.data_ptr(), tuple(kpm.shape), kpm._version)
    for ptr, shape, ver, _, bits in _KPM_BITS:
        if (ptr, shape, ver) == key:
            return bits
    B, Tk = kpm.shape
    nw = (Tk + 63) // 64
    m = kpm != 0
    if nw * 64 != Tk:
        m = torch.cat([m, torch.ones(B, nw * 64 - Tk, dtype=torch.bool, device=kpm.device)], 1)
    w = _BIT_WEIGHTS.get(kpm.device)
    if w is None:
        w = _BIT_WEIGHTS[kpm.device] = torch.ones(64, dtype=torch.int64, device=kpm.device) << torch.arange(64, dtype=torch.int64, device=kpm.device)
    bits = (m.view(B, nw, 64).to(torch.int64) * w).sum(-1).contiguous()  # distinct powers of two: the wrapping sum is the OR
    _KPM_BITS.append(key + (kpm, bits))
    if len(_KPM_BITS) > 8:
        _KPM_BITS.pop(0)
    return bits


def attn_fwd(q, k, v, H, D, kpm, causal, scale, layout_q="bt", layout_kv="bt", drop_p=0.0, drop_key=0, kv_len=None):
    o = torch.empty_like(q)
    if layout_q == "bt":
        B, Tq = q.shape[0], q.shape[1]
    else:
        Tq, B = q.shape[0], q.shape[1]
    lse = torch.empty(B, H, Tq, dtype=torch.float32, device=q.device)
    d = attn_desc(q, k, v, o, lse, H, D, kpm, causal, scale, layout_q, layout_kv, drop_p, drop_key, kv_len)
    L.check(L.load().cst_attn_fwd(ctypes.byref(d), L.stream_ptr()), "cst_attn_fwd")
    return o, lse


def attn_fwd_desc(d):
    L.check(L.load().cst_attn_fwd(ctypes.byref(d), L.stream_ptr()), "cst_attn_fwd")


def attn_bwd_desc(d):
    L.check(L.load().cst_attn_bwd(ctypes.byref(d), L.stream_ptr()), "cst_attn_bwd")


def attn_bwd_fill(d, do, dq, dk, dv, delta, D, layout_q="bt", layout_kv="bt"):
    """Fill the backward half of an attention descriptor (gradient tensors may be strided views, d contiguous)."""
    def st(t, lay):
        sb, _, stt = _bhtd_strides(t, lay)
        return sb, D, stt

    d.dO = do.data_ptr(); d.do_sb, d.do_sh, d.do_st = st(do, layout_q)
    d.dQ = dq.data_ptr(); d.dq_sb, d.dq_sh, d.dq_st = st(dq, layout_q)
    d.dK = dk.data_ptr(); d.dk_sb, d.dk_sh, d.dk_st = st(dk, layout_kv)
    d.dV = dv.data_ptr(); d.dv_sb, d.dv_sh, d.dv_st = st(dv, layout_kv)
    d.delta = delta.data_ptr()
    # live-tile flags (cst_attn_desc.q_flags): the backward stops at the last 64-query tile with a non-zero upstream gradient
    flags = torch.empty(int(d.B) * int(d.H) * ((int(d.Tq) + 63) // 64), dtype=torch.uint8, device=do.device)  # d.B / d.Tq: sequences / longest one when packed
    d.q_flags = flags.data_ptr()
    STATS["attn_q_flags"] = STATS.get("attn_q_flags", 0) + 1
    d._q_flags_owner = flags  # the workspace lives as long as the descriptor (i.e. until the launch has been enqueued)
    # statistics workspace of the DMA-staged backward kernels (cst_attn_desc.bwd_ws)
    ws = torch.empty(int(L.load().cst_attn_bwd_workspace(ctypes.byref(d))) // 4, dtype=torch.float32, device=do.device)
    d.bwd_ws = ws.data_ptr()
    d._bwd_ws_owner = ws


def attn_bwd(do, q, k, v, o, lse, H, D, kpm, causal, scale, layout_q="bt", layout_kv="bt", drop_p=0.0, drop_key=0, kv_len=None, seq=None,
             grads=None):
    """grads = (dq, dk, dv): where the gradients go (channel slices of one packed buffer); fresh tensors like q, k, v when None."""
    dq, dk, dv = grads if grads is not None else (torch.empty_like(q), torch.empty_like(k), torch.empty_like(v))
    delta = torch.empty_like(lse)
    d = attn_desc(q, k, v, o, lse, H, D, kpm, causal, scale, layout_q, layout_kv, drop_p, drop_key, kv_len, seq)
    attn_bwd_fill(d, do, dq, dk, dv, delta, D, layout_q, layout_kv)
    attn_bwd_desc(d)
    return dq, dk, dv


def conv0_fwd(wav, w, gamma, beta, k, stride, eps=1e-5, frame_limit=None):
    """wav [B,S] fp32; w [C,k]; -> y [B,L,C] channels-last, (mean, rstd, gram) saved for backward.  frame_limit (int32 [B]): frames
    from there on are unread and left unwritten (include/cst.h)."""
    assert wav.dtype == torch.float32 and wav.is_contiguous()
    B, S = wav.shape
    C = w.shape[0]
    Lo = (S - k) // stride + 1
    y = torch.empty(B, Lo, C, dtype=w.dtype, device=wav.device)
    mean = torch.empty(B, C, dtype=torch.float32, device=wav.device)
    rstd = torch.empty(B, C, dtype=torch.float32, device=wav.device)
    gram = torch.empty(B, k * k + k, dtype=torch.float32, device=wav.device)
    lib = L.load()
    ws = workspace(lib.cst_conv0_fwd_workspace(B, S, k, stride), wav.device)
    L.check(lib.cst_conv0_gn_gelu_fwd(L.ptr(wav), L.ptr(w), L.ptr(gamma), L.ptr(beta), L.ptr(y), L.ptr(mean), L.ptr(rstd),
                                      L.ptr(gram), L.ptr(ws), _lim(frame_limit, B), B, S, C, k, stride, eps, L.dtype_code(w.dtype),
                                      L.stream_ptr()), "cst_conv0_gn_gelu_fwd")
    return y, mean, rstd, gram


def _lim(frame_limit, B):
    if frame_limit is None:
        return None
    assert frame_limit.dtype == torch.int32 and frame_limit.numel() == B and frame_limit.is_contiguous()
    STATS["conv0_frame_limit"] = STATS.get("conv0_frame_limit", 0) + 1
    return L.ptr(frame_limit)


def conv0_bwd(dy, wav, w, gamma, beta, mean, rstd, gram, k, stride, frame_limit=None):
    B, S = wav.shape
    C = w.shape[0]
    lib = L.load()
    dw = torch.empty(C, k, dtype=torch.float32, device=wav.device)
    dg = torch.empty(C, dtype=torch.float32, device=wav.device)
    db = torch.empty(C, dtype=torch.float32, device=wav.device)
    ws = workspace(lib.cst_conv0_bwd_workspace(B, S, C, k, stride), wav.device)
    L.check(lib.cst_conv0_gn_gelu_bwd(L.ptr(dy), L.ptr(wav), L.ptr(w), L.ptr(gamma), L.ptr(beta), L.ptr(mean), L.ptr(rstd),
                                      L.ptr(gram), L.ptr(dw), L.ptr(dg), L.ptr(db), L.ptr(ws), _lim(frame_limit, B), B, S, C, k, stride,
                                      L.dtype_code(w.dtype), L.stream_ptr()), "cst_conv0_gn_gelu_bwd")
    return dw, dg, db


def conv0_ln_fwd(wav, w, bias, gamma, beta, k, stride, eps=1e-5, frame_limit=None):
    """Layer 0 of the layer-norm feature extractor.  wav [B,S] fp32; w [C,k]; bias, gamma, beta [C] -> y [B,L,C] channels-last and the
    per-frame (mean, rstd) [B,L].  frame_limit (int32 [B]): frames from there on are unread and left unwritten (include/cst.h)."""
    assert wav.dtype == torch.float32 and wav.is_contiguous()
    B, S = wav.shape
    C = w.shape[0]
    Lo = (S - k) // stride + 1
    y = torch.empty(B, Lo, C, dtype=w.dtype, device=wav.device)
    mean = torch.empty(B, Lo, dtype=torch.float32, device=wav.device)
    rstd = torch.empty(B, Lo, dtype=torch.float32, device=wav.device)
    L.check(L.load().cst_conv0_ln_gelu_fwd(L.ptr(wav), L.ptr(w), L.ptr(bias), L.ptr(gamma), L.ptr(beta), L.ptr(y), L.ptr(mean),
                                           L.ptr(rstd), _lim(frame_limit, B), B, S, C, k, stride, eps, L.dtype_code(w.dtype),
                                           L.stream_ptr()), "cst_conv0_ln_gelu_fwd")
    return y, mean, rstd


def conv0_ln_bwd(dy, wav, w, bias, gamma, beta, mean, rstd, k, stride, frame_limit=None):
    """-> (dw [C,k], dbias, dgamma, dbeta [C]) fp32."""
    B, S = wav.shape
    C = w.shape[0]
    lib = L.load()
    dw = torch.empty(C, k, dtype=torch.float32, device=wav.device)
    dbi, dg, db = (torch.empty(C, dtype=torch.float32, device=wav.device) for _ in range(3))
    ws = workspace(lib.cst_conv0_ln_bwd_workspace(B, S, C, k, stride), wav.device)
    L.check(lib.cst_conv0_ln_gelu_bwd(L.ptr(dy), L.ptr(wav), L.ptr(w), L.ptr(bias), L.ptr(gamma), L.ptr(beta), L.ptr(mean),
                                      L.ptr(rstd), L.ptr(dw), L.ptr(dbi), L.ptr(dg), L.ptr(db), L.ptr(ws), _lim(frame_limit, B), B, S,
                                      C, k, stride, L.dtype_code(w.dtype), L.stream_ptr()), "cst_conv0_ln_gelu_bwd")
    return dw, dbi, dg, db


def _row_lim(row_limit, B):
    if row_limit is None:
        return None
    assert row_limit.dtype == torch.int32 and row_limit.numel() == B and row_limit.is_contiguous()
    return L.ptr(row_limit)


def ln_gelu_fwd(u, gamma, beta, eps=1e-5, row_limit=None):
    """u [B,L,C] contiguous -> y = GELU(LayerNorm_C(u)), (mean, rstd) [B,L].  Rows t >= row_limit[b] are not read; y is zero there."""
    assert u.dim() == 3 and u.is_contiguous()
    B, Lr, C = u.shape
    y = torch.empty_like(u)
    mean = torch.empty(B, Lr, dtype=torch.float32, device=u.device)
    rstd = torch.empty(B, Lr, dtype=torch.float32, device=u.device)
    L.check(L.load().cst_ln_gelu_fwd(L.ptr(u), L.ptr(gamma), L.ptr(beta), L.ptr(y), L.ptr(mean), L.ptr(rstd), _row_lim(row_limit, B),
                                     B, Lr, C, eps, L.dtype_code(u.dtype), L.stream_ptr()), "cst_ln_gelu_fwd")
    return y, mean, rstd


def ln_gelu_bwd(dy, u, gamma, beta, mean, rstd, row_limit=None, want_colsum=False, padded=False):
    """-> (du, dgamma, dbeta, colsum(du) or None); the three vectors fp32.  padded: du is the interior view of a [B, L+2, C] allocation
    whose first and last row per utterance are zero (the layout of functional._row_padded, restated here because this module does not
    import that one: what the windowed dX GEMMs of functional.conv1d_cl read without a copy)."""
    assert dy.is_contiguous() and u.is_contiguous()
    B, Lr, C = u.shape
    lib = L.load()
    if padded:
        full = torch.empty(B, Lr + 2, C, dtype=u.dtype, device=u.device)
        full[:, 0].zero_()
        full[:, Lr + 1].zero_()
        du = full[:, 1:1 + Lr]
    else:
        du = torch.empty_like(u)
    dg, db = (torch.empty(C, dtype=torch.float32, device=u.device) for _ in range(2))
    dc = torch.empty(C, dtype=torch.float32, device=u.device) if want_colsum else None
    ws = workspace(lib.cst_ln_gelu_bwd_workspace(B * Lr, C), u.device)
    L.check(lib.cst_ln_gelu_bwd(L.ptr(dy), L.ptr(u), L.ptr(gamma), L.ptr(beta), L.ptr(mean), L.ptr(rstd), L.ptr(du), du.stride(0),
                                L.ptr(dg), L.ptr(db), L.ptr(dc), L.ptr(ws), _row_lim(row_limit, B), B, Lr, C, L.dtype_code(u.dtype),
                                L.stream_ptr()), "cst_ln_gelu_bwd")
    return du, dg, db, dc


def glu_fwd(z):
    z = _2d(z)
    rows, C2 = z.shape
    y = torch.empty(rows, C2 // 2, dtype=z.dtype, device=z.device)
    L.check(L.load().cst_glu_fwd(L.ptr(z), L.ptr(y), rows, C2 // 2, L.dtype_code(z.dtype), L.stream_ptr()), "cst_glu_fwd")
    return y


def glu_bwd(dy, z):
    dy, z = _2d(dy), _2d(z)
    rows, C2 = z.shape
    dz = torch.empty_like(z)
    L.check(L.load().cst_glu_bwd(L.ptr(dy), L.ptr(z), L.ptr(dz), rows, C2 // 2, L.dtype_code(z.dtype), L.stream_ptr()), "cst_glu_bwd")
    return dz


def act_bwd(dy, z, act):
    assert dy.is_contiguous() and z.is_contiguous()
    dx = torch.empty_like(z)
    L.check(L.load().cst_act_bwd(L.ptr(dy), L.ptr(z), L.ptr(dx), z.numel(), act, L.dtype_code(z.dtype), L.stream_ptr()), "cst_act_bwd")
    return dx


def posconv_fwd(x, wg, bias, groups, m_len=None):
    """Positional convolution forward on the channels-last input (posconv.hip): x [B,T,C] bf16, wg [g][co][j][ci] -> (y, z)."""
    B, T, C = x.shape
    k = wg.shape[2]
    assert x.is_contiguous() and wg.is_contiguous() and x.dtype == torch.bfloat16 and wg.dtype == x.dtype
    y = torch.empty_like(x)
    z = torch.empty_like(x)
    L.check(L.load().cst_posconv_fwd(L.ptr(x), L.ptr(wg), L.ptr(bias) if bias is not None else None, L.ptr(y), L.ptr(z),
                                     _per_batch(m_len, B, "gemm_m_len"), B, T, C, groups, k, L.stream_ptr()), "cst_posconv_fwd")
    return y, z


def posconv_dx(dz, wflip, dy, groups, m_len=None):
    """dx = dy + the transposed convolution of dz: wflip [g][ci][j'][co]."""
    B, T, C = dz.shape
    k = wflip.shape[2]
    assert dz.is_contiguous() and dy.is_contiguous() and wflip.is_contiguous() and dz.dtype == torch.bfloat16
    dx = torch.empty_like(dz)
    L.check(L.load().cst_posconv_dx(L.ptr(dz), L.ptr(wflip), L.ptr(dy), L.ptr(dx), _per_batch(m_len, B, "gemm_m_len"),
                                    B, T, C, groups, k, L.stream_ptr()), "cst_posconv_dx")
    return dx


def posconv_dw(dz, x, groups, k, db=None, k_live=None):
    """Weight gradient [C, C/groups, k] (the parameter's layout) over every frame of the batch; db ([C], optional) receives the bias gradient."""
    B, T, C = dz.shape
    assert dz.is_contiguous() and x.is_contiguous() and dz.dtype == torch.bfloat16 and x.dtype == dz.dtype
    assert db is None or (db.dtype == dz.dtype and db.numel() == C and db.is_contiguous())
    dw = torch.empty(C, C // groups, k, dtype=dz.dtype, device=dz.device)
    Tp = T + k - 1 + (1 if k % 2 == 0 else 0)
    stamps, epoch = _stamps(k_live, B * Tp - (k - 1), "gemm_k_live")  # (the limits count under the GEMM route's names: same meaning)
    L.check(L.load().cst_posconv_dw(L.ptr(dz), L.ptr(x), L.ptr(dw), L.ptr(db) if db is not None else None,
                                    stamps, epoch, B, T, C, groups, k, L.stream_ptr()), "cst_posconv_dw")
    return dw


def act_fwd(x, act):
    assert x.is_contiguous()
    y = torch.empty_like(x)
    L.check(L.load().cst_act_fwd(L.ptr(x), L.ptr(y), x.numel(), act, L.dtype_code(x.dtype), L.stream_ptr()), "cst_act_fwd")
    return y


def colsum(x, out_dtype=torch.float32, live=None, defer=False):
    """Column sums (bias gradients) in `out_dtype`: row-chunk fp32 partials + a fixed-order reduce that writes the parameter
    dtype (cst_colsum_typed) — deterministic, and two launches where the atomics version needs three (zero-fill, kernel, dtype
    conversion).  (A single-launch variant with a last-arriving-block finalize was measured earlier: the agent-scope release
    every workgroup needs before its ticket made it slower, elementwise 4.4 -> 7.4 ms per update.)
    defer: the caller allows the second stage to wait for the deferred-reduction flush (the result is a parameter gradient)."""
    x = _2d(x)
    rows, cols = x.shape
    lib = L.load()
    out = torch.empty(cols, dtype=out_dtype, device=x.device)

    def launch(ws, po):
        if live is not None:  # (stamps, epoch) of x's 64-row tiles: dead tiles are all zero and skipped
            assert live[0].numel() * 64 >= rows
            L.check(lib.cst_colsum_typed_live(L.ptr(x), x.stride(0), po, L.ptr(ws), rows, cols, L.dtype_code(x.dtype),
                                              L.dtype_code(out_dtype), L.ptr(live[0]), live[1], L.stream_ptr()), "cst_colsum_typed_live")
        else:
            L.check(lib.cst_colsum_typed(L.ptr(x), x.stride(0), po, L.ptr(ws), rows, cols, L.dtype_code(x.dtype), L.dtype_code(out_dtype),
                                         L.stream_ptr()), "cst_colsum_typed")

    _two_stage(lib.cst_colsum_workspace(rows, cols), (out,), defer, launch)
    return out


def dropout_colsum(x, p, key, out_dtype=torch.float32, live=None, defer=False):
    """(x * mask / (1 - p), column sums of that) in one pass (cst_dropout_colsum): the masked gradient of a dropped Linear output and
    its bias gradient.  Same bits as dropout() followed by colsum().  defer: as in colsum()."""
    x = _2d(x)
    assert x.is_contiguous()
    rows, cols = x.shape
    lib = L.load()
    xd = torch.empty_like(x)
    out = torch.empty(cols, dtype=out_dtype, device=x.device)

    def launch(ws, po):
        L.check(lib.cst_dropout_colsum(L.ptr(x), L.ptr(xd), po, L.ptr(ws), rows, cols, L.dtype_code(x.dtype),
                                       L.dtype_code(out_dtype), float(p), int(key) & 0xFFFFFFFF, L.ptr(live[0]) if live is not None else None,
                                       live[1] if live is not None else 0, L.stream_ptr()), "cst_dropout_colsum")

    _two_stage(lib.cst_colsum_workspace(rows, cols), (out,), defer, launch)
    return xd, out


def colsum_atomic(x):
    """cst_colsum: the atomics version (fp32 output), kept in the ABI."""
    x = _2d(x)
    rows, cols = x.shape
    out = torch.empty(cols, dtype=torch.float32, device=x.device)
    L.check(L.load().cst_colsum(L.ptr(x), x.stride(0), L.ptr(out), rows, cols, L.dtype_code(x.dtype), L.stream_ptr()), "cst_colsum")
    return out


def col2im1d(dcol, z, B, Lin, Lout, C, k, stride, pad, dact):
    dx = torch.empty(B, Lin, C, dtype=dcol.dtype, device=dcol.device)
    L.check(L.load().cst_col2im1d(L.ptr(dcol), L.ptr(z), L.ptr(dx), B, Lin, Lout, C, k, stride, pad, dact,
                                  L.dtype_code(dcol.dtype), L.stream_ptr()), "cst_col2im1d")
    return dx


def mask_rows(x, mask_u8):
    x = _2d(x)
    y = torch.empty_like(x)
    L.check(L.load().cst_mask_rows(L.ptr(x), L.ptr(mask_u8), L.ptr(y), x.shape[0], x.shape[1], L.dtype_code(x.dtype),
                                   L.stream_ptr()), "cst_mask_rows")
    return y


def rows_pack(x, seq_off, n_rows, tail_sum):
    """[B, T, C] -> [n_rows, C] (include/cst.h: cst_rows_pack)."""
    assert x.dim() == 3 and x.is_contiguous() and seq_off.dtype == torch.int32 and seq_off.numel() == x.shape[0] + 1
    out = torch.empty(n_rows, x.shape[2], dtype=x.dtype, device=x.device)
    L.check(L.load().cst_rows_pack(L.ptr(x), L.ptr(seq_off), L.ptr(out), x.shape[0], x.shape[1], x.shape[2], int(bool(tail_sum)), L.dtype_code(x.dtype),
                                   L.stream_ptr()), "cst_rows_pack")
    return out


def rows_unpack(y, seq_off, B, T, tail_broadcast):
    """[n_rows, C] -> [B, T, C] (include/cst.h: cst_rows_unpack)."""
    assert y.dim() == 2 and y.is_contiguous() and seq_off.dtype == torch.int32 and seq_off.numel() == B + 1
    out = torch.empty(B, T, y.shape[1], dtype=y.dtype, device=y.device)
    L.check(L.load().cst_rows_unpack(L.ptr(y), L.ptr(seq_off), L.ptr(out), B, T, y.shape[1], int(bool(tail_broadcast)), L.dtype_code(y.dtype),
                                     L.stream_ptr()), "cst_rows_unpack")
    return out


def dropout(x, p, key):
    """y = x * keep(key, idx) / (1 - p); x contiguous."""
    assert x.is_contiguous()
    y = torch.empty_like(x)
    L.check(L.load().cst_dropout(L.ptr(x), L.ptr(y), x.numel(), float(p), int(key) & 0xFFFFFFFF, L.dtype_code(x.dtype), L.stream_ptr()),
            "cst_dropout")
    return y


def conv_row_limits(nz_last, conv_spec, samples):
    """int32 [L, 1 + smax, B] live-frame limits of every conv layer from the real frame counts behind the last one (include/cst.h:
    cst_conv_row_limits) — one launch instead of ~15 tiny torch kernels per layer."""
    Lc = len(conv_spec)
    ks = (ctypes.c_int32 * Lc)(*[int(c[1]) for c in conv_spec])
    st = (ctypes.c_int32 * Lc)(*[int(c[2]) for c in conv_spec])
    smax = max([int(c[2]) for c in conv_spec[1:]] or [1])
    B = nz_last.numel()
    assert nz_last.dtype == torch.int32 and nz_last.is_contiguous()
    out = torch.empty(Lc, 1 + smax, B, dtype=torch.int32, device=nz_last.device)
    L.check(L.load().cst_conv_row_limits(L.ptr(nz_last), ks, st, Lc, int(samples), L.ptr(out), B, smax, L.stream_ptr()), "cst_conv_row_limits")
    return out


def dropout_scale(x, alpha, p, key):
    """y = alpha * x * keep(key, idx) / (1 - p); x contiguous, numel % 8 == 0."""
    assert x.is_contiguous()
    y = torch.empty_like(x)
    L.check(L.load().cst_dropout_scale(L.ptr(x), L.ptr(y), x.numel(), float(alpha), float(p), int(key) & 0xFFFFFFFF, L.dtype_code(x.dtype),
                                       L.stream_ptr()), "cst_dropout_scale")
    return y


def embed_pos_fwd(tokens, pad_mask, embed, x, pos_table, scale, pad_idx, p, key):
    """dropout(scale * (embed[tokens] | x) + pos_table[make_positions(pad_mask | tokens)]) -> [B, T, C] (include/cst.h)."""
    ref = tokens if tokens is not None else (pad_mask if pad_mask is not None else x)
    B, T = ref.shape[0], ref.shape[1]
    src = embed if embed is not None else x
    C = src.shape[-1]
    V = embed.shape[0] if embed is not None else 0
    assert src.is_contiguous() and (tokens is None or (tokens.dtype == torch.int64 and tokens.is_contiguous()))
    assert pad_mask is None or (pad_mask.dtype == torch.uint8 and pad_mask.is_contiguous() and pad_mask.shape == (B, T))
    assert pos_table is None or (pos_table.dtype == torch.float32 and pos_table.is_contiguous() and pos_table.shape[1] == C)
    out = torch.empty(B, T, C, dtype=src.dtype, device=src.device)
    L.check(L.load().cst_embed_pos_fwd(L.ptr(tokens), L.ptr(pad_mask), L.ptr(embed), L.ptr(x), L.ptr(pos_table), float(scale), int(pad_idx),
                                       L.ptr(out), B, T, C, V, 0 if pos_table is None else pos_table.shape[0], float(p), int(key) & 0xFFFFFFFF,
                                       L.dtype_code(src.dtype), L.stream_ptr()), "cst_embed_pos_fwd")
    return out


def embed_bwd(dy, tokens, V, scale, pad_idx, p, key, grad_dtype):
    """Deterministic embedding-table gradient [V, C] of embed_pos_fwd (include/cst.h)."""
    dy = dy.reshape(-1, dy.shape[-1])
    assert dy.is_contiguous() and tokens.is_contiguous() and tokens.numel() == dy.shape[0]
    dE = torch.empty(V, dy.shape[1], dtype=grad_dtype, device=dy.device)
    L.check(L.load().cst_embed_bwd(L.ptr(dy), L.ptr(tokens), L.ptr(dE), float(scale), int(pad_idx), dy.shape[0], dy.shape[1], V, float(p),
                                   int(key) & 0xFFFFFFFF, L.dtype_code(dy.dtype), L.dtype_code(grad_dtype), L.stream_ptr()), "cst_embed_bwd")
    return dE


def ls_ce_fwd(logits, target, eps, pad):
    logits = _2d(logits)
    rows, V = logits.shape
    out2 = torch.empty(2, dtype=torch.float32, device=logits.device)
    lse = torch.empty(rows, dtype=torch.float32, device=logits.device)
    ws = workspace(2 * rows * 4, logits.device)
    L.check(L.load().cst_ls_ce_fwd(L.ptr(logits), L.ptr(target), L.ptr(out2), L.ptr(lse), L.ptr(ws), rows, V, eps, pad,
                                   L.dtype_code(logits.dtype), L.stream_ptr()), "cst_ls_ce_fwd")
    return out2, lse


def ls_ce_bwd(logits, target, lse, gscale, eps, pad):
    logits = _2d(logits)
    rows, V = logits.shape
    d = torch.empty_like(logits)
    L.check(L.load().cst_ls_ce_bwd(L.ptr(logits), L.ptr(target), L.ptr(lse), L.ptr(gscale), L.ptr(d), rows, V, eps, pad,
                                   L.dtype_code(logits.dtype), L.stream_ptr()), "cst_ls_ce_bwd")
    return d


CTC_L_MAX = 2047  # include/cst.h: the longest padded target cst_ctc_fwd takes


def _ctc_layout(logits):
    """[T, B, V] logits -> (tensor, stride_t, stride_b) with unit class stride; a copy only where the class stride is not 1."""
    if logits.dim() != 3:
        raise ValueError("ctc: logits must be [T, B, V], got %s" % (tuple(logits.shape),))
    if logits.stride(2) != 1 and logits.shape[2] > 1:
        logits = logits.contiguous()
    T, B, V = logits.shape
    # (a dimension of one element has no stride to speak of)
    return logits, (logits.stride(0) if T > 1 else max(logits.stride(0), V)), (logits.stride(1) if B > 1 else max(logits.stride(1), V))


def _ctc_lens(t, n, name):
    if t.dtype != torch.int64 or tuple(t.shape) != (n,):
        raise ValueError("ctc: %s must be int64 [%d], got %s %s" % (name, n, t.dtype, tuple(t.shape)))
    return t.contiguous()


def ctc_fwd(logits, targets, target_len, input_len, blank, zero_infinity=False, need_grad=True, check_targets=False):
    """cst_ctc_fwd (include/cst.h): logits [T, B, V] fp32 / bf16 in any layout with unit class stride (the time-major view of batch-major
    memory included), targets int64 [B, Lmax] padded, target_len / input_len int64 [B] ON THE DEVICE ->
    (loss fp32 [1], nll fp32 [B], saved), `saved` = what ctc_bwd needs.  check_targets=True reads the labels' range on the host (one
    synchronisation) and raises ValueError for a label outside [0, V) or equal to the blank; the training path leaves it off."""
    logits, st, sb = _ctc_layout(logits)
    T, B, V = logits.shape
    if targets.dtype != torch.int64 or targets.dim() != 2 or targets.shape[0] != B:
        raise ValueError("ctc: targets must be int64 [%d, Lmax], got %s %s" % (B, targets.dtype, tuple(targets.shape)))
    targets = targets.contiguous()
    Lmax = targets.shape[1]
    target_len, input_len = _ctc_lens(target_len, B, "target_len"), _ctc_lens(input_len, B, "input_len")
    if check_targets and Lmax:
        live = targets[torch.arange(Lmax, device=targets.device)[None, :] < target_len[:, None]]
        if live.numel():
            lo, hi, nb = torch.stack([live.min(), live.max(), live.eq(blank).sum()]).tolist()
            if lo < 0 or hi >= V or nb:
                raise ValueError("ctc: labels must lie in [0, %d) and differ from the blank %d; found %d .. %d, %d blanks" % (V, blank, lo, hi, nb))
    dev = logits.device
    S = 2 * min(Lmax, CTC_L_MAX) + 1  # (beyond the cap the entry refuses before it touches a buffer)
    f32 = dict(dtype=torch.float32, device=dev)
    nll, loss, lse = torch.empty(B, **f32), torch.empty(1, **f32), torch.empty(B, T, **f32)
    emit, alpha = torch.empty(B, T, S, **f32), torch.empty(B, T, S, **f32)
    beta = torch.empty(B, T, S, **f32) if need_grad else None
    L.check(L.load().cst_ctc_fwd(L.ptr(logits), st, sb, L.ptr(targets), Lmax, L.ptr(target_len), L.ptr(input_len), int(blank),
                                 int(bool(zero_infinity)), L.ptr(nll), L.ptr(loss), L.ptr(lse), L.ptr(emit), L.ptr(alpha), L.ptr(beta),
                                 T, B, V, L.dtype_code(logits.dtype), L.stream_ptr()), "cst_ctc_fwd")
    return loss, nll, (logits, targets, target_len, input_len, nll, lse, alpha, beta)


def ctc_bwd(saved, gscale, blank, zero_infinity=False):
    """cst_ctc_bwd: gscale fp32 device scalar [1] -> dlogits in the logits' dtype, [T, B, V] contiguous."""
    logits, targets, target_len, input_len, nll, lse, alpha, beta = saved
    assert beta is not None, "ctc_fwd ran with need_grad=False"
    _, st, sb = _ctc_layout(logits)
    T, B, V = logits.shape
    d = torch.empty(T, B, V, dtype=logits.dtype, device=logits.device)
    L.check(L.load().cst_ctc_bwd(L.ptr(logits), st, sb, L.ptr(targets), targets.shape[1], L.ptr(target_len), L.ptr(input_len), int(blank),
                                 int(bool(zero_infinity)), L.ptr(nll), L.ptr(lse), L.ptr(alpha), L.ptr(beta), L.ptr(gscale), L.ptr(d),
                                 B * V, V, T, B, V, L.dtype_code(logits.dtype), L.stream_ptr()), "cst_ctc_bwd")
    return d


def ctc_greedy(logits, input_len, blank):
    """cst_ctc_greedy: logits [T, B, V] (layouts as ctc_fwd), input_len int64 [B] on the device -> (ids int32 [B, T], counts int32 [B]),
    views of ONE int32 buffer `packed` [B*T + B], also returned: one transfer brings both to the host."""
    logits, st, sb = _ctc_layout(logits)
    T, B, V = logits.shape
    input_len = _ctc_lens(input_len, B, "input_len")
    packed = torch.empty(B * T + B, dtype=torch.int32, device=logits.device)
    ids, counts = packed[:B * T].view(B, T), packed[B * T:]
    ws = workspace(B * T * 4, logits.device)
    L.check(L.load().cst_ctc_greedy(L.ptr(logits), st, sb, L.ptr(input_len), int(blank), L.ptr(ws), L.ptr(ids), L.ptr(counts), T, B, V,
                                    L.dtype_code(logits.dtype), L.stream_ptr()), "cst_ctc_greedy")
    return ids, counts, packed


CTC_BEAM_K_MAX, CTC_BEAM_N_MAX, CTC_BEAM_KN_MAX = 128, 128, 8192  # include/cst.h: the envelope of cst_ctc_beam


def ctc_beam_supported(K, N):
    """Whether cst_ctc_beam takes a beam of K prefixes with N classes per frame (beyond: CST_ERR_UNSUPPORTED)."""
    return 1 <= K <= CTC_BEAM_K_MAX and 1 <= N <= CTC_BEAM_N_MAX and K * N <= CTC_BEAM_KN_MAX


def ctc_topn(logits, input_len, blank, N, check=False):
    """cst_ctc_topn: logits [T, B, V] (layouts as ctc_fwd), input_len int64 [B] on the device -> (lse fp32 [B, T], blank_lp fp32 [B, T],
    tok_id int32 [B, T, N], tok_lp fp32 [B, T, N]).  check=True validates blank and N here and raises ValueError."""
    logits, st, sb = _ctc_layout(logits)
    T, B, V = logits.shape
    input_len = _ctc_lens(input_len, B, "input_len")
    if check and not (0 <= blank < V and 1 <= N <= CTC_BEAM_N_MAX):
        raise ValueError("ctc_topn: blank %d must lie in [0, %d) and N %d in [1, %d]" % (blank, V, N, CTC_BEAM_N_MAX))
    dev = logits.device
    n = max(int(N), 1)
    lse, blank_lp = torch.empty(B, T, dtype=torch.float32, device=dev), torch.empty(B, T, dtype=torch.float32, device=dev)
    tok_id, tok_lp = torch.empty(B, T, n, dtype=torch.int32, device=dev), torch.empty(B, T, n, dtype=torch.float32, device=dev)
    L.check(L.load().cst_ctc_topn(L.ptr(logits), st, sb, L.ptr(input_len), int(blank), int(N), L.ptr(lse), L.ptr(blank_lp), L.ptr(tok_id),
                                  L.ptr(tok_lp), T, B, V, L.dtype_code(logits.dtype), L.stream_ptr()), "cst_ctc_topn")
    return lse, blank_lp, tok_id, tok_lp


def ctc_beam(logits, input_len, blank, lists, K, beam_threshold, nbest, trace=False, check=False):
    """cst_ctc_beam over `lists` = ctc_topn(logits, input_len, blank, N): -> dict(tokens int32 [B, nbest, T] (-1 padded), len int32
    [B, nbest], score fp32 [B, nbest], n_hyp int32 [B], packed — ONE int32 buffer all four are views of (score through a float32 view):
    one transfer brings the result to the host) and, with trace, trace_node int32 / trace_pb / trace_pnb fp32 [B, T, K] and nodes int32
    [B, 4, 1 + T K] (parents, tokens, child links).  check=True validates the envelope here and raises ValueError."""
    logits, st, sb = _ctc_layout(logits)
    T, B, V = logits.shape
    input_len = _ctc_lens(input_len, B, "input_len")
    lse, blank_lp, tok_id, tok_lp = lists
    N = tok_id.shape[2]
    K, nbest = int(K), int(nbest)
    if check and not (ctc_beam_supported(K, N) and 1 <= nbest <= K):
        raise ValueError("ctc_beam: beam %d, %d classes per frame, nbest %d outside K <= %d, N <= %d, K N <= %d, 1 <= nbest <= K"
                         % (K, N, nbest, CTC_BEAM_K_MAX, CTC_BEAM_N_MAX, CTC_BEAM_KN_MAX))
    dev = logits.device
    nb, kk = max(nbest, 1), max(K, 1)
    packed = torch.empty(B * nb * T + 2 * B * nb + B, dtype=torch.int32, device=dev)
    o1, o2, o3 = B * nb * T, B * nb * T + B * nb, B * nb * T + 2 * B * nb
    tokens, lens, score, n_hyp = packed[:o1].view(B, nb, T), packed[o1:o2].view(B, nb), packed[o2:o3].view(torch.float32).view(B, nb), packed[o3:]
    nodes = torch.empty(B, 4, 1 + T * kk, dtype=torch.int32, device=dev) if trace else None
    ws = nodes if trace else workspace(int(L.load().cst_ctc_beam_workspace_bytes(T, B, kk, N)), dev)
    tn = tb = tnb = None
    if trace:
        tn = torch.full((B, T, kk), -1, dtype=torch.int32, device=dev)
        tb = torch.full((B, T, kk), float("-inf"), dtype=torch.float32, device=dev)
        tnb = torch.full((B, T, kk), float("-inf"), dtype=torch.float32, device=dev)
    L.check(L.load().cst_ctc_beam(L.ptr(logits), st, sb, L.ptr(input_len), int(blank), L.ptr(lse), L.ptr(blank_lp), L.ptr(tok_id),
                                  L.ptr(tok_lp), N, K, float(beam_threshold), nbest, L.ptr(ws), L.ptr(tokens), L.ptr(lens), L.ptr(score),
                                  L.ptr(n_hyp), L.ptr(tn), L.ptr(tb), L.ptr(tnb), T, B, V, L.dtype_code(logits.dtype), L.stream_ptr()),
            "cst_ctc_beam")
    out = dict(tokens=tokens, len=lens, score=score, n_hyp=n_hyp, packed=packed)
    if trace:
        out.update(trace_node=tn, trace_pb=tb, trace_pnb=tnb, nodes=nodes)
    return out


def edit_distance(a, b):
    """cst_edit_distance: Levenshtein distance of two sequences of ints (host)."""
    import ctypes

    import numpy as np
    a, b = np.ascontiguousarray(a, dtype=np.int64), np.ascontiguousarray(b, dtype=np.int64)
    lib = L.load()
    d = lib.cst_edit_distance(a.ctypes.data_as(ctypes.c_void_p) if a.size else None, a.size,
                              b.ctypes.data_as(ctypes.c_void_p) if b.size else None, b.size)
    if d < 0:
        raise RuntimeError("cst_edit_distance failed (%d): %s" % (d, lib.cst_last_error().decode()))
    return int(d)


def _score_rows(x):
    """[B, T, V] -> the 2-D view [B*T, V] (unit column stride, one row stride); a copy only where [B, T] is not one run of rows."""
    B, T, V = x.shape
    step = x.stride(1) if T > 1 else x.stride(0)
    if x.stride(2) == 1 and step >= V and (B == 1 or T == 1 or x.stride(0) == T * step):
        return x.as_strided((B * T, V), (step, 1))
    return x.contiguous().view(B * T, V)


def score_tokens(logits_list, target, pad):
    """Scores of given target tokens under one model or an ensemble (cst_score_tokens): logits_list = N <= 8 tensors [B, T, V] of one
    dtype and shape, target int64 [B, T] -> (pos fp32 [B, T], score fp32 [B], len int32 [B]), views of ONE buffer `packed` (fp32
    [B*T + 2B], also returned: one transfer brings all three to the host).  The kernel cannot validate device data, so the target ids
    are checked here: an id outside [0, V) that is not `pad` raises ValueError and nothing is launched."""
    logits_list = list(logits_list)
    if not 1 <= len(logits_list) <= 8:
        raise ValueError("score_tokens takes 1 to 8 ensemble members, got %d" % len(logits_list))
    B, T, V = logits_list[0].shape
    if tuple(target.shape) != (B, T) or target.dtype != torch.int64:
        raise ValueError("score_tokens: target must be int64 [%d, %d], got %s %s" % (B, T, target.dtype, tuple(target.shape)))
    for x in logits_list:
        if x.shape != logits_list[0].shape or x.dtype != logits_list[0].dtype:
            raise ValueError("score_tokens: the members' logits differ in shape or dtype")
    rows = [_score_rows(x) for x in logits_list]
    if len({x.stride(0) for x in rows}) > 1:  # one row stride serves all members
        rows = [x.contiguous() for x in rows]
    ld = max(rows[0].stride(0), V)  # (a single row has no stride to speak of)
    target = target.contiguous()
    live = target[target.ne(pad)]
    if live.numel():
        lo, hi = torch.stack([live.min(), live.max()]).tolist()
        if lo < 0 or hi >= V:
            raise ValueError("score_tokens: target ids must lie in [0, %d) or be the pad index %d; found %d .. %d" % (V, pad, lo, hi))
    packed = torch.empty(B * T + 2 * B, dtype=torch.float32, device=target.device)
    pos, score, length = packed[:B * T].view(B, T), packed[B * T:B * T + B], packed[B * T + B:].view(torch.int32)
    others = (L.c_p * 7)(*[x.data_ptr() for x in rows[1:]])
    L.check(L.load().cst_score_tokens(L.ptr(rows[0]), others, len(rows), ld, L.ptr(target), int(pad), L.ptr(pos), L.ptr(score),
                                      L.ptr(length), B, T, V, L.dtype_code(rows[0].dtype), L.stream_ptr()), "cst_score_tokens")
    return pos, score, length, packed


def attn_avg_probs(q, k, H, kpm, scale, k_strides=None, out=None, out_row_stride=None, step=None, max_len=0, out_scale=1.0,
                   accumulate=False):
    """Head-averaged attention probabilities (cst_attn_avg_probs): q [B, Tq, H*D] (unit channel stride, one row stride), k [B, S, H*D]
    with unit channel stride — or any layout given as k_strides = (k_sb, k_sh, k_st) in elements with k's shape [B, S, ...] only read
    for B and S — kpm uint8 / bool [B, S] or None -> fp32 [B, Tq, S].  out / out_row_stride / step / max_len / out_scale / accumulate:
    the kernel's own (include/cst.h); without `out` a fresh tensor is returned."""
    B, Tq, C = q.shape
    S, D = k.shape[1], C // H
    if q.stride(2) != 1 or (B > 1 and q.stride(0) != Tq * q.stride(1)):
        q = q.contiguous()
    if k_strides is None:
        if k.stride(2) != 1:
            k = k.contiguous()
        k_strides = (k.stride(0), D, k.stride(1))
    if kpm is not None:
        kpm = kpm.to(torch.uint8).contiguous()
    if out is None:
        out = torch.empty(B, Tq, S, dtype=torch.float32, device=q.device)
        out_row_stride = S
    L.check(L.load().cst_attn_avg_probs(L.ptr(q), q.stride(1), L.ptr(k), *k_strides, L.ptr(kpm), L.ptr(out), out_row_stride, L.ptr(step),
                                        max_len, B, Tq, H, D, S, float(scale), float(out_scale), int(bool(accumulate)),
                                        L.dtype_code(q.dtype), L.stream_ptr()), "cst_attn_avg_probs")
    return out


def w2v_negatives(key, B, M, K, Kx=0, device="cuda"):
    """cst_w2v_negatives: the negatives of every masked position, int32 [B, M, K + Kx] flat row indices into [B * M] (K from the position's
    own utterance, Kx from the whole batch), drawn from the counter hash at `key` (rng.next_key()); rng.negatives_numpy is the twin."""
    out = torch.empty(B, M, K + Kx, dtype=torch.int32, device=device)
    L.check(L.load().cst_w2v_negatives(int(key) & 0xFFFFFFFF, B, M, K, Kx, L.ptr(out), L.stream_ptr()), "cst_w2v_negatives")
    return out


def infonce_fwd(x, y, idx, inv_temp, want_logits=False):
    """cst_infonce_fwd (include/cst.h): x, y [N, D] fp32 / bf16, idx int32 [N, K'] -> (loss fp32 [1], nll fp32 [N], counters int32 [2] =
    (correct, count), saved, logits); `saved` is what infonce_bwd needs, `logits` fp32 [N, K' + 1] only under want_logits (tests)."""
    if x.dim() != 2 or x.shape != y.shape or x.dtype != y.dtype:
        raise ValueError("infonce: x and y must be [N, D] of one dtype, got %s %s / %s %s" % (tuple(x.shape), x.dtype, tuple(y.shape), y.dtype))
    N, D = x.shape
    if idx.dtype != torch.int32 or idx.dim() != 2 or idx.shape[0] != N:
        raise ValueError("infonce: idx must be int32 [%d, K'], got %s %s" % (N, idx.dtype, tuple(idx.shape)))
    x, y, idx = x.contiguous(), y.contiguous(), idx.contiguous()
    KP = idx.shape[1]
    dev = x.device
    f32 = dict(dtype=torch.float32, device=dev)
    nll, loss, stats = torch.empty(N, **f32), torch.empty(1, **f32), torch.empty(3, N, **f32)
    counters = torch.empty(2, dtype=torch.int32, device=dev)
    logits = torch.empty(N, KP + 1, **f32) if want_logits else None
    flags = workspace(N * 4, dev)
    lse, nx, ny = stats[0], stats[1], stats[2]
    L.check(L.load().cst_infonce_fwd(L.ptr(x), L.ptr(y), L.ptr(idx), float(inv_temp), L.ptr(nll), L.ptr(loss), L.ptr(counters), L.ptr(lse),
                                     L.ptr(nx), L.ptr(ny), L.ptr(flags), L.ptr(logits), N, KP, D, L.dtype_code(x.dtype), L.stream_ptr()),
            "cst_infonce_fwd")
    return loss, nll, counters, (x, y, idx, stats), logits


def infonce_bwd(saved, gscale, inv_temp, need_dy=True):
    """cst_infonce_bwd_x, then cst_infonce_bwd_y through the inverted index of the targets: gscale fp32 device scalar [1] -> (dx, dy) in
    the operands' dtype.  The index is integers only and is built on the device without a host read: a stable sort of the keys
    cat(0 .. N-1, idx.flatten()) (a row's own positive first, then its draws in ascending (position, j)) and the rows' first places."""
    x, y, idx, stats = saved
    N, D = x.shape
    KP = idx.shape[1]
    lse, nx, ny = stats[0], stats[1], stats[2]
    dx = torch.empty_like(x)
    pairs = torch.empty(N, KP + 1, 2, dtype=torch.float32, device=x.device)
    code = L.dtype_code(x.dtype)
    L.check(L.load().cst_infonce_bwd_x(L.ptr(x), L.ptr(y), L.ptr(idx), float(inv_temp), L.ptr(lse), L.ptr(nx), L.ptr(ny), L.ptr(gscale),
                                       L.ptr(dx), L.ptr(pairs), N, KP, D, code, L.stream_ptr()), "cst_infonce_bwd_x")
    if not need_dy:
        return dx, None
    rows = torch.arange(N + 1, dtype=torch.int32, device=x.device)
    keys = torch.cat([rows[:N], idx.reshape(-1).clamp(0, N - 1)])
    skeys, perm = torch.sort(keys, stable=True)
    offs = torch.searchsorted(skeys, rows, out_int32=True)
    dy = torch.empty_like(y)
    L.check(L.load().cst_infonce_bwd_y(L.ptr(x), L.ptr(y), L.ptr(perm), L.ptr(offs), L.ptr(pairs), L.ptr(nx), L.ptr(ny), L.ptr(dy), N, KP, D,
                                       code, L.stream_ptr()), "cst_infonce_bwd_y")
    return dx, dy


def gumbel_vq_fwd(logits, vars_, G, training, key=0, noise=None):
    """cst_gumbel_vq_fwd (include/cst.h): logits [N, G * V], vars_ [G * V, d] of one dtype -> (q [N, G * d], idx int32 [N, G], onehot
    [N, G * V], avg_probs fp32 [G, V], stats fp32 [2] = (prob_perplexity, code_perplexity), exph fp32 [G]).  noise: fp32 [N, G, V] read
    instead of the counter hash at `key` (tests, fixtures)."""
    if logits.dim() != 2 or vars_.dim() != 2 or logits.dtype != vars_.dtype or logits.shape[1] != vars_.shape[0] or logits.shape[1] % G:
        raise ValueError("gumbel_vq: logits [N, G V] and vars [G V, d] of one dtype expected, got %s %s / %s %s, G = %d"
                         % (tuple(logits.shape), logits.dtype, tuple(vars_.shape), vars_.dtype, G))
    logits, vars_ = logits.contiguous(), vars_.contiguous()
    N, GV = logits.shape
    V, d = GV // G, vars_.shape[1]
    if noise is not None:
        if noise.dtype != torch.float32 or noise.numel() != N * GV:
            raise ValueError("gumbel_vq: noise must be fp32 [%d, %d, %d], got %s %s" % (N, G, V, noise.dtype, tuple(noise.shape)))
        noise = noise.contiguous()
    dev = logits.device
    lib = L.load()
    q = torch.empty(N, G * d, dtype=logits.dtype, device=dev)
    onehot = torch.empty(N, GV, dtype=logits.dtype, device=dev)
    idx = torch.empty(N, G, dtype=torch.int32, device=dev)
    avg = torch.empty(G, V, dtype=torch.float32, device=dev)
    stats = torch.empty(2 + G, dtype=torch.float32, device=dev)
    ws = workspace(max(int(lib.cst_gumbel_vq_workspace(N, G, V)), 4), dev)
    L.check(lib.cst_gumbel_vq_fwd(L.ptr(logits), L.ptr(vars_), L.ptr(noise), int(key) & 0xFFFFFFFF, int(bool(training)), L.ptr(q), L.ptr(idx),
                                  L.ptr(onehot), L.ptr(avg), L.ptr(stats), L.ptr(stats[2:]), L.ptr(ws), N, G, V, d,
                                  L.dtype_code(logits.dtype), L.stream_ptr()), "cst_gumbel_vq_fwd")
    return q, idx, onehot, avg, stats[:2], stats[2:]


def gumbel_vq_bwd(logits, gy, avg, exph, dppl, G, inv_tau, key=0, noise=None):
    """cst_gumbel_vq_bwd: gy [N, G * V] in the logits' dtype, dppl fp32 device scalar [1] -> d logits [N, G * V]."""
    N, GV = logits.shape
    dl = torch.empty_like(logits)
    L.check(L.load().cst_gumbel_vq_bwd(L.ptr(logits), L.ptr(noise), int(key) & 0xFFFFFFFF, float(inv_tau), L.ptr(gy), L.ptr(avg), L.ptr(exph),
                                       L.ptr(dppl), L.ptr(dl), N, G, GV // G, L.dtype_code(logits.dtype), L.stream_ptr()), "cst_gumbel_vq_bwd")
    return dl


def sumsq(x, out):
    lib = L.load()
    ws = workspace(lib.cst_sumsq_workspace(), x.device)
    L.check(lib.cst_sumsq(L.ptr(x), x.numel(), L.ptr(out), L.ptr(ws), L.dtype_code(x.dtype), L.stream_ptr()), "cst_sumsq")


def contrastive_fwd(a, t, temp):
    """a, t [B, M, C] contiguous -> (loss fp32[1], sim, na, nt)."""
    B, M, C = a.shape
    loss = torch.empty(1, dtype=torch.float32, device=a.device)
    sim = torch.empty(B, M, M, dtype=torch.float32, device=a.device)
    na = torch.empty(B, M, dtype=torch.float32, device=a.device)
    nt = torch.empty_like(na)
    ws = workspace(B * 4, a.device)
    L.check(L.load().cst_contrastive_fwd(L.ptr(a), L.ptr(t), L.ptr(loss), L.ptr(ws), L.ptr(sim), L.ptr(na), L.ptr(nt), B, M, C, float(temp),
                                         L.dtype_code(a.dtype), L.stream_ptr()), "cst_contrastive_fwd")
    return loss, sim, na, nt


def contrastive_bwd(a, t, sim, na, nt, gscale, temp):
    B, M, C = a.shape
    da, dt = torch.empty_like(a), torch.empty_like(t)
    L.check(L.load().cst_contrastive_bwd(L.ptr(a), L.ptr(t), L.ptr(sim), L.ptr(na), L.ptr(nt), L.ptr(gscale), L.ptr(da), L.ptr(dt), B, M, C,
                                         float(temp), L.dtype_code(a.dtype), L.stream_ptr()), "cst_contrastive_bwd")
    return da, dt


def adam_step(master, m, v, grad, param, lr, beta1, beta2, eps, wd, step, grad_scale):
    L.check(L.load().cst_adam_step(L.ptr(master), L.ptr(m), L.ptr(v), L.ptr(grad), L.ptr(param), master.numel(), lr, beta1, beta2,
                                   eps, wd, step, L.ptr(grad_scale), L.dtype_code(grad.dtype), L.dtype_code(param.dtype),
                                   L.stream_ptr()), "cst_adam_step")


def weight_norm_fwd(v, g):
    """v [..., C] contiguous, g [C] -> (w = v * g / ||v||_{all but last dim}, norm fp32 [C])."""
    C = v.shape[-1]
    R = v.numel() // C
    lib = L.load()
    w = torch.empty_like(v)
    norm = torch.empty(C, dtype=torch.float32, device=v.device)
    ws = torch.empty(int(lib.cst_weight_norm_workspace(R, C)) // 4, dtype=torch.float32, device=v.device)
    L.check(lib.cst_weight_norm_fwd(v.data_ptr(), g.data_ptr(), w.data_ptr(), norm.data_ptr(), ws.data_ptr(), R, C, L.dtype_code(v.dtype),
                                    L.stream_ptr()), "cst_weight_norm_fwd")
    return w, norm


def weight_norm_bwd(v, g, dw, norm):
    C = v.shape[-1]
    R = v.numel() // C
    lib = L.load()
    dv, dg = torch.empty_like(v), torch.empty_like(g)
    ws = torch.empty(int(lib.cst_weight_norm_workspace(R, C)) // 4, dtype=torch.float32, device=v.device)
    L.check(lib.cst_weight_norm_bwd(v.data_ptr(), g.data_ptr(), dw.data_ptr(), norm.data_ptr(), dv.data_ptr(), dg.data_ptr(), ws.data_ptr(), R, C,
                                    L.dtype_code(v.dtype), L.stream_ptr()), "cst_weight_norm_bwd")
    return dv, dg


def transpose2d(x, out=None):
    """[R, C] contiguous -> [C, R] contiguous (cst_transpose2d)."""
    R, C = x.shape
    if out is None:
        out = torch.empty(C, R, dtype=x.dtype, device=x.device)
    assert out.shape == (C, R) and out.is_contiguous() and out.dtype == x.dtype
    L.check(L.load().cst_transpose2d(x.data_ptr(), out.data_ptr(), R, C, L.dtype_code(x.dtype), L.stream_ptr()), "cst_transpose2d")
    return out


def transpose_table(pairs):
    """[(src [R, C], dst [C, R]), ...] of one dtype / device -> (device table, n, total tiles, dtype code) for transpose2d_multi.
    The table reaches the device through pinned memory (a pageable copy would drain the stream)."""
    rows, tile0 = [], 0
    for src, dst in pairs:
        R, C = src.shape
        assert src.is_contiguous() and dst.is_contiguous() and dst.shape == (C, R) and dst.dtype == src.dtype
        rows.append([src.data_ptr(), dst.data_ptr(), R, C, tile0])
        tile0 += ((R + 63) // 64) * ((C + 63) // 64)
    host = torch.tensor(rows, dtype=torch.int64).pin_memory()
    return host.to(pairs[0][0].device, non_blocking=True), len(rows), tile0, L.dtype_code(pairs[0][0].dtype), host


def transpose2d_multi(table):
    """Every matrix of a transpose_table in one launch (cst_transpose2d_multi)."""
    dev, n, total, dt = table[:4]
    L.check(L.load().cst_transpose2d_multi(dev.data_ptr(), n, total, dt, L.stream_ptr()), "cst_transpose2d_multi")


TOK_U8, TOK_U16, TOK_I32, TOK_I64 = range(4)  # include/cst.h: cst_tok_dtype
TOK_BYTES = (1, 2, 4, 8)


def collate_pairs(src_stream, tgt_stream, tok_dtype, src_off, tgt_off, idx, S, T, pad, eos, left_pad_source, left_pad_target, out=None):
    """One translation batch from a device-resident binarised corpus (cst_collate_pairs).  src_stream / tgt_stream: uint8 tensors
    holding the token streams' BYTES as stored (`tok_dtype` names the element type of both); src_off / tgt_off int64 [N + 1] element
    offsets; idx int64 [B] sentence indices in row order.  Returns (src_tokens [B, S], src_lengths [B], prev_output_tokens [B, T],
    target [B, T], buffer): int64 views of ONE buffer (`out`, int64 [B*S + 2*B*T + B], allocated when not given); every word is written."""
    B, N = idx.numel(), src_off.numel() - 1
    for t in (src_off, tgt_off, idx):
        if t.dtype != torch.int64 or not t.is_contiguous():
            raise ValueError("collate_pairs: offsets and indices must be contiguous int64 tensors")
    if tgt_off.numel() != N + 1:
        raise ValueError("collate_pairs: %d source and %d target sentences" % (N, tgt_off.numel() - 1))
    if src_stream.dtype != torch.uint8 or tgt_stream.dtype != torch.uint8:
        raise ValueError("collate_pairs: the token streams are passed as their bytes (uint8 tensors)")
    total = B * S + 2 * B * T + B
    if out is None:
        out = torch.empty(total, dtype=torch.int64, device=idx.device)
    elif out.dtype != torch.int64 or out.numel() != total or not out.is_contiguous():
        raise ValueError("collate_pairs: out must be a contiguous int64 tensor of %d words" % total)
    L.check(L.load().cst_collate_pairs(L.ptr(src_stream), L.ptr(tgt_stream), int(tok_dtype), L.ptr(src_off), L.ptr(tgt_off), N, L.ptr(idx),
                                       B, int(S), int(T), int(pad), int(eos), int(bool(left_pad_source)), int(bool(left_pad_target)),
                                       L.ptr(out), L.stream_ptr()), "cst_collate_pairs")
    a, b = B * S, B * S + B * T
    return out[:a].view(B, S), out[b + B * T:], out[a:b].view(B, T), out[b:b + B * T].view(B, T), out


def collate_blocks(stream, tok_dtype, blocks, idx, T, pad, eos, out=None):
    """One language_modeling batch from a device-resident binarised corpus (cst_collate_blocks).  stream: a uint8 tensor holding the
    token stream's BYTES as stored (`tok_dtype` names the element type); blocks int64 [n_blocks, 3] = (start element, length, prev:
    the element before the block in its source row, negative = the dictionary's eos); idx int64 [B] block indices in row order.
    Returns (src_tokens [B, T], src_lengths [B], target [B, T], buffer): int64 views of ONE buffer (`out`, int64 [2*B*T + B],
    allocated when not given); every word is written."""
    B = idx.numel()
    for t in (blocks, idx):
        if t.dtype != torch.int64 or not t.is_contiguous():
            raise ValueError("collate_blocks: blocks and indices must be contiguous int64 tensors")
    if blocks.dim() != 2 or blocks.size(1) != 3:
        raise ValueError("collate_blocks: blocks must be [n_blocks, 3], got %s" % (tuple(blocks.shape),))
    if stream.dtype != torch.uint8:
        raise ValueError("collate_blocks: the token stream is passed as its bytes (a uint8 tensor)")
    total = 2 * B * T + B
    if out is None:
        out = torch.empty(total, dtype=torch.int64, device=idx.device)
    elif out.dtype != torch.int64 or out.numel() != total or not out.is_contiguous():
        raise ValueError("collate_blocks: out must be a contiguous int64 tensor of %d words" % total)
    L.check(L.load().cst_collate_blocks(L.ptr(stream), int(tok_dtype), L.ptr(blocks), blocks.size(0), L.ptr(idx), B, int(T), int(pad),
                                        int(eos), L.ptr(out), L.stream_ptr()), "cst_collate_blocks")
    a = B * T
    return out[:a].view(B, T), out[2 * a:], out[a:2 * a].view(B, T), out
