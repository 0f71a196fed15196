"""torch.autograd.Function seam over the C-ABI kernels (the reference's seam on this
path is nn.Module.forward / autograd.Function calling ATen; here they call libcst_hip.so).

Every function requires CUDA(HIP) tensors; there is no CPU path."""
import os as _os
import weakref as _weakref

import torch

from . import kernels as K
from . import lib as L

_ACT = {None: L.ACT_NONE, "none": L.ACT_NONE, "relu": L.ACT_RELU, "gelu": L.ACT_GELU}


def _flat2d(x):
    return x.reshape(-1, x.shape[-1]).contiguous()


# ------------------------------------------------------------------------------------------------
# Linear (+bias +activation +residual) — F.linear call sites listed in include/cst.h
# ------------------------------------------------------------------------------------------------
def _vec(dtype):
    return 8 if dtype == torch.bfloat16 else 4


# Live-tile stamps: a LayerNorm backward knows, for free, which 64-row tiles of the gradient it writes are not exactly zero (the
# rows of padded frames are).  The stamps ride on the gradient tensor as an attribute (PyObject preservation keeps it on the
# way to the next node's backward; any op in between — an accumulation, a copy — yields a fresh tensor without it, which only
# means "no skipping") and the weight-gradient GEMMs that reduce over those rows skip the dead K blocks (cst_gemm_desc.k_live).
def _with_tiles(t, tiles):
    if t.is_contiguous():  # row r of the producer = row r of t flattened to [rows, cols]
        t._cst_live_tiles = (tiles[0], tiles[1], t.data_ptr(), t.numel(), t.shape[-1], t._version)
        if t._base is not None:  # views made further down the graph report the ultimate base, not `t`
            t._base._cst_live_tiles = t._cst_live_tiles
    return t


def _tiles_of(t, rows):
    """The stamps of `t` if — and only if — t is still the very tensor they were made for: same storage, same extent, same row
    width, contiguous (so that _flat2d(t) is a view with the producer's row order) and not written since (the version counter is
    shared by a base and its views; autograd may accumulate a second incoming gradient into the first one IN PLACE)."""
    lt = getattr(t, "_cst_live_tiles", None)
    if lt is None and t._base is not None:  # a view (e.g. the [T,B,C] <-> [B,T,C] transposes of the layout seam, undone again)
        lt = getattr(t._base, "_cst_live_tiles", None)
    if (lt is None or not t.is_contiguous() or lt[2] != t.data_ptr() or lt[3] != t.numel() or lt[4] != t.shape[-1]
            or lt[5] != t._version or lt[0].numel() != (rows + 63) // 64):
        return None
    return (lt[0], lt[1])


_WT_MIN_ROWS = int(_os.environ.get("CST_WT_MIN_ROWS", 512))  # token rows from which the dX GEMM takes a transposed weight copy
# (4064-row decoder shapes: 4064 x 512 x 512 20.9 us as an mn-major read, 7.6 us through the copy; the copies cost one launch per update)


def _want_wt(M, w):
    return (M >= _WT_MIN_ROWS and w.is_cuda and w.dim() == 2 and w.is_contiguous() and w.shape[0] % _vec(w.dtype) == 0
            and w.shape[1] % _vec(w.dtype) == 0 and not _os.environ.get("CST_NO_WT"))


def _wversion(w):
    """Autograd version of a weight operand; the stacked q | k | v view (stacked_rows) shares only q's counter, so it carries its
    three parameters and reports the sum of theirs."""
    parts = getattr(w, "_cst_parts", None)
    return w._version if parts is None else sum(p._version for p in parts)


class _WeightTransposes:
    """W^T copies of the Linear weights the dX GEMMs read (see _dx_gemm), kept across updates.  A weight changes only in the
    optimizer step (optim.PARAM_EPOCH counts every raw-pointer write of the flat parameter buffer) or through an in-place torch op
    (its autograd version): the first request after an optimizer step refreshes EVERY registered copy in one launch
    (cst_transpose2d_multi — one launch per update instead of one small launch per Linear per backward pass: 0.75 -> 0.15 ms per
    update on the bench configuration, ~110 launches fewer); a weight changed any other way is re-transposed on its own when it is
    asked for.

    Only weights that outlive an update are cached: views of a flat parameter buffer registered by optim.FlatParamBuffers (the
    entries go when the buffers object is collected) and free-standing nn.Parameters (held weakly).  Anything else — the torch.cat
    fallback of stacked_rows, a zero-padded odd-width weight — is transposed into a fresh tensor and forgotten."""

    def __init__(self):
        self.entries = {}     # (data_ptr, shape, dtype) -> [src: detached w | weakref to a Parameter, wt, version, epoch, storage ptr]
        self.tables = {}      # (device, dtype) -> transpose table over the entries of that kind
        self.refreshes = 0    # whole-table launches (tests)
        self.persistent = {}  # storage data_ptr of a registered flat parameter buffer -> weakref to its owner

    def register_storage(self, owner, flat):
        sp = flat.untyped_storage().data_ptr()
        self.persistent[sp] = _weakref.ref(owner)
        _weakref.finalize(owner, self._drop_storage, sp)

    def _drop_storage(self, sp):
        self.persistent.pop(sp, None)
        for k in [k for k, e in self.entries.items() if e[4] == sp]:
            del self.entries[k]
        self.tables.clear()

    def invalidate(self):
        """Forget every copy (between models of one process: bench.py's extra legs, test suites)."""
        self.entries.clear()
        self.tables.clear()

    @staticmethod
    def _src(e):
        return e[0]() if isinstance(e[0], _weakref.ref) else e[0]

    def get(self, w):
        from .optim import PARAM_EPOCH
        epoch = PARAM_EPOCH[0]
        key = (w.data_ptr(), tuple(w.shape), w.dtype)
        e = self.entries.get(key)
        if e is not None and self._src(e) is None:  # a dead Parameter whose address was handed out again
            del self.entries[key]
            self.tables.pop((w.device, w.dtype), None)
            e = None
        if e is None:
            sp = w.untyped_storage().data_ptr()
            owner = self.persistent.get(sp)
            if owner is not None and owner() is not None:
                src = w.detach()
                parts = getattr(w, "_cst_parts", None)
                if parts is not None:
                    src._cst_parts = parts
            elif isinstance(w, torch.nn.Parameter):
                src, sp = _weakref.ref(w), None
            else:
                return K.transpose2d(w)  # a temporary: not cached
            e = self.entries[key] = [src, K.transpose2d(w), _wversion(w), epoch, sp]
            self.tables.pop((w.device, w.dtype), None)
            return e[1]
        if e[2] != _wversion(w):  # written by a torch op since (load_state_dict, manual edits)
            K.transpose2d(w, e[1])
            e[2], e[3] = _wversion(w), epoch
            return e[1]
        if e[3] != epoch:  # an optimizer step since: refresh every stale copy of this kind at once
            kind = (w.device, w.dtype)
            stale = []
            for k, v in list(self.entries.items()):
                t = self._src(v)
                if t is None or t.data_ptr() != k[0]:
                    # dead, or a Parameter re-homed since it was cached (FlatParamBuffers: `p.data = view`): it is asked for under
                    # its new address from now on; this entry would be re-transposed every update into a copy nobody reads
                    del self.entries[k]
                    self.tables.pop(kind, None)
                elif t.device == w.device and k[2] == w.dtype and v[3] != epoch:
                    stale.append(v)
            ids = [id(v) for v in stale]
            t = self.tables.get(kind)
            if t is None or t[5] != ids:  # (the table is rebuilt only when the set of weights changed: first updates of a run)
                t = self.tables[kind] = K.transpose_table([(self._src(v), v[1]) for v in stale]) + (ids,)
            K.transpose2d_multi(t)
            self.refreshes += 1
            for v in stale:
                v[2], v[3] = _wversion(self._src(v)), epoch
        return e[1]


WEIGHT_TRANSPOSES = _WeightTransposes()


def _may_defer(*params):
    """May the second stage of a reduction that produces the gradients of `params` wait for the deferred-reduction flush
    (kernels.DEFER)?  Only while the mode is on, none of them is shared between modules (trainer.py marks those: a second gradient
    would be added to the first at once) and none is being accumulated into (a later micro-batch of an update)."""
    if not K.DEFER.on:
        return False
    for w in params:
        if w is None:
            continue
        for p in (getattr(w, "_cst_parts_params", None) or (w,)):
            if not isinstance(p, torch.nn.Parameter) or p.grad is not None or getattr(p, "_cst_shared", False):
                return False
    return True


def _grad_out(w):
    """The flat-gradient-buffer slot of weight `w` as the output tensor of its weight-gradient GEMM (optim.grad_slot), or None."""
    if _os.environ.get("CST_NO_GRAD_SLOT"):
        return None
    from .optim import grad_slot
    return grad_slot(w)


class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, resid, act, drop_p, drop_key):
        """y = dropout(act(x W^T + b)) + resid  (dropout fused into the GEMM epilogue, before the residual add)."""
        x2 = _flat2d(x)
        M, Kd = x2.shape
        N = weight.shape[0]
        w = weight.contiguous()
        ctx.bias_obj = bias  # (the Parameter / stacked view itself: _may_defer looks at its .grad and marks in backward)
        # odd output widths (e.g. a 60-symbol test vocabulary in bf16): zero-pad the rows of W up to the 16-byte vector
        # the dX / dW loaders need; real shapes (512/768/1024/2048/3072/10000) never take this branch.
        Np = (N + _vec(x.dtype) - 1) // _vec(x.dtype) * _vec(x.dtype)
        if Np != N:
            wp = torch.zeros(Np, Kd, dtype=w.dtype, device=w.device)
            wp[:N] = w
            w = wp
            if bias is not None:
                bp = torch.zeros(Np, dtype=bias.dtype, device=bias.device)
                bp[:N] = bias
                bias = bp
            assert resid is None and drop_p == 0.0
        y = torch.empty(M, Np, dtype=x.dtype, device=x.device)
        z = torch.empty_like(y) if act != L.ACT_NONE else None
        r2 = _flat2d(resid) if resid is not None else None
        K.gemm(x2, w, y, M, Np, Kd, a_kmajor=1, b_kmajor=1, lda=Kd, ldb=Kd, ldc=Np, bias=bias, act=act, aux_out=z, ld_aux_out=Np,
               resid=r2, ld_resid=Np, split_k=1, drop_p=drop_p, drop_key=drop_key)
        ctx.save_for_backward(x2, w, z)
        ctx.act, ctx.has_bias, ctx.has_resid = act, bias is not None, resid is not None
        ctx.drop = (drop_p, drop_key)
        ctx.xshape, ctx.N = x.shape, N
        if Np != N:
            y = y[:, :N].contiguous()
        return y.view(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        return _linear_backward(ctx, dy, None)


def _dx_gemm(dz, w, M, *, use_wt, like, resid=None, dact=L.ACT_NONE, aux_in=None, drop=(0.0, 0), m_live=None):
    """dX [M, n_in] = dropout((dz [M, n_out] W [n_out, n_in]) * act'(aux_in)) + resid, allocated like `like`.
    use_wt (large token counts, _want_wt): W^T [n_in, n_out] as a k-major B operand — both operands are then read the way the
    forward GEMM reads them (the transpose reads of an mn-major W measured 15-20 % slower on the 31 760-row shapes); the
    transposed copy of a <= 5 MB weight costs a few microseconds."""
    n_out, n_in = w.shape
    dx = torch.empty(M, n_in, dtype=like.dtype, device=like.device)
    b, b_kmajor, ldb = (WEIGHT_TRANSPOSES.get(w), 1, n_out) if use_wt else (w, 0, n_in)
    K.gemm(dz, b, dx, M, n_in, n_out, a_kmajor=1, b_kmajor=b_kmajor, lda=n_out, ldb=ldb, ldc=n_in, dact=dact, aux_in=aux_in, ld_aux_in=n_in,
           resid=resid, ld_resid=n_in, split_k=1, drop_p=drop[0], drop_key=drop[1], m_live=m_live)
    return dx


def _dw_gemm(dz, x2, w, bias_obj, M, *, db_in_dw, live, dz_travels_on, allow_slot=True, allow_defer=True):
    """(dW [n_out, n_in] = dz^T x2 over M rows, its bias gradient or None): THE weight-gradient launch of a Linear.
    dW goes into the weight's slot of the flat gradient buffer where there is one (allow_slot).  db_in_dw: the bias gradient rides in
    this GEMM (cst_gemm_desc.colsum: the caller has asked dw_colsum_is_fused).  The split-K reduce may wait for the deferred flush
    when _may_defer says so for the weight — and for bias_obj, the bias Parameter / stacked view itself, when its gradient rides along.
    A small layer's weight gradient runs on the side stream, off the dX chain (kernels.side_gemm); not when dz IS the incoming
    gradient that also travels on as the residual gradient (dz_travels_on): something upstream might add into it in place."""
    n_out, n_in = w.shape
    dw = _grad_out(w) if allow_slot else None
    if dw is None:
        dw = torch.empty(n_out, n_in, dtype=w.dtype, device=w.device)
    db = torch.empty(n_out, dtype=w.dtype, device=w.device) if db_in_dw else None
    may = allow_defer and _may_defer(w, bias_obj if db_in_dw else None)
    big = not may or not K.dw_colsum_is_fused(n_out, n_in, M, w.dtype) or dz_travels_on
    K.side_gemm(big, (dz, x2, live[0] if live is not None else None), dz, x2, dw, n_out, n_in, M, a_kmajor=0, b_kmajor=0, lda=n_out, ldb=n_in,
                ldc=n_in, split_k=-1, k_live=live, colsum=db, defer=may)
    return dw, db


def _drop_grad(dy2, drop, out_dtype, live, *, with_colsum, defer):
    """(dy2 * the dropout mask regenerated from drop = (p, key), the bias gradient or None).  with_colsum: the masked gradient is
    what the bias sees and nothing else produces its gradient: mask + column sums in one pass (second stage deferrable: `defer`)."""
    if with_colsum and not _os.environ.get("CST_NO_DROP_COLSUM"):
        return K.dropout_colsum(dy2.contiguous(), drop[0], drop[1], out_dtype, live, defer=defer)
    return K.dropout(dy2.contiguous(), *drop), None


def _linear_backward(ctx, dy, dxp):
    """Shared by _LinearFn / _LinearPassFn.  dxp: gradient that reached the pass-through alias of x (the residual branch of the
    block this projection opens); it is added in the dX GEMM's epilogue instead of by an autograd accumulation kernel."""
    x2, w, z = ctx.saved_tensors
    M, Kd = x2.shape
    Np, N = w.shape[0], ctx.N
    if dy is None:  # only the pass-through was consumed
        return dxp, None, None, None, None, None, None
    dy2 = _flat2d(dy)
    live = _tiles_of(dy, M)  # rows of dy that are exactly zero stay zero through the mask / activation derivative below
    if Np != N:
        dyp = torch.zeros(M, Np, dtype=dy2.dtype, device=dy2.device)
        dyp[:, :N] = dy2
        dy2 = dyp
    db_fused = None
    want_db = ctx.has_bias and ctx.needs_input_grad[2]
    # the bias gradient rides in the weight-gradient GEMM when that GEMM's kernel builds it for free (cst_gemm_desc.colsum)
    db_in_dw = want_db and ctx.needs_input_grad[1] and Np % 8 == 0 and not _os.environ.get("CST_NO_GEMM_COLSUM") and K.dw_colsum_is_fused(Np, Kd, M, w.dtype)
    may_b = want_db and Np == N and _may_defer(w, ctx.bias_obj)  # the bias gradient's second stage may wait for the flush
    if ctx.drop[0] > 0.0:  # gradient of the dropped branch: the same mask, regenerated
        dy2, db_fused = _drop_grad(dy2, ctx.drop, w.dtype, live, defer=may_b,
                                   with_colsum=not db_in_dw and ctx.act == L.ACT_NONE and want_db and Np == N and N % 8 == 0)
    dz = K.act_bwd(dy2, z, ctx.act) if ctx.act != L.ACT_NONE else dy2
    dx = dw = db = dres = None
    if ctx.needs_input_grad[0]:
        dx = _dx_gemm(dz, w, M, use_wt=_want_wt(M, w), like=x2, resid=_flat2d(dxp) if dxp is not None else None,
                      m_live=live).view(ctx.xshape)
        if live is not None and dxp is None:
            dx = _with_tiles(dx, live)  # a zero row of dz is a zero row of dz W
    if ctx.needs_input_grad[1]:
        dw, db = _dw_gemm(dz, x2, w, ctx.bias_obj, M, db_in_dw=db_in_dw, live=live, dz_travels_on=dz.data_ptr() == dy.data_ptr() and ctx.has_resid,
                          allow_slot=Np == N, allow_defer=Np == N)
        dw = dw[:N]
        if db is not None:
            db = db[:N]
    if want_db and db is None:
        db = db_fused if db_fused is not None else K.colsum(dz, w.dtype, live, defer=may_b)[:N]
    if ctx.has_resid and ctx.needs_input_grad[3]:
        dres = dy
    return dx, dw, db, dres, None, None, None


class _LinearPassFn(torch.autograd.Function):
    """(y, x') = (linear(x), alias of x).  A post-norm block takes x' as its residual: the residual-branch gradient and the
    projection's dX then arrive in ONE backward call and are summed in the dX GEMM's epilogue (same idea as _LayerNormPassFn)."""

    @staticmethod
    def forward(ctx, x, weight, bias, act, drop_p, drop_key):
        y = _LinearFn.forward(ctx, x, weight, bias, None, act, drop_p, drop_key)
        ctx.set_materialize_grads(False)
        return y, x.view_as(x)

    @staticmethod
    def backward(ctx, dy, dxp):
        g = _linear_backward(ctx, dy, dxp)
        return g[0], g[1], g[2], None, None, None


def linear_pass(x, weight, bias=None, act=None, dropout_p=0.0):
    """Returns (linear(x), x') where x' aliases x and must be used for the enclosing block's residual connection."""
    return _LinearPassFn.apply(x, weight, bias, _ACT[act], *_drop_args(dropout_p))


def linear(x, weight, bias=None, act=None, resid=None, dropout_p=0.0):
    """y = dropout(act(x W^T + b)) (+ resid)."""
    return _LinearFn.apply(x, weight, bias, resid, _ACT[act], *_drop_args(dropout_p))


class _FFNFn(torch.autograd.Function):
    """y = W2 act(W1 x + b1) + b2 (+ resid): two GEMMs forward; in backward the activation derivative is the epilogue of
    the dH GEMM (dz1 = (dy W2) * act'(z1)), so no separate act-backward pass over the [tokens, ffn] tensor."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, resid, act, p_act, key_act, p_out, key_out):
        """y = resid + dropout_out(W2 dropout_act(act(W1 x + b1)) + b2): both dropouts are GEMM epilogues."""
        x2 = _flat2d(x)
        M, d = x2.shape
        F_ = w1.shape[0]
        dout = w2.shape[0]
        z1 = torch.empty(M, F_, dtype=x.dtype, device=x.device)
        h = torch.empty_like(z1)
        K.gemm(x2, w1, h, M, F_, d, a_kmajor=1, b_kmajor=1, lda=d, ldb=d, ldc=F_, bias=b1, act=act, aux_out=z1, ld_aux_out=F_, split_k=1,
               drop_p=p_act, drop_key=key_act)
        y = torch.empty(M, dout, dtype=x.dtype, device=x.device)
        r2 = _flat2d(resid) if resid is not None else None
        K.gemm(h, w2, y, M, dout, F_, a_kmajor=1, b_kmajor=1, lda=F_, ldb=F_, ldc=dout, bias=b2, resid=r2, ld_resid=dout, split_k=1,
               drop_p=p_out, drop_key=key_out)
        ctx.save_for_backward(x2, w1, w2, z1, h)
        ctx.cfg = (act, b1 is not None, b2 is not None, resid is not None, x.shape)
        # post-norm block: the residual IS the block input -> its gradient (dy) is added in the dX GEMM's epilogue
        ctx.res_is_x = (resid is not None and resid.data_ptr() == x.data_ptr() and resid.shape == x.shape
                        and resid.stride() == x.stride() and dout == d)
        ctx.drop = (p_act, key_act, p_out, key_out)
        ctx.bias_objs = (b1, b2)
        return y.view(*x.shape[:-1], dout)

    @staticmethod
    def backward(ctx, dy):
        x2, w1, w2, z1, h = ctx.saved_tensors
        act, has_b1, has_b2, has_res, xshape = ctx.cfg
        M, d = x2.shape
        F_, dout = w1.shape[0], w2.shape[0]
        dy2 = _flat2d(dy)
        live = _tiles_of(dy, M)  # zero rows of dy are zero rows of dy2 (mask) and of dz1 (row-wise GEMM, act', mask)
        p_act, key_act, p_out, key_out = ctx.drop
        b1, b2 = ctx.bias_objs
        db2_fused = None
        gcs = not _os.environ.get("CST_NO_GEMM_COLSUM")
        db2_in_dw = gcs and has_b2 and ctx.needs_input_grad[4] and ctx.needs_input_grad[3] and dout % 8 == 0 and K.dw_colsum_is_fused(dout, F_, M, w2.dtype)
        db1_in_dw = gcs and has_b1 and ctx.needs_input_grad[2] and ctx.needs_input_grad[1] and F_ % 8 == 0 and K.dw_colsum_is_fused(F_, d, M, w1.dtype)
        if p_out > 0.0:  # d(fc2 output) = dy * mask_out
            dy2, db2_fused = _drop_grad(dy2, (p_out, key_out), w2.dtype, live, defer=_may_defer(w2, b2),
                                        with_colsum=not db2_in_dw and has_b2 and ctx.needs_input_grad[4] and dout % 8 == 0)
        use_wt = _want_wt(M, w2) and _want_wt(M, w1)  # both dX GEMMs or neither
        dz1 = _dx_gemm(dy2, w2, M, use_wt=use_wt, like=dy2, dact=act, aux_in=z1, drop=(p_act, key_act), m_live=live)
        dx = dw1 = db1 = dw2 = db2 = None
        if ctx.needs_input_grad[3]:
            dw2, db2 = _dw_gemm(dy2, h, w2, b2, M, db_in_dw=db2_in_dw, live=live, dz_travels_on=dy2.data_ptr() == dy.data_ptr() and has_res)
        if has_b2 and ctx.needs_input_grad[4] and db2 is None:
            db2 = db2_fused if db2_fused is not None else K.colsum(dy2, w2.dtype, live, defer=_may_defer(w2, b2))
        if ctx.needs_input_grad[0]:
            dx = _dx_gemm(dz1, w1, M, use_wt=use_wt, like=x2, resid=_flat2d(dy) if ctx.res_is_x else None, m_live=live).view(xshape)
        if ctx.needs_input_grad[1]:
            dw1, db1 = _dw_gemm(dz1, x2, w1, b1, M, db_in_dw=db1_in_dw, live=live, dz_travels_on=False)
        if has_b1 and ctx.needs_input_grad[2] and db1 is None:
            db1 = K.colsum(dz1, w1.dtype, live, defer=_may_defer(w1, b1))
        dres = dy if has_res and ctx.needs_input_grad[5] and not (ctx.res_is_x and ctx.needs_input_grad[0]) else None
        return dx, dw1, db1, dw2, db2, dres, None, None, None, None, None


def ffn(x, w1, b1, w2, b2, act, resid=None, activation_dropout_p=0.0, dropout_p=0.0):
    """Position-wise feed-forward block with fused epilogues (fc1: bias+activation+dropout, fc2: bias+dropout+residual)."""
    assert _ACT[act] != L.ACT_NONE
    return _FFNFn.apply(x, w1.contiguous(), b1, w2.contiguous(), b2, resid, _ACT[act], *_drop_args(activation_dropout_p), *_drop_args(dropout_p))


# ------------------------------------------------------------------------------------------------
# LayerNorm with fused residual add
# ------------------------------------------------------------------------------------------------
class _LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, res, gamma, beta, eps):
        x2 = _flat2d(x)
        r2 = _flat2d(res) if res is not None else None
        y, s, mean, rstd = K.layernorm_fwd(x2, r2, gamma, beta, eps, want_sum=True)
        src = s if res is not None else x2
        ctx.save_for_backward(src, gamma, mean, rstd)
        ctx.has_res = res is not None
        ctx.shape = x.shape
        ctx.set_materialize_grads(False)  # an unused second output must not cost a zero-filled [rows, cols] gradient
        if res is not None:
            return y.view(x.shape), s.view(x.shape)
        return y.view(x.shape), None

    @staticmethod
    def backward(ctx, dy, ds):
        src, gamma, mean, rstd = ctx.saved_tensors
        if dy is None:  # only the sum output was consumed
            return ds, (ds if ctx.has_res else None), None, None, None
        dy2 = _flat2d(dy)
        dres = _flat2d(ds) if ds is not None else None
        dx, dg, db, tiles = K.layernorm_bwd(dy2, src, gamma, mean, rstd, dres, grad_dtype=gamma.dtype, want_tiles=True, defer=_may_defer(gamma))
        dx = _with_tiles(dx.view(ctx.shape), tiles)
        return dx, (dx if ctx.has_res else None), dg, db, None


def layer_norm(x, gamma, beta, eps=1e-5):
    return _LayerNormFn.apply(x, None, gamma, beta, eps)[0]


def add_layer_norm(x, res, gamma, beta, eps=1e-5):
    """s = x + res;  returns (LN(s), s) from one kernel."""
    return _LayerNormFn.apply(x, res, gamma, beta, eps)


class _LayerNormPassFn(torch.autograd.Function):
    """y = LN(x) and x handed back as a second output: a pre-norm block uses the pass-through as its residual, so the
    residual-branch gradient and the LN gradient arrive in ONE backward call and are summed inside cst_layernorm_bwd
    (no separate autograd accumulation kernel per block)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        x2 = _flat2d(x)
        y, _, mean, rstd = K.layernorm_fwd(x2, None, gamma, beta, eps)
        ctx.save_for_backward(x2, gamma, mean, rstd)
        ctx.shape = x.shape
        ctx.set_materialize_grads(False)
        return y.view(x.shape), x.view_as(x)

    @staticmethod
    def backward(ctx, dy, dxp):
        x2, gamma, mean, rstd = ctx.saved_tensors
        dres = _flat2d(dxp) if dxp is not None else None
        if dy is None:
            return (dxp, None, None, None)
        dx, dg, db = K.layernorm_bwd(_flat2d(dy), x2, gamma, mean, rstd, dres, grad_dtype=gamma.dtype, defer=_may_defer(gamma))
        return dx.view(ctx.shape), dg, db, None


def layer_norm_residual(x, gamma, beta, eps=1e-5):
    """Returns (LN(x), x') where x' aliases x and must be used for the block's residual connection."""
    return _LayerNormPassFn.apply(x, gamma, beta, eps)


# ------------------------------------------------------------------------------------------------
# fused attention
# ------------------------------------------------------------------------------------------------
_MASK_CACHE = []  # [(source mask (kept alive), version, uint8 mask, kv_len)] — one padding mask serves every layer of a pass


_PAD_TILES = []  # [(uint8 mask (kept alive), bool [ceil(B*T/64)]: every row of the 64-row tile of the flattened [B*T] rows is padding)]


def _pad_tiles(u8):
    for src, pt in _PAD_TILES:
        if src is u8:
            return pt
    flat = u8.reshape(-1)
    pad = (-flat.numel()) % 64
    if pad:
        flat = torch.cat([flat, torch.ones(pad, dtype=flat.dtype, device=flat.device)])
    pt = flat.view(-1, 64).amin(dim=1) > 0
    _PAD_TILES.append((u8, pt))
    if len(_PAD_TILES) > 8:
        _PAD_TILES.pop(0)
    return pt


def _mask_and_len(key_padding_mask):
    """(uint8 [B,Tk] mask, int32 [B] kv_len) of a key padding mask; kv_len[b] = 1 + index of the last real key, so that the
    kernels skip the all-padding key tiles at the end of every utterance of a length-sorted batch (cst_attn_desc.kv_len)."""
    if key_padding_mask is None:
        return None, None
    if _os.environ.get("CST_ATTN_NO_KVLEN"):  # test hook: walk every key tile (results are bit-identical either way)
        return key_padding_mask.to(torch.uint8).contiguous(), None
    for src, ver, u8, kvl in _MASK_CACHE:
        if src is key_padding_mask and ver == key_padding_mask._version:
            return u8, kvl
    u8 = key_padding_mask.to(torch.uint8).contiguous()
    Tk = u8.shape[1]
    pos = torch.arange(1, Tk + 1, device=u8.device, dtype=torch.int32)
    kvl = (pos * (u8 == 0)).amax(dim=1).to(torch.int32).contiguous()
    _MASK_CACHE.append((key_padding_mask, key_padding_mask._version, u8, kvl))
    if len(_MASK_CACHE) > 8:
        _MASK_CACHE.pop(0)
    return u8, kvl


def _laid_out_like(do, o):
    """The incoming gradient of an attention output, copied into o's strides where autograd delivers it in others."""
    if do.stride() == o.stride():
        return do
    tmp = torch.empty_like(o)
    tmp.copy_(do)
    return tmp


class _AttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, kpm, kvl, H, causal, scale, layout_q, layout_kv, drop_p, drop_key):
        D = q.shape[-1] // H
        o, lse = K.attn_fwd(q, k, v, H, D, kpm, causal, scale, layout_q, layout_kv, drop_p, drop_key, kvl)
        ctx.save_for_backward(q, k, v, o, lse, kpm, kvl)
        ctx.cfg = (H, D, causal, scale, layout_q, layout_kv, drop_p, drop_key)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse, kpm, kvl = ctx.saved_tensors
        H, D, causal, scale, lq, lkv, drop_p, drop_key = ctx.cfg
        dq, dk, dv = K.attn_bwd(_laid_out_like(do, o), q, k, v, o, lse, H, D, kpm, causal, scale, lq, lkv, drop_p, drop_key, kvl)
        return dq, dk, dv, None, None, None, None, None, None, None, None, None


class _AttnKVFn(torch.autograd.Function):
    """Attention whose keys and values are the two channel halves of ONE projection kv [B, Tk, 2C] (cross-attention / memory
    attention: k_proj and v_proj read the same rows, so they run as one [2C, C] GEMM).  The backward writes dk | dv into one buffer:
    the projection's dX and dW are single GEMMs and the key/value rows receive a single gradient (no autograd sum of two)."""

    @staticmethod
    def forward(ctx, q, kv, kpm, kvl, H, scale, drop_p, drop_key):
        C = kv.shape[-1] // 2
        D = C // H
        k, v = kv[..., :C], kv[..., C:]
        o, lse = K.attn_fwd(q, k, v, H, D, kpm, False, scale, "bt", "bt", drop_p, drop_key, kvl)
        ctx.save_for_backward(q, kv, o, lse, kpm, kvl)
        ctx.cfg = (H, D, C, scale, drop_p, drop_key)
        return o

    @staticmethod
    def backward(ctx, do):
        q, kv, o, lse, kpm, kvl = ctx.saved_tensors
        H, D, C, scale, drop_p, drop_key = ctx.cfg
        dq, dkv = torch.empty_like(q), torch.empty_like(kv)
        K.attn_bwd(_laid_out_like(do, o), q, kv[..., :C], kv[..., C:], o, lse, H, D, kpm, False, scale, "bt", "bt", drop_p, drop_key, kvl,
                   grads=(dq, dkv[..., :C], dkv[..., C:]))
        return dq, dkv, None, None, None, None, None, None


def attention_kv(q, kv, num_heads, key_padding_mask=None, scale=None, dropout_p=0.0):
    """q [B,Tq,C], kv [B,Tk,2C] (k | v along channels, contiguous) -> [B,Tq,C]; non-causal."""
    C = q.shape[-1]
    if scale is None:
        scale = (C // num_heads) ** -0.5
    key_padding_mask, kv_len = _mask_and_len(key_padding_mask)
    assert q.stride(-1) == 1 and kv.is_contiguous() and kv.shape[-1] == 2 * C
    return _AttnKVFn.apply(q, kv, key_padding_mask, kv_len, num_heads, float(scale), *_drop_args(dropout_p))


def _drop_args(dropout_p):
    """(p, key) of one dropout site: a fresh key of the process-wide stream when p > 0."""
    if dropout_p and dropout_p > 0.0:
        from . import rng
        return float(dropout_p), rng.next_key()
    return 0.0, 0


def attention(q, k, v, num_heads, key_padding_mask=None, causal=False, scale=None, layout_q="bt", layout_kv="bt", dropout_p=0.0):
    """q [B,Tq,C] / k,v [B,Tk,C] (layout "bt") or time-major ("tb"); channels of head h at [h*D,(h+1)*D).
    key_padding_mask: bool/uint8 [B,Tk], True = pad.  dropout_p > 0: attention-probability dropout inside the kernels."""
    if scale is None:
        scale = (q.shape[-1] // num_heads) ** -0.5
    key_padding_mask, kv_len = _mask_and_len(key_padding_mask)
    assert q.stride(-1) == 1 and k.stride(-1) == 1 and v.stride(-1) == 1
    return _AttnFn.apply(q, k, v, key_padding_mask, kv_len, num_heads, bool(causal), float(scale), layout_q, layout_kv,
                         *_drop_args(dropout_p))


def attention_avg_probs(q, k, num_heads, key_padding_mask=None, scale=None):
    """The head-averaged attention probabilities fp32 [B, Tq, Tk] of q [B,Tq,C] over k [B,Tk,C] (k may be a channel slice of a packed
    projection) — what the reference's MultiheadAttention returns as its second value (multihead_attention.py:352-362).  No gradient:
    inference only (the fused kernels of attention() never materialise the probabilities; this is a kernel of its own)."""
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad):
        raise NotImplementedError("attention weights are computed under torch.no_grad() only")
    if scale is None:
        scale = (q.shape[-1] // num_heads) ** -0.5
    if key_padding_mask is not None and key_padding_mask.dim() == 0:
        key_padding_mask = None
    return K.attn_avg_probs(q, k, num_heads, key_padding_mask, float(scale))


class _AttnPackedFn(torch.autograd.Function):
    """Self-attention on a packed projection qkv [B, T, 3C] (q | k | v along channels).  The backward writes dq/dk/dv
    into ONE [B, T, 3C] buffer, so the projection's dX / dW are single GEMMs and x receives a single gradient."""

    @staticmethod
    def forward(ctx, qkv, kpm, kvl, H, causal, scale, drop_p, drop_key, pad_tiles=None, seq=None):
        ctx.pad_tiles = pad_tiles
        C = qkv.shape[-1] // 3
        D = C // H
        q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
        B, T = qkv.shape[0], qkv.shape[1]
        o = torch.empty(B, T, C, dtype=qkv.dtype, device=qkv.device)
        # packed sequences: lse / delta are [sequences, H, longest sequence]
        lse = torch.empty((seq[0].numel() - 1) if seq is not None else B, H, int(seq[1]) if seq is not None else T, dtype=torch.float32, device=qkv.device)
        d = K.attn_desc(q, k, v, o, lse, H, D, kpm, causal, scale, "bt", "bt", drop_p, drop_key, kvl, seq)
        K.attn_fwd_desc(d)
        ctx.save_for_backward(qkv, o, lse, kpm, kvl, seq[0] if seq is not None else None)
        ctx.cfg = (H, D, C, causal, scale, drop_p, drop_key, int(seq[1]) if seq is not None else None)
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse, kpm, kvl, seq_off = ctx.saved_tensors
        H, D, C, causal, scale, drop_p, drop_key, seq_max = ctx.cfg
        seq = (seq_off, seq_max) if seq_off is not None else None
        live = _tiles_of(do, qkv.shape[0] * qkv.shape[1]) if ctx.pad_tiles is not None else None
        if not do.is_contiguous():
            do = do.contiguous()
        dqkv = torch.empty_like(qkv)
        K.attn_bwd(do, qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], o, lse, H, D, kpm, causal, scale, "bt", "bt", drop_p, drop_key, kvl, seq,
                   grads=(dqkv[..., :C], dqkv[..., C:2 * C], dqkv[..., 2 * C:]))
        if live is not None:
            # row t of dq|dk|dv is exactly zero when dO_t is (dS_t. = P_t. * 0) AND key t is padding (P_.t = 0): a 64-row tile
            # that is dead in dO and all padding is dead here; every other tile is declared live
            stamps = torch.where(ctx.pad_tiles, live[0], torch.full_like(live[0], live[1] if live[1] < 2 ** 31 else live[1] - 2 ** 32))
            dqkv = _with_tiles(dqkv, (stamps, live[1]))
        return dqkv, None, None, None, None, None, None, None, None, None


def attention_packed(qkv, num_heads, key_padding_mask=None, causal=False, scale=None, dropout_p=0.0, seq=None):
    """qkv [B, T, 3C] contiguous -> [B, T, C].
    seq = PackedRows (see pack_rows): qkv is [1, rows, 3C] holding variable-length sequences back to back; sequence b attends to its
    first seq.kv_len[b] rows (its real frames); key_padding_mask must be None."""
    C = qkv.shape[-1] // 3
    if scale is None:
        scale = (C // num_heads) ** -0.5
    assert qkv.is_contiguous()
    if seq is not None:
        assert key_padding_mask is None and qkv.shape[0] == 1 and qkv.shape[1] == seq.rows
        return _AttnPackedFn.apply(qkv, None, seq.kv_len, num_heads, bool(causal), float(scale), *_drop_args(dropout_p), None, (seq.offsets, seq.longest))
    key_padding_mask, kv_len = _mask_and_len(key_padding_mask)
    pad_tiles = _pad_tiles(key_padding_mask) if (key_padding_mask is not None and qkv.requires_grad) else None
    return _AttnPackedFn.apply(qkv, key_padding_mask, kv_len, num_heads, bool(causal), float(scale), *_drop_args(dropout_p), pad_tiles)


# ------------------------------------------------------------------------------------------------
# q | k | v parameters as one packed operand
# ------------------------------------------------------------------------------------------------
class _StackedRowsFn(torch.autograd.Function):
    """Parameters that sit back to back in memory (optim.FlatParamBuffers lays the q, k, v projections of an attention module out
    that way) seen as ONE [n C, ...] tensor: a view, no copy.  backward hands each parameter its row block of the packed gradient
    (views of the one tensor the dW GEMM wrote)."""

    @staticmethod
    def forward(ctx, *ts):
        a = ts[0]
        ctx.rows, ctx.n = a.shape[0], len(ts)
        return torch.as_strided(a, (len(ts) * a.shape[0],) + tuple(a.shape[1:]), a.stride(), a.storage_offset())

    @staticmethod
    def backward(ctx, g):
        r = ctx.rows
        return tuple(g[i * r:(i + 1) * r] for i in range(ctx.n))


def stacked_rows(*ts):
    """cat(ts, 0) for two or three equal-shaped parameters (q | k | v, or k | v); free when they are adjacent in memory."""
    a = ts[0]
    n = a.numel() * a.element_size()
    if (not _os.environ.get("CST_NO_QKV_VIEW") and all(t.shape == a.shape and t.is_contiguous() for t in ts)
            and all(ts[i].data_ptr() + n == ts[i + 1].data_ptr() for i in range(len(ts) - 1))
            and a.untyped_storage().data_ptr() == ts[-1].untyped_storage().data_ptr()):
        K.STATS["qkv_view"] = K.STATS.get("qkv_view", 0) + 1
        out = _StackedRowsFn.apply(*ts)
        out._cst_parts = tuple(t.detach() for t in ts)  # version counters of all of them (WEIGHT_TRANSPOSES, _wversion)
        out._cst_parts_params = tuple(ts)               # ... and the parameters themselves (optim.grad_slot)
        return out
    return torch.cat(ts, 0)


# ------------------------------------------------------------------------------------------------
# packed (padding-free) row sets — include/cst.h: cst_rows_pack / cst_rows_unpack
# ------------------------------------------------------------------------------------------------
class PackedRows:
    """Where the sequences of a packed [rows, C] tensor live: offsets int32 [B+1] (device), kv_len int32 [B] (device: real frames per
    sequence = its keys), rows (total), longest (longest sequence), B, T (the padded shape it came from)."""

    def __init__(self, offsets, kv_len, rows, longest, B, T, host_lens=None):
        self.offsets, self.kv_len, self.rows, self.longest, self.B, self.T = offsets, kv_len, rows, longest, B, T
        self.host_lens = host_lens  # real frames per sequence as host integers (read with the plan's one host transfer)
        self.kept_host = None       # rows each sequence keeps (offsets[b + 1] - offsets[b]) as host integers, where the planner knows them


def plan_packed_rows(padding_mask, margin):
    """padding_mask bool [B, T] (True = padding, a suffix per row).  Sequence b keeps n_b = min(T, len_b + margin + 1) rows: its real
    frames, the `margin` padding frames that are still influenced by real ones, and ONE more that stands for every identical
    padding frame behind it.  One host read of B integers (the plan sizes the packed allocations)."""
    B, T = padding_mask.shape
    lens = (~padding_mask).sum(dim=1).to(torch.int32)
    n = torch.clamp(lens + (margin + 1), max=T)
    off = torch.zeros(B + 1, dtype=torch.int32, device=padding_mask.device)
    off[1:] = torch.cumsum(n, 0)
    host = torch.cat((off[-1:], n.max().view(1), lens)).tolist()  # the step's packing plan: total rows, longest sequence, lengths
    plan = PackedRows(off.contiguous(), lens.contiguous(), int(host[0]), int(host[1]), B, T, [int(v) for v in host[2:]])
    plan.kept_host = [min(T, v + margin + 1) for v in plan.host_lens]
    return plan


def plan_from_lengths(lens_dev, host_lens, T):
    """The plan of a later stage whose sequence lengths follow from an earlier plan's by host arithmetic (the subsampled frames
    behind wav2vec2): device offsets by device ops, the allocation sizes from the host copies — no further host read.  Sequence b
    keeps exactly its lens[b] real rows."""
    B = lens_dev.numel()
    n = torch.clamp(lens_dev.to(torch.int32), max=T)
    off = torch.zeros(B + 1, dtype=torch.int32, device=lens_dev.device)
    off[1:] = torch.cumsum(n, 0)
    hl = [min(int(v), T) for v in host_lens]
    return PackedRows(off.contiguous(), n.contiguous(), sum(hl), max(hl), B, T, hl)


class _PackRowsFn(torch.autograd.Function):
    """[B, T, C] -> [1, rows, C]: the rows each sequence keeps; backward = unpack with zeros behind the kept rows."""

    @staticmethod
    def forward(ctx, x, seq):
        ctx.seq = seq
        return K.rows_pack(x.contiguous(), seq.offsets, seq.rows, tail_sum=False).unsqueeze(0)

    @staticmethod
    def backward(ctx, dy):
        s = ctx.seq
        dy2 = dy.reshape(s.rows, dy.shape[-1])
        return K.rows_unpack(dy2.contiguous(), s.offsets, s.B, s.T, tail_broadcast=False), None


class _UnpackRowsFn(torch.autograd.Function):
    """[1, rows, C] -> [B, T, C]: rows behind a sequence's kept ones repeat its last kept row (they are identical padding frames);
    backward = pack with the gradients of those copies summed into that row, in index order."""

    @staticmethod
    def forward(ctx, y, seq, broadcast):
        ctx.seq, ctx.broadcast = seq, broadcast
        y2 = y.reshape(seq.rows, y.shape[-1])
        return K.rows_unpack(y2.contiguous(), seq.offsets, seq.B, seq.T, tail_broadcast=broadcast)

    @staticmethod
    def backward(ctx, dx):
        s = ctx.seq
        return K.rows_pack(dx.contiguous(), s.offsets, s.rows, tail_sum=ctx.broadcast).unsqueeze(0), None, None


def pack_rows(x, seq):
    return _PackRowsFn.apply(x, seq)


def unpack_rows(y, seq, broadcast=True):
    """broadcast=False: the rows behind a sequence's kept ones come back as zeros (nobody reads them) and their gradient is dropped."""
    return _UnpackRowsFn.apply(y, seq, bool(broadcast))


# ------------------------------------------------------------------------------------------------
# wav2vec2 conv layer 0 + GroupNorm + GELU
# ------------------------------------------------------------------------------------------------
def no_mlen():
    """CST_NO_MLEN (A/B switch of the tests, read per call): the frame limits are off, every conv computes the frames past each
    utterance's end as well.  Same bits."""
    return bool(_os.environ.get("CST_NO_MLEN"))


def _conv0_args(wav, w, write_limit, grad_limit):
    """-> (fp32 contiguous wav, w as [C, k], k, the frame limits) of the two layer-0 Functions."""
    C, _, k = w.shape
    if no_mlen() or _os.environ.get("CST_GEMM_NO_KLIVE"):
        write_limit = grad_limit = None  # (with the GEMM-side skipping off, every frame of this layer is read)
    return wav.float().contiguous(), w.reshape(C, k).contiguous(), k, write_limit, grad_limit


class _Conv0Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, wav, w, gamma, beta, stride, eps, write_limit, grad_limit):
        wav, w2, k, write_limit, grad_limit = _conv0_args(wav, w, write_limit, grad_limit)
        y, mean, rstd, gram = K.conv0_fwd(wav, w2, gamma, beta, k, stride, eps, frame_limit=write_limit)
        ctx.save_for_backward(wav, w2, gamma, beta, mean, rstd, gram)
        ctx.k, ctx.stride, ctx.grad_limit = k, stride, grad_limit
        return y

    @staticmethod
    def backward(ctx, dy):
        wav, w2, gamma, beta, mean, rstd, gram = ctx.saved_tensors
        dw, dg, db = K.conv0_bwd(dy.contiguous(), wav, w2, gamma, beta, mean, rstd, gram, ctx.k, ctx.stride, frame_limit=ctx.grad_limit)
        return None, dw.view(w2.shape[0], 1, ctx.k).to(w2.dtype), dg.to(gamma.dtype), db.to(gamma.dtype), None, None, None, None


def conv0_gn_gelu(wav, weight, gn_weight, gn_bias, stride, eps=1e-5, write_limit=None, grad_limit=None):
    """wav [B,S] -> channels-last [B, L, C] = GELU(GroupNorm_C(conv1d(wav, weight[C,1,k], stride))).
    write_limit / grad_limit (int32 [B], cst_conv_row_limits rows [0][1] / [0][0]): frames nobody reads are not written, frames whose
    gradient is exactly zero are not read in backward."""
    return _Conv0Fn.apply(wav, weight, gn_weight, gn_bias, stride, eps, write_limit, grad_limit)


# ------------------------------------------------------------------------------------------------
# the feature extractor in extractor_mode="layer_norm": conv (+ bias) -> LayerNorm over channels -> GELU in every layer
# ------------------------------------------------------------------------------------------------
class _Conv0LnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, wav, w, bias, gamma, beta, stride, eps, write_limit, grad_limit):
        wav, w2, k, write_limit, grad_limit = _conv0_args(wav, w, write_limit, grad_limit)
        y, mean, rstd = K.conv0_ln_fwd(wav, w2, bias, gamma, beta, k, stride, eps, frame_limit=write_limit)
        ctx.save_for_backward(wav, w2, bias, gamma, beta, mean, rstd)
        ctx.k, ctx.stride, ctx.grad_limit = k, stride, grad_limit
        return y

    @staticmethod
    def backward(ctx, dy):
        wav, w2, bias, gamma, beta, mean, rstd = ctx.saved_tensors
        dw, dbi, dg, db = K.conv0_ln_bwd(dy.contiguous(), wav, w2, bias, gamma, beta, mean, rstd, ctx.k, ctx.stride, frame_limit=ctx.grad_limit)
        return (None, dw.view(w2.shape[0], 1, ctx.k).to(w2.dtype), dbi.to(bias.dtype), dg.to(gamma.dtype), db.to(gamma.dtype),
                None, None, None, None)


def conv0_ln_gelu(wav, weight, bias, ln_weight, ln_bias, stride, eps=1e-5, write_limit=None, grad_limit=None):
    """wav [B,S] -> channels-last [B, L, C] = GELU(LayerNorm_C(conv1d(wav, weight[C,1,k], stride) + bias)), one pass
    (cst_conv0_ln_gelu_fwd / _bwd).  write_limit / grad_limit as in conv0_gn_gelu."""
    return _Conv0LnFn.apply(wav, weight, bias, ln_weight, ln_bias, stride, eps, write_limit, grad_limit)


class _LnGeluFn(torch.autograd.Function):
    """y = GELU(LayerNorm_C(u)) over channels-last rows [B, L, C].  `conv_bias` (optional) is the bias the conv GEMM in front added to
    u: its gradient is the column sum of du, which the backward kernel accumulates on its way (the conv is then called with a
    detached bias and needs no column-sum pass of its own)."""

    @staticmethod
    def forward(ctx, u, gamma, beta, conv_bias, eps, row_limit):
        if no_mlen():
            row_limit = None
        u = u.contiguous()
        y, mean, rstd = K.ln_gelu_fwd(u, gamma, beta, eps, row_limit)
        ctx.save_for_backward(u, gamma, beta, mean, rstd)
        ctx.row_limit = row_limit
        ctx.bias_dtype = conv_bias.dtype if conv_bias is not None else None
        return y

    @staticmethod
    def backward(ctx, dy):
        u, gamma, beta, mean, rstd = ctx.saved_tensors
        want_bias = ctx.bias_dtype is not None and ctx.needs_input_grad[3]
        du, dg, db, dc = K.ln_gelu_bwd(dy.contiguous(), u, gamma, beta, mean, rstd, ctx.row_limit,
                                       want_colsum=want_bias, padded=True)
        return du, dg.to(gamma.dtype), db.to(gamma.dtype), (dc.to(ctx.bias_dtype) if want_bias else None), None, None


def ln_gelu(u, ln_weight, ln_bias, conv_bias=None, eps=1e-5, row_limit=None):
    """GELU(LayerNorm over the last axis) of u [B, L, C] (cst_ln_gelu_fwd / _bwd).  row_limit (int32 [B]): rows t >= row_limit[b] are
    read by nobody and carry exactly zero gradient (cst_conv_row_limits): they are skipped and come back as zeros."""
    return _LnGeluFn.apply(u, ln_weight, ln_bias, conv_bias, eps, row_limit)


# ------------------------------------------------------------------------------------------------
# channels-last conv1d as implicit GEMM (wav2vec2 conv layers 1.., subsampler)
# ------------------------------------------------------------------------------------------------
def _padded_base(t, L, C):
    """If `t` [B, L, C] is the interior view of a [B, L+2, C] allocation (one spare row before and after every utterance),
    return that allocation as a tensor, else None."""
    if t.dim() == 3 and t.stride(2) == 1 and t.stride(1) == C and t.stride(0) == (L + 2) * C and t.storage_offset() >= C:
        return torch.as_strided(t, (t.shape[0], L + 2, C), t.stride(), t.storage_offset() - C)
    return None


def _row_padded(B, L, C, dtype, device, zero_edges):
    """-> (allocation [B, L+2, C], its interior view [B, L, C], uninitialised): the layout _padded_base recognises.  zero_edges: the
    spare row before and the one after every utterance are zero-filled (the windowed dX GEMMs read them at utterance boundaries)."""
    full = torch.empty(B, L + 2, C, dtype=dtype, device=device)
    if zero_edges:
        full[:, 0].zero_()
        full[:, L + 1].zero_()
    return full, full[:, 1:1 + L]


def _zero_edged(shape, dim, at, src):
    """An uninitialised tensor of `shape` whose rows [at, at + n) along `dim` are `src` (n rows there) and whose rows before and
    behind them are zero: only those edge rows are zero-filled, not the whole buffer."""
    n = src.shape[dim]
    out = torch.empty(shape, dtype=src.dtype, device=src.device)
    out.narrow(dim, 0, at).zero_()
    out.narrow(dim, at + n, shape[dim] - at - n).zero_()
    out.narrow(dim, at, n).copy_(src)
    return out


class _Conv1dCLFn(torch.autograd.Function):
    """Channels-last conv1d as implicit GEMMs.
    forward : y[b,t,:] = act(W . x[b, t*s : t*s+k, :])            one GEMM, A rows overlap (lda = s*Cin < K = k*Cin)
    dW      : per-utterance [Cout, k*Cin] partials (both operands mn-major, B rows overlap), summed over the batch
    dX      : pad == 0 and k <= s + 1 (the wav2vec2 CNN): for every residue r of l mod s one GEMM
                 dx[b, s*u + r, :] = sum_i dz[b, u - i, :] . W[:, :, r + s*i]
              whose A rows are again overlapping windows of the (row-padded) dz and whose C rows are written with ldc = s*Cin
              straight into dx — no [B, Lout, k*Cin] column buffer and no col2im pass; GELU'(prev_z) is the epilogue.
              (k <= s + 1: i <= 1, and s*u + r < Lin <= s*(Lout - 1) + k + s - 1 gives u <= Lout: dz rows -1 .. Lout, one spare row each side.)
              otherwise (padded subsampler convs): column-gradient GEMM + cst_col2im1d.
    Layers whose incoming gradient is already d/dz (grad_is_dz) keep y / z / dx in a [B, L+2, C] allocation (_row_padded: interior
    views) so the zero rows the dX windows need at utterance boundaries exist without copying."""

    @staticmethod
    def forward(ctx, x, w_cl, bias, k, stride, pad, act, prev_z, grad_is_dz, nz_out=None, nz_in=None, unread_ok=False):
        if no_mlen():
            nz_in = None
            fwd_len = None
        else:
            # (with a bias the rows of a skipped tile hold act(bias), not 0: only where the caller states that nobody reads them)
            fwd_len = nz_out if (bias is None or unread_ok) else None
        ctx.nz_out = nz_out  # int32 [B]: the incoming gradient's rows t >= nz_out[b] are exactly zero (frames past the utterance's end)
        ctx.nz_in = nz_in    # int32 [stride, B]: live rows of each residue class of dx (cst_conv_row_limits); dx is zero behind them
        B, Lin, Cin = x.shape
        Cout = w_cl.shape[0]
        if pad:
            xp = _zero_edged((B, Lin + 2 * pad, Cin), 1, pad, x)
        elif x.stride(2) == 1 and x.stride(1) == Cin:
            xp = x  # contiguous or an interior view of a row-padded allocation: only the batch stride differs
        else:
            xp = x.contiguous()
        Lp = Lin + 2 * pad
        Lout = (Lp - k) // stride + 1
        padded_out = bool(grad_is_dz) and act != L.ACT_NONE
        if padded_out:  # (the spare rows of y and z are read by nobody: not zeroed)
            y_full, y = _row_padded(B, Lout, Cout, x.dtype, x.device, zero_edges=False)
            z_full, z = _row_padded(B, Lout, Cout, x.dtype, x.device, zero_edges=False)
        else:
            y_full = y = torch.empty(B, Lout, Cout, dtype=x.dtype, device=x.device)
            z_full = z = torch.empty_like(y) if act != L.ACT_NONE else None
        K.gemm(xp, w_cl, y_full, Lout, Cout, k * Cin, a_kmajor=1, b_kmajor=1, lda=stride * Cin, ldb=k * Cin, ldc=Cout, bias=bias,
               act=act, aux_out=z_full, ld_aux_out=Cout, batch0=B, sa=(xp.stride(0), 0), sc=(y_full.stride(0), 0), split_k=1,
               a_off=0, c_off=Cout if padded_out else 0, m_len=fwd_len)  # frames past an utterance's end: unread, left at act(0) = 0
        ctx.save_for_backward(xp, w_cl, z, prev_z)
        ctx.cfg = (B, Lin, Cin, Cout, k, stride, pad, Lout, act, bias is not None, grad_is_dz)
        ctx.set_materialize_grads(False)  # the pre-activation output never carries a gradient
        if act != L.ACT_NONE:
            ctx.mark_non_differentiable(z)
            return y, z
        return y, None

    @staticmethod
    def backward(ctx, dy, _dz_unused):
        xp, w_cl, z, prev_z = ctx.saved_tensors
        B, Lin, Cin, Cout, k, stride, pad, Lout, act, has_bias, grad_is_dz = ctx.cfg
        windowed = pad == 0 and k <= stride + 1  # every dX window then stays inside the row-padded dz
        need_dx, need_dw, need_db = ctx.needs_input_grad[0], ctx.needs_input_grad[1], has_bias and ctx.needs_input_grad[2]
        dzc, dzp = _conv_dz(dy, z, act, grad_is_dz, windowed)
        dz2 = None
        if (need_dx and not windowed) or need_db:  # dz as [B * Lout, Cout] (a view of dzc; a copy of the interior of a padded dy)
            dz2 = (dzc if dzc is not None else dzp[:, 1:1 + Lout]).reshape(B * Lout, Cout)
        dx = dw = db = None
        if need_dx and windowed:
            dx = _conv_dx_windowed(dzp, w_cl, prev_z, ctx.nz_in, Lin, Cin, k, stride)
        elif need_dx:
            dx = _conv_dx_col2im(dz2, w_cl, prev_z, B, Lin, Lout, Cin, k, stride, pad)
        if need_dw:
            dw = _conv_dw(dzc, dzp, xp, w_cl, ctx.nz_out, Lout, k, stride)
        if need_db:
            db = K.colsum(dz2, w_cl.dtype)
        return dx, dw, db, None, None, None, None, None, None, None, None, None


def _conv_dz(dy, z, act, grad_is_dz, windowed):
    """The gradient at the conv's pre-activation output, as the backward GEMMs of _Conv1dCLFn read it -> (dzc, dzp):
    dzc  contiguous [B, Lout, Cout]; None when dy arrived as the interior of a row-padded allocation and is dz already (no copy)
    dzp  dz in a [B, Lout+2, Cout] allocation with zero spare rows (_row_padded); None when no windowed dX GEMM will read it"""
    B, Lout, Cout = dy.shape
    dzp = _padded_base(dy, Lout, Cout) if (act == L.ACT_NONE or grad_is_dz) else None
    if dzp is not None:
        return None, dzp
    dyc = dy.contiguous()
    dzc = K.act_bwd(dyc, z.contiguous(), act) if (act != L.ACT_NONE and not grad_is_dz) else dyc
    if windowed:
        dzp, interior = _row_padded(B, Lout, Cout, dy.dtype, dy.device, zero_edges=True)
        interior.copy_(dzc)
    return dzc, dzp


def _conv_dx_windowed(dzp, w_cl, prev_z, nz_in, Lin, Cin, k, stride):
    """dx [B, Lin, Cin] (pad == 0, k <= stride + 1) from the row-padded dz [B, Lout+2, Cout]: one windowed GEMM per residue of l mod
    stride with GELU'(prev_z) as its epilogue.  A row-padded prev_z makes dx the interior of a row-padded allocation too."""
    B, Lout, Cout = dzp.shape[0], dzp.shape[1] - 2, dzp.shape[2]
    pz_base = _padded_base(prev_z, Lin, Cin) if prev_z is not None else None
    dx_padded = pz_base is not None
    if dx_padded:
        dx_full, dx = _row_padded(B, Lin, Cin, dzp.dtype, dzp.device, zero_edges=True)
    else:
        dx_full = dx = torch.empty(B, Lin, Cin, dtype=dzp.dtype, device=dzp.device)
        pz_base = prev_z if prev_z is None else prev_z.contiguous()
    w3 = w_cl.view(Cout, k, Cin)
    for r in range(stride):
        n = len(range(r, k, stride))  # taps r, r + s, ...
        U = (Lin - r + stride - 1) // stride
        if n == 0 or U <= 0:
            continue
        # B_r[ci][q*Cout + co] = W[co][ci][r + s*(n-1-q)]   (window position q <-> dz[u - (n-1) + q])
        # (taps r, r + s, ... in reverse order by a strided slice and a flip: indexing with a Python list would build the
        #  index tensor on the host — a pageable copy, i.e. a stream synchronisation in the middle of the backward pass)
        wr = w3[:, r::stride, :].flip(1).permute(2, 1, 0).reshape(Cin, n * Cout).contiguous()
        # rows u with stride * u + r >= nz_in[b] read only dz rows that are exactly zero: their K loop is skipped
        ml = nz_in[r] if nz_in is not None else None
        K.gemm(dzp, wr, dx_full, U, Cin, n * Cout, a_kmajor=1, b_kmajor=1, lda=Cout, ldb=n * Cout, ldc=stride * Cin,
               batch0=B, sa=((Lout + 2) * Cout, 0), sc=(dx_full.stride(0), 0), a_off=(2 - n) * Cout,
               c_off=(Cin if dx_padded else 0) + r * Cin, dact=L.ACT_GELU if prev_z is not None else L.ACT_NONE,
               aux_in=pz_base, ld_aux_in=stride * Cin, split_k=1, m_len=ml)
    return dx


def _conv_dx_col2im(dz2, w_cl, prev_z, B, Lin, Lout, Cin, k, stride, pad):
    """dx [B, Lin, Cin] of any other conv (the padded subsampler convs) from dz2 [B * Lout, Cout]: the column-gradient GEMM and
    cst_col2im1d, which multiplies by GELU'(prev_z) on its way if prev_z is given."""
    Cout = w_cl.shape[0]
    dcol = torch.empty(B * Lout, k * Cin, dtype=dz2.dtype, device=dz2.device)
    K.gemm(dz2, w_cl, dcol, B * Lout, k * Cin, Cout, a_kmajor=1, b_kmajor=0, lda=Cout, ldb=k * Cin, ldc=k * Cin, split_k=1)
    pzc = prev_z if prev_z is None else prev_z.contiguous()
    return K.col2im1d(dcol, pzc, B, Lin, Lout, Cin, k, stride, pad, L.ACT_GELU if prev_z is not None else 0)


def _conv_dw(dzc, dzp, xp, w_cl, nz_out, Lout, k, stride):
    """dW [Cout, k*Cin] in the parameter dtype from dz (dzc, else the interior of the row-padded dzp: _conv_dz) and the saved input xp
    [B, Lp, Cin]: per-utterance partials, summed over the batch.  nz_out (int32 [B] or None): dz rows t >= nz_out[b] are zero."""
    B, Cin, Cout = xp.shape[0], xp.shape[2], w_cl.shape[0]
    dz_rows, dz_bs, dz_off = (dzc, Lout * Cout, 0) if dzc is not None else (dzp, (Lout + 2) * Cout, Cout)
    part = torch.empty(B, Cout, k * Cin, dtype=torch.float32, device=xp.device)
    # one 256 x 256 workgroup per CU: B x tiles workgroups should fill whole rounds of 256 (B = 32, k = 3: 384 = 1.5
    # rounds -> a 2-way split of the frame axis gives 768 = 3 rounds of half the length)
    wgs = B * ((Cout + 255) // 256) * ((k * Cin + 255) // 256)
    rem = wgs % 256
    sk = 2 if (wgs >= 256 and 0 < rem < 192 and Lout >= 2048) else 1
    # the sum over the utterances (and over the K slices) is ONE fixed-order pass of cst_reduce_multi over the fp32 partials,
    # written in the parameter dtype (before: split-K reduce launch + torch sum over the batch + dtype conversion)
    dw = torch.empty(Cout, k * Cin, dtype=w_cl.dtype, device=xp.device)
    K.gemm(dz_rows, xp, part, Cout, k * Cin, Lout, a_kmajor=0, b_kmajor=0, lda=Cout, ldb=stride * Cin, ldc=k * Cin, batch0=B,
           sa=(dz_bs, 0), sb=(xp.stride(0), 0), sc=(Cout * k * Cin, 0), a_off=dz_off, split_k=sk, k_len=nz_out, reduce_to=dw)
    # (not deferred: autograd re-lays this gradient out — permute / reshape back to [Cout, Cin, k] — as soon as it is returned)
    return dw


def conv1d_cl(x, weight, bias, stride, pad=0, act=None, prev_z=None, grad_is_dz=False, nz_out=None, nz_in=None, unread_ok=False):
    """Channels-last conv1d.  x [B,Lin,Cin]; weight [Cout,Cin,k] (torch layout).  Returns (y, z) where z is
    the pre-activation (None without activation).  If `prev_z` (pre-GELU tensor that produced x = GELU(prev_z))
    is given, the returned input-gradient is already multiplied by GELU'(prev_z), i.e. it is d/d prev_z; the
    producing layer must then be built with grad_is_dz=True so it does not apply GELU' a second time
    (see the wav2vec2 feature extractor: one fused col2im+GELU' pass per layer instead of two)."""
    Cout, Cin, k = weight.shape
    w_cl = weight.permute(0, 2, 1).reshape(Cout, k * Cin)
    if not w_cl.is_contiguous():
        w_cl = w_cl.contiguous()
    return _Conv1dCLFn.apply(x, w_cl, bias, k, stride, pad, _ACT[act], prev_z, bool(grad_is_dz), nz_out, nz_in, bool(unread_ok))


# ------------------------------------------------------------------------------------------------
# grouped positional conv of wav2vec2 (k taps, `groups` groups, pad k//2, SamePad, GELU, + residual)
# ------------------------------------------------------------------------------------------------
# the sliding-window kernels (posconv.hip) are built for 48 channels per group and up to 128 taps
_POSCONV_WINDOW_CG, _POSCONV_WINDOW_KMAX = 48, 128


def _posconv_window_route(x_dtype, w_dtype, bias_dtype, cg, k, gemm_forced):
    """bf16 with 48 channels per group (wav2vec2: 768 / 16) and k <= 128 takes the window kernels; everything else, and every call
    while CST_POSCONV_GEMM is set (gemm_forced; read per call: A/B runs and parity tests), the batched implicit GEMM."""
    return (x_dtype == torch.bfloat16 and w_dtype == x_dtype and cg == _POSCONV_WINDOW_CG and k <= _POSCONV_WINDOW_KMAX
            and (bias_dtype is None or bias_dtype == x_dtype) and not gemm_forced)


def _posconv_geometry(B, T, k):
    """-> zero frames in front of an utterance's x (padl) / dz (lp), frames per padded utterance Tp, rows Kr of dW's axis kappa = b Tp + t"""
    padl = k // 2
    Tp = T + k - 1 + (1 if k % 2 == 0 else 0)  # even k: torch pads k//2 both sides, SamePad drops the last output
    return padl, k - 1 - padl, Tp, B * Tp - (k - 1)


def _posconv_limit(lim, offset, T):
    """Frames from lim[b] on are zero, so the windows of output frames >= lim[b] + offset are: cst_gemm_desc.m_len (int32 [B]) or None."""
    return None if lim is None else torch.clamp(lim.to(torch.int32) + offset, max=T).contiguous()


def _posconv_w_fwd(weight, groups):
    """[C, C/g, k] -> [g][co][j][ci]"""
    cg, k = weight.shape[1], weight.shape[2]
    return weight.view(groups, cg, cg, k).permute(0, 1, 3, 2).contiguous()


def _posconv_w_dx(weight, groups):
    """[C, C/g, k] -> the flipped [g][ci][j'][co]:
    dx[m] = dy[m] + sum_j dz[m + padl - j] w_j  = dy[m] + sum_j' dzp[m + j'] wflip[j'],  dzp[(k-1-padl) + t] = dz[t]"""
    cg, k = weight.shape[1], weight.shape[2]
    return weight.view(groups, cg, cg, k).flip(3).permute(0, 2, 3, 1).contiguous()


def _posconv_group_major(v, groups, Tp, at):
    """Channels-last v [B, T, C] -> [G, B, Tp, C/G] with v's frames at rows [at, at + T) and zero rows around them.  Group-major OUTSIDE
    the batch, so that one group's frames of all utterances are one [B * Tp, C/G] matrix (the weight-gradient GEMM runs over it with
    K = every frame of the batch)."""
    B, T, C = v.shape
    cg = C // groups
    return _zero_edged((groups, B, Tp, cg), 2, at, v.view(B, T, groups, cg).permute(2, 0, 1, 3))


def posconv_k_block_stamps(rows, B, Tp, Kr):
    """The live-block stamps of the weight gradient's K axis kappa = b Tp + t (cst_gemm_desc.k_live: 1 = live): dz is zero from frame
    rows[b] of utterance b on, and 64-row block kb is live if it starts inside utterance b's live frames, or runs past Tp into a live
    utterance b + 1.  rows: host integers (list / numpy) -> numpy int32, or a torch tensor -> torch int32 on its device; one rule."""
    import numpy as np
    nkb = (Kr + 63) // 64
    if isinstance(rows, torch.Tensor):
        n, ks = rows.to(torch.int64), torch.arange(nkb, device=rows.device, dtype=torch.int64) * 64
    else:
        n, ks = np.asarray(rows, dtype=np.int64), np.arange(nkb, dtype=np.int64) * 64
    b0 = ks // Tp
    t0 = ks - b0 * Tp
    nxt = (b0 + 1).clip(max=B - 1)
    live = (t0 < n[b0]) | ((t0 + 64 > Tp) & (b0 + 1 < B) & (n[nxt] > 0))
    return live.to(torch.int32) if isinstance(rows, torch.Tensor) else live.astype(np.int32)


def _posconv_k_live(grad_rows, grad_rows_host, B, Tp, Kr):
    """cst_gemm_desc.k_live of the weight-gradient reduction, (stamps, epoch 1), or None.  dz is zero from frame grad_rows[b] of
    utterance b on: the 64-row K blocks of A that lie in those stretches (a third of them at the bench's lengths) are skipped.
    Row kappa = b Tp + t; a block may run from one utterance's tail into the head of the next."""
    if grad_rows is None or _os.environ.get("CST_GEMM_NO_KLIVE"):
        return None
    if grad_rows_host is None:
        return posconv_k_block_stamps(grad_rows, B, Tp, Kr), 1
    # the plan's row counts are host integers already (its one host read): the stamps are a few hundred numbers of
    # numpy arithmetic and ONE asynchronous copy from a pinned buffer instead of a dozen small launches
    st = posconv_k_block_stamps(grad_rows_host, B, Tp, Kr)
    # (a fresh pinned block per call: torch's host allocator does not hand it out again before the copy has run, which
    #  a buffer kept here could not promise across the micro-batches of an accumulated update)
    return torch.from_numpy(st).pin_memory().to(grad_rows.device, non_blocking=True), 1


class _PosConvWindowFn(torch.autograd.Function):
    """x + GELU(conv(x) + bias) by the sliding-window kernels of posconv.hip, which read x / dz in their channels-last layout, keep a
    workgroup's frame window in LDS and write dw in the parameter's layout — no staging tensors."""

    @staticmethod
    def forward(ctx, x, weight, bias, groups, lens, grad_rows, grad_rows_host):
        B, T, C = x.shape
        padl = _posconv_geometry(B, T, weight.shape[2])[0]
        ml = _posconv_limit(lens, padl, T)
        xc = x.contiguous()
        y, z = K.posconv_fwd(xc, _posconv_w_fwd(weight, groups), bias, groups, ml)
        ctx.save_for_backward(xc, weight, z)
        ctx.groups, ctx.grad_rows, ctx.grad_rows_host = groups, grad_rows, grad_rows_host
        return y

    @staticmethod
    def backward(ctx, dy):
        xc, weight, z = ctx.saved_tensors
        B, T, C = xc.shape
        k, groups = weight.shape[2], ctx.groups
        padl, lp, Tp, Kr = _posconv_geometry(B, T, k)
        dy = dy.contiguous()
        dz = K.act_bwd(dy, z, L.ACT_GELU)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            wflip = _posconv_w_dx(weight, groups)
            ml = _posconv_limit(ctx.grad_rows, lp, T)  # (dead tiles: dx = 0 + dy = dy, exactly)
            dx = K.posconv_dx(dz, wflip, dy, groups, ml)
        if ctx.needs_input_grad[1]:
            # the GEMM route's sums in the same order (_PosConvGemmFn.backward), from the channels-last dz and the saved channels-last
            # input, written as [C, C/g, k] in the parameter's dtype; db: as there
            if ctx.needs_input_grad[2] and not _os.environ.get("CST_NO_GEMM_COLSUM"):
                db = torch.empty(C, dtype=dy.dtype, device=dy.device)
            dw = K.posconv_dw(dz, xc, groups, k, db, _posconv_k_live(ctx.grad_rows, ctx.grad_rows_host, B, Tp, Kr))
        if ctx.needs_input_grad[2] and db is None:
            db = K.colsum(dz.view(B * T, C), weight.dtype)
        return dx, dw, db, None, None, None, None


class _PosConvGemmFn(torch.autograd.Function):
    """x + GELU(conv(x) + bias) as a batched implicit GEMM.  The input is re-staged GROUP-MAJOR ([G, B, T+k, C/G]: a permuting copy
    of x plus two zero fills, and the same again for dz in the backward pass — 136 us of copies and 22 us of fills per call at B=32,
    profiles/posconv_before.txt) so that for one (utterance, group) the im2col row of frame t is the contiguous window starting at
    frame t: a plain k-major operand with lda = C/G < K (overlapping rows) — no segmented addressing in the inner loop."""

    @staticmethod
    def forward(ctx, x, weight, bias, groups, lens, grad_rows, grad_rows_host):
        B, T, C = x.shape
        k = weight.shape[2]
        cg = C // groups
        padl, lp, Tp, Kr = _posconv_geometry(B, T, k)
        ml = _posconv_limit(lens, padl, T)
        xg = _posconv_group_major(x, groups, Tp, padl)
        wg = _posconv_w_fwd(weight, groups)
        y = torch.empty(B, T, C, dtype=x.dtype, device=x.device)
        z = torch.empty_like(y)
        xc = x.contiguous()
        K.gemm(xg, wg, y, T, cg, k * cg, a_kmajor=1, b_kmajor=1, lda=cg, ldb=k * cg, ldc=C, batch0=B, batch1=groups,
               sa=(Tp * cg, B * Tp * cg), sb=(0, cg * k * cg), sc=(T * C, cg), bias=bias, sbias=(0, cg), act=L.ACT_GELU,
               aux_out=z, ld_aux_out=C, resid=xc, ld_resid=C, split_k=1, m_len=ml)
        ctx.save_for_backward(xg, weight, z)
        ctx.grad_rows, ctx.grad_rows_host = grad_rows, grad_rows_host
        return y

    @staticmethod
    def backward(ctx, dy):
        xg, weight, z = ctx.saved_tensors
        groups, B, _, cg = xg.shape
        T, C, k = dy.shape[1], dy.shape[2], weight.shape[2]
        padl, lp, Tp, Kr = _posconv_geometry(B, T, k)
        dy = dy.contiguous()
        dz = K.act_bwd(dy, z, L.ACT_GELU)
        dx = dw = db = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            # dzg[g, b, lp + t] = dz[b, t, group g], zero rows around it, in the frame stride Tp of xg: the operand of BOTH gradient GEMMs
            dzg = _posconv_group_major(dz, groups, Tp, lp)
        if ctx.needs_input_grad[0]:
            wflip = _posconv_w_dx(weight, groups)
            ml = _posconv_limit(ctx.grad_rows, lp, T)  # (dead tiles: dx = 0 + dy = dy, exactly)
            dx = torch.empty(B, T, C, dtype=dy.dtype, device=dy.device)
            K.gemm(dzg, wflip, dx, T, cg, k * cg, a_kmajor=1, b_kmajor=1, lda=cg, ldb=k * cg, ldc=C, batch0=B, batch1=groups,
                   sa=(Tp * cg, B * Tp * cg), sb=(0, cg * k * cg), sc=(T * C, cg), resid=dy, ld_resid=C, split_k=1, m_len=ml)
        if ctx.needs_input_grad[1]:
            # dw[g][co][(j,ci)] = sum_{b,t} dz[b, t, g, co] xg[g, b, t + j, ci]: ONE reduction over the frames of the whole batch per
            # group.  Row kappa = b Tp + t of A is dzg's row kappa + lp (zero for t >= T: the windows that would run from one
            # utterance into the next contribute nothing); row kappa of B is the k-frame window of xg starting at frame kappa
            # (overlapping mn-major rows, ldb = cg).  (Before: one [cg, k cg] product per (utterance, group) — 600 MB of fp32
            # partial sums written and read back by a sum over the batch.)
            if ctx.needs_input_grad[2] and not _os.environ.get("CST_NO_GEMM_COLSUM"):
                # the bias gradient = column sums of this GEMM's A operand (every dz row is inside its K range, the rest are zeros):
                # [groups][cg] = channel order (cst_gemm_desc.colsum)
                db = torch.empty(C, dtype=dy.dtype, device=dy.device)
            dwg = torch.empty(groups, cg, k * cg, dtype=torch.float32, device=dy.device)
            K.gemm(dzg, xg, dwg, cg, k * cg, Kr, a_kmajor=0, b_kmajor=0, lda=cg, ldb=cg, ldc=k * cg, batch0=1, batch1=groups,
                   sa=(0, B * Tp * cg), sb=(0, B * Tp * cg), sc=(0, cg * k * cg), a_off=lp * cg, split_k=1, colsum=db,
                   k_live=_posconv_k_live(ctx.grad_rows, ctx.grad_rows_host, B, Tp, Kr))
            dw = dwg.view(groups, cg, k, cg).permute(0, 1, 3, 2).reshape(C, cg, k).to(weight.dtype)
            if db is not None:
                db = db.to(weight.dtype)
        if ctx.needs_input_grad[2] and db is None:
            db = K.colsum(dz.view(B * T, C), weight.dtype)
        return dx, dw, db, None, None, None, None


class _WeightNormFn(torch.autograd.Function):
    """nn.utils.weight_norm(conv, dim=2) (wav2vec2.py:773-779): w = v * g / ||v||, norms over all dims but the last."""

    @staticmethod
    def forward(ctx, v, g):
        vc, gc = v.contiguous(), g.reshape(-1).contiguous()
        w, norm = K.weight_norm_fwd(vc, gc)
        ctx.save_for_backward(vc, gc, norm)
        ctx.gshape = g.shape
        return w

    @staticmethod
    def backward(ctx, dw):
        vc, gc, norm = ctx.saved_tensors
        dv, dg = K.weight_norm_bwd(vc, gc, dw.contiguous(), norm)
        return dv, dg.view(ctx.gshape)


def weight_norm_last_dim(v, g):
    return _WeightNormFn.apply(v, g)


def pos_conv_gelu_residual(x, weight, bias, groups, lens=None, grad_rows=None, grad_rows_host=None):
    """x [B,T,C]; weight [C, C/g, k] -> x + GELU(conv(x) + bias)   (one fused launch on either route).
    lens (int32 [B], device): frames of x from lens[b] on are ZERO (wav2vec2.py:820-821 zeroes the padding in front of this
    convolution).  The window of output frame t >= lens[b] + k // 2 then holds nothing but zeros, so its row of the implicit
    GEMM's A operand is zero: cst_gemm_desc.m_len = lens + k // 2 lets the tiles behind it skip their K loop, and their epilogue
    on zero accumulators — GELU(bias) + x — IS the value of those frames: every output frame keeps its bits.
    grad_rows (int32 [B], device): the gradient of the output is exactly zero from frame grad_rows[b] on (the rows a packing plan
    keeps: pack_rows' backward writes zeros behind them); the windows of dx frames >= grad_rows[b] + k - 1 - k // 2 are zero.
    Two routes with the same bits, one Function each."""
    window = _posconv_window_route(x.dtype, weight.dtype, None if bias is None else bias.dtype, x.shape[2] // groups, weight.shape[2],
                                   bool(_os.environ.get("CST_POSCONV_GEMM")))
    return (_PosConvWindowFn if window else _PosConvGemmFn).apply(x, weight, bias, groups, lens, grad_rows, grad_rows_host)


# ------------------------------------------------------------------------------------------------
class _GluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z):
        z2 = _flat2d(z)
        ctx.save_for_backward(z2)
        ctx.shape = z.shape
        return K.glu_fwd(z2).view(*z.shape[:-1], z.shape[-1] // 2)

    @staticmethod
    def backward(ctx, dy):
        (z2,) = ctx.saved_tensors
        return K.glu_bwd(_flat2d(dy), z2).view(ctx.shape)


def glu(z):
    """F.glu over the last (channel) dimension of a channels-last tensor."""
    return _GluFn.apply(z)


class _MaskRowsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask):
        m = mask.reshape(-1).to(torch.uint8).contiguous()
        ctx.save_for_backward(m)
        ctx.shape = x.shape
        return K.mask_rows(_flat2d(x), m).view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        (m,) = ctx.saved_tensors
        return K.mask_rows(_flat2d(dy), m).view(ctx.shape), None


def mask_rows(x, mask):
    """x[mask] = 0 over the leading dims (wav2vec2.py:820-821)."""
    return _MaskRowsFn.apply(x, mask)


class _DropoutFn(torch.autograd.Function):
    """FairseqDropout (modules/fairseq_dropout.py): y = x * keep / (1 - p); backward re-evaluates the same counter-based mask."""

    @staticmethod
    def forward(ctx, x, p, key):
        ctx.p, ctx.key = p, key
        xc = x.contiguous()
        return K.dropout(xc, p, key).view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        dc = dy.contiguous()
        return K.dropout(dc, ctx.p, ctx.key).view(dy.shape), None, None


def dropout(x, p, key=None):
    """Training-mode dropout on the HIP path; `key` defaults to the next site key of the process-wide stream (rng.py)."""
    if p <= 0.0:
        return x
    from . import rng
    return _DropoutFn.apply(x, float(p), rng.next_key() if key is None else key)


class _EmbedPosFn(torch.autograd.Function):
    """dropout(scale * (E[tokens] | x) + sinusoidal_positions): one kernel forward (cst_embed_pos_fwd); backward = the
    deterministic table gradient cst_embed_bwd (embedding) or cst_dropout_scale (dense features).  The positional table
    is data (no gradient), make_positions is evaluated inside the kernel."""

    @staticmethod
    def forward(ctx, tokens, pad_mask, embed, x, pos_table, scale, pad_idx, p, key):
        out = K.embed_pos_fwd(tokens, pad_mask, embed, x, pos_table, scale, pad_idx, p, key)
        ctx.save_for_backward(tokens)
        ctx.cfg = (scale, pad_idx, p, key, embed.shape[0] if embed is not None else 0, embed.dtype if embed is not None else None)
        return out

    @staticmethod
    def backward(ctx, dy):
        (tokens,) = ctx.saved_tensors
        scale, pad_idx, p, key, V, gdt = ctx.cfg
        dy = dy.contiguous()
        if V:
            dE = K.embed_bwd(dy, tokens, V, scale, pad_idx, p, key, gdt) if ctx.needs_input_grad[2] else None
            return None, None, dE, None, None, None, None, None, None
        dx = K.dropout_scale(dy, scale, p, key) if ctx.needs_input_grad[3] else None
        return None, None, None, dx, None, None, None, None, None


def embed_positions(tokens=None, pad_mask=None, embed=None, x=None, pos_table=None, scale=1.0, pad_idx=1, dropout_p=0.0):
    """[B, T, C] = dropout(scale * (embed[tokens] or x) + pos_table[make_positions(pad_mask or tokens, pad_idx)]).
    tokens int64 [B, T]; pad_mask bool/uint8 [B, T] (True = pad; takes precedence as the position source); pos_table fp32
    [>= pad_idx + 1 + T, C] or None."""
    if pad_mask is not None:
        pad_mask = pad_mask.to(torch.uint8).contiguous()
    if tokens is not None:
        tokens = tokens.contiguous()
    if x is not None and not x.is_contiguous():
        x = x.contiguous()
    return _EmbedPosFn.apply(tokens, pad_mask, embed, x, pos_table, float(scale), int(pad_idx), *_drop_args(dropout_p))


class _LsCeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, eps, pad):
        l2 = _flat2d(logits)
        t = target.reshape(-1).contiguous()
        out2, lse = K.ls_ce_fwd(l2, t, eps, pad)
        ctx.save_for_backward(l2, t, lse)
        ctx.cfg = (eps, pad, logits.shape)
        ctx.mark_non_differentiable(out2)
        return out2[0].clone(), out2

    @staticmethod
    def backward(ctx, dloss, _):
        l2, t, lse = ctx.saved_tensors
        eps, pad, shape = ctx.cfg
        g = dloss.reshape(1).float().contiguous()
        return K.ls_ce_bwd(l2, t, lse, g, eps, pad).view(shape), None, None, None


def label_smoothed_nll_loss(logits, target, eps, pad):
    """Returns (loss_sum [differentiable], nll_sum [detached]); fp32 scalars on device."""
    loss, out2 = _LsCeFn.apply(logits, target, float(eps), int(pad))
    return loss, out2[1]


class _CtcFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, target_len, input_len, blank, zero_infinity):
        loss, nll, saved = K.ctc_fwd(logits, targets, target_len, input_len, blank, zero_infinity, need_grad=ctx.needs_input_grad[0])
        ctx.save_for_backward(*[t for t in saved if t is not None])
        ctx.cfg = (blank, zero_infinity)
        ctx.mark_non_differentiable(nll)
        return loss[0].clone(), nll

    @staticmethod
    def backward(ctx, dloss, _):
        blank, zero_infinity = ctx.cfg
        g = dloss.reshape(1).float().contiguous()
        return K.ctc_bwd(ctx.saved_tensors, g, blank, zero_infinity), None, None, None, None, None


def ctc_loss(logits, targets, target_len, input_len, blank=0, zero_infinity=False):
    """CTC on raw logits [T, B, V] (any layout with unit class stride; no log-probability tensor is built): returns
    (loss_sum [differentiable fp32 scalar], nll fp32 [B], detached).  targets int64 [B, Lmax] padded; target_len / input_len int64 [B]
    on the device.  F.ctc_loss(F.log_softmax(logits.float(), -1), ..., reduction="sum") of the reference."""
    return _CtcFn.apply(logits, targets, target_len, input_len, int(blank), bool(zero_infinity))


def ctc_greedy(logits, input_len, blank=0):
    """Best-path decode on the device: (ids int32 [B, T] — counts[b] ids, then -1 —, counts int32 [B], packed) — K.ctc_greedy."""
    return K.ctc_greedy(logits, input_len, int(blank))


def ctc_prefix_beam_search(logits, input_len, blank, beam, beam_size_token, beam_threshold, nbest, trace=False):
    """CTC prefix beam search on the device (cst_ctc_topn + cst_ctc_beam, include/cst.h) on raw logits [T, B, V]: per utterance the
    list, best first, of (tokens — a list of ints —, score), at most min(nbest, beam) long.  Each frame offers its
    min(beam_size_token, V - 1) most probable classes.  ONE transfer brings the packed result to the host.  trace=True returns
    (hyps, trace) with trace = dict(node, pb, pnb [B, T, beam], nodes [B, 4, 1 + T beam]) as host numpy arrays.  A request beyond the
    kernel's envelope raises (RuntimeError, CST_ERR_UNSUPPORTED); ctc_decoder.CtcBeamDecoder routes such requests to the host."""
    T, B, V = logits.shape
    N = max(1, min(int(beam_size_token), V - 1))
    nb = max(1, min(int(nbest), int(beam)))
    lists = K.ctc_topn(logits, input_len, int(blank), N)
    r = K.ctc_beam(logits, input_len, int(blank), lists, int(beam), float(beam_threshold), nb, trace=trace)
    host = r["packed"].cpu().numpy()
    o1, o2, o3 = B * nb * T, B * nb * T + B * nb, B * nb * T + 2 * B * nb
    tokens, lens = host[:o1].reshape(B, nb, T), host[o1:o2].reshape(B, nb)
    score, n_hyp = host[o2:o3].view("float32").reshape(B, nb), host[o3:]
    hyps = [[(tokens[b, h, :lens[b, h]].tolist(), float(score[b, h])) for h in range(int(n_hyp[b]))] for b in range(B)]
    if not trace:
        return hyps
    return hyps, dict(node=r["trace_node"].cpu().numpy(), pb=r["trace_pb"].cpu().numpy(), pnb=r["trace_pnb"].cpu().numpy(),
                      nodes=r["nodes"].cpu().numpy())


class _InfoNceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, idx, inv_temp):
        loss, nll, counters, saved, _ = K.infonce_fwd(x, y, idx, inv_temp)
        ctx.save_for_backward(*saved)
        ctx.inv_temp = inv_temp
        ctx.mark_non_differentiable(nll, counters)
        return loss[0].clone(), nll, counters

    @staticmethod
    def backward(ctx, dloss, _nll, _counters):
        g = dloss.reshape(1).float().contiguous()
        dx, dy = K.infonce_bwd(ctx.saved_tensors, g, ctx.inv_temp, need_dy=ctx.needs_input_grad[1])
        return (dx if ctx.needs_input_grad[0] else None), dy, None, None


def infonce_loss(x, y, neg_idx, logit_temp):
    """The contrastive loss of wav2vec2 pre-training on the masked positions: x [N, D] (final_proj), y [N, D] (project_q), neg_idx int32
    [N, K'] flat row indices of each position's negatives (sample_negatives) -> (loss_sum [differentiable fp32 scalar], nll fp32 [N],
    counters int32 [2] = (correct, count), both detached).  compute_preds (models/wav2vec/wav2vec2.py:512-525) + F.cross_entropy against
    class 0 with reduction="sum" (criterions/wav2vec_criterion.py:64-103) without the gathered [K' + 1, N, D] targets or the logits."""
    return _InfoNceFn.apply(x, y, neg_idx, 1.0 / float(logit_temp))


def sample_negatives(B, M, num_negatives, cross_sample_negatives=0, key=None, device="cuda"):
    """Negatives of B utterances with M masked positions each: int32 [B * M, K + Kx] for infonce_loss.  key: one dropout-site key
    (rng.next_key() when None), so the draws follow the update's seed like every mask."""
    if key is None:
        from . import rng
        key = rng.next_key()
    K_, Kx = int(num_negatives), int(cross_sample_negatives)
    return K.w2v_negatives(key, B, M, K_, Kx, device).view(B * M, K_ + Kx)


class _GumbelVqFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, vars_, G, tau, training, key, noise):
        q, idx, onehot, avg, stats, exph = K.gumbel_vq_fwd(logits, vars_, G, training, key, noise)
        ctx.save_for_backward(logits.contiguous(), vars_.contiguous(), onehot, avg, exph, noise)
        ctx.cfg = (G, tau, key, training)
        ctx.set_materialize_grads(False)  # an output nobody differentiated arrives as None in backward, not as zeros
        code_ppl = stats[1].clone()
        ctx.mark_non_differentiable(idx, avg, code_ppl)  # (ONE call: a second one replaces the first's list)
        return q, stats[0].clone(), code_ppl, idx, avg

    @staticmethod
    def backward(ctx, dq, dppl, *_):
        logits, vars_, onehot, avg, exph, noise = ctx.saved_tensors
        G, tau, key, training = ctx.cfg
        N, GV = logits.shape
        V, d = GV // G, vars_.shape[1]
        if dq is None and dppl is None:
            return None, None, None, None, None, None, None
        has_dq = dq is not None
        if not has_dq:  # only prob_perplexity was differentiated
            dq = torch.zeros(N, G * d, dtype=logits.dtype, device=logits.device)
        dq = dq.contiguous()
        dl = dvars = None
        if ctx.needs_input_grad[0] and not training:
            # eval takes the hard argmax of the raw logits: as in the reference, q passes nothing to them there; prob_perplexity would
            # (softmax of the logits), and that gradient is not built for eval — refused rather than returned as zeros
            if dppl is not None:
                raise NotImplementedError("gumbel_vector_quantize: the gradient of prob_perplexity in eval mode is not built; run "
                                          "evaluation under torch.no_grad() or differentiate q alone")
            dl = torch.zeros_like(logits)
        elif ctx.needs_input_grad[0]:
            gy = torch.empty(N, GV, dtype=logits.dtype, device=logits.device)
            for g in range(G):  # gy_g [N, V] = dq_g [N, d] vars_g^T: a forward-form product with K = d
                K.gemm(dq, vars_, gy, N, V, d, a_kmajor=1, b_kmajor=1, lda=G * d, ldb=d, ldc=GV, a_off=g * d, b_off=g * V * d, c_off=g * V,
                       split_k=1)
            g1 = (dppl if dppl is not None else torch.zeros((), device=logits.device)).reshape(1).float().contiguous()
            dl = K.gumbel_vq_bwd(logits, gy, avg, exph, g1, G, 1.0 / tau, key, noise)
        if ctx.needs_input_grad[1] and has_dq:
            dvars = torch.empty_like(vars_)
            for g in range(G):  # d vars_g [V, d] = onehot_g^T dq_g over the N rows: the weight-gradient form, dense and exact in the one-hot
                K.gemm(onehot, dq, dvars, V, d, N, a_kmajor=0, b_kmajor=0, lda=GV, ldb=G * d, ldc=d, a_off=g * V, b_off=g * d, c_off=g * V * d,
                       split_k=-1)
        return dl, dvars, None, None, None, None, None


def gumbel_vector_quantize(logits, vars_, groups, tau, training=True, key=None, noise=None):
    """GumbelVectorQuantizer.forward after its weight_proj (modules/gumbel_vector_quantizer.py:148-199): logits [N, G * V], vars_
    [G * V, d] -> (q [N, G * d], prob_perplexity, code_perplexity, idx int32 [N, G], avg_probs fp32 [G, V]).  q carries the
    straight-through gradient of F.gumbel_softmax(hard=True) to the logits and the dense gradient to vars_; prob_perplexity carries
    the diversity term.  In eval mode (the hard argmax of the raw logits) q still carries the dense gradient to vars_, as the
    reference's hard_x * vars does, and nothing to the logits; a gradient of prob_perplexity is refused there.  key: one dropout-site key (rng.next_key() when None and training); noise: fp32 [N, G, V] used instead."""
    if training and key is None and noise is None:
        from . import rng
        key = rng.next_key()
    return _GumbelVqFn.apply(logits, vars_, int(groups), float(tau), bool(training), int(key or 0), noise)


class _MeanSquareFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        out = torch.zeros(1, dtype=torch.float32, device=x.device)
        K.sumsq(x, out)  # fixed-order two-stage reduction: reproducible
        ctx.save_for_backward(x)
        return out[0] / x.numel()

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return (x.float() * (g.float() * (2.0 / x.numel()))).to(x.dtype)


def mean_square(x):
    """x.float().pow(2).mean() — the features_pen of wav2vec2 pre-training (models/wav2vec/wav2vec2.py:537) — through cst_sumsq: no
    fp32 copy or square of the CNN's output is built."""
    return _MeanSquareFn.apply(x)


class _ContrastiveFn(torch.autograd.Function):
    """compute_contrastive (criterions/triplet_st_mt_contrastive.py:154-169), summed over utterances and text slots."""

    @staticmethod
    def forward(ctx, a, t, temp):
        a, t = a.contiguous(), t.contiguous()
        loss, sim, na, nt = K.contrastive_fwd(a, t, temp)
        ctx.save_for_backward(a, t, sim, na, nt)
        ctx.temp = temp
        return loss[0]

    @staticmethod
    def backward(ctx, dloss):
        a, t, sim, na, nt = ctx.saved_tensors
        da, dt = K.contrastive_bwd(a, t, sim, na, nt, dloss.reshape(1).float().contiguous(), ctx.temp)
        return da, dt, None


def contrastive_loss(mem_audio_bm, mem_text_bm, temp):
    """mem_* [B, M, C] batch-major (same dtype) -> fp32 scalar, sum over utterances and text slots."""
    assert mem_audio_bm.shape == mem_text_bm.shape and mem_audio_bm.dtype == mem_text_bm.dtype
    return _ContrastiveFn.apply(mem_audio_bm, mem_text_bm, float(temp))
