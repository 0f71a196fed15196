"""cst_layernorm_fwd / _bwd / _bwd_tiles, cst_ln_gelu_fwd / _bwd and cst_conv0_ln_gelu_fwd / _bwd on a real MI355X against the fp64
restatements of norm_ref.py, under ITS per-element bounds (counted from the kernels' operation sequences; test_norm_ref_cpu.py shows
that a faithful fp32 evaluation stays inside them and that every listed defect leaves them).  The shapes are the smallest that reach
each path: every vector-slot filling (nvec = 1, 9, 64, 65, 96, 128, 129, 256), NV = 1, 2, 4, the grid-stride loops of all four row
kernels (more rows than 4 x the block cap, twice over), the generic KC = 16 layer-0 kernels next to the k = 10 instantiation, two
layer-0 backward blocks with the second partly filled.  mean and rstd are outputs in their own right.

colsum(du): test_ln_gelu allows it 2e-4 (fp32) / 2e-2 (bf16) of max|du| sqrt(rows).  The counted bound is stated in sum |du| and the
bounds of du, per column: at 3 x 5471 x 64 with the inputs of norm_ref.py (rows with rstd ~ 300 make max|du| ~ 300) the largest column's
bound is 2.2 times below that scale in both dtypes (24.1 against 52.8 in fp32, 2408 against 5276 in bf16), the median column's 8.3 times
(fp32) and 4.8 times (bf16) — and unlike the scale it is not the same for a column whose terms are small
(test_norm_ref_cpu.py::test_colsum_bound_is_tighter_than_the_old_scale prints these figures and asserts the order).

Every test prints `RATIO <kernel> <dtype> <quantity> ... worst err/bound` (pytest -s)."""
from importlib import import_module

import pytest
import torch

import norm_ref as R
from conftest import load_pkg

pytestmark = pytest.mark.gpu
DTS = [R.F, R.B]
IDS = ["f32", "bf16"]


@pytest.fixture(scope="module")
def K():
    load_pkg()
    return import_module("chimera-st_amd.kernels"), import_module("chimera-st_amd.lib")


def within(got, ref, bound, what):
    got = got.detach().cpu()
    assert bool(torch.isfinite(got.float()).all()), what + ": non-finite output"
    ratio, bad = R.worst_ratio(got, ref, bound)
    print("RATIO %-44s worst err/bound %.3f" % (what, ratio))
    assert bad == 0, "%s: %d of %d elements outside the bound, worst err/bound %.3f" % (what, bad, got.numel(), ratio)


def cu(*ts):
    return [None if t is None else t.cuda() for t in ts]


# ------------------------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ------------------------------------------------------------------------------------------------------------------------------------
def _ln_forward(k, rows, cols, dt, with_res, want_sum, tag):
    x, res, gamma, beta, _, _ = R.ln_case(rows, cols, dt, with_res)
    r = R.ln_fwd64(x, res, gamma, beta, R.EPS)
    b = R.ln_fwd_bounds(r, dt)
    y, s, mean, rstd = k.layernorm_fwd(*cu(x, res, gamma, beta), R.EPS, want_sum=want_sum)
    within(y, r["y"], b["y"], tag + " y")
    within(mean, r["mean"], b["mean"], tag + " mean")
    within(rstd, r["rstd"], b["rstd"], tag + " rstd")
    assert (s is not None) == (with_res and want_sum)
    if s is not None:
        within(s, r["sum"], b["sum"], tag + " sum")
    return y, s, mean, rstd


def _ln_backward(k, rows, cols, dt, s, mean, rstd, with_dres, tag):
    """s, mean, rstd: what the forward kernel wrote (device).  The reference is a function of exactly these."""
    _, _, gamma, _, dy, dres = R.ln_case(rows, cols, dt, True)
    if not with_dres:
        dres = None
    r = R.ln_bwd64(dy, s.cpu(), gamma, mean.cpu(), rstd.cpu(), dres)
    b = R.ln_bwd_bounds(r, dt)
    ddy, dg_, ddres = cu(dy, gamma, dres)
    dx, dg, db = k.layernorm_bwd(ddy, s, dg_, mean, rstd, ddres)
    within(dx, r["dx"], b["dx"], tag + " dx")
    within(dg, r["dgamma"], b["dgamma"], tag + " dgamma")
    within(db, r["dbeta"], b["dbeta"], tag + " dbeta")
    # gradients written in the parameter dtype: the fp32 result rounded once, bit for bit
    dx2, dg2, db2 = k.layernorm_bwd(ddy, s, dg_, mean, rstd, ddres, grad_dtype=dt)
    assert dg2.dtype == dt and torch.equal(dx2, dx) and torch.equal(dg2, dg.to(dt)) and torch.equal(db2, db.to(dt))
    return ddy, dg_, ddres, dx, dg, db


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("cols", R.LN_COLS)
def test_layernorm_columns(K, cols, dt):
    k, _ = K
    rows = R.LN_ROWS
    tag = "ln %s" % R.NAME[dt]
    y, s, mean, rstd = _ln_forward(k, rows, cols, dt, True, True, tag + " fwd res+sum %dx%d" % (rows, cols))
    y1, s1, mean1, rstd1 = _ln_forward(k, rows, cols, dt, True, False, tag + " fwd res %dx%d" % (rows, cols))
    assert s1 is None and torch.equal(y1, y) and torch.equal(mean1, mean) and torch.equal(rstd1, rstd)
    for want_sum in (False, True):   # without a residual nothing is written back, whatever is asked
        _ln_forward(k, rows, cols, dt, False, want_sum, tag + " fwd nores %dx%d" % (rows, cols))
    for with_dres in (True, False):
        _ln_backward(k, rows, cols, dt, s, mean, rstd, with_dres, tag + " bwd %s %dx%d" % ("dres" if with_dres else "nodres", rows, cols))


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("cols", R.BIG_COLS)
def test_layernorm_forward_grid_stride(K, cols, dt):
    """More rows than two full grids: cst_layernorm_fwd launches ln_blocks(rows, 2048) blocks of 4 rows, so every wave runs the
    prefetch branch (row + rstep < rows) twice, or once and a last row without it."""
    k, _ = K
    rows = R.LN_FWD_BIG
    assert rows > 2 * 4 * R.LN_FWD_CAP
    _ln_forward(k, rows, cols, dt, True, True, "ln %s fwd res+sum %dx%d" % (R.NAME[dt], rows, cols))


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("cols", R.BIG_COLS)
def test_layernorm_backward_grid_stride(K, cols, dt):
    """A wave accumulates dgamma / dbeta over two or three rows; the deferred second stage and the live-tile route give the bits of
    the plain call; a tile whose rows have dy = 0 and dres = 0 stays unstamped, every other tile carries the epoch."""
    k, L = K
    rows = R.LN_BWD_BIG
    nb = L.load().cst_layernorm_bwd_workspace(rows, cols) // (8 * cols)
    assert rows > 2 * 4 * nb, "the block cap was raised: this shape no longer reaches the grid-stride loop"
    x, res, gamma, beta, _, _ = R.ln_case(rows, cols, dt, True)
    _, s, mean, rstd = k.layernorm_fwd(*cu(x, res, gamma, beta), R.EPS, want_sum=True)
    tag = "ln %s bwd dres %dx%d" % (R.NAME[dt], rows, cols)
    ddy, dg_, ddres, dx, dg, db = _ln_backward(k, rows, cols, dt, s, mean, rstd, True, tag)
    before = k.DEFER.flushes
    with k.deferred_reductions(True) as ctx:
        assert ctx.enabled
        dx_d, dg_d, db_d = k.layernorm_bwd(ddy, s, dg_, mean, rstd, ddres, defer=True)
    assert k.DEFER.flushes == before + 1
    assert torch.equal(dx_d, dx) and torch.equal(dg_d, dg) and torch.equal(db_d, db), "the deferred second stage changes bits"
    # tiles of 64 rows: 5 lies in the first grid-stride iteration, 70 only in the second (rows 4480 ..), 128 (3 rows) only in the third
    dead = [5, 70]
    zdy, zdres = ddy.clone(), ddres.clone()
    for t in dead:
        zdy[64 * t:64 * t + 64] = 0
        zdres[64 * t:64 * t + 64] = 0
    plain = k.layernorm_bwd(zdy, s, dg_, mean, rstd, zdres)
    dx_t, dg_t, db_t, (stamps, epoch) = k.layernorm_bwd(zdy, s, dg_, mean, rstd, zdres, want_tiles=True)
    assert torch.equal(dx_t, plain[0]) and torch.equal(dg_t, plain[1]) and torch.equal(db_t, plain[2]), "the tile route changes bits"
    st = stamps.cpu().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    assert st.numel() == (rows + 63) // 64 == 129
    live = torch.ones(st.numel(), dtype=torch.bool)
    live[dead] = False
    assert bool((st[live] == epoch).all()), "a live tile is unstamped: %s" % torch.nonzero(st != epoch).reshape(-1).tolist()
    assert bool((st[~live] != epoch).all()) and bool((dx_t[64 * 70:64 * 71] == 0).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# ln_gelu
# ------------------------------------------------------------------------------------------------------------------------------------
def _ln_gelu(k, Bn, L, C, dt, which, padded):
    u, gamma, beta, dy = R.lg_case(Bn, L, C, dt)
    lim = R.lg_limit(Bn, L, which)
    r = R.ln_gelu_fwd64(u, gamma, beta, R.EPS, lim)
    b = R.ln_gelu_fwd_bounds(r, dt)
    du_, dg_, db_, ddy, dlim = cu(u, gamma, beta, dy, lim)
    y, mean, rstd = k.ln_gelu_fwd(du_, dg_, db_, R.EPS, row_limit=dlim)
    tag = "ln_gelu %s" % R.NAME[dt]
    case = " %dx%dx%d lim=%s" % (Bn, L, C, which)
    within(y, r["y"], b["y"], tag + " y" + case)
    within(mean, r["mean"], b["mean"], tag + " mean" + case)
    within(rstd, r["rstd"], b["rstd"], tag + " rstd" + case)
    dead = (~r["live"]).view(Bn, L)
    assert bool((y.cpu()[dead] == 0).all()) and bool((mean.cpu()[dead] == 0).all()) and bool((rstd.cpu()[dead] == 0).all())
    rb = R.ln_gelu_bwd64(dy, u, gamma, beta, mean.cpu(), rstd.cpu(), lim)
    bb = R.ln_gelu_bwd_bounds(rb, dt)
    first = None
    for pad in padded:
        out = k.ln_gelu_bwd(ddy, du_, dg_, db_, mean, rstd, row_limit=dlim, want_colsum=True, padded=pad)   # (dy is NOT zeroed from the limit on)
        if pad:
            assert out[0].stride(0) == (L + 2) * C
        for n, o in zip(("du", "dgamma", "dbeta", "colsum"), out):
            within(o, rb[n], bb[n], tag + " %s%s%s" % (n, case, " padded" if pad else ""))
        assert bool((out[0].cpu()[dead] == 0).all())
        if first is not None:
            assert all(torch.equal(a, c) for a, c in zip(first, out)), "padded and plain du differ"
        first = out


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("C", R.LG_COLS)
def test_ln_gelu_columns(K, C, dt):
    k, _ = K
    for which in (None, "L", "L/3", "0"):
        _ln_gelu(k, R.LG_B, R.LG_L, C, dt, which, (False, True))


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("which", [None, "L/3"])
@pytest.mark.parametrize("C", R.BIG_COLS)
def test_ln_gelu_grid_stride(K, C, which, dt):
    """3 x 5471 rows: above 4 x LG_FWD_BLOCKS = 16384 and four times 4 x LG_BWD_BLOCKS; 5471 divides neither block stride, so the
    utterance index of a wave's rows changes from one iteration to the next."""
    k, L = K
    Bn, Lr = R.LG_B, R.LG_BIG_L
    assert Bn * Lr > 4 * R.LG_FWD_CAP and (4 * R.LG_FWD_CAP) % Lr != 0 and (4 * R.LG_BWD_CAP) % Lr != 0
    assert Bn * Lr > 4 * L.load().cst_ln_gelu_bwd_workspace(Bn * Lr, C) // (12 * C), "the block cap was raised"
    _ln_gelu(k, Bn, Lr, C, dt, which, (which is not None,))


# ------------------------------------------------------------------------------------------------------------------------------------
# layer 0
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("k_,stride,C,S", R.C0_CASES)
def test_conv0_ln(K, k_, stride, C, S, dt):
    """k = 10 is the specialised instantiation, every other k the generic KC = 16 kernel with zero-padded taps.  L > 2048: two backward
    blocks per utterance, the second partly filled; L is no multiple of the forward block's 128 frames."""
    k, _ = K
    wav, w, bias, gamma, beta, dy = R.c0_case(k_, stride, C, S, dt)
    L = R.c0_L(k_, stride, S)
    assert L > R.C0_BWD_TB and L % 128 != 0
    dwav, dw_, dbias_, dg_, db_, ddy = cu(wav, w, bias, gamma, beta, dy)
    for which in R.C0_LIMITS:
        lim = R.c0_limit(L, which)
        dlim = None if lim is None else lim.cuda()
        r = R.conv0_ln_fwd64(wav, w, bias, gamma, beta, k_, stride, R.EPS, lim)
        b = R.conv0_ln_fwd_bounds(r, dt)
        y, mean, rstd = k.conv0_ln_fwd(dwav, dw_, dbias_, dg_, db_, k_, stride, R.EPS, frame_limit=dlim)
        live = r["live"].view(R.C0_B, L)
        tag = "conv0_ln %s" % R.NAME[dt]
        case = " k%d s%d C%d lim=%s" % (k_, stride, C, which)
        yc, mc, rc = y.cpu(), mean.cpu(), rstd.cpu()
        within(yc[live], r["y"][live], b["y"][live], tag + " y" + case)
        within(mc[live], r["mean"][live], b["mean"][live], tag + " mean" + case)
        within(rc[live], r["rstd"][live], b["rstd"][live], tag + " rstd" + case)
        rb = R.conv0_ln_bwd64(dy, wav, w, bias, gamma, beta, mc, rc, k_, stride, lim)
        bb = R.conv0_ln_bwd_bounds(rb, dt)
        out = k.conv0_ln_bwd(ddy, dwav, dw_, dbias_, dg_, db_, mean, rstd, k_, stride, frame_limit=dlim)
        for n, o in zip(("dW", "dbias", "dgamma", "dbeta"), out):
            within(o, rb[n], bb[n], tag + " " + n + case)


# ------------------------------------------------------------------------------------------------------------------------------------
# the GELU constants: what norm_ref.A_GELU / A_DGELU rest on
# ------------------------------------------------------------------------------------------------------------------------------------
def test_gelu_on_the_device(K):
    """The erf forms (fp32 storage) on 2.4 M points over [-6, 6] against fp64: the worst error, doubled, is inside A_GELU / A_DGELU.
    The polynomials (bf16 storage) on every bf16 argument in [-6, 6]: the stored result is the rounded fp32 restatement of norm_ref.py,
    bit for bit — the restatement, whose error test_norm_ref_cpu.py measures on a dense fp32 grid, is the device function."""
    k, L = K
    x = torch.linspace(-6.0, 6.0, 2400008, dtype=torch.float64).float()
    xd = x.cuda()
    y = k.act_fwd(xd, L.ACT_GELU).cpu().double()
    d = k.act_bwd(torch.ones_like(xd), xd, L.ACT_GELU).cpu().double()
    for name, got, ref, a in (("gelu", y, R.gelu64(x.double()), R.A_GELU[R.F]), ("gelu'", d, R.dgelu64(x.double()), R.A_DGELU[R.F])):
        err = (got - ref).abs()
        print("MEASURED erf %-5s worst abs error %.4e at x = %.4f (constant %.3e)" % (name, float(err.max()), float(x[err.argmax()]), a))
        assert 2.0 * float(err.max()) <= a, name
    xb = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    xb = xb[torch.isfinite(xb.float()) & (xb.float().abs() <= 6.0)]
    xb = xb[:xb.numel() // 8 * 8]   # (cst_act_fwd takes multiples of 8)
    assert xb.numel() > 33000
    xbd = xb.cuda()
    assert torch.equal(k.act_fwd(xbd, L.ACT_GELU).cpu(), R.gelu_poly32(xb.float()).to(torch.bfloat16))
    assert torch.equal(k.act_bwd(torch.ones_like(xbd), xbd, L.ACT_GELU).cpu(), R.dgelu_poly32(xb.float()).to(torch.bfloat16))
