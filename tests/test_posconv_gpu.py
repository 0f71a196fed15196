"""cst_posconv_fwd / _dx / _dw (csrc/posconv.hip) and the implicit-GEMM route (functional._PosConvGemmFn) on a real MI355X against the fp64
restatements of posconv_ref.py, under ITS per-element bounds (counted from the kernels' operation sequences; test_posconv_ref_cpu.py
shows that a faithful fp32 evaluation stays inside them in two summation shapes and that every listed defect leaves them).  The cases
are the smallest shapes that reach each path of the three kernels (posconv_ref.CASES names the path next to every case).

Through the function every reference is a function of the device's own intermediates: z and y from x, w and bias; dz = act_bwd(dy, z)
recomputed here (the same deterministic kernel: nothing is asserted about it, test_helper_gpu.py covers it); dx from that dz, the
parameter-layout (unflipped) weight and dy; dw and db from that dz and x.  The weight re-layouts and the flip of functional.py are so held
against fp64 and not against themselves.  No element is excluded anywhere.  The GEMM route (CST_POSCONV_GEMM=1) must return the window
route's bits at every case, and is therefore inside the same bounds.

Every test prints `RATIO posconv <case> <quantity> worst err/bound` (pytest -s)."""
import functools
import importlib

import pytest
import torch

import posconv_ref as R
from conftest import load_pkg

pytestmark = pytest.mark.gpu
QUANT = ("y", "z", "dx", "dw", "db")
WINDOW_CALLS = ["posconv_fwd", "posconv_dx", "posconv_dw"]


@pytest.fixture(scope="module")
def mods():
    load_pkg()
    return tuple(importlib.import_module("chimera-st_amd." + m) for m in ("functional", "kernels", "lib"))


def within(got, ref, bound, what):
    got = got.detach().cpu()
    assert bool(torch.isfinite(got.float()).all()), what + ": non-finite output"
    assert got.shape == ref.shape, "%s: shape %s, expected %s" % (what, tuple(got.shape), tuple(ref.shape))
    ratio, bad = R.worst_ratio(got, ref, bound)
    print("RATIO posconv %-36s worst err/bound %.3f" % (what, ratio))
    assert bad == 0, "%s: %d of %d elements outside the bound, worst err/bound %.3f" % (what, bad, got.numel(), ratio)


def same_bits(a, b, what):
    for name in QUANT:
        assert a[name].shape == b[name].shape and a[name].dtype == b[name].dtype, "%s %s" % (what, name)
        assert torch.equal(a[name], b[name]), "%s: %s differs on %d of %d elements (max |diff| %.3e)" % (
            what, name, int((a[name] != b[name]).sum()), a[name].numel(), float((a[name].float() - b[name].float()).abs().max()))


def run(mods, monkeypatch, gemm_route, c, lens=None, host=False):
    """One call of pos_conv_gelu_residual + backward (the launch-recording wrapper of test_posconv_window_gpu.run) -> y, z, dz, dx, dw, db
    and the window-kernel launches of the call.  lens: passed as lens AND as grad_rows (host: also as grad_rows_host)."""
    CF, Kn, L = mods
    if gemm_route:
        monkeypatch.setenv("CST_POSCONV_GEMM", "1")
    else:
        monkeypatch.delenv("CST_POSCONV_GEMM", raising=False)
    calls = []
    for name in WINDOW_CALLS:
        fn = getattr(Kn, name)
        monkeypatch.setattr(Kn, name, (lambda f, n: lambda *a, **kw: (calls.append(n), f(*a, **kw))[1])(fn, name))
    x, w, b = (c[n].cuda().requires_grad_(True) for n in ("x", "w", "bias"))
    dy = c["dy"].cuda()
    lim = None if lens is None else torch.tensor(lens, dtype=torch.int32, device="cuda")
    y = CF.pos_conv_gelu_residual(x, w, b, c["G"], lim, lim, list(lens) if (host and lens is not None) else None)
    z = y.grad_fn.saved_tensors[2].clone()
    y.backward(dy)
    monkeypatch.undo()
    dz = Kn.act_bwd(dy, z, L.ACT_GELU)
    return {"y": y.detach(), "z": z, "dz": dz, "dx": x.grad, "dw": w.grad, "db": b.grad, "calls": calls}


@functools.lru_cache(maxsize=None)
def forward_reference(name, lens=None):
    """z, y in fp64 and their bounds: a function of the case alone, shared by the tests of that case."""
    c = R.case(name, lens)
    z, y = R.fwd64(c["x"], c["w"], c["bias"], c["G"], lens)
    return dict(z=z, y=y), R.fwd_bounds(c["x"], c["w"], c["bias"], c["G"])


def hold(out, c, name, lens, tag):
    """Every output of one call against fp64 under the counted bounds."""
    ref, b = forward_reference(name, lens)
    within(out["z"], ref["z"], b["z"], "%s z" % tag)
    within(out["y"], ref["y"], b["y"], "%s y" % tag)
    dz = out["dz"].cpu()
    within(out["dx"], R.dx64(dz, c["w"], c["dy"], c["G"]), R.dx_bounds(dz, c["w"], c["dy"], c["G"])["dx"], "%s dx" % tag)
    dw, db = R.dw64(dz, c["x"], c["G"], c["k"])
    bw = R.dw_bounds(dz, c["x"], c["G"], c["k"])
    within(out["dw"], dw, bw["dw"], "%s dw" % tag)
    within(out["db"], db, bw["db"], "%s db" % tag)


@pytest.mark.parametrize("name", list(R.CASES))
def test_function_under_the_bounds_and_both_routes_same_bits(mods, monkeypatch, name):
    """Every case of both tables.  past_list: dy is non-zero on the case's two short stretches only, so the device's dz is too; the
    forward / dX kernels run 129 frame blocks per utterance and both weight-gradient routes walk 1032 K blocks without stamps."""
    c = R.case(name)
    new = run(mods, monkeypatch, False, c)
    assert new["calls"] == WINDOW_CALLS
    hold(new, c, name, None, name)
    old = run(mods, monkeypatch, True, c)
    assert old["calls"] == []
    same_bits(new, old, "%s: window route vs GEMM route" % name)


@pytest.mark.parametrize("host", [False, True], ids=["device_stamps", "host_rows"])
@pytest.mark.parametrize("name", sorted(R.LIMITS))
def test_limited_calls_keep_every_bit(mods, monkeypatch, name, host):
    """lens = grad_rows with a dead frame block behind a live one and an utterance with nothing live: the limited call has the bits of
    the unlimited call on the same (zeroed) inputs, on both routes; dx of a dead block is dy itself."""
    lens = R.LIMITS[name]
    c = R.case(name, lens)
    free = run(mods, monkeypatch, False, c)
    lim = run(mods, monkeypatch, False, c, lens, host)
    old = run(mods, monkeypatch, True, c, lens, host)
    assert free["calls"] == WINDOW_CALLS and lim["calls"] == WINDOW_CALLS and old["calls"] == []
    hold(lim, c, name, lens, "%s limited" % name)
    same_bits(free, lim, "%s: limited vs unlimited" % name)
    same_bits(lim, old, "%s limited: window route vs GEMM route" % name)
    geo = R.geometry(c["B"], c["T"], c["G"], c["k"])
    dy, dead_blocks = c["dy"].cuda(), 0
    for b, n in enumerate(lens):
        for blk in range(geo["nblk"]):
            if blk * R.FBM >= min(n + geo["lp"], c["T"]):
                rows = slice(blk * R.FBM, (blk + 1) * R.FBM)
                assert torch.equal(lim["dx"][b, rows], dy[b, rows]), "%s: dx of dead block %d of utterance %d is not dy" % (name, blk, b)
                dead_blocks += 1
    assert dead_blocks >= 2


def _wg(w, G):
    k = w.shape[2]
    return w.view(G, R.CG, R.CG, k).permute(0, 1, 3, 2).contiguous()   # [g][co][j][ci]


@pytest.mark.parametrize("name", ["full4p1", "k127"])
def test_forward_without_bias(mods, name):
    _, Kn, _ = mods
    c = R.case(name)
    y, z = Kn.posconv_fwd(c["x"].cuda(), _wg(c["w"].cuda(), c["G"]), None, c["G"])
    zr, yr = R.fwd64(c["x"], c["w"], None, c["G"])
    b = R.fwd_bounds(c["x"], c["w"], None, c["G"])
    within(z, zr, b["z"], "%s nobias z" % name)
    within(y, yr, b["y"], "%s nobias y" % name)


@pytest.mark.parametrize("name", ["nkb5", "k126"])
def test_dw_without_db_has_the_same_bits(mods, name):
    _, Kn, _ = mods
    c = R.case(name)
    dz, x = c["dz"].cuda(), c["x"].cuda()
    db = torch.full((c["C"],), 7.0, dtype=R.BF, device="cuda")
    with_db = Kn.posconv_dw(dz, x, c["G"], c["k"], db)
    without = Kn.posconv_dw(dz, x, c["G"], c["k"], None)
    assert torch.equal(with_db, without)
    dwr, dbr = R.dw64(c["dz"], c["x"], c["G"], c["k"])
    b = R.dw_bounds(c["dz"], c["x"], c["G"], c["k"])
    within(without, dwr, b["dw"], "%s direct dw" % name)
    within(db, dbr, b["db"], "%s direct db" % name)


def test_more_k_blocks_than_the_live_list_holds(mods):
    """nkb = 1032 > DKLIST: every block runs.  The blocks past index 1024 carry weight (the last 100 frames of utterance 1); with stamps
    the list is still not built, and the result has the bits of the call without them."""
    _, Kn, _ = mods
    name = "past_list"
    for lens in (None, R.PAST_LIST_ROWS):
        c = R.case(name, lens)
        dz, x = c["dz"].cuda(), c["x"].cuda()
        db = torch.full((c["C"],), 7.0, dtype=R.BF, device="cuda")
        dw = Kn.posconv_dw(dz, x, c["G"], c["k"], db)
        dwr, dbr = R.dw64(c["dz"], c["x"], c["G"], c["k"])
        b = R.dw_bounds(c["dz"], c["x"], c["G"], c["k"])
        tag = name + ("" if lens is None else " stamped")
        within(dw, dwr, b["dw"], tag + " dw")
        within(db, dbr, b["db"], tag + " db")
        if lens is not None:
            # (the stamps mark dead only blocks whose dz is zero anyway, as the caller's contract demands: honouring them would give
            #  the same bits, so this run pins the bit-equality of the stamped call, not that the stamps are left unread)
            stamps = R.k_block_stamps(c["B"], c["T"], c["k"], lens).cuda()
            db2 = torch.full((c["C"],), 7.0, dtype=R.BF, device="cuda")
            dw2 = Kn.posconv_dw(dz, x, c["G"], c["k"], db2, (stamps, 1))
            assert torch.equal(dw2, dw) and torch.equal(db2, db)


def _seven(*shape):
    return torch.full(shape, 7.0, dtype=R.BF, device="cuda")


def test_every_k_block_dead_writes_zeros(mods):
    """grad_rows = (0, 0): no K block is live (nk = 0), and dw and db are still written — as zero bits."""
    _, _, L = mods
    c = R.case("wrap", (0, 0))
    B, T, G, k, C = (c[n] for n in ("B", "T", "G", "k", "C"))
    assert not bool(c["dz"].any())
    stamps = R.k_block_stamps(B, T, k, (0, 0)).cuda()
    assert stamps.numel() * 64 >= B * R.geometry(B, T, G, k)["Tp"] - (k - 1) and not bool(stamps.any())
    dz, x = c["dz"].cuda(), c["x"].cuda()
    dw, db = _seven(C, R.CG, k), _seven(C)
    rc = L.load().cst_posconv_dw(L.ptr(dz), L.ptr(x), L.ptr(dw), L.ptr(db), stamps.data_ptr(), 1, B, T, C, G, k, L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert not bool(dw.view(torch.int16).any()) and not bool(db.view(torch.int16).any())


def test_refusals_touch_nothing(mods):
    _, _, L = mods
    lib, P, S = L.load(), L.ptr, L.stream_ptr
    B, T, G, k = 2, 9, 2, 5
    C = R.CG * G
    x, dy = (torch.randn(B, T, C, device="cuda").to(R.BF) for _ in range(2))
    w = torch.randn(G, R.CG, k, R.CG, device="cuda").to(R.BF)
    bias = torch.randn(C, device="cuda").to(R.BF)
    y, z, dx, dw, db = _seven(B, T, C), _seven(B, T, C), _seven(B, T, C), _seven(C, R.CG, k), _seven(C)
    BIG = dict(B_=1 << 16, T_=1 << 10)   # B T C = 2^26 * 96 >= 2^31: numbers only, nothing of that size exists

    def fwd(x_=x, B_=B, T_=T, C_=C, G_=G, k_=k):
        return lib.cst_posconv_fwd(P(x_), P(w), P(bias), P(y), P(z), None, B_, T_, C_, G_, k_, S())

    def bdx(x_=x, B_=B, T_=T, C_=C, G_=G, k_=k):
        return lib.cst_posconv_dx(P(x_), P(w), P(dy), P(dx), None, B_, T_, C_, G_, k_, S())

    def bdw(x_=x, B_=B, T_=T, C_=C, G_=G, k_=k):
        return lib.cst_posconv_dw(P(dy), P(x_), P(dw), P(db), None, 0, B_, T_, C_, G_, k_, S())

    assert BIG["B_"] * BIG["T_"] * C >= 1 << 31
    for fn, entry in ((fwd, b"cst_posconv_fwd"), (bdx, b"cst_posconv_dx"), (bdw, b"cst_posconv_dw")):
        for kw in (dict(C_=96, G_=3), dict(k_=0), dict(k_=129), dict(x_=None), BIG):
            assert fn(**kw) == -1, (entry, kw)                    # CST_ERR_BAD_ARG: what CST_REQUIRE returns
            assert entry in lib.cst_last_error(), (entry, kw, lib.cst_last_error())
    torch.cuda.synchronize()
    for t in (y, z, dx, dw, db):
        assert bool((t == 7.0).all())
    assert fwd() == 0 and bdx() == 0 and bdw() == 0               # the same calls with nothing wrong are accepted
    torch.cuda.synchronize()
    for t in (y, z, dx, dw, db):
        assert not bool((t == 7.0).all())
