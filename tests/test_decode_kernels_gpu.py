"""The kernels that run once per generated token — cst_dec_self_attn, cst_dec_cross_attn (VALU kernel and the matrix-core kernel),
cst_dec_ln_q_cross_attn, cst_dec_linear / cst_dec_ln_linear, cst_dec_embed — on a real MI355X against the fp64 restatements of
decode_ref.py, under ITS per-element bounds (counted from the kernels' operation sequences; test_decode_ref_cpu.py shows that a faithful
fp32 evaluation stays inside them and that every listed defect leaves them).  No element is exempt.  What is exact is compared with
torch.equal: the cache append, untouched cache slots and output padding, a second launch, the no-op when *step > max_len.  The shapes
are the smallest that reach each path (decode_ref.py lists them); bsz = 3 throughout.

Every comparison prints `RATIO <kernel> <quantity> <dtype> ... worst err/bound`, and the module prints the worst ratio per kernel,
quantity and dtype at its end (pytest -s).  test_ab_switches runs the cross-attention and linear cases again under each documented A/B
switch (read once per process), one fresh child process after the other."""
import os
import subprocess
import sys
from importlib import import_module

import pytest
import torch

import decode_ref as R
from conftest import ROOT, load_pkg

pytestmark = pytest.mark.gpu
F, B = R.F, R.B
WORST = {}
MAX_LEN, STEP, LATE = 20, 3, 99


def _env_int(name, allowed):
    v = os.environ.get(name)
    return int(v) if v is not None and v.isdigit() and int(v) in allowed else 0


# the switches of this process, as the launchers read them
VALU_ONLY = os.environ.get("CST_DEC_CROSS_VALU") is not None
CROSS_NW = 8 if _env_int("CST_DEC_CROSS_NW", (8,)) else 4
LIN_NW = _env_int("CST_DEC_LINEAR_NW", (4, 8, 16))


@pytest.fixture(scope="module")
def KL():
    load_pkg()
    yield import_module("chimera-st_amd.kernels"), import_module("chimera-st_amd.lib")
    print()
    for key in sorted(WORST):
        print("WORST %-22s %-10s %-5s %.3f" % (key + (WORST[key],)))


def within(got, ref, bound, key, what=""):
    """key = (kernel, quantity, dtype name)."""
    got = got.detach().to(ref.device)
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(bound).all()), "%s: the reference is not finite" % (key,)
    assert bool(torch.isfinite(got.float()).all()), "%s %s: non-finite output" % (key, what)
    ratio, bad = R.worst_ratio(got, ref, bound)
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print("RATIO %-16s %-8s %-5s %-44s worst err/bound %.3f" % (key + (what, ratio)))
    assert bad == 0, "%s %s: %d of %d elements outside the bound, worst err/bound %.3f" % (key, what, bad, got.numel(), ratio)


def cu(*ts):
    return [None if t is None else t.cuda() for t in ts]


def istep(v):
    return torch.tensor([v], dtype=torch.int32, device="cuda")


# ------------------------------------------------------------------------------------------------------------------------------------
# cross attention
# ------------------------------------------------------------------------------------------------------------------------------------
CROSS_CASES = sorted(set(R.VALU_CASES) | set(R.MC_CASES), key=lambda c: (R.NAME[c[0]],) + c[1:])


def _route(c):
    return R.cross_route(c[0], c[1], c[4], VALU_ONLY)


def _cross_launch(L, q, kx, vx, kpm, out, step, beam, scale):
    Bn, H, S, D = kx.shape
    L.check(L.load().cst_dec_cross_attn(L.ptr(q), L.ptr(kx), L.ptr(vx), L.ptr(kpm), L.ptr(out), L.ptr(step), MAX_LEN, Bn, beam, H, D, S, scale,
                                        L.dtype_code(q.dtype), L.stream_ptr()), "cst_dec_cross_attn")


@pytest.mark.parametrize("case", CROSS_CASES, ids=["%s-%s" % (_route(c), R.cross_id(c)) for c in CROSS_CASES])
def test_cross_attn(KL, case):
    """Four masks (none, suffix, prefix, scattered) on planted logits: sentence 1 climbs by 17 log2 units per tile of a wave, sentence 2
    has a one-hot row whose key sits in wave 3's last tile.  The route is the launcher's own choice, restated (R.cross_route)."""
    _, L = KL
    dt, D, H, S, beam = case
    route = _route(case)
    assert route == ("mc" if dt == B and D == 64 and beam <= 32 and not VALU_ONLY else "valu")
    q, kx, vx, scale = R.cross_inputs(S, beam, H, D, dt)
    qd, kxd, vxd = cu(q, kx, vx)
    for mk in R.MASKS:
        kpm = R.cross_mask(S, mk)
        r = R.cross64(q, kx, vx, kpm, scale, beam, route, CROSS_NW)
        kd = None if kpm is None else kpm.cuda()
        out = torch.full((R.BSZ * beam, H * D), 7.0, dtype=dt, device="cuda")
        _cross_launch(L, qd, kxd, vxd, kd, out, istep(STEP), beam, scale)
        within(out.cpu(), r["out"], r["bound"], ("dec_cross_" + route, "out", R.NAME[dt]), "%s %s" % (R.cross_id(case), mk))
        again = torch.full_like(out, 7.0)
        _cross_launch(L, qd, kxd, vxd, kd, again, istep(STEP), beam, scale)
        assert torch.equal(out, again), "a second launch gives other bits"
        _cross_launch(L, qd, kxd, vxd, kd, again, istep(LATE), beam, scale)
        assert torch.equal(out, again), "past max_len the launch must be a no-op"


ALL_MASKED = [(B, 64, 2, 97, 5), (B, 64, 2, 97, 33), (F, 64, 2, 97, 5), (B, 32, 3, 33, 9), (F, 32, 3, 33, 1)]


@pytest.mark.parametrize("case", ALL_MASKED, ids=["%s-%s" % (_route(c), R.cross_id(c)) for c in ALL_MASKED])
def test_cross_attn_all_masked_sentence_is_plus_zero(KL, case):
    """A sentence whose every key is masked: its rows come back as +0 on both routes (a NaN row would stay in the state of a replayed
    graph); the other sentences keep their bound."""
    _, L = KL
    dt, D, H, S, beam = case
    route = _route(case)
    q, kx, vx, scale = R.cross_inputs(S, beam, H, D, dt)
    kpm = R.cross_mask(S, "suffix").clone()
    kpm[1] = 1
    out = torch.full((R.BSZ * beam, H * D), 7.0, dtype=dt, device="cuda")
    _cross_launch(L, *cu(q, kx, vx, kpm), out, istep(STEP), beam, scale)
    out = out.cpu()
    dead = out[beam:2 * beam]
    assert bool((dead == 0).all()) and not bool(torch.signbit(dead).any()), "rows of the all-masked sentence are not +0"
    live = torch.cat([torch.arange(beam), torch.arange(2 * beam, 3 * beam)])
    kpm[1] = 0
    r = R.cross64(q, kx, vx, kpm, scale, beam, route, CROSS_NW)
    within(out[live], r["out"][live], r["bound"][live], ("dec_cross_" + route, "out", R.NAME[dt]), "%s beside an all-masked sentence" % R.cross_id(case))


@pytest.mark.parametrize("case", R.QX_CASES, ids=["qx-" + R.qx_id(c) for c in R.QX_CASES])
def test_ln_q_cross_attn(KL, case):
    """LayerNorm + query projection + cross attention in one launch: K = 256 / 512 (one / two K iterations of a wave), ldx > C, rows of
    x whose scores spread with a standard deviation of 2 to 3, the same four masks."""
    _, L = KL
    eng = import_module("chimera-st_amd.decode_engine").BeamDecodeEngine
    H, beam, S = case
    p = R.qx_inputs(H, beam, S)
    C = p["C"]
    x, wfrag, sg, sb, kx, vx = cu(p["x"], eng.fragment_major(p["Wg"], H), p["sg"], p["sb"], p["kx"], p["vx"])
    lib = L.load()

    def launch(kd, out, step):
        L.check(lib.cst_dec_ln_q_cross_attn(L.ptr(x), x.stride(0), L.ptr(wfrag), L.ptr(sg), L.ptr(sb), R.LN_EPS, L.ptr(kx), L.ptr(vx), L.ptr(kd), L.ptr(out),
                                            L.ptr(step), MAX_LEN, R.BSZ, beam, H, 64, S, p["scale"], L.dtype_code(B), L.stream_ptr()), "cst_dec_ln_q_cross_attn")

    assert x.stride(0) > C
    for mk in R.MASKS:
        kpm = R.cross_mask(S, mk)
        r = R.qx64(p, kpm, beam)
        kd = None if kpm is None else kpm.cuda()
        out = torch.full((R.BSZ * beam, C), 7.0, dtype=B, device="cuda")
        launch(kd, out, istep(STEP))
        within(out.cpu(), r["out"], r["bound"], ("dec_ln_q_cross", "out", "bf16"), "%s %s" % (R.qx_id(case), mk))
        again = torch.full_like(out, 7.0)
        launch(kd, again, istep(STEP))
        assert torch.equal(out, again)
        launch(kd, again, istep(LATE))
        assert torch.equal(out, again)


# ------------------------------------------------------------------------------------------------------------------------------------
# self-attention
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,D", R.SELF_CASES, ids=["%s-D%d" % (R.NAME[dt], D) for dt, D in R.SELF_CASES])
def test_self_attn(KL, dt, D):
    """rows = 5, H = 3 (15 waves: the last workgroup is partly idle); the steps on both sides of each configuration's own batch of
    KPI * UNR keys and max_len itself; a shuffled ancestry whose other parity names other rows; a dominant early key in head 1."""
    _, L = KL
    lib = L.load()
    bk, max_len, steps = R.self_geometry(dt, D)
    rows, H = R.SELF_ROWS, R.SELF_H
    assert (rows * H) % 4 != 0 and max_len <= 4000

    def launch(qkv, kc, vc, anc, step, out):
        L.check(lib.cst_dec_self_attn(L.ptr(qkv), L.ptr(kc), L.ptr(vc), L.ptr(anc), L.ptr(step), L.ptr(out), rows, H, D, max_len, D ** -0.5,
                                      L.dtype_code(dt), L.stream_ptr()), "cst_dec_self_attn")

    for s in steps:
        qkv, kc, vc, anc, scale = R.self_inputs(dt, D, s)
        r = R.self64(qkv, kc, vc, anc, s, scale)
        qd, kd, vd, ad = cu(qkv, kc, vc, anc)
        out = torch.full((rows, H * D), 7.0, dtype=dt, device="cuda")
        launch(qd, kd, vd, ad, istep(s), out)
        within(out.cpu(), r["out"], r["bound"], ("dec_self_attn", "out", R.NAME[dt]), "D%d s=%d" % (D, s))
        assert torch.equal(kd.cpu(), r["kc"]) and torch.equal(vd.cpu(), r["vc"]), "the append, or a slot that must stay untouched (s=%d)" % s
        again = torch.full_like(out, 7.0)
        launch(qd, kd, vd, ad, istep(s), again)
        assert torch.equal(out, again) and torch.equal(kd.cpu(), r["kc"]) and torch.equal(vd.cpu(), r["vc"])
    kd, vd = cu(kc, vc)
    launch(qd, kd, vd, ad, istep(max_len + 1), again)
    assert torch.equal(out, again) and torch.equal(kd.cpu(), kc) and torch.equal(vd.cpu(), vc), "past max_len the launch must be a no-op"


# ------------------------------------------------------------------------------------------------------------------------------------
# Linear, LayerNorm-folded Linear
# ------------------------------------------------------------------------------------------------------------------------------------
LIN_COMBOS = [("none", True, False), ("relu", False, True), ("gelu", True, True)]    # (activation, bias, residual)


@pytest.mark.parametrize("ln", [False, True], ids=["plain", "ln"])
@pytest.mark.parametrize("case", R.LIN_CASES, ids=["linear-" + R.lin_id(c) for c in R.LIN_CASES])
def test_linear(KL, case, ln):
    """Every instantiation the default dispatch reaches, LayerNorm fold off and on; ldx > K, a residual with ldr != N, ldy = N + 8 and
    N + 1 (the second takes the scalar stores); M = 81 / 161 put ONE row into the last row tile.  The path is asserted first: wg1, nw and
    steps restated from the launcher, so that a change of the dispatch cannot silently empty a case."""
    _, L = KL
    lib = L.load()
    name, M, N, K = case
    ty, nw = (M + 79) // 80, (LIN_NW or 8)
    wg1 = (N + 15) // 16 * ty
    while nw > 4 and K % (nw * 64):
        nw >>= 1
    if wg1 > 1024:
        nt, nw = 4, 4
    elif wg1 > 320:
        nt, nw = 2, (8 if nw == 16 else nw)
    else:
        nt = 1
    steps = K // nw // 32
    un = 2 if nt == 4 else (4 if nw == 4 or steps % 4 == 0 else 2)
    d = R.lin_dispatch(M, N, K, LIN_NW)
    assert (d["nt"], d["un"], d["nw"], d["steps"], d["wg1"]) == (nt, un, nw, steps, wg1)
    if not LIN_NW:
        assert d["name"] == name, d
    assert (M - 1) % 80 == 0 or M == 80
    p = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in R.lin_inputs(M, N, K, ln).items()}
    code = {"none": L.ACT_NONE, "relu": L.ACT_RELU, "gelu": L.ACT_GELU}

    def launch(y, act, hb, hr, step):
        x, r = p["x"], (p["resid"] if hr else None)
        if ln:
            L.check(lib.cst_dec_ln_linear(L.ptr(x), L.ptr(p["W"]), L.ptr(p["sg"]), L.ptr(p["sb"]), R.LN_EPS, L.ptr(r), L.ptr(y), M, N, K, x.stride(0),
                                          r.stride(0) if hr else 0, y.stride(0), code[act], L.ptr(step), MAX_LEN, L.dtype_code(B), L.stream_ptr()), "cst_dec_ln_linear")
        else:
            L.check(lib.cst_dec_linear(L.ptr(x), L.ptr(p["W"]), L.ptr(p["bias"]) if hb else None, L.ptr(r), L.ptr(y), M, N, K, x.stride(0),
                                       r.stride(0) if hr else 0, y.stride(0), code[act], L.ptr(step), MAX_LEN, L.dtype_code(B), L.stream_ptr()), "cst_dec_linear")

    assert p["x"].stride(0) > K and p["resid"].stride(0) != N
    for act, hb, hr in LIN_COMBOS:
        r = R.lin64(p, ln, act, hb, hr, nw)        # (on the device: up to 161 x 5472 x 1024)
        for ldy in (N + 8, N + 1):
            assert ldy == N + 8 or ldy % 4 != 0      # the kernel packs four columns only if ((ldy | n) & 3) == 0: N + 1 takes the scalar stores
            y = torch.full((M, ldy), 7.0, dtype=B, device="cuda")
            launch(y, act, hb, hr, istep(STEP))
            within(y[:, :N], r["y"], r["bound"], ("dec_ln_linear" if ln else "dec_linear", "y", "bf16"),
                   "%s %s bias=%d resid=%d ldy=N+%d nw=%d" % (R.lin_id(case), act, hb, hr, ldy - N, nw))
            assert bool((y[:, N:] == 7.0).all()), "written behind the row"
            again = torch.full_like(y, 7.0)
            launch(again, act, hb, hr, istep(STEP))
            assert torch.equal(y, again)
            launch(again, act, hb, hr, istep(LATE))
            assert torch.equal(y, again), "past max_len the launch must be a no-op"


# ------------------------------------------------------------------------------------------------------------------------------------
# embed
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F, B], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", R.EMBED_CS)
def test_embed(KL, C, dt):
    """Exact.  C = 8, C below and above one pass of the 256 threads (no multiple of 256); the position table has pad + 1 + max_len - 3
    rows, so the last steps clamp to its last row."""
    _, L = KL
    rows, max_len, V, pad, scale = 7, 21, 50, 1, 3.25
    g = R._gen(81 + C)
    E = torch.randn(V, C, generator=g).to(dt).cuda()
    P = torch.randn(pad + 1 + max_len - 3, C, generator=g).cuda()
    tokens = torch.randint(0, V, (2, rows, max_len + 2), generator=g).cuda()
    x = torch.full((rows, C), 7.0, dtype=dt, device="cuda")
    clamped = 0
    for s in (0, 1, 6, max_len - 4, max_len - 3, max_len):
        clamped += pad + 1 + s >= P.shape[0]
        L.check(L.load().cst_dec_embed(L.ptr(tokens), L.ptr(istep(s)), L.ptr(E), L.ptr(P), scale, pad, L.ptr(x), rows, C, max_len, P.shape[0],
                                       L.dtype_code(dt), L.stream_ptr()), "cst_dec_embed")
        assert torch.equal(x, R.embed_ref(tokens, s, E, P, scale, pad, max_len)), (C, s)
    assert clamped == 2
    before = x.clone()
    L.check(L.load().cst_dec_embed(L.ptr(tokens), L.ptr(istep(max_len + 1)), L.ptr(E), L.ptr(P), scale, pad, L.ptr(x), rows, C, max_len, P.shape[0],
                                   L.dtype_code(dt), L.stream_ptr()), "cst_dec_embed")
    assert torch.equal(x, before)


# ------------------------------------------------------------------------------------------------------------------------------------
# the documented A/B switches, each read once per process: one fresh child process per setting
# ------------------------------------------------------------------------------------------------------------------------------------
AB = [("CST_DEC_CROSS_VALU", "1", "cross_attn"),                 # bf16 / D = 64 / beam <= 32 reach the VALU kernel
      ("CST_DEC_CROSS_SLOTS", "3", "mc or qx"), ("CST_DEC_CROSS_SLOTS", "4", "mc or qx"),
      ("CST_DEC_CROSS_NW", "8", "valu"),
      ("CST_DEC_LINEAR_NW", "4", "linear"), ("CST_DEC_LINEAR_NW", "16", "linear")]
AB_NAMES = sorted({n for n, _, _ in AB})


def test_ab_switches():
    """This module's cross-attention and linear cases under each setting, one child after the other, never two at a time; the first child
    that does not exit cleanly ends the test (nothing more is started on the GPU after it)."""
    assert not any(n in os.environ for n in AB_NAMES), "run the parent without the A/B switches"
    print()
    for name, value, select in AB:
        env = dict(os.environ)
        env[name] = value
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-s", "-x", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                            "(%s) and not ab_switches" % select], capture_output=True, text=True, timeout=240, cwd=ROOT, env=env)
        for line in r.stdout.splitlines():
            if "WORST" in line:
                print("AB %s=%s %s" % (name, value, line[line.index("WORST"):]))
        tail = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
        print("AB %s=%s exit %d: %s" % (name, value, r.returncode, tail))
        assert r.returncode == 0, "%s=%s:\n%s\n%s" % (name, value, r.stdout[-3000:], r.stderr[-1500:])
        assert " passed" in tail and "failed" not in tail
