"""The bounds of conv0_gn_ref.py are sound, sharp and not vacuous, shown without a GPU.
  * faithful: at every case of test_conv0_gn_gpu.py the fp32 emulation of the route the case takes lies inside every bound;
  * defects: each listed defect leaves the bound of the output named in DEFECT_AT, at the case named there, where the faithful emulation
    has just passed;
  * autograd: the closed form of the backward equals torch.autograd through an fp64 conv1d -> group_norm -> erf-GELU to 1e-10;
  * caps: conditions on the reference alone (no kernel, no emulation) that keep the bounds from being vacuous;
  * the LDS envelope: the cases named largest / smallest in conv0_gn_ref.py are that, by the launch code's own formulas.

Why a defect shows where DEFECT_AT says (reasoning, not a measured figure).  The bounds are linear in the sum of the absolute terms, the
sums over frames of a random dy are random walks: a dropped TERM of the closed form shows where the sums are short (L = 15), a dropped
frame or block where one frame's |dz| ~ 0.4 is large against c u sum |dz| (fp32 storage).
  unbiased_variance         rstd: a factor sqrt(L / (L - 1)), 2.4e-4 at L = 2049, against ~ 30 u of the randn utterance
  eps_outside_sqrt          rstd of the `tiny` utterance: 1 / (sd + eps) against 1 / sqrt(var + eps), var far below eps
  stats_over_live_frames_only   rstd: the `spike` utterance's statistics over its 7 live frames
  gram_lower_triangle_not_mirrored   gram itself (the lower triangle is missing), and with it rstd
  tap_k_minus_1_dropped     y and dW
  no_s1_term / no_s2_term / mean_m_term_missing   dW at L = 15: the terms are of the size of the result (the last one in the `offset` utterance)
  gelu_prime_is_cdf         dbeta
  last_frame_dropped        gram (the Gram pass) and dbeta (the backward pass)
  second_block_dropped      gram (256 of 512 lanes) and dbeta (frame 2048 of the four utterances whose limit lies above it)
  utterance_32_dropped      dbeta at B = 33
  limit_frame_counted       dbeta when dy is NOT zero in the limit frame (the reference zeroes dz there whatever dy holds)
  lo_half_dropped           dgamma with a one-signed dy, C = 512, L = 64: truncation errs one way, so u of the `offset` utterance is shifted
                            by 2^-8 of sum w x: with the equal-tap filter that is 0.015 in uhat on every frame, and s2 moves by 0.015 s1,
                            which a one-signed dy makes 0.015 sum |dz|, against A' |dy uhat| = 6e-4 per term.  (In r the loss, 2^-8 per term
                            on average, is of the size of the bf16 rounding of dz that the bound must allow: r cannot show it.)
  s2_from_rounded_dz        dgamma at L = 3, B = 1: one rounding of 2^-9 |dz| in a sum of three terms against A' = 6.2e-4 |dy|
  ones_row_is_tap_10        dbeta: sum dz x[s t + 10] instead of sum dz"""
import pytest
import torch

import conv0_gn_ref as R
import norm_ref as N

FWD_OUT = ("y", "mean", "rstd", "gram")
BWD_OUT = ("dW", "dgamma", "dbeta")


def _in(got, ref, bound, what):
    ratio, bad = R.worst_ratio(got, ref, bound)
    print("clean %-52s worst err/bound %.3f" % (what, ratio))
    assert bad == 0, "%s: the faithful emulation leaves the bound on %d elements (worst ratio %.3f)" % (what, bad, ratio)


def _out(got, ref, bound, what):
    err = (got.double() - ref.double()).abs()
    o = ~(err <= bound.expand_as(err))
    print("defect %-60s outside on %d of %d" % (what, int(o.sum()), o.numel()))
    assert int(o.sum()) >= 1, what + ": the defect stays inside the bound"


def _live_y(c, t):
    return t[R.live_of(c["limit"], c["Bn"], c["L"])]


def _forward(c, defect=None):
    a = (c["wav"], c["w"], c["gamma"], c["beta"], c["k"], c["stride"])
    return dict(zip(FWD_OUT, R.fwd_emulate32(*a, limit=c["limit"], defect=defect, generic=c["route"] == "generic")))


def _backward(c, st, defect=None, dy=None):
    a = (c["dy"] if dy is None else dy, c["wav"], c["w"], c["gamma"], c["beta"], st["mean"], st["rstd"], st["gram"], c["k"], c["stride"])
    return dict(zip(BWD_OUT, R.bwd_emulate(c["route"], *a, limit=c["limit"], defect=defect)))


def _refs(c, st, want_fwd=True):
    r = R.fwd64(c["wav"], c["w"], c["gamma"], c["beta"], c["k"], c["stride"]) if want_fwd else None
    b = R.fwd_bounds(r, c["dt"]) if want_fwd else None
    rb = R.bwd64(c["dy"], c["wav"], c["w"], c["gamma"], c["beta"], st["mean"], st["rstd"], st["gram"], c["k"], c["stride"], c["limit"])
    return r, b, rb, R.bwd_bounds(rb, c["dt"], c["route"])


def _check_fwd(c, f, r, b, tag):
    _in(_live_y(c, f["y"]), _live_y(c, r["y"]), _live_y(c, b["y"]), tag + " y")
    for n in FWD_OUT[1:]:
        _in(f[n], r[n], b[n], tag + " " + n)


def _caps(c, r, b, rb, bb, tag):
    """The conditions of the issue, on the reference alone.  For |z| > 6 the bf16 polynomial's allowance is not the constant A_GELU but
    norm_ref.a_gelu(z) = |z| (A / 4 + 3.2e-5) — the error the clamped polynomial has there: the frames that carry the spike of the
    `spike` utterance have |z| up to sqrt(L) |gamma|, and the cap of y is stated with a_gelu(z), which IS A_GELU on [-6, 6]."""
    dt = c["dt"]
    nz = c["w"].float().abs().sum(1) > 0
    rel = (b["rstd"] / r["rstd"])[:, nz]
    assert float(rel.max()) <= 1e-3, "%s: bound(rstd) / rstd = %.3e" % (tag, float(rel.max()))
    ycap = 4.0 * (R.UBF * r["y"].abs() + N.a_gelu(r["z"], dt)) if dt == R.B else 1e-4 * r["y"].abs().clamp_min(1.0)
    yr = float((b["y"] / ycap).max())
    assert yr <= 1.0, "%s: bound(y) is %.3f of its cap" % (tag, yr)
    cap = 1e-2 if dt == R.B else 1e-4
    worst = {}
    for n in BWD_OUT:
        t = rb["terms"][n]
        assert bool((bb[n] <= cap * t + N.ETA * c["Bn"] * c["L"] * 2).all()), "%s: bound(%s) above %.0e of its terms" % (tag, n, cap)
        worst[n] = float(torch.where(t > 0, bb[n] / t.clamp_min(1e-300), torch.zeros_like(t)).max())
    print("caps   %-52s bound(rstd)/rstd %.2e  bound(y)/cap %.3f  bound/terms dW %.2e dgamma %.2e dbeta %.2e"
          % (tag, float(rel.max()), yr, worst["dW"], worst["dgamma"], worst["dbeta"]))
    kd = torch.arange(c["Bn"]) % 8 == R.OFFSET
    if bool(kd.any()):
        cond = (r["mean"] ** 2 / r["var"].clamp_min(1e-300))[kd][:, nz]
        print("CONDITIONING %-46s offset kind: mean^2/var up to %.1f, terms/var up to %.1f, bound(rstd)/rstd up to %.2e"
              % (tag, float(cond.max()), float((b["terms_var"] / r["var"].clamp_min(1e-300))[kd][:, nz].max()), float((b["rstd"] / r["rstd"])[kd][:, nz].max())))


@pytest.mark.parametrize("cs", R.ALL_CASES, ids=[c[0] for c in R.ALL_CASES])
def test_faithful_and_caps(cs):
    c = R.case(*cs)
    f = _forward(c)
    r, b, rb, bb = _refs(c, f)
    _check_fwd(c, f, r, b, cs[0])
    o = _backward(c, f)
    for n in BWD_OUT:
        _in(o[n], rb[n], bb[n], cs[0] + " " + n)
    _caps(c, r, b, rb, bb, cs[0])
    z = torch.arange(c["Bn"]) % 8 == R.ZERO
    if bool(z.any()):   # the zero utterance: variance exactly 0, y = GELU(beta)
        assert bool((r["var"][z] == 0).all()) and bool((r["mean"][z] == 0).all()) and bool((f["mean"][z] == 0).all())
        assert bool((f["rstd"][z] == torch.tensor(1.0 / N.f32(R.EPS) ** 0.5, dtype=torch.float32)).all())


def test_mfma_cases_also_hold_on_the_register_emulation():
    """CST_CONV0_NO_MFMA sends bf16 C = 512 to conv0_bwd_reg_kernel<bf16_t, 10>: its emulation under the `reg` bounds at the same inputs."""
    cs = R.CASES[2]
    c = dict(R.case(*cs), route="reg")
    f = _forward(c)
    _, _, rb, bb = _refs(c, f, want_fwd=False)
    o = _backward(c, f)
    for n in BWD_OUT:
        _in(o[n], rb[n], bb[n], cs[0] + " (register route) " + n)


# ------------------------------------------------------------------------------------------------------------------------------------
# defects
# ------------------------------------------------------------------------------------------------------------------------------------
BIG_F32 = R._c(10, 5, 8, R.F, 2049)          # a case of the GPU list
SMALL_F32 = R._c(10, 5, 8, R.F, 15)
B33 = R.CASES[2]                             # k10 s5 C512 bf16 L15 B33, the MFMA route
MFMA_POS = R._c(10, 5, 512, R.B, 64, 2)      # dy made one-signed below
MFMA_L3 = R._c(10, 5, 512, R.B, 3, 1)
DEFECT_AT = {
    "unbiased_variance": (BIG_F32, ("rstd",)),
    "eps_outside_sqrt": (BIG_F32, ("rstd",)),
    "stats_over_live_frames_only": (BIG_F32, ("rstd",)),
    "gram_lower_triangle_not_mirrored": (BIG_F32, ("gram", "rstd")),
    "tap_k_minus_1_dropped": (SMALL_F32, ("y", "dW")),
    "no_s1_term": (SMALL_F32, ("dW",)),
    "no_s2_term": (SMALL_F32, ("dW",)),
    "mean_m_term_missing": (SMALL_F32, ("dW",)),
    "gelu_prime_is_cdf": (SMALL_F32, ("dbeta",)),
    "last_frame_dropped": (BIG_F32, ("gram", "dbeta")),
    "second_block_dropped": (BIG_F32, ("gram", "dbeta")),
    "utterance_32_dropped": (B33, ("dbeta",)),
    "limit_frame_counted": (SMALL_F32, ("dbeta",)),
    "lo_half_dropped": (MFMA_POS, ("dgamma",)),
    "s2_from_rounded_dz": (MFMA_L3, ("dgamma",)),
    "ones_row_is_tap_10": (B33, ("dbeta",)),
}


def test_every_defect_has_a_case():
    assert set(DEFECT_AT) == set(R.DEFECTS) | set(R.MFMA_DEFECTS)


@pytest.mark.parametrize("defect", list(DEFECT_AT))
def test_defect_leaves_its_bound(defect):
    cs, outs = DEFECT_AT[defect]
    c = dict(R.case(*cs))
    if cs is MFMA_POS:
        c["dy"] = c["dy"].abs()
    f = _forward(c)
    r, b, rb, bb = _refs(c, f)
    _check_fwd(c, f, r, b, cs[0])
    o = _backward(c, f)
    for n in BWD_OUT:
        _in(o[n], rb[n], bb[n], cs[0] + " " + n)
    fd = _forward(c, defect) if (defect in R.DEFECTS and any(n in FWD_OUT for n in outs)) else None
    dy = None
    if defect == "limit_frame_counted":   # a gradient that breaks the contract in the limit frame alone
        dy = c["dy"].clone()
        for bi in range(c["Bn"]):
            if int(c["limit"][bi]) < c["L"]:
                dy[bi, int(c["limit"][bi])] = 1.0
    od = _backward(c, f, defect, dy) if any(n in BWD_OUT for n in outs) else None
    for n in outs:
        tag = "%s @ %s: %s" % (defect, cs[0], n)
        if n == "y":
            _out(_live_y(c, fd["y"]), _live_y(c, r["y"]), _live_y(c, b["y"]), tag)
        elif n in FWD_OUT:
            _out(fd[n], r[n], b[n], tag)
        else:
            _out(od[n], rb[n], bb[n], tag)


# ------------------------------------------------------------------------------------------------------------------------------------
# the closed form against autograd
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,stride,C,L", [(4, 2, 8, 9), (10, 5, 16, 23), (1, 1, 8, 5)])
def test_closed_form_equals_autograd(k, stride, C, L):
    Bn = 8
    wav, w, gamma, beta = R.make_inputs(Bn, R.S_of(k, stride, L), C, k, stride, R.F)
    limit = R.limits_of(Bn, L).clamp_max(L - 2)
    limit[0] = R.NOLIMIT
    dy = R.make_dy(Bn, L, C, R.F, limit).double()
    r = R.fwd64(wav, w, gamma, beta, k, stride)
    wd, gd, bd = (t.double().requires_grad_(True) for t in (w, gamma, beta))
    u = torch.nn.functional.conv1d(wav.double()[:, None], wd[:, None], stride=stride)            # [B, C, L]
    y = torch.nn.functional.gelu(torch.nn.functional.group_norm(u, C, gd, bd, N.f32(R.EPS))).transpose(1, 2)
    assert float((y.detach() - r["y"]).abs().max()) <= 1e-10 * max(1.0, float(y.detach().abs().max()))
    (y * dy).sum().backward()
    rb = R.bwd64(dy, wav, w, gamma, beta, r["mean"], r["rstd"], r["gram"], k, stride, limit)   # the exact statistics handed in
    for n, g in (("dW", wd.grad), ("dgamma", gd.grad), ("dbeta", bd.grad)):
        rel = float((rb[n] - g).abs().max() / g.abs().max())
        print("autograd k%d s%d C%d L%d %-6s max |closed form - autograd| / max |autograd| = %.2e" % (k, stride, C, L, n, rel))
        assert rel <= 1e-10, n


# ------------------------------------------------------------------------------------------------------------------------------------
# the LDS envelope
# ------------------------------------------------------------------------------------------------------------------------------------
def test_lds_envelope_cases_are_the_edge():
    """Among the generic (k, stride, C) with C <= 2048, k <= 16: LDS_*_MAX fit 160 KiB and no accepted triple asks for more; LDS_*_REFUSED
    do not fit and no refused triple asks for less; the *_WIDE ones fit."""
    assert R.fwd_lds(*R.LDS_FWD_WIDE) <= R.LDS_MAX and R.bwd_lds(*R.LDS_BWD_WIDE, R.F) <= R.LDS_MAX
    for dt in (R.F, R.B):
        fm, fr = R.fwd_lds(*R.LDS_FWD_MAX), R.fwd_lds(*R.LDS_FWD_REFUSED)
        bm, br = R.bwd_lds(*R.LDS_BWD_MAX, dt), R.bwd_lds(*R.LDS_BWD_REFUSED, dt)
        assert fm <= R.LDS_MAX < fr and bm <= R.LDS_MAX < br
        fa = [R.fwd_lds(k, s, C) for k in range(1, 17) for s in range(1, 700) for C in range(8, 2049, 8) if not R.is_reg(k, C)]
        ba = [R.bwd_lds(k, s, C, dt) for k in range(1, 17) for s in range(1, 30) for C in range(8, 2049, 8) if not R.is_reg(k, C)]
        assert max(v for v in fa if v <= R.LDS_MAX) == fm and min(v for v in fa if v > R.LDS_MAX) == fr
        assert max(v for v in ba if v <= R.LDS_MAX) == bm and min(v for v in ba if v > R.LDS_MAX) == br
    # the figures of the issue
    assert R.bwd_lds(16, 7, 512, R.F) == 4 * (16 * 512 + 4 * 512 + 2048 * 7 + 16) > 96 * 1024
    assert R.bwd_lds(3, 2, 2048, R.F) > 72 * 1024 and R.bwd_lds(16, 8, 2048, R.F) > R.LDS_MAX


def test_lds_refusals_happen_before_any_device_call():
    """The guard sits in argument validation: shown here on addresses that are never followed.  Also the register routes, whose staged
    span outgrows a CU's LDS from stride 20 (backward) and 320 (forward) on; the MFMA kernel fits up to stride 16 and hands over to the
    register kernel behind that."""
    assert R.route_of(10, 512, R.B, 16) == "mfma" and R.route_of(10, 512, R.B, 17) == "reg" and R.mfma_lds(16) <= R.LDS_MAX < R.mfma_lds(17)
    import os
    import __graft_entry__ as ge
    from conftest import load_pkg
    lib = load_pkg().lib
    if not os.path.exists(lib.LIB_PATH):
        ge.build()
    c, last, A, L = lib.load(), lib.load().cst_last_error, 0x10000, 37

    def fwd(k, s, C, dt):
        return c.cst_conv0_gn_gelu_fwd(A, A, A, A, A, A, A, A, A, None, 1, R.S_of(k, s, L), C, k, s, R.EPS, lib.dtype_code(dt), None)

    def bwd(k, s, C, dt):
        return c.cst_conv0_gn_gelu_bwd(A, A, A, A, A, A, A, A, A, A, A, A, None, 1, R.S_of(k, s, L), C, k, s, lib.dtype_code(dt), None)
    for dt in (R.F, R.B):
        assert fwd(*R.LDS_FWD_REFUSED, dt) == -1 and b"needs 163844 bytes of LDS" in last()
        assert bwd(*R.LDS_BWD_REFUSED, dt) == -1 and b"needs 163844 bytes of LDS" in last()
        assert bwd(*R.LDS_FWD_MAX, dt) == -1 and b"bytes of LDS" in last()
        assert bwd(10, 20, 512, dt) == -1 and ("needs %d bytes of LDS" % R.bwd_lds(10, 20, 512, dt)).encode() in last()
        assert R.bwd_lds(10, 19, 512, dt) <= R.LDS_MAX < R.bwd_lds(10, 20, 512, dt) == 4 * (2048 * 20 + 10)
        assert fwd(10, 320, 512, dt) == -1 and ("needs %d bytes of LDS" % R.fwd_lds(10, 320, 512)).encode() in last()
        assert R.fwd_lds(10, 319, 512) <= R.LDS_MAX < R.fwd_lds(10, 320, 512)
