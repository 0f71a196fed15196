"""The bounds of norm_ref.py are sound and sharp, shown without a GPU.  For every input case of norm_ref.py and both dtypes:
  * the faithful fp32 emulation of each kernel lies inside the bound against fp64 on EVERY element;
  * every listed defect leaves the bound on at least one element of the rows (or of the output) it names, in the very case in which
    the faithful emulation has just passed;
  * the kernels' GELU formulas, restated in fp32 from csrc/cst_common.h, stay inside the constants stated there on [-6, 6].

Which rows a defect names (reasoning, not a measured figure):
  eps_outside_sqrt        rstd of the rows with variance ~ eps: 1 / (sd + eps) against 1 / sqrt(var + eps) differ by tens of per cent
  unbiased_variance       rstd of the N(0, 1) rows: a factor sqrt((C - 1) / C), at least 2.4e-4 at C = 2048, against ~ 30 u32
  one_pass_variance       rstd of the rows with mean 100, fp32: E[x^2] ~ 1e4 is rounded to 1e-3, the variance is 1e-2
  stats_of_rounded_sum    mean, bf16: the rounded sum's mean is off by ~ ubf |s| / sqrt(C) >= 8e-5, the bound is ~ 30 u32 |s| = 2e-6
  residual_missing...     sum_out itself
  no_xhat_term / no_mean_term / dres_not_added / gelu_prime_is_cdf     dx (du): terms of the size of the result
  dgamma_from_g           dgamma
  last_row_dropped        dgamma and dbeta: one row's |dy xhat| ~ 0.6 per column against chain * u32 * sum |terms|
  second_stride_iteration_dropped   dgamma / dbeta of the shapes with more rows than 4 * the block cap (elsewhere the defect does not exist)
  limit_row_not_zeroed    y from the limit on (the bound there is zero), and dbeta, which gains dy GELU'(beta) of those rows
  bias_missing / tap_k_minus_1_dropped   mean (every frame moves by the mean bias / by the tap's share)
  dbias_from_dz           dbias
Where a defect is NOT demanded (demanded() below is the one place that says so; test_every_defect_is_demanded_somewhere shows that each
defect of each kernel is still demanded in at least one shape and dtype):
  one_pass_variance       bf16: the mean-100 rows are stored as 100 or 100 +- 0.5, their variance is no longer small against E[x^2] ulp
  stats_of_rounded_sum    fp32 (the store does not round), and without a residual (nothing is stored)
  last_row_dropped        bf16 at 16413 rows: the GELU' polynomial's 6e-4 |dy| per row adds up to more than one row's term
  colsum(du) of the dropped-row / dropped-iteration defects   bf16: the constant and variance ~ eps rows have rstd ~ 300, |du| ~ 300
                          there, and one ordinary row is small against the bf16 bound of their sum; dgamma and dbeta are demanded
  second_stride_iteration_dropped   shapes with at most 4 * the block cap rows, and limits that leave the second iteration empty
  limit_row_not_zeroed    without a limit below L, or with no live row
  dres_not_added          without dres"""
import pytest
import torch

import norm_ref as R

DTS = [R.F, R.B]
IDS = ["f32", "bf16"]


def _in(got, ref, bound, what):
    ratio, bad = R.worst_ratio(got, ref, bound)
    print("clean %-28s worst err/bound %.3f" % (what, ratio))
    assert bad == 0, "%s: the faithful emulation leaves the bound on %d elements (worst ratio %.3f)" % (what, bad, ratio)


def demanded(defect, dt, big=False, with_res=True, with_dres=True, two_iterations=True, partial_limit=True):
    """Whether `defect` must leave the bound in a case of that description (module docstring)."""
    if defect == "one_pass_variance":
        return dt == R.F
    if defect == "stats_of_rounded_sum":
        return dt == R.B and with_res
    if defect == "residual_missing_from_sum_out":
        return with_res
    if defect == "dres_not_added":
        return with_dres
    if defect == "second_stride_iteration_dropped":
        return two_iterations
    if defect == "limit_row_not_zeroed":
        return partial_limit
    if defect == "last_row_dropped_gelu":
        return not (dt == R.B and big)
    return True


def _out(got, ref, bound, what, rows=None):
    err = (got.double() - ref.double()).abs()
    o = err > bound.expand_as(err)
    if rows is not None:
        o = o[rows]
    print("defect %-44s outside on %d of %d" % (what, int(o.sum()), o.numel()))
    assert int(o.sum()) >= 1, what + ": the defect stays inside the bound"
    return o


# ------------------------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ------------------------------------------------------------------------------------------------------------------------------------
LN_SHAPES = [(R.LN_ROWS, c) for c in R.LN_COLS] + [(rows, c) for rows in (R.LN_FWD_BIG, R.LN_BWD_BIG) for c in R.BIG_COLS]


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("with_res", [True, False], ids=["res", "nores"])
@pytest.mark.parametrize("rows,cols", LN_SHAPES)
def test_layernorm_forward(rows, cols, with_res, dt):
    x, res, gamma, beta, _, _ = R.ln_case(rows, cols, dt, with_res)
    r = R.ln_fwd64(x, res, gamma, beta, R.EPS)
    b = R.ln_fwd_bounds(r, dt)
    y, so, mu, rs = R.ln_fwd_emulate32(x, res, gamma, beta, R.EPS)
    tag = "ln fwd %s %dx%d " % (R.NAME[dt], rows, cols)
    _in(y, r["y"], b["y"], tag + "y")
    _in(mu, r["mean"], b["mean"], tag + "mean")
    _in(rs, r["rstd"], b["rstd"], tag + "rstd")
    if with_res:
        _in(so, r["sum"], b["sum"], tag + "sum")
    kd = R.kind_of(rows)
    const = kd == R.CONST
    assert bool((r["var"][const] == 0).all()) and bool((r["y"][const] == beta.double()[None]).all())
    plain = R.is_plain(kd)
    for defect in (() if heavy(rows, cols) else R.LN_FWD_DEFECTS):
        yd, sod, mud, rsd = R.ln_fwd_emulate32(x, res, gamma, beta, R.EPS, defect=defect)
        if defect == "eps_outside_sqrt":
            o = _out(rsd, r["rstd"], b["rstd"], tag + defect + " rstd", kd == R.TINY)
            assert bool(o.all())
            _out(yd, r["y"], b["y"], tag + defect + " y", kd == R.TINY)
        elif defect == "unbiased_variance":
            o = _out(rsd, r["rstd"], b["rstd"], tag + defect + " rstd", plain)
            assert bool(o.all())
        elif not demanded(defect, dt, with_res=with_res):
            print("defect %s not demanded here" % (tag + defect))
        elif defect == "one_pass_variance":
            _out(rsd, r["rstd"], b["rstd"], tag + defect + " rstd", kd == R.OFFSET)
        elif defect == "stats_of_rounded_sum":
            _out(mud, r["mean"], b["mean"], tag + defect + " mean", plain)
        else:
            assert defect == "residual_missing_from_sum_out"
            _out(sod, r["sum"], b["sum"], tag + defect + " sum")


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("with_dres", [True, False], ids=["dres", "nodres"])
@pytest.mark.parametrize("rows,cols", LN_SHAPES)
def test_layernorm_backward(rows, cols, with_dres, dt):
    x, res, gamma, beta, dy, dres = R.ln_case(rows, cols, dt, True)
    if not with_dres:
        dres = None
    _, s, mean, rstd = R.ln_fwd_emulate32(x, res, gamma, beta, R.EPS)
    r = R.ln_bwd64(dy, s, gamma, mean, rstd, dres)
    b = R.ln_bwd_bounds(r, dt)
    dx, dg, db = R.ln_bwd_emulate32(dy, s, gamma, mean, rstd, dres)
    tag = "ln bwd %s %dx%d " % (R.NAME[dt], rows, cols)
    _in(dx, r["dx"], b["dx"], tag + "dx")
    _in(dg, r["dgamma"], b["dgamma"], tag + "dgamma")
    _in(db, r["dbeta"], b["dbeta"], tag + "dbeta")
    two_iterations = rows > 4 * R.LN_BWD_CAP
    plain = R.is_plain(R.kind_of(rows))
    for defect in (("second_stride_iteration_dropped",) if heavy(rows, cols) else R.LN_BWD_DEFECTS):
        if not demanded(defect, dt, with_dres=with_dres, two_iterations=two_iterations):
            print("defect %s not demanded here" % (tag + defect))
            continue
        dxd, dgd, dbd = R.ln_bwd_emulate32(dy, s, gamma, mean, rstd, dres, defect=defect)
        if defect in ("no_xhat_term", "no_mean_term", "dres_not_added"):
            _out(dxd, r["dx"], b["dx"], tag + defect + " dx", plain)
        elif defect == "dgamma_from_g":
            _out(dgd, r["dgamma"], b["dgamma"], tag + defect + " dgamma")
        else:
            assert defect in ("last_row_dropped", "second_stride_iteration_dropped")
            _out(dgd, r["dgamma"], b["dgamma"], tag + defect + " dgamma")
            _out(dbd, r["dbeta"], b["dbeta"], tag + defect + " dbeta")


# ------------------------------------------------------------------------------------------------------------------------------------
# ln_gelu
# ------------------------------------------------------------------------------------------------------------------------------------
LG_SHAPES = [(R.LG_B, R.LG_L, c) for c in R.LG_COLS] + [(R.LG_B, R.LG_BIG_L, c) for c in R.BIG_COLS]


def heavy(rows, cols):
    """The two shapes with NV = 4 AND the grid-stride loops (17 M elements): the emulation is shown inside the bounds, and of the defects
    only the one that needs such a shape, the dropped second iteration, is run — the others do not depend on the row count and are
    demanded at 1032 columns in the small shape and at these row counts with 64 columns; the limits there are none and L / 3."""
    return rows * cols > 10_000_000


LG_PARAMS = [(Bn, L, C, w) for Bn, L, C in LG_SHAPES for w in ((None, "L/3") if heavy(Bn * L, C) else (None, "L", "L/3", "0"))]


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("Bn,L,C,which", LG_PARAMS)
def test_ln_gelu(Bn, L, C, which, dt):
    u, gamma, beta, dy = R.lg_case(Bn, L, C, dt)
    lim = R.lg_limit(Bn, L, which)
    r = R.ln_gelu_fwd64(u, gamma, beta, R.EPS, lim)
    b = R.ln_gelu_fwd_bounds(r, dt)
    y, mean, rstd = R.ln_gelu_fwd_emulate32(u, gamma, beta, R.EPS, lim)
    tag = "ln_gelu %s %dx%dx%d lim=%s " % (R.NAME[dt], Bn, L, C, which)
    _in(y, r["y"], b["y"], tag + "y")
    _in(mean, r["mean"], b["mean"], tag + "mean")
    _in(rstd, r["rstd"], b["rstd"], tag + "rstd")
    rb = R.ln_gelu_bwd64(dy, u, gamma, beta, mean, rstd, lim)
    bb = R.ln_gelu_bwd_bounds(rb, dt)
    out = R.ln_gelu_bwd_emulate32(dy, u, gamma, beta, mean, rstd, lim)
    names = ("du", "dgamma", "dbeta", "colsum")
    for n, o in zip(names, out):
        _in(o, rb[n], bb[n], tag + n)
    live = r["live"]
    nlive = int(live.sum())
    dead = (~live).view(Bn, L)
    if nlive < Bn * L:
        assert bool((y[dead] == 0).all()) and bool((out[0][dead] == 0).all())
    kd = R.kind_of(Bn * L).view(Bn, L)
    for defect in (() if heavy(Bn * L, C) else R.LG_FWD_DEFECTS):
        yd, md, rd = R.ln_gelu_fwd_emulate32(u, gamma, beta, R.EPS, lim, defect=defect)
        if nlive == 0 or not demanded(defect, dt, partial_limit=nlive < Bn * L):
            print("defect %s not demanded here" % (tag + defect))
        elif defect == "eps_outside_sqrt":
            assert bool(_out(rd, r["rstd"], b["rstd"], tag + defect + " rstd", (kd == R.TINY) & ~dead).all())
        elif defect == "unbiased_variance":
            assert bool(_out(rd, r["rstd"], b["rstd"], tag + defect + " rstd", R.is_plain(kd) & ~dead).all())
        elif defect == "one_pass_variance":
            _out(rd, r["rstd"], b["rstd"], tag + defect + " rstd", (kd == R.OFFSET) & ~dead)
        else:
            assert defect == "limit_row_not_zeroed"
            _out(yd, r["y"], b["y"], tag + defect + " y", dead)
    two_iterations = Bn * L > 4 * R.LG_BWD_CAP
    for defect in (("second_stride_iteration_dropped",) if heavy(Bn * L, C) else R.LG_BWD_DEFECTS):
        key = "last_row_dropped_gelu" if defect == "last_row_dropped" else defect
        if nlive == 0 or not demanded(key, dt, big=Bn * L > 100, two_iterations=two_iterations and which in (None, "L"), partial_limit=nlive < Bn * L):
            print("defect %s not demanded here" % (tag + defect))
            continue
        od = dict(zip(names, R.ln_gelu_bwd_emulate32(dy, u, gamma, beta, mean, rstd, lim, defect=defect)))
        if defect in ("no_xhat_term", "no_mean_term", "gelu_prime_is_cdf"):
            _out(od["du"], rb["du"], bb["du"], tag + defect + " du")
        elif defect == "limit_row_not_zeroed":   # (du stays zero there: the forward left rstd = 0; what shows is dy GELU'(beta) in dbeta)
            _out(od["dbeta"], rb["dbeta"], bb["dbeta"], tag + defect + " dbeta")
        elif defect == "dgamma_from_g":
            _out(od["dgamma"], rb["dgamma"], bb["dgamma"], tag + defect + " dgamma")
        else:
            assert defect in ("last_row_dropped", "second_stride_iteration_dropped")
            for n in ("dgamma", "dbeta") + (("colsum",) if dt == R.F else ()):
                _out(od[n], rb[n], bb[n], tag + defect + " " + n)


def test_every_defect_is_demanded_somewhere():
    """demanded() must not switch a defect off everywhere: each one is asked for in some shape and dtype of the lists above."""
    lg_limits = [None, "L", "L/3", "0"]
    for d in R.LN_FWD_DEFECTS:
        assert any(demanded(d, dt, with_res=wr) for dt in DTS for wr in (True, False)), d
    for d in R.LN_BWD_DEFECTS:
        assert any(demanded(d, dt, with_dres=wd, two_iterations=rows > 4 * R.LN_BWD_CAP) for dt in DTS for wd in (True, False) for rows, _ in LN_SHAPES), d
    for d in R.LG_FWD_DEFECTS:
        assert any(demanded(d, dt, partial_limit=w == "L/3") for dt in DTS for w in lg_limits), d
    for d in R.LG_BWD_DEFECTS:
        key = "last_row_dropped_gelu" if d == "last_row_dropped" else d
        for dt in DTS:   # (every backward defect in BOTH dtypes)
            assert any(demanded(key, dt, big=Bn * L > 100, two_iterations=Bn * L > 4 * R.LG_BWD_CAP and w in (None, "L"), partial_limit=w == "L/3")
                       for Bn, L, _ in LG_SHAPES for w in lg_limits), (d, dt)


def test_colsum_bound_is_tighter_than_the_old_scale():
    """test_ln_gelu allows colsum(du) an error of 2e-4 (fp32) / 2e-2 (bf16) of max|du| sqrt(rows); the counted bound is smaller."""
    for dt, rel in ((R.F, 2e-4), (R.B, 2e-2)):
        u, gamma, beta, dy = R.lg_case(R.LG_B, R.LG_BIG_L, 64, dt)
        _, mean, rstd = R.ln_gelu_fwd_emulate32(u, gamma, beta, R.EPS)
        rb = R.ln_gelu_bwd64(dy, u, gamma, beta, mean, rstd)
        bb = R.ln_gelu_bwd_bounds(rb, dt)
        old = rel * float(rb["du"].abs().max()) * (R.LG_B * R.LG_BIG_L) ** 0.5
        print("colsum(du) %s: counted bound max %.3e median %.3e, old scale %.3e" % (R.NAME[dt], float(bb["colsum"].max()),
                                                                                     float(bb["colsum"].median()), old))
        assert float(bb["colsum"].max()) < old


# ------------------------------------------------------------------------------------------------------------------------------------
# layer 0
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("which", R.C0_LIMITS, ids=["nolimit", "limL", "lim700"])
@pytest.mark.parametrize("k,stride,C,S", R.C0_CASES)
def test_conv0_ln(k, stride, C, S, which, dt):
    wav, w, bias, gamma, beta, dy = R.c0_case(k, stride, C, S, dt)
    L = R.c0_L(k, stride, S)
    assert L > R.C0_BWD_TB and L % 128 != 0
    lim = R.c0_limit(L, which)
    r = R.conv0_ln_fwd64(wav, w, bias, gamma, beta, k, stride, R.EPS, lim)
    b = R.conv0_ln_fwd_bounds(r, dt)
    y, mean, rstd = R.conv0_ln_fwd_emulate32(wav, w, bias, gamma, beta, k, stride, R.EPS, lim)
    live = r["live"].view(R.C0_B, L)
    tag = "conv0_ln %s k%d s%d C%d lim=%s " % (R.NAME[dt], k, stride, C, which)
    _in(y[live], r["y"][live], b["y"][live], tag + "y")
    _in(mean[live], r["mean"][live], b["mean"][live], tag + "mean")
    _in(rstd[live], r["rstd"][live], b["rstd"][live], tag + "rstd")
    rb = R.conv0_ln_bwd64(dy, wav, w, bias, gamma, beta, mean, rstd, k, stride, lim)
    bb = R.conv0_ln_bwd_bounds(rb, dt)
    names = ("dW", "dbias", "dgamma", "dbeta")
    out = R.conv0_ln_bwd_emulate32(dy, wav, w, bias, gamma, beta, mean, rstd, k, stride, lim)
    for n, o in zip(names, out):
        _in(o, rb[n], bb[n], tag + n)
    for defect in R.C0_DEFECTS:
        if defect == "dbias_from_dz":
            od = R.conv0_ln_bwd_emulate32(dy, wav, w, bias, gamma, beta, mean, rstd, k, stride, lim, defect=defect)
            _out(od[1], rb["dbias"], bb["dbias"], tag + defect + " dbias")
        else:
            _, md, _ = R.conv0_ln_fwd_emulate32(wav, w, bias, gamma, beta, k, stride, R.EPS, lim, defect=defect)
            _out(md[live], r["mean"][live], b["mean"][live], tag + defect + " mean")


# ------------------------------------------------------------------------------------------------------------------------------------
# the GELU constants of csrc/cst_common.h
# ------------------------------------------------------------------------------------------------------------------------------------
def test_gelu_formulas_stay_inside_the_stated_constants():
    x = torch.linspace(-6.0, 6.0, 1200001, dtype=torch.float64).float()
    z = x.double()
    for name, got, ref, a in (("gelu erf", R.gelu_erf32(x), R.gelu64(z), R.A_GELU[R.F]), ("gelu' erf", R.dgelu_erf32(x), R.dgelu64(z), R.A_DGELU[R.F]),
                              ("gelu poly", R.gelu_poly32(x), R.gelu64(z), R.A_GELU[R.B]), ("gelu' poly", R.dgelu_poly32(x), R.dgelu64(z), R.A_DGELU[R.B])):
        err = (got.double() - ref).abs()
        print("%-10s max abs error %.3e at x = %.4f (stated %.1e)" % (name, float(err.max()), float(x[err.argmax()]), a))
        assert float(err.max()) <= a, name
