"""The bounds of loss_optim_ref.py discriminate, shown without a GPU: at every shape test_loss_optim_gpu.py uses, a faithful fp32
evaluation of each kernel (the op-by-op emulation) lies inside the bound against fp64 on EVERY element, and every defective variant
leaves it on a stated minimum share of the elements the defect touches.  Each test prints the shares it measured (pytest -s).

Where the minimum shares come from (reasoning, not the measured figure):
  Adam, weight decay dropped / L2 instead of decoupled — the result moves by wd*lr*|p| = 1e-5 |p| (L2: m moves by (1-b1)*wd*|p| =
      1e-3 |p|), the bound is ~ 2 u32 |p| = 1.2e-7 |p| plus ~ 1e-6 of the update: every element with |p| > 1e-3 must show it.
  Adam, no bias correction — the update is scaled by (1-b1^t)/sqrt(1-b2^t) = 1.12 at t = 3, 0.71 at t = 1; the update's median is
      ~ 7e-4 against a bound of ~ 1e-7: only elements whose m' all but cancels can hide, 99 % must show it.  (At t = 150000 both
      corrections are 1 to fp32 precision: the defect does not exist there and is not tested.)
  Adam, eps inside the square root — sqrt(v + eps) against sqrt(v) + eps: with v ~ 1e-2 the denominators differ by 4e-7 relative, below
      the rounding of |p| unless |p| is small — a handful of elements, reported but not demanded; with v' ~ eps^2 they differ by a
      factor ~ 1e4 and 99 % must show it.
  CE, no smoothing term — every entry of a live row moves by g*eps/V; a bf16 store hides that only where |d| > 128 g eps/V, i.e.
      p > 129/V, the few largest probabilities of a row: 99 % of the entries of live rows must show it, in fp32 too.
  CE, target coefficient 1 — the target entry moves by g*eps = 0.037 against u_out*|d| <= 1.5e-3: every target entry of a live row.
  CE, gradient on pad rows — the bound there is zero: every entry that the defect makes non-zero, 99 % of the entries of pad rows.
"""
import pytest
import torch

import loss_optim_ref as R

HP = R.ADAM_HP


def _share(got, ref, bound, mask=None):
    err = (got.double() - ref).abs()
    out = err > bound
    if mask is not None:
        out = out[mask]
    return (float(out.double().mean()) if out.numel() else float("nan")), int(out.sum()), out.numel()


@pytest.mark.parametrize("case", R.ADAM_CASES, ids=R.adam_case_id)
def test_adam_bounds_hold_for_the_emulation_and_reject_each_defect(case):
    n, gdt, pdt, wd, step, gs, small = case
    master, m, v, g = R.adam_inputs(n, gdt, small)
    args = (master, m, v, g, gs, HP["lr"], HP["b1"], HP["b2"], HP["eps"], wd, step)
    r = R.adam_ref64(*args)
    bp, bm, bv = R.adam_bounds(r)
    p32, m32, v32 = R.adam_emulate32(*args)
    for name, got, ref, b in (("master", p32, r["master"], bp), ("m", m32, r["m"], bm), ("v", v32, r["v"], bv),
                              ("param", p32.to(pdt), r["master"], R.param_bound(r, bp, pdt))):
        ratio, bad = R.worst_ratio(got, ref, b)
        print("adam clean %-6s worst err/bound %.3f, %d of %d outside" % (name, ratio, bad, n))
        assert bad == 0, "%s: the clean emulation leaves the bound on %d of %d elements (worst ratio %.3f)" % (name, bad, n, ratio)
    big_p = master.abs() > 1e-3
    for defect in R.ADAM_DEFECTS:
        pd, md, vd = R.adam_emulate32(*args, defect=defect)
        sp = _share(pd, r["master"], bp)
        sm = _share(md, r["m"], bm)
        print("adam %-18s master outside %d of %d, m outside %d of %d" % (defect, sp[1], sp[2], sm[1], sm[2]))
        if defect == "no_weight_decay" and wd != 0:
            s = _share(pd, r["master"], bp, big_p)
            print("   of the elements with |p| > 1e-3: %d of %d" % (s[1], s[2]))
            assert s[1] == s[2]
        if defect == "l2_decay" and wd != 0:
            s = _share(md, r["m"], bm, big_p)
            print("   m, of the elements with |p| > 1e-3: %d of %d" % (s[1], s[2]))
            assert s[1] == s[2]
        if defect == "no_bias_correction" and step < 100:
            assert sp[0] >= 0.99 if n >= 1000 else sp[1] == sp[2]
        if defect == "eps_inside_sqrt" and small:
            assert sp[0] >= 0.99
        if defect == "eps_inside_sqrt" and not small and n == 100003:
            assert sp[1] >= 1


@pytest.mark.parametrize("dt", [R.F, R.B], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", R.SUMSQ_SIZES)
def test_sumsq_bound_holds_for_the_emulation(n, dt):
    x = R.sumsq_inputs(n, dt)
    ref = R.sumsq_ref64(x)
    bound = R.sumsq_bound(ref, n)
    got = R.sumsq_emulate32(x)
    err = abs(float(got.double()) - float(ref))
    print("sumsq n=%d chain %d: err/bound %.3f (relative error %.2e)" % (n, R.sumsq_chain(n), err / bound, err / float(ref)))
    assert err <= bound
    # the last element (the tail block 0 handles, or the last 8-element item) carries far more than the bound: dropping it must show
    lost = R.sumsq_emulate32(x[:-1]) if n > 1 else torch.zeros(1)
    assert abs(float(lost.double()) - float(ref)) > 10 * bound
    # accumulate contract of the emulation itself (out[0] += ...)
    assert float(R.sumsq_emulate32(x, out0=3.5)) == float(torch.tensor(3.5) + got)


def _lsce_case(rows, V, dt, kind):
    tgt = R.lsce_targets(rows, V)
    lg = R.lsce_logits(rows, V, dt, kind)
    return [(lg, tgt)] if kind != "shift" else [(lg[0], tgt), (lg[1], tgt)]


@pytest.mark.parametrize("kind", ["plain", "shift", "peaked"])
@pytest.mark.parametrize("dt", [R.F, R.B], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,V", R.LSCE_SHAPES)
def test_lsce_bounds_hold_for_the_emulation_and_reject_each_defect(rows, V, dt, kind):
    for logits, tgt in _lsce_case(rows, V, dt, kind):
        r = R.lsce_ref64(logits, tgt, R.LSCE_EPS, R.LSCE_PAD, R.LSCE_G)
        b = R.lsce_bounds(r, dt)
        loss, nll, lse, d = R.lsce_emulate32(logits, tgt, R.LSCE_EPS, R.LSCE_PAD, R.LSCE_G)
        for name, got, ref, bb in (("loss", loss, r["loss"], torch.tensor(b["loss"])), ("nll", nll, r["nll"], torch.tensor(b["nll"])),
                                   ("lse", lse, r["lse"], b["lse"]), ("dlogits", d, r["dlogits"], b["dlogits"])):
            ratio, bad = R.worst_ratio(got, ref, bb)
            print("ls-ce clean %-7s worst err/bound %.3f" % (name, ratio))
            assert bad == 0, "%s: the clean emulation leaves the bound on %d elements (worst ratio %.3f)" % (name, bad, ratio)
        live = r["live"]
        rowsum = d.double().sum(1).abs()
        assert bool((rowsum[live] <= b["dlogits"].sum(1)[live]).all())
        assert bool((d[~live] == 0).all())
        is_t = r["onehot"].bool() & live[:, None]
        for defect in R.LSCE_DEFECTS:
            lossd, _, _, dd = R.lsce_emulate32(logits, tgt, R.LSCE_EPS, R.LSCE_PAD, R.LSCE_G, defect=defect)
            if defect == "no_smoothing":
                s = _share(dd, r["dlogits"], b["dlogits"], live[:, None].expand_as(dd))
                assert s[0] >= 0.99
                assert V == 1 or abs(float(lossd) - float(r["loss"])) > b["loss"]  # (V = 1: every loss term is zero)
            elif defect == "target_coef_one":
                s = _share(dd, r["dlogits"], b["dlogits"], is_t)
                assert s[1] == s[2]
                rs = dd.double().sum(1).abs()
                assert bool((rs[live] > b["dlogits"].sum(1)[live]).all()), "the row invariant must see a wrong target coefficient"
                assert V == 1 or abs(float(lossd) - float(r["loss"])) > b["loss"]  # (V = 1: every loss term is zero)
            else:
                if bool(live.all()):
                    continue
                s = _share(dd, r["dlogits"], b["dlogits"], (~live)[:, None].expand_as(dd))
                assert s[0] >= 0.99
                assert V == 1 or abs(float(lossd) - float(r["loss"])) > b["loss"]  # (V = 1: every loss term is zero)
            print("ls-ce %-16s outside on %d of the %d entries it touches" % (defect, s[1], s[2]))
