"""cst_adam_step, cst_sumsq and cst_ls_ce_fwd / cst_ls_ce_bwd on a real MI355X against the fp64 restatements of loss_optim_ref.py,
under ITS per-element bounds (derived from the kernels' operation sequences; test_loss_optim_ref_cpu.py shows that they hold for a
faithful fp32 evaluation and reject dropped weight decay, eps inside the square root, missing bias corrections, L2 decay, a missing
smoothing term, a wrong target coefficient and gradients on pad rows).  Also: the bit-level promises of the source — the parameter
store, one element = one result across the vector loop, the scalar kernel and spans, the accumulate contract of cst_sumsq.

Every test prints the worst observed error / bound per quantity (pytest -s): the head-room of the constants."""
import math
from importlib import import_module

import pytest
import torch

import loss_optim_ref as R
from conftest import load_pkg

pytestmark = pytest.mark.gpu

HP = R.ADAM_HP
NAME = {torch.float32: "f32", torch.bfloat16: "bf16"}


@pytest.fixture(scope="module")
def K():
    load_pkg()
    return import_module("chimera-st_amd.kernels"), import_module("chimera-st_amd.lib")


def within(got, ref, bound, what):
    got = got.detach().cpu()
    assert bool(torch.isfinite(got.float()).all()), what + ": non-finite output"
    if not torch.is_tensor(bound):
        bound = torch.tensor(float(bound), dtype=torch.float64)
    ratio, bad = R.worst_ratio(got, ref, bound)
    print("RATIO %-34s worst err/bound %.3f" % (what, ratio))
    assert bad == 0, "%s: %d of %d elements outside the bound, worst err/bound %.3f" % (what, bad, got.numel(), ratio)


# ------------------------------------------------------------------------------------------------------------------------------------
# Adam
# ------------------------------------------------------------------------------------------------------------------------------------
def _run_adam(k, master, m, v, g, pdt, wd, step, gs):
    dm, dmm, dv, dg = master.cuda(), m.cuda(), v.cuda(), g.cuda()
    p = torch.full((master.numel(),), float("nan"), dtype=pdt, device="cuda")
    gst = None if gs is None else torch.tensor([gs], dtype=torch.float32, device="cuda")
    k.adam_step(dm, dmm, dv, dg, p, HP["lr"], HP["b1"], HP["b2"], HP["eps"], wd, step, gst)
    return dm, dmm, dv, p


@pytest.mark.parametrize("case", R.ADAM_CASES, ids=R.adam_case_id)
def test_adam_step_against_fp64(K, case):
    k, _ = K
    n, gdt, pdt, wd, step, gs, small = case
    master, m, v, g = R.adam_inputs(n, gdt, small)
    r = R.adam_ref64(master, m, v, g, gs, HP["lr"], HP["b1"], HP["b2"], HP["eps"], wd, step)
    bp, bm, bv = R.adam_bounds(r)
    dm, dmm, dv, p = _run_adam(k, master, m, v, g, pdt, wd, step, gs)
    tag = "adam g%s/p%s " % (NAME[gdt], NAME[pdt])
    within(dm, r["master"], bp, tag + "master")
    within(dmm, r["m"], bm, tag + "m")
    within(dv, r["v"], bv, tag + "v")
    within(p, r["master"], R.param_bound(r, bp, pdt), tag + "param")
    # the parameter store: the master rounded to nearest even, bit for bit (fp32: the master itself)
    assert torch.equal(p, dm.to(pdt))


@pytest.mark.parametrize("gdt,pdt", [(torch.bfloat16, torch.bfloat16), (torch.float32, torch.float32)], ids=["bf16", "f32"])
def test_adam_one_element_one_result(K, gdt, pdt):
    """The whole buffer in one call (float4 loop, two grid-stride iterations, scalar tail), the same data in spans cut at multiples of
    optim.ALIGN, and the same data in views shifted by one element (not 16-byte aligned: the scalar kernel, five grid-stride
    iterations) give every element the same bits."""
    k, _ = K
    ALIGN = import_module("chimera-st_amd.optim").ALIGN
    n, wd, step, gs = R.ADAM_BIG, 0.01, 3, 0.25
    master, m, v, g = R.adam_inputs(n, gdt)
    whole = _run_adam(k, master, m, v, g, pdt, wd, step, gs)

    gst = torch.tensor([gs], dtype=torch.float32, device="cuda")
    cuts = [0, ALIGN * 1, ALIGN * 1000, ALIGN * 100001, n]
    sm, smm, sv, sg = master.cuda(), m.cuda(), v.cuda(), g.cuda()
    sp = torch.full((n,), float("nan"), dtype=pdt, device="cuda")
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        k.adam_step(sm[lo:hi], smm[lo:hi], sv[lo:hi], sg[lo:hi], sp[lo:hi], HP["lr"], HP["b1"], HP["b2"], HP["eps"], wd, step, gst)

    def shifted(t, dt):
        buf = torch.zeros(n + 1, dtype=dt, device="cuda")
        buf[1:].copy_(t)
        return buf[1:]
    um, umm, uv, ug = shifted(master, torch.float32), shifted(m, torch.float32), shifted(v, torch.float32), shifted(g, gdt)
    up = shifted(torch.full((n,), float("nan")), pdt)
    assert um.data_ptr() % 16 != 0
    k.adam_step(um, umm, uv, ug, up, HP["lr"], HP["b1"], HP["b2"], HP["eps"], wd, step, gst)

    for name, a, b, c in zip(("master", "m", "v", "param"), whole, (sm, smm, sv, sp), (um, umm, uv, up)):
        assert torch.equal(a, b), name + ": spans differ from the single call"
        assert torch.equal(a, c), name + ": the scalar kernel differs from the vector kernel"


def test_fused_adam_two_steps_against_fp64(K):
    """optim.FusedAdam over a small FlatParamBuffers: two step()s with clipping active and multiply != 1 under a warm-up schedule,
    each against adam_ref64 fed the fp64 clip coefficient, the lr of that update and its number — the _scale plumbing, num_updates
    and the schedule, not only the kernel.  Every update starts from the state the device holds, so each is judged on its own.

    The scale reaches the kernel as an fp32 device scalar computed by torch: sum of squares (sumsq_chain roundings, halved by the
    square root), sqrt 2, * multiply 2 (its fp32 value and the product), + 1e-6 2, the division 2, * multiply 1, and the kernel's
    g * scale 1 (torch's device sqrt and division counted as 2 each) — that many roundings sit in the scaled gradient (kg)."""
    k, _ = K
    optim = import_module("chimera-st_amd.optim")
    gen = torch.Generator().manual_seed(90)
    shapes = [(7,), (13, 5), (3,), (129,), (1, 31)]
    params = [torch.nn.Parameter((torch.randn(*s, generator=gen) * 0.5).to(torch.bfloat16).cuda()) for s in shapes]
    clip, mult, wd = 0.5, 0.375, 0.01
    opt = optim.FusedAdam(params, lr=1e-3, betas=(HP["b1"], HP["b2"]), eps=HP["eps"], weight_decay=wd, clip_norm=clip,
                          warmup_updates=4, warmup_init_lr=1e-4)
    buf = opt.buf
    assert buf.total % optim.ALIGN == 0 and buf.total > sum(p.numel() for p in params)
    kg = math.ceil(R.sumsq_chain(buf.total) / 2) + 2 + 2 + 2 + 2 + 1 + 1
    for update in (1, 2):
        opt.zero_grad()
        for i, (p, view) in enumerate(zip(buf.params, buf.grad_views)):
            view.copy_((torch.randn(*p.shape, generator=gen) * (1.0 + i)).to(torch.bfloat16))
        lr = opt.get_lr()
        assert lr == optim.inverse_sqrt_lr(update - 1, 1e-3, 4, 1e-4) and (update == 1 or lr != 1e-4)
        master, m, v, g = opt.master.cpu(), opt.exp_avg.cpu(), opt.exp_avg_sq.cpu(), buf.flat_grad.cpu()
        gnorm64 = R.f32(mult) * math.sqrt(float(R.sumsq_ref64(g)))
        coef64 = min(1.0, clip / (gnorm64 + 1e-6))
        assert coef64 < 1.0, "the clip must be active"
        gnorm = opt.step(multiply=mult)
        assert opt.num_updates == update
        assert abs(float(gnorm) - gnorm64) <= kg * R.U32 * gnorm64
        r = R.adam_ref64(master, m, v, g, coef64 * R.f32(mult), lr, HP["b1"], HP["b2"], HP["eps"], wd, update)
        bp, bm, bv = R.adam_bounds(r, kg=kg)
        within(opt.master, r["master"], bp, "FusedAdam update %d master" % update)
        within(opt.exp_avg, r["m"], bm, "FusedAdam update %d m" % update)
        within(opt.exp_avg_sq, r["v"], bv, "FusedAdam update %d v" % update)
        assert torch.equal(buf.flat_param, opt.master.to(torch.bfloat16))
        for p, o in zip(buf.params, buf.offsets):  # the parameters are views of what was just written
            assert torch.equal(p.data.reshape(-1), buf.flat_param[o:o + p.numel()])


# ------------------------------------------------------------------------------------------------------------------------------------
# sumsq
# ------------------------------------------------------------------------------------------------------------------------------------
def _sumsq(k, x, prefill=0.0):
    out = torch.full((1,), prefill, dtype=torch.float32, device="cuda")
    k.sumsq(x, out)
    return out


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", R.SUMSQ_SIZES)
def test_sumsq_against_fp64(K, n, dt):
    k, _ = K
    x = R.sumsq_inputs(n, dt)
    ref = R.sumsq_ref64(x)
    dx = x.cuda()
    out = _sumsq(k, dx)
    within(out, ref.reshape(1), R.sumsq_bound(ref, n), "sumsq %s n=%d" % (NAME[dt], n))
    assert torch.equal(out, _sumsq(k, dx)), "a repeated call must give the same bits"


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_sumsq_accumulates_into_out(K, dt):
    """out[0] += sum: FusedAdam.grad_sumsq adds the spans of a sharded state into one scalar."""
    k, _ = K
    n, cut, prefill = 100003, 8 * 5001, 1024.0
    x = R.sumsq_inputs(n, dt)
    dx = x.cuda()
    out = torch.full((1,), prefill, dtype=torch.float32, device="cuda")
    k.sumsq(dx[:cut], out)
    k.sumsq(dx[cut:], out)
    s1, s2 = R.sumsq_ref64(x[:cut]), R.sumsq_ref64(x[cut:])
    ref = prefill + s1 + s2
    # non-negative terms throughout: the longer of the two chains, one more addition for the second call
    bound = R.sumsq_bound(ref, max(cut, n - cut), extra=1)
    within(out, ref.reshape(1), bound, "sumsq %s prefill + two spans" % NAME[dt])
    assert abs(float(out) - float(s1 + s2)) > 100 * bound, "the prefill must survive"


@pytest.mark.parametrize("n", [100003, R.SUMSQ_BIG])
def test_sumsq_sees_an_inf_in_the_tail(K, n):
    """The trainer skips an update whose gradient norm is not finite: an Inf in the last element — in the tail that block 0 adds —
    must reach the result."""
    k, _ = K
    x = R.sumsq_inputs(n, torch.bfloat16)
    x[-1] = float("inf")
    assert n % 8 != 0
    assert not bool(torch.isfinite(_sumsq(k, x.cuda())).any())


# ------------------------------------------------------------------------------------------------------------------------------------
# label-smoothed cross entropy
# ------------------------------------------------------------------------------------------------------------------------------------
def _run_lsce(k, logits, tgt):
    dl, dt_ = logits.cuda(), tgt.cuda()
    out2, lse = k.ls_ce_fwd(dl, dt_, R.LSCE_EPS, R.LSCE_PAD)
    gs = torch.tensor([R.LSCE_G], dtype=torch.float32, device="cuda")
    d = k.ls_ce_bwd(dl, dt_, lse, gs, R.LSCE_EPS, R.LSCE_PAD)
    return out2.cpu(), lse.cpu(), d.cpu()


def _check_lsce(k, logits, tgt, tag):
    r = R.lsce_ref64(logits, tgt, R.LSCE_EPS, R.LSCE_PAD, R.LSCE_G)
    b = R.lsce_bounds(r, logits.dtype)
    out2, lse, d = _run_lsce(k, logits, tgt)
    within(out2[0:1], r["loss"].reshape(1), b["loss"], tag + " loss")
    within(out2[1:2], r["nll"].reshape(1), b["nll"], tag + " nll")
    within(lse, r["lse"], b["lse"], tag + " lse")
    within(d, r["dlogits"], b["dlogits"], tag + " dlogits")
    live = r["live"]
    assert bool((d[~live] == 0).all()), "dlogits of pad rows must be exactly zero"
    # row invariant, independent of the reference: sum_v dlogits = g * (1 - (1-eps) - eps) = 0 up to the bound summed over the row
    rowsum = d.double().sum(1).abs()
    rb = b["dlogits"].sum(1)
    if bool(live.any()):
        print("RATIO %-34s worst |row sum|/bound %.3f" % (tag + " row sum", float((rowsum[live] / rb[live]).max())))
    assert bool((rowsum[live] <= rb[live]).all())
    return r, b, d


@pytest.mark.parametrize("kind", ["plain", "peaked"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,V", R.LSCE_SHAPES)
def test_label_smoothed_ce_against_fp64(K, rows, V, dt, kind):
    k, _ = K
    tgt = R.lsce_targets(rows, V)
    assert int(tgt[0]) == 0 and int(tgt[-1]) == V - 1 and (rows < 3 or int(tgt[2]) == R.LSCE_PAD)
    _check_lsce(k, R.lsce_logits(rows, V, dt, kind), tgt, "ls-ce %s %s V=%d" % (NAME[dt], kind, V))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,V", R.LSCE_SHAPES)
def test_label_smoothed_ce_is_shift_invariant(K, rows, V, dt):
    """Every logit + 80 (fp32) / + 60 (bf16), exactly: the same softmax, so the same fp64 dlogits; without the max subtraction the
    exponentials overflow (fp32) or lose every bit.  Both runs lie inside their own bound of the one reference."""
    k, _ = K
    tgt = R.lsce_targets(rows, V)
    lo, hi = R.lsce_logits(rows, V, dt, "shift")
    tag = "ls-ce %s V=%d" % (NAME[dt], V)
    r0, b0, d0 = _check_lsce(k, lo, tgt, tag + " unshifted")
    r1, b1, d1 = _check_lsce(k, hi, tgt, tag + " shifted")
    assert float((r0["dlogits"] - r1["dlogits"]).abs().max()) <= 1e-12
    assert bool(((d0.double() - d1.double()).abs() <= b0["dlogits"] + b1["dlogits"]).all())


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_label_smoothed_ce_all_rows_pad(K, dt):
    k, _ = K
    rows, V = 5, 255
    tgt = torch.full((rows,), R.LSCE_PAD, dtype=torch.int64)
    out2, lse, d = _run_lsce(k, R.lsce_logits(rows, V, dt), tgt)
    assert bool((out2 == 0).all()) and bool((d == 0).all())
