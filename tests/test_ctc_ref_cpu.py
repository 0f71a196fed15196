"""ctc_ref.py checked without a GPU: its fp64 restatement equals torch's F.ctc_loss on fp64 log_softmax (values and autograd) at every
case of test_ctc_gpu.py; its bounds accept a faithful fp32 evaluation of the kernels' operation sequence at every case and storage type;
and they reject every listed defect at one case at least.  Prints worst error / bound (pytest -s)."""
import pytest
import torch
import torch.nn.functional as F

import ctc_ref as R

DTYPES = [torch.float32, torch.bfloat16]
NAME = {torch.float32: "f32", torch.bfloat16: "bf16"}


reference = R.reference


judge = R.judge


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_reference_equals_torch_fp64(name):
    (x, tg, tl, il, blank, zi), r, _ = reference(name, torch.float32)
    xd = x.double().requires_grad_(True)
    loss = F.ctc_loss(F.log_softmax(xd, -1), tg, il, tl, blank=blank, reduction="none", zero_infinity=zi)
    loss.sum().backward()
    expect = loss.detach().sum()
    with torch.no_grad():  # (under zero_infinity torch reports 0 for an infeasible utterance; the kernels keep +inf in nll, 0 in the sum)
        loss = F.ctc_loss(F.log_softmax(xd, -1), tg, il, tl, blank=blank, reduction="none", zero_infinity=False)
    fin = torch.isfinite(r["nll"])
    assert torch.equal(torch.isfinite(loss), fin)
    assert torch.allclose(loss[fin], r["nll"][fin], rtol=1e-10, atol=1e-10)
    for b in range(x.shape[1]):
        if fin[b] or zi:
            assert float((xd.grad[:, b] - r["grad"][:, b]).abs().max()) < 1e-8, (name, b)
        else:
            assert not bool(torch.isfinite(r["grad"][:int(il[b]), b]).all()) and not bool(torch.isfinite(xd.grad[:, b]).all())
    assert torch.isinf(r["loss"]) if torch.isinf(expect) else abs(float(expect - r["loss"])) < 1e-9 * max(1.0, abs(float(expect)))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_bounds_accept_a_faithful_fp32_evaluation(name, dtype):
    (x, tg, tl, il, blank, zi), _, _ = reference(name, dtype)
    got = R.ctc_eval(x, tg, tl, il, blank, zi, dt=torch.float32)
    got["grad"] = got["grad"].to(dtype)
    ratios, bad, M = judge(name, dtype, got)
    print("RATIO ctc %-16s %-4s nll %.3f loss %.3f grad %.3f   M_b %s" % ((name, NAME[dtype]) + ratios + (["%.3g" % m for m in M.tolist()],)))
    assert bad == 0


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_bounds_reject_defect(defect):
    rejected = []
    for name in ("edge", "edge_blank_last", "repeats_inf", "repeats_zero_inf", "wave"):
        (x, tg, tl, il, blank, zi), _, _ = reference(name, torch.float32)
        got = R.ctc_eval(x, tg, tl, il, blank, zi, dt=torch.float32, defect=defect)
        if judge(name, torch.float32, got)[1]:
            rejected.append(name)
    print("DEFECT %-20s rejected at %s" % (defect, rejected))
    assert rejected


@pytest.mark.parametrize("name", ["wave", "workgroup", "longest"])
def test_alpha_beta_bounds_accept_fp32_and_reject_a_striding_slip(name):
    """The forward / backward variables under their own log-domain bounds: a faithful fp32 evaluation passes at the cases with S > 64,
    S > 1024 and T = 1499; a beta recursion that loses the skip transition from state 1024 on fails where such states exist."""
    (x, tg, tl, il, blank, zi), _, _ = reference(name, torch.float32)
    got = R.ctc_eval(x, tg, tl, il, blank, zi, dt=torch.float32)
    worst, bad = R.judge_alpha_beta(name, torch.float32, [t["alpha"] for t in got["terms"]], [t["beta"] for t in got["terms"]])
    print("RATIO ctc alpha/beta %-10s %.3f" % (name, worst))
    assert bad == 0
    if name == "workgroup":
        for d in R.RECURSION_DEFECTS:
            mut = R.ctc_eval(x, tg, tl, il, blank, zi, dt=torch.float32, defect=d)
            assert R.judge_alpha_beta(name, torch.float32, [t["alpha"] for t in mut["terms"]], [t["beta"] for t in mut["terms"]])[1] > 0, d


def test_greedy_rule_and_its_defects():
    x, il, blank = R.greedy_logits()
    ref = R.greedy_ref(x, il, blank)
    assert ref[0] == [3, 3, 2, 5, 2, 6, 1, 4] and ref[1] == [4, 2] and ref[2] == [] and ref[3][-1] == 5
    for d in R.GREEDY_DEFECTS:
        assert R.greedy_ref(x, il, blank, defect=d) != ref, d
    # rows without planted ties: torch's argmax / unique_consecutive (the reference criterion's own calls)
    for b in (1, 2):
        toks = x[:int(il[b]), b].argmax(dim=-1).unique_consecutive()
        assert toks[toks != blank].tolist() == ref[b]
