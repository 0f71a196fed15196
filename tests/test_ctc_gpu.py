"""cst_ctc_fwd / cst_ctc_bwd / cst_ctc_greedy on a real MI355X against the fp64 restatement of ctc_ref.py under ITS per-element bounds
(test_ctc_ref_cpu.py shows that they hold for a faithful fp32 evaluation and reject skips across equal labels or onto blanks, a final
sum without the last blank, a wrong blank index, gradients past the input length, a missing softmax term and a gradient kept under
zero_infinity), plus the bit-level promises of include/cst.h: layout independence, determinism, batch independence, refusals that touch
nothing.  Prints worst error / bound per quantity (pytest -s)."""
from importlib import import_module

import pytest
import torch

import ctc_ref as R
from conftest import load_pkg

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
NAME = {torch.float32: "f32", torch.bfloat16: "bf16"}


@pytest.fixture(scope="module")
def CF():
    load_pkg()
    return import_module("chimera-st_amd.functional")


@pytest.fixture(scope="module")
def K():
    load_pkg()
    return import_module("chimera-st_amd.kernels"), import_module("chimera-st_amd.lib")


def run(CF, x, tg, tl, il, blank, zi, gscale=1.0):
    """loss, nll, gradient of CF.ctc_loss on device tensors; the upstream gradient is `gscale`."""
    x = x.detach().requires_grad_(True)
    loss, nll = CF.ctc_loss(x, tg, tl, il, blank, zi)
    (loss * gscale).backward()
    return dict(loss=loss.detach().cpu(), nll=nll.cpu(), grad=x.grad.cpu())


def on_device(case):
    x, tg, tl, il, blank, zi = case
    return x.cuda(), tg.cuda(), tl.cuda(), il.cuda(), blank, zi


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_ctc_against_fp64(CF, name, dtype):
    case, r, (bn, bl, bg, M) = R.reference(name, dtype)
    x, tg, tl, il, blank, zi = on_device(case)
    if name == "wide1000":  # row stride 1003, the base shifted by one element: no row is 16-byte aligned by accident
        T, B, V = x.shape
        buf = torch.zeros(T * B * 1003 + 1, dtype=dtype, device="cuda")
        xs = buf[1:].view(T, B, 1003)[:, :, :V]
        xs.copy_(x)
        x = xs
    got = run(CF, x, tg, tl, il, blank, zi)
    ratios, bad, _ = R.judge(name, dtype, got)
    print("RATIO ctc %-16s %-4s nll %.3f loss %.3f grad %.3f   M_b %s" % ((name, NAME[dtype]) + ratios + (["%.3g" % m for m in M.tolist()],)))
    assert bad == 0
    # frames at or past the input length: zero bits
    for b in range(x.shape[1]):
        assert int(got["grad"][int(case[3][b]):, b].view(torch.int16 if dtype == torch.bfloat16 else torch.int32).ne(0).sum()) == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
def test_infeasible_utterance(CF, dtype):
    """a a b b in 6 frames is exactly feasible, in 5 it is not.  zero_infinity off: loss +inf, a non-finite gradient element there, the
    other utterance within its bounds (test_ctc_against_fp64[repeats_inf]); on: the other utterance's loss, all zero bits."""
    case, r, _ = R.reference("repeats_inf", dtype)
    got = run(CF, *on_device(case))
    assert float(got["loss"]) == float("inf") and float(got["nll"][1]) == float("inf") and bool(torch.isfinite(got["nll"][0]))
    assert not bool(torch.isfinite(got["grad"][:5, 1].float()).all())
    assert bool(torch.isfinite(got["grad"][:, 0].float()).all())
    case, r, _ = R.reference("repeats_zero_inf", dtype)
    got = run(CF, *on_device(case))
    assert float(got["nll"][1]) == float("inf")
    assert float(got["loss"]) == float(got["nll"][0])
    assert int(got["grad"][:, 1].view(torch.int16 if dtype == torch.bfloat16 else torch.int32).ne(0).sum()) == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("name", ["edge", "wave"])
def test_layout_determinism_batch_independence(CF, name, dtype):
    case, _, _ = R.reference(name, dtype)
    x, tg, tl, il, blank, zi = on_device(case)
    a = run(CF, x, tg, tl, il, blank, zi)
    again = run(CF, x, tg, tl, il, blank, zi)
    bm = x.transpose(0, 1).contiguous()  # batch-major memory [B, T, V]
    view = run(CF, bm.transpose(0, 1), tg, tl, il, blank, zi)  # modules.to_time_major_view
    for k in ("loss", "nll", "grad"):
        assert torch.equal(a[k], again[k]), "two calls differ in " + k
        assert torch.equal(a[k], view[k]), "the time-major view of batch-major memory differs in " + k
    for b in range(x.shape[1]):
        L = int(case[2][b])
        alone = run(CF, x[:, b:b + 1].contiguous(), tg[b:b + 1, :L].contiguous(), tl[b:b + 1], il[b:b + 1], blank, zi)
        assert torch.equal(alone["nll"][0], a["nll"][b]) and torch.equal(alone["grad"][:, 0], a["grad"][:, b]), "utterance %d" % b


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("name", ["wave", "workgroup", "longest"])
def test_forward_backward_variables(K, name, dtype):
    """alpha and beta as cst_ctc_fwd leaves them, state by state, under ctc_ref's log-domain bounds (S > 64: 256 threads; S > 1024: the
    1024-thread recursion with more than one state per thread; T = 1499).  The gradient's occupancy bound is loose at these sizes; this
    one is not: a state that read a wrong neighbour would be off by far more."""
    k, _ = K
    case, _, _ = R.reference(name, dtype)
    x, tg, tl, il, blank, zi = on_device(case)
    saved = k.ctc_fwd(x, tg, tl, il, blank, zi)[2]
    alpha, beta = saved[6].cpu(), saved[7].cpu()
    Tb, S = case[3].tolist(), [2 * int(n) + 1 for n in case[2]]
    worst, bad = R.judge_alpha_beta(name, dtype, [alpha[b, :Tb[b], :S[b]] for b in range(len(S))], [beta[b, :Tb[b], :S[b]] for b in range(len(S))])
    print("RATIO ctc alpha/beta %-10s %-4s %.3f" % (name, NAME[dtype], worst))
    assert bad == 0


def test_gradient_scale(CF):
    """The upstream gradient arrives as a device scalar: a power of two scales every element exactly."""
    case, _, _ = R.reference("edge", torch.float32)
    one, quarter = run(CF, *on_device(case)), run(CF, *on_device(case), gscale=0.25)
    assert torch.equal(one["grad"] * 0.25, quarter["grad"])


def test_refusals_touch_nothing(K):
    k, lib = K
    T, B, V = 8, 2, 6
    x = torch.randn(T, B, V, device="cuda")
    il = torch.full((B,), T, dtype=torch.int64, device="cuda")
    tl = torch.full((B,), 2, dtype=torch.int64, device="cuda")
    long_t = torch.ones(B, k.CTC_L_MAX + 1, dtype=torch.int64, device="cuda")
    f = lambda *s: torch.full(s, 7.0, device="cuda")
    nll, loss, lse, ws = f(B), f(1), f(B, T), f(B, T, 5)
    P = lib.ptr

    def fwd(logits=x, st=B * V, sb=V, tg=long_t[:, :2].contiguous(), Lmax=2, blank=0, dtype=0, T_=T):
        return lib.load().cst_ctc_fwd(P(logits), st, sb, P(tg), Lmax, P(tl), P(il), blank, 0, P(nll), P(loss), P(lse), P(ws), P(ws), None,
                                      T_, B, V, dtype, lib.stream_ptr())
    assert fwd(tg=long_t, Lmax=k.CTC_L_MAX + 1) == -4 and b"exceed the supported" in lib.load().cst_last_error()
    for kw, msg in ((dict(blank=V), b"blank"), (dict(blank=-1), b"blank"), (dict(dtype=5), b"bad dtype"), (dict(T_=0), b"bad shape"),
                    (dict(st=V - 1), b"strides"), (dict(Lmax=-1), b"null operand")):
        assert fwd(**kw) == -1 and msg in lib.load().cst_last_error(), kw
    with pytest.raises(RuntimeError, match="exceed the supported"):
        k.ctc_fwd(x, long_t, tl, il, 0)
    ids, cnt = torch.full((B, T), 7, dtype=torch.int32, device="cuda"), torch.full((B,), 7, dtype=torch.int32, device="cuda")
    assert lib.load().cst_ctc_greedy(P(x), B * V, V, P(il), V, P(ids), P(ids), P(cnt), T, B, V, 0, lib.stream_ptr()) == -1
    d = f(T, B, V)
    assert lib.load().cst_ctc_bwd(P(x), B * V, V, P(long_t), k.CTC_L_MAX + 1, P(tl), P(il), 0, 0, P(nll), P(lse), P(ws), P(ws), P(loss), P(d),
                                  B * V, V, T, B, V, 0, lib.stream_ptr()) == -4
    torch.cuda.synchronize()
    for t in (nll, loss, lse, ws, d):
        assert bool((t == 7.0).all())
    assert bool((ids == 7).all()) and bool((cnt == 7).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("layout", ["contiguous", "batch_major"])
def test_greedy(CF, dtype, layout):
    x, il, blank = R.greedy_logits()  # (its planted values are bf16-exact, the rest are compared after rounding)
    x = x.to(dtype)
    ref = R.greedy_ref(x, il, blank)
    xd = x.cuda()
    if layout == "batch_major":
        xd = xd.transpose(0, 1).contiguous().transpose(0, 1)
    ids, counts, packed = CF.ctc_greedy(xd, il.cuda(), blank)
    host = packed.cpu()  # one transfer: B*T ids and B counts
    T, B = x.shape[0], x.shape[1]
    ids, counts = host[:B * T].view(B, T), host[B * T:]
    for b in range(B):
        n = int(counts[b])
        assert ids[b, :n].tolist() == ref[b], "utterance %d" % b
        assert bool((ids[b, n:] == -1).all())
    for b in (1, 2):  # rows without ties: torch's argmax / unique_consecutive on the CPU, the reference criterion's calls
        toks = x[:int(il[b]), b].float().argmax(dim=-1).unique_consecutive()
        assert toks[toks != blank].tolist() == ids[b, :int(counts[b])].tolist()


def test_greedy_wide_rows_and_long_utterance(CF):
    """V = 1000 (the 256-thread rows) at T = 600 (three chunks of the compaction), a tie across two threads' elements."""
    g = torch.Generator(device="cpu")
    g.manual_seed(11)
    T, B, V = 600, 2, 1000
    x = torch.randn(T, B, V, generator=g)
    x[5, 0, 900] = x[5, 0, 17] = 30.0
    il = torch.tensor([600, 333], dtype=torch.int64)
    ref = R.greedy_ref(x, il, 3)
    _, _, packed = CF.ctc_greedy(x.cuda(), il.cuda(), 3)
    host = packed.cpu()
    for b in range(B):
        assert host[b * T:b * T + int(host[B * T + b])].tolist() == ref[b]
