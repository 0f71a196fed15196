"""cst_w2v_negatives / cst_infonce_fwd / cst_infonce_bwd_x / cst_infonce_bwd_y on a real MI355X against the fp64 restatement of
w2v_pretrain_ref.py under ITS per-element bounds (test_w2v_pretrain_ref_cpu.py shows that they hold for a faithful fp32 evaluation and
reject a missing eps clamp, a dropped -inf mask, a duplicate negative counted once and a backward without 1 / temp), plus the bit-level
promises of include/cst.h: the sampler equals its numpy twin, exact counters, determinism, batch independence, refusals that touch
nothing.  Below them cst_gumbel_vq_fwd / cst_gumbel_vq_bwd, functional.gumbel_vector_quantize and wav2vec2.GumbelVectorQuantizer: exact
choices (own counter-hash noise, injected noise, eval mode with planted ties), perplexities, d logits, gy and d vars under the bounds.
Prints worst error / bound per quantity (pytest -s)."""
from importlib import import_module

import numpy as np
import pytest
import torch

import w2v_pretrain_ref as R
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
    return import_module("chimera-st_amd.kernels"), import_module("chimera-st_amd.lib"), import_module("chimera-st_amd.rng")


def run(CF, K, x, y, idx, inv_temp, gscale=1.0):
    """loss, nll, counters and both gradients of CF.infonce_loss on device tensors, and the forward's debug logits."""
    x, y = x.detach().requires_grad_(True), y.detach().requires_grad_(True)
    loss, nll, counters = CF.infonce_loss(x, y, idx, 1.0 / inv_temp)
    (loss * gscale).backward()
    logits = K[0].infonce_fwd(x.detach(), y.detach(), idx, inv_temp, want_logits=True)[4]
    c = counters.cpu()
    return dict(loss=loss.detach().cpu(), nll=nll.cpu(), dx=x.grad.cpu(), dy=y.grad.cpu(), logits=logits.cpu(), correct=int(c[0]), count=int(c[1]))


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_infonce_against_fp64(CF, K, name, dtype):
    (x, y, idx, inv_temp, _, _), ref = R.reference(name, dtype)
    assert abs(1.0 / (1.0 / inv_temp) - inv_temp) < 1e-6
    got = run(CF, K, x.cuda(), y.cuda(), idx.cuda(), inv_temp)
    ratios, bad = R.judge(ref, got)
    print("RATIO infonce %-10s %-4s %s" % (name, NAME[dtype], "  ".join("%s %.3f" % kv for kv in ratios.items())))
    assert bad == 0
    assert (got["correct"], got["count"]) == (ref["correct"], ref["count"])
    if name == "planted":  # every negative of position 2 equals its positive: nll 0, zero-bit gradient, no pull on the rows it drew
        assert float(got["nll"][2]) == 0.0 and int(bits(got["dx"][2]).ne(0).sum()) == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
def test_determinism_and_batch_independence(CF, K, dtype):
    """Two runs give identical bits; at Kx = 0 an utterance's numbers equal the utterance run alone."""
    (x, y, idx, inv_temp, (B, M, Kn, Kx), _), _ = R.reference("duplicates", dtype)
    xd, yd, idd = x.cuda(), y.cuda(), idx.cuda()
    a, again = run(CF, K, xd, yd, idd, inv_temp), run(CF, K, xd, yd, idd, inv_temp)
    for k in ("loss", "nll", "dx", "dy", "logits"):
        assert torch.equal(bits(a[k]), bits(again[k])), "two calls differ in " + k
    for b in range(B):
        s = slice(b * M, (b + 1) * M)
        alone = run(CF, K, xd[s], yd[s], (idd[s] - b * M).contiguous(), inv_temp)
        for k in ("nll", "dx", "dy", "logits"):
            assert torch.equal(bits(alone[k]), bits(a[k][s])), "utterance %d: %s" % (b, k)


def test_gradient_scale(CF, K):
    """The upstream gradient arrives as a device scalar: a power of two scales every element exactly."""
    (x, y, idx, inv_temp, _, _), _ = R.reference("cross", torch.float32)
    one, quarter = run(CF, K, x.cuda(), y.cuda(), idx.cuda(), inv_temp), run(CF, K, x.cuda(), y.cuda(), idx.cuda(), inv_temp, gscale=0.25)
    assert torch.equal(one["dx"] * 0.25, quarter["dx"]) and torch.equal(one["dy"] * 0.25, quarter["dy"])


@pytest.mark.parametrize("shape", [(1, 2, 1, 0), (3, 37, 100, 0), (2, 300, 100, 0), (2, 16, 4, 3), (4, 5, 0, 6)])
def test_sampler_equals_numpy_twin(CF, K, shape):
    B, M, Kn, Kx = shape
    _, _, rng = K
    for key in (0, 0x9E3779B9, 0xFFFFFFFF):
        got = CF.sample_negatives(B, M, Kn, Kx, key=key).cpu().numpy()
        assert got.dtype == np.int32 and np.array_equal(got, rng.negatives_numpy(key, B, M, Kn, Kx).reshape(B * M, Kn + Kx))
    rng.reseed(123)
    first = CF.sample_negatives(B, M, Kn, Kx).cpu().numpy()
    rng.reseed(123)
    assert np.array_equal(first, rng.negatives_numpy(rng.next_key(), B, M, Kn, Kx).reshape(B * M, Kn + Kx))


def test_refusals_touch_nothing(K):
    k, lib, _ = K
    N, KP, D = 6, 3, 16
    x, y = torch.randn(N, D, device="cuda"), torch.randn(N, D, device="cuda")
    idx = torch.zeros(N, KP, dtype=torch.int32, device="cuda")
    f = lambda *s: torch.full(s, 7.0, device="cuda")
    i7 = lambda *s: torch.full(s, 7, dtype=torch.int32, device="cuda")
    nll, loss, lse, nx, ny, cnt, flags, dx, pairs = f(N), f(1), f(N), f(N), f(N), i7(2), i7(N), f(N, D), f(N, KP + 1, 2)
    perm, offs = torch.zeros(N * (KP + 1), dtype=torch.int64, device="cuda"), torch.zeros(N + 1, dtype=torch.int32, device="cuda")
    P, last = lib.ptr, lib.load().cst_last_error
    wide = torch.randn(N, 1032, device="cuda")

    def fwd(x_=x, y_=y, N_=N, KP_=KP, D_=D, dtype=0):
        return lib.load().cst_infonce_fwd(P(x_), P(y_), P(idx), 10.0, P(nll), P(loss), P(cnt), P(lse), P(nx), P(ny), P(flags), None,
                                          N_, KP_, D_, dtype, lib.stream_ptr())

    def bwd_x(D_=D, KP_=KP):
        return lib.load().cst_infonce_bwd_x(P(x), P(y), P(idx), 10.0, P(lse), P(nx), P(ny), P(loss), P(dx), P(pairs), N, KP_, D_, 0,
                                            lib.stream_ptr())

    def bwd_y(D_=D):
        return lib.load().cst_infonce_bwd_y(P(x), P(y), P(perm), P(offs), P(pairs), P(nx), P(ny), P(dx), N, KP, D_, 0, lib.stream_ptr())
    for kw, msg in ((dict(D_=12), b"multiple of 8"), (dict(x_=wide, y_=wide, D_=1032), b"multiple of 8"), (dict(dtype=5), b"bad dtype"),
                    (dict(N_=0), b"bad shape"), (dict(KP_=1024), b"negatives exceed"), (dict(x_=x.view(-1)[1:]), b"aligned")):
        assert fwd(**kw) == -1 and msg in last(), kw
    assert bwd_x(D_=12) == -1 and bwd_x(KP_=0) == -1 and bwd_y(D_=20) == -1
    out = i7(2, 1, 4)
    neg = lambda B, M, Kn, Kx, o=out: lib.load().cst_w2v_negatives(1, B, M, Kn, Kx, P(o), lib.stream_ptr())
    assert neg(2, 1, 4, 0) == -1 and b"M >= 2" in last()
    assert neg(1, 1, 0, 4) == -1 and b"B M >= 2" in last()
    assert neg(2, 2, 0, 0) == -1 and neg(0, 2, 1, 0) == -1 and neg(2, 2, 1, 0, None) == -1
    with pytest.raises(RuntimeError, match="multiple of 8"):
        k.infonce_fwd(torch.randn(N, 12, device="cuda"), torch.randn(N, 12, device="cuda"), idx, 10.0)
    torch.cuda.synchronize()
    for t in (nll, loss, lse, nx, ny, dx, pairs):
        assert bool((t == 7.0).all())
    for t in (cnt, flags, out):
        assert bool((t == 7).all())


# ---- Gumbel vector quantizer ----
VQ_KEYS = ("avg_probs", "exph", "prob_perplexity", "code_perplexity")


def vq_fwd(K, c, training, noise=None):
    k = K[0]
    q, idx, onehot, avg, stats, exph = k.gumbel_vq_fwd(c["l"].cuda(), c["vars"].cuda(), c["G"], training, c["key"],
                                                       None if noise is None else noise.cuda())
    return dict(q=q.cpu(), idx=idx.cpu().long(), onehot=onehot.cpu(), avg_probs=avg.cpu(), exph=exph.cpu(),
                prob_perplexity=stats[0].cpu(), code_perplexity=stats[1].cpu())


def check_choice(c, got, idx):
    """q is the chosen codebook row bit for bit, onehot marks it"""
    G, (N, GV) = c["G"], c["l"].shape
    V, d = GV // G, c["vars"].shape[1]
    assert torch.equal(got["idx"], idx)
    rows = (idx + torch.arange(G)[None, :] * V).reshape(-1)
    assert torch.equal(bits(got["q"].reshape(N * G, d)), bits(c["vars"][rows]))
    want = torch.zeros(N * G, V).scatter_(-1, idx.reshape(-1, 1), 1.0).to(c["l"].dtype)
    assert torch.equal(bits(got["onehot"].reshape(N * G, V)), bits(want))


@pytest.mark.parametrize("injected", [False, True], ids=["own_noise", "injected"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("name", sorted(R.VQ_CASES))
def test_vq_forward_and_backward_against_fp64(K, name, dtype, injected):
    """Training mode.  own_noise: the choices equal those made from rng.gumbel_uniform_numpy's uniforms (no choice is undecided at these
    seeds: test_w2v_pretrain_ref_cpu.py), so bits -> u is what the twin says."""
    c, noise, ref = R.vq_reference(name, dtype, injected)
    got = vq_fwd(K, c, True, noise)
    check_choice(c, got, ref["idx"])
    ratios, bad = R.judge(ref, got, keys=VQ_KEYS)
    # backward: avg_probs / exph as the forward kernel left them and a gy rounded to the storage type are its exact inputs
    gy = ref["gy"].to(dtype)
    rb = R.vq_eval(c, noise=noise, a_in=got["avg_probs"], exph_in=got["exph"], gy=gy, with_bounds=True, store=dtype)
    dppl = torch.tensor([c["dppl"]], device="cuda")
    run_b = lambda: K[0].gumbel_vq_bwd(c["l"].cuda(), gy.cuda(), got["avg_probs"].cuda(), got["exph"].cuda(), dppl, c["G"], c["inv_tau"],
                                       c["key"], None if noise is None else noise.cuda()).cpu()
    dl = run_b()
    rb_ratios, rb_bad = R.judge(rb, dict(dl=dl), keys=("dl",))
    print("RATIO vq %-10s %-4s %-9s %s  dl %.3f" % (name, NAME[dtype], "injected" if injected else "own", "  ".join("%s %.3f" % kv for kv in ratios.items()),
                                                 rb_ratios["dl"]))
    assert bad == 0 and rb_bad == 0
    again = vq_fwd(K, c, True, noise)
    for k in ("q", "idx", "onehot") + VQ_KEYS:
        assert torch.equal(got[k], again[k]), "two calls differ in " + k
    assert torch.equal(bits(dl), bits(run_b()))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
def test_vq_eval_mode_and_planted_ties(K, dtype):
    c, _, _ = R.vq_reference("two_groups", dtype)
    c = dict(c, l=c["l"].clone())
    N, G, V = 67, 2, 320
    l3 = c["l"].view(N, G, V)
    l3[0, 0, 70] = l3[0, 0, 5] = 30.0       # an exact tie across two lanes' classes
    l3[1, 1, 300] = l3[1, 1, 301] = 30.0    # and between neighbours
    l3[2, 0, :] = 1.5                       # a constant row: code 0
    ref = R.vq_eval(c, training=False, with_bounds=False)
    got = vq_fwd(K, c, False)
    assert got["idx"][0, 0] == 5 and got["idx"][1, 1] == 300 and got["idx"][2, 0] == 0
    check_choice(c, got, ref["idx"])


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("name", sorted(R.VQ_CASES))
def test_vq_functional_gradients(CF, K, name, dtype):
    """functional.gumbel_vector_quantize end to end: d vars (the weight-gradient GEMM on the one-hot) and gy (the K = d product) under
    their bounds; d logits equal, bit for bit, the backward kernel fed with that gy (judged above)."""
    k = K[0]
    c, _, ref = R.vq_reference(name, dtype)
    G, (N, GV) = c["G"], c["l"].shape
    V, d = GV // G, c["vars"].shape[1]
    l, vr = c["l"].cuda().requires_grad_(True), c["vars"].cuda().requires_grad_(True)
    q, ppl, cpl, idx, avg = CF.gumbel_vector_quantize(l, vr, G, 1.0 / c["inv_tau"], training=True, key=c["key"])
    assert torch.equal(idx.cpu().long(), ref["idx"])
    ((q.float() * c["dq"].cuda().float()).sum() + c["dppl"] * ppl).backward()
    dq = c["dq"].cuda()
    gy = torch.empty(N, GV, dtype=dtype, device="cuda")
    for g in range(G):
        k.gemm(dq, vr.detach(), gy, N, V, d, a_kmajor=1, b_kmajor=1, lda=G * d, ldb=d, ldc=GV, a_off=g * d, b_off=g * V * d, c_off=g * V, split_k=1)
    ratios, bad = R.judge(ref, dict(dvars=vr.grad.cpu(), gy=gy.cpu()), keys=("dvars", "gy"))
    print("RATIO vq functional %-10s %-4s dvars %.3f gy %.3f" % (name, NAME[dtype], ratios["dvars"], ratios["gy"]))
    assert bad == 0
    exph = k.gumbel_vq_fwd(l.detach(), vr.detach(), G, True, c["key"])[5]
    dl = k.gumbel_vq_bwd(l.detach(), gy, avg, exph, torch.tensor([c["dppl"]], device="cuda"), G, c["inv_tau"], c["key"])
    assert torch.equal(bits(l.grad.cpu()), bits(dl.cpu()))


def test_vq_refusals_touch_nothing(K):
    k, lib, _ = K
    N, G, V, d = 4, 2, 8, 8
    l, vr = torch.randn(N, G * V, device="cuda"), torch.randn(G * V, d, device="cuda")
    f = lambda *s: torch.full(s, 7.0, device="cuda")
    q, oh, avg, st, ex, ws, dl = f(N, G * d), f(N, G * V), f(G, V), f(2), f(G), f(1024), f(N, G * V)
    idx = torch.full((N, G), 7, dtype=torch.int32, device="cuda")
    P, last = lib.ptr, lib.load().cst_last_error

    def fwd(V_=V, d_=d, dtype=0, N_=N, vars_=vr):
        return lib.load().cst_gumbel_vq_fwd(P(l), P(vars_), None, 1, 1, P(q), P(idx), P(oh), P(avg), P(st), P(ex), P(ws), N_, G, V_, d_, dtype,
                                            lib.stream_ptr())
    for kw, msg in ((dict(V_=1025), b"exceed the supported"), (dict(d_=12), b"multiple of 8"), (dict(dtype=2), b"bad dtype"), (dict(N_=0), b"bad shape"),
                    (dict(vars_=None), b"null operand")):
        assert fwd(**kw) == -1 and msg in last(), kw
    bwd = lambda it, V_=V: lib.load().cst_gumbel_vq_bwd(P(l), None, 1, it, P(l), P(avg), P(ex), P(st), P(dl), N, G, V_, 0, lib.stream_ptr())
    assert bwd(0.0) == -1 and b"positive" in last()
    assert bwd(1.0, 2048) == -1 and b"exceed the supported" in last()
    with pytest.raises(ValueError, match="one dtype"):
        k.gumbel_vq_fwd(l, vr.bfloat16(), G, True)
    torch.cuda.synchronize()
    for t in (q, oh, avg, st, ex, ws, dl):
        assert bool((t == 7.0).all())
    assert bool((idx == 7).all())


def test_quantizer_module(K):
    """wav2vec2.GumbelVectorQuantizer on the fused kernels against the reference module's formulas in fp64 (a recorded noise replayed):
    quantised features, targets, perplexities and every parameter gradient within the project's 1e-3; eval mode; the temperature."""
    load_pkg()
    W = import_module("chimera-st_amd.wav2vec2")
    torch.manual_seed(5)
    B, T, C, V, G, vq = 3, 11, 32, 8, 2, 16
    m = W.GumbelVectorQuantizer(C, V, G, vq, temp=(2.0, 0.5, 0.9)).cuda()
    assert [k for k, _ in m.named_parameters()] == ["vars", "weight_proj.weight", "weight_proj.bias"]
    m.set_num_updates(3)
    assert m.curr_temp == 2.0 * 0.9 ** 3
    m.set_num_updates(1000)
    assert m.curr_temp == 0.5
    m.set_num_updates(3)
    x = torch.randn(B, T, C)
    noise = -torch.log(torch.empty(B * T, G, V).exponential_())
    w64, b64, v64 = (p.detach().cpu().double().requires_grad_(True) for p in (m.weight_proj.weight, m.weight_proj.bias, m.vars))
    c = dict(l=torch.nn.functional.linear(x.double(), w64, b64).reshape(B * T, G * V), vars=v64[0], dq=None, dppl=0.3, inv_tau=1.0 / m.curr_temp, G=G)
    dq = torch.randn(B * T, vq)
    # the reference's forward on these logits, spelt out (w2v_pretrain_ref.vq_torch_composition without its detach of the inputs)
    l2 = c["l"].reshape(B * T * G, V)
    avg = torch.softmax(l2.view(B * T, G, V), -1).mean(0)
    ppl = torch.exp(-(avg * torch.log(avg + 1e-7)).sum(-1)).sum()
    ys = ((l2 + noise.double().reshape(-1, V)) * c["inv_tau"]).softmax(-1)
    idx = ys.argmax(-1, keepdim=True)
    ret = torch.zeros_like(l2).scatter_(-1, idx, 1.0) - ys.detach() + ys
    q = (ret.view(B * T, G * V, 1) * v64).view(B * T, G, V, -1).sum(-2).view(B * T, -1)
    ((q * dq.double()).sum() + 0.3 * ppl).backward()
    m.train()
    res = m(x.cuda(), produce_targets=True, noise=noise.cuda())
    assert res["x"].shape == (B, T, vq) and res["targets"].shape == (B, T, G) and res["num_vars"] == G * V and res["temp"] == m.curr_temp
    assert torch.equal(res["targets"].cpu().reshape(-1, 1), idx)
    ((res["x"].reshape(B * T, vq) * dq.cuda()).sum() + 0.3 * res["prob_perplexity"]).backward()
    close = lambda a, b: float((a.detach().cpu().double() - b).abs().max()) <= 1e-3 * max(1.0, float(b.abs().max()))
    assert close(res["x"].reshape(B * T, vq), q.detach()) and close(res["prob_perplexity"], ppl.detach())
    for p, r in ((m.weight_proj.weight, w64), (m.weight_proj.bias, b64), (m.vars, v64)):
        assert close(p.grad, r.grad)
    m.eval()
    xq, tg = m.forward_idx(x.cuda())
    assert torch.equal(tg.cpu().reshape(-1, 1), l2.argmax(-1, keepdim=True)) and torch.equal(xq, m.quantize(x.cuda()))
    m.train()
    rng = K[2]
    rng.reseed(9)
    a = m(x.cuda())["x"]
    rng.reseed(9)
    assert torch.equal(a, m(x.cuda())["x"]), "the noise does not follow the update's seed"
