"""cst_ctc_topn and cst_ctc_beam (csrc/ctc_decode.hip) against the fp64 restatement and the counted bounds of ctc_beam_ref.py: the
per-frame lists, exact cases (tokens and order of every hypothesis, brute force, the host route), step replay through the trace at
the long shapes, batch independence, refusals."""
import ctypes
import functools
import math
from importlib import import_module

import numpy as np
import pytest
import torch

import ctc_beam_ref as R
from conftest import load_pkg
from ctc_ref import SLACK, U32

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]


@functools.lru_cache(maxsize=None)
def mods():
    load_pkg()
    return (import_module("chimera-st_amd.kernels"), import_module("chimera-st_amd.functional"), import_module("chimera-st_amd.ctc_decoder"),
            import_module("chimera-st_amd.lib"))


def grid_logits(T, B, V, seed, dtype, std=3.0):
    """Logits on a grid of 1/16: neighbours in the order differ by far more than any bound, or are exact ties (broken by class id)."""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return (torch.round(torch.randn(T, B, V, generator=g) * std * 16) / 16).to(dtype)


def judge_topn(x, in_len, blank, N, got, dtype):
    """ids exact, log-probabilities within dl + u |lp| of the fp64 ones; frames past the length -1 / -inf."""
    lse, blp, tid, tlp = (t.cpu() for t in got)
    T, B, V = x.shape
    worst = 0.0
    for b in range(B):
        n = int(in_len[b])
        if n:
            lp, dl = R.row_terms(x[:n, b].double().numpy(), dtype)
        for t in range(T):
            if t >= n:
                assert tid[b, t].eq(-1).all() and torch.isinf(tlp[b, t]).all() and blp[b, t] == float("-inf") and lse[b, t] == 0
                continue
            ids = R.top_list(lp[t], blank, N)
            assert tid[b, t, :len(ids)].tolist() == ids, (b, t)
            assert tid[b, t, len(ids):].eq(-1).all() and (tlp[b, t, len(ids):] == float("-inf")).all()
            ref = np.array([lp[t, blank]] + [lp[t, c] for c in ids])
            g = np.array([float(blp[b, t])] + tlp[b, t, :len(ids)].double().tolist())
            bound = (dl[t] + U32 * np.abs(ref)) * SLACK
            worst = max(worst, float((np.abs(g - ref) / bound).max()))
            assert (np.abs(g - ref) <= bound).all(), (b, t, float((np.abs(g - ref) / bound).max()))
    return worst


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("T,B,V,N,blank", [(7, 2, 5, 3, 0), (7, 2, 5, 8, 0), (9, 3, 32, 31, 0), (9, 2, 32, 4, 31), (5, 2, 513, 100, 0),
                                           (5, 2, 1000, 128, 999), (3, 2, 10000, 100, 0)])
def test_topn_lists(T, B, V, N, blank, dtype):
    K, _, _, _ = mods()
    x = grid_logits(T, B, V, 11 + V, dtype)
    x[1, 0, :] = x[1, 0, 0]  # a row of equal logits: the lowest ids first
    in_len = torch.tensor([T, max(T - 3, 1), 0][:B], dtype=torch.int64)
    xg = x.clone()
    for b in range(B):
        xg[int(in_len[b]):, b] = float("nan")  # frames past the length must not be read
    got = K.ctc_topn(xg.cuda(), in_len.cuda(), blank, N, check=True)
    print("topn worst err / bound", judge_topn(x, in_len, blank, N, got, dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("V", [32, 513, 1001])
def test_topn_layouts_give_equal_bits(V, dtype):
    K, _, _, _ = mods()
    T, B, N = 6, 3, 20
    x = grid_logits(T, B, V, 5, dtype).cuda()
    in_len = torch.tensor([T, T - 2, 1], dtype=torch.int64).cuda()
    ref = K.ctc_topn(x, in_len, 0, N)
    bm = x.transpose(0, 1).contiguous().transpose(0, 1)  # the time-major view of batch-major memory
    assert bm.stride(0) == V and bm.stride(1) == T * V
    flat = torch.empty(T * B * V + 8, dtype=dtype, device="cuda")
    un = flat[1:1 + T * B * V].view(T, B, V)  # an unaligned base
    un.copy_(x)
    assert un.data_ptr() % 16 != 0
    for other in (bm, un):
        got = K.ctc_topn(other, in_len, 0, N)
        for a, b in zip(ref, got):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    judge_topn(x.cpu(), in_len.cpu(), 0, N, ref, dtype)


def run_device(x, in_len, blank, c, nbest, trace=False):
    _, CF, _, _ = mods()
    return CF.ctc_prefix_beam_search(x.cuda(), torch.tensor(in_len, dtype=torch.int64).cuda(), blank, c["K"], c["N"],
                                     c.get("theta", math.inf), nbest, trace=trace)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", sorted(R.EXACT_CASES))
def test_exact_cases(name, dtype):
    """Tokens and order of all nbest hypotheses equal the fp64 restatement's, scores within the counted bound; the host route gives the
    same hypotheses; the brute-force cases equal the enumeration."""
    _, _, D, _ = mods()
    x, in_len, blank, c, res = R.exact_case(name, dtype)
    nbest = c.get("nbest", min(c["K"], 5))
    got = run_device(x, in_len, blank, c, nbest)
    host = D.prefix_beam_search_host(x, in_len, blank, c["K"], c["N"], c.get("theta", math.inf), nbest)
    for b, r in enumerate(res):
        want = r["hyps"][:nbest]
        assert [tuple(h[0]) for h in got[b]] == [h[0] for h in want], (b, got[b][:2], want[:2])
        assert [tuple(h[0]) for h in host[b]] == [h[0] for h in want]
        err = max(abs(g[1] - w[1]) for g, w in zip(got[b], want))
        print(name, b, "score err %.3g bound %.3g gap %.3g" % (err, r["bound"], r["gap"]))
        assert err <= r["bound"]
        assert max(abs(g[1] - w[1]) for g, w in zip(host[b], want)) <= 1e-9
        if in_len[b] == 0:
            assert got[b] == [([], 0.0)]
    if name.startswith("brute"):
        lp, _ = R.row_terms(x[:, 0].double().numpy(), dtype)
        br = R.brute(lp, blank)
        top = max(br, key=br.get)
        assert tuple(got[0][0][0]) == top and abs(got[0][0][1] - br[top]) <= res[0]["bound"]
        if name == "brute4":  # unpruned: every labelling is in the beam
            full = run_device(x, in_len, blank, c, c["K"])[0]
            assert {tuple(h[0]) for h in full} == set(br)
            assert max(abs(s - br[tuple(h)]) for h, s in full) <= res[0]["bound"]


def replay(x, in_len, blank, K, N, theta, dtype, hyps, tr):
    worst = 0.0
    for b in range(x.shape[1]):
        n = int(in_len[b])
        lp, dl = R.row_terms(x[:n, b].double().numpy(), dtype)
        par, tok = tr["nodes"][b, 0], tr["nodes"][b, 1]
        labs = {0: ()}

        def lab(nd):
            if nd not in labs:
                labs[nd] = lab(int(par[nd])) + (int(tok[nd]),)
            return labs[nd]
        prev = [((), 0.0, R.NINF)]
        for t in range(n):
            live = tr["node"][b, t] >= 0
            nxt = [(lab(int(nd)), float(pb), float(pnb)) for nd, pb, pnb in zip(tr["node"][b, t][live], tr["pb"][b, t][live], tr["pnb"][b, t][live])]
            ok, why, bound = R.check_step(prev, dict(lp=lp[t], dl=dl[t], blank=blank, K=K, N=N, theta=theta), nxt)
            assert ok, (b, t, why)
            prev = nxt
        assert [tuple(h[0]) for h in hyps[b]] == [p[0] for p in prev[:len(hyps[b])]]
        for h, p in zip(hyps[b], prev):
            assert abs(h[1] - R.lae(p[1], p[2])) <= U32 * (3.8 + abs(h[1])) * SLACK
    return worst


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("T,V,K,N,std", [(600, 32, 50, 31, 2.0), (40, 1000, 64, 100, 2.0), (1499, 32, 8, 31, 2.0)])
def test_step_replay(T, V, K, N, std, dtype):
    """Every frame of the traced search is a legal step of the fp64 restatement from the beam the kernel itself held; the hypotheses
    are the final beam's, in order."""
    x = R.make_logits(T, V, 3, std, torch.float32).to(dtype)[:, None, :]
    c = dict(K=K, N=N)
    hyps, tr = run_device(x, (T,), 0, c, min(K, 10), trace=True)
    replay(x, (T,), 0, K, N, math.inf, dtype, hyps, tr)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_batch_independence_and_bit_reproducibility(dtype):
    K, _, _, _ = mods()
    T, B, V, Kb, N = 50, 3, 40, 16, 12
    x = grid_logits(T, B, V, 21, dtype, std=1.0).cuda()
    in_len = torch.tensor([50, 17, 33], dtype=torch.int64).cuda()

    def run(xx, ll):
        r = K.ctc_beam(xx, ll, 0, K.ctc_topn(xx, ll, 0, N), Kb, 4.0, Kb, check=True)
        return r["packed"].clone()
    whole = run(x, in_len)
    assert torch.equal(whole, run(x, in_len))
    nb = Kb
    for b in range(B):
        one = run(x[:, b:b + 1].contiguous(), in_len[b:b + 1])
        tok = whole[:B * nb * T].view(B, nb, T)[b]
        ln = whole[B * nb * T:B * nb * T + B * nb].view(B, nb)[b]
        sc = whole[B * nb * T + B * nb:B * nb * T + 2 * B * nb].view(B, nb)[b]
        assert torch.equal(one[:nb * T].view(nb, T), tok) and torch.equal(one[nb * T:nb * T + nb], ln)
        assert torch.equal(one[nb * T + nb:nb * T + 2 * nb], sc) and one[-1] == whole[B * nb * T + 2 * B * nb + b]


def test_refusals_touch_nothing():
    K, _, _, L = mods()
    lib = L.load()
    T, B, V, N, Kb = 4, 2, 8, 4, 4
    x = torch.randn(T, B, V, device="cuda")
    il = torch.full((B,), T, dtype=torch.int64, device="cuda")
    lists = K.ctc_topn(x, il, 0, N)
    f = lambda *s: torch.full(s, 7.0, device="cuda")
    i = lambda *s: torch.full(s, 7, dtype=torch.int32, device="cuda")
    o_lse, o_blp, o_id, o_lp = f(B, T), f(B, T), i(B, T, N), f(B, T, N)
    p = L.ptr

    def topn(logits, dtype, n):
        return lib.cst_ctc_topn(logits, B * V, V, p(il), 0, n, p(o_lse), p(o_blp), p(o_id), p(o_lp), T, B, V, dtype, L.stream_ptr())
    assert topn(None, 0, N) == -1 and b"null operand" in lib.cst_last_error()
    assert topn(p(x), 7, N) == -1 and b"bad dtype" in lib.cst_last_error()
    rc_unsup = topn(p(x), 0, 129)
    assert rc_unsup not in (0, -1)
    h_tok, h_len, h_sc, h_n = i(B, Kb, T), i(B, Kb), f(B, Kb), i(B)
    ws = torch.zeros(int(lib.cst_ctc_beam_workspace_bytes(T, B, 200, N)) // 4, dtype=torch.int32, device="cuda")

    def beam(logits, dtype, k, n):
        return lib.cst_ctc_beam(logits, B * V, V, p(il), 0, p(lists[0]), p(lists[1]), p(lists[2]), p(lists[3]), n, k, 25.0, min(k, Kb), p(ws),
                                p(h_tok), p(h_len), p(h_sc), p(h_n), None, None, None, T, B, V, dtype, L.stream_ptr())
    assert beam(None, 0, Kb, N) == -1
    assert beam(p(x), 7, Kb, N) == -1
    assert beam(p(x), 0, 129, N) == rc_unsup and b"beyond the supported" in lib.cst_last_error()
    assert beam(p(x), 0, 128, 128) == rc_unsup
    torch.cuda.synchronize()
    for t in (o_lse, o_blp, o_lp, h_sc):
        assert bool((t == 7.0).all())
    for t in (o_id, h_tok, h_len, h_n):
        assert bool((t == 7).all())
    assert not bool(ws.any())
    with pytest.raises(ValueError):
        K.ctc_beam(x, il, 0, lists, 129, 25.0, 1, check=True)


def test_beyond_envelope_decoder_takes_host_route():
    """K = 200 is beyond the envelope: CtcBeamDecoder lands on the host route; on the unpruned brute-force case the result equals the
    device's at K = 128 (all 64 labellings fit either beam)."""
    from argparse import Namespace
    _, _, D, _ = mods()
    x, in_len, blank, c, res = R.exact_case("brute4", torch.float32)

    class Dict:
        indices = {}

        def __len__(self):
            return c["V"]

        def bos(self):
            return blank
    mk = lambda k: D.CtcBeamDecoder(Namespace(beam=k, nbest=64, beam_threshold=math.inf, beam_size_token=3), Dict())
    il = torch.tensor(in_len, dtype=torch.int64)
    far, near = mk(200), mk(128)
    a, b = far.decode(x.cuda(), il.cuda()), near.decode(x.cuda(), il.cuda())
    assert far.last_route == "host" and near.last_route == "device"
    assert [h["tokens"].tolist() for h in a[0]] == [h["tokens"].tolist() for h in b[0]] == [list(h[0]) for h in res[0]["hyps"]]
    assert max(abs(p["score"] - q["score"]) for p, q in zip(a[0], b[0])) <= res[0]["bound"]
