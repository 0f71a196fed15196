"""The fused attention training kernels — cst_attn_fwd / cst_attn_bwd on the generic route (attn_fwd_kernel, attn_delta_kernel,
attn_bwd_dq_kernel, attn_bwd_dkv_kernel) and on the LDS-DMA route (fa_fwd_kernel, fa_dq_kernel, fa_dkv_kernel) — on a real MI355X against
the fp64 restatements of attn_ref.py, under ITS per-element bounds (counted from the kernels' operation sequences; test_attn_ref_cpu.py
shows that a faithful fp32 evaluation stays inside them and that every listed defect leaves them).  Every element of o, lse, dQ, dK and dV
is compared; no element is exempt.  The backward runs on the forward kernel's own o and lse, as a training step does (the bounds carry the
forward's).  Exact: rows without a key give o = dQ = 0 and lse = -inf, masked keys give dK = dV = 0, nothing is NaN, and a packed (seq=)
call equals the padded call bit for bit on the kept rows.  Every fast-eligible case runs on both routes (CST_ATTN_GENERIC, read per call)
and the route is asserted from STATS["attn_fast"].

Every comparison prints `RATIO <route> <case> <output> worst err/bound`, and the module prints the worst ratio per route and output at its
end (pytest -s)."""
import functools
from importlib import import_module

import pytest
import torch

import attn_ref as R
from conftest import load_pkg

pytestmark = pytest.mark.gpu
WORST = {}
DROP_KEY = 4242
MARGIN = 9      # padding rows a packed sequence keeps behind its real ones (+ one more), as functional.plan_packed_rows does


@pytest.fixture(scope="module")
def KL():
    load_pkg()
    yield import_module("chimera-st_amd.kernels"), import_module("chimera-st_amd.rng")
    print()
    for key in sorted(WORST):
        print("WORST attn %-8s %-4s %.3f" % (key + (WORST[key],)))


@functools.lru_cache(maxsize=None)
def _inputs(name):
    return R.inputs(R.CASES[name])


def _keep(rng, c):
    if c["drop"] == 0:
        return None
    return torch.from_numpy(rng.keep_mask_attn_numpy(DROP_KEY, c["Bn"] * c["H"] * c["Tq"], c["Tk"], c["drop"])).view(c["Bn"], c["H"], c["Tq"], c["Tk"])


def within(got, ref, bound, route, name, what):
    got = got.detach().cpu()
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(bound).all()), "%s %s: the reference is not finite" % (name, what)
    assert bool(torch.isfinite(got.float()).all()), "%s %s %s: non-finite output" % (route, name, what)
    ratio, bad = R.worst_ratio(got, ref, bound)
    WORST[(route, what)] = max(WORST.get((route, what), 0.0), ratio)
    print("RATIO %-7s %-28s %-4s worst err/bound %.3f" % (route, name, what, ratio))
    assert bad == 0, "%s %s %s: %d of %d elements outside the bound, worst err/bound %.3f" % (route, name, what, bad, got.numel(), ratio)


def _set_route(monkeypatch, c, route):
    if route == "generic" and R.fast_eligible(c):
        monkeypatch.setenv("CST_ATTN_GENERIC", "1")
    else:
        monkeypatch.delenv("CST_ATTN_GENERIC", raising=False)


def _full(shape, dt):
    return torch.full(shape, R.GARBAGE, dtype=dt, device="cuda")


def _run(k, c, inp, route):
    """Forward and backward through the descriptor calls on pre-filled outputs -> dict of R.OUTS in the 'bt' layout (GPU tensors)."""
    Bn, H, D, Tq, Tk, dt = c["Bn"], c["H"], c["D"], c["Tq"], c["Tk"], c["dt"]
    C = H * D
    q, kk, v, do = (inp[n].cuda() for n in ("q", "k", "v", "do"))
    lay = c["layout"]
    if c["slices"]:                       # K / V and the three gradients as channel slices of packed buffers (Tq == Tk)
        qkv = torch.cat([q, kk, v], -1).contiguous()
        q, kk, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
        g = _full((Bn, Tq, 3 * C), dt)
        dq, dk, dv = g[..., :C], g[..., C:2 * C], g[..., 2 * C:]
    else:
        if lay == "tb":
            q, kk, v, do = (t.transpose(0, 1).contiguous() for t in (q, kk, v, do))
        dq, dk, dv = _full(q.shape, dt), _full(kk.shape, dt), _full(v.shape, dt)
    o = _full(q.shape, dt)
    lse = _full((Bn, H, Tq), torch.float32)
    kpm = None if inp["masked"] is None else inp["masked"].to(torch.uint8).contiguous().cuda()
    kv_len = None if inp["kv_len"] is None else inp["kv_len"].cuda()
    before = k.STATS.get("attn_fast", 0)
    d = k.attn_desc(q, kk, v, o, lse, H, D, kpm, c["causal"], inp["scale"], lay, lay, c["drop"], DROP_KEY, kv_len)
    k.attn_fwd_desc(d)
    delta = torch.empty_like(lse)
    k.attn_bwd_fill(d, do, dq, dk, dv, delta, D, lay, lay)
    k.attn_bwd_desc(d)
    torch.cuda.synchronize()
    assert k.STATS.get("attn_fast", 0) - before == (1 if route == "fast" else 0), "%s did not take the %s route" % (c["name"], route)
    bt = (lambda t: t.transpose(0, 1)) if lay == "tb" else (lambda t: t)
    return dict(o=bt(o), lse=lse, dq=bt(dq), dk=bt(dk), dv=bt(dv))


@pytest.mark.parametrize("name,route", R.RUNS, ids=["%s-%s" % (r, n) for n, r in R.RUNS])
def test_attention_under_counted_bounds(KL, monkeypatch, name, route):
    k, rng = KL
    c, inp = R.CASES[name], _inputs(name)
    _set_route(monkeypatch, c, route)
    r = R.ref64(c, inp, route, _keep(rng, c))
    got = {n: t.cpu() for n, t in _run(k, c, inp, route).items()}
    for n in R.OUTS:
        assert not bool(torch.isnan(got[n].float()).any()), "%s %s: NaN in %s" % (route, name, n)
    fin = torch.isfinite(r["lse"])
    assert bool((got["lse"][~fin] == R.NINF).all()), "lse of a row without a key must be -inf"
    assert bool(torch.isfinite(got["lse"][fin]).all())
    zero = lambda t: torch.zeros_like(t)
    within(torch.where(fin, got["lse"], zero(got["lse"])), torch.where(fin, r["lse"], zero(r["lse"])), r["b_lse"], route, name, "lse")
    for n in ("o", "dq", "dk", "dv"):
        within(got[n], r[n], r["b_" + n], route, name, n)
    dead = r["dead"]
    if bool(dead.any()):
        dflat = dead.transpose(1, 2)[..., None].expand(-1, -1, -1, c["D"]).reshape(c["Bn"], c["Tq"], -1)
        assert bool((got["o"][dflat] == 0).all()) and bool((got["dq"][dflat] == 0).all()), "rows without a key must give exact zeros"
        for b in range(c["Bn"]):
            if bool(dead[b].all()):      # an utterance without a key contributes nothing to dK / dV
                assert bool((got["dk"][b] == 0).all()) and bool((got["dv"][b] == 0).all())
    if inp["masked"] is not None:
        mk = inp["masked"]
        assert bool((got["dk"][mk] == 0).all()) and bool((got["dv"][mk] == 0).all()), "dK / dV of masked keys must be exact zeros"
    if c["do_zero"]:
        z = R.dozero_rows(c["Tq"])
        assert bool((got["dq"][:, z] == 0).all()), "dQ of rows with dO = 0 must be exact zeros"


PACKED = [n for n, c in R.CASES.items() if R.fast_eligible(c) and c["mask"] == "suffix" and c["Tq"] == c["Tk"]]


@pytest.mark.parametrize("name", PACKED)
def test_packed_call_equals_the_padded_call_bit_for_bit(KL, monkeypatch, name):
    """Each suffix-masked fast self-attention case (the launcher takes packed rows for Tq == Tk only) again with seq=: the kept rows of
    o, lse, dQ, dK, dV equal the padded call's, whose dO is zero behind the kept rows."""
    k, _ = KL
    c, inp = R.CASES[name], _inputs(name)
    assert PACKED and min(c["marg"]) > 0
    monkeypatch.delenv("CST_ATTN_GENERIC", raising=False)
    Bn, H, D, T = c["Bn"], c["H"], c["D"], c["Tq"]
    C = H * D
    lens = list(c["marg"])
    kept = [min(T, n + MARGIN + 1) for n in lens]
    off = [0]
    for n in kept:
        off.append(off[-1] + n)
    rows, longest = off[-1], max(kept)
    qkv = torch.cat([inp[n] for n in ("q", "k", "v")], -1).cuda().contiguous()
    do = inp["do"].cuda().clone()
    for b in range(Bn):
        do[b, kept[b]:] = 0
    kpm = inp["masked"].to(torch.uint8).contiguous().cuda()
    kv_len = None if inp["kv_len"] is None else inp["kv_len"].cuda()
    before = k.STATS.get("attn_fast", 0)
    o, lse = _full((Bn, T, C), R.B), _full((Bn, H, T), torch.float32)
    d = k.attn_desc(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], o, lse, H, D, kpm, False, inp["scale"], "bt", "bt", 0.0, 0, kv_len)
    k.attn_fwd_desc(d)
    g = _full((Bn, T, 3 * C), R.B)
    k.attn_bwd_fill(d, do, g[..., :C], g[..., C:2 * C], g[..., 2 * C:], torch.empty_like(lse), D)
    k.attn_bwd_desc(d)
    pack = lambda x: torch.cat([x[b, :kept[b]] for b in range(Bn)], 0).unsqueeze(0).contiguous()
    pq, pdo = pack(qkv), pack(do)
    po, plse = _full((1, rows, C), R.B), _full((Bn, H, longest), torch.float32)
    offd = torch.tensor(off, dtype=torch.int32, device="cuda")
    lend = torch.tensor(lens, dtype=torch.int32, device="cuda")
    d2 = k.attn_desc(pq[..., :C], pq[..., C:2 * C], pq[..., 2 * C:], po, plse, H, D, None, False, inp["scale"], "bt", "bt", 0.0, 0, lend, (offd, longest))
    k.attn_fwd_desc(d2)
    pg = _full((1, rows, 3 * C), R.B)
    k.attn_bwd_fill(d2, pdo, pg[..., :C], pg[..., C:2 * C], pg[..., 2 * C:], torch.empty_like(plse), D)
    k.attn_bwd_desc(d2)
    torch.cuda.synchronize()
    assert k.STATS.get("attn_fast", 0) - before == 2
    for b in range(Bn):
        sl = slice(off[b], off[b + 1])
        assert torch.equal(po[0, sl], o[b, :kept[b]]), "output rows of sequence %d" % b
        assert torch.equal(plse[b, :, :kept[b]], lse[b, :, :kept[b]]), "lse of sequence %d" % b
        assert torch.equal(pg[0, sl], g[b, :kept[b]]), "gradient rows of sequence %d" % b
