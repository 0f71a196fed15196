"""attn_ref.py checks itself, without a GPU: on every case and route that test_attn_gpu.py runs, a faithful fp32 op-by-op evaluation of the
attention training kernels (forward, dQ, dK / dV; the backward on the emulated forward's own o and lse) stays inside every counted bound
(bad == 0, worst err / bound < 1, printed), and every listed defect, planted into the same evaluation, leaves the bound on the case named
for it.  What the planted cases are meant to reach is asserted from the fp64 scores: the raises of the lazy maximum per planted row, the
wholly masked leading tiles, the rows without a key."""
import functools

import pytest
import torch

import attn_ref as R

WORST = {}


@functools.lru_cache(maxsize=None)
def _setup(name, route):
    c = R.CASES[name]
    inp = R.inputs(c)
    keep = R.cpu_keep(c) if c["drop"] > 0 else None
    return c, inp, keep, R.ref64(c, inp, route, keep)


def _ratios(got, r):
    return {n: R.worst_ratio(got[n], r[n], r["b_" + n]) for n in got}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print()
    for key in sorted(WORST):
        print("WORST %-8s %-4s faithful emulation err/bound %.3f" % (key + (WORST[key],)))


@pytest.mark.parametrize("name,route", R.RUNS, ids=["%s-%s" % (r, n) for n, r in R.RUNS])
def test_faithful_emulation_is_inside_every_bound(name, route):
    c, inp, keep, r = _setup(name, route)
    got = R.emulate32(c, inp, route, keep)
    for n in R.OUTS:
        assert not bool(torch.isnan(got[n].float()).any()), "%s: NaN in %s" % (name, n)
    fin = torch.isfinite(r["lse"])
    assert torch.equal(torch.isfinite(got["lse"]), fin) and bool((got["lse"][~fin] == R.NINF).all())
    for n, (ratio, bad) in _ratios({n: (torch.where(fin, got[n], torch.zeros_like(got[n])) if n == "lse" else got[n]) for n in R.OUTS},
                                   dict(r, lse=torch.where(fin, r["lse"], torch.zeros_like(r["lse"])))).items():
        print("RATIO %-7s %-28s %-4s faithful worst err/bound %.3f" % (route, name, n, ratio))
        WORST[(route, n)] = max(WORST.get((route, n), 0.0), ratio)
        assert bad == 0 and ratio < 1.0, "%s %s %s: %d elements outside the bound, worst err/bound %.3f" % (route, name, n, bad, ratio)
    # rows without a key: zeros and -inf, exactly
    dead = r["dead"]
    if bool(dead.any()):
        dflat = dead.transpose(1, 2)[..., None].expand(-1, -1, -1, c["D"]).reshape(c["Bn"], c["Tq"], -1)
        assert bool((got["o"][dflat] == 0).all()) and bool((got["dq"][dflat] == 0).all())
    if inp["masked"] is not None:
        mk = inp["masked"]
        assert bool((got["dk"][mk] == 0).all()) and bool((got["dv"][mk] == 0).all())


@pytest.mark.parametrize("defect", sorted(R.DEFECTS))
def test_defect_leaves_the_bound(defect):
    name, route, outs = R.DEFECTS[defect]
    c, inp, keep, r = _setup(name, route)
    got = R.emulate32(c, inp, route, keep, defect, want=outs)
    fin = torch.isfinite(r["lse"])
    hit = []
    for n in outs:
        g, ref = got[n], r[n]
        if n == "lse":
            g, ref = torch.where(fin, g, torch.zeros_like(g)), torch.where(fin, ref, torch.zeros_like(ref))
        ratio, bad = R.worst_ratio(g, ref, r["b_" + n])
        print("DEFECT %-42s %-28s %-4s worst err/bound %.3g, %d outside" % (defect, name, n, ratio, bad))
        hit.append(bad)
    assert sum(hit) > 0, "%s stays inside the bounds of %s on %s: they are blind to it" % (defect, outs, name)


def test_every_named_defect_case_exists():
    for name, route, outs in R.DEFECTS.values():
        assert (name, route) in R.RUNS and set(outs) <= set(R.OUTS)


def test_climb_raises_on_planted_rows_only():
    """climb: every planted row raises the lazy maximum at each of the 8 tiles (the first set and 7 raises), and every wave (32 rows) also
    holds rows that only set it once: both arms of the wave-uniform branch run in one wave.  descend sets it once and the last tile's
    probabilities underflow (below 2^-126).  N(0, 1) scores never raise a second time."""
    c, inp, _, r = _setup("climb-200x449", "fast")
    n = R.raises64(r["t"], r["ok"])
    planted = R.climb_rows(c["Tq"])
    assert int(n[:, :, planted].min()) == 8 and int(n[:, :, planted].max()) == 8
    once = (n == 1)
    for q0 in range(0, c["Tq"], 32):
        assert bool(once[:, :, q0:q0 + 32].any(-1).all()) and bool(planted[q0:q0 + 32].any())
    c, inp, _, r = _setup("descend-64x449", "fast")
    n = R.raises64(r["t"], r["ok"])
    planted = R.climb_rows(c["Tq"])
    assert int(n[:, :, planted].max()) == 1
    t = r["t"][:, :, planted]
    assert float((t[..., 448:].amax(-1) - t.amax(-1)).max()) < -126.0
    for name in ("geo-129x192", "geo-200x257", "geo-64x449"):
        c, inp, _, r = _setup(name, "fast")
        assert int(R.raises64(r["t"], r["ok"]).max()) == 1


def test_one_hot_and_shift_scores():
    c, inp, _, r = _setup("onehot-129x192", "fast")
    for b, jh in enumerate(R.one_hot_keys(c)):
        row = r["t"][b].clone()
        lead = row[..., jh].clone()
        row[..., jh] = R.NINF
        row = torch.where(r["ok"][b], row, torch.full_like(row, R.NINF))
        assert float((lead - row.amax(-1)).min()) > 40.0 and bool(r["ok"][b, :, :, jh].all())
    assert R.one_hot_keys(c) == (63, 64, 149)
    c, inp, _, r = _setup("shift-128x65", "fast")
    assert float(r["t"][0].min()) > 60.0 and float(r["t"][1].max()) < -60.0
    assert float(r["lse"][0].min()) > 60.0 * R.LN2 and float(r["lse"][1].max()) < -60.0 * R.LN2


def test_masks_reach_what_they_are_meant_to():
    assert R.leading_masked_tiles(R.case_mask(R.CASES["prefix-129x192"])).tolist() == [0, 1, 2]
    assert R.leading_masked_tiles(R.case_mask(R.CASES["prefix-64x449"])).tolist() == [0, 3, 6]
    m = R.case_mask(R.CASES["scattered-200x257"])
    assert bool(m[:, 128:192].all()) and m[0, 64:128].nonzero().flatten().tolist() == [0, 31, 32, 63] and not bool(m[:, :64].any())
    assert R.case_mask(R.CASES["suffix-129x192"]).logical_not().sum(1).tolist() == [1, 64, 65]
    for name in ("allmasked-129x192", "allmasked-129x192-kvlen"):
        c, inp, _, r = _setup(name, "fast")
        assert bool(r["dead"][1].all()) and not bool(r["dead"][0].any()) and not bool(r["dead"][2].any())
    for name, rows in (("causal-100x40-bf16-D64", 60), ("causal-100x40-f32-D32", 60), ("causal-40x100-f32-D64", 0)):
        c, inp, _, r = _setup(name, "generic")
        assert r["dead"][0, 0].sum().item() == rows and bool(r["dead"][..., :rows].all())
    z = R.dozero_rows(200)
    assert bool(z[:128].all()) and not bool(z[128:192].any()) and bool(z[192:].all())


def test_case_table():
    big = max(c["Bn"] * c["H"] * c["Tq"] * c["Tk"] for c in R.CASES.values())
    assert big == 3 * 3 * 200 * 449
    for c in R.CASES.values():
        inp = R.inputs(c)
        for n in ("q", "k", "v", "do"):
            assert inp[n].dtype == c["dt"] and torch.equal(inp[n].to(R.B).to(c["dt"]), inp[n]), "%s: %s is not bf16-exact" % (c["name"], n)
        again = R.inputs(c)
        assert all(torch.equal(inp[n], again[n]) for n in ("q", "k", "v", "do"))
    assert {r for _, r in R.RUNS} == {"fast", "generic"}


def test_restated_reference_against_plain_softmax():
    """N(0, 1): the fast route's reference scores with q^ = bf16(fl32(q c2)) instead of q c2: |delta t_j| <= (2^-8 + 2^-24) sum_d |q_d c2 k_d|,
    and a softmax whose scores move by at most e (natural units) moves each weight by a factor within exp(+-2 e): |delta o| <= expm1(2 e)
    sum_j w_j |v_j| with w the restated weights."""
    c, inp, _, r = _setup("geo-129x192", "fast")
    plain = R.plain64(c, inp)
    Q, K, V = (R._heads(inp[n], c).double() for n in ("q", "k", "v"))
    c2 = float(R._c2(inp["scale"]))
    e = (R.UB + 2 * R.U32) * torch.einsum("bhqd,bhjd->bhqj", Q.abs(), K.abs()).amax(-1, keepdim=True) * c2 * R.LN2
    e = e + abs(c2 * R.LN2 - inp["scale"]) * torch.einsum("bhqd,bhjd->bhqj", Q, K).abs().amax(-1, keepdim=True)
    w = torch.softmax(r["t"] * R.LN2, -1)
    allow = R._flat(torch.expm1(2 * e) * torch.einsum("bhqj,bhjd->bhqd", w, V.abs()))
    err = (plain - r["o"]).abs()
    print("restated vs plain: worst |delta o| %.3g, worst ratio to the allowance %.3f" % (float(err.max()), float((err / allow).max())))
    assert bool((err <= allow).all()) and float(err.max()) > 0.0
