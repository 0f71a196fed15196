"""No-GPU checks of gemm_ref.py: every case's row reaches the route it records, the cases cover every launch arm of gemm_route, the
persistent launcher's arithmetic gives the scheduling state the case table claims, the two input conditions of the exact cases hold,
an fp32 evaluation in two summation shapes equals the fp64 reference bit for bit (exact) or stays inside the counted bounds
(bounded), and every listed defect leaves its case.  Run with -s for the routes, shares, ratios and per-defect counts."""
import ctypes
import os

import pytest
import torch

import gemm_ref as G
from conftest import load_pkg
from test_gemm_route_cpu import make_desc, parse, route_of


R128, R256, RN = G.R128, G.R256, G.RN
# every launch arm gemm_route can return without the experiment hook (csrc/gemm.hip: gemm_route / launch_route), counted:
#   reg   128x128: the three layouts with an mn-major operand + the SEG instantiation for k/k (k/k without segments goes to the DMA
#         ring)                                                                                                                4
#         256x256: the same three layouts (bf16 k/m is taken by 8p where it is supported; f32 reaches it)                        3
#         64x128 (NarrowM): m/m                                                                                                  1
#   glds  k/k only: 64x64 ns4, 64x64 ns2, 128x128 ns2, 128x64 ns2 (NarrowN), 256x256 ns2                                         5
#   8p    k/k, k/m (A k-major only)                                                                                              2
#   4w                                                                                                                           1
ARMS = ({"reg %s %s" % (lay, R128) for lay in ("mm", "km", "mk")} | {"reg kk seg " + R128} | {"reg %s %s" % (lay, R256) for lay in ("mm", "km", "mk")}
        | {"reg mm " + RN} | {"glds kk 64x64 nt256 ns4", "glds kk 64x64 nt256 ns2", "glds kk %s ns2" % R128, "glds kk 128x64 nt256 ns2",
                              "glds kk %s ns2" % R256} | {"8p kk", "8p km", "4w"})
assert len(ARMS) == 16


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    L = load_pkg().lib
    if not os.path.exists(L.LIB_PATH):
        ge.build()
    return L, L.load()


def test_every_case_reaches_its_route_and_the_cases_cover_every_arm(built):
    reached = {}
    for c in G.CASES:
        got = route_of(*built, c["row"])
        print("ROUTE %-24s %-78s %s" % (c["name"], c["row"], got))
        assert got == c["route"], "case %s no longer reaches its arm: %r routes to %r, not %r" % (c["name"], c["row"], got, c["route"])
        reached.setdefault(G.arm_of(got), []).append(c["name"])
    assert set(reached) == ARMS, (sorted(ARMS - set(reached)), sorted(set(reached) - ARMS))
    # every arm by an exact case, not only by a bounded one
    exact = {G.arm_of(c["route"]) for c in G.CASES if c["kind"] == "exact"}
    assert exact == ARMS, sorted(ARMS - exact)
    print("ARMS %d: %s" % (len(reached), sorted(reached)))


def test_the_recorded_split_counts_and_fused_column_sums_are_the_dispatchers(built):
    L, lib = built
    for c in G.CASES:
        d = make_desc(L, c["row"])
        o_splits = int(c["route"].rsplit("split", 1)[1]) if "split" in c["route"] else max(parse(c["row"])[5].get("split", -1), 1)
        assert lib.cst_gemm_splits(ctypes.byref(d)) == o_splits, c["name"]
        if "colsum" in parse(c["row"])[4]:
            assert lib.cst_gemm_colsum_is_fused(ctypes.byref(d)) == int(" colsum" in c["route"]), c["name"]


def test_the_persistent_launchers_arithmetic_gives_the_claimed_state():
    """launch8p's rules on 256 CUs: tiles, avail, half_from, nitems, claims, gperm_full, mrot; and the epilogue mode."""
    n = 0
    for c in G.CASES:
        if not c["route"].startswith("8p"):
            continue
        M, N, K, lay, flags, kv = parse(c["row"])
        nb = kv.get("b0", 1) * kv.get("b1", 1)
        st = G.launch8p_state(M, N, nb, max(kv.get("split", 1), 1), "m_len" in flags)
        for k, v in c.get("state", {}).items():
            assert st[k] == v, (c["name"], k, st)
        if st["tiles"] <= 256:
            assert st["half_from"] is None and not st["claims"] and st["nitems"] == st["tiles"], c["name"]   # one round, static
        assert G.mode8p(G.operands(c["name"])) == c["mode"], c["name"]
        n += 1
    assert n >= 30
    # the reserved-CU states of the grouped GPU test, for 256 CUs
    s = G.launch8p_state(3592, 3608, 1, 1, False, reserved=216)
    assert (s["avail"], s["tiles"], s["half_from"], s["claims"]) == (40, 225, None, True)            # remainder 25 > 20: no halves
    s = G.launch8p_state(3592, 3608, 1, 1, False, reserved=248)
    assert (s["avail"], s["half_from"], s["nitems"], s["claims"]) == (8, 224, 226, True)             # remainder 1: one tile as two halves
    s = G.launch8p_state(3592, 3608, 1, 1, False, reserved=248, no_halves=True)
    assert (s["half_from"], s["nitems"], s["claims"]) == (None, 225, True)
    # the item -> tile walk visits every tile once, the tail tiles as two halves
    for M, N, reserved in ((3592, 3608, 0), (3592, 3608, 248), (4300, 4096, 0), (4300, 4100, 0)):
        tm, tn = -(-M // 256), -(-N // 256)
        st = G.launch8p_state(M, N, 1, 1, False, reserved=reserved)
        seen = sorted(G.tile_of_item8p(v, st, tm, tn) for v in range(st["nitems"]))
        nh = 0 if st["half_from"] is None else st["tiles"] - st["half_from"]
        assert len(set(seen)) == st["nitems"] and {(a, b) for a, b, _ in seen} == {(a, b) for a in range(tm) for b in range(tn)}
        assert sum(h >= 0 for _, _, h in seen) == 2 * nh and sum(h == 1 for _, _, h in seen) == nh


@pytest.mark.parametrize("name", [c["name"] for c in G.CASES])
def test_conditions_and_fp32_evaluations(name):
    """exact: headroom below 2^24, at most 2 % of the bf16 outputs at 256 or above, and fp32 arithmetic in two shapes gives the reference's
    bits; bounded: the same two shapes stay inside the counted bounds."""
    o = G.operands(name)
    ex = G.expected(name)
    rows = G.sample_rows(o["M"])
    if o["kind"] == "exact":
        assert G.headroom(o) < 2 ** 24, G.headroom(o)
        assert float(o["b"].abs().min()) >= 1 and float(o["a"][o["a"] != 0].abs().min()) >= 1   # integers; zero only where declared dead
        sh = G.share_ge_256(ex, o)
        print("SHARE %-24s %s" % (name, " ".join("%s %.4f%%" % (k, 100 * v) for k, v in sh.items()) or "(fp32 outputs)"))
        assert all(v <= 0.02 for v in sh.values()), sh
        want = {"C": G.c_stack(o, ex["C"])[:, rows]}
        if "aux_out" in ex:
            want["aux_out"] = G.c_stack(o, ex["aux_out"])[:, rows]
        if "colsum" in ex:
            want["colsum"] = ex["colsum"]
        for shape in G.SHAPES:
            got = G.emulate32(name, shape, rows)
            for k, w in want.items():
                assert torch.equal(got[k], w), (name, shape, k, int((got[k] != w).sum()))
    else:
        bd = G.bounds(name, ex)
        for shape in G.SHAPES:
            got = G.emulate32(name, shape, rows)
            for k, b in bd.items():
                sel = (lambda t: t) if k == "colsum" else (lambda t: t[:, rows])
                r, bad = G.worst_ratio(got[k], sel(ex["v64"][k]), sel(b))
                print("RATIO %s %s %s worst err/bound %.4f" % (name, k, shape, r))
                assert bad == 0 and r <= 1.0, (name, shape, k, r, bad)


@pytest.mark.parametrize("defect", sorted(G.DEFECTS))
def test_every_defect_leaves_its_case(defect):
    """An index-level mistake changes bits of its (exact) case, in at least 1 element of 10 000."""
    name = G.DEFECTS[defect]
    assert G.BY_NAME[name]["kind"] == "exact"
    good, bad = G.expected(name), G.expected(name, defect)
    moved, total = 0, 0
    for k in ("C", "aux_out", "colsum"):
        if k in good:
            g, b = good[k].double(), bad[k].double()
            moved += int((~((g == b) | (torch.isnan(g) & torch.isnan(b)))).sum())
            total += g.numel()
    print("DEFECT %-36s in %-22s moves %d of %d elements" % (defect, name, moved, total))
    assert moved >= 1 and moved * 10000 >= total, (defect, moved, total)
