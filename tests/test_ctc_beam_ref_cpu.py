"""The fp64 restatement of CTC prefix beam search (ctc_beam_ref.py) against brute-force enumeration, its defect variants, check_step,
the gap condition of every committed exact case, and the host route of the package against the restatement.  No GPU."""
import math
from importlib import import_module

import numpy as np
import pytest
import torch

import ctc_beam_ref as R
from conftest import load_pkg

SEEDS = range(5)
HUGE = 10 ** 6


def unpruned(seed, defect=None):
    x = R.make_logits(6, 4, seed)
    lp, dl = R.row_terms(x.double().numpy())
    return lp, R.prefix_beam_search(lp, 0, HUGE, 3, math.inf, defect=defect, dl=dl)


def differs(hyps, br):
    h = {}
    for lab, s in hyps:
        h.setdefault(lab, []).append(s)
    return set(h) != set(br) or any(len(v) != 1 or abs(v[0] - br[k]) > 1e-9 for k, v in h.items())


@pytest.mark.parametrize("seed", SEEDS)
def test_unpruned_restatement_equals_brute_force(seed):
    lp, r = unpruned(seed)
    br = R.brute(lp, 0)
    assert len(br) == 358
    assert not differs(r["hyps"], br)


# threshold_before_merge acts only under a finite threshold and stay_from_list_only only where the list leaves classes out: with
# unpruned settings they ARE the restatement, so they are compared under the pruning that triggers them, against the restatement.
UNPRUNED_DEFECTS = [d for d in R.DEFECTS if d not in ("threshold_before_merge", "stay_from_list_only")]
PRUNED = {"threshold_before_merge": dict(K=HUGE, N=3, theta=3.0), "stay_from_list_only": dict(K=HUGE, N=1, theta=math.inf)}


@pytest.mark.parametrize("defect", UNPRUNED_DEFECTS)
def test_defects_fail_brute_force(defect):
    bad = 0
    for seed in SEEDS:
        lp, r = unpruned(seed, defect)
        bad += differs(r["hyps"], R.brute(lp, 0))
    assert bad >= 1


@pytest.mark.parametrize("defect", sorted(PRUNED))
def test_pruning_defects_differ_from_restatement(defect):
    bad = 0
    for seed in SEEDS:
        lp, _ = R.row_terms(R.make_logits(6, 4, seed).double().numpy())
        good = R.prefix_beam_search(lp, 0, **PRUNED[defect])
        bad += differs(R.prefix_beam_search(lp, 0, defect=defect, **PRUNED[defect])["hyps"], dict(good["hyps"]))
    assert bad >= 1


def steps_of(lp, dl, K, N, theta, defect):
    """[(prev beam, frame, next beam)] along the GOOD trajectory, the next beam computed with `defect`."""
    trie, beam, out = R.Trie(), [(0, 0.0, R.NINF)], []
    for t in range(lp.shape[0]):
        prev = [(trie.prefix(i), pb, pnb) for i, pb, pnb in beam]
        cands, cut, _, _ = R.step(trie, beam, lp[t], 0, K, N, theta, defect)
        nxt = [(trie.prefix(i), pb, pnb) for i, pb, pnb in R.select(cands, cut, K)[0]]
        out.append((prev, dict(lp=lp[t], dl=dl[t], blank=0, K=K, N=N, theta=theta), nxt))
        cands, cut, _, _ = R.step(trie, beam, lp[t], 0, K, N, theta)
        beam = R.select(cands, cut, K)[0]
    return out


@pytest.mark.parametrize("defect", [None] + list(R.DEFECTS))
def test_check_step_accepts_own_steps_and_rejects_defects(defect):
    cfg = PRUNED.get(defect, dict(K=HUGE, N=3, theta=math.inf))
    cfg = dict(cfg, K=12)
    rejected = 0
    for seed in SEEDS:
        x = R.make_logits(8, 4, seed)
        lp, dl = R.row_terms(x.double().numpy())
        for prev, frame, nxt in steps_of(lp, dl, cfg["K"], cfg["N"], cfg["theta"], defect):
            ok, why, _ = R.check_step(prev, frame, nxt)
            if defect is None:
                assert ok, why
            rejected += not ok
    assert (rejected == 0) if defect is None else rejected >= 1


def test_check_step_rejects_a_score_outside_the_bound_and_an_illegal_selection():
    x = R.make_logits(5, 6, 0)
    lp, dl = R.row_terms(x.double().numpy())
    prev, frame, nxt = steps_of(lp, dl, 4, 5, math.inf, None)[3]
    ok, _, bound = R.check_step(prev, frame, nxt)
    assert ok
    off = [(nxt[0][0], nxt[0][1], nxt[0][2] + 3 * bound)] + nxt[1:]
    assert nxt[0][2] > R.NINF
    assert not R.check_step(prev, frame, off)[0]
    assert not R.check_step(prev, frame, nxt[1:] + [(nxt[0][0] + (1, 2, 3), R.NINF, -50.0)])[0]  # no candidate
    assert not R.check_step(prev, frame, nxt[1:])[0]                                              # the best one left out
    assert not R.check_step(prev, frame, nxt[::-1])[0]                                            # out of order


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", sorted(R.EXACT_CASES))
def test_exact_cases_keep_their_decisions_clear_of_the_bound(name, dtype):
    """The condition the GPU test's exact comparison rests on: the smallest decision gap is at least 4 x the counted bound on a score."""
    _, _, _, _, res = R.exact_case(name, dtype)
    for r in res:
        print(name, "gap %.3g bound %.3g" % (r["gap"], r["bound"]))
        assert r["gap"] >= 4 * r["bound"]


@pytest.mark.parametrize("name", ["merges", "threshold3", "short_list", "lengths"])
def test_host_route_equals_restatement(name):
    load_pkg()
    D = import_module("chimera-st_amd.ctc_decoder")
    x, in_len, blank, c, res = R.exact_case(name, torch.float32)
    got = D.prefix_beam_search_host(x, in_len, blank, c["K"], c["N"], c.get("theta", math.inf), c["K"])
    for b, r in enumerate(res):
        assert [tuple(h[0]) for h in got[b]] == [h[0] for h in r["hyps"]]
        assert np.allclose([h[1] for h in got[b]], [h[1] for h in r["hyps"]], rtol=0, atol=1e-9)
