"""w2v_pretrain_ref.py on the CPU: the fp64 restatement of the InfoNCE kernels equals torch's own composition (cosine_similarity,
cross_entropy, autograd) in fp64; its bounds hold for a faithful fp32 evaluation and reject each listed defect; the sampler's numpy twin
keeps the reference's promises (never the position itself among the own-utterance draws, in range, the reference's shift at Kx > 0).
The same for the Gumbel quantizer's restatement (against F.gumbel_softmax(hard=True) spelt out on a given noise), with the count of
undecided hard choices asserted zero at the seeds the GPU test uses."""
from importlib import import_module

import numpy as np
import pytest
import torch

import w2v_pretrain_ref as R
from conftest import load_pkg

SMALL = ["tiny", "wide", "cross", "planted", "duplicates"]


@pytest.fixture(scope="module")
def rng():
    load_pkg()
    return import_module("chimera-st_amd.rng")


@pytest.mark.parametrize("name", SMALL)
def test_restatement_equals_torch_composition_fp64(name):
    (x, y, idx, inv_temp, _, _), ref = R.reference(name, torch.float32)
    t = R.torch_composition(x, y, idx, 1.0 / inv_temp, gscale=1.0)
    fin = torch.isfinite(t["logits"])
    assert torch.equal(fin, torch.isfinite(ref["logits"])), "the -inf masks differ"
    assert float((t["logits"][fin] - ref["logits"][fin]).abs().max()) < 1e-12
    assert abs(float(t["loss"]) - float(ref["loss"])) < 1e-10 * max(1.0, abs(float(ref["loss"])))
    for k in ("dx", "dy"):
        scale = float(ref[k].abs().max())
        assert float((t[k] - ref[k]).abs().max()) <= 1e-11 * scale, k
    assert (t["correct"], t["count"]) == (ref["correct"], ref["count"])


def test_planted_case_is_what_it_claims():
    (x, y, idx, inv_temp, _, _), ref = R.reference("planted", torch.float32)
    assert bool(ref["masked"][2, 1:].all()) and float(ref["nll"][2]) == 0.0 and float(ref["bounds"]["nll"][2]) == 0.0
    assert int(ref["dx"][2].ne(0).sum()) == 0
    assert bool(ref["masked"][0, 1]) and bool(ref["masked"][0, 2])
    assert float(x[7].abs().max()) == 0.0 and float(y[8].abs().max()) == 0.0 and int(idx[9, 0]) == 8
    assert bool(torch.isfinite(ref["dx"]).all()) and bool(torch.isfinite(ref["dy"]).all())
    (_, _, idx_d, _, (B, M, K, Kx), _), _ = R.reference("duplicates", torch.float32)
    assert K > M - 1 and all(len(set(r.tolist())) < K for r in idx_d)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", SMALL)
def test_bounds_hold_for_fp32_evaluation(name, dtype):
    (x, y, idx, inv_temp, _, _), ref = R.reference(name, dtype)
    got = R.infonce_eval(x, y, idx, inv_temp, dt=torch.float32)
    if dtype == torch.bfloat16:
        got["dx"], got["dy"] = got["dx"].bfloat16(), got["dy"].bfloat16()
    ratios, bad = R.judge(ref, got)
    print("RATIO infonce fp32-eval %-10s %s" % (name, {k: "%.3f" % v for k, v in ratios.items()}))
    assert bad == 0
    assert (got["correct"], got["count"]) == (ref["correct"], ref["count"])


CASE_OF_DEFECT = {"no_eps_clamp": "planted", "no_mask": "planted", "duplicate_once": "duplicates", "no_temp_in_backward": "cross"}


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_bounds_reject_defect(defect):
    assert set(CASE_OF_DEFECT) == set(R.DEFECTS)
    (x, y, idx, inv_temp, _, _), ref = R.reference(CASE_OF_DEFECT[defect], torch.float32)
    got = R.infonce_eval(x, y, idx, inv_temp, dt=torch.float32, defect=defect)
    _, bad = R.judge(ref, got)
    assert bad > 0


@pytest.mark.parametrize("shape", [(1, 2, 1, 0), (3, 37, 100, 0), (2, 16, 4, 3), (4, 5, 0, 6), (2, 300, 100, 0)])
def test_negatives_numpy(rng, shape):
    B, M, K, Kx = shape
    idx = rng.negatives_numpy(0xC0FFEE11, B, M, K, Kx)
    assert idx.dtype == np.int32 and idx.shape == (B, M, K + Kx)
    pos = (np.arange(B)[:, None] * M + np.arange(M)[None, :])[:, :, None]
    own, cross = idx[:, :, :K], idx[:, :, K:]
    assert not (own == pos).any(), "a position drew itself"
    assert (own >= np.arange(B)[:, None, None] * M).all() and (own < (np.arange(B)[:, None, None] + 1) * M).all(), "outside the utterance"
    assert (cross >= 0).all() and (cross < B * M).all()
    # the reference's shift (wav2vec2.py:488-493): the flat value equal to the TIME index m is never produced
    assert not (cross == np.arange(M)[None, :, None]).any()
    assert np.array_equal(idx, rng.negatives_numpy(0xC0FFEE11, B, M, K, Kx))
    assert not np.array_equal(idx, rng.negatives_numpy(0xC0FFEE12, B, M, K, Kx)) or idx.size < 3


def test_negatives_numpy_is_uniform(rng):
    """every other position of the utterance is drawn about equally often (the one-wave-per-row backward relies on it)"""
    B, M, K = 2, 50, 2000
    idx = rng.negatives_numpy(7, B, M, K, 0)
    counts = np.bincount(idx.reshape(-1), minlength=B * M)
    expect = M * K / M  # each row is drawn by M - 1 positions, K / (M - 1) times each
    assert abs(counts / expect - 1.0).max() < 0.1


def test_hash_bits_numpy_is_the_dropout_hash(rng):
    """keep_mask_numpy reads 16-bit halves of the same words"""
    key, n, p = 0xABCD1234, 4096, 0.25
    bits = rng.hash_bits_numpy(key, np.arange(n // 2, dtype=np.uint64))
    halves = np.stack([bits & np.uint64(0xFFFF), bits >> np.uint64(16)], 1).reshape(-1)
    assert np.array_equal(halves >= np.uint64(int(p * 65536.0 + 0.5)), rng.keep_mask_numpy(key, n, p))


# ---- Gumbel vector quantizer ----
VQ_SMALL = ["tiny", "two_groups", "unused"]


@pytest.mark.parametrize("name", VQ_SMALL + ["one_group"])
def test_vq_restatement_equals_torch_composition_fp64(name):
    c, noise, ref = R.vq_reference(name, torch.float32, injected=True)
    t = R.vq_torch_composition(c, noise)
    assert torch.equal(t["idx"], ref["idx"])
    assert float((t["q"] - ref["q"]).abs().max()) < 1e-12
    for k in ("prob_perplexity", "code_perplexity"):
        assert abs(float(t[k]) - float(ref[k])) < 1e-6 * float(ref[k]), k  # (1e-7 against its fp32 value inside the logarithm)
    for k in ("dl", "dvars"):
        assert float((t[k] - ref[k]).abs().max()) <= 1e-6 * float(ref[k].abs().max()) + 1e-12, k


@pytest.mark.parametrize("injected", [False, True], ids=["own_noise", "injected"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", sorted(R.VQ_CASES))
def test_vq_no_choice_is_undecided(name, dtype, injected):
    """Every hard choice's fp64 top-2 margin exceeds the bound of (l + g) at these seeds: a wrong argmax cannot hide behind the cap."""
    _, _, ref = R.vq_reference(name, dtype, injected)
    assert ref["undecided"] == 0
    if name == "unused":
        V = R.VQ_CASES[name][2]
        assert int(ref["idx"].max()) < V // 2 and float(ref["avg_probs"][:, V // 2:].max()) < 1e-12


@pytest.mark.parametrize("injected", [False, True], ids=["own_noise", "injected"])
@pytest.mark.parametrize("name", VQ_SMALL)
def test_vq_bounds_hold_for_fp32_evaluation(name, injected):
    c, noise, ref = R.vq_reference(name, torch.float32, injected)
    got = R.vq_eval(c, noise=noise, dt=torch.float32)
    ratios, bad = R.judge(ref, got, keys=("dl", "avg_probs", "exph", "prob_perplexity", "code_perplexity", "dvars", "gy"))
    print("RATIO vq fp32-eval %-10s %s" % (name, {k: "%.3f" % v for k, v in ratios.items()}))
    assert bad == 0 and torch.equal(got["idx"], ref["idx"]) and torch.equal(got["q"].double(), ref["q"])


@pytest.mark.parametrize("defect", R.VQ_DEFECTS)
def test_vq_bounds_reject_defect(defect):
    c, noise, ref = R.vq_reference("unused", torch.float32, True)
    got = R.vq_eval(c, noise=noise, dt=torch.float32, defect=defect)
    _, bad = R.judge(ref, got, keys=("dl", "prob_perplexity", "code_perplexity"))
    assert bad > 0


def test_gumbel_uniform_numpy(rng):
    u = rng.gumbel_uniform_numpy(0x1234ABCD, 1 << 16)
    assert u.dtype == np.float32 and float(u.min()) >= 2.0 ** -24 and float(u.max()) <= 1.0 - 2.0 ** -24
    k = (rng.hash_bits_numpy(0x1234ABCD, np.arange(1 << 16, dtype=np.uint64)) >> np.uint64(9)).astype(np.float64)
    assert np.array_equal(u.astype(np.float64), (k + 0.5) * 2.0 ** -23), "u is not exact in fp32"
    assert abs(float(u.mean()) - 0.5) < 0.01


# ---- the real reference's fixture ----
@pytest.mark.parametrize("case", ["train", "eval", "cross"])
def test_oracle_composition_reproduces_the_reference_fixture(case):
    """tests/golden/w2v_pretrain_tiny.npz (the real reference, tools/ref_harness/make_w2v_pretrain_goldens.py) against the pre-training
    head restated on the oracle's wav2vec2 trunk, in fp32 on the CPU, with the recorded mask, negative indices and noise replayed:
    logits, loss terms, counts and (train) every parameter gradient within the project's 1e-3."""
    import w2v_pretrain_util as PU
    from conftest import load_golden
    from parity_util import max_abs_rel
    g = load_golden("w2v_pretrain_tiny.npz")
    p, a = PU.params()
    r = PU.pretrain_oracle(p, a, torch.from_numpy(g["in/source"]), g[case + "/mask"], g[case + "/neg_idx"], g.get(case + "/noise"),
                           training=case != "eval")
    ref = torch.from_numpy(g[case + "/logits"])
    inf = torch.isinf(ref)
    assert bool(inf.any()) and torch.equal(torch.isinf(r["logits"]), inf)
    assert max_abs_rel(r["logits"][~inf], ref[~inf]) < 1e-3
    for k in ("loss", "loss_0", "loss_1", "loss_2", "prob_perplexity", "code_perplexity", "features_pen"):
        assert abs(float(r[k]) - float(g[case + "/" + k])) <= 1e-3 * max(1.0, abs(float(g[case + "/" + k]))), k
    assert (r["correct"], r["count"]) == (int(g[case + "/correct"]), int(g[case + "/count"]))
    M = ref.shape[1]
    assert M >= 4 and int(g[case + "/sample_size"]) == ref.shape[0] * M
    if case == "train":
        r["loss"].backward()
        for k, v in p.items():
            got = v.grad if v.grad is not None else torch.zeros_like(v)
            assert max_abs_rel(got, torch.from_numpy(g["grad/" + k])) < 1e-3, k
