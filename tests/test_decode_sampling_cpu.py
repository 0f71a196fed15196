"""No-GPU checks of sampling decode (--sampling / --sampling-topk / --sampling-topp / --nbest): the fp64 restatement of
tests/decode_sampling_util.py against the kept sets the REAL reference's Sampling._sample_topp / topk produced
(tests/golden/decode_sampling_tiny.npz), the numpy twin of the draws' uniforms, the share of undecidable draws on the kernel test's own
inputs, the host loop's Sampling strategy against the restatement, and the command line's argument checks."""
from argparse import Namespace
from importlib import import_module

import numpy as np
import pytest
import torch

import decode_sampling_util as U
from conftest import load_golden, load_pkg

TOPP, TOPK = (0.3, 0.9, 0.999), (1, 8)


def SGM():
    load_pkg()
    return import_module("chimera-st_amd.sequence_generator")


# ---- the kept sets of the reference -------------------------------------------------------------------------------------------------
def test_restatement_kept_sets_equal_the_reference():
    """Sets exact, trimmed probabilities to 1e-6, for every recorded row at every p and k of the fixture."""
    g = load_golden("decode_sampling_tiny.npz")
    rows = g["rows"].astype(np.float64)
    assert rows.shape[0] >= 24
    sizes = []
    for p in TOPP:
        idx, probs = g["topp/p%g/indices" % p], g["topp/p%g/probs" % p]
        for r in range(rows.shape[0]):
            kept, order, _ = U.kept_set(rows[r], topp=p)
            n = int((probs[r] > 0).sum())
            assert sorted(idx[r, :n].tolist()) == np.nonzero(kept)[0].tolist(), (p, r)
            assert idx[r, :n].tolist() == order[:n].tolist(), (p, r)  # ... and in the same (descending) order
            assert np.abs(np.exp(rows[r][order[:n]]) - probs[r, :n]).max() <= 1e-6, (p, r)
            assert not probs[r, n:].any()
            sizes.append(n)
    assert min(sizes) == 1 and max(sizes) == rows.shape[1]  # from a single token to the whole vocabulary
    for k in TOPK:
        idx = g["topk/k%d/indices" % k]
        for r in range(rows.shape[0]):
            assert sorted(idx[r].tolist()) == np.nonzero(U.kept_set(rows[r], topk=k)[0])[0].tolist(), (k, r)


def test_host_strategy_kept_sets_equal_the_reference():
    """sequence_generator.Sampling.kept (the host loop's form, torch) on the same rows."""
    g = load_golden("decode_sampling_tiny.npz")
    rows = torch.from_numpy(g["rows"])

    class D:
        pad = staticmethod(lambda: 1)
        unk = staticmethod(lambda: 3)
        eos = staticmethod(lambda: 2)

        def __len__(self):
            return rows.shape[1]

    S = SGM().Sampling
    for p in TOPP:
        probs = g["topp/p%g/probs" % p]
        kept = S(D(), sampling_topp=p).kept(rows)
        for r in range(rows.shape[0]):
            n = int((probs[r] > 0).sum())
            assert sorted(g["topp/p%g/indices" % p][r, :n].tolist()) == kept[r].nonzero().flatten().tolist(), (p, r)
    for k in TOPK:
        kept = S(D(), sampling_topk=k).kept(rows)
        for r in range(rows.shape[0]):
            assert sorted(g["topk/k%d/indices" % k][r].tolist()) == kept[r].nonzero().flatten().tolist(), (k, r)


# ---- the uniforms -------------------------------------------------------------------------------------------------------------------
def test_uniform_twin():
    n = 100000
    idx = np.arange(n)
    u1, u2 = U.uniforms(0x1234ABCD, idx), U.uniforms(0x1234ABCE, idx)
    for u in (u1, u2):
        assert u.min() >= 0.0 and u.max() < 1.0
        assert abs(u.mean() - 0.5) <= 4.0 * (1.0 / 12.0) ** 0.5 / n ** 0.5
    assert (u1 != u2).mean() > 0.99
    assert np.array_equal(u1 * 2.0 ** 24, np.floor(u1 * 2.0 ** 24))  # 24-bit fractions: exact in fp32
    # the package's twin (the host loop's draws) is the same function
    assert np.array_equal(SGM().sample_uniforms(0x1234ABCD, idx), u1)
    rng = import_module("chimera-st_amd.rng")
    key = 0x1234ABCD
    assert np.array_equal(rng._bits32(key, (key * 0x2C1B3C6D + 0x297A2D39) & 0xFFFFFFFF, idx.astype(np.uint64)) >> np.uint64(8),
                          (u1 * 2.0 ** 24).astype(np.uint64))


def test_sample_keys_differ_by_seed_and_call():
    M = SGM()
    keys = {M.sample_key_of(seed, call) for seed in (1, 2, 1 << 40) for call in (1, 2, 3)}
    assert len(keys) == 9 and all(0 <= k < 1 << 32 for k in keys)


# ---- the kernel test's inputs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(U.VARIANTS))
def test_undecidable_share_of_the_kernel_test_inputs(variant):
    """The restatement alone, on every case of the kernel test: at most 1 % of the draws are undecidable (else the kernel test could
    forgive its way through), and every sentence ends with `beam` samples."""
    n = bad = 0
    for dtype_name, V, members in U.CASES:
        st, nn, bb = U.run_restatement(dtype_name, V, members, variant)
        n, bad = n + nn, bad + bb
        assert st["finished"].tolist() == [1] * U.BSZ and st["nfinal"].tolist() == [U.BEAM] * U.BSZ
    print("%s: %d draws, %d undecidable (%.3f %%)" % (variant, n, bad, 100.0 * bad / n))
    assert bad <= 0.01 * n


def test_host_strategy_draws_what_the_restatement_draws():
    """sequence_generator.Sampling.step on restated rows: same tokens and scores wherever the draw is decidable."""
    M = SGM()

    class D:
        pad = staticmethod(lambda: U.PAD)
        unk = staticmethod(lambda: U.UNK)
        eos = staticmethod(lambda: U.EOS)

        def __len__(self):
            return 60

    for topk, topp in ((0, 0.0), (8, 0.0), (0, 0.9)):
        st = U.new_state()
        st["scores"][:, 2] = -torch.arange(U.BSZ * U.BEAM, dtype=torch.float64)
        strat = M.Sampling(D(), sampling_topk=topk or -1, sampling_topp=topp or -1.0)
        for s in (0, 3):
            lp = U.masked_lprobs(st, U.step_logits("fp32", 60, 1, s), s)
            want = U.step_draws(st, lp, s, 77, topk, topp)
            sc, tok, beams = strat.step(s, lp.float().view(U.BSZ, U.BEAM, 60), st["scores"].float().view(U.BSZ, U.BEAM, -1)[:, :, :s],
                                        key=77, max_len=U.MAX_LEN)
            assert beams.tolist() == [[0] * U.BEAM if s == 0 else list(range(U.BEAM))] * U.BSZ
            for i, d in enumerate(want):
                if d["decidable"]:
                    assert int(tok.view(-1)[i]) == d["tok"], (topk, topp, s, i)
                    assert abs(float(sc.view(-1)[i]) - d["score"]) < 1e-5


# ---- the command line ------------------------------------------------------------------------------------------------------------
def test_parser_defaults_and_refused_combinations():
    load_pkg()
    cli = import_module("chimera-st_amd.cli")
    base = ["data", "--path", "m.pt"]
    a = cli.check_generate_args(cli.generate_parser().parse_args(base))
    assert (a.sampling, a.sampling_topk, a.sampling_topp, a.nbest, a.seed) == (False, -1, -1.0, 1, 1)
    ok = cli.check_generate_args(cli.generate_parser().parse_args(base + ["--sampling", "--sampling-topp", "0.9", "--beam", "3", "--nbest", "3"]))
    assert ok.sampling and ok.sampling_topp == 0.9 and ok.nbest == 3
    parse = lambda extra: cli.check_generate_args(cli.generate_parser().parse_args(base + extra))
    with pytest.raises(ValueError, match="--sampling-topk requires --sampling"):
        parse(["--sampling-topk", "5"])
    with pytest.raises(ValueError, match="--sampling-topp requires --sampling"):
        parse(["--sampling-topp", "0.9"])
    with pytest.raises(ValueError, match="--nbest 6 must be between 1 and --beam 5"):
        parse(["--nbest", "6"])


def test_build_generator_honours_the_sampling_flags():
    """tasks.build_generator: --sampling -> the Sampling strategy with its parameters and the seed; the reference's two assertions."""
    from test_decode_constraints_cpu import _tiny_model
    model, task = _tiny_model()
    M = SGM()
    gen = task.build_generator([model], Namespace(beam=3, sampling=True, sampling_topk=7, sampling_topp=0.8, seed=5))
    assert type(gen.search) is M.Sampling and (gen.search.sampling_topk, gen.search.sampling_topp, gen.seed) == (7, 0.8, 5)
    assert gen.sampling and gen.fused
    plain = task.build_generator([model], Namespace(beam=3))
    assert type(plain.search) is M.BeamSearch and not plain.sampling and plain.fused

    class Other(M.Sampling):
        pass

    assert not M.SequenceGenerator([model], task.target_dictionary, beam_size=2, search_strategy=Other(task.target_dictionary)).fused
    with pytest.raises(AssertionError, match="--sampling-topk requires --sampling"):
        task.build_generator([model], Namespace(beam=3, sampling_topk=7))
    with pytest.raises(AssertionError, match="--sampling-topp requires --sampling"):
        task.build_generator([model], Namespace(beam=3, sampling_topp=0.8))
