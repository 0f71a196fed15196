"""GPU tests of sampling decode (--sampling, --sampling-topk, --sampling-topp, --nbest; beam_search.hip cst_beam_step with
cst_beam_desc.sampling, decode_engine.py, sequence_generator.py Sampling, cli.py):
  * cst_beam_step called directly, every register-resident dispatch family, against the fp64 restatement of decode_sampling_util.py;
  * the frequencies of 10 240 draws against the kept distribution (Pearson);
  * engine and host loop against the hypotheses of the REAL reference's SequenceGenerator + Sampling (decode_sampling_tiny.npz);
  * engine == host loop at top-p 0.9, replay of one captured graph with other keys, bad arguments, the wide-vocabulary route, the node
    count of a step, and the command line with --nbest."""
import ast
import ctypes
import math
import os
import shutil
from argparse import Namespace
from importlib import import_module

import numpy as np
import pytest
import torch

import decode_sampling_util as U
from conftest import GOLDEN, load_golden, load_pkg
from test_decode_constraints_gpu import _ragged_sample, fixture_models
from test_decode_engine_gpu import _beam_state, _build_s2t
from test_model_gpu import assert_close

pytestmark = pytest.mark.gpu
BSZ, BEAM, MAX_LEN, PAD, EOS, UNK = U.BSZ, U.BEAM, U.MAX_LEN, U.PAD, U.EOS, U.UNK
ERR_BAD_ARG, ERR_UNSUPPORTED = -1, -4
# 0.999 quantiles of chi-square, 1 .. 40 degrees of freedom
CHI2_999 = [10.828, 13.816, 16.266, 18.467, 20.515, 22.458, 24.322, 26.124, 27.877, 29.588, 31.264, 32.909, 34.528, 36.123, 37.697, 39.252,
            40.79, 42.312, 43.82, 45.315, 46.797, 48.268, 49.728, 51.179, 52.62, 54.052, 55.476, 56.892, 58.301, 59.703, 61.098, 62.487, 63.87,
            65.247, 66.619, 67.985, 69.346, 70.703, 72.055, 73.402]


def SGM():
    load_pkg()
    return import_module("chimera-st_amd.sequence_generator")


@pytest.fixture(scope="module")
def L():
    load_pkg()
    return import_module("chimera-st_amd.lib")


def _sampling_desc(L, d, topk, topp, key):
    """Switches a beam descriptor to sampling; returns the key buffer (kept alive by the caller)."""
    kb = torch.tensor([key - (1 << 32) if key >= (1 << 31) else key], dtype=torch.int32, device="cuda")
    d.sampling, d.sample_topk, d.sample_topp, d.sample_key = 1, topk, topp, kb.data_ptr()
    return kb


def _device_candidates(st, bsz, beam):
    """(value, token) of the sentence's `beam` candidates as the row kernel left them in the workspace: 64 bytes of ticket, then the value
    array and the token array of bsz * beam * 2 * beam entries each; sampling uses the first bsz * beam of either."""
    n = bsz * beam * 2 * beam
    ws = st["ws"]
    val = ws[64:64 + 4 * n].view(torch.float32)[:bsz * beam].cpu()
    tok = ws[64 + 4 * n:64 + 8 * n].view(torch.int32)[:bsz * beam].cpu()
    return val, tok


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(U.VARIANTS))
@pytest.mark.parametrize("dtype_name,V,members", U.CASES)
def test_beam_step_sampling_matches_restatement(L, dtype_name, V, members, variant):
    """bsz 3 x beam 4, max_len 12, run to the end on fresh logits per step: after EVERY step the device state equals the fp64
    restatement's — tokens, ancestry, cands_to_ignore, finished, nfinal, fin_tokens, fin_len exactly; scores and fin_score to 1e-5.
    A draw may differ only where the restatement calls it undecidable (DELTA from the kernel's stated addition chain), and then only to
    a token of the DELTA-widened kept set with that token's own score; the restatement adopts it.  At most 2 % of a case's draws."""
    topk, topp, temperature, ngram, with_prefix, min_len = U.VARIANTS[variant]
    dtype = torch.bfloat16 if dtype_name == "bf16" else torch.float32
    assert U.family(dtype_name, V) in ("NV1", "NV3", "NV5")
    lib = L.load()
    bbsz, Vp = BSZ * BEAM, (V + 7) // 8 * 8
    bufs = [torch.zeros(bbsz, Vp, dtype=dtype, device="cuda") for _ in range(members)]
    st, d = _beam_state(L, BSZ, BEAM, V, MAX_LEN, min_len, dtype, bufs[0], temperature=temperature, pad=PAD, unk=UNK, eos=EOS)
    if members > 1:
        d.members = members
        for n in range(1, members):
            d.logits_n[n - 1] = bufs[n].data_ptr()
    d.no_repeat_ngram = ngram
    prefix = torch.tensor(U.PREFIX, dtype=torch.int64) if with_prefix else None
    prefix_d = prefix.cuda() if with_prefix else None
    if with_prefix:
        d.prefix_tokens, d.prefix_len = prefix_d.data_ptr(), prefix.size(1)
    key = U.case_key(dtype_name, V, members, variant)
    kb = _sampling_desc(L, d, topk, topp, key)
    L.check(lib.cst_beam_init(ctypes.byref(d), L.stream_ptr()), "cst_beam_init")
    ref = U.new_state()
    draws = forgiven = undecidable = 0
    worst = 0.0
    for s in range(MAX_LEN + 1):
        logits = U.step_logits(dtype_name, V, members, s)
        for buf, x in zip(bufs, logits):
            buf[:, :V] = x.cuda()
        L.check(lib.cst_beam_step(ctypes.byref(d), L.stream_ptr()), "cst_beam_step")
        assert int(st["step"].item()) == s + 1
        lp = U.masked_lprobs(ref, logits, s, temperature, ngram, prefix, min_len)
        cands = U.step_draws(ref, lp, s, key, topk, topp, prefix)
        dev_val, dev_tok = _device_candidates(st, BSZ, BEAM)
        for i, c in enumerate(cands):
            draws += 1
            undecidable += not c["decidable"]
            t = int(dev_tok[i])
            if t != c["tok"]:
                assert not c["decidable"], ("a decidable draw differs", s, i, t, c["tok"])
                assert 0 <= t < V and c["wide"][t], ("drawn outside the widened kept set", s, i, t)
                U.adopt(ref, c, t, s)
                forgiven += 1
            assert c["tok"] == PAD or c["kept"][t] or (not c["decidable"] and c["wide"][t]), ("drawn outside the kept set", s, i, t)
            v = float(dev_val[i])
            if math.isinf(c["score"]):
                assert v == c["score"], (s, i)
            else:
                worst = max(worst, abs(v - c["score"]))
        U.bookkeeping(ref, cands, s)
        nxt = (s + 1) & 1 if s < MAX_LEN else s & 1  # the last step writes no new rows
        n_tok = min(s + 2, MAX_LEN + 1)
        assert torch.equal(st["tokens"][nxt, :, :n_tok].cpu(), ref["tokens"][:, :n_tok]), s
        assert torch.equal(st["anc"][nxt, :, :n_tok].cpu(), ref["anc"][:, :n_tok]), s
        got, want = st["scores"][nxt, :, :min(s + 1, MAX_LEN)].cpu().double(), ref["scores"][:, :min(s + 1, MAX_LEN)]
        assert torch.equal(torch.isinf(got), torch.isinf(want)), s
        err = float((got - want).nan_to_num(0.0, 0.0, 0.0).abs().max())
        fin_err = float((st["fin_score"].cpu().double() - ref["fin_score"]).abs().max())
        print("step %2d  max |scores - restatement| %.2e  candidates %.2e  fin_score %.2e  max |score| %.1f" % (
            s, err, worst, fin_err, float(want.nan_to_num(0.0, 0.0, 0.0).abs().max())))
        assert err <= 1e-5 and worst <= 1e-5 and fin_err <= 1e-5, s
        for k in ("ignore", "finished", "nfinal", "fin_len"):
            assert torch.equal(st[k].cpu(), ref[k]), (k, s)
        assert torch.equal(st["fin_tokens"].cpu(), ref["fin_tokens"]), s
    print("%d draws, %d undecidable, %d forgiven" % (draws, undecidable, forgiven))
    assert forgiven <= 0.02 * draws
    assert ref["finished"].tolist() == [1] * BSZ and ref["nfinal"].tolist() == [BEAM] * BSZ and int(st["num_remaining"].item()) == 0
    if with_prefix:  # eos inside the prefix: `beam` identical hypotheses
        assert st["fin_tokens"][1, :, :2].tolist() == [[U.PREFIX[1][0], EOS]] * BEAM and st["fin_len"][1].tolist() == [2] * BEAM
    del kb


# ---- 2. frequencies ----------------------------------------------------------------------------------------------------------------
def test_draw_frequencies_follow_the_kept_distribution(L):
    """One fixed row, V = 64, top-p 0.9, bsz 64 x beam 20 at step 0, 8 keys = 10 240 draws: Pearson's statistic against the renormalised
    kept distribution stays below the 0.999 quantile of chi-square (fixed keys: a fixed outcome)."""
    lib = L.load()
    V, bsz, beam = 64, 64, 20
    g = torch.Generator().manual_seed(5)
    row = torch.randn(V, generator=g) * 1.5
    logits = row.repeat(bsz * beam, 1).cuda().contiguous()
    lp = torch.log_softmax(row.double(), dim=-1)
    lp[PAD] = -math.inf
    lp[EOS] = -math.inf  # step 0 < min_len 1
    kept = U.kept_set(lp.numpy(), topp=0.9)[0]
    expect = np.where(kept, np.exp(lp.numpy()), 0.0)
    expect /= expect.sum()
    assert 8 <= kept.sum() <= 40
    counts = np.zeros(V)
    for key in range(8):
        st, d = _beam_state(L, bsz, beam, V, 12, 1, torch.float32, logits, pad=PAD, unk=UNK, eos=EOS)
        kb = _sampling_desc(L, d, 0, 0.9, 1000003 * (key + 1))
        L.check(lib.cst_beam_init(ctypes.byref(d), L.stream_ptr()), "cst_beam_init")
        L.check(lib.cst_beam_step(ctypes.byref(d), L.stream_ptr()), "cst_beam_step")
        tok = _device_candidates(st, bsz, beam)[1].numpy()
        counts += np.bincount(tok, minlength=V)
        del kb
    n = counts.sum()
    assert n == 10240 and not counts[~kept].any()
    stat = float((((counts - n * expect) ** 2)[kept] / (n * expect[kept])).sum())
    dof = int(kept.sum()) - 1
    print("Pearson %.2f at %d degrees of freedom (0.999 quantile %.2f); smallest expected count %.1f" % (
        stat, dof, CHI2_999[dof - 1], n * expect[kept].min()))
    assert stat < CHI2_999[dof - 1]


# ---- 3. the fixture of the real reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", ["topk1", "topp1e-6"])
def test_sampling_matches_reference_generator(name, fused):
    """The reference's SequenceGenerator with its Sampling strategy where it has no choice (top-k 1, top-p 1e-6): ids exact, scores to
    1e-4, the `beam` hypotheses of a sentence identical — device engine and host loop, fp32."""
    m = fixture_models()
    g = load_golden("decode_sampling_tiny.npz")
    kw = ast.literal_eval(str(g["meta/settings"]))[name]
    M = SGM()
    d = m["task"].target_dictionary
    model = m["fitted"]
    gen = M.SequenceGenerator([model], d, beam_size=int(g["meta/beam"]), max_len_a=0, max_len_b=int(g["meta/max_len_b"]),
                              search_strategy=M.Sampling(d, **kw), fused=fused, seed=3)
    sample = {"net_input": {"src_tokens": torch.from_numpy(g["in/src_tokens"]).cuda(), "src_lengths": torch.from_numpy(g["in/src_lengths"]).cuda()}}
    hyps = gen.generate([model], sample)
    assert (gen._engine is not None) == fused
    for b in range(len(hyps)):
        n = int(g["gen/%s/b%d/n" % (name, b)])
        assert len(hyps[b]) == n == int(g["meta/beam"]), (name, b)
        for r in range(n):
            key = "gen/%s/b%d/r%d/" % (name, b, r)
            assert hyps[b][r]["tokens"].tolist() == g[key + "tokens"].tolist() == hyps[b][0]["tokens"].tolist(), key
            assert abs(float(hyps[b][r]["score"]) - float(g[key + "score"])) < 1e-4, key
            assert_close(hyps[b][r]["positional_scores"], g[key + "pos_scores"], 1e-3, key + "pos_scores")


# ---- 4. engine == host loop, keys on one captured graph --------------------------------------------------------------------------------
def _flat(hyps):
    return [[(h["tokens"].tolist(), float(h["score"])) for h in hb] for hb in hyps]


def test_engine_equals_host_loop_and_replays_with_new_keys():
    """fp32 s2t_transformer, top-p 0.9, beam 4.  The host loop runs a recording subclass of Sampling (a subclass takes the host loop):
    per sentence the first step with an undecidable draw.  Up to there the engine's samples are the host loop's; at least 90 % of the
    sentences are compared to the end.  Keys a, b, a on ONE captured graph: first and third call bit-identical, the second differs."""
    M = SGM()
    model, task = _build_s2t(torch.float32, tied=False)
    with torch.no_grad():  # sharper still: a nucleus of a handful of tokens has few CDF edges and a large step at its cut, so few draws are undecidable
        model.decoder.output_projection.weight.mul_(2.0)
    d = task.target_dictionary
    g = torch.Generator().manual_seed(29)
    B, T, beam = 12, 97, 4
    src = torch.randn(B, T, 80, generator=g).cuda()
    lens = torch.tensor([97, 90, 85, 80, 72, 64, 51, 47, 40, 33, 26, 20]).cuda()
    sample = {"net_input": {"src_tokens": src, "src_lengths": lens}}
    first_bad = {}

    class Recording(M.Sampling):
        def step(self, step, lprobs, scores, key=0, max_len=None):
            lp = lprobs.double().cpu()
            rows = lp[:, ::lp.size(1)].expand(-1, lp.size(1), -1) if step == 0 else lp
            u = U.uniforms(key, np.arange(lp.size(0) * lp.size(1)) * (max_len + 1) + step).reshape(lp.size(0), lp.size(1))
            for b in range(lp.size(0)):
                for k in range(lp.size(1)):
                    if b not in first_bad and not U.draw(rows[b, k], float(u[b, k]), 0, self.sampling_topp)["decidable"]:
                        first_bad[b] = step
            return super().step(step, lprobs, scores, key=key, max_len=max_len)

    kw = dict(beam_size=beam, max_len_a=0, max_len_b=10)
    gen = M.SequenceGenerator([model], d, search_strategy=M.Sampling(d, sampling_topp=0.9), **kw)
    mirror = M.SequenceGenerator([model], d, search_strategy=Recording(d, sampling_topp=0.9), **kw)
    assert gen.fused and gen.sampling and not mirror.fused
    key_a, key_b = 0xC0FFEE11, 0x0BADF00D
    h_a = gen.generate([model], sample, sample_key=key_a)
    graphs = [st["graph"] for st in gen._engine._state.values()]
    assert len(graphs) == 1 and graphs[0] is not None
    h_b = gen.generate([model], sample, sample_key=key_b)
    h_a2 = gen.generate([model], sample, sample_key=key_a)
    assert [st["graph"] for st in gen._engine._state.values()] == graphs  # replayed, not re-captured
    for b in range(B):
        for x, y in zip(h_a[b], h_a2[b]):
            assert torch.equal(x["tokens"], y["tokens"]) and torch.equal(x["score"], y["score"])
            assert torch.equal(x["positional_scores"], y["positional_scores"])
    assert sum(_flat(h_a)[b] != _flat(h_b)[b] for b in range(B)) >= 1
    want = mirror.generate([model], sample, sample_key=key_a)
    assert mirror._engine is None
    whole = 0
    for b in range(B):
        assert len(h_a[b]) == len(want[b]) == beam
        t = first_bad.get(b)
        if t is None:
            whole += 1
            for x, y in zip(h_a[b], want[b]):
                assert x["tokens"].tolist() == y["tokens"].tolist(), b
                assert abs(float(x["score"]) - float(y["score"])) < 1e-4
        else:  # the samples agree in their first t tokens (as a multiset: the order of the hypotheses follows the scores)
            assert sorted(x["tokens"].tolist()[:t] for x in h_a[b]) == sorted(y["tokens"].tolist()[:t] for y in want[b]), (b, t)
    print("%d of %d sentences compared to the end; first undecidable steps %s" % (whole, B, first_bad))
    assert whole >= 0.9 * B
    assert len({tuple(x["tokens"].tolist()) for b in range(B) for x in h_a[b]}) > B  # samples of a sentence differ
    # the generator's own stream of keys: two calls draw differently, two generators with one seed draw alike
    g1 = M.SequenceGenerator([model], d, search_strategy=M.Sampling(d, sampling_topp=0.9), seed=7, **kw)
    g2 = M.SequenceGenerator([model], d, search_strategy=M.Sampling(d, sampling_topp=0.9), seed=7, **kw)
    c1, c2 = _flat(g1.generate([model], sample)), _flat(g1.generate([model], sample))
    assert c1 != c2 and _flat(g2.generate([model], sample)) == c1


# ---- 5. bad arguments --------------------------------------------------------------------------------------------------------------
def test_beam_step_rejects_bad_sampling_arguments(L):
    lib = L.load()
    logits = torch.zeros(BSZ * BEAM, 64, device="cuda")
    st, d = _beam_state(L, BSZ, BEAM, 60, MAX_LEN, 1, torch.float32, logits)
    L.check(lib.cst_beam_init(ctypes.byref(d), L.stream_ptr()), "cst_beam_init")
    kb = torch.zeros(1, dtype=torch.int32, device="cuda")
    step = lib.cst_beam_step
    for sampling, topk, key in ((1, 0, None), (1, -1, kb.data_ptr()), (1, 61, kb.data_ptr()), (0, -3, None), (0, 61, None)):
        d.sampling, d.sample_topk, d.sample_topp, d.sample_key = sampling, topk, 0.0, key
        assert step(ctypes.byref(d), L.stream_ptr()) == ERR_BAD_ARG, (sampling, topk)
    torch.cuda.synchronize()
    assert int(st["step"].item()) == 0  # nothing was launched
    # the wide family only selects: a message and the library's "unsupported" status, nothing launched
    wide = torch.zeros(BSZ * BEAM, 10248, device="cuda")
    st2, d2 = _beam_state(L, BSZ, BEAM, 10248, MAX_LEN, 1, torch.float32, wide)
    L.check(lib.cst_beam_init(ctypes.byref(d2), L.stream_ptr()), "cst_beam_init")
    d2.sampling, d2.sample_key = 1, kb.data_ptr()
    assert step(ctypes.byref(d2), L.stream_ptr()) == ERR_UNSUPPORTED and b"host loop" in lib.cst_last_error()
    torch.cuda.synchronize()
    assert int(st2["step"].item()) == 0
    d.sampling, d.sample_topk, d.sample_topp, d.sample_key = 1, 60, 0.0, kb.data_ptr()
    L.check(step(ctypes.byref(d), L.stream_ptr()), "cst_beam_step")
    assert int(st["step"].item()) == 1


# ---- 6. / 7. the wide-vocabulary route and the node count ------------------------------------------------------------------------------
def test_wide_vocabulary_takes_the_host_loop_and_the_node_count_is_unchanged():
    M = SGM()
    eng = import_module("chimera-st_amd.decode_engine").BeamDecodeEngine
    assert eng.sampling_supported(10240, torch.float32) and not eng.sampling_supported(10241, torch.float32)
    assert eng.sampling_supported(20480, torch.bfloat16) and not eng.sampling_supported(20481, torch.bfloat16)
    sample = _ragged_sample()
    wide_model, wide_task = _build_s2t(torch.float32, V=10300, tied=True)
    dw = wide_task.target_dictionary
    kw = dict(beam_size=2, max_len_a=0, max_len_b=4)
    gen = M.SequenceGenerator([wide_model], dw, search_strategy=M.Sampling(dw, sampling_topk=4), **kw)
    hyps = gen.generate([wide_model], sample)
    assert gen.fused and gen._engine is None and all(len(h) == 2 for h in hyps)  # picked up front: no engine was built
    beam_gen = M.SequenceGenerator([wide_model], dw, **kw)
    beam_gen.generate([wide_model], sample)
    assert beam_gen._engine is not None  # beam search still runs on the engine's wide kernel
    model, task = _build_s2t(torch.float32, tied=False)
    d = task.target_dictionary
    kw = dict(beam_size=4, max_len_a=0, max_len_b=8)
    samp = M.SequenceGenerator([model], d, search_strategy=M.Sampling(d, sampling_topp=0.9), **kw)
    off = M.SequenceGenerator([model], d, **kw)
    samp.generate([model], sample)
    off.generate([model], sample)
    rows = 4 * 4
    assert samp._engine.opt.sampling and not off._engine.opt.sampling
    assert samp._engine.nodes_per_step(torch.float32, rows) == off._engine.nodes_per_step(torch.float32, rows)


# ---- 8. the command line -----------------------------------------------------------------------------------------------------------
def test_cli_sampling_with_nbest(tmp_path, capsys):
    """fairseq_generate.py --sampling --sampling-topp 0.9 --beam 3 --nbest 3 on tests/golden/data_tiny: three H- lines per sentence,
    nothing ignored, and the summary names the sampling settings."""
    cli = import_module("chimera-st_amd.cli")
    cu = import_module("chimera-st_amd.checkpoint_utils")
    m = fixture_models()
    model, args = m["unfitted"], m["args"]
    data = os.path.join(GOLDEN, "data_tiny")
    root = tmp_path / "data"
    root.mkdir()
    for f in os.listdir(data):
        if not f.endswith(".wav"):
            shutil.copy(os.path.join(data, f), root / f)
    (root / "config_wave.yaml").write_text((root / "config_wave.yaml").read_text().replace("AUDIO_ROOT", data))
    lines = (root / "dict.txt").read_text().splitlines()
    V = model.decoder.embed_tokens.num_embeddings
    lines += ["filler%d 1" % i for i in range(V - 4 - len(lines))]
    (root / "dict.txt").write_text("\n".join(lines) + "\n")
    a = Namespace(**vars(args))
    a.arch, a.task, a.no_save_optimizer_state = "s2t_transformer_w2v2_interlingua_base", "triplet", True
    a.data, a.config_yaml = str(root), "config_wave.yaml"
    path = str(tmp_path / "m.pt")
    cu.save_state(path, a, model.state_dict(), None, None, 0)
    argv = [str(root), "--path", path, "--task", "triplet", "--config-yaml", "config_wave.yaml", "--gen-subset", "dev_st", "--max-tokens",
            "12000", "--beam", "3", "--max-len-b", "12", "--max-source-positions", "2000000", "--sampling", "--sampling-topp", "0.9",
            "--nbest", "3", "--seed", "11"]
    capsys.readouterr()
    summary = cli.generate_main(argv)
    out = capsys.readouterr().out.splitlines()
    n_h = {}
    for l in out:
        if l.startswith("H-"):
            sid = int(l.split("\t")[0][2:])
            n_h[sid] = n_h.get(sid, 0) + 1
    assert summary["sentences"] == len(n_h) > 0 and set(n_h.values()) == {3}
    assert sum(l.startswith("D-") for l in out) == sum(l.startswith("P-") for l in out) == 3 * len(n_h)
    assert summary["ignored_flags"] == [] and summary["sampling"] is True and summary["nbest"] == 3 and summary["seed"] == 11
    with pytest.raises(ValueError, match="--nbest 4 must be between 1 and --beam 3"):
        cli.generate_main(argv[:-4] + ["--nbest", "4"])
