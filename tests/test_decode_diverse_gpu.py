"""GPU tests of the diverse decoding strategies --diverse-beam-groups / --diverse-beam-strength and --diversity-rate (beam_search.hip
cst_beam_step ABI 12, decode_engine.py, sequence_generator.py, cli.py):
  * cst_beam_step called directly, one case per row-kernel family, step by step against the torch restatement of
    tests/decode_diverse_util.py; identity of G = 1 and R = 0 with a plain step; bad arguments;
  * the engine and the host loop against the hypotheses of the REAL reference's SequenceGenerator (decode_diverse_tiny.npz);
  * engine == host loop on a two-member ensemble; the node count of the captured step; the command line."""
import ast
import ctypes
import os
import shutil
from argparse import Namespace
from importlib import import_module

import pytest
import torch

from conftest import GOLDEN, load_golden, load_pkg
from decode_diverse_util import BSZ, CASES, EOS, MAX_LEN, PAD, PREFIX, UNK, VARIANTS, SEEDS, new_state, search_step, step_logits
from test_decode_constraints_gpu import _ragged_sample, fixture_models
from test_decode_engine_gpu import _beam_state, _build_s2t
from test_model_gpu import assert_close

pytestmark = pytest.mark.gpu
ERR_BAD_ARG = -1  # CST_ERR_BAD_ARG


def sgm():
    load_pkg()
    return import_module("chimera-st_amd.sequence_generator")


@pytest.fixture(scope="module")
def L():
    load_pkg()
    return import_module("chimera-st_amd.lib")


def _set_mode(d, mode):
    if mode[0] == "groups":
        d.diverse_groups, d.diverse_strength = mode[1], mode[2]
    else:
        d.diverse_siblings, d.sibling_rate = 1, mode[1]


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("dtype_name,V,members", CASES)
def test_beam_step_diverse_matches_restatement(L, dtype_name, V, members, variant):
    """bsz 3, max_len 12, run to the end on fresh logits per step: after EVERY step the device state equals that of the fp32 torch
    restatement — tokens, ancestry (the parents), cands_to_ignore, finished, nfinal, fin_tokens, fin_len exactly; scores and fin_score to
    1e-5 (the kernel adds the penalty to lp + score, the reference to lp: one fp32 rounding, and test_decode_diverse_cpu.py shows that
    no id hangs on it).  bf16 cases feed the restatement the bf16-rounded logits."""
    beam, mode, ngram, with_prefix = VARIANTS[variant]
    seed = SEEDS.get((dtype_name, V, members, variant), 0)
    dtype = torch.bfloat16 if dtype_name == "bf16" else torch.float32
    lib = L.load()
    bbsz, Vp = BSZ * beam, (V + 7) // 8 * 8
    bufs = [torch.zeros(bbsz, Vp, dtype=dtype, device="cuda") for _ in range(members)]
    st, d = _beam_state(L, BSZ, beam, V, MAX_LEN, 1, dtype, bufs[0], pad=PAD, unk=UNK, eos=EOS)
    if members > 1:
        d.members = members
        for n in range(1, members):
            d.logits_n[n - 1] = bufs[n].data_ptr()
    d.no_repeat_ngram = ngram
    prefix = torch.tensor(PREFIX, dtype=torch.int64, device="cuda") if with_prefix else None
    if with_prefix:
        d.prefix_tokens, d.prefix_len = prefix.data_ptr(), prefix.size(1)
    _set_mode(d, mode)
    L.check(lib.cst_beam_init(ctypes.byref(d), L.stream_ptr()), "cst_beam_init")
    ref = new_state(beam, "cuda")
    for s in range(MAX_LEN + 1):
        logits = [x.cuda() for x in step_logits(dtype_name, V, members, s, beam, seed)]
        for buf, x in zip(bufs, logits):
            buf[:, :V] = x
        L.check(lib.cst_beam_step(ctypes.byref(d), L.stream_ptr()), "cst_beam_step")
        search_step(ref, logits, s, beam, mode=mode, ngram=ngram, prefix=prefix)
        assert int(st["step"].item()) == s + 1
        nxt = (s + 1) & 1 if s < MAX_LEN else s & 1  # the last step writes no new rows
        n_tok = min(s + 2, MAX_LEN + 1)
        assert torch.equal(st["tokens"][nxt, :, :n_tok], ref["tokens"][:, :n_tok]), s
        assert torch.equal(st["anc"][nxt, :, :n_tok], ref["anc"][:, :n_tok]), s
        got, want = st["scores"][nxt, :, :min(s + 1, MAX_LEN)], ref["scores"][:, :min(s + 1, MAX_LEN)]
        assert torch.equal(torch.isinf(got), torch.isinf(want)), s
        err = float((got - want).nan_to_num(0.0, 0.0, 0.0).abs().max())
        print("step %2d  max |scores - restatement| %.2e  max |score| %.1f  fin_score %.2e" % (
            s, err, float(want.nan_to_num(0.0, 0.0, 0.0).abs().max()), float((st["fin_score"] - ref["fin_score"]).abs().max())))
        assert err <= 1e-5, s  # (-inf on both sides: junk beams of a forced prefix)
        for k in ("ignore", "finished", "nfinal", "fin_len"):
            assert torch.equal(st[k], ref[k]), (k, s)
        assert torch.equal(st["fin_tokens"], ref["fin_tokens"]), s
        assert float((st["fin_score"] - ref["fin_score"]).abs().max()) <= 1e-5, s
    assert ref["finished"].tolist() == [1] * BSZ and int(st["num_remaining"].item()) == 0
    if with_prefix:  # eos inside the prefix: `beam` identical hypotheses
        assert st["fin_tokens"][1, :, :2].tolist() == [[PREFIX[1][0], EOS]] * beam and st["fin_len"][1].tolist() == [2] * beam


@pytest.mark.parametrize("mode", [("groups", 1, 0.5), ("siblings", 0.0)], ids=["G1", "R0"])
@pytest.mark.parametrize("dtype_name,V,members", [("fp32", 60, 1), ("bf16", 10000, 1)])
def test_one_group_and_rate_zero_equal_plain_beam_search_bitwise(L, dtype_name, V, members, mode):
    beam = 4
    dtype = torch.bfloat16 if dtype_name == "bf16" else torch.float32
    lib = L.load()
    buf = torch.zeros(BSZ * beam, (V + 7) // 8 * 8, dtype=dtype, device="cuda")
    runs = []
    for m in (None, mode):
        st, d = _beam_state(L, BSZ, beam, V, MAX_LEN, 1, dtype, buf, pad=PAD, unk=UNK, eos=EOS)
        if m is not None:
            _set_mode(d, m)
        L.check(lib.cst_beam_init(ctypes.byref(d), L.stream_ptr()), "cst_beam_init")
        snaps = []
        for s in range(MAX_LEN + 1):
            buf[:, :V] = step_logits(dtype_name, V, members, s, beam)[0].cuda()
            L.check(lib.cst_beam_step(ctypes.byref(d), L.stream_ptr()), "cst_beam_step")
            snaps.append({k: st[k].clone() for k in ("tokens", "scores", "anc", "ignore", "finished", "nfinal", "fin_tokens", "fin_pos",
                                                     "fin_score", "fin_len", "num_remaining")})
        runs.append(snaps)
    for s, (a, b) in enumerate(zip(*runs)):
        for k in a:
            same = torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) if a[k].dtype == torch.float32 else torch.equal(a[k], b[k])
            assert same, (k, s)
    assert runs[0][-1]["finished"].tolist() == [1] * BSZ


def test_beam_step_rejects_bad_diverse_arguments(L):
    lib = L.load()
    beam = 4
    logits = torch.zeros(BSZ * beam, 64, device="cuda")
    st, d = _beam_state(L, BSZ, beam, 60, MAX_LEN, 1, torch.float32, logits)
    L.check(lib.cst_beam_init(ctypes.byref(d), L.stream_ptr()), "cst_beam_init")
    torch.cuda.synchronize()
    before = {k: v.clone() for k, v in st.items()}
    key = torch.zeros(1, dtype=torch.int32, device="cuda")
    step = lib.cst_beam_step
    # (groups, strength, siblings, rate, sampling)
    for G, S, sib, R, samp in ((2, -0.5, 0, 0.0, 0), (0, 0.0, 1, -0.5, 0), (3, 0.5, 0, 0.0, 0), (8, 0.5, 0, 0.0, 0), (-1, 0.5, 0, 0.0, 0),
                               (2, 0.5, 1, 0.5, 0), (2, 0.5, 0, 0.0, 1), (0, 0.0, 1, 0.5, 1), (2, 0.5, 1, 0.5, 1), (2, float("nan"), 0, 0.0, 0)):
        d.diverse_groups, d.diverse_strength, d.diverse_siblings, d.sibling_rate = G, S, sib, R
        d.sampling, d.sample_key = samp, (key.data_ptr() if samp else None)
        assert step(ctypes.byref(d), L.stream_ptr()) == ERR_BAD_ARG, (G, S, sib, R, samp)
    torch.cuda.synchronize()
    for k, v in st.items():  # nothing was launched: the state buffers are untouched
        assert torch.equal(v, before[k]), k
    assert int(st["step"].item()) == 0
    d.diverse_groups, d.diverse_strength, d.diverse_siblings, d.sibling_rate, d.sampling, d.sample_key = 2, 0.5, 0, -1.0, 0, None
    L.check(step(ctypes.byref(d), L.stream_ptr()), "cst_beam_step")  # (the rate is read only when the switch is on)
    assert int(st["step"].item()) == 1


# ---- 2. the fixture of the real reference ---------------------------------------------------------------------------------------------
def _strategy(kw, tgt_dict):
    sg = sgm()
    if "groups" in kw:
        return sg.DiverseBeamSearch(tgt_dict, kw["groups"], kw["strength"])
    if "rate" in kw:
        return sg.DiverseSiblingsSearch(tgt_dict, kw["rate"])
    return None


SETTING_NAMES = ["base_b4", "base_b5", "base_b6", "base_ngram2", "base_prefix", "g2", "g2_ngram2", "g2_prefix", "g3", "g4", "sib4", "sib5"]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", SETTING_NAMES)
def test_diverse_matches_reference_generator(name, fused):
    """Every finalized hypothesis of the reference's SequenceGenerator in its order: ids exact, scores and positional scores to 1e-4 —
    device engine and host loop (DiverseBeamSearch / DiverseSiblingsSearch), fp32."""
    m = fixture_models()
    fx, rec = load_golden("decode_diverse_tiny.npz"), load_golden("decode_recipe_tiny.npz")
    settings = ast.literal_eval(str(fx["meta/settings"]))
    assert sorted(settings) == SETTING_NAMES
    kw = settings[name]
    model, d = m[kw["model"]], m["task"].target_dictionary
    gen = sgm().SequenceGenerator([model], d, beam_size=kw["beam_size"], max_len_a=0, max_len_b=kw["max_len_b"],
                                  no_repeat_ngram_size=kw.get("no_repeat_ngram_size", 0), temperature=kw.get("temperature", 1.0),
                                  search_strategy=_strategy(kw, d), fused=fused)
    sample = {"net_input": {"src_tokens": torch.from_numpy(rec["in/b/src_tokens"]).cuda(),
                            "src_lengths": torch.from_numpy(rec["in/b/src_lengths"]).cuda()}}
    prefix = torch.from_numpy(fx["meta/prefix"]).cuda() if kw.get("prefix") else None
    hyps = gen.generate([model], sample, prefix_tokens=prefix)
    assert (gen._engine is not None) == fused
    for b in range(len(hyps)):
        n = int(fx["gen/%s/b%d/n" % (name, b)])
        assert len(hyps[b]) == n, (name, b)
        for r in range(n):
            key = "gen/%s/b%d/r%d/" % (name, b, r)
            assert hyps[b][r]["tokens"].tolist() == fx[key + "tokens"].tolist(), key
            assert abs(float(hyps[b][r]["score"]) - float(fx[key + "score"])) < 1e-4, key
            assert_close(hyps[b][r]["positional_scores"], fx[key + "pos_scores"], 1e-4, key + "pos_scores")


# ---- 3. engine == host loop, the step graph ---------------------------------------------------------------------------------------------
def _flat(hyps):
    return [[(h["tokens"].tolist(), float(h["score"])) for h in hb] for hb in hyps]


def test_engine_equals_host_loop_on_an_ensemble_with_two_groups():
    models, task = [], None
    for k in range(2):
        m, task = _build_s2t(torch.float32, tied=(k == 1), seed=3 + k)
        models.append(m)
    d = task.target_dictionary
    sample = _ragged_sample()
    sg = sgm()
    kw = dict(beam_size=4, max_len_a=0, max_len_b=20, min_len=3)
    fused = sg.SequenceGenerator(models, d, search_strategy=sg.DiverseBeamSearch(d, 2, 0.5), **kw)
    mirror = sg.SequenceGenerator(models, d, search_strategy=sg.DiverseBeamSearch(d, 2, 0.5), fused=False, **kw)
    h1, h2 = fused.generate(models, sample), mirror.generate(models, sample)
    assert fused._engine is not None and len(fused._engine.decs) == 2 and fused._engine.opt.diverse_groups == 2 and mirror._engine is None
    plain = _flat(sg.SequenceGenerator(models, d, **kw).generate(models, sample))
    for b in range(4):
        assert len(h1[b]) == len(h2[b]) == 4
        for r in range(4):
            assert h1[b][r]["tokens"].tolist() == h2[b][r]["tokens"].tolist(), (b, r)
            assert abs(float(h1[b][r]["score"]) - float(h2[b][r]["score"])) < 1e-4
    assert [[t for t, _ in hb] for hb in _flat(h1)] != [[t for t, _ in hb] for hb in plain]


def test_step_graph_has_the_same_nodes_with_a_diverse_strategy():
    """The diverse strategies live in the merge kernel, so a step is the same launch sequence.  Counted per strategy, not assumed: the
    launch records of ONE step of the engine — the sequence its graph captures, one node per launch — in the library's profiler.
    (The captured graph's own DOT dump, torch's debug_dump, writes no file on this stack, so the count is taken from the launches.)"""
    model, task = _build_s2t(torch.float32, tied=False)
    d = task.target_dictionary
    sample = _ragged_sample()
    sg, lib = sgm(), import_module("chimera-st_amd.lib")
    launches = {}
    for name, strat in (("plain", None), ("groups", sg.DiverseBeamSearch(d, 2, 0.5)), ("siblings", sg.DiverseSiblingsSearch(d, 0.5))):
        gen = sg.SequenceGenerator([model], d, beam_size=4, max_len_a=0, max_len_b=8, search_strategy=strat)
        gen.generate([model], sample)
        eng = gen._engine
        states = list(eng._state.values())
        assert len(states) == 1 and states[0]["graph"] is not None
        assert (eng.opt.diverse_groups, eng.opt.sibling_rate) == {"plain": (0, None), "groups": (2, None), "siblings": (0, 0.5)}[name]
        st, pk = states[0], eng._packed[1]
        lib.check(lib.load().cst_beam_init(ctypes.byref(st["desc"]), lib.stream_ptr()), "cst_beam_init")  # back to step 0
        torch.cuda.synchronize()
        lib.prof_enable(True)
        eng._step(st, pk, 4)
        torch.cuda.synchronize()
        table = lib.prof_query()
        lib.prof_enable(False)
        launches[name] = sum(v["launches"] for v in table.values())
    print("launch records of a step", launches)
    assert launches["groups"] == launches["siblings"] == launches["plain"] > 2, launches


# ---- 4. the command line ----------------------------------------------------------------------------------------------------
def test_cli_diverse_flags(tmp_path, capsys):
    """fairseq_generate.py --beam 4 --nbest 4 with --diverse-beam-groups 2 / --diversity-rate 0.5 on tests/golden/data_tiny: the summary
    carries the flags and no ignored flag, 4 hypotheses per sentence are printed, and they are those of a direct SequenceGenerator call
    with the same strategy (which differ from plain beam search's); --diverse-beam-groups 2 --sampling is refused."""
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
    common = [str(root), "--path", path, "--task", "triplet", "--config-yaml", "config_wave.yaml", "--gen-subset", "dev_st", "--max-tokens",
              "12000", "--beam", "4", "--nbest", "4", "--max-len-b", "12", "--max-source-positions", "2000000", "--temperature", "2"]

    seen = {}  # the batches the command line handed to its generator: the independent call below decodes the same ones
    sg = sgm()
    orig = sg.SequenceGenerator.generate

    def spy(self, models, sample, **kw):
        seen["gen"] = self
        seen.setdefault("calls", []).append((models, sample, kw))
        return orig(self, models, sample, **kw)

    def run(extra):
        capsys.readouterr()
        seen.clear()
        sg.SequenceGenerator.generate = spy
        try:
            summary = cli.generate_main(common + extra)
        finally:
            sg.SequenceGenerator.generate = orig
        out = capsys.readouterr().out.splitlines()
        hyp = {}
        for l in out:
            if l.startswith("H-"):
                hyp.setdefault(int(l.split("\t")[0][2:]), []).append(l.split("\t")[-1])
        return summary, hyp, seen["gen"], list(seen["calls"])

    printed = {}
    for extra, make, params, want in (
            (["--diverse-beam-groups", "2"], lambda d: sg.DiverseBeamSearch(d, 2, 0.5), dict(num_groups=2, diversity_strength=0.5),
             dict(diverse_beam_groups=2, diverse_beam_strength=0.5, diversity_rate=-1.0)),
            (["--diversity-rate", "0.5"], lambda d: sg.DiverseSiblingsSearch(d, 0.5), dict(diversity_rate=0.5),
             dict(diverse_beam_groups=-1, diversity_rate=0.5)),
            ([], lambda d: None, {}, dict(diverse_beam_groups=-1, diversity_rate=-1.0))):
        summary, hyp, cli_gen, calls = run(extra)
        assert summary["ignored_flags"] == [] and summary["nbest"] == 4
        for k, v in want.items():
            assert summary[k] == v, (k, summary)
        tgt = cli_gen.tgt_dict
        strat = make(tgt)
        assert type(cli_gen.search) is (sg.BeamSearch if strat is None else type(strat)) and cli_gen.fused
        for k, v in params.items():  # the flags' values reached the strategy
            assert getattr(cli_gen.search, k) == v, k
        # a direct SequenceGenerator call with the strategy built HERE, on the batches the command line decoded
        direct = sg.SequenceGenerator(calls[0][0], tgt, beam_size=4, max_len_a=0, max_len_b=12, temperature=2.0, search_strategy=strat)
        hyps = [hb for models, sample, kw in calls for hb in direct.generate(models, sample, **kw)]
        assert direct._engine is not None
        assert summary["sentences"] == len(hyp) == len(hyps) > 0 and all(len(h) == 4 for h in hyp.values())
        strings = sorted(tuple(tgt.string(h["tokens"].cpu()) for h in hb[:4]) for hb in hyps)
        assert sorted(tuple(h) for h in hyp.values()) == strings
        printed[tuple(extra)] = hyp
    assert printed[("--diverse-beam-groups", "2")] != printed[()] and printed[("--diversity-rate", "0.5")] != printed[()]
    with pytest.raises(ValueError, match="mutually exclusive"):
        cli.generate_main(common + ["--diverse-beam-groups", "2", "--sampling"])
