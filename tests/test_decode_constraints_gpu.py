"""GPU tests of the decoding constraints --no-repeat-ngram-size / --prefix-size (beam_search.hip cst_beam_step, decode_engine.py,
sequence_generator.py, cli.py):
  * cst_beam_step called directly, every dispatch family, against the torch restatement of tests/decode_constraints_util.py;
  * the engine and the host loop against the hypotheses of the REAL reference's SequenceGenerator (decode_constraints_tiny.npz);
  * engine == host loop on fresh ragged audio, also for a 2-member ensemble;
  * graph replay with a new prefix, the node count of a step, and the command line."""
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

from conftest import GOLDEN, load_golden, load_pkg
from decode_constraints_util import BEAM, BSZ, CASES, EOS, MAX_LEN, PAD, PREFIX, UNK, VARIANTS, new_state, search_step, step_logits
from test_decode_engine_gpu import _beam_state, _build_s2t
from test_model_gpu import assert_close, build_from_golden

pytestmark = pytest.mark.gpu


def SG():
    load_pkg()
    return import_module("chimera-st_amd.sequence_generator").SequenceGenerator


@pytest.fixture(scope="module")
def L():
    load_pkg()
    return import_module("chimera-st_amd.lib")


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("dtype_name,V,members", CASES)
def test_beam_step_constraints_match_restatement(L, dtype_name, V, members, variant):
    """bsz 3 x beam 4, max_len 12, run to the end on fresh logits per step (six tokens far above the rest, so hypotheses repeat):
    after EVERY step the device state equals that of the fp32 torch restatement — tokens, ancestry, cands_to_ignore, finished, nfinal,
    fin_tokens, fin_len exactly; scores and fin_score to 1e-5.  bf16 cases feed the restatement the bf16-rounded logits."""
    ngram, with_prefix, min_len = VARIANTS[variant]
    dtype = torch.bfloat16 if dtype_name == "bf16" else torch.float32
    lib = L.load()
    bbsz, Vp = BSZ * BEAM, (V + 7) // 8 * 8
    bufs = [torch.zeros(bbsz, Vp, dtype=dtype, device="cuda") for _ in range(members)]
    st, d = _beam_state(L, BSZ, BEAM, V, MAX_LEN, min_len, dtype, bufs[0], pad=PAD, unk=UNK, eos=EOS)
    if members > 1:
        d.members = members
        for n in range(1, members):
            d.logits_n[n - 1] = bufs[n].data_ptr()
    d.no_repeat_ngram = ngram
    prefix = torch.tensor(PREFIX, dtype=torch.int64, device="cuda") if with_prefix else None
    if with_prefix:
        d.prefix_tokens, d.prefix_len = prefix.data_ptr(), prefix.size(1)
    L.check(lib.cst_beam_init(ctypes.byref(d), L.stream_ptr()), "cst_beam_init")
    ref = new_state("cuda")
    for s in range(MAX_LEN + 1):
        logits = [x.cuda() for x in step_logits(dtype_name, V, members, s)]
        for buf, x in zip(bufs, logits):
            buf[:, :V] = x
        L.check(lib.cst_beam_step(ctypes.byref(d), L.stream_ptr()), "cst_beam_step")
        search_step(ref, logits, s, ngram=ngram, prefix=prefix, min_len=min_len)
        assert int(st["step"].item()) == s + 1
        nxt = (s + 1) & 1 if s < MAX_LEN else s & 1  # the last step writes no new rows
        n_tok = min(s + 2, MAX_LEN + 1)
        assert torch.equal(st["tokens"][nxt, :, :n_tok], ref["tokens"][:, :n_tok]), s
        assert torch.equal(st["anc"][nxt, :, :n_tok], ref["anc"][:, :n_tok]), s
        got, want = st["scores"][nxt, :, :min(s + 1, MAX_LEN)], ref["scores"][:, :min(s + 1, MAX_LEN)]
        assert torch.equal(torch.isinf(got), torch.isinf(want)), s
        print("step %2d  max |scores - restatement| %.2e  max |score| %.1f  fin_score %.2e" % (
            s, float((got - want).nan_to_num(0.0, 0.0, 0.0).abs().max()), float(want.nan_to_num(0.0, 0.0, 0.0).abs().max()),
            float((st["fin_score"] - ref["fin_score"]).abs().max())))
        assert float((got - want).nan_to_num(0.0, 0.0, 0.0).abs().max()) <= 1e-5, s  # (-inf on both sides: junk beams of a forced prefix)
        for k in ("ignore", "finished", "nfinal", "fin_len"):
            assert torch.equal(st[k], ref[k]), (k, s)
        assert torch.equal(st["fin_tokens"], ref["fin_tokens"]), s
        assert float((st["fin_score"] - ref["fin_score"]).abs().max()) <= 1e-5, s
    assert ref["finished"].tolist() == [1] * BSZ and int(st["num_remaining"].item()) == 0
    if ngram:
        assert ref["banned_pairs"] >= BSZ * BEAM * (MAX_LEN + 1) / 4  # the comparison above saw the ban at work
    if with_prefix:  # eos inside the prefix: `beam` identical hypotheses
        assert st["fin_tokens"][1, :, :2].tolist() == [[PREFIX[1][0], EOS]] * BEAM and st["fin_len"][1].tolist() == [2] * BEAM


def test_beam_step_rejects_bad_constraint_arguments(L):
    lib = L.load()
    logits = torch.zeros(BSZ * BEAM, 64, device="cuda")
    st, d = _beam_state(L, BSZ, BEAM, 60, MAX_LEN, 1, torch.float32, logits)
    L.check(lib.cst_beam_init(ctypes.byref(d), L.stream_ptr()), "cst_beam_init")
    prefix = torch.full((BSZ, MAX_LEN + 1), 7, dtype=torch.int64, device="cuda")
    bad = L.load().cst_beam_step
    ERR_BAD_ARG = -1  # CST_ERR_BAD_ARG
    for ngram, ptr, plen in ((1, None, 0), (-2, None, 0), (0, None, 2), (0, prefix.data_ptr(), MAX_LEN + 1), (0, prefix.data_ptr(), -1)):
        d.no_repeat_ngram, d.prefix_tokens, d.prefix_len = ngram, ptr, plen
        assert bad(ctypes.byref(d), L.stream_ptr()) == ERR_BAD_ARG, (ngram, plen)
    torch.cuda.synchronize()
    assert int(st["step"].item()) == 0  # nothing was launched
    d.no_repeat_ngram, d.prefix_tokens, d.prefix_len = 2, prefix.data_ptr(), MAX_LEN
    L.check(bad(ctypes.byref(d), L.stream_ptr()), "cst_beam_step")
    assert int(st["step"].item()) == 1


# ---- 2. the fixture of the real reference ---------------------------------------------------------------------------------------------
_MODELS = {}


def fixture_models():
    """fitted = decode_tiny.npz; unfitted = the same with the tensors decode_constraints_tiny.npz stores (float16-exact values)."""
    if not _MODELS:
        g, con = load_golden("decode_tiny.npz"), load_golden("decode_constraints_tiny.npz")
        gu = dict(g)
        for name, v in con.items():
            if name.startswith("unfitted/param/"):
                key = "param/" + name[len("unfitted/param/"):]
                assert key in gu
                gu[key] = v.astype(np.float32)
        fitted, task, args = build_from_golden(g, "chimera", torch.float32)
        unfitted, _, _ = build_from_golden(gu, "chimera", torch.float32)
        _MODELS.update(fitted=fitted.eval(), unfitted=unfitted.eval(), task=task, args=args, con=con)
    return _MODELS


def _fixture_sample(con):
    return {"net_input": {"src_tokens": torch.from_numpy(con["in/src_tokens"]).cuda(), "src_lengths": torch.from_numpy(con["in/src_lengths"]).cuda()}}


SETTING_NAMES = ["base_fitted", "base_fitted_minlen", "base_unfitted", "ngram2", "ngram3", "prefix", "prefix_ngram_minlen"]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", SETTING_NAMES)
def test_constraints_match_reference_generator(name, fused):
    """Every finalized hypothesis of the reference's SequenceGenerator in its order: ids exact, scores to 1e-4, positional scores to
    1e-3 (the bars of the recipe test) — device engine and host loop, fp32."""
    m = fixture_models()
    con = m["con"]
    settings = ast.literal_eval(str(con["meta/settings"]))
    assert sorted(settings) == SETTING_NAMES
    kw = settings[name]
    model = m[kw["model"]]
    gen = SG()([model], m["task"].target_dictionary, beam_size=kw["beam_size"], max_len_a=0, max_len_b=kw["max_len_b"],
               min_len=kw.get("min_len", 1), no_repeat_ngram_size=kw.get("no_repeat_ngram_size", 0), fused=fused)
    prefix = torch.from_numpy(con["meta/prefix"]).cuda() if kw.get("prefix") else None
    hyps = gen.generate([model], _fixture_sample(con), prefix_tokens=prefix)
    assert (gen._engine is not None) == fused
    for b in range(len(hyps)):
        n = int(con["gen/%s/b%d/n" % (name, b)])
        assert len(hyps[b]) == n, (name, b)
        for r in range(n):
            key = "gen/%s/b%d/r%d/" % (name, b, r)
            assert hyps[b][r]["tokens"].tolist() == con[key + "tokens"].tolist(), key
            assert abs(float(hyps[b][r]["score"]) - float(con[key + "score"])) < 1e-4, key
            assert_close(hyps[b][r]["positional_scores"], con[key + "pos_scores"], 1e-3, key + "pos_scores")


# ---- 3. engine == host loop on fresh ragged audio -------------------------------------------------------------------------------------
def _flat(hyps):
    return [[(h["tokens"].tolist(), float(h["score"])) for h in hb] for hb in hyps]


def _ragged_sample(B=4, T=97):
    g = torch.Generator().manual_seed(23)
    src = torch.randn(B, T, 80, generator=g).cuda()
    return {"net_input": {"src_tokens": src, "src_lengths": torch.tensor([97, 80, 51, 20]).cuda()}}


@pytest.mark.parametrize("members", [1, 2])
def test_engine_equals_host_loop_with_both_constraints(members):
    models, task = [], None
    for k in range(members):
        m, task = _build_s2t(torch.float32, tied=(k == 1), seed=3 + k)  # a tied random-init model repeats one token: blocking has work to do
        models.append(m)
    d = task.target_dictionary
    sample = _ragged_sample()
    prefix = torch.tensor([[10, 11, 12], [13, d.eos(), d.pad()], [14, d.pad(), d.pad()], [15, 16, d.pad()]]).cuda()
    kw = dict(beam_size=4, max_len_a=0, max_len_b=20, min_len=3, no_repeat_ngram_size=2)
    fused, mirror = SG()(models, d, **kw), SG()(models, d, fused=False, **kw)
    h1, h2 = fused.generate(models, sample, prefix_tokens=prefix), mirror.generate(models, sample, prefix_tokens=prefix)
    assert fused._engine is not None and len(fused._engine.decs) == members and mirror._engine is None
    plain = SG()(models, d, beam_size=4, max_len_a=0, max_len_b=20, min_len=3).generate(models, sample)
    differs = 0
    for b in range(4):
        assert len(h1[b]) == len(h2[b]) == 4
        for r in range(4):
            toks = h1[b][r]["tokens"].tolist()
            assert toks == h2[b][r]["tokens"].tolist(), (b, r)
            assert abs(float(h1[b][r]["score"]) - float(h2[b][r]["score"])) < 1e-4
            grams = list(zip([d.eos()] + toks, toks))
            assert len(grams) == len(set(grams)), toks
            want = [t for t in prefix[b].tolist() if t != d.pad()]
            assert toks[:len(want)] == want
        differs += h1[b][0]["tokens"].tolist() != plain[b][0]["tokens"].tolist()
    assert h1[1][0]["tokens"].tolist() == [13, d.eos()] and differs == 4


# ---- 4. graph replay ----------------------------------------------------------------------------------------------------------
def test_replayed_graph_reads_the_new_prefix_and_has_no_extra_node():
    model, task = _build_s2t(torch.float32, tied=False)
    d = task.target_dictionary
    sample = _ragged_sample()
    kw = dict(beam_size=4, max_len_a=0, max_len_b=16, no_repeat_ngram_size=3)
    gen, mirror = SG()([model], d, **kw), SG()([model], d, fused=False, **kw)
    p1 = torch.tensor([[10, 11], [12, 13], [14, d.pad()], [15, 16]]).cuda()
    p2 = torch.tensor([[20, 21], [22, d.pad()], [23, 24], [25, 26]]).cuda()
    first = _flat(gen.generate([model], sample, prefix_tokens=p1))
    graphs = [st["graph"] for st in gen._engine._state.values()]
    assert len(graphs) == 1 and graphs[0] is not None
    keep = p2.clone()
    second = _flat(gen.generate([model], sample, prefix_tokens=p2))
    assert [st["graph"] for st in gen._engine._state.values()] == graphs  # replayed, not re-captured
    assert torch.equal(p2, keep)
    for p, got in ((p1, first), (p2, second)):
        want = _flat(mirror.generate([model], sample, prefix_tokens=p))
        for b in range(4):
            need = [t for t in p[b].tolist() if t != d.pad()]
            for r in range(4):
                assert got[b][r][0][:len(need)] == need
                assert got[b][r][0] == want[b][r][0] and abs(got[b][r][1] - want[b][r][1]) < 1e-4
    assert first != second
    off = SG()([model], d, beam_size=4, max_len_a=0, max_len_b=16)
    off.generate([model], sample)
    rows = 4 * 4
    assert gen._engine.nodes_per_step(torch.float32, rows) == off._engine.nodes_per_step(torch.float32, rows)
    # ... and the count is the captured graph's own: the engine's launch sequence does not depend on the constraints
    assert gen._engine.opt.no_repeat_ngram_size == 3 and off._engine.opt.no_repeat_ngram_size == 0


# ---- 5. the command line ----------------------------------------------------------------------------------------------------
def test_cli_prefix_size_and_no_repeat_ngram_size(tmp_path, capsys):
    """fairseq_generate.py --prefix-size 2 --no-repeat-ngram-size 2 on tests/golden/data_tiny: every H- line starts with its T- line's
    first two tokens and holds no bigram twice; without the flags some hypothesis does not start that way."""
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
              "12000", "--beam", "4", "--max-len-b", "12", "--max-source-positions", "2000000"]

    def run(extra):
        capsys.readouterr()
        summary = cli.generate_main(common + extra)
        out = capsys.readouterr().out.splitlines()
        pick = lambda tag: {int(l.split("\t")[0][2:]): l.split("\t")[-1].split() for l in out if l.startswith(tag)}
        return summary, pick("H-"), pick("T-")

    summary, hyp, ref = run(["--prefix-size", "2", "--no-repeat-ngram-size", "2"])
    assert summary["sentences"] == len(hyp) == len(ref) > 0
    for sid, h in hyp.items():
        assert h[:2] == ref[sid][:2], (sid, h, ref[sid])
        grams = list(zip(h, h[1:]))
        assert len(grams) == len(set(grams)), (sid, h)
    _, plain, _ = run([])
    assert any(plain[sid][:2] != ref[sid][:2] for sid in ref)
    assert any(len(set(zip(h, h[1:]))) != len(h) - 1 for h in plain.values())
