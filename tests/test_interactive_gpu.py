"""GPU tests of typed input (fairseq_interactive.py) and of generation from decoder-only models, against the fixture the REAL reference
made (interactive_tiny.npz: tools/ref_harness/make_interactive_goldens.py):
  * the fixture's LM on prompts — every setting through the device engine (decoder-only members: no cross block, no encoder K/V) and
    through the host loop: token ids exact, scores and positional scores within 1e-4; an ensemble of the LM twice equals the LM;
  * speech and MT end to end through interactive_main --input FILE at buffer sizes 1 and 3;
  * bf16, the other search strategies on prompts, the command line on an LM checkpoint.
Every test here fails on the parent commit: the driver and the tasks' typed-input methods do not exist there, and the generator reads
`model.encoder` of a model that has none."""
import io
import json
import math
import os
from argparse import Namespace
from importlib import import_module

import pytest
import torch

import interactive_util as U
from conftest import GOLDEN, load_golden, load_pkg
from interactive_util import cli
from test_decode_lm_gpu import _build_lm, fixture_lm

pytestmark = pytest.mark.gpu
PAD, EOS = 1, 2
TOL = 1e-4  # scores and positional scores, natural log


def SG():
    load_pkg()
    return import_module("chimera-st_amd.sequence_generator")


@pytest.fixture(scope="module")
def g():
    return load_golden("interactive_tiny.npz")


def gen_kw(setting):
    kw = dict(setting)
    return dict(beam_size=kw.pop("beam_size"), max_len_a=0, max_len_b=kw.pop("max_len_b"), min_len=1, **kw)


def lm_batches(g, task, buf):
    lines = [str(x) for x in g["lm/prompts/" + buf]]
    return list(cli.make_batches(lines, U.batch_args(batch_size=len(lines)), task, 1024, lambda x: x, err=io.StringIO(), prompt_ok=lambda n: True))


def to_sample(batch):
    ni = batch["net_input"]
    return {"net_input": {"src_tokens": ni["src_tokens"].cuda(), "src_lengths": ni["src_lengths"].cuda()}}


def assert_hyps(hyps, g, key, what=""):
    want = U.fixture_hyps(g, key)
    assert len(hyps) == len(want), (key, what)
    worst = 0.0
    for b, (hb, wb) in enumerate(zip(hyps, want)):
        assert len(hb) == len(wb), (key, what, b, len(hb), len(wb))
        for r, (h, w) in enumerate(zip(hb, wb)):
            assert h["tokens"].tolist() == w["tokens"].tolist(), (key, what, b, r)
            ds = abs(float(h["score"]) - float(w["score"]))
            dp = float((h["positional_scores"].cpu().float() - w["positional_scores"]).abs().max())
            worst = max(worst, ds, dp)
            assert ds < TOL and dp < TOL, (key, what, b, r, ds, dp)
    return worst


# ---- 1. the fixture's LM on prompts, fp32 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["beam5", "beam1", "lenpen_ngram", "boundary"])
def test_lm_prompts_match_the_reference(g, name):
    """Every setting, both buffers (the ragged batch of three: one sentence generates freely while another is still forced; the batch
    of one: at beam 1 a single row), engine and host loop: ids exact, scores and positional scores within 1e-4 of the reference's, and
    of each other.  `boundary`: the longest prompt is exactly max_len long — its one finite hypothesis is the prompt and eos."""
    lm, _, _ = fixture_lm()
    task = U.lm_task()
    kw = gen_kw(U.lm_settings(g)[name])
    fused = SG().SequenceGenerator([lm], task.target_dictionary, **kw)
    host = SG().SequenceGenerator([lm], task.target_dictionary, fused=False, **kw)
    assert fused.fused and not fused.has_encoder and not host.fused
    for buf in ("ragged", "one"):
        for j, (ids, batch, _) in enumerate(lm_batches(g, task, buf)):
            key = "lm/%s/%s/batch%d" % (name, buf, j)
            h1 = task.inference_step(fused, [lm], to_sample(batch))
            h2 = task.inference_step(host, [lm], to_sample(batch))
            eng = fused._engine
            assert eng is not None and eng.decoder_only and eng.lm is None and host._engine is None
            print(key, "engine %.2e host %.2e" % (assert_hyps(h1, g, key, "engine"), assert_hyps(h2, g, key, "host loop")))
            for b in range(len(h1)):
                prompt = [t for t in batch["net_input"]["src_tokens"][b, 1:].tolist() if t != PAD]
                for a, c in zip(h1[b], h2[b]):
                    assert a["tokens"].tolist() == c["tokens"].tolist() and a["tokens"].tolist()[:len(prompt)] == prompt
                    assert abs(float(a["score"]) - float(c["score"])) < TOL
                if name == "boundary" and len(prompt) == kw["max_len_b"]:
                    assert len(h1[b]) == 1 and h1[b][0]["tokens"].tolist() == prompt + [EOS]
            if name == "beam1" and buf == "one":
                assert next(iter(eng._state.values()))["tokens"].shape[1] == 1  # one row


def test_decoder_only_engine_state_and_plan(g):
    """No cross blocks, no encoder K/V, no source length in the state key; the launch count is the LM member's of shallow fusion."""
    lm, _, _ = fixture_lm()
    task = U.lm_task()
    gen = SG().SequenceGenerator([lm], task.target_dictionary, **gen_kw(U.lm_settings(g)["beam5"]))
    (ids, batch, _), = lm_batches(g, task, "ragged")
    first = task.inference_step(gen, [lm], to_sample(batch))
    eng = gen._engine
    (key, st), = eng._state.items()
    assert key[2] is None and key[5] is None and key[6] == 4  # (lane, bsz, S, dtype, device, has_mask, prefix_len, options, lex)
    (m,) = st["members"]
    assert not m["plan"].cross and m["plan"].cross_mode is None and not any(k in m for k in ("kx", "vx", "q", "kpm", "proj"))
    assert all("ln_q" not in p for p in eng._packed[1][0]["layers"])
    assert eng.nodes_per_step(torch.float32, 15) == 1 + 7 * len(lm.decoder.layers) + 1 + 1 + 2
    graph = st["graph"]
    again = task.inference_step(gen, [lm], to_sample(batch))  # the same configuration replays the captured graph
    assert next(iter(eng._state.values()))["graph"] is graph
    assert [[h["tokens"].tolist() for h in hb] for hb in again] == [[h["tokens"].tolist() for h in hb] for hb in first]
    # empty prompts: a batch of their own, no prefix — the fixture's unprompted decode
    free = task.inference_step(gen, [lm], {"net_input": {"src_tokens": torch.full((2, 1), EOS).cuda(), "src_lengths": torch.ones(2, dtype=torch.long).cuda()}})
    assert free[0][0]["tokens"].tolist() == free[1][0]["tokens"].tolist() == g["lm/unprompted/b0/r0/tokens"].tolist()
    assert abs(float(free[0][0]["score"]) - float(g["lm/unprompted/b0/r0/score"])) < TOL
    with pytest.raises(ValueError, match="starts with eos or pad"):  # (_check_prefix is what it was: the DRIVER keeps empty prompts apart)
        gen.generate([lm], {"net_input": {"src_tokens": torch.tensor([[EOS, 9], [EOS, PAD]]).cuda()}}, prefix_tokens=torch.tensor([[9], [PAD]]).cuda())


@pytest.mark.parametrize("fused", [True, False])
def test_an_ensemble_of_the_lm_twice_equals_the_lm(g, fused):
    lm, _, _ = fixture_lm()
    twin, _, _ = fixture_lm()
    task = U.lm_task()
    kw = gen_kw(U.lm_settings(g)["beam5"])
    gen = SG().SequenceGenerator([lm, twin], task.target_dictionary, fused=fused, **kw)
    for buf in ("ragged", "one"):
        for j, (ids, batch, _) in enumerate(lm_batches(g, task, buf)):
            hyps = task.inference_step(gen, [lm, twin], to_sample(batch))
            assert_hyps(hyps, g, "lm/beam5/%s/batch%d" % (buf, j), "ensemble")
    if fused:
        eng = gen._engine
        assert len(eng.decs) == 2 and eng.decoder_only and len(next(iter(eng._state.values()))["members"]) == 2
        assert eng.nodes_per_step(torch.float32, 15) == 2 * (1 + 7 * len(lm.decoder.layers) + 1 + 1) + 2


def test_mixed_members_and_fusion_into_an_lm_are_refused():
    from test_ensemble_gpu import fixture_members
    models, task, _, _ = fixture_members(1)
    lm, _, _ = fixture_lm()
    E = import_module("chimera-st_amd.decode_engine")
    with pytest.raises(ValueError, match="of one kind"):
        SG().SequenceGenerator([models[0], lm], task.target_dictionary)
    with pytest.raises(ValueError, match="of one kind"):
        E.BeamDecodeEngine([models[0].decoder, lm.decoder], task.target_dictionary, E.DecodeOptions(5, 12))
    with pytest.raises(ValueError, match="itself a language model"):
        SG().SequenceGenerator([lm], task.target_dictionary, lm_model=lm, lm_weight=0.3)
    with pytest.raises(ValueError, match="cross attention"):
        SG().SequenceGenerator([lm], task.target_dictionary, return_attention=True)
    with pytest.raises(NotImplementedError, match="bos_token"):
        SG().SequenceGenerator([lm], task.target_dictionary).generate([lm], {"net_input": {"src_tokens": torch.full((1, 1), EOS).cuda()}}, bos_token=0)


STRATEGIES = {"sampling_topk": lambda S, d: S.Sampling(d, 5, -1.0), "sampling_topp": lambda S, d: S.Sampling(d, -1, 0.8),
              "diverse_groups": lambda S, d: S.DiverseBeamSearch(d, 2, 0.5), "siblings": lambda S, d: S.DiverseSiblingsSearch(d, 0.3)}


@pytest.mark.parametrize("name", sorted(STRATEGIES))
def test_the_other_strategies_on_prompts_engine_equals_host_loop(g, name):
    """Sampling (top-k, top-p), the diverse strategies, with temperature, an unk penalty and min_len 3: the kernels do not care where
    the logits came from.  The ragged prompt batch, beam 4: engine and host loop give the same hypotheses, and each begins with its prompt."""
    S = SG()
    lm, _, _ = fixture_lm()
    task = U.lm_task()
    d = task.target_dictionary
    kw = dict(beam_size=4, max_len_a=0, max_len_b=10, min_len=3, temperature=0.9, unk_penalty=0.2, seed=7)
    fused = S.SequenceGenerator([lm], d, search_strategy=STRATEGIES[name](S, d), **kw)
    host = S.SequenceGenerator([lm], d, search_strategy=STRATEGIES[name](S, d), fused=False, **kw)
    (ids, batch, _), = lm_batches(g, task, "ragged")
    h1, h2 = task.inference_step(fused, [lm], to_sample(batch)), task.inference_step(host, [lm], to_sample(batch))
    assert fused._engine is not None and fused._engine.decoder_only and host._engine is None
    for b in range(3):
        prompt = [t for t in batch["net_input"]["src_tokens"][b, 1:].tolist() if t != PAD]
        assert len(h1[b]) == len(h2[b]) > 0
        for a, c in zip(h1[b], h2[b]):
            assert a["tokens"].tolist() == c["tokens"].tolist() and a["tokens"].tolist()[:len(prompt)] == prompt
            assert len(a["tokens"]) >= 4 and abs(float(a["score"]) - float(c["score"])) < TOL


# ---- 2. speech and MT end to end ---------------------------------------------------------------------------------------------------------
def run_main(argv, capsys):
    capsys.readouterr()
    summary = cli.interactive_main(argv)
    cap = capsys.readouterr()
    return summary, cap.out, cap.err


def assert_stdout(got, want):
    """Line by line: the tag, the id and every text field are the recorded bytes; the numeric fields (which the reference's own CPU runs
    do not reproduce to the last digit between buffer sizes: H-0 of st/buf1 and st/buf3 differ in the 8th) within 1e-4 in natural log,
    that is 1e-4 / ln 2 as printed (P- prints four decimals: both sides' rounding adds up to 1e-4); W- carries the run's own time."""
    got, want = got.splitlines(), want.splitlines()
    assert [l.split("\t")[0] for l in got] == [l.split("\t")[0] for l in want]
    for a, b in zip(got, want):
        (ta, na, xa), (tb, nb, xb) = U.split_line(a), U.split_line(b)
        assert ta == tb and xa == xb and len(na) == len(nb), (a, b)
        assert all(abs(x - y) < TOL / math.log(2) + (1e-4 if ta.startswith("P-") else 0.0) for x, y in zip(na, nb)), (a, b)
        if a.startswith("W-"):
            assert a.split("\t")[2] == "seconds" and float(a.split("\t")[1]) >= 0.0


@pytest.mark.parametrize("size", [1, 3])
def test_speech_end_to_end(g, tmp_path, capsys, size):
    """fairseq_interactive.py <data> --task triplet --config-yaml config_wave.yaml --path ref_checkpoint_tiny.pt on typed audio paths
    (talk_a, talk_b, talk_a; --max-tokens cuts the buffer of three into [0, 2] and [1]): no S-/W-/C- lines, the H-/D-/P- lines of the
    reference in input order, nothing else on stdout; the JSON summary on stderr."""
    root = U.speech_data_dir(tmp_path / "d")
    inp = tmp_path / "paths.txt"
    inp.write_text("".join(os.path.join(U.DATA_TINY, str(x)) + "\n" for x in g["st/lines"]))
    summary, out, err = run_main([root, "--task", "triplet", "--config-yaml", "config_wave.yaml", "--path", os.path.join(GOLDEN, "ref_checkpoint_tiny.pt"),
                                  "--max-tokens", str(int(g["st/max_tokens"])), "--max-source-positions", "2000000", "--beam", str(int(g["st/beam"])),
                                  "--max-len-b", str(int(g["st/max_len_b"])), "--buffer-size", str(size), "--input", str(inp)], capsys)
    assert_stdout(out, str(g["st/buf%d/stdout" % size]))
    assert "S-" not in out and "W-" not in out
    last = json.loads(err.strip().splitlines()[-1])
    assert last["event"] == "interactive" and last["sentences"] == summary["sentences"] == 3 and last["tokens"] > 0
    assert last["seconds"] >= last["translate_seconds"] > 0


def mt_checkpoint(tmp_path):
    import ast

    import numpy as np
    cu = import_module("chimera-st_amd.checkpoint_utils")
    fx = load_golden("chimera_tiny.npz")
    a = Namespace(**ast.literal_eval(str(fx["meta/model_args"])))
    a.arch, a.task, a.no_save_optimizer_state = "s2t_transformer_w2v2_interlingua_base", "translation", True
    a.w2v2_model_path, a.w2v_args = "synthetic:golden_tiny", ast.literal_eval(str(fx["meta/w2v_args"]))
    a.data, a.source_lang, a.target_lang, a.left_pad_source, a.left_pad_target = U.MT_ROOT, None, None, "True", "False"
    path = str(tmp_path / "mt.pt")
    cu.save_state(path, a, {k[len("param/"):]: torch.from_numpy(np.array(v)) for k, v in fx.items() if k.startswith("param/")}, None, None, 0)
    return path


@pytest.mark.parametrize("case", ["plain", "plain_buf1", "constrained"])
def test_translation_end_to_end(g, tmp_path, capsys, case):
    """Typed sentences through a checkpoint saved from the fixture's parameters: S-/W-/C-/H-/D-/P- as recorded, at buffer sizes 3 and 1
    (recorded apart: this model's output for a sentence depends on the padding beside it in its batch, in the reference too)."""
    size = int(g["mt/%s/buffer_size" % case])
    path = mt_checkpoint(tmp_path)
    inp = tmp_path / "lines.txt"
    inp.write_text("".join(str(x) + "\n" for x in g["mt/%s/lines" % case]), encoding="utf-8")
    argv = [U.MT_ROOT, "--task", "translation", "--path", path, "--max-tokens", str(int(g["mt/max_tokens"])), "--beam", str(int(g["mt/beam"])),
            "--max-len-a", str(float(g["mt/max_len_a"])), "--max-len-b", str(int(g["mt/max_len_b"])), "--buffer-size", str(size), "--input", str(inp)]
    summary, out, err = run_main(argv + (["--constraints"] if case == "constrained" else []), capsys)
    assert_stdout(out, str(g["mt/%s/stdout" % case]))
    assert summary["sentences"] == len(g["mt/%s/lines" % case])
    assert out.count("W-") == summary["sentences"] and (out.count("C-") == 2) == (case == "constrained")


# ---- 3. the command line on an LM checkpoint ---------------------------------------------------------------------------------------------
def lm_checkpoint(tmp_path, name="lm.pt"):
    cu = import_module("chimera-st_amd.checkpoint_utils")
    lm, lm_args, _ = fixture_lm()
    root = tmp_path / "lm_data"
    root.mkdir(exist_ok=True)
    (root / "dict.txt").write_text("".join("w%d 1\n" % i for i in range(U.VOCAB - 4)))
    a = Namespace(**vars(lm_args))
    a.task, a.data, a.no_save_optimizer_state = "language_modeling", str(root), True
    path = str(tmp_path / name)
    cu.save_state(path, a, lm.state_dict(), None, None, 0)
    return str(root), path


def test_cli_on_a_language_model_checkpoint(g, tmp_path, capsys):
    """Prompts, an empty prompt and one beyond max_len in one buffer, on one checkpoint and on the ensemble a.pt:b.pt: the H- lines of
    the prompts are the fixture's hypotheses, the empty prompt gets the unprompted decode, the long one a message and no lines."""
    root, path = lm_checkpoint(tmp_path)
    _, twin = lm_checkpoint(tmp_path, "twin.pt")
    prompts = [str(x) for x in g["lm/prompts/ragged"]]
    lines = prompts[:2] + ["", " ".join("w%d" % i for i in range(13))] + prompts[2:]
    inp = tmp_path / "prompts.txt"
    inp.write_text("".join(l + "\n" for l in lines))
    d = U.word_dictionary()
    for p in (path, path + ":" + twin):
        summary, out, err = run_main([root, "--path", p, "--beam", "5", "--max-len-b", "12", "--buffer-size", "5", "--batch-size", "5", "--input", str(inp)], capsys)
        rows = out.splitlines()
        assert [l.split("\t")[0] for l in rows] == [t + str(i) for i in (0, 1, 2, 4) for t in ("S-", "W-", "H-", "D-", "P-")]
        assert summary["sentences"] == 4 and summary["models"] == len(p.split(":"))
        assert [l for l in err.splitlines() if l.startswith("input")] == ["input 3 skipped: a prompt of 13 tokens exceeds the step limit max_len "
                                                                          "(--max-len-a, --max-len-b, the model's positions)"]
        got = {int(l.split("\t")[0][2:]): l.split("\t") for l in rows if l.startswith("H-")}
        src = {int(l.split("\t")[0][2:]): l.split("\t")[1] for l in rows if l.startswith("S-")}
        assert [src[i] for i in (0, 1, 2, 4)] == [prompts[0], prompts[1], "", prompts[2]]
        for i, b in ((0, 0), (1, 1), (4, 2)):
            key = "lm/beam5/ragged/batch0/b%d/r0/" % b
            assert got[i][2] == d.string(g[key + "tokens"].tolist())
            assert abs(float(got[i][1]) * math.log(2) - float(g[key + "score"])) < TOL
        assert got[2][2] == d.string(g["lm/unprompted/b0/r0/tokens"].tolist())
    with pytest.raises(NotImplementedError, match="language_modeling"):  # fairseq_generate.py keeps refusing the checkpoint
        cli.generate_main([root, "--path", path])
    # the reference dies on a prompt beyond the model's positions; so does this driver, unless told to skip
    with pytest.raises(Exception, match="--skip-invalid-size-inputs-valid-test"):
        cli.interactive_main([root, "--path", path, "--max-target-positions", "3", "--input", str(inp)])


# ---- 4. bf16 -------------------------------------------------------------------------------------------------------------------------------
def test_bf16_lm_prompts_real_dimensions():
    """C 512, 8 heads, F 4096, 2 layers, V 10 000, beam 5 in bf16 — the LayerNorm-folded projections and the split-K fc2 of a decoder-only
    member: the decode of 8 ragged prompts completes, every hypothesis begins with its prompt, scores are finite and ordered, and first
    free tokens agree with the bf16 host loop in >= 6 of 8 (the standard of test_decode_lm_gpu.test_bf16_real_dimensions)."""
    lm = _build_lm(torch.bfloat16, d=512, heads=8, layers=2, V=10000, ffn=4096)
    task = U.tasks.LanguageModelingTask(Namespace(tokens_per_sample=1024), U.Dictionary.synthetic(10000))
    gq = torch.Generator().manual_seed(3)
    lens = [1, 2, 3, 4, 5, 6, 7, 9]
    src = torch.full((8, 10), PAD, dtype=torch.long)
    src[:, 0] = EOS
    for b, n in enumerate(lens):
        src[b, 1:1 + n] = torch.randint(4, 10000, (n,), generator=gq)
    sample = {"net_input": {"src_tokens": src.cuda(), "src_lengths": torch.tensor([n + 1 for n in lens]).cuda()}}
    kw = dict(beam_size=5, max_len_a=0, max_len_b=20)
    fused = SG().SequenceGenerator([lm], task.target_dictionary, **kw)
    h1 = task.inference_step(fused, [lm], sample)
    h2 = task.inference_step(SG().SequenceGenerator([lm], task.target_dictionary, fused=False, **kw), [lm], sample)
    eng = fused._engine
    assert eng is not None and eng.decoder_only and all("ln_qkv" in p and "ln_fc1" in p and "ln_q" not in p for p in eng._packed[1][0]["layers"])
    assert eng._member_nodes(lm.decoder, torch.bfloat16, 40) == 1 + 6 * 2 + 1 + 1
    agree = 0
    for b, n in enumerate(lens):
        prompt = src[b, 1:1 + n].tolist()
        sc = [float(h["score"]) for h in h1[b]]
        assert len(sc) == 5 and all(math.isfinite(s) for s in sc) and sc == sorted(sc, reverse=True)
        assert all(h["tokens"].tolist()[:n] == prompt for h in h1[b]) and all(h["tokens"].tolist()[:n] == prompt for h in h2[b])
        agree += int(h1[b][0]["tokens"][n]) == int(h2[b][0]["tokens"][n])
    assert agree >= 6


def test_bf16_speech_end_to_end(g, tmp_path, capsys):
    """--bf16 on the typed audio paths: the decode completes, one H-/D-/P- group per path in input order, finite scores, and the two
    readings of talk_a.wav (one batch) get the same tokens."""
    root = U.speech_data_dir(tmp_path / "d")
    inp = tmp_path / "paths.txt"
    inp.write_text("".join(os.path.join(U.DATA_TINY, str(x)) + "\n" for x in g["st/lines"]))
    summary, out, _ = run_main([root, "--task", "triplet", "--config-yaml", "config_wave.yaml", "--path", os.path.join(GOLDEN, "ref_checkpoint_tiny.pt"),
                                "--max-tokens", str(int(g["st/max_tokens"])), "--max-source-positions", "2000000", "--beam", "5", "--max-len-b", "12",
                                "--buffer-size", "3", "--input", str(inp), "--bf16"], capsys)
    rows = out.splitlines()
    assert [l.split("\t")[0] for l in rows] == [t + str(i) for i in range(3) for t in ("H-", "D-", "P-")] and summary["sentences"] == 3
    assert all(math.isfinite(float(l.split("\t")[1])) for l in rows if l[0] in "HD")
    assert rows[0].split("\t")[2] == rows[6].split("\t")[2] and abs(float(rows[0].split("\t")[1]) - float(rows[6].split("\t")[1])) < 1e-2
