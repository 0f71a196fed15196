"""fairseq_interactive.py on the host (no GPU): buffered_read, the parser's defaults, checks and refusals, and — against the fixture
the REAL reference made (interactive_tiny.npz: tools/ref_harness/make_interactive_goldens.py) — every task's tokens and lengths, the
inference dataset's batches and their order, the printed lines, bad lines, and the batching of empty prompts."""
import io
import os
from argparse import Namespace
from importlib import import_module

import numpy as np
import pytest
import torch

import interactive_util as U
from conftest import load_golden
from interactive_util import cli

PAD, EOS = 1, 2


@pytest.fixture(scope="module")
def g():
    return load_golden("interactive_tiny.npz")


def parse(extra):
    return cli.interactive_parser().parse_args(["DATA", "--path", "m.pt"] + extra)


# ---- reading and the parser ---------------------------------------------------------------------------------------------------
def test_buffered_read(tmp_path, monkeypatch):
    p = tmp_path / "in.txt"
    p.write_text("  a b \nc\n\n d\te \ne\n", encoding="utf-8")
    assert list(cli.buffered_read(str(p), 2)) == [["a b", "c"], ["", "d\te"], ["e"]]  # stripped; the tab inside a line stays
    assert list(cli.buffered_read(str(p), 5)) == [["a b", "c", "", "d\te", "e"]]
    assert list(cli.buffered_read(str(p), 1)) == [["a b"], ["c"], [""], ["d\te"], ["e"]]
    monkeypatch.setattr("sys.stdin", io.StringIO("x\ny\nz\n"))
    assert list(cli.buffered_read("-", 2)) == [["x", "y"], ["z"]]
    empty = tmp_path / "empty.txt"
    empty.write_text("")
    assert list(cli.buffered_read(str(empty), 3)) == []


def test_parser_defaults_are_generates_and_interactives():
    a, gen = parse([]), cli.generate_parser().parse_args(["DATA", "--path", "m.pt"])
    for k, v in vars(gen).items():
        if k not in ("max_source_positions", "max_target_positions"):  # (here: the checkpoint's, see interactive_parser)
            assert getattr(a, k) == v, k
    assert (a.max_source_positions, a.max_target_positions) == (None, None)
    assert (a.buffer_size, a.input, a.bpe, a.sentencepiece_model, a.tokenizer, a.skip_invalid_size_inputs_valid_test) == (0, "-", None, None, None, False)
    cli.check_interactive_args(a)
    assert a.buffer_size == 1 and a.batch_size == 1  # raised to 1; neither --max-tokens nor --batch-size: sentences one by one
    b = cli.check_interactive_args(parse(["--max-tokens", "100", "--buffer-size", "4"]))
    assert b.batch_size is None and b.buffer_size == 4
    c = cli.check_interactive_args(parse(["--batch-size", "4", "--buffer-size", "4", "--sampling", "--nbest", "5"]))
    assert c.batch_size == 4


def test_checks_and_refusals_by_name(monkeypatch):
    cu = cli.checkpoint_utils
    monkeypatch.setattr(cu, "load_model_ensemble_and_task", lambda *a, **k: pytest.fail("a checkpoint was read before the checks"))
    with pytest.raises(AssertionError, match="--sampling requires --nbest to be equal to --beam"):
        cli.interactive_main(["DATA", "--path", "m.pt", "--sampling", "--nbest", "2"])
    with pytest.raises(AssertionError, match="--batch-size cannot be larger than --buffer-size"):
        cli.interactive_main(["DATA", "--path", "m.pt", "--batch-size", "4", "--buffer-size", "2"])
    for flags, exc, name in ((["--score-reference"], NotImplementedError, "--score-reference"),
                             (["--prefix-size", "2"], NotImplementedError, "--prefix-size"),
                             (["--tokenizer", "moses"], NotImplementedError, "moses"),
                             (["--bpe", "gpt2"], NotImplementedError, "gpt2"),
                             (["--bpe", "sentencepiece"], ValueError, "--sentencepiece-model"),
                             (["--constraints", "--constraints-file", "c.tsv"], ValueError, "--constraints-file"),
                             (["--constraints", "--sampling", "--nbest", "5"], ValueError, "mutually exclusive"),
                             (["--nbest", "7"], ValueError, "--nbest")):
        with pytest.raises(exc, match=name):
            cli.interactive_main(["DATA", "--path", "m.pt"] + flags)
    cli.check_interactive_args(parse(["--constraints"]))  # alone it is legal: the phrases come with the lines


@pytest.mark.parametrize("kind,flags,name", [
    ("language_modeling", ["--constraints"], "--constraints"), ("triplet", ["--constraints", "unordered"], "--constraints"),
    ("language_modeling", ["--print-alignment"], "--print-alignment"), ("language_modeling", ["--lm-path", "lm.pt"], "--lm-path")])
def test_refusals_that_need_the_checkpoints_task(monkeypatch, tmp_path, kind, flags, name):
    task = U.lm_task() if kind == "language_modeling" else U.speech_task(tmp_path / "d")

    class Model(torch.nn.Module):
        def to(self, *a, **k):
            pytest.fail("the model was moved to the device before the refusal")

    monkeypatch.setattr(cli.checkpoint_utils, "load_model_ensemble_and_task", lambda *a, **k: ([Model()], Namespace(task=kind), task))
    with pytest.raises((NotImplementedError, ValueError), match=name):
        cli.interactive_main(["DATA", "--path", "m.pt"] + flags)


def test_resolve_max_positions_and_prompt_limit():
    assert cli.resolve_max_positions(1024, 512, None) == 512
    assert cli.resolve_max_positions((2000000, 1024), (None, 200), (6000, 300)) == (6000, 200)
    assert cli.resolve_max_positions(None) is None
    # max_len = min(int(a * (1 + n) + b), positions - 1): a prompt may be exactly max_len long
    assert cli.lm_prompt_limit(4, 0, 4, 1024) and not cli.lm_prompt_limit(5, 0, 4, 1024)
    assert cli.lm_prompt_limit(9, 1.0, 0, 1024) and not cli.lm_prompt_limit(9, 0.5, 0, 1024)
    assert cli.lm_prompt_limit(7, 0, 200, 8) and not cli.lm_prompt_limit(8, 0, 200, 8)


# ---- the four tasks against the reference's batches ---------------------------------------------------------------------------
def run_batches(lines, args, task, max_positions, **kw):
    err = io.StringIO()
    out = list(cli.make_batches(list(lines), args, task, max_positions, lambda x: x, err=err, **kw))
    return out, err.getvalue()


@pytest.mark.parametrize("buf", ["ragged", "one"])
def test_language_modeling_batches(g, buf):
    task = U.lm_task()
    lines = [str(x) for x in g["lm/prompts/" + buf]]
    tokens, lengths = task.get_interactive_tokens_and_lengths(lines, lambda x: x)
    assert lengths == g["lm/%s/lengths" % buf].tolist()
    for i, t in enumerate(tokens):
        assert t.dtype == torch.int64 and t.tolist() == g["lm/%s/tokens/%d" % (buf, i)].tolist()
    batches, err = run_batches(lines, U.batch_args(batch_size=len(lines)), task, 1024, prompt_ok=lambda n: True)
    assert err == "" and len(batches) == int(g["lm/%s/nbatches" % buf])
    for j, (ids, batch, lists) in enumerate(batches):
        key = "lm/%s/batch%d/" % (buf, j)
        assert ids == g[key + "id"].tolist() and lists is None
        assert sorted(batch) == ["id", "net_input", "target"]
        for k in ("src_tokens", "src_lengths"):
            assert batch["net_input"][k].dtype == torch.int64
            np.testing.assert_array_equal(batch["net_input"][k].numpy(), g[key + k])
        np.testing.assert_array_equal(batch["target"].numpy(), g[key + "target"])
    if buf == "ragged":  # eos first, right-padded, rows in input order (this collater does not sort)
        src = batches[0][1]["net_input"]["src_tokens"]
        assert src[:, 0].tolist() == [EOS] * 3 and src[0, 2:].tolist() == [PAD] * 3 and batches[0][0] == [0, 1, 2]


@pytest.mark.parametrize("kind", ["triplet", "speech_to_text"])
@pytest.mark.parametrize("size", [1, 3])
def test_speech_batches(g, tmp_path, kind, size):
    """The lines are audio paths; lengths are waveform samples (use_audio_input); batches by descending length under --max-tokens.
    (speech_to_text builds SpeechToTextDataset over the same paths: the same batches.)"""
    task = U.speech_task(tmp_path / "d", kind)
    lines = [os.path.join(U.DATA_TINY, str(x)) for x in g["st/lines"]]
    paths, n = task.get_interactive_tokens_and_lengths(lines, lambda x: x)
    assert paths == lines and n == g["st/lengths"].tolist()
    ds = task.build_dataset_for_inference(paths, n)
    assert type(ds).__name__ == ("TripletDataset" if kind == "triplet" else "SpeechToTextDataset") and ds.split == "interactive"
    assert not ds.is_train_split and ds.tgt_texts is None
    args = U.batch_args(max_tokens=int(g["st/max_tokens"]))
    start, reordered = 0, False
    for k, keys in U.buffers(g, "st/buf%d" % size):
        batches, err = run_batches(lines[start:start + size], args, task, (2000000, 1024))
        assert err == "" and len(batches) == len(keys)
        for (ids, batch, lists), key in zip(batches, keys):
            assert ids == g[key + "/id"].tolist() and lists is None
            np.testing.assert_array_equal(batch["net_input"]["src_lengths"].numpy(), g[key + "/src_lengths"])
            assert batch["net_input"]["src_tokens"].dtype == torch.float32
            np.testing.assert_array_equal(batch["net_input"]["src_tokens"].numpy(), g[key + "/src_tokens"])
        order = [i for ids, _, _ in batches for i in ids]
        reordered = reordered or order != sorted(order)
        start += size
    assert reordered == (size == 3)  # the buffer of three comes back as [0, 2], [1]: the driver's re-sort is observable


@pytest.mark.parametrize("case", ["plain", "plain_buf1", "constrained"])
def test_translation_batches(g, case):
    lex = import_module("chimera-st_amd.lexical_constraints")
    task = U.mt_task()
    lines = [str(x) for x in g["mt/%s/lines" % case]]
    args = U.batch_args(max_tokens=int(g["mt/max_tokens"]), constraints="ordered" if case == "constrained" else None)
    size, start, reordered = int(g["mt/%s/buffer_size" % case]), 0, False
    for k, keys in U.buffers(g, "mt/" + case):
        batches, err = run_batches(lines[start:start + size], args, task, (1024, 1024))
        assert err == "" and len(batches) == len(keys)
        for (ids, batch, lists), key in zip(batches, keys):
            assert ids == g[key + "/id"].tolist()
            for name in ("src_tokens", "src_lengths"):
                np.testing.assert_array_equal(batch["net_input"][name].numpy(), g[key + "/" + name])
            assert batch["target"] is None and "prev_output_tokens" not in batch["net_input"]
            if case == "constrained":  # the same constraints per row; the reference pads every batch to the buffer's widest row
                want = [lex.unpack_constraints(row) for row in g[key + "/constraints"].tolist()]
                assert lists == want
                packed = lex.pack_constraints(lists, pad=PAD, eos=EOS)
                w = packed.shape[1]
                assert packed.tolist() == g[key + "/constraints"][:, :w].tolist() and not g[key + "/constraints"][:, w:].any()
            else:
                assert lists is None
        order = [i for ids, _, _ in batches for i in ids]
        reordered = reordered or order != sorted(order)
        start += size
    assert reordered == (size > 1)
    if case == "constrained":
        assert any(len(c) == 2 for ids, _, lists in batches for c in lists)


# ---- printing -------------------------------------------------------------------------------------------------------------------
def print_recorded(g, key, src_dict, tgt_dict, text):
    out = io.StringIO()
    args = Namespace(post_process=None, nbest=1, print_alignment=False)
    lex = import_module("chimera-st_amd.lexical_constraints")
    start = 0
    for k, keys in U.buffers(g, key):
        results, n = [], 0
        for bk in keys:
            ids, hyps = g[bk + "/id"].tolist(), U.fixture_hyps(g, bk)
            cons = [lex.unpack_constraints(r) for r in g[bk + "/constraints"].tolist()] if bk + "/constraints" in g else [[] for _ in ids]
            for i, (id_, h) in enumerate(zip(ids, hyps)):
                row = torch.from_numpy(g[bk + "/src_tokens"][i])
                results.append((start + id_, row[row.ne(PAD)] if text else None, h, {"constraints": cons[i], "time": 0.0}))
            n += len(ids)
        cli.print_translations(results, args, src_dict, tgt_dict, lambda x: x, out=out)
        start += n  # (no line of the fixture is skipped: the buffer's size)
    return out.getvalue()


@pytest.mark.parametrize("key", ["st/buf1", "st/buf3", "mt/plain", "mt/plain_buf1", "mt/constrained"])
def test_printed_lines_are_the_recorded_ones_byte_for_byte(g, tmp_path, key):
    """print_translations on the fixture's hypotheses: S-/W-/C- for text sources only, H-/D- with the fp32 score / ln 2 under `{}`,
    P- with %.4f in base 2, the buffer's results in input order, ids running on across buffers."""
    if key.startswith("st/"):
        task = U.speech_task(tmp_path / "d")
        got = print_recorded(g, key, task.source_dictionary, task.target_dictionary, text=False)
        assert "S-" not in got and "W-" not in got
    else:
        task = U.mt_task()
        got = print_recorded(g, key, task.source_dictionary, task.target_dictionary, text=True)
    assert got == str(g[key + "/stdout"])
    assert got.encode("utf-8") == str(g[key + "/stdout"]).encode("utf-8")


def test_nbest_alignment_and_unk_in_the_detokenized_line():
    d = U.word_dictionary()
    hyp = {"tokens": torch.tensor([5, 3, 7, EOS]), "score": torch.tensor(-0.5), "positional_scores": torch.tensor([-0.1, -0.2, -0.3, -1.4]),
           "attention": torch.tensor([[0.9, 0.1, 0.2, 0.5], [0.1, 0.9, 0.8, 0.5]]), "alignment": None}
    worse = dict(hyp, score=torch.tensor(-0.75))
    out = io.StringIO()
    args = Namespace(post_process=None, nbest=2, print_alignment=True)
    n = cli.print_translations([(4, torch.tensor([EOS, 9, 8]), [hyp, worse, worse], {"constraints": [[6, 7]], "time": 0.25})], args, d, d, lambda x: x, out=out)
    lines = out.getvalue().splitlines()
    assert lines[:3] == ["S-4\tw5 w4", "W-4\t0.250\tseconds", "C-4\tw2 w3"]
    assert lines[3] == "H-4\t{}\tw1 <unk> w3".format(float(torch.tensor(-0.5) / np.log(2)))
    assert lines[4].split("\t")[2] == "w1   w3"  # <unk> replaced by a space in the D- line only
    assert lines[5] == "P-4\t-0.1443 -0.2885 -0.4328 -2.0198" and lines[6] == "A-4\t0-0 1-1 1-2"
    assert len(lines) == 11 and lines[7].startswith("H-4\t-1.08") and n == 4  # nbest 2 of 3; the token count is the best one's


# ---- bad lines, empty prompts -----------------------------------------------------------------------------------------------------
def test_a_bad_path_is_named_on_stderr_and_the_buffer_goes_on(g, tmp_path):
    task = U.speech_task(tmp_path / "d")
    good = os.path.join(U.DATA_TINY, "talk_b.wav")
    junk = tmp_path / "junk.wav"
    junk.write_bytes(b"RIFF\x00\x00not a wave file at all")
    mp3 = tmp_path / "speech.mp3"
    mp3.write_bytes(b"\xff\xfb\x90\x00" * 64)
    lines = [good, str(tmp_path / "missing.wav"), str(junk), good, str(mp3), ""]
    batches, err = run_batches(lines, U.batch_args(max_tokens=int(g["st/max_tokens"])), task, (2000000, 1024), start_id=10)
    assert [ids for ids, _, _ in batches] == [[0, 3]]  # positions in the buffer; the bad lines are in no batch
    msgs = err.splitlines()
    assert len(msgs) == 4 and [m.split()[1] for m in msgs] == ["11", "12", "14", "15"]  # ids run on from start_id
    assert "missing.wav" in msgs[0] and "junk.wav" in msgs[1] and all(m.startswith("input ") and "skipped" in m for m in msgs)
    # a buffer of bad lines only yields nothing, and raises nothing
    batches, err = run_batches([str(junk)], U.batch_args(batch_size=1), task, (2000000, 1024))
    assert batches == [] and "input 0 skipped" in err


def test_a_line_beyond_the_positions_raises_unless_skipped(g, tmp_path):
    task = U.speech_task(tmp_path / "d")
    lines = [os.path.join(U.DATA_TINY, str(x)) for x in g["st/lines"][:2]]
    with pytest.raises(Exception, match="--skip-invalid-size-inputs-valid-test"):
        run_batches(lines, U.batch_args(batch_size=1), task, (20000, 1024))
    batches, err = run_batches(lines, U.batch_args(batch_size=1, skip_invalid_size_inputs_valid_test=True), task, (20000, 1024))
    assert [ids for ids, _, _ in batches] == [[1]] and err == ""
    mt = U.mt_task()
    with pytest.raises(Exception, match="--skip-invalid-size-inputs-valid-test"):
        run_batches(["w1 w2 w3 w4", "w1"], U.batch_args(batch_size=2), mt, (3, 1024))


def test_empty_prompts_are_batched_apart_and_long_ones_reported():
    task = U.lm_task()
    lines = ["w1 w2", "", "w3", "w4 w5 w6 w7 w8", "", "w9 w10 w11"]
    ok = lambda n: cli.lm_prompt_limit(n, 0, 4, 1024)
    batches, err = run_batches(lines, U.batch_args(batch_size=6), task, 1024, prompt_ok=ok, start_id=3)
    assert [ids for ids, _, _ in batches] == [[0, 2, 5], [1, 4]]
    full, empty = batches[0][1]["net_input"], batches[1][1]["net_input"]
    assert full["src_tokens"].tolist() == [[EOS, 5, 6, PAD], [EOS, 7, PAD, PAD], [EOS, 13, 14, 15]] and full["src_lengths"].tolist() == [3, 2, 4]
    assert empty["src_tokens"].tolist() == [[EOS], [EOS]] and empty["src_lengths"].tolist() == [1, 1]
    assert err.splitlines() == ["input 6 skipped: a prompt of 5 tokens exceeds the step limit max_len (--max-len-a, --max-len-b, the model's positions)"]
    # the task's inference_step: the prompt batch becomes prefix_tokens without its eos column; an empty batch has no prefix
    seen = []

    class Gen:
        def generate(self, models, sample, prefix_tokens=None, bos_token=None, **kw):
            seen.append((None if prefix_tokens is None else prefix_tokens.tolist(), bos_token))
            return []

    task.inference_step(Gen(), [], {"net_input": full})
    task.inference_step(Gen(), [], {"net_input": empty})
    assert seen == [([[5, 6, PAD], [7, PAD, PAD], [13, 14, 15]], EOS), (None, EOS)]
    with pytest.raises(NotImplementedError, match="Constrained decoding"):
        task.inference_step(Gen(), [], {"net_input": full}, constraints=torch.zeros(3, 1, dtype=torch.long))
