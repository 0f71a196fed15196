"""fairseq_infer.py without a GPU: parser defaults, the by-name refusals, result files, WER arithmetic, n-best rescoring arithmetic, the
dictionary check, and --load-emissions with the Viterbi decoder on the host route against the numbers the reference recorded in
tests/golden/ctc_tiny.npz."""
import json
import math
import os
from argparse import Namespace
from importlib import import_module

import numpy as np
import pytest
import torch

import wav2vec_ctc_util as U
from conftest import load_pkg


@pytest.fixture(scope="module")
def cli():
    load_pkg()
    return import_module("chimera-st_amd.cli")


@pytest.fixture(scope="module")
def CD():
    load_pkg()
    return import_module("chimera-st_amd.ctc_decoder")


def test_parser_defaults(cli):
    a = cli.check_infer_args(cli.infer_parser().parse_args(["data", "--labels", "ltr", "--path", "m.pt"]))
    assert (a.task, a.criterion, a.w2l_decoder, a.gen_subset) == ("audio_pretraining", "ctc", "viterbi", "test")
    assert (a.beam, a.nbest, a.beam_threshold, a.beam_size_token) == (5, 1, 25.0, 100)
    assert (a.lm_weight, a.word_score, a.sil_weight, a.unk_weight) == (0.2, 1.0, 0.0, -math.inf)
    assert a.post_process == "letter" and a.max_tokens == 4000000 and a.batch_size is None and a.results_path is None
    b = cli.check_infer_args(cli.infer_parser().parse_args(["data", "--labels", "ltr", "--path", "m.pt", "--batch-size", "3", "--remove-bpe", "sentencepiece"]))
    assert b.max_tokens is None and b.batch_size == 3 and b.post_process == "sentencepiece"


@pytest.mark.parametrize("flags,word", [
    (["--w2l-decoder", "kenlm"], "--w2l-decoder beam"), (["--w2l-decoder", "fairseqlm"], "--w2l-decoder beam"),
    (["--lexicon", "lex.txt"], "--lexicon"), (["--sil-weight", "0.5"], "--sil-weight"), (["--unk-weight", "-1"], "--unk-weight"),
    (["--path", "a.pt:b.pt"], "models\\[0\\]"), (["--dump-features", "f"], "--dump-features"), (["--criterion", "asg_loss"], "asg_loss")])
def test_refusals_by_name(cli, flags, word):
    argv = ["data", "--labels", "ltr"] + ([] if "--path" in flags else ["--path", "m.pt"]) + flags
    with pytest.raises(NotImplementedError, match=word):
        cli.check_infer_args(cli.infer_parser().parse_args(argv))


def test_wer_args_stays_refused():
    load_pkg()
    C = import_module("chimera-st_amd.criterions")
    d = U.letter_dictionary(U.fixture())
    with pytest.raises(NotImplementedError, match="--wer-args"):
        C.CtcCriterion(Namespace(target_dictionary=d), wer_args="('lm.bin', 'lex', 2, -1)")


def test_result_file_names_and_lines(cli, tmp_path):
    g = U.fixture()
    d = U.letter_dictionary(g)
    args = Namespace(results_path=str(tmp_path), path="/x/y/checkpoint_best.pt", load_emissions=None, gen_subset="dev", nbest=1,
                     post_process="letter", quiet=True)
    names = cli.infer_result_files(args)
    assert {os.path.basename(v) for v in names.values()} == {"%s-checkpoint_best.pt-dev.txt" % k for k in ("hypo.word", "hypo.units", "ref.word", "ref.units")}
    files = {k: open(v, "w") for k, v in names.items()}
    enc = lambda s: [d.index(c) for c in s.split()]
    hyp, ref = enc("T H E | C A T |"), enc("T H E | C A T S |")
    w_err, w_len, c_err, c_len = cli.process_predictions(args, [{"tokens": torch.tensor(hyp)}, {"tokens": torch.tensor(ref)}], d, ref, files, None, 7)
    for f in files.values():
        f.close()
    assert (w_err, w_len, c_err, c_len) == (1, 2, 1, 9)  # only the top hypothesis is scored
    assert open(names["hypo.units"]).read() == "T H E | C A T | (None-7)\n"
    assert open(names["hypo.word"]).read() == "THE CAT (None-7)\n"
    assert open(names["ref.units"]).read() == "T H E | C A T S | (None-7)\n"
    assert open(names["ref.word"]).read() == "THE CATS (None-7)\n"


def test_word_errors(cli):
    assert cli.word_errors("a b c".split(), "a x c d".split()) == (2, 4)
    assert cli.word_errors([], "a b".split()) == (2, 2)
    assert cli.word_errors("a".split(), []) == (1, 0)


def beam_args(**kw):
    return Namespace(**dict(dict(beam=4, nbest=4, beam_threshold=25.0, beam_size_token=100, lm_weight=0.5, word_score=2.0, post_process="letter"), **kw))


def test_rescoring_arithmetic_and_stable_order(CD):
    d = U.letter_dictionary(U.fixture())
    dec = CD.CtcBeamDecoder(beam_args(), d)
    enc = lambda s: [d.index(c) for c in s.split()]
    hyps = [(enc("A | B |"), -1.0), (enc("A B |"), -1.5), (enc("A |"), -2.0), (enc("B |"), -3.0)]
    lm = [-4.0, -1.0, -2.0, 0.0]  # what a stub language model returns
    out = dec.rescore(hyps, lm)
    want = [-1.0 + 0.5 * -4.0 + 2.0 * 2, -1.5 + 0.5 * -1.0 + 2.0 * 1, -2.0 + 0.5 * -2.0 + 2.0 * 1, -3.0 + 0.0 + 2.0 * 1]
    assert want == [1.0, 0.0, -1.0, -1.0]
    assert [h["score"] for h in out] == [1.0, 0.0, -1.0, -1.0]
    assert [h["tokens"].tolist() for h in out] == [h[0] for h in hyps]  # the tie of the last two keeps the first-pass order
    assert [(h["ctc_score"], h["lm_score"]) for h in out] == [(s, l) for (_, s), l in zip(hyps, lm)]
    flat = CD.CtcBeamDecoder(beam_args(lm_weight=0.0, word_score=0.0), d).rescore(hyps, lm)
    assert [h["tokens"].tolist() for h in flat] == [h[0] for h in hyps] and [h["score"] for h in flat] == [s for _, s in hyps]
    up = CD.CtcBeamDecoder(beam_args(lm_weight=1.0, word_score=0.0), d).rescore(hyps, lm)
    assert [h["tokens"].tolist() for h in up] == [hyps[1][0], hyps[3][0], hyps[2][0], hyps[0][0]]


def test_dictionary_mismatch_raises(CD):
    g = U.fixture()
    d, other = U.letter_dictionary(g), U.letter_dictionary(g)
    CD.check_lm_dictionary(other, d)
    other.symbols[7], other.symbols[8] = other.symbols[8], other.symbols[7]
    with pytest.raises(ValueError, match="symbol 7"):
        CD.check_lm_dictionary(other, d)
    other.add_symbol("#")
    with pytest.raises(ValueError, match="symbols"):
        CD.check_lm_dictionary(other, d)
    with pytest.raises(ValueError, match="--lm-model"):
        CD.CtcBeamDecoder(beam_args(), d, lm_model=object(), lm_dict=other)


def fixture_data(root, g):
    """A `dev` split whose labels are the fixture's targets, and the fixture's logits as an emissions file."""
    d = U.letter_dictionary(g)
    U.write_manifest(root, g, splits=(("dev", 3),))
    with open(os.path.join(root, "dev.ltr"), "w") as f:
        for row, n in zip(g["in/target"], g["in/target_lengths"]):
            f.write(" ".join(d[int(t)] for t in row[:int(n)]) + "\n")
    lp = torch.log_softmax(torch.from_numpy(g["out/logits"]).float(), dim=-1)
    lens = (~g["out/frame_padding_mask"]).sum(1)
    em = np.empty(3, dtype=object)
    for b in range(3):
        em[b] = lp[:int(lens[b]), b].numpy()
    path = os.path.join(root, "emissions.npy")
    np.save(path, em, allow_pickle=True)
    return path


def test_load_emissions_viterbi_host_route_reproduces_the_reference(cli, tmp_path, capsys, monkeypatch):
    g = U.fixture()
    root = str(tmp_path / "data")
    os.makedirs(root)
    em = fixture_data(root, g)
    monkeypatch.setenv("CST_CTC_BEAM", "host")
    out = str(tmp_path / "out")
    task, wer = cli.infer_main([root, "--task", "audio_pretraining", "--labels", "ltr", "--gen-subset", "dev", "--load-emissions", em,
                                "--w2l-decoder", "viterbi", "--results-path", out, "--quiet"])
    lines = capsys.readouterr().out.splitlines()
    ev = [json.loads(l) for l in lines if l.startswith("{")][-1]
    assert wer == 100.0 * int(g["eval/w_errors"]) / int(g["eval/w_total"])
    assert ev["c_errors"] == int(g["eval/c_errors"]) and ev["c_total"] == int(g["eval/c_total"]) and ev["route"] == "host"
    assert "WER: %s" % wer in lines and "| Generate dev with beam=5" in lines
    assert any(l.startswith("| Processed 3 sentences") for l in lines)
    for k in ("hypo.word", "hypo.units", "ref.word", "ref.units"):
        rows = open(os.path.join(out, "%s-emissions.npy-dev.txt" % k)).read().splitlines()
        assert len(rows) == 3 and sorted(r.rsplit(" ", 1)[1] for r in rows) == ["(None-0)", "(None-1)", "(None-2)"]
    # the beam decoder on the host route at beam 1 .. is a search of its own; at least it runs and scores on the same files
    _, wer_b = cli.infer_main([root, "--labels", "ltr", "--gen-subset", "dev", "--load-emissions", em, "--w2l-decoder", "beam", "--beam", "4",
                               "--quiet"])
    assert wer_b is not None
