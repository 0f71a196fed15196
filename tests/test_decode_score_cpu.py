"""No-GPU checks of --score-reference (sequence_scorer.py, tasks.build_generator, cli.generate_parser, include/cst.h ABI 13): the
plain-torch scorer against the fixture the REAL reference's SequenceScorer produced (decode_score_tiny.npz), the fp64 restatement and
its derived bound (tests/score_ref.py) — which must hold for a faithful fp32 evaluation and reject every listed defect."""
import os
import re
from argparse import Namespace
from importlib import import_module

import pytest
import torch

from conftest import ROOT, load_golden, load_pkg
from score_ref import SCORE_DEFECTS, score_check, score_emulate32, score_inputs, score_ref64

PAD = 1


@pytest.fixture(scope="module")
def SS():
    load_pkg()
    return import_module("chimera-st_amd.sequence_scorer")


@pytest.fixture(scope="module")
def fix():
    return load_golden("decode_score_tiny.npz")


def fixture_batch(fix, tag, N):
    logits = [torch.from_numpy(fix["%s/logits/m%d" % (tag, k)]) for k in range(N)]
    return logits, torch.from_numpy(fix["%s/target" % tag])


@pytest.mark.parametrize("N", [1, 2, 3])
@pytest.mark.parametrize("tag", ["a", "b"])
def test_torch_scorer_reproduces_the_reference(SS, fix, tag, N):
    logits, target = fixture_batch(fix, tag, N)
    assert bool(target.eq(PAD).any())
    pos, score, length = SS.score_tokens_torch(logits, target, PAD)
    assert length.tolist() == fix["n%d/%s/len" % (N, tag)].tolist()
    assert float((pos - torch.from_numpy(fix["n%d/%s/pos_scores" % (N, tag)])).abs().max()) < 1e-4
    assert float((score - torch.from_numpy(fix["n%d/%s/score" % (N, tag)])).abs().max()) < 1e-4


@pytest.mark.parametrize("N", [1, 2, 3])
def test_restatement_agrees_with_the_reference_fixture(fix, N):
    """The fp64 restatement is the definition the kernel is held to: it must be the reference's number too."""
    for tag in ("a", "b"):
        logits, target = fixture_batch(fix, tag, N)
        r = score_ref64(logits, target, PAD)
        assert float((r["pos"] - torch.from_numpy(fix["n%d/%s/pos_scores" % (N, tag)]).double()).abs().max()) < 1e-4
        assert float((r["score"] - torch.from_numpy(fix["n%d/%s/score" % (N, tag)]).double()).abs().max()) < 1e-4


CASES = [(3, 7, 257, 1, torch.float32), (3, 7, 257, 3, torch.float32), (3, 7, 63, 2, torch.bfloat16), (3, 7, 10000, 3, torch.bfloat16),
         (1, 1, 5, 1, torch.float32), (3, 7, 64, 8, torch.bfloat16)]


@pytest.mark.parametrize("B,T,V,N,dtype", CASES)
def test_bound_holds_for_the_torch_scorer_and_the_emulation(SS, B, T, V, N, dtype):
    xs, t = score_inputs(B, T, V, N, dtype)
    r = score_ref64(xs, t, PAD)
    for name, got in (("torch", SS.score_tokens_torch(xs, t, PAD)), ("emulation", score_emulate32(xs, t, PAD))):
        (rp, bp), (rs, bs), exact = score_check(*got, r, dtype)
        print("%s B%d T%d V%d N%d %s: worst pos ratio %.3f, worst score ratio %.3f" % (name, B, T, V, N, dtype, rp, rs))
        assert bp == 0 and bs == 0 and exact, (name, rp, rs)


@pytest.mark.parametrize("defect", SCORE_DEFECTS)
def test_bound_rejects_defect(defect):
    """Each defect, emulated in fp32, must leave elements over the bound.  no_max_subtraction: one member, logits offset by +100 (every
    exponential overflows); mean_of_logprobs: three members; divide_by_T / pad_counted: one member, padded sentences."""
    N = 3 if defect == "mean_of_logprobs" else 1
    xs, t = score_inputs(3, 7, 257, N, torch.float32, offsets=(100.0,) if defect == "no_max_subtraction" else (0.0, 80.0, -80.0))
    r = score_ref64(xs, t, PAD)
    (_, bp), (_, bs), _ = score_check(*score_emulate32(xs, t, PAD), r, torch.float32)
    assert bp == 0 and bs == 0, "the faithful emulation must pass on these inputs"
    (rp, bp), (rs, bs), _ = score_check(*score_emulate32(xs, t, PAD, defect=defect), r, torch.float32)
    print(defect, "pos ratio %.3g (%d over), score ratio %.3g (%d over)" % (rp, bp, rs, bs))
    assert bs > 0 if defect == "divide_by_T" else bp > 0


def test_parser_and_task_select_the_scorer(SS):
    cli = import_module("chimera-st_amd.cli")
    tasks = import_module("chimera-st_amd.tasks")
    args = cli.generate_parser().parse_args(["data", "--path", "x.pt", "--score-reference", "--beam", "4", "--nbest", "3"])
    assert args.score_reference is True
    assert cli.generate_parser().parse_args(["data", "--path", "x.pt"]).score_reference is False
    task = tasks.TripletTask(Namespace(data=None, synthetic_vocab_size=40))
    gen = task.build_generator([], args)
    assert isinstance(gen, SS.SequenceScorer) and gen.pad == task.target_dictionary.pad() and gen.fused
    with pytest.raises(ValueError, match="target"):
        gen.generate([], {"net_input": {}})


def test_header_declares_the_entry_and_abi_13():
    src = open(os.path.join(ROOT, "include", "cst.h")).read()
    assert re.search(r"#define CST_ABI_VERSION 13\b", src)
    assert re.search(r"\bint cst_score_tokens\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    load_pkg()
    L = import_module("chimera-st_amd.lib")
    assert L.ABI_VERSION == 13 and "cst_score_tokens" in {n for n, _, _ in L.SYMBOLS}
