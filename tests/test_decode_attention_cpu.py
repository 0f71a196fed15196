"""No-GPU checks of hypotheses' attention / --print-alignment:
  * cli.hard_alignment on hand-made matrices: ties to the smallest source index, padded (all-zero) source rows, the eos column dropped;
  * the invariants of tests/golden/decode_attention_tiny.npz (the REAL reference generator over the reference base decoder's attention,
    tools/ref_harness/make_decode_attention_goldens.py): shapes [S, len(tokens)], columns sum to 1 within 1e-6, padded rows exactly 0;
  * the hard-alignment column cap of the GPU tests: they compare hard alignments only in columns whose reference top-2 gap is >= 4e-4
    (four times the 1e-4 probability tolerance: an entry can move by 1e-4, so a gap under 2e-4 could flip the argmax; 4e-4 doubles that),
    and at most 5 % of a case's columns may be left out — asserted on the fixture itself here;
  * nodes_per_step: off = the formula without the feature, on = + 1 per MODEL member, + 2 where the query projection runs inside the
    cross-attention launch, nothing for a language model;
  * `attention` is the engine's keyword (like `lexical`): DecodeOptions and a zero-filled cst_beam_desc tail are what they were, the
    generator hands return_attention to the engine it builds; the command line refuses --score-reference with --print-alignment."""
import dataclasses
from importlib import import_module

import numpy as np
import pytest
import torch

from conftest import load_golden, load_pkg
from test_decode_plan_cpu import BENCH_ROW, BF16, F32, FP32_ROW, FUSED_ROW, SWITCHES, _dec, _Dict

GAP, CAP = 4e-4, 0.05
CASES = {"chimera": [("a", 1), ("a", 5), ("b", 1), ("b", 5)], "ens2": [("a", 5), ("b", 5)], "padded": [("x", 5)]}
PAD, EOS = 1, 2


def fixture_hyps(g, case, tag, beam):
    """[(sentence, rank, tokens, score, attention [S, n])] of one (case, utterance set, beam) of the fixture, every finalised hypothesis."""
    out, b = [], 0
    while "%s/%s/beam%d/b%d/n" % (case, tag, beam, b) in g:
        for r in range(int(g["%s/%s/beam%d/b%d/n" % (case, tag, beam, b)])):
            key = "%s/%s/beam%d/b%d/r%d/" % (case, tag, beam, b, r)
            out.append((b, r, g[key + "tokens"], float(g[key + "score"]), g[key + "attention"]))
        b += 1
    assert out, (case, tag, beam)
    return out


def admitted_columns(att):
    """bool [n]: the columns of a reference attention matrix whose two largest entries are at least GAP apart."""
    if att.shape[0] < 2:
        return np.ones(att.shape[1], dtype=bool)
    top = np.sort(att, axis=0)[-2:]
    return (top[1] - top[0]) >= GAP


@pytest.fixture(scope="module")
def cli():
    load_pkg()
    return import_module("chimera-st_amd.cli")


def test_hard_alignment_ties_padding_and_eos(cli):
    att = torch.tensor([[0.50, 0.20, 0.10, 0.30],
                        [0.50, 0.70, 0.10, 0.30],
                        [0.00, 0.10, 0.80, 0.40],
                        [0.00, 0.00, 0.00, 0.00]])  # (a padded source row: exactly 0)
    toks = [7, 9, 11, EOS]
    assert cli.hard_alignment(att, toks, PAD, EOS) == [(0, 0), (1, 1), (2, 2)]  # tie -> the smallest index; the eos column is dropped
    assert cli.hard_alignment(att.numpy(), torch.tensor(toks), PAD, EOS) == [(0, 0), (1, 1), (2, 2)]
    assert cli.hard_alignment(att[:, 3:], [EOS], PAD, EOS) == []
    assert cli.hard_alignment(torch.zeros(3, 2), [5, EOS], PAD, EOS) == [(0, 0)]  # an all-zero column: index 0
    assert cli.hard_alignment(att, [7, PAD, 11, EOS], PAD, EOS) == [(0, 0), (2, 2)]
    one = torch.tensor([[1.0, 1.0]])
    assert cli.hard_alignment(one, [4, EOS], PAD, EOS) == [(0, 0)]
    with pytest.raises(ValueError, match="does not match"):
        cli.hard_alignment(att, toks[:3], PAD, EOS)


def test_fixture_invariants_and_column_cap():
    g = load_golden("decode_attention_tiny.npz")
    assert float(g["meta/gap"]) == GAP and int(g["meta/max_len_b"]) == 12
    for case, sets in CASES.items():
        cols = left_out = 0
        for tag, beam in sets:
            B = g["in/%s/%s/src_tokens" % (case, tag)].shape[0]
            hyps = fixture_hyps(g, case, tag, beam)
            assert sorted({b for b, *_ in hyps}) == list(range(B))
            for b, r, tokens, score, att in hyps:
                assert att.dtype == np.float32 and att.ndim == 2 and att.shape[1] == len(tokens) and tokens[-1] == EOS, (case, tag, beam, b, r)
                assert np.abs(att.astype(np.float64).sum(0) - 1.0).max() <= 1e-6
                assert (att >= 0).all()
                if case == "padded":
                    valid = int(g["padded/x/b%d/src_valid" % b])
                    assert att.shape[0] == 23 and valid == (23, 19, 11)[b]
                    assert (att[valid:] == 0).all(), "padded source rows must be exactly 0"
                else:
                    assert att.shape[0] == 8  # the memory slots
                ok = admitted_columns(att)
                cols, left_out = cols + ok.size, left_out + int((~ok).sum())
        print("%s: %d columns, %d left out of the hard-alignment comparison (%.1f %%)" % (case, cols, left_out, 100.0 * left_out / cols))
        assert left_out <= CAP * cols, (case, left_out, cols)


@pytest.fixture
def E(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    load_pkg()
    return import_module("chimera-st_amd.decode_engine")


def _engines(E, decs, beam, lm=None, **opts):
    return [E.BeamDecodeEngine(decs, _Dict(), E.DecodeOptions(beam=beam, max_len=20, **opts), lm_decoder=lm, attention=a) for a in (False, True)]


@pytest.mark.parametrize("dtype,dims,beam,rows,off,extra", [
    (F32, FP32_ROW, 4, 20, 27, 1),
    (BF16, FUSED_ROW, 4, 20, 19, 2),                 # the query projection inside the cross-attention launch: + the projection
    (BF16, (512, 32, 2048, 2), 4, 20, 21, 1),        # head dim 32: the projection is a launch of its own already
    (BF16, BENCH_ROW, 5, 160, 53, 2),
])
def test_nodes_per_step_with_attention(E, dtype, dims, beam, rows, off, extra):
    e_off, e_on = _engines(E, [_dec(*dims)], beam)
    assert e_off.attention is False and e_on.attention is True
    assert E.BeamDecodeEngine([_dec(*dims)], _Dict(), E.DecodeOptions(beam=beam, max_len=20)).attention is False  # off by default
    assert e_off.nodes_per_step(dtype, rows) == off  # today's figure (test_decode_plan_cpu.SINGLE)
    assert e_on.nodes_per_step(dtype, rows) == off + extra
    assert extra == 1 + e_on._plan(e_on.decs[0], dtype, rows).q_in_cross


def test_nodes_per_step_of_ensembles_and_language_models(E):
    off, on = _engines(E, [_dec(*FP32_ROW), _dec(*FP32_ROW)], 4)
    assert off.nodes_per_step(F32, 20) == 52 and on.nodes_per_step(F32, 20) == 54
    lm = _dec(512, 64, 2048, 3, cross=False)
    off, on = _engines(E, [_dec(*FUSED_ROW)], 4, lm=lm, lm_weight=0.5)
    assert off.nodes_per_step(BF16, 20) == 37 and on.nodes_per_step(BF16, 20) == 39  # the language model adds nothing


def test_descriptor_tail_and_options_are_unchanged_when_off(E):
    """The feature adds one tail field to cst_beam_desc and nothing to DecodeOptions: fill() leaves the pointer null (the engine's state
    allocation sets it, only with attention on)."""
    assert "attention" not in [f.name for f in dataclasses.fields(E.DecodeOptions)]
    BeamDesc = import_module("chimera-st_amd.lib").BeamDesc
    d = BeamDesc()
    E.DecodeOptions(beam=4, max_len=20).fill(d, 1)
    assert not d.fin_anc and BeamDesc._fields_[-1][0] == "fin_anc"


def test_cli_refuses_score_reference_with_print_alignment(cli):
    p = cli.generate_parser()
    assert p.parse_args(["d", "--path", "m.pt"]).print_alignment is False
    args = p.parse_args(["d", "--path", "m.pt", "--print-alignment", "--score-reference"])
    with pytest.raises(ValueError, match="--print-alignment cannot be combined with --score-reference"):
        cli.check_generate_args(args)
    assert cli.check_generate_args(p.parse_args(["d", "--path", "m.pt", "--print-alignment", "--nbest", "2"])).print_alignment is True


def test_generator_takes_return_attention():
    from test_decode_constraints_cpu import _tiny_model
    from argparse import Namespace
    SG = import_module("chimera-st_amd.sequence_generator").SequenceGenerator
    tiny, task = _tiny_model()
    assert SG([tiny], task.target_dictionary, beam_size=2).return_attention is False
    gen = SG([tiny], task.target_dictionary, beam_size=2, return_attention=True)
    assert gen.return_attention is True and gen.options == SG([tiny], task.target_dictionary, beam_size=2).options
    assert task.build_generator([tiny], Namespace(beam=3, print_alignment=True)).return_attention is True
    assert task.build_generator([tiny], Namespace(beam=3)).return_attention is False
