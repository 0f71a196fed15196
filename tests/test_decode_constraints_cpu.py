"""No-GPU checks of the decoding constraints --no-repeat-ngram-size / --prefix-size:
  * the fixture the REAL reference's SequenceGenerator produced (tools/ref_harness/make_decode_constraints_goldens.py ->
    decode_constraints_tiny.npz) does show the constraints at work — the conditions its generator script asserts, re-asserted here;
  * the host loop's tensor forms of the two rules against element-by-element restatements;
  * the generator's argument checks and the two command-line flags;
  * the restatement the GPU kernel test compares with is not vacuous on that test's inputs."""
import ast
import math
from argparse import Namespace
from importlib import import_module

import pytest
import torch

from conftest import load_golden, load_pkg
from decode_constraints_util import CASES, EOS, PAD, VARIANTS, banned_tokens, family, run_restatement


def _hyps(g, name, b):
    return [g["gen/%s/b%d/r%d/tokens" % (name, b, r)].tolist() for r in range(int(g["gen/%s/b%d/n" % (name, b)]))]


def _has_repeated_ngram(tokens, n):
    grams = [tuple(tokens[i:i + n]) for i in range(len(tokens) - n + 1)]
    return len(grams) != len(set(grams))


def _required_start(row):
    out = []
    for t in row:
        if t == PAD:
            break
        out.append(t)
        if t == EOS:
            break
    return out


@pytest.fixture(scope="module")
def fixture():
    g = load_golden("decode_constraints_tiny.npz")
    return g, ast.literal_eval(str(g["meta/settings"])), g["meta/prefix"].tolist()


def test_fixture_blocking_changes_the_best_hypotheses(fixture):
    g, settings, prefix = fixture
    for name in ("ngram2", "ngram3"):
        changed = sum(_hyps(g, name, b)[0] != _hyps(g, settings[name]["base"], b)[0] for b in range(len(prefix)))
        assert changed >= 2, (name, changed)


def test_fixture_has_no_repeated_ngram(fixture):
    g, settings, prefix = fixture
    seen = 0
    for name, kw in settings.items():
        n = kw.get("no_repeat_ngram_size", 0)
        for b in range(len(prefix)):
            for toks in _hyps(g, name, b):
                if n:
                    seen += 1
                    assert not _has_repeated_ngram([EOS] + toks, n), (name, b, toks)  # (the windows start at the initial eos)
    assert seen >= 3 * 4 * 3
    # ... and the baseline of the blocking settings does repeat: the constraint has something to do
    assert all(_has_repeated_ngram(_hyps(g, "base_unfitted", b)[0], 2) for b in range(len(prefix)))


def test_fixture_prefix_hypotheses_start_with_their_prefix(fixture):
    g, settings, prefix = fixture
    assert prefix == [[7, 9, 11], [8, EOS, PAD], [13, PAD, PAD]]
    for name in ("prefix", "prefix_ngram_minlen"):
        assert settings[name]["prefix"]
        for b in range(len(prefix)):
            hyps = _hyps(g, name, b)
            assert len(hyps) == settings[name]["beam_size"]
            for toks in hyps:
                want = _required_start(prefix[b])
                assert toks[:len(want)] == want, (name, b, toks)
        # eos inside the prefix: the first beam is copied over the others — `beam` identical hypotheses
        assert all(t == [8, EOS] for t in _hyps(g, name, 1))
        assert len({float(g["gen/%s/b1/r%d/score" % (name, r)]) for r in range(5)}) == 1
    # min_len 4 is suspended during the prefix steps: [8, eos] (2 tokens) is finalised although min_len is 4
    assert settings["prefix_ngram_minlen"]["min_len"] == 4 and len(_hyps(g, "prefix_ngram_minlen", 1)[0]) == 2
    assert all(len(t) > 4 for b in range(3) for t in _hyps(g, "base_fitted_minlen", b))


def _tiny_model(vocab=40):
    load_pkg()
    s2t = import_module("chimera-st_amd.s2t_transformer")
    tasks = import_module("chimera-st_amd.tasks")
    registry = import_module("chimera-st_amd.registry")
    args = Namespace(arch="s2t_transformer_s", task="speech_to_text", data=None, synthetic_vocab_size=vocab, encoder_embed_dim=32,
                     encoder_ffn_embed_dim=64, encoder_attention_heads=2, decoder_attention_heads=2, encoder_layers=1, decoder_layers=1,
                     dropout=0.0, conv_channels=32, share_decoder_input_output_embed=True)
    registry.ARCH_CONFIG_REGISTRY[args.arch](args)
    torch.manual_seed(vocab)
    task = tasks.SpeechToTextTask(args)
    return s2t.S2TTransformerModel.build_model(args, task), task


def test_generator_argument_checks():
    model, task = _tiny_model()
    SG = import_module("chimera-st_amd.sequence_generator").SequenceGenerator
    d = task.target_dictionary
    with pytest.raises(ValueError, match="eos can never be emitted"):
        SG([model], d, beam_size=2, no_repeat_ngram_size=1)
    with pytest.raises(ValueError, match="at least 2"):
        SG([model], d, beam_size=2, no_repeat_ngram_size=-3)
    assert SG([model], d, beam_size=2, no_repeat_ngram_size=3).no_repeat_ngram_size == 3
    gen = SG([model], d, beam_size=2, max_len_a=0, max_len_b=5)
    sample = {"net_input": {"src_tokens": torch.zeros(2, 50, 80), "src_lengths": torch.tensor([50, 40])}}
    with pytest.raises(ValueError, match="starts with eos or pad"):
        gen.generate([model], sample, prefix_tokens=torch.tensor([[7, 8], [d.eos(), 9]]))
    with pytest.raises(ValueError, match="starts with eos or pad"):
        gen.generate([model], sample, prefix_tokens=torch.tensor([[d.pad(), 8], [7, 9]]))
    with pytest.raises(ValueError, match="step limit max_len is 5"):
        gen.generate([model], sample, prefix_tokens=torch.full((2, 6), 7))
    with pytest.raises(ValueError, match="batch 2"):
        gen.generate([model], sample, prefix_tokens=torch.full((3, 2), 7))


def test_cli_parser_accepts_both_flags():
    load_pkg()
    cli = import_module("chimera-st_amd.cli")
    a = cli.generate_parser().parse_args(["data", "--path", "m.pt"])
    assert a.no_repeat_ngram_size == 0 and a.prefix_size == 0
    a = cli.generate_parser().parse_args(["data", "--path", "m.pt", "--no-repeat-ngram-size", "3", "--prefix-size", "2"])
    assert a.no_repeat_ngram_size == 3 and a.prefix_size == 2
    # the task hands the blocking size to the generator
    model, task = _tiny_model()
    assert task.build_generator([model], Namespace(beam=2, no_repeat_ngram_size=2)).no_repeat_ngram_size == 2
    assert task.build_generator([model], Namespace(beam=2)).no_repeat_ngram_size == 0


@pytest.mark.parametrize("n", [2, 3, 4])
def test_host_loop_ngram_ban_matches_elementwise_rule(n):
    """SequenceGenerator._ban_repeated_ngrams (unfold / scatter_add on the device tensors) against the rule applied token by token."""
    model, task = _tiny_model()
    SG = import_module("chimera-st_amd.sequence_generator").SequenceGenerator
    gen = SG([model], task.target_dictionary, beam_size=2, no_repeat_ngram_size=n)
    g = torch.Generator().manual_seed(n)
    rows, V, LT = 16, 12, 14
    hit = 0
    for step in range(0, LT - 1):
        tokens = torch.full((rows, LT), PAD, dtype=torch.long)
        tokens[:, 0] = EOS
        tokens[:, 1:step + 1] = torch.randint(4, 7, (rows, step), generator=g)  # three symbols: plenty of repeats
        lprobs = torch.randn(rows, V, generator=g)
        lprobs[:, 5] = -math.inf  # an already masked candidate stays masked
        want = lprobs.clone()
        for h in range(rows):
            for t in banned_tokens(tokens[h].tolist(), step, n):
                hit += 1
                want[h, t] = -math.inf
        got = gen._ban_repeated_ngrams(tokens, lprobs.clone(), step)
        assert torch.equal(got, want), step
    assert hit > rows


def test_host_loop_prefix_matches_elementwise_rule():
    model, task = _tiny_model()
    SG = import_module("chimera-st_amd.sequence_generator").SequenceGenerator
    gen = SG([model], task.target_dictionary, beam_size=3)
    g = torch.Generator().manual_seed(3)
    beam, V = 3, 12
    prefix = torch.tensor([[7, 9], [8, EOS], [6, PAD]])
    lprobs = torch.randn(9, V, generator=g)
    tokens = torch.randint(4, V, (9, 5), generator=g)
    scores = torch.randn(9, 4, generator=g)
    lp, tk, sc = gen._force_prefix(1, lprobs.clone(), scores.clone(), tokens.clone(), prefix, beam)
    for r in range(3):  # sentence 0: only token 9 survives, with its own log-probability
        assert float(lp[r, 9]) == float(lprobs[r, 9]) and int(torch.isfinite(lp[r]).sum()) == 1
    for r in range(3, 6):  # sentence 1: eos only, and the first beam's row, tokens and scores everywhere
        assert float(lp[r, EOS]) == float(lprobs[3, EOS]) and int(torch.isfinite(lp[r]).sum()) == 1
        assert torch.equal(tk[r], tokens[3]) and torch.equal(sc[r], scores[3])
    assert torch.equal(lp[6:], lprobs[6:]) and torch.equal(tk[6:], tokens[6:]) and torch.equal(tk[:3], tokens[:3])  # pad: unconstrained


@pytest.mark.parametrize("dtype_name,V,members", CASES)
def test_kernel_test_inputs_make_the_ban_bite(dtype_name, V, members):
    """The restatement ALONE, on the logits the GPU kernel test uses: in the settings with blocking the ban removes a finite candidate
    in at least a quarter of the (row, step) pairs, every sentence finalises `beam` hypotheses, none of which repeats an n-gram."""
    for variant, (n, with_prefix, min_len) in VARIANTS.items():
        if not n:
            continue
        st, frac = run_restatement(dtype_name, V, members, variant)
        assert frac >= 0.25, (variant, frac)
        assert st["finished"].tolist() == [1, 1, 1] and st["nfinal"].tolist() == [4, 4, 4]
        for b in range(3):
            for r in range(4):
                toks = st["fin_tokens"][b, r, :int(st["fin_len"][b, r])].tolist()
                assert toks[-1] == EOS and not _has_repeated_ngram([EOS] + toks, n), (variant, b, r, toks)


def test_cases_cover_every_dispatch_family():
    assert [family(d, V) for d, V, m in CASES] == ["NV1", "NV5", "wide", "NV3", "wide", "NV1", "wide"]
