"""No-GPU checks of checkpoint-ensemble decoding (`--path a.pt:b.pt:c.pt`): the fixture the REAL reference's SequenceGenerator
produced for 2- and 3-member ensembles (tools/ref_harness/make_decode_ensemble_goldens.py -> decode_ensemble_tiny.npz) is
reproduced by the CPU oracle with the averaging rule restated here, and members with different dictionaries are refused."""
import ast
import math
import os
from argparse import Namespace
from importlib import import_module

import pytest
import torch

from conftest import golden_cfg, golden_params, load_golden, load_pkg
from oracle import chimera_oracle as O

SETTINGS = {"beam5": dict(beam=5), "recipe": dict(beam=10, len_penalty=1.5), "temp": dict(beam=5, temperature=0.7)}


def member_params(g, ens, k):
    """Member 0 = decode_tiny.npz; members 1, 2 = member 0 with the tensors the ensemble fixture stores (float16-exact values)."""
    p = golden_params(g)
    if k > 0:
        pre = "member%d/param/" % k
        stored = {n[len(pre):]: torch.from_numpy(v).float() for n, v in ens.items() if n.startswith(pre)}
        assert stored and all(n in p and p[n].shape == v.shape for n, v in stored.items())
        p.update(stored)
    return p


def test_fixture_settings_are_the_ones_tested():
    ens = load_golden("decode_ensemble_tiny.npz")
    assert ast.literal_eval(str(ens["meta/settings"])) == {
        n: {("beam_size" if k == "beam" else k): v for k, v in kw.items()} for n, kw in SETTINGS.items()}


@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("name", sorted(SETTINGS))
@pytest.mark.parametrize("tag", ["a", "b"])
def test_oracle_reproduces_reference_ensemble(N, name, tag):
    """logprob_fn = logsumexp_n(log_softmax(decoder_n(...)[:, -1].float() / T)) - log N over the oracle's decoder (nothing under
    oracle/ knows about ensembles) through oracle.beam_search_with: EVERY finalized hypothesis of the reference's EnsembleModel
    search, in its order — token ids exact, scores to 1e-4 (the bar of test_final_decoding_recipe_matches_reference_generator)."""
    g, rec, ens = load_golden("decode_tiny.npz"), load_golden("decode_recipe_tiny.npz"), load_golden("decode_ensemble_tiny.npz")
    cfg = golden_cfg(g)
    kw = dict(SETTINGS[name])
    T = kw.pop("temperature", 1.0)
    beam = kw["beam"]
    src, lens = torch.from_numpy(rec["in/%s/src_tokens" % tag]), torch.from_numpy(rec["in/%s/src_lengths" % tag])
    params = [member_params(g, ens, k) for k in range(N)]
    with torch.no_grad():
        mems = [O.chimera_encoder(p, src, lens, cfg)[0] for p in params]
    B = mems[0].size(1)

    def logprob_fn(b, tokens):
        lps = []
        for p, mem in zip(params, mems):
            e = mem[:, b:b + 1].repeat(1, beam, 1)
            with torch.no_grad():
                logits = O.decoder(p, tokens, e, torch.zeros(beam, e.size(0), dtype=torch.bool), cfg)
            lps.append(torch.log_softmax(logits[:, -1].float() / T, dim=-1))
        return torch.logsumexp(torch.stack(lps, 0), 0) - math.log(N)

    hyps = O.beam_search_with(logprob_fn, B, max_len=int(ens["meta/max_len_b"]), **kw)
    for b in range(B):
        n = int(ens["n%d/gen/%s/%s/b%d/n" % (N, name, tag, b)])
        assert len(hyps[b]) == n
        for r in range(n):
            key = "n%d/gen/%s/%s/b%d/r%d/" % (N, name, tag, b, r)
            assert hyps[b][r]["tokens"].tolist() == ens[key + "tokens"].tolist(), key
            assert abs(hyps[b][r]["score"] - float(ens[key + "score"])) < 1e-4, key
            assert float((hyps[b][r]["positional_scores"] - torch.from_numpy(ens[key + "pos_scores"])).abs().max()) < 1e-3, key


def test_fixture_is_not_reproduced_by_the_first_member_alone():
    """What the fixture is for: decoding only the first file of --path must NOT pass.  For each N some best hypothesis of the
    ensemble differs in token ids from the best hypothesis of member 0 decoded alone by the reference (own/...)."""
    ens = load_golden("decode_ensemble_tiny.npz")
    for N in (2, 3):
        differs = 0
        for name in SETTINGS:
            for tag, B in (("a", 2), ("b", 3)):
                for b in range(B):
                    differs += ens["n%d/gen/%s/%s/b%d/r0/tokens" % (N, name, tag, b)].tolist() != ens["own/gen/%s/%s/b%d/r0/tokens" % (name, tag, b)].tolist()
        assert differs > 0, N


def _write_checkpoint(path, vocab):
    load_pkg()
    s2t = import_module("chimera-st_amd.s2t_transformer")
    tasks = import_module("chimera-st_amd.tasks")
    registry = import_module("chimera-st_amd.registry")
    cu = import_module("chimera-st_amd.checkpoint_utils")
    args = Namespace(arch="s2t_transformer_s", task="speech_to_text", data=None, synthetic_vocab_size=vocab, encoder_embed_dim=32,
                     encoder_ffn_embed_dim=64, encoder_attention_heads=2, decoder_attention_heads=2, encoder_layers=1, decoder_layers=1,
                     dropout=0.0, conv_channels=32, share_decoder_input_output_embed=True, no_save_optimizer_state=True)
    registry.ARCH_CONFIG_REGISTRY[args.arch](args)
    torch.manual_seed(vocab)
    task = tasks.SpeechToTextTask(args)
    model = s2t.S2TTransformerModel.build_model(args, task)
    cu.save_state(path, args, model.state_dict(), None, None, 0)
    return model, task


def test_members_with_different_dictionaries_raise(tmp_path):
    a, b, c = (os.path.join(str(tmp_path), n) for n in ("a.pt", "b.pt", "c.pt"))
    _write_checkpoint(a, 40)
    _write_checkpoint(b, 40)
    _write_checkpoint(c, 44)
    cu = import_module("chimera-st_amd.checkpoint_utils")
    models, _, task = cu.load_model_ensemble_and_task([a, b])
    assert len(models) == 2 and len(task.target_dictionary) == 40
    with pytest.raises(ValueError, match="share the target dictionary") as ei:
        cu.load_model_ensemble_and_task([a, c])
    assert "a.pt" in str(ei.value) and "c.pt" in str(ei.value)
    # the generator refuses such a list as well (models handed over directly, no files)
    SG = import_module("chimera-st_amd.sequence_generator").SequenceGenerator
    other, _ = _write_checkpoint(c, 44)
    with pytest.raises(ValueError, match="share the target dictionary"):
        SG([models[0], other], task.target_dictionary, beam_size=2)
