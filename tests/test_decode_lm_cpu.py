"""No-GPU checks of shallow fusion with a target-side language model (--lm-path / --lm-weight): the C ABI of cst_beam_step_lm, the
command line, the transformer_lm mirror, the fixture the REAL reference's SequenceGenerator(lm_model=..., lm_weight=...) produced
(tools/ref_harness/make_decode_lm_goldens.py -> decode_lm_tiny.npz) reproduced by the plain-torch restatement, and the CPU side of
the kernel tests' bounds and seeds (tests/lm_fusion_util.py)."""
import ast
import math
import os
import re
from argparse import Namespace
from importlib import import_module

import pytest
import torch

import lm_fusion_util as U
from conftest import ROOT, golden_cfg, golden_params, load_golden, load_pkg
from oracle import chimera_oracle as O

SETTINGS = {"beam5": dict(beam_size=5, lm_weight=0.3), "recipe": dict(beam_size=10, len_penalty=1.5, lm_weight=0.5),
            "temp": dict(beam_size=5, temperature=0.7, lm_weight=0.3), "ngram2": dict(beam_size=5, lm_weight=0.3, no_repeat_ngram_size=2),
            "ens2": dict(beam_size=5, lm_weight=0.3, members=2)}


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_fusion_entry_and_the_version_stays_13():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cst.h")).read(), flags=re.S)
    assert re.search(r"int\s+cst_beam_step_lm\s*\(\s*const\s+cst_beam_desc\s*\*\s*\w+\s*,\s*const\s+cst_lm_fusion_desc\s*\*\s*\w+\s*,\s*cst_stream\s+\w+\s*\)\s*;", src)
    body = dict((n, b) for b, n in re.findall(r"typedef struct \{([^{}]*)\} (\w+);", src))["cst_lm_fusion_desc"]
    names = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", decl)[-1] for decl in body.split(";") if decl.strip()]
    lib = load_pkg().lib
    assert names == [f[0] for f in lib.LmFusionDesc._fields_] == ["lm_logits", "lm_weight", "lprobs_out"]
    assert re.search(r"#define\s+CST_ABI_VERSION\s+13\b", src) and lib.ABI_VERSION == 13
    assert "cst_beam_step_lm" in {s[0] for s in lib.SYMBOLS}


# ---- the command line ------------------------------------------------------------------------------------------------------------
def test_parser_accepts_the_flags_and_refuses_the_bad_combinations():
    load_pkg()
    cli = import_module("chimera-st_amd.cli")
    base = ["data", "--path", "m.pt"]
    parse = lambda extra: cli.check_generate_args(cli.generate_parser().parse_args(base + extra))
    a = parse([])
    assert a.lm_path is None and a.lm_weight == 0.0
    a = parse(["--lm-path", "lm.pt", "--lm-weight", "0.3"])
    assert a.lm_path == "lm.pt" and a.lm_weight == 0.3
    assert parse(["--lm-path", "lm.pt"]).lm_weight == 0.0
    with pytest.raises(ValueError, match="--lm-weight requires --lm-path"):
        parse(["--lm-weight", "0.3"])
    with pytest.raises(ValueError, match="--score-reference"):
        parse(["--lm-path", "lm.pt", "--score-reference"])


def _fixture_lm():
    """The fixture's LM as a model of this package (CPU, fp32), its args, and the dictionary."""
    load_pkg()
    TL = import_module("chimera-st_amd.transformer_lm")
    Dictionary = import_module("chimera-st_amd.dictionary").Dictionary
    cu = import_module("chimera-st_amd.checkpoint_utils")
    g = load_golden("decode_lm_tiny.npz")
    args = Namespace(**ast.literal_eval(str(g["meta/lm_args"])))
    sd = {k[len("lm/param/"):]: torch.from_numpy(v).float() for k, v in g.items() if k.startswith("lm/param/")}
    d = Dictionary.synthetic(sd["decoder.embed_tokens.weight"].shape[0])
    model = TL.TransformerLanguageModel.build_model(args, cu._DictTask(d))
    return model, sd, args, d, g


def test_language_model_loads_the_fixture_strictly_with_the_reference_keys():
    model, sd, args, d, g = _fixture_lm()
    own = model.state_dict()
    ref_keys = set(str(k) for k in g["meta/lm_keys"].tolist())
    assert set(own.keys()) == ref_keys, sorted(set(own.keys()) ^ ref_keys)
    stored = dict(sd)
    for k in ref_keys - set(stored):  # what the fixture does not store: the buffers
        assert "_float_tensor" in k or k == "decoder.version", k
        stored[k] = own[k]
    model.load_state_dict(stored, strict=True)
    assert all(l.encoder_attn is None and l.normalize_before for l in model.decoder.layers) and model.decoder.layer_norm is not None
    assert model.decoder.output_projection.weight is model.decoder.embed_tokens.weight  # tied, like the reference's
    registry = import_module("chimera-st_amd.registry")
    for arch, (layers, width) in {"transformer_lm": (6, 512), "transformer_lm_big": (12, 1024), "transformer_lm_gpt": (12, 768),
                                  "transformer_lm_gpt2_small": (24, 1024)}.items():
        a = Namespace()
        registry.ARCH_CONFIG_REGISTRY[arch](a)
        assert (a.decoder_layers, a.decoder_embed_dim) == (layers, width) and a.decoder_normalize_before
    TL = import_module("chimera-st_amd.transformer_lm")
    cu = import_module("chimera-st_amd.checkpoint_utils")
    for flag, kw in (("--adaptive-input", dict(adaptive_input=True)), ("--adaptive-softmax-cutoff", dict(adaptive_softmax_cutoff="10,20")),
                     ("--character-embeddings", dict(character_embeddings=True)), ("--decoder-learned-pos", dict(decoder_learned_pos=True))):
        with pytest.raises(NotImplementedError, match=flag):
            TL.TransformerLanguageModel.build_model(Namespace(**dict(vars(args), **kw)), cu._DictTask(d))


def test_load_language_model_checks_the_vocabulary(tmp_path):
    model, sd, args, d, g = _fixture_lm()
    cu = import_module("chimera-st_amd.checkpoint_utils")
    Dictionary = import_module("chimera-st_amd.dictionary").Dictionary
    path = str(tmp_path / "lm.pt")
    a = Namespace(**vars(args))
    a.no_save_optimizer_state = True
    cu.save_state(path, a, model.state_dict(), None, None, 0)
    lm = cu.load_language_model(path, d)
    assert type(lm).__name__ == "TransformerLanguageModel" and not lm.training
    with pytest.raises(ValueError, match=r"60 symbols.*64") as ei:
        cu.load_language_model(path, Dictionary.synthetic(64))
    assert "target dictionary" in str(ei.value)
    # the generator refuses such a model as well, and build_generator hands the LM through
    SG = import_module("chimera-st_amd.sequence_generator").SequenceGenerator
    from test_decode_constraints_cpu import _tiny_model
    tiny, task = _tiny_model()
    if len(task.target_dictionary) != 60:
        with pytest.raises(ValueError, match="target dictionary"):
            SG([tiny], task.target_dictionary, beam_size=2, lm_model=lm, lm_weight=0.3)
    gen = task.build_generator([tiny], Namespace(beam=3), extra_gen_cls_kwargs={"lm_model": None, "lm_weight": 0.25})
    assert gen.lm_model is None and gen.lm_weight == 0.25
    assert SG([tiny], task.target_dictionary, beam_size=2).lm_weight == 1.0  # the reference's default


# ---- the fixture -----------------------------------------------------------------------------------------------------------------------
def test_fixture_settings_are_the_ones_tested():
    g = load_golden("decode_lm_tiny.npz")
    assert ast.literal_eval(str(g["meta/settings"])) == SETTINGS


def _member_params(g, ens, k):
    p = golden_params(g)
    pre = "member%d/param/" % k
    p.update({n[len(pre):]: torch.from_numpy(v).float() for n, v in ens.items() if n.startswith(pre)})
    return p


def _restate(name, tag, lm_mode="fused"):
    """The fixture's setting `name` on input `tag` through lm_fusion_util.search over the oracle's decoder and lm_forward.
    lm_mode: "fused" (the reference's rule), "none" (no LM), "tempered" (the LM divided by the temperature too)."""
    g, rec, ens, fx = (load_golden(f) for f in ("decode_tiny.npz", "decode_recipe_tiny.npz", "decode_ensemble_tiny.npz", "decode_lm_tiny.npz"))
    cfg = golden_cfg(g)
    kw = dict(SETTINGS[name])
    N, w, T, beam = kw.pop("members", 1), kw.pop("lm_weight"), kw.pop("temperature", 1.0), kw.pop("beam_size")
    src, lens = torch.from_numpy(rec["in/%s/src_tokens" % tag]), torch.from_numpy(rec["in/%s/src_lengths" % tag])
    params = [_member_params(g, ens, k) for k in range(N)]
    lmp = {k[len("lm/param/"):]: torch.from_numpy(v).float() for k, v in fx.items() if k.startswith("lm/param/")}
    la = ast.literal_eval(str(fx["meta/lm_args"]))
    with torch.no_grad():
        mems = [O.chimera_encoder(p, src, lens, cfg)[0] for p in params]

    def lp_fn(b, tokens):
        lps = []
        with torch.no_grad():
            for p, mem in zip(params, mems):
                e = mem[:, b:b + 1].repeat(1, beam, 1)
                logits = O.decoder(p, tokens, e, torch.zeros(beam, e.size(0), dtype=torch.bool), cfg)
                lps.append(torch.log_softmax(logits[:, -1].float() / T, dim=-1))
            lp = lps[0] if N == 1 else torch.logsumexp(torch.stack(lps, 0), 0) - math.log(N)
            if lm_mode == "none":
                return lp
            lm = U.lm_forward(lmp, tokens, la["decoder_attention_heads"], la["decoder_layers"])[:, -1].float()
            return lp + torch.log_softmax(lm / (T if lm_mode == "tempered" else 1.0), dim=-1) * w

    hyps, gap = U.search(lp_fn, mems[0].size(1), beam, int(fx["meta/max_len_b"]), len_penalty=kw.get("len_penalty", 1.0),
                         ngram=kw.get("no_repeat_ngram_size", 0))
    return hyps, gap, fx


def _mismatch(hyps, fx, name, tag):
    """Largest score difference to the fixture, inf where the ids or the counts differ."""
    worst = 0.0
    for b in range(len(hyps)):
        n = int(fx["gen/%s/%s/b%d/n" % (name, tag, b)])
        if len(hyps[b]) != n:
            return math.inf
        for r in range(n):
            key = "gen/%s/%s/b%d/r%d/" % (name, tag, b, r)
            if hyps[b][r]["tokens"].tolist() != fx[key + "tokens"].tolist():
                return math.inf
            worst = max(worst, abs(hyps[b][r]["score"] - float(fx[key + "score"])))
            worst = max(worst, 0.1 * float((hyps[b][r]["positional_scores"] - torch.from_numpy(fx[key + "pos_scores"])).abs().max()))
    return worst


@pytest.mark.parametrize("name", sorted(SETTINGS))
@pytest.mark.parametrize("tag", ["a", "b"])
def test_restatement_reproduces_the_reference(name, tag):
    """EVERY finalized hypothesis of the reference's fused search, in its order: ids exact, scores to 1e-4, positional scores to 1e-3;
    the top-2*beam boundary gap of every step is above 1e-4."""
    hyps, gap, fx = _restate(name, tag)
    assert gap > 1e-4
    assert _mismatch(hyps, fx, name, tag) < 1e-4


def test_fixture_is_not_reproduced_without_the_lm_or_with_a_tempered_lm():
    differs = 0
    fx = load_golden("decode_lm_tiny.npz")
    for name in SETTINGS:
        for tag, B in (("a", 2), ("b", 3)):
            for b in range(B):
                differs += fx["gen/%s/%s/b%d/r0/tokens" % (name, tag, b)].tolist() != fx["own/gen/%s/%s/b%d/r0/tokens" % (name, tag, b)].tolist()
    assert differs > 0, "the reference's own un-fused decode has the fixture's best hypotheses"
    for tag in ("a", "b"):
        assert not _mismatch(_restate("beam5", tag, "none")[0], fx, "beam5", tag) < 1e-4
        assert not _mismatch(_restate("temp", tag, "tempered")[0], fx, "temp", tag) < 1e-4


# ---- the CPU side of the kernel tests ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,T,dt", U.KERNEL_CASES)
def test_fp32_torch_error_of_the_fused_lprobs_stays_below_the_cap(N, T, dt):
    """The bound of the per-element kernel test is min(4 x this error, CAP): the fp32 torch evaluation of lp' against fp64 on the
    stored inputs (160 x 10 000, w = 0.5) stays below the cap in every case, so the bound is never looser than 4 x a passing value.
    Measured: between 2.2e-6 and 4.3e-6; the largest |lp'| is about 33 (one fp32 ulp there: 3.8e-6)."""
    x, y = U.model_logits(N, U.tdtype(dt)), U.lm_logits(U.tdtype(dt))
    err, big = U.fp32_torch_error(x, y, U.W, T)
    print("N=%d T=%g %s: fp32 torch max |err| %.3e, max |lp'| %.1f" % (N, T, dt, err, big))
    assert err < U.CAP and big < 64.0
    ref = U.fused_lprobs(x, y, U.W, T, torch.float64)
    fin = torch.isfinite(ref)
    assert int((~fin[9]).sum()) == len(range(0, U.VOCAB, 11)) and int((~fin[7]).sum()) == len(range(0, U.VOCAB, 13))
    assert bool(fin[5].all()) and not torch.isnan(ref).any()  # (-inf in one member only leaves the element finite)


@pytest.mark.parametrize("dt,V,N,variant", U.SEARCH_PARAMS)
def test_search_seeds_keep_every_selection_gap_above_1e_4(dt, V, N, variant):
    """What lets the GPU search test demand exact ids: in fp64 no two neighbours among a sentence's first 2 * beam + 1 candidates of
    any step are closer than 1e-4 (the kernel's per-element bound times the steps is 4.6e-5); hypotheses finish within the steps."""
    st, states = U.run_restatement(dt, V, N, variant)
    assert st["min_gap"] > 1e-4, st["min_gap"]
    assert int(st["nfinal"].sum()) > 0, "no hypothesis finished within the steps taken"
    if variant == "plain":  # the LM matters: the same inputs searched without it take another path
        st0 = U.new_state()
        for s in range(U.STEPS):
            model, lm = U.search_logits(dt, V, N, s)
            U.select_step(st0, U.masked(st0, U.fused_step_lprobs(model, lm, 0.0), s), s)
        assert not torch.equal(st0["tokens"], st["tokens"])
