"""GPU tests of lexically constrained decoding, --constraints [ordered|unordered] (beam_search.hip cst_lex_init / cst_beam_step_lex,
decode_engine.py, sequence_generator.py LexicallyConstrainedBeamSearch, cli.py):
  * cst_beam_step_lex called directly, one case per row-kernel family, step by step against the restatement of
    tests/decode_lexical_util.py; identity of a batch without constraints and of x = NULL with cst_beam_step; bad arguments;
  * the engine and the host loop against the hypotheses of the REAL reference's SequenceGenerator (decode_lexical_tiny.npz);
  * engine == host loop on a two-member ensemble and with a language model; the launches of a step; the fallback beyond the device
    limits; constraints that cannot be met; the command line."""
import ast
import ctypes
import os
import shutil
from argparse import Namespace
from importlib import import_module

import pytest
import torch

import decode_lexical_util as U
from conftest import GOLDEN, load_golden, load_pkg
from decode_lexical_util import BSZ, CASES, EOS, MAX_LEN, PAD, UNK, SEEDS, VARIANTS
from decode_diverse_util import new_state, step_logits
from test_decode_constraints_gpu import _ragged_sample, fixture_models
from test_decode_engine_gpu import _beam_state, _build_s2t
from test_model_gpu import assert_close

pytestmark = pytest.mark.gpu
ERR_BAD_ARG, ERR_UNSUPPORTED = -1, -4  # CST_ERR_BAD_ARG, CST_ERR_UNSUPPORTED


def sgm():
    load_pkg()
    return import_module("chimera-st_amd.sequence_generator")


def lcm():
    load_pkg()
    return import_module("chimera-st_amd.lexical_constraints")


@pytest.fixture(scope="module")
def L():
    load_pkg()
    return import_module("chimera-st_amd.lib")


def _lex(L, representation, packed, bsz, beam):
    """(descriptor, the tensors it points to) of cst_lex_init / cst_beam_step_lex."""
    packed = packed.to(device="cuda", dtype=torch.int64).contiguous()
    ws = torch.zeros(L.load().cst_lex_workspace(bsz, beam, packed.size(1)), dtype=torch.uint8, device="cuda")
    x = L.LexDesc()
    x.representation = {"ordered": 1, "unordered": 2}[representation]
    x.constraints, x.width, x.workspace = packed.data_ptr(), packed.size(1), ws.data_ptr()
    return x, (packed, ws)


def _check_states(L, ws, half, states, beam, s):
    """The device's constraint states of the rows against the restatement's: node, bank, finished, next tokens."""
    dev = L.lex_states(ws, BSZ, beam)[half].cpu()
    for b in range(BSZ):
        for r in range(beam):
            want, got = states[b][r], dev[b * beam + r].tolist()
            nxt = want.next_tokens()
            assert got[0] == want.word() and got[1] == want.bank and got[2] == int(want.finished), (s, b, r, got[:4])
            assert got[3] == len(nxt) and got[8:8 + len(nxt)] == nxt, (s, b, r, got[3:8 + len(nxt)], nxt)


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("dtype_name,V,members", CASES)
def test_beam_step_lex_matches_restatement(L, dtype_name, V, members, variant):
    """bsz 3, max_len 12, run to the end on fresh logits per step: after EVERY step the device state equals that of the restatement —
    tokens, ancestry (the parents), constraint states, cands_to_ignore, finished, nfinal, fin_tokens, fin_len exactly; scores and fin_score
    to 1e-5 (test_decode_lexical_cpu.py shows that no id hangs on the rounding of the log-softmax)."""
    beam, representation, constraints, ngram, with_lm = VARIANTS[variant]
    seed = SEEDS.get((dtype_name, V, members, variant), 0)
    dtype = torch.bfloat16 if dtype_name == "bf16" else torch.float32
    lib = L.load()
    bbsz, Vp = BSZ * beam, (V + 7) // 8 * 8
    bufs = [torch.zeros(bbsz, Vp, dtype=dtype, device="cuda") for _ in range(members)]
    lm_buf = torch.zeros(bbsz, Vp, dtype=dtype, device="cuda")
    st, d = _beam_state(L, BSZ, beam, V, MAX_LEN, 1, dtype, bufs[0], pad=PAD, unk=UNK, eos=EOS)
    if members > 1:
        d.members = members
        for n in range(1, members):
            d.logits_n[n - 1] = bufs[n].data_ptr()
    d.no_repeat_ngram = ngram
    f = L.LmFusionDesc()
    f.lm_logits, f.lm_weight, f.lprobs_out = (lm_buf.data_ptr() if with_lm else None), U.LM_WEIGHT, None
    x, (packed, ws) = _lex(L, representation, U.pack(constraints), BSZ, beam)
    L.check(lib.cst_beam_init(ctypes.byref(d), L.stream_ptr()), "cst_beam_init")
    L.check(lib.cst_lex_init(ctypes.byref(d), ctypes.byref(x), L.stream_ptr()), "cst_lex_init")
    ref = new_state(beam, "cuda")
    states = U.root_states(representation, constraints, beam)
    for half in (0, 1):
        _check_states(L, ws, half, states, beam, -1)
    for s in range(MAX_LEN + 1):
        logits = [t.cuda() for t in U.lex_step_logits(dtype_name, V, members, s, beam, seed)]
        for buf, t in zip(bufs, logits):
            buf[:, :V] = t
        lm = U.lm_step_logits(dtype_name, V, s, beam, seed).cuda() if with_lm else None
        if with_lm:
            lm_buf[:, :V] = lm
        L.check(lib.cst_beam_step_lex(ctypes.byref(d), ctypes.byref(f), ctypes.byref(x), L.stream_ptr()), "cst_beam_step_lex")
        U.search_step(ref, logits, s, beam, states, ngram=ngram, lm_logits=lm)
        assert int(st["step"].item()) == s + 1
        nxt = (s + 1) & 1 if s < MAX_LEN else s & 1  # the last step writes no new rows
        n_tok = min(s + 2, MAX_LEN + 1)
        assert torch.equal(st["tokens"][nxt, :, :n_tok], ref["tokens"][:, :n_tok]), s
        assert torch.equal(st["anc"][nxt, :, :n_tok], ref["anc"][:, :n_tok]), s
        _check_states(L, ws, nxt, states, beam, s)
        got, want = st["scores"][nxt, :, :min(s + 1, MAX_LEN)], ref["scores"][:, :min(s + 1, MAX_LEN)]
        assert torch.equal(torch.isinf(got), torch.isinf(want)), s
        err = float((got - want).nan_to_num(0.0, 0.0, 0.0).abs().max())
        print("step %2d  max |scores - restatement| %.2e  max |score| %.1f  fin_score %.2e" % (
            s, err, float(want.nan_to_num(0.0, 0.0, 0.0).abs().max()), float((st["fin_score"] - ref["fin_score"]).abs().max())))
        assert err <= 1e-5, s
        for k in ("ignore", "finished", "nfinal", "fin_len"):
            assert torch.equal(st[k], ref[k]), (k, s)
        assert torch.equal(st["fin_tokens"], ref["fin_tokens"]), s
        assert float((st["fin_score"] - ref["fin_score"]).abs().max()) <= 1e-5, s
    assert ref["finished"].tolist() == [1] * BSZ and int(st["num_remaining"].item()) == 0
    for b in range(BSZ):  # the hypotheses hold their constraints
        for r in range(int(st["nfinal"][b])):
            n = int(st["fin_len"][b, r])
            assert U.contains(st["fin_tokens"][b, r, :n - 1].tolist(), constraints[b], representation == "ordered"), (b, r)


def _snapshots(L, dtype_name, V, beam, step_fn):
    dtype = torch.bfloat16 if dtype_name == "bf16" else torch.float32
    buf = torch.zeros(BSZ * beam, (V + 7) // 8 * 8, dtype=dtype, device="cuda")
    st, d = _beam_state(L, BSZ, beam, V, MAX_LEN, 1, dtype, buf, pad=PAD, unk=UNK, eos=EOS)
    L.check(L.load().cst_beam_init(ctypes.byref(d), L.stream_ptr()), "cst_beam_init")
    keep = step_fn(d, None)
    snaps = []
    for s in range(MAX_LEN + 1):
        buf[:, :V] = step_logits(dtype_name, V, 1, s, beam)[0].cuda()
        step_fn(d, keep)
        snaps.append({k: st[k].clone() for k in ("tokens", "scores", "anc", "ignore", "finished", "nfinal", "fin_tokens", "fin_pos",
                                                 "fin_score", "fin_len", "num_remaining")})
    return snaps


@pytest.mark.parametrize("how", ["no_constraints_ordered", "no_constraints_unordered", "null_x"])
@pytest.mark.parametrize("dtype_name,V", [("fp32", 60), ("bf16", 10000)])
def test_no_constraints_and_null_descriptor_equal_plain_beam_search_bitwise(L, dtype_name, V, how):
    beam = 4
    lib = L.load()

    def plain(d, keep):
        if keep is not None:
            L.check(lib.cst_beam_step(ctypes.byref(d), L.stream_ptr()), "cst_beam_step")
        return ()

    def lex(d, keep):
        if keep is None:
            if how == "null_x":
                return ()
            x, held = _lex(L, how.split("_")[-1], torch.zeros(BSZ, 1, dtype=torch.long), BSZ, beam)
            L.check(lib.cst_lex_init(ctypes.byref(d), ctypes.byref(x), L.stream_ptr()), "cst_lex_init")
            return (x, held)
        L.check(lib.cst_beam_step_lex(ctypes.byref(d), None, ctypes.byref(keep[0]) if keep else None, L.stream_ptr()), "cst_beam_step_lex")
        return keep

    a, b = _snapshots(L, dtype_name, V, beam, plain), _snapshots(L, dtype_name, V, beam, lex)
    for s, (p, q) in enumerate(zip(a, b)):
        for k in p:
            same = torch.equal(p[k].view(torch.int32), q[k].view(torch.int32)) if p[k].dtype == torch.float32 else torch.equal(p[k], q[k])
            assert same, (k, s)
    assert a[-1]["finished"].tolist() == [1] * BSZ


def test_beam_step_lex_rejects_bad_arguments(L):
    lib = L.load()
    beam = 4
    logits = torch.zeros(BSZ * beam, 64, device="cuda")
    st, d = _beam_state(L, BSZ, beam, 60, MAX_LEN, 1, torch.float32, logits)
    L.check(lib.cst_beam_init(ctypes.byref(d), L.stream_ptr()), "cst_beam_init")
    x, (packed, ws) = _lex(L, "ordered", U.pack([[[7]], [], [[8, 9]]]), BSZ, beam)
    L.check(lib.cst_lex_init(ctypes.byref(d), ctypes.byref(x), L.stream_ptr()), "cst_lex_init")
    torch.cuda.synchronize()
    before = {k: v.clone() for k, v in st.items()}
    ws_before = ws.clone()
    key = torch.zeros(1, dtype=torch.int32, device="cuda")
    prefix = torch.full((BSZ, 1), 5, dtype=torch.int64, device="cuda")
    wide = torch.zeros(BSZ, 66, dtype=torch.int64, device="cuda")

    def both(want, what):
        assert lib.cst_beam_step_lex(ctypes.byref(d), None, ctypes.byref(x), L.stream_ptr()) == want, what
        assert lib.cst_lex_init(ctypes.byref(d), ctypes.byref(x), L.stream_ptr()) == want, what

    for rep in (0, 3, -1):
        x.representation = rep
        both(ERR_BAD_ARG, ("representation", rep))
    x.representation = 1
    x.workspace = None
    both(ERR_BAD_ARG, "null workspace")
    x.workspace = ws.data_ptr()
    x.constraints, x.width = wide.data_ptr(), 66
    both(ERR_UNSUPPORTED, "width 66")
    x.constraints, x.width = packed.data_ptr(), packed.size(1)
    for field, value, extra in (("sampling", 1, ("sample_key", key.data_ptr())), ("diverse_groups", 2, ("diverse_strength", 0.5)),
                                ("diverse_siblings", 1, ("sibling_rate", 0.5)), ("prefix_len", 1, ("prefix_tokens", prefix.data_ptr()))):
        setattr(d, field, value)
        setattr(d, *extra)
        both(ERR_BAD_ARG, field)
        setattr(d, field, 0)
        setattr(d, extra[0], None if extra[0] in ("sample_key", "prefix_tokens") else 0.0)
    torch.cuda.synchronize()
    for k, v in st.items():  # nothing was launched: the state buffers are untouched
        assert torch.equal(v, before[k]), k
    assert torch.equal(ws, ws_before) and int(st["step"].item()) == 0
    L.check(lib.cst_beam_step_lex(ctypes.byref(d), None, ctypes.byref(x), L.stream_ptr()), "cst_beam_step_lex")
    assert int(st["step"].item()) == 1


# ---- 2. the fixture of the real reference ---------------------------------------------------------------------------------------------
SETTING_NAMES = ["base", "base_ngram2", "ord", "ord_ngram2", "unord"]


def _fixture_run(name, fused, widen=0):
    """(generator, hypotheses, fixture) of setting `name`; widen > 0: the packed constraints padded with zeros to that width."""
    m = fixture_models()
    fx, rec = load_golden("decode_lexical_tiny.npz"), load_golden("decode_recipe_tiny.npz")
    settings = ast.literal_eval(str(fx["meta/settings"]))
    assert sorted(settings) == SETTING_NAMES
    kw = settings[name]
    model, d = m[kw["model"]], m["task"].target_dictionary
    sg = sgm()
    strategy = sg.LexicallyConstrainedBeamSearch(d, kw["constraints"]) if "constraints" in kw else None
    gen = sg.SequenceGenerator([model], d, beam_size=kw["beam_size"], max_len_a=0, max_len_b=kw["max_len_b"],
                               no_repeat_ngram_size=kw.get("no_repeat_ngram_size", 0), temperature=kw.get("temperature", 1.0),
                               search_strategy=strategy, fused=fused)
    sample = {"net_input": {"src_tokens": torch.from_numpy(rec["in/b/src_tokens"]).cuda(),
                            "src_lengths": torch.from_numpy(rec["in/b/src_lengths"]).cuda()}}
    packed = torch.from_numpy(fx["meta/constraints/" + name]) if "constraints" in kw else None
    if packed is not None and widen:
        packed = torch.cat((packed, torch.zeros(packed.size(0), widen - packed.size(1), dtype=torch.long)), 1)
    return gen, gen.generate([model], sample, constraints=packed), fx


def _assert_fixture(name, hyps, fx):
    for b in range(len(hyps)):
        n = int(fx["gen/%s/b%d/n" % (name, b)])
        assert len(hyps[b]) == n, (name, b)
        for r in range(n):
            key = "gen/%s/b%d/r%d/" % (name, b, r)
            assert hyps[b][r]["tokens"].tolist() == fx[key + "tokens"].tolist(), key
            assert abs(float(hyps[b][r]["score"]) - float(fx[key + "score"])) < 1e-4, key
            assert_close(hyps[b][r]["positional_scores"], fx[key + "pos_scores"], 1e-4, key + "pos_scores")


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", SETTING_NAMES)
def test_lexical_matches_reference_generator(name, fused):
    """Every finalized hypothesis of the reference's SequenceGenerator + LexicallyConstrainedBeamSearch in its order: ids exact, scores
    and positional scores to 1e-4 — device engine and host loop, fp32."""
    gen, hyps, fx = _fixture_run(name, fused)
    assert (gen._engine is not None) == fused
    if fused and name not in ("base", "base_ngram2"):
        assert gen._engine.lexical == gen.lexical and any(st["lex_desc"] is not None for st in gen._engine._state.values())
    _assert_fixture(name, hyps, fx)


def test_beyond_the_device_limits_the_host_loop_decodes():
    """A packed width of 66 is beyond what cst_lex_init takes (refused above with CST_ERR_UNSUPPORTED): the generator takes the host
    loop up front and still finds the reference's hypotheses of the fixture's setting.  So it does for 33 real constraint tokens in one
    sentence (sentence 1, which must then contain them; the other two decode as plain beam search)."""
    gen, hyps, fx = _fixture_run("ord", True, widen=66)
    assert gen.fused and gen._engine is None
    _assert_fixture("ord", hyps, fx)
    gen, hyps, fx = _fixture_run("ord", True, widen=65)  # the widest the engine takes
    assert gen._engine is not None
    _assert_fixture("ord", hyps, fx)
    lc = lcm()
    assert not lc.device_limits_ok(lc.pack_constraints([[list(range(4, 37))]]))
    m = fixture_models()
    model, d = m["unfitted"], m["task"].target_dictionary
    rec = load_golden("decode_recipe_tiny.npz")
    sg = sgm()
    gen = sg.SequenceGenerator([model], d, beam_size=4, max_len_a=0, max_len_b=40, temperature=2.0,
                               search_strategy=sg.LexicallyConstrainedBeamSearch(d, "ordered"))
    sample = {"net_input": {"src_tokens": torch.from_numpy(rec["in/b/src_tokens"]).cuda(),
                            "src_lengths": torch.from_numpy(rec["in/b/src_lengths"]).cuda()}}
    long = list(range(4, 37))
    hyps = gen.generate([model], sample, constraints=lc.pack_constraints([[], [long], []]))
    assert gen.fused and gen._engine is None  # the host loop took it
    assert all(U.contains(h["tokens"].tolist()[:-1], [long], True) for h in hyps[1]) and len(hyps[1]) >= 1
    plain = sg.SequenceGenerator([model], d, beam_size=4, max_len_a=0, max_len_b=40, temperature=2.0).generate([model], sample)
    for b in (0, 2):
        assert [h["tokens"].tolist() for h in hyps[b]] == [h["tokens"].tolist() for h in plain[b]]


@pytest.mark.parametrize("fused", [True, False])
def test_constraints_that_cannot_be_met_raise(fused):
    """A 5-token constraint with max_len_b 3: every last-step candidate of the sentence is -inf, nothing is finalised — RuntimeError
    naming the sentence, in the engine (which must not trip its termination assertion) and in the host loop."""
    m = fixture_models()
    model, d = m["unfitted"], m["task"].target_dictionary
    rec = load_golden("decode_recipe_tiny.npz")
    sg = sgm()
    gen = sg.SequenceGenerator([model], d, beam_size=4, max_len_a=0, max_len_b=3, temperature=2.0,
                               search_strategy=sg.LexicallyConstrainedBeamSearch(d, "ordered"), fused=fused)
    sample = {"net_input": {"src_tokens": torch.from_numpy(rec["in/b/src_tokens"]).cuda(),
                            "src_lengths": torch.from_numpy(rec["in/b/src_lengths"]).cuda()}}
    packed = lcm().pack_constraints([[], [[5, 6, 7, 8, 9]], []])
    with pytest.raises(RuntimeError, match=r"lexical constraints not met within max_len: sentences \[1\]"):
        gen.generate([model], sample, constraints=packed)
    assert (gen._engine is not None) == fused
    hyps = gen.generate([model], sample, constraints=lcm().pack_constraints([[], [[5]], []]))  # the generator is still usable
    assert all(len(h) >= 1 for h in hyps) and all(5 in h["tokens"].tolist() for h in hyps[1])


# ---- 3. engine == host loop, the step graph ---------------------------------------------------------------------------------------------
def _flat(hyps):
    return [[(h["tokens"].tolist(), float(h["score"])) for h in hb] for hb in hyps]


def _same(h1, h2):
    assert len(h1) == len(h2)
    for b in range(len(h1)):
        assert len(h1[b]) == len(h2[b]) >= 1, b
        for r in range(len(h1[b])):
            assert h1[b][r]["tokens"].tolist() == h2[b][r]["tokens"].tolist(), (b, r)
            assert abs(float(h1[b][r]["score"]) - float(h2[b][r]["score"])) < 1e-4


def _ragged_constraints(representation):
    """For the four sentences of _ragged_sample (vocabulary 500): a branching pair + a single, none, a repeated phrase, a long phrase."""
    cons = [[[40, 41], [40, 42], [77]], [], [[90], [90]], [[120, 121, 122]]]
    if representation == "ordered":
        cons[0] = [[40, 41], [77]]
    return cons


def test_engine_equals_host_loop_on_an_ensemble_unordered():
    models, task = [], None
    for k in range(2):
        m, task = _build_s2t(torch.float32, tied=(k == 1), seed=3 + k)
        models.append(m)
    d = task.target_dictionary
    sample = _ragged_sample()
    sg = sgm()
    cons = _ragged_constraints("unordered")
    packed = lcm().pack_constraints(cons)
    kw = dict(beam_size=4, max_len_a=0, max_len_b=20, min_len=3)
    fused = sg.SequenceGenerator(models, d, search_strategy=sg.LexicallyConstrainedBeamSearch(d, "unordered"), **kw)
    mirror = sg.SequenceGenerator(models, d, search_strategy=sg.LexicallyConstrainedBeamSearch(d, "unordered"), fused=False, **kw)
    h1, h2 = fused.generate(models, sample, constraints=packed), mirror.generate(models, sample, constraints=packed)
    assert fused._engine is not None and len(fused._engine.decs) == 2 and fused._engine.lexical == "unordered" and mirror._engine is None
    _same(h1, h2)
    for b, cs in enumerate(cons):
        assert all(U.contains(h["tokens"].tolist()[:-1], cs, False) for h in h1[b]), b
    plain = sg.SequenceGenerator(models, d, **kw).generate(models, sample)
    assert _flat(h1)[1] == _flat(plain)[1] and _flat(h1)[0] != _flat(plain)[0]
    # the same generator without constraints: the plain path, plain hypotheses; and with them again (a second state configuration)
    assert _flat(fused.generate(models, sample)) == _flat(plain)
    _same(fused.generate(models, sample, constraints=packed), h1)


def test_engine_equals_host_loop_with_a_language_model_and_in_two_lanes():
    from test_decode_lm_gpu import _build_lm
    model, task = _build_s2t(torch.float32, layers=2, tied=False)
    lm = _build_lm(torch.float32, layers=2)
    d = task.target_dictionary
    sample = _ragged_sample()
    sg = sgm()
    cons = _ragged_constraints("ordered")
    packed = lcm().pack_constraints(cons)
    kw = dict(beam_size=4, max_len_a=0, max_len_b=20, lm_model=lm, lm_weight=0.5, no_repeat_ngram_size=3)
    fused = sg.SequenceGenerator([model], d, search_strategy=sg.LexicallyConstrainedBeamSearch(d, "ordered"), **kw)
    mirror = sg.SequenceGenerator([model], d, search_strategy=sg.LexicallyConstrainedBeamSearch(d, "ordered"), fused=False, **kw)
    h1, h2 = fused.generate([model], sample, constraints=packed), mirror.generate([model], sample, constraints=packed)
    assert fused._engine is not None and fused._engine.lm is not None and mirror._engine is None
    _same(h1, h2)
    for b, cs in enumerate(cons):
        assert all(U.contains(h["tokens"].tolist()[:-1], cs, True) for h in h1[b]), b
    # two lanes: each lane has its own constraint buffer, tables and states
    E = import_module("chimera-st_amd.decode_engine")
    import dataclasses
    eng = E.BeamDecodeEngine([model.decoder], d, dataclasses.replace(fused.options, max_len=20), lm_decoder=lm.decoder, lanes=2,
                             lexical="ordered")
    enc = [model.encoder.forward_torchscript(sample["net_input"])]
    h3 = eng.generate(enc, 4, constraints=packed)
    assert len(eng._state) == 2
    _same(h3, h1)


def test_step_graph_has_the_same_nodes_with_lexical_constraints():
    """The constraint code lives in the two search kernels, so a step is the same launch sequence: the launch records of ONE step of the
    engine in the library's profiler, plain against constrained, and nodes_per_step unchanged."""
    model, task = _build_s2t(torch.float32, tied=False)
    d = task.target_dictionary
    sample = _ragged_sample()
    sg, lib = sgm(), import_module("chimera-st_amd.lib")
    packed = lcm().pack_constraints(_ragged_constraints("unordered"))
    launches, nodes = {}, {}
    for name in ("plain", "lexical"):
        strat = sg.LexicallyConstrainedBeamSearch(d, "unordered") if name == "lexical" else None
        gen = sg.SequenceGenerator([model], d, beam_size=4, max_len_a=0, max_len_b=8, search_strategy=strat)
        gen.generate([model], sample, constraints=packed if name == "lexical" else None)
        eng = gen._engine
        states = list(eng._state.values())
        assert len(states) == 1 and states[0]["graph"] is not None and (states[0]["lex_desc"] is not None) == (name == "lexical")
        st, pk = states[0], eng._packed[1]
        lib.check(lib.load().cst_beam_init(ctypes.byref(st["desc"]), lib.stream_ptr()), "cst_beam_init")  # back to step 0
        torch.cuda.synchronize()
        lib.prof_enable(True)
        eng._step(st, pk, 4)
        torch.cuda.synchronize()
        table = lib.prof_query()
        lib.prof_enable(False)
        launches[name] = sum(v["launches"] for v in table.values())
        nodes[name] = eng.nodes_per_step(torch.float32, 16)
    print("launch records of a step", launches, nodes)
    assert launches["lexical"] == launches["plain"] > 2 and nodes["lexical"] == nodes["plain"]


# ---- 4. the command line ----------------------------------------------------------------------------------------------------
def test_cli_constraints(tmp_path, capsys):
    """fairseq_generate.py --constraints [unordered] --constraints-file F on tests/golden/data_tiny: the C- lines name the constraints,
    every printed hypothesis of a constrained utterance holds its phrases, utterances without a line decode as without the flag, and the
    hypotheses are those of a direct SequenceGenerator call with the same packed constraints."""
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

    sg = sgm()
    seen = {}
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
        hyp, con = {}, {}
        for l in out:
            if l.startswith("H-"):
                hyp.setdefault(int(l.split("\t")[0][2:]), []).append(l.split("\t")[-1])
            if l.startswith("C-"):
                con.setdefault(int(l.split("\t")[0][2:]), []).append(l.split("\t")[-1])
        return summary, hyp, con, seen["gen"], list(seen["calls"])

    summary0, hyp0, con0, gen0, _ = run([])
    assert con0 == {} and summary0["constraints"] is None and type(gen0.search) is sg.BeamSearch
    tgt = gen0.tgt_dict
    ids = [l.split("\t")[0] for l in (root / "dev_st.tsv").read_text().splitlines()[1:]]
    assert len(ids) >= 2
    # phrases made of dictionary symbols no plain hypothesis of the utterance uses
    used = set(w for hs in hyp0.values() for h in hs for w in h.split())
    free = [tgt[i] for i in range(4, len(tgt)) if tgt[i] not in used and not tgt[i].startswith("filler")][:3]
    assert len(free) == 3
    cfile = tmp_path / "c.tsv"
    cfile.write_text("%s\t%s %s\t%s\n" % (ids[0], free[0], free[1], free[2]), encoding="utf-8")
    for flag, rep in (["--constraints"], "ordered"), (["--constraints", "unordered"], "unordered"):
        summary, hyp, con, gen, calls = run(flag + ["--constraints-file", str(cfile)])
        assert summary["ignored_flags"] == [] and summary["constraints"] == rep and summary["nbest"] == 4
        assert type(gen.search) is sg.LexicallyConstrainedBeamSearch and gen.search.representation == rep and gen.fused
        assert con == {0: ["%s %s" % (free[0], free[1]), free[2]]}
        assert all(kw.get("constraints") is not None for _, _, kw in calls)
        assert len(hyp[0]) >= 1 and all(("%s %s" % (free[0], free[1])) in h and free[2] in h.split() for h in hyp[0])
        for sid in hyp0:  # utterances without a line: as without the flag
            if sid != 0:
                assert hyp[sid] == hyp0[sid], sid
        direct = sg.SequenceGenerator(calls[0][0], tgt, beam_size=4, max_len_a=0, max_len_b=12, temperature=2.0,
                                      search_strategy=sg.LexicallyConstrainedBeamSearch(tgt, rep))
        hyps = [hb for models, sample, kw in calls for hb in direct.generate(models, sample, **kw)]
        assert direct._engine is not None
        strings = sorted(tuple(tgt.string(h["tokens"].cpu()) for h in hb[:4]) for hb in hyps)
        assert sorted(tuple(h) for h in hyp.values()) == strings
    with pytest.raises(ValueError, match="go together"):
        cli.generate_main(common + ["--constraints"])
    with pytest.raises(ValueError, match="mutually exclusive"):
        cli.generate_main(common + ["--constraints", "--constraints-file", str(cfile), "--sampling"])
    cfile.write_text("nobody\t%s\n" % free[0], encoding="utf-8")
    with pytest.raises(ValueError, match="not in the manifest"):
        cli.generate_main(common + ["--constraints", "--constraints-file", str(cfile)])
