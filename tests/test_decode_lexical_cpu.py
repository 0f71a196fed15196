"""No-GPU tests of lexically constrained decoding (--constraints):
  (a) chimera-st_amd/lexical_constraints.py against hand-written transition tables, both representations, pack / unpack;
  (b) the host search class LexicallyConstrainedBeamSearch.step against the restatement of tests/decode_lexical_util.py;
  (c) the kernel test's inputs (tests/test_decode_lexical_gpu.py) are not vacuous and decide every id with a margin;
  (d) the conditions of tests/golden/decode_lexical_tiny.npz, re-asserted on the committed file;
  (e) the generator's selection and refusals, the command-line flags, the constraints file;
  (f) the C ABI: the header documents the new entries, the binding declares them, the ABI version stands."""
import ast
import os
import re
from argparse import Namespace
from importlib import import_module

import numpy as np
import pytest
import torch

import decode_lexical_util as U
from conftest import GOLDEN, ROOT, load_pkg
from decode_lexical_util import BSZ, CASES, EOS, MAX_LEN, PAD, VARIANTS
from decode_diverse_util import new_state


def LC():
    load_pkg()
    return import_module("chimera-st_amd.lexical_constraints")


def SG():
    load_pkg()
    return import_module("chimera-st_amd.sequence_generator")


class Dict:
    """The three special symbols and a size: all a search class asks of a dictionary."""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    pad, eos, unk = (lambda self: PAD), (lambda self: EOS), (lambda self: 3)


# ---- (a) the state machines ------------------------------------------------------------------------------------------------------
def test_pack_and_unpack_round_trip():
    lc = LC()
    batch = [[[3, 1 + 4, 2 + 4], [7], [4, 5, 6, 7]], [], [[11, 8, 9, 10, 11, 4, 11, 12]]]
    packed = lc.pack_constraints(batch)
    assert packed.dtype == torch.long and packed.tolist() == [[3, 3, 5, 6, 0, 7, 0, 4, 5, 6, 7, 0], [0] * 12, [1, 11, 8, 9, 10, 11, 4, 11, 12, 0, 0, 0]]
    assert [lc.unpack_constraints(r) for r in packed] == batch
    assert lc.pack_constraints([[], []]).tolist() == [[0], [0]]
    assert lc.pack_constraints([[torch.tensor([5, 6])]]).tolist() == [[1, 5, 6, 0]]
    for bad in ([[0]], [[5, 0, 6]], [[PAD]], [[EOS]], [[-1]], [[]]):
        with pytest.raises(ValueError):
            lc.pack_constraints([[bad[0]]], pad=PAD, eos=EOS)
    assert lc.pack_constraints([[[PAD]]]).tolist() == [[1, PAD, 0]]  # (pad / eos are refused only where the caller names them)


def _walk(state, tokens):
    out = []
    for t in tokens:
        state = state.advance(t)
        out.append((getattr(state, "state", getattr(state, "node", None)), state.bank, state.finished, state.next_tokens()))
    return out


def test_ordered_state_transition_table():
    lc = LC()
    s = lc.create_state("ordered", lc.pack_constraints([[[5, 6], [7]]])[0])
    assert (s.state, s.bank, s.finished, s.next_tokens(), s.num_distinct) == (-1, 0, False, [5], 3)
    #                       token: (state, bank, finished, next tokens)
    assert _walk(s, [9, 5, 5, 6, 9, 5, 7, 9, 5]) == [
        (-1, 0, False, [5]),      # 9 at the root: the root reads endpoints[-1] (true) and stays
        (0, 1, False, [6]),       # 5 starts; state 0 is not "> 0", so the first token is not offered again
        (0, 1, False, [6]),       # 5 again inside [5 6]: not an endpoint, but the first token of all -> state 0
        (1, 2, False, [5, 7]),    # 6 ends the first constraint; from here the first token is offered too
        (1, 2, False, [5, 7]),    # anything between two constraints
        (1, 2, False, [5, 7]),    # ... the first token included: it is not the next token, and the state is an endpoint
        (2, 3, True, [5]),        # 7: finished; next_tokens still names the first token
        (2, 3, True, [5]),
        (2, 3, True, [5]),
    ]
    mid = lc.create_state("ordered", lc.pack_constraints([[[5, 6, 7]]])[0])
    assert _walk(mid, [5, 6, 9]) == [(0, 1, False, [6]), (1, 2, False, [5, 7]), (-1, 0, False, [5])]  # falls back to the root
    assert _walk(mid, [5, 6, 5]) [-1] == (0, 1, False, [6])                                            # ... or onto the first token
    rep = lc.create_state("ordered", lc.pack_constraints([[[8, 8, 9]]])[0])
    assert rep.num_distinct == 2 and _walk(rep, [8, 8, 8])[-1] == (0, 1, False, [8])  # distinct < total; [8 8] + 8 restarts at state 0
    none = lc.create_state("ordered", lc.pack_constraints([[]])[0])
    assert (none.bank, none.finished, none.next_tokens(), none.num_distinct) == (0, True, [], 0)
    assert _walk(none, [5, EOS]) == [(-1, 0, True, []), (-1, 0, True, [])]


def test_unordered_state_transition_table():
    lc = LC()
    # trie: root -> 5 (node 1) -> 6 (node 2, terminal); 5 -> 7 (node 3, terminal); root -> 8 (node 4, terminal)
    s = lc.create_state("unordered", lc.pack_constraints([[[5, 6], [5, 7], [8]]])[0])
    assert s.trie.token == [-1, 5, 6, 7, 8] and s.trie.parent == [-1, 0, 1, 1, 0]
    assert s.trie.terminal == [0, 0, 1, 1, 1] and s.trie.num_constraints == [3, 2, 1, 1, 1]
    assert (s.node, s.bank, s.finished, s.next_tokens(), s.num_distinct) == (0, 0, False, [5, 8], 4)
    assert _walk(s, [9, 5, 6, 5, 6, 7, 8, 9]) == [
        (0, 0, False, [5, 8]),
        (1, 1, False, [5, 6, 7, 8]),   # the root's children united with the node's
        (2, 2, False, [5, 8]),         # [5 6] generated; completed only when the state leaves it
        (1, 3, False, [5, 6, 7, 8]),   # 5 from node 2: back to the root and down again; rewind marks node 2 completed
        (0, 2, False, [5, 8]),         # 6 is saturated (generated 1 of 1): fall off; node 1 is no terminal -> un-generated
        (0, 2, False, [5, 8]),         # 7 is no child of the root
        (4, 3, False, [5, 8]),
        (0, 3, False, [5, 8]),         # leaving node 4 completes [8]; [5 7] is still open
    ]
    done = s
    for t in (5, 6, 5, 7, 8):
        done = done.advance(t)
    assert (done.node, done.bank, done.finished) == (4, 5, True)  # the node itself counts while it is an unfinished terminal
    dup = lc.create_state("unordered", lc.pack_constraints([[[5], [5]]])[0])
    assert dup.trie.terminal == [0, 2] and dup.trie.num_constraints == [2, 2] and dup.num_distinct == 1
    assert _walk(dup, [5, 5, 5, 9]) == [(1, 1, False, [5]), (1, 2, True, [5]), (0, 2, True, [5]), (0, 2, True, [5])]
    none = lc.create_state("unordered", lc.pack_constraints([[]])[0])
    assert (none.bank, none.finished, none.next_tokens(), none.num_distinct) == (0, True, [], 0)


def test_both_implementations_agree_on_random_walks():
    """lexical_constraints.py and the restatement's own state classes were written apart; 2000 random constraint sets x 16 tokens."""
    import random
    lc = LC()
    rnd = random.Random(0)
    for _ in range(2000):
        cons = [[rnd.choice([5, 6, 7, 8]) for _ in range(rnd.randint(1, 3))] for _ in range(rnd.randint(0, 4))]
        row = U.pack([cons])[0]
        for rep, cls in (("ordered", U.Ordered), ("unordered", U.Unordered)):
            a, b = lc.create_state(rep, row), cls(cons)
            for _ in range(16):
                assert (a.bank, a.finished, a.next_tokens(), a.num_distinct) == (b.bank, b.finished, b.next_tokens(), b.nd), (cons, rep)
                t = rnd.choice([5, 6, 7, 8, 9])
                a, b = a.advance(t), b.advance(t)


def test_device_limits():
    lc = LC()
    E = import_module("chimera-st_amd.decode_engine").BeamDecodeEngine
    ok = lc.pack_constraints([[list(range(4, 36))], []])                      # 32 tokens
    assert lc.device_limits_ok(ok) and E.lexical_supported(ok, 5) and ok.size(1) == 34
    assert not E.lexical_supported(lc.pack_constraints([[list(range(4, 37))]]), 5)   # 33 tokens
    fan16 = lc.pack_constraints([[[t] for t in range(4, 20)]])
    fan17 = lc.pack_constraints([[[t] for t in range(4, 21)]])
    assert E.lexical_supported(fan16, 5) and not E.lexical_supported(fan17, 5)       # next tokens of the root
    assert not E.lexical_supported(lc.pack_constraints([[[4, t] for t in range(5, 14)] + [[t] for t in range(20, 27)]]), 5)  # 1 + 7 + 9 = 17 under node 4
    assert not E.lexical_supported(ok, 21)
    wide = torch.zeros(2, 66, dtype=torch.long)
    assert E.lexical_supported(wide[:, :65], 5) and not E.lexical_supported(wide, 5)  # the width alone


# ---- (b) the host search class ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_host_search_step_equals_restatement(variant):
    """Every step of the search on the smallest case: the candidates of LexicallyConstrainedBeamSearch.step (given the masked
    log-probabilities and the cumulative scores of the restatement's state) are the restatement's — ids exact, values to 1e-6 — and so
    are the states after update_constraints."""
    dtype_name, V, members = CASES[0]
    beam, representation, constraints, ngram, with_lm = VARIANTS[variant]
    seed = U.SEEDS.get((dtype_name, V, members, variant), 0)
    search = SG().LexicallyConstrainedBeamSearch(Dict(V), representation)
    search.init_constraints(U.pack(constraints), beam)
    st, states = new_state(beam), U.root_states(representation, constraints, beam)
    for s in range(MAX_LEN + 1):
        logits = U.lex_step_logits(dtype_name, V, members, s, beam, seed)
        lm = U.lm_step_logits(dtype_name, V, s, beam, seed) if with_lm else None
        lp = U.masked_lprobs(st, logits, s, ngram=ngram, lm_logits=lm)
        sc, tok, par = search.step(s, lp.view(BSZ, beam, V), st["scores"].view(BSZ, beam, -1)[:, :, :s])
        trace = {}
        U.search_step(st, logits, s, beam, states, ngram=ngram, lm_logits=lm, trace=trace)
        assert tok.tolist() == trace["c_tok"].tolist() and par.tolist() == trace["c_beam"].tolist(), s
        assert torch.equal(torch.isinf(sc), torch.isinf(trace["c_score"])), s
        assert float((sc - trace["c_score"]).nan_to_num(0.0, 0.0, 0.0).abs().max()) <= 1e-6, s
        if s < MAX_LEN:
            search.update_constraints(torch.tensor(trace["act"]))
            for b in range(BSZ):
                for mine, theirs in zip(search.constraint_states[b], states[b]):
                    assert (mine.bank, mine.finished, mine.next_tokens()) == (theirs.bank, theirs.finished, theirs.next_tokens()), (s, b)
    assert st["finished"].tolist() == [1] * BSZ


def test_host_search_without_constraints_is_beam_search():
    sg = SG()
    V, beam = 60, 4
    search, plain = sg.LexicallyConstrainedBeamSearch(Dict(V), "ordered"), sg.BeamSearch(Dict(V))
    g = torch.Generator().manual_seed(3)
    lp, scores = torch.log_softmax(torch.randn(BSZ, beam, V, generator=g), -1), torch.randn(BSZ, beam, 3, generator=g)
    for s in (0, 3):
        for a, b in zip(search.step(s, lp, scores[:, :, :s]), plain.step(s, lp, scores[:, :, :s])):
            assert torch.equal(a, b)
    search.init_constraints(U.pack([[], [], []]), beam)  # constraint states of sentences that ask for nothing: the same candidates
    for a, b in zip(search.step(3, lp, scores), plain.step(3, lp, scores)):
        assert torch.equal(a, b)


# ---- (c) the kernel test's inputs --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("dtype_name,V,members", CASES)
def test_kernel_test_inputs_are_decisive(dtype_name, V, members, variant):
    beam, representation, constraints, ngram, with_lm = VARIANTS[variant]
    st, stats = U.run_restatement(dtype_name, V, members, variant)
    # every sentence finishes before the forced eos of step MAX_LEN, `beam` hypotheses each, and every one holds its constraints
    assert st["finished"].tolist() == [1] * BSZ and st["nfinal"].tolist() == [beam] * BSZ
    assert int(st["fin_len"].max()) <= MAX_LEN
    for b in range(BSZ):
        for r in range(beam):
            n = int(st["fin_len"][b, r])
            assert U.contains(st["fin_tokens"][b, r, :n - 1].tolist(), constraints[b], representation == "ordered"), (b, r)
    # in at least a quarter of the live (sentence, step) places a selected candidate was not in the plain top 2*beam
    print("places %d forced %d key gap %.3g value gap %.3g" % (stats["places"], stats["forced"], stats["key_gap"], stats["val_gap"]))
    assert stats["places"] >= 12 and stats["forced"] >= stats["places"] / 4.0
    # no id hangs on the rounding of the kernel's log-softmax: the keys of two distinct finite candidates adjacent in key order, one of
    # them selected, lie further apart than 1e-4 + 4 ulp of the key's largest addend (100 * nd); so do the plain top 2*beam values
    nd = max(len(set(t for c in cs for t in c)) for cs in constraints)
    assert stats["key_gap"] > 1e-4 + 4 * U.ulp32(100.0 * nd)
    assert stats["val_gap"] > 1e-4


# ---- (d) the fixture ---------------------------------------------------------------------------------------------------------------
def _fixture():
    return np.load(os.path.join(GOLDEN, "decode_lexical_tiny.npz"), allow_pickle=False)


def test_fixture_conditions():
    fx = _fixture()
    settings = ast.literal_eval(str(fx["meta/settings"]))
    assert sorted(settings) == ["base", "base_ngram2", "ord", "ord_ngram2", "unord"]
    hyps = lambda name, b: [fx["gen/%s/b%d/r%d/tokens" % (name, b, r)].tolist() for r in range(int(fx["gen/%s/b%d/n" % (name, b)]))]
    lc = LC()
    constrained = 0
    for name, kw in settings.items():
        if "constraints" not in kw:
            continue
        packed = fx["meta/constraints/" + name]
        assert packed.dtype == np.int64 and packed.shape[0] == 3
        for b in range(3):
            cons = lc.unpack_constraints(packed[b].tolist())
            if not cons:  # the unconstrained sentence equals the baseline exactly
                assert hyps(name, b) == hyps(kw["base"], b) and len(hyps(name, b)) == kw["beam_size"]
                for r in range(len(hyps(name, b))):
                    for part in ("score", "pos_scores"):
                        assert np.array_equal(fx["gen/%s/b%d/r%d/%s" % (name, b, r, part)], fx["gen/%s/b%d/r%d/%s" % (kw["base"], b, r, part)])
                continue
            constrained += 1
            base_best = hyps(kw["base"], b)[0]
            assert all(t not in base_best for c in cons[:1] for t in c[-1:]), (name, b)  # asks for something the baseline does not say
            assert hyps(name, b) and hyps(name, b)[0] != base_best, (name, b)
            for h in hyps(name, b):
                assert h[-1] == EOS and U.contains(h[:-1], cons, kw["constraints"] == "ordered"), (name, b, h)
    assert constrained == 6


# ---- (e) selection, flags, the constraints file ------------------------------------------------------------------------------------
class _Decoder:
    embed_tokens = None

    def eval(self):
        return self


class _Model:
    decoder = _Decoder()

    def eval(self):
        return self

    def max_decoder_positions(self):
        return 1024


def test_build_generator_selects_and_refuses():
    sg = SG()
    cli = import_module("chimera-st_amd.cli")
    T = import_module("chimera-st_amd.tasks")
    D = import_module("chimera-st_amd.dictionary").Dictionary
    d = D.synthetic(40)

    class Task(T.FairseqTask):
        def __init__(self):
            pass

        target_dictionary = property(lambda self: d)

    task = Task()
    base = dict(beam=4, max_len_a=0, max_len_b=8, min_len=1, unnormalized=False, lenpen=1.0, unkpen=0.0, temperature=1.0,
                no_repeat_ngram_size=0, seed=1)
    for rep in ("ordered", "unordered"):
        gen = task.build_generator([_Model()], Namespace(constraints=rep, **base))
        assert type(gen.search) is sg.LexicallyConstrainedBeamSearch and gen.search.representation == rep
        assert gen.lexical == rep and gen.fused and gen.options is not None
    plain = task.build_generator([_Model()], Namespace(constraints=None, **base))
    assert type(plain.search) is sg.BeamSearch and plain.lexical is None
    for extra in (dict(sampling=True), dict(diverse_beam_groups=2), dict(diversity_rate=0.5), dict(prefix_size=2)):
        with pytest.raises(ValueError, match="mutually exclusive|--prefix-size"):
            task.build_generator([_Model()], Namespace(constraints="ordered", **base, **extra))
    with pytest.raises(ValueError):
        sg.LexicallyConstrainedBeamSearch(d, "sorted")
    # constraints handed to a generator whose strategy cannot take them
    with pytest.raises(ValueError, match="LexicallyConstrainedBeamSearch"):
        plain._check_constraints(torch.zeros(1, 1, dtype=torch.long), None, 1)
    gen = task.build_generator([_Model()], Namespace(constraints="ordered", **base))
    with pytest.raises(ValueError, match="prefix"):
        gen._check_constraints(torch.zeros(1, 1, dtype=torch.long), torch.ones(1, 1, dtype=torch.long), 1)
    with pytest.raises(ValueError, match="packed"):
        gen._check_constraints(torch.zeros(2, 1, dtype=torch.long), None, 1)
    with pytest.raises(ValueError, match="constraint token"):
        gen._check_constraints(torch.tensor([[1, d.eos(), 0]]), None, 1)
    with pytest.raises(RuntimeError, match=r"lexical constraints not met within max_len: sentences \[1\]"):
        gen._unmet([[{}], [], [{}]])
    # the command line
    parse = lambda argv: cli.check_generate_args(cli.generate_parser().parse_args(["data", "--path", "m.pt"] + argv))
    assert parse([]).constraints is None
    assert parse(["--constraints", "--constraints-file", "c.tsv"]).constraints == "ordered"
    assert parse(["--constraints", "unordered", "--constraints-file", "c.tsv"]).constraints == "unordered"
    for argv in (["--constraints"], ["--constraints-file", "c.tsv"]):
        with pytest.raises(ValueError, match="go together"):
            parse(argv)
    for extra in (["--sampling"], ["--diverse-beam-groups", "2", "--beam", "4"], ["--diversity-rate", "0.5"], ["--prefix-size", "2"],
                  ["--score-reference"]):
        with pytest.raises(ValueError):
            parse(["--constraints", "--constraints-file", "c.tsv"] + extra)
    with pytest.raises(SystemExit):
        parse(["--constraints", "sorted", "--constraints-file", "c.tsv"])


def test_constraints_file(tmp_path):
    cli = import_module("chimera-st_amd.cli")
    D = import_module("chimera-st_amd.dictionary").Dictionary
    d = D.synthetic(40)
    words = [d[i] for i in range(4, 12)]
    f = tmp_path / "c.tsv"
    f.write_text("utt2\t%s %s\t%s\n\nutt0\t%s\nutt1\n" % (words[0], words[1], words[2], words[3]), encoding="utf-8")
    table = cli.read_constraints_file(str(f))
    assert table == {"utt2": ["%s %s" % (words[0], words[1]), words[2]], "utt0": [words[3]], "utt1": []}

    class DS:
        ids = ["utt0", "utt1", "utt2", "utt3"]

        def tokenize_text(self, text, side="target"):
            assert side == "target"
            return text

    assert cli.encode_constraints(DS(), table, d) == [[[7]], [], [[4, 5], [6]], []]
    with pytest.raises(ValueError, match="not in the manifest"):
        cli.encode_constraints(DS(), {"nobody": ["x"]}, d)
    f.write_text("utt0\ta\nutt0\tb\n")
    with pytest.raises(ValueError, match="twice"):
        cli.read_constraints_file(str(f))
    f.write_text("utt0\ta\t\tb\n")
    with pytest.raises(ValueError, match="empty phrase"):
        cli.read_constraints_file(str(f))


# ---- (f) the C ABI -----------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_lexical_entries():
    lib = load_pkg().lib
    src = open(os.path.join(ROOT, "include", "cst.h")).read()
    assert lib.ABI_VERSION == 13 and "#define CST_ABI_VERSION 13" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for decl in (r"int64_t cst_lex_workspace\(int64_t bsz, int64_t beam, int64_t width\);",
                 r"int cst_lex_init\(const cst_beam_desc\* d, const cst_lex_desc\* x, cst_stream stream\);",
                 r"int cst_beam_step_lex\(const cst_beam_desc\* d, const cst_lm_fusion_desc\* f, const cst_lex_desc\* x, cst_stream stream\);"):
        assert re.search(decl, code), decl
    body = re.search(r"typedef struct \{([^{}]*)\} cst_lex_desc;", code).group(1)
    fields = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", part)[-1] for part in body.split(";") if part.strip()]
    assert fields == [f[0] for f in lib.LexDesc._fields_] == ["representation", "constraints", "width", "workspace"]
    bound = {name: args for name, _, args in lib.SYMBOLS}
    assert len(bound["cst_lex_workspace"]) == 3 and len(bound["cst_lex_init"]) == 3 and len(bound["cst_beam_step_lex"]) == 4
    doc = " ".join(src.split())
    for phrase in ("LexicallyConstrainedBeamSearch :210-523", "eos ban", "endpoints[-1]", "(nd - bank) * -100", "cyclically", "stripe",
                   "CST_ERR_UNSUPPORTED", "cst_lex_desc, cst_lex_workspace, cst_lex_init and cst_beam_step_lex"):
        assert phrase in doc, phrase
