#!/usr/bin/env python3
"""tests/golden/decode_lexical_tiny.npz — the REAL reference's SequenceGenerator (imported through ref_import.py) with its
`LexicallyConstrainedBeamSearch` (search.py:210-523, token_generation_constraints.py: --constraints ordered | unordered).

Build container only:   python tools/ref_harness/make_decode_lexical_goldens.py
Holds data only — settings, the packed constraints and the generator's outputs (token ids, scores, positional scores), never reference
source.  Model parameters and audio are those of other fixtures and are NOT stored again:
  unfitted  the tiny Chimera model of decode_tiny.npz with the "unfitted/param/" tensors of decode_constraints_tiny.npz;
  audio     the three "b" utterances of decode_recipe_tiny.npz ("in/b/src_tokens", "in/b/src_lengths").

Settings (all finalized hypotheses of every sentence, in the reference's order); temperature 2, beam 4:
  base / base_ngram2          plain beam search, max_len_b 12 / max_len_b 16 with no_repeat_ngram_size 2
  ord, unord                  ordered / unordered constraints                              <- base
  ord_ngram2                  ordered constraints with no_repeat_ngram_size 2              <- base_ngram2
The constraint tokens are chosen from the tokens the baseline's best hypothesis of the sentence does NOT contain (pick()); sentence 1
has no constraints.  ordered: sentence 0 one two-token phrase, sentence 2 two one-token phrases; unordered: sentence 0 two phrases that
share their first token (a branching trie), sentence 2 the same phrase twice and another one.
Conditions (check(), re-asserted on the committed file by tests/test_decode_lexical_cpu.py): every hypothesis of a constrained
sentence contains its constraints (in order for `ordered`); its best hypothesis differs from the baseline's; the unconstrained
sentence equals the baseline exactly (tokens and scores of every hypothesis)."""
import ast
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ref_import import import_reference  # noqa: E402

import_reference()
import make_goldens as MG  # noqa: E402

EOS, PAD, B = 2, 1, 3
SETTINGS = {
    "base": dict(model="unfitted", temperature=2.0, beam_size=4, max_len_b=12),
    "base_ngram2": dict(model="unfitted", temperature=2.0, beam_size=4, max_len_b=16, no_repeat_ngram_size=2),
    "ord": dict(model="unfitted", temperature=2.0, beam_size=4, max_len_b=12, constraints="ordered", base="base"),
    "unord": dict(model="unfitted", temperature=2.0, beam_size=4, max_len_b=12, constraints="unordered", base="base"),
    "ord_ngram2": dict(model="unfitted", temperature=2.0, beam_size=4, max_len_b=16, no_repeat_ngram_size=2, constraints="ordered",
                       base="base_ngram2"),
}


def pick(best, V):
    """Four tokens the hypothesis `best` does not contain: spread over the vocabulary, never a special symbol."""
    free = [t for t in range(4, V) if t not in set(best)]
    return [free[len(free) * k // 5] for k in range(1, 5)]


def constraints_for(kind, best0, best2, V):
    a, b, c, _ = pick(best0, V)
    p, q, _, _ = pick(best2, V)
    if kind == "ordered":
        return [[[a, b]], [], [[p], [q]]]
    return [[[a, b], [a, c]], [], [[p], [p], [q]]]


def holds(tokens, constraints, ordered):
    tokens, at = list(tokens), 0
    for c in constraints:
        found = next((i for i in range(at if ordered else 0, len(tokens) - len(c) + 1) if tokens[i:i + len(c)] == list(c)), None)
        if found is None:
            return False
        at = found + len(c) if ordered else 0
    return True


def unpack(row):
    row, out, at = [int(t) for t in row], [], 1
    for _ in range(row[0]):
        end = row.index(0, at)
        out.append(row[at:end])
        at = end + 1
    return out


def check(out):
    """The fixture's conditions, on the dict that is (or was) written to the file."""
    settings = ast.literal_eval(str(out["meta/settings"]))
    hyps = lambda name, b: [out["gen/%s/b%d/r%d/tokens" % (name, b, r)].tolist() for r in range(int(out["gen/%s/b%d/n" % (name, b)]))]
    seen = 0
    for name, kw in settings.items():
        if "constraints" not in kw:
            continue
        packed = out["meta/constraints/" + name]
        for b in range(B):
            cons = unpack(packed[b])
            if not cons:  # the unconstrained sentence: the baseline's hypotheses, bit for bit
                assert hyps(name, b) == hyps(kw["base"], b), (name, b)
                for r in range(int(out["gen/%s/b%d/n" % (name, b)])):
                    for part in ("score", "pos_scores"):
                        assert np.array_equal(out["gen/%s/b%d/r%d/%s" % (name, b, r, part)], out["gen/%s/b%d/r%d/%s" % (kw["base"], b, r, part)])
                continue
            seen += 1
            assert hyps(name, b), (name, b)
            for h in hyps(name, b):
                assert holds(h[:-1], cons, kw["constraints"] == "ordered"), (name, b, h, cons)
                assert not holds(hyps(kw["base"], b)[0][:-1], cons[:1], True), (name, b)  # the baseline's best does not hold them
            assert hyps(name, b)[0] != hyps(kw["base"], b)[0], (name, b)
    assert seen == 6


def main():
    from fairseq import search
    from fairseq.models.chimera.w2v2_transformer_interlingua import S2TTransformerInterlinguaModelW2V2
    from fairseq.sequence_generator import SequenceGenerator
    from fairseq.token_generation_constraints import pack_constraints

    g = np.load(os.path.join(MG.OUT, "decode_tiny.npz"), allow_pickle=False)
    con = np.load(os.path.join(MG.OUT, "decode_constraints_tiny.npz"), allow_pickle=False)
    rec = np.load(os.path.join(MG.OUT, "decode_recipe_tiny.npz"), allow_pickle=False)
    d = MG.make_dictionary()
    assert d.eos() == EOS and d.pad() == PAD
    task = MG.TaskStub(d)
    with tempfile.TemporaryDirectory() as tmp:
        w2v_path = os.path.join(tmp, "w2v_tiny.pt")
        MG.build_w2v_ckpt(w2v_path, seed=11)
        torch.manual_seed(12)
        unfitted = S2TTransformerInterlinguaModelW2V2.build_model(MG.model_args(w2v_path), task)
    sdu = {k[len("param/"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param/")}
    for k in con.files:
        if k.startswith("unfitted/param/"):
            assert k[len("unfitted/param/"):] in sdu
            sdu[k[len("unfitted/param/"):]] = torch.from_numpy(con[k].astype(np.float32))
    missing, unexpected = unfitted.load_state_dict(sdu, strict=False)
    assert not unexpected and all("_float_tensor" in k or k == "decoder.version" for k in missing), (missing, unexpected)
    unfitted.eval()

    src, lens = torch.from_numpy(rec["in/b/src_tokens"]), torch.from_numpy(rec["in/b/src_lengths"])
    assert src.size(0) == B
    out = {"meta/settings": np.array(repr(SETTINGS))}
    best = {}
    for name, kw in SETTINGS.items():  # (the baselines come first)
        strategy, packed = None, None
        if "constraints" in kw:
            strategy = search.LexicallyConstrainedBeamSearch(d, kw["constraints"])
            cons = constraints_for(kw["constraints"], best[kw["base"]][0], best[kw["base"]][2], len(d))
            packed = pack_constraints([[torch.tensor(c) for c in sent] for sent in cons])
            out["meta/constraints/" + name] = packed.numpy().astype(np.int64)
        gen = SequenceGenerator([unfitted], d, beam_size=kw["beam_size"], max_len_a=0, max_len_b=kw["max_len_b"],
                                no_repeat_ngram_size=kw.get("no_repeat_ngram_size", 0), temperature=kw.get("temperature", 1.0),
                                search_strategy=strategy)
        with torch.no_grad():
            hyps = gen.generate([unfitted], {"net_input": {"src_tokens": src, "src_lengths": lens}}, constraints=packed)
        best[name] = [h[0]["tokens"].tolist() for h in hyps]
        for b, h in enumerate(hyps):
            out["gen/%s/b%d/n" % (name, b)] = np.int64(len(h))
            for r, hyp in enumerate(h):
                key = "gen/%s/b%d/r%d/" % (name, b, r)
                out[key + "tokens"] = hyp["tokens"].numpy()
                out[key + "score"] = np.float64(float(hyp["score"]))
                out[key + "pos_scores"] = hyp["positional_scores"].numpy()
            print(name, b, "n", len(h), [hyp["tokens"].tolist() for hyp in h], "%.4f" % float(h[0]["score"]))
        if packed is not None:
            print(name, "constraints", packed.tolist())
    check(out)
    path = os.path.join(MG.OUT, "decode_lexical_tiny.npz")
    np.savez_compressed(path, **out)
    print("wrote decode_lexical_tiny.npz: %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
