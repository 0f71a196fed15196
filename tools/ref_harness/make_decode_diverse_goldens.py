#!/usr/bin/env python3
"""tests/golden/decode_diverse_tiny.npz — the REAL reference's SequenceGenerator (imported through ref_import.py)
with its two diverse search strategies: `DiverseBeamSearch` (search.py:551-618: --diverse-beam-groups, --diverse-beam-strength) and
`DiverseSiblingsSearch` (search.py:745-814: --diversity-rate).

Build container only:   python tools/ref_harness/make_decode_diverse_goldens.py
Holds data only — settings and the generator's outputs (token ids, scores, positional scores), never reference source.  Model parameters
and audio are those of other fixtures and are NOT stored again:
  fitted    the tiny Chimera model of decode_tiny.npz;
  unfitted  the same with the "unfitted/param/" tensors of decode_constraints_tiny.npz (it loops, so n-gram blocking has work to do);
  audio     the three "b" utterances of decode_recipe_tiny.npz ("in/b/src_tokens", "in/b/src_lengths").

Settings (all finalized hypotheses of every sentence, in the reference's order), each next to its plain-beam baseline:
  base_b4, base_b5, base_b6   unfitted, temperature 2, beam 4 / 5 / 6, max_len_b 12
  g2, g4                      beam 4, 2 / 4 groups, strength 0.5                         <- base_b4
  g3                          beam 6, 3 groups, strength 0.3 (products not exact in fp32) <- base_b6
  sib4                        beam 4, diversity rate 0.5                                 <- base_b4
  sib5                        beam 5, diversity rate 0.3                                 <- base_b5
  base_ngram2 / g2_ngram2     unfitted, beam 4, max_len_b 16, no_repeat_ngram_size 2 / + 2 groups, strength 0.5
  base_prefix / g2_prefix     fitted, beam 4, prefix [[7, 9, 11], [8, eos, pad], [13, pad, pad]] / + 2 groups, strength 0.5
Why temperature 2 on the unfitted model: at temperature 1 both models are so sure of their next token that a penalty of 0.5 never
changes a group's first token (the fitted model's four groups of one beam then all find the SAME hypothesis: fewer distinct first tokens
than plain beam search, 1 against 2).  With the flatter distributions the reference's diverse searches do what they are for.
Conditions (check()): in every sentence a diverse setting's SET of hypotheses differs from its baseline's — except g2_prefix in the
sentence whose prefix holds eos, where every search can only return `beam` copies of the forced prefix (asserted instead); and for
g2 and g4 (strength 0.5, free first token) the number of distinct first tokens is at least the baseline's in every sentence and larger
in at least one.
The conditions asserted by check() are re-asserted on the committed file by tests/test_decode_diverse_cpu.py."""
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ref_import import import_reference  # noqa: E402

import_reference()
import make_goldens as MG  # noqa: E402

EOS, PAD = 2, 1
PREFIX = [[7, 9, 11], [8, EOS, PAD], [13, PAD, PAD]]
SETTINGS = {
    "base_b4": dict(model="unfitted", temperature=2.0, beam_size=4, max_len_b=12),
    "base_b5": dict(model="unfitted", temperature=2.0, beam_size=5, max_len_b=12),
    "base_b6": dict(model="unfitted", temperature=2.0, beam_size=6, max_len_b=12),
    "g2": dict(model="unfitted", temperature=2.0, beam_size=4, max_len_b=12, groups=2, strength=0.5, base="base_b4"),
    "g4": dict(model="unfitted", temperature=2.0, beam_size=4, max_len_b=12, groups=4, strength=0.5, base="base_b4"),
    "g3": dict(model="unfitted", temperature=2.0, beam_size=6, max_len_b=12, groups=3, strength=0.3, base="base_b6"),
    "sib4": dict(model="unfitted", temperature=2.0, beam_size=4, max_len_b=12, rate=0.5, base="base_b4"),
    "sib5": dict(model="unfitted", temperature=2.0, beam_size=5, max_len_b=12, rate=0.3, base="base_b5"),
    "base_ngram2": dict(model="unfitted", beam_size=4, max_len_b=16, no_repeat_ngram_size=2),
    "g2_ngram2": dict(model="unfitted", beam_size=4, max_len_b=16, no_repeat_ngram_size=2, groups=2, strength=0.5, base="base_ngram2"),
    "base_prefix": dict(model="fitted", beam_size=4, max_len_b=12, prefix=True),
    "g2_prefix": dict(model="fitted", beam_size=4, max_len_b=12, prefix=True, groups=2, strength=0.5, base="base_prefix"),
}
FIRST_TOKEN_SETTINGS = ("g2", "g4")  # the group settings with strength 0.5 and a free first token


def check(out, settings=SETTINGS, B=len(PREFIX)):
    """The fixture's conditions, on the dict that is (or was) written to the file."""
    hyps = lambda name, b: [out["gen/%s/b%d/r%d/tokens" % (name, b, r)].tolist() for r in range(int(out["gen/%s/b%d/n" % (name, b)]))]
    for name, kw in settings.items():
        if "base" not in kw:
            continue
        for b in range(B):  # a diverse search finds another SET of hypotheses than its baseline, in every sentence
            if kw.get("prefix") and EOS in PREFIX[b]:  # (eos inside the forced prefix: `beam` copies of it, whatever the search)
                forced = PREFIX[b][:PREFIX[b].index(EOS) + 1]
                assert hyps(name, b) == hyps(kw["base"], b) == [forced] * kw["beam_size"], (name, b)
                continue
            assert set(map(tuple, hyps(name, b))) != set(map(tuple, hyps(kw["base"], b))), (name, b)
    for name in FIRST_TOKEN_SETTINGS:
        firsts = lambda n, b: len(set(h[0] for h in hyps(n, b)))
        pairs = [(firsts(name, b), firsts(settings[name]["base"], b)) for b in range(B)]
        assert all(d >= p for d, p in pairs) and any(d > p for d, p in pairs), (name, pairs)


def main():
    from fairseq import search
    from fairseq.models.chimera.w2v2_transformer_interlingua import S2TTransformerInterlinguaModelW2V2
    from fairseq.sequence_generator import SequenceGenerator

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
        fitted = S2TTransformerInterlinguaModelW2V2.build_model(MG.model_args(w2v_path), task)
        torch.manual_seed(12)
        unfitted = S2TTransformerInterlinguaModelW2V2.build_model(MG.model_args(w2v_path), task)
    sd = {k[len("param/"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param/")}
    sdu = dict(sd)
    for k in con.files:
        if k.startswith("unfitted/param/"):
            assert k[len("unfitted/param/"):] in sdu
            sdu[k[len("unfitted/param/"):]] = torch.from_numpy(con[k].astype(np.float32))
    for model, state in ((fitted, sd), (unfitted, sdu)):
        missing, unexpected = model.load_state_dict(state, strict=False)
        assert not unexpected and all("_float_tensor" in k or k == "decoder.version" for k in missing), (missing, unexpected)
        model.eval()
    with torch.no_grad():  # the loaded model must BE the one decode_tiny.npz was made with
        (logits, _), _ = fitted.forward_with_internal(torch.from_numpy(g["in/src_tokens"]), torch.from_numpy(g["in/src_lengths"]),
                                                      torch.from_numpy(g["in/prev_output_tokens"]))
    assert float((logits - torch.from_numpy(g["out/st_logits"])).abs().max()) < 1e-5
    models = {"fitted": fitted, "unfitted": unfitted}

    src, lens = torch.from_numpy(rec["in/b/src_tokens"]), torch.from_numpy(rec["in/b/src_lengths"])
    assert src.size(0) == len(PREFIX)
    out = {"meta/settings": np.array(repr(SETTINGS)), "meta/prefix": np.array(PREFIX, dtype=np.int64)}
    prefix = torch.tensor(PREFIX, dtype=torch.long)
    for name, kw in SETTINGS.items():
        model = models[kw["model"]]
        strategy = None
        if "groups" in kw:
            strategy = search.DiverseBeamSearch(d, kw["groups"], kw["strength"])
        elif "rate" in kw:
            strategy = search.DiverseSiblingsSearch(d, kw["rate"])
        gen = SequenceGenerator([model], d, beam_size=kw["beam_size"], max_len_a=0, max_len_b=kw["max_len_b"],
                                no_repeat_ngram_size=kw.get("no_repeat_ngram_size", 0), temperature=kw.get("temperature", 1.0),
                                search_strategy=strategy)
        with torch.no_grad():
            hyps = gen.generate([model], {"net_input": {"src_tokens": src, "src_lengths": lens}},
                                prefix_tokens=prefix if kw.get("prefix") else None)
        for b, h in enumerate(hyps):
            out["gen/%s/b%d/n" % (name, b)] = np.int64(len(h))
            for r, hyp in enumerate(h):
                key = "gen/%s/b%d/r%d/" % (name, b, r)
                out[key + "tokens"] = hyp["tokens"].numpy()
                out[key + "score"] = np.float64(float(hyp["score"]))
                out[key + "pos_scores"] = hyp["positional_scores"].numpy()
            print(name, b, "n", len(h), [hyp["tokens"].tolist() for hyp in h], "%.4f" % float(h[0]["score"]))
    hyps = lambda name, b: [out["gen/%s/b%d/r%d/tokens" % (name, b, r)].tolist() for r in range(int(out["gen/%s/b%d/n" % (name, b)]))]
    for name, kw in SETTINGS.items():
        if "base" in kw:
            print(name, "per sentence (set differs from %s, distinct first tokens, baseline's):" % kw["base"],
                  [(set(map(tuple, hyps(name, b))) != set(map(tuple, hyps(kw["base"], b))), len(set(h[0] for h in hyps(name, b))),
                    len(set(h[0] for h in hyps(kw["base"], b)))) for b in range(len(PREFIX))])
    check(out)
    path = os.path.join(MG.OUT, "decode_diverse_tiny.npz")
    np.savez_compressed(path, **out)
    print("wrote decode_diverse_tiny.npz: %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
