#!/usr/bin/env python3
"""tests/golden/decode_constraints_tiny.npz — the REAL reference's SequenceGenerator (imported from /root/reference through
ref_import.py) with its two decoding constraints: `no_repeat_ngram_size` (sequence_generator.py:_no_repeat_ngram :734-767) and
`prefix_tokens` (:336-347, _prefix_tokens :543-575).

Build container only:   python tools/ref_harness/make_decode_constraints_goldens.py
Holds data only — model parameters, inputs and the generator's outputs (token ids, scores, positional scores), never reference source.

Two models:
  fitted    the tiny Chimera model of decode_tiny.npz (parameters read from that fixture).  It barely repeats: blocking changes 0 or 1 of
            its 5 hypotheses per sentence and never the best one, so it serves the PREFIX settings only.
  unfitted  the same architecture as built by torch.manual_seed(77) (never trained), values rounded to what a float16 holds exactly
            and stored under "unfitted/param/" in half the bytes.  It loops: its unconstrained best hypotheses repeat one token up to the
            length limit, so n-gram blocking changes every hypothesis.
Audio: the three "b" utterances of decode_recipe_tiny.npz (seed 31, lengths 4800 / 3520 / 2560).

Settings (all finalized hypotheses of every sentence, in the reference's order):
  base_unfitted         unfitted, beam 4, max_len_b 16                                   <- baseline of the next two
  ngram2, ngram3        + no_repeat_ngram_size 2 / 3
  base_fitted           fitted, beam 5, max_len_b 12                                     <- baseline of `prefix`
  prefix                + prefix_tokens [[7, 9, 11], [8, eos, pad], [13, pad, pad]]: full width, eos inside, shorter than the batch's width
  base_fitted_minlen    fitted, beam 5, max_len_b 12, min_len 4                          <- baseline of the next one
  prefix_ngram_minlen   + the same prefix and no_repeat_ngram_size 2 (min-len is suspended for the whole batch during the prefix steps)
The conditions asserted at the bottom are re-asserted on the committed file by tests/test_decode_constraints_cpu.py."""
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
    "base_unfitted": dict(model="unfitted", beam_size=4, max_len_b=16),
    "ngram2": dict(model="unfitted", beam_size=4, max_len_b=16, no_repeat_ngram_size=2, base="base_unfitted"),
    "ngram3": dict(model="unfitted", beam_size=4, max_len_b=16, no_repeat_ngram_size=3, base="base_unfitted"),
    "base_fitted": dict(model="fitted", beam_size=5, max_len_b=12),
    "prefix": dict(model="fitted", beam_size=5, max_len_b=12, prefix=True, base="base_fitted"),
    "base_fitted_minlen": dict(model="fitted", beam_size=5, max_len_b=12, min_len=4),
    "prefix_ngram_minlen": dict(model="fitted", beam_size=5, max_len_b=12, min_len=4, no_repeat_ngram_size=2, prefix=True,
                                base="base_fitted_minlen"),
}
UNFITTED_SEED = 77


def has_repeated_ngram(tokens, n):
    grams = [tuple(tokens[i:i + n]) for i in range(len(tokens) - n + 1)]
    return len(grams) != len(set(grams))


def prefix_of(row):
    """The tokens a hypothesis must start with: the prefix row up to its first pad; an eos ends the hypothesis there."""
    out = []
    for t in row:
        if t == PAD:
            break
        out.append(t)
        if t == EOS:
            break
    return out


def check(out, settings=SETTINGS, prefix=PREFIX):
    """The fixture's conditions, on the dict that is (or was) written to the file."""
    B = len(prefix)
    hyps = lambda name, b: [out["gen/%s/b%d/r%d/tokens" % (name, b, r)].tolist() for r in range(int(out["gen/%s/b%d/n" % (name, b)]))]
    for name, kw in settings.items():
        n = kw.get("no_repeat_ngram_size", 0)
        for b in range(B):
            for toks in hyps(name, b):
                # the n-gram windows of the reference start at the initial eos (tokens[:, 0])
                assert n == 0 or not has_repeated_ngram([EOS] + toks, n), (name, b, toks)
                if kw.get("prefix"):
                    want = prefix_of(prefix[b])
                    assert toks[:len(want)] == want, (name, b, toks, want)
        if name in ("ngram2", "ngram3"):
            changed = sum(hyps(name, b)[0] != hyps(kw["base"], b)[0] for b in range(B))
            assert changed >= 2, (name, "best hypotheses changed by blocking", changed)
    eos_row = [b for b in range(B) if EOS in prefix[b]][0]
    for name in ("prefix", "prefix_ngram_minlen"):  # eos inside the prefix: `beam` identical hypotheses
        h = hyps(name, eos_row)
        assert len(h) == settings[name]["beam_size"] and all(t == prefix_of(prefix[eos_row]) for t in h), (name, h)


def main():
    from fairseq.models.chimera.w2v2_transformer_interlingua import S2TTransformerInterlinguaModelW2V2
    from fairseq.sequence_generator import SequenceGenerator

    g = np.load(os.path.join(MG.OUT, "decode_tiny.npz"), allow_pickle=False)
    rec = np.load(os.path.join(MG.OUT, "decode_recipe_tiny.npz"), allow_pickle=False)
    d = MG.make_dictionary()
    assert d.eos() == EOS and d.pad() == PAD
    task = MG.TaskStub(d)
    with tempfile.TemporaryDirectory() as tmp:
        w2v_path = os.path.join(tmp, "w2v_tiny.pt")
        MG.build_w2v_ckpt(w2v_path, seed=11)
        torch.manual_seed(12)
        fitted = S2TTransformerInterlinguaModelW2V2.build_model(MG.model_args(w2v_path), task)
        torch.manual_seed(UNFITTED_SEED)
        unfitted = S2TTransformerInterlinguaModelW2V2.build_model(MG.model_args(w2v_path), task)
    sd = {k[len("param/"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param/")}
    missing, unexpected = fitted.load_state_dict(sd, strict=False)
    assert not unexpected and all("_float_tensor" in k or k == "decoder.version" for k in missing), (missing, unexpected)
    fitted.eval()
    with torch.no_grad():  # the loaded model must BE the one decode_tiny.npz was made with
        (logits, _), _ = fitted.forward_with_internal(torch.from_numpy(g["in/src_tokens"]), torch.from_numpy(g["in/src_lengths"]),
                                                      torch.from_numpy(g["in/prev_output_tokens"]))
    assert float((logits - torch.from_numpy(g["out/st_logits"])).abs().max()) < 1e-5

    out = {"meta/settings": np.array(repr(SETTINGS)), "meta/prefix": np.array(PREFIX, dtype=np.int64),
           "meta/unfitted_seed": np.int64(UNFITTED_SEED)}
    done = set()
    with torch.no_grad():
        for name, v in unfitted.state_dict().items():
            if name not in sd:
                continue
            if v.is_floating_point() and v.data_ptr() not in done:
                done.add(v.data_ptr())  # (tied tensors once)
                v.copy_(v.half().float())
        for name, v in unfitted.state_dict().items():
            if name in sd and not torch.equal(v, sd[name]):  # only what differs from the fitted model's (read from decode_tiny.npz)
                assert v.is_floating_point() and torch.equal(v.half().float(), v), name
                out["unfitted/param/" + name] = v.detach().cpu().half().numpy()
    unfitted.eval()
    models = {"fitted": fitted, "unfitted": unfitted}

    src, lens = torch.from_numpy(rec["in/b/src_tokens"]), torch.from_numpy(rec["in/b/src_lengths"])
    assert src.size(0) == len(PREFIX)
    out["in/src_tokens"], out["in/src_lengths"] = src.numpy(), lens.numpy()
    prefix = torch.tensor(PREFIX, dtype=torch.long)
    for name, kw in SETTINGS.items():
        model = models[kw["model"]]
        gen = SequenceGenerator([model], d, beam_size=kw["beam_size"], max_len_a=0, max_len_b=kw["max_len_b"], min_len=kw.get("min_len", 1),
                                no_repeat_ngram_size=kw.get("no_repeat_ngram_size", 0))
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
            print(name, b, "n", len(h), "best", h[0]["tokens"].tolist(), "%.4f" % float(h[0]["score"]))
            if "base" in kw:
                base_n = int(out["gen/%s/b%d/n" % (kw["base"], b)])
                changed = sum(r >= base_n or out["gen/%s/b%d/r%d/tokens" % (kw["base"], b, r)].tolist() != hyp["tokens"].tolist()
                              for r, hyp in enumerate(h))
                print("    %d of %d hypotheses differ from %s" % (changed, len(h), kw["base"]))
    check(out)
    path = os.path.join(MG.OUT, "decode_constraints_tiny.npz")
    np.savez_compressed(path, **out)
    print("wrote decode_constraints_tiny.npz: %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
