#!/usr/bin/env python3
"""tests/golden/decode_sampling_tiny.npz — the REAL reference's `Sampling` search strategy (search.py:621-742, imported from
/root/reference through ref_import.py), in the two places where it is deterministic.

Build container only:   python tools/ref_harness/make_decode_sampling_goldens.py
Holds data only — recorded inputs and the reference's outputs, never reference source.

Part 1, the kept sets.  ROWS log-probability rows (V = 60, fp32; recorded in the file): log-softmax of seeded logits, a third of them
  peaked (six tokens far above unit noise), a third moderately peaked, a third nearly flat.
    topp/p<p>/indices, probs   what Sampling._sample_topp(rows) returns at p in {0.3, 0.9, 0.999}: the descending order truncated to the
                               widest row, and the probabilities with everything outside a row's nucleus set to 0
    topk/k<k>/indices          lprobs.topk(k) of the rows at k in {1, 8} (what Sampling.step samples among)
  No row has two equal values anywhere (asserted), so no cut falls on a tie and the sets do not depend on the sort's tie order.
Part 2, the generator.  SequenceGenerator(search_strategy=Sampling(...)) on the tiny Chimera model of decode_tiny.npz and the three
  "b" utterances of decode_recipe_tiny.npz, beam 3, max_len_b 12, at sampling_topk = 1 and at sampling_topp = 1e-6.  Both keep exactly
  one token per row, so torch.multinomial has no choice and nothing needs patching: every finalized hypothesis is recorded."""
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ref_import import import_reference  # noqa: E402

import_reference()
import make_goldens as MG  # noqa: E402

ROWS, V = 36, 60
TOPP, TOPK = (0.3, 0.9, 0.999), (1, 8)
SETTINGS = {"topk1": dict(sampling_topk=1), "topp1e-6": dict(sampling_topp=1e-6)}
BEAM, MAX_LEN_B = 3, 12


def recorded_rows():
    g = torch.Generator().manual_seed(20261)
    x = torch.randn(ROWS, V, generator=g)
    hot = [5, 9, 17, 33, 41, 50]
    for r in range(ROWS):
        if r % 3 == 0:
            x[r, hot] = 14.0 - torch.arange(6, dtype=torch.float32) + torch.randn(6, generator=g)
        elif r % 3 == 1:
            x[r] *= 2.5
        else:
            x[r] *= 0.3
    lp = torch.log_softmax(x, dim=-1)
    for r in range(ROWS):
        assert len(set(lp[r].tolist())) == V and len(set(lp[r].exp().tolist())) == V, "a tie in row %d" % r
    return lp


def main():
    from fairseq.models.chimera.w2v2_transformer_interlingua import S2TTransformerInterlinguaModelW2V2
    from fairseq.search import Sampling
    from fairseq.sequence_generator import SequenceGenerator

    d = MG.make_dictionary()
    out = {}
    # ---- part 1 ----
    lp = recorded_rows()
    out["rows"] = lp.numpy()
    for p in TOPP:
        probs, idx = Sampling(d, sampling_topp=p)._sample_topp(lp.clone().view(ROWS, 1, V))
        out["topp/p%g/indices" % p] = idx.view(ROWS, -1).numpy()
        out["topp/p%g/probs" % p] = probs.view(ROWS, -1).numpy()
        n = (probs.view(ROWS, -1) > 0).sum(1)
        print("top-p %g: nucleus sizes min %d median %d max %d" % (p, int(n.min()), int(n.median()), int(n.max())))
    for k in TOPK:
        out["topk/k%d/indices" % k] = lp.topk(k)[1].numpy()
    # ---- part 2 ----
    g = np.load(os.path.join(MG.OUT, "decode_tiny.npz"), allow_pickle=False)
    rec = np.load(os.path.join(MG.OUT, "decode_recipe_tiny.npz"), allow_pickle=False)
    task = MG.TaskStub(d)
    with tempfile.TemporaryDirectory() as tmp:
        w2v_path = os.path.join(tmp, "w2v_tiny.pt")
        MG.build_w2v_ckpt(w2v_path, seed=11)
        torch.manual_seed(12)
        model = S2TTransformerInterlinguaModelW2V2.build_model(MG.model_args(w2v_path), task)
    sd = {k[len("param/"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param/")}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all("_float_tensor" in k or k == "decoder.version" for k in missing), (missing, unexpected)
    model.eval()
    src, lens = torch.from_numpy(rec["in/b/src_tokens"]), torch.from_numpy(rec["in/b/src_lengths"])
    out["in/src_tokens"], out["in/src_lengths"] = src.numpy(), lens.numpy()
    out["meta/settings"] = np.array(repr(SETTINGS))
    out["meta/beam"], out["meta/max_len_b"] = np.int64(BEAM), np.int64(MAX_LEN_B)
    for name, kw in SETTINGS.items():
        gen = SequenceGenerator([model], d, beam_size=BEAM, max_len_a=0, max_len_b=MAX_LEN_B, search_strategy=Sampling(d, **kw))
        with torch.no_grad():
            hyps = gen.generate([model], {"net_input": {"src_tokens": src, "src_lengths": lens}})
        for b, h in enumerate(hyps):
            out["gen/%s/b%d/n" % (name, b)] = np.int64(len(h))
            assert len(h) == BEAM and all(x["tokens"].tolist() == h[0]["tokens"].tolist() for x in h), (name, b)
            for r, hyp in enumerate(h):
                key = "gen/%s/b%d/r%d/" % (name, b, r)
                out[key + "tokens"] = hyp["tokens"].numpy()
                out[key + "score"] = np.float64(float(hyp["score"]))
                out[key + "pos_scores"] = hyp["positional_scores"].numpy()
            print(name, b, "n", len(h), h[0]["tokens"].tolist(), "%.4f" % float(h[0]["score"]))
    path = os.path.join(MG.OUT, "decode_sampling_tiny.npz")
    np.savez_compressed(path, **out)
    print("wrote decode_sampling_tiny.npz: %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
