#!/usr/bin/env python3
"""tests/golden/decode_attention_tiny.npz — the `attention` of every finalised hypothesis (sequence_generator.py:349-355, :523-526,
:609-611, :664-674: the last decoder layer's cross attention, averaged over the heads, one column per emitted token) as the REAL
reference's SequenceGenerator returns it, imported through ref_import.py.

Build container only:   python tools/ref_harness/make_decode_attention_goldens.py
Holds data only — inputs and the generator's outputs (token ids, scores, attention matrices), never reference source.

The reference's speech decoders drop the attention (TransformerDecoderScriptable.extract_features returns `x, None`), so its generator
yields an empty tensor for them.  The base class keeps it: here every model's decoder gets
    decoder.extract_features = types.MethodType(TransformerDecoder.extract_features, decoder)
and the same generator then returns fp32 [src_len, n] matrices.  Those are the semantics recorded: the reference generator's over the
reference base decoder's attention.

Cases (keys <case>/<tag>/beam<k>/b<i>/n and .../r<j>/{tokens, score, attention}; inputs in/<case>/<tag>/{src_tokens, src_lengths}):
  chimera   the fitted tiny Chimera model of decode_tiny.npz on the utterance sets "a" and "b" of make_decode_recipe_goldens.py, beam 1
            and beam 5, max_len_b 12.  The source axis is the 8 memory slots.
  padded    the s2t_transformer_w2v2 model and audio of s2t_w2v2_tiny.npz (3 utterances of 3600 / 3000 / 1700 samples -> 23 encoder
            frames with 0 / 4 / 12 padded), beam 5: the padded source rows are exactly 0.  <case>/<tag>/b<i>/src_valid = valid frames.
  ens2      members 0 and 1 of decode_ensemble_tiny.npz (member 1 re-derived by that fixture's script and checked against its stored
            tensors), sets "a" and "b", beam 5: the members' attention summed / 2.
Printed per case: the smallest gap between the two largest entries of a column, and how many columns fall under 4e-4 (the cap the tests
leave out of the hard-alignment comparison)."""
import os
import sys
import tempfile
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ref_import import import_reference  # noqa: E402

import_reference()
import make_decode_ensemble_goldens as ME  # noqa: E402
import make_goldens as MG  # noqa: E402

MAX_LEN_B = 12
GAP = 4e-4


def bind_base_attention(model):
    from fairseq.models.transformer import TransformerDecoder

    model.decoder.extract_features = types.MethodType(TransformerDecoder.extract_features, model.decoder)
    return model


def load_params(model, g):
    sd = {k[len("param/"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param/")}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all("_float_tensor" in k or k == "decoder.version" for k in missing), (missing, unexpected)
    return model.eval()


def record(out, case, tag, beam, models, d, src, lens, valid=None):
    from fairseq.sequence_generator import SequenceGenerator

    gen = SequenceGenerator(models, d, beam_size=beam, max_len_a=0, max_len_b=MAX_LEN_B, min_len=1)
    with torch.no_grad():
        hyps = gen.generate(models, {"net_input": {"src_tokens": src, "src_lengths": lens}})
    gaps = []
    for b, h in enumerate(hyps):
        out["%s/%s/beam%d/b%d/n" % (case, tag, beam, b)] = np.int64(len(h))
        for r, hyp in enumerate(h):
            key = "%s/%s/beam%d/b%d/r%d/" % (case, tag, beam, b, r)
            att = hyp["attention"].float()
            assert att.dim() == 2 and att.size(1) == len(hyp["tokens"]), (key, att.shape)
            assert float((att.sum(0) - 1).abs().max()) < 1e-6, key
            if valid is not None:
                assert bool((att[valid[b]:] == 0).all()), key
            out[key + "tokens"] = hyp["tokens"].numpy()
            out[key + "score"] = np.float64(float(hyp["score"]))
            out[key + "attention"] = att.numpy()
            if att.size(0) > 1:
                top = torch.topk(att, 2, dim=0).values
                gaps += (top[0] - top[1]).tolist()
    return gaps


def main():
    from fairseq.models.chimera.w2v2_transformer import S2TTransformerModelW2V2
    from fairseq.models.chimera.w2v2_transformer_interlingua import S2TTransformerInterlinguaModelW2V2

    g = np.load(os.path.join(MG.OUT, "decode_tiny.npz"), allow_pickle=False)
    rec = np.load(os.path.join(MG.OUT, "decode_recipe_tiny.npz"), allow_pickle=False)
    ens = np.load(os.path.join(MG.OUT, "decode_ensemble_tiny.npz"), allow_pickle=False)
    s2t = np.load(os.path.join(MG.OUT, "s2t_w2v2_tiny.npz"), allow_pickle=False)
    d = MG.make_dictionary()
    task = MG.TaskStub(d)
    with tempfile.TemporaryDirectory() as tmp:
        w2v_path = os.path.join(tmp, "w2v_tiny.pt")
        MG.build_w2v_ckpt(w2v_path, seed=11)
        torch.manual_seed(12)
        m0 = load_params(S2TTransformerInterlinguaModelW2V2.build_model(MG.model_args(w2v_path), task), g)
        w2v_path2 = os.path.join(tmp, "w2v_tiny2.pt")
        MG.build_w2v_ckpt(w2v_path2, seed=21)
        torch.manual_seed(22)
        ms = load_params(S2TTransformerModelW2V2.build_model(MG.model_args(w2v_path2, encoder_layers=3), task), s2t)
    with torch.no_grad():  # the loaded model must BE the one decode_tiny.npz was made with
        (logits, _), _ = m0.forward_with_internal(torch.from_numpy(g["in/src_tokens"]), torch.from_numpy(g["in/src_lengths"]),
                                                  torch.from_numpy(g["in/prev_output_tokens"]))
    assert float((logits - torch.from_numpy(g["out/st_logits"])).abs().max()) < 1e-5
    m1 = ME.perturbed(m0, ME.SEEDS[1], ME.NOISE)
    for k in ens.files:  # member 1 IS the ensemble fixture's
        if k.startswith("member1/param/"):
            assert torch.equal(m1.state_dict()[k[len("member1/param/"):]], torch.from_numpy(ens[k]).float()), k
    for m in (m0, m1, ms):
        bind_base_attention(m)

    out = {"meta/max_len_b": np.int64(MAX_LEN_B), "meta/gap": np.float64(GAP)}
    inputs = {tag: (torch.from_numpy(rec["in/%s/src_tokens" % tag]), torch.from_numpy(rec["in/%s/src_lengths" % tag])) for tag in ("a", "b")}
    report = {}
    for tag, (src, lens) in inputs.items():
        for case in ("chimera", "ens2"):
            out["in/%s/%s/src_tokens" % (case, tag)] = src.numpy()
            out["in/%s/%s/src_lengths" % (case, tag)] = lens.numpy()
        for beam in (1, 5):
            report.setdefault("chimera", []).extend(record(out, "chimera", tag, beam, [m0], d, src, lens))
        report.setdefault("ens2", []).extend(record(out, "ens2", tag, 5, [m0, m1], d, src, lens))
    src, lens = torch.from_numpy(s2t["in/src_tokens"]), torch.from_numpy(s2t["in/src_lengths"])
    with torch.no_grad():
        enc = ms.encoder(src, lens)
    mask = enc.encoder_padding_mask
    valid = [int(enc.encoder_out.size(0) - (int(mask[b].sum()) if mask is not None else 0)) for b in range(src.size(0))]
    out["in/padded/x/src_tokens"], out["in/padded/x/src_lengths"] = src.numpy(), lens.numpy()
    for b, v in enumerate(valid):
        out["padded/x/b%d/src_valid" % b] = np.int64(v)
    report["padded"] = record(out, "padded", "x", 5, [ms], d, src, lens, valid)
    for case, gaps in report.items():
        under = sum(1 for x in gaps if x < GAP)
        print("%s: %d columns, min top-2 gap %.3e, %d under %.0e = %.1f %%" % (case, len(gaps), min(gaps), under, GAP, 100.0 * under / len(gaps)))
        assert under <= 0.05 * len(gaps), case
    path = os.path.join(MG.OUT, "decode_attention_tiny.npz")
    np.savez_compressed(path, **out)
    print("wrote decode_attention_tiny.npz: %d bytes, %d keys" % (os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
