#!/usr/bin/env python3
"""tests/golden/decode_ensemble_tiny.npz — checkpoint ENSEMBLES decoded by the REAL reference's SequenceGenerator
(`--path a.pt:b.pt:c.pt`: EnsembleModel.forward_decoder, sequence_generator.py:806-868 — per member the last position's logits
/ temperature -> fp32 log-softmax, then logsumexp over the members - log N), imported through ref_import.py.

Build container only:   python tools/ref_harness/make_decode_ensemble_goldens.py
Holds data only — the members' parameters and the generator's outputs, never reference source.

Member 0 is the fitted tiny Chimera model of decode_tiny.npz (its parameters stay in that fixture).  Members 1 and 2 are derived
from it deterministically: every floating-point tensor under PERTURB gets seeded Gaussian noise of NOISE x that tensor's own
standard deviation and is rounded to a value float16 holds exactly; only those tensors are stored (as float16; a member's other
tensors are member 0's).  The inputs are the "a" and "b" utterances of decode_recipe_tiny.npz (not stored again).

Settings, each for N = 2 (members 0, 1) and N = 3 (members 0, 1, 2):
  beam5         beam 5, defaults
  recipe        beam 10, len_penalty 1.5                       <- the final recipe
  temp          beam 5, temperature 0.7
Keys: member<k>/param/<name>;  own/gen/<setting>/<tag>/b<i>/r0/tokens (member 0 decoded alone);  n<N>/gen/<setting>/<tag>/b<i>/n  and  .../r<j>/{tokens, score, pos_scores}  (the recipe fixture's layout).

Before anything is written the script asserts that the fixture cannot hide a failure:
  * for each N the ensemble's best hypothesis differs in token ids from member 0's own on some utterance of a + b;
  * under temperature 0.7 some hypothesis' score differs by > 1e-3 from "temperature applied after averaging";
  * within every sentence no two finalized scores are closer than 1e-3, and at every step the last kept and the first dropped
    candidate of the top-2*beam are more than 1e-4 apart (recomputed with plain torch from the members' step log-probabilities),
    so exact token ids do not hang on fp32 summation order.
If a seed fails a condition, change the seed, not the condition."""
import copy
import math
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ref_import import import_reference  # noqa: E402

import_reference()
import make_goldens as MG  # noqa: E402

SETTINGS = {
    "beam5": dict(beam_size=5),
    "recipe": dict(beam_size=10, len_penalty=1.5),
    "temp": dict(beam_size=5, temperature=0.7),
}
SEEDS = {1: 1014, 2: 2007}  # found by trying 1001.., 2001.. in turn against the conditions below
NOISE = 0.3
# what differs between the members: the interlingua (memory) layers and the final LayerNorm of the encoder — so every member has
# its OWN encoder output — and the whole decoder.  The speech front end stays member 0's: two full models would not fit the
# repository's size limit for one file.
PERTURB = ("encoder.interlingua_layers.", "encoder.layer_norm.", "decoder.")
MAX_LEN_B = 12


def perturbed(model, seed, noise):
    m = copy.deepcopy(model)
    gen = torch.Generator().manual_seed(seed)
    done = set()
    with torch.no_grad():
        for k, v in sorted(m.state_dict().items()):
            if k.startswith(PERTURB) and v.is_floating_point() and v.numel() > 1 and v.data_ptr() not in done:
                done.add(v.data_ptr())  # (tied tensors once)
                v.add_(torch.randn(v.shape, generator=gen) * (noise * float(v.std())))
                v.copy_(v.half().float())  # values a float16 holds exactly: the fixture stores them in half the bytes
    return m.eval()


def search(lp_fn, B, beam, max_len, len_penalty=1.0, pad=1, eos=2, unk=3):
    """Plain-torch restatement of the reference's beam search (min_len 1, normalised scores) over
    lp_fn(sentence, tokens[beam, step + 1]) -> [beam, V]; also returns the smallest gap between the last kept and the first
    dropped candidate of any step's top-2*beam."""
    results, min_gap = [], math.inf
    for b in range(B):
        tokens = torch.full((beam, max_len + 2), pad, dtype=torch.long)
        tokens[:, 0] = eos
        scores = torch.zeros(beam, max_len + 1)
        fin = []
        for step in range(max_len + 1):
            lp = lp_fn(b, tokens[:, :step + 1]).clone()
            lp[lp != lp] = -math.inf
            lp[:, pad] = -math.inf
            if step >= max_len:
                lp[:, :eos] = -math.inf
                lp[:, eos + 1:] = -math.inf
            if step < 1:
                lp[:, eos] = -math.inf
            V = lp.size(-1)
            cand = lp[0:1] if step == 0 else lp + scores[:, step - 1].unsqueeze(-1)
            top_s, top_i = torch.topk(cand.reshape(-1), k=2 * beam + 1)
            if top_s[2 * beam] != -math.inf:
                min_gap = min(min_gap, float(top_s[2 * beam - 1] - top_s[2 * beam]))
            top_s, top_i = top_s[:2 * beam], top_i[:2 * beam]
            beams, idx = top_i // V, top_i.fmod(V)
            eos_mask = idx.eq(eos) & top_s.ne(-math.inf)
            for j in range(beam):
                if eos_mask[j] and len(fin) < beam:
                    bi = int(beams[j])
                    fin.append(dict(tokens=torch.cat([tokens[bi, 1:step + 1], torch.tensor([eos])]),
                                    score=float(top_s[j]) / ((step + 1) ** len_penalty)))
            if len(fin) >= beam or step >= max_len:
                break
            keep = [j for j in range(2 * beam) if not eos_mask[j]][:beam]
            kb = beams[keep]
            new_tokens, new_scores = tokens[kb].clone(), scores[kb].clone()
            new_tokens[:, step + 1] = idx[keep]
            new_scores[:, step] = top_s[keep]
            tokens, scores = new_tokens, new_scores
        fin.sort(key=lambda h: -h["score"])
        results.append(fin)
    return results, min_gap


def main(seeds=SEEDS, noise=NOISE, write=True, only_n=(2, 3)):
    from fairseq.models.chimera.w2v2_transformer_interlingua import S2TTransformerInterlinguaModelW2V2
    from fairseq.sequence_generator import SequenceGenerator

    g = np.load(os.path.join(MG.OUT, "decode_tiny.npz"), allow_pickle=False)
    rec = np.load(os.path.join(MG.OUT, "decode_recipe_tiny.npz"), allow_pickle=False)
    d = MG.make_dictionary()
    task = MG.TaskStub(d)
    with tempfile.TemporaryDirectory() as tmp:
        w2v_path = os.path.join(tmp, "w2v_tiny.pt")
        MG.build_w2v_ckpt(w2v_path, seed=11)
        torch.manual_seed(12)
        m0 = S2TTransformerInterlinguaModelW2V2.build_model(MG.model_args(w2v_path), task)
    sd = {k[len("param/"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param/")}
    missing, unexpected = m0.load_state_dict(sd, strict=False)
    assert not unexpected and all("_float_tensor" in k or k == "decoder.version" for k in missing), (missing, unexpected)
    m0.eval()
    with torch.no_grad():  # the loaded model must BE the one decode_tiny.npz was made with
        (logits, _), _ = m0.forward_with_internal(torch.from_numpy(g["in/src_tokens"]), torch.from_numpy(g["in/src_lengths"]),
                                                  torch.from_numpy(g["in/prev_output_tokens"]))
    assert float((logits - torch.from_numpy(g["out/st_logits"])).abs().max()) < 1e-5
    members = [m0, perturbed(m0, seeds[1], noise), perturbed(m0, seeds[2], noise)]

    out = {"meta/settings": np.array(repr(SETTINGS)), "meta/max_len_b": np.int64(MAX_LEN_B), "meta/noise": np.float64(noise),
           "meta/seeds": np.array(repr(seeds))}
    sd0 = m0.state_dict()
    for k in (1, 2):  # only the tensors that differ from member 0's (the rest is read from decode_tiny.npz)
        for name, v in members[k].state_dict().items():
            if not torch.equal(v, sd0[name]):
                assert torch.equal(v.half().float(), v)
                out["member%d/param/%s" % (k, name)] = v.detach().cpu().half().numpy()

    inputs = {tag: (torch.from_numpy(rec["in/%s/src_tokens" % tag]), torch.from_numpy(rec["in/%s/src_lengths" % tag])) for tag in ("a", "b")}
    for N in only_n:
        ens = members[:N]
        differs = False
        for name, kw in SETTINGS.items():
            temp_differs = 0.0
            for tag, (src, lens) in inputs.items():
                net = {"src_tokens": src, "src_lengths": lens}
                with torch.no_grad():
                    hyps = SequenceGenerator(ens, d, max_len_a=0, max_len_b=MAX_LEN_B, min_len=1, **kw).generate(ens, {"net_input": net})
                    own = SequenceGenerator([m0], d, max_len_a=0, max_len_b=MAX_LEN_B, min_len=1, **kw).generate([m0], {"net_input": net})
                    encs = [m.encoder.forward_torchscript(net) for m in ens]
                for b, h in enumerate(hyps):
                    sc = sorted(float(x["score"]) for x in h)
                    assert all(y - x > 1e-3 for x, y in zip(sc, sc[1:])), ("finalized scores too close", N, name, tag, b, sc)
                beam, T = kw["beam_size"], kw.get("temperature", 1.0)

                def member_lps(b, tokens):
                    lps = []
                    for m, enc in zip(ens, encs):
                        e = m.encoder.reorder_encoder_out(enc, torch.full((tokens.size(0),), b, dtype=torch.long))
                        with torch.no_grad():
                            lg = m.decoder(tokens, encoder_out=e)[0][:, -1, :].float()
                        lps.append(lg)
                    return torch.stack(lps, 0)

                def lp_ref(b, tokens):
                    return torch.logsumexp(torch.log_softmax(member_lps(b, tokens) / T, -1), 0) - math.log(N)

                def lp_after(b, tokens):  # the WRONG order: average the T = 1 distributions, then apply the temperature
                    avg = torch.logsumexp(torch.log_softmax(member_lps(b, tokens), -1), 0) - math.log(N)
                    return torch.log_softmax(avg / T, -1)

                mine, gap = search(lp_ref, src.size(0), beam, MAX_LEN_B, kw.get("len_penalty", 1.0))
                assert gap > 1e-4, ("top-2*beam boundary gap", N, name, tag, gap)
                if T != 1.0:
                    alt, _ = search(lp_after, src.size(0), beam, MAX_LEN_B, kw.get("len_penalty", 1.0))
                for b, h in enumerate(hyps):
                    out["n%d/gen/%s/%s/b%d/n" % (N, name, tag, b)] = np.int64(len(h))
                    assert len(mine[b]) == len(h)
                    for r, hyp in enumerate(h):
                        key = "n%d/gen/%s/%s/b%d/r%d/" % (N, name, tag, b, r)
                        out[key + "tokens"] = hyp["tokens"].numpy()
                        out[key + "score"] = np.float64(float(hyp["score"]))
                        out[key + "pos_scores"] = hyp["positional_scores"].numpy()
                        # the plain-torch restatement used for the conditions IS the reference's search
                        assert mine[b][r]["tokens"].tolist() == hyp["tokens"].tolist(), (key, mine[b][r]["tokens"], hyp["tokens"])
                        assert abs(mine[b][r]["score"] - float(hyp["score"])) < 1e-4, key
                        if T != 1.0 and r < len(alt[b]):
                            temp_differs = max(temp_differs, abs(alt[b][r]["score"] - float(hyp["score"])))
                    differs = differs or h[0]["tokens"].tolist() != own[b][0]["tokens"].tolist()
                    out["own/gen/%s/%s/b%d/r0/tokens" % (name, tag, b)] = own[b][0]["tokens"].numpy()  # member 0 ALONE: what must not pass
                    print(N, name, tag, b, "n", len(h), "best", h[0]["tokens"].tolist(), "%.4f" % float(h[0]["score"]),
                          "| member 0 alone", own[b][0]["tokens"].tolist(), "| gap %.2e" % gap)
            if kw.get("temperature", 1.0) != 1.0:
                print(N, name, "max score difference to temperature-after-averaging: %.4f" % temp_differs)
                assert temp_differs > 1e-3, ("temperature order not observable", N, temp_differs)
        assert differs, ("the ensemble's best hypotheses equal member 0's own", N)
    if not write:
        return
    np.savez_compressed(os.path.join(MG.OUT, "decode_ensemble_tiny.npz"), **out)
    print("wrote decode_ensemble_tiny.npz: %d bytes" % os.path.getsize(os.path.join(MG.OUT, "decode_ensemble_tiny.npz")))


if __name__ == "__main__":
    main()
