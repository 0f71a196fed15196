#!/usr/bin/env python3
"""tests/golden/decode_score_tiny.npz — given targets SCORED by the REAL reference's SequenceScorer (fairseq/sequence_scorer.py, what
`fairseq-generate --score-reference` builds, tasks/fairseq_task.py:313-320), imported through ref_import.py: the fitted tiny Chimera
model of decode_tiny.npz alone (N = 1) and as the ensembles N = 2 and N = 3 of decode_ensemble_tiny.npz (the members' parameters are
read from those two fixtures, not stored again).

Build container only:   python tools/ref_harness/make_decode_score_goldens.py
Holds data only — targets, the members' logits and the scorer's outputs, never reference source.

Inputs: the "a" and "b" utterance batches of decode_recipe_tiny.npz (not stored again).  Every utterance is scored against TWO targets:
the recipe fixture's best hypothesis (gen/recipe/<tag>/b<i>/r0/tokens) and a seeded sequence of arbitrary non-special tokens + eos of
another length (low-probability tokens occur there).  A batch is the tag's utterances with each row repeated twice,
    src_tokens = in/<tag>/src_tokens.repeat_interleave(2, 0),  rows 2i, 2i+1 = utterance i with its best hypothesis / its seeded target,
right-padded with pad, prev_output_tokens = the eos-shifted targets (data_utils.collate_tokens).

Keys:  <tag>/target, <tag>/prev_output_tokens int64 [B, T];  <tag>/logits/m<k> float32 [B, T, V], member k's decoder output;
n<N>/<tag>/pos_scores float32 [B, T] (0 at pad), n<N>/<tag>/score float32 [B], n<N>/<tag>/len int64 [B].

Before anything is written the script asserts that the fixture cannot hide a failure:
  * every batch contains at least one pad position;
  * for each N > 1 some token's ensemble score differs by more than 1e-3 from member 0's own;
  * for each N > 1 some token's ensemble score differs by more than 1e-3 from the mean of the members' LOG-probabilities;
  * some sentence's score differs by more than 1e-3 from the sum divided by T (the wrong length);
  * no reference probability underflowed: every stored score is finite.
If a seed fails a condition, change the seed, not the condition."""
import copy
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ref_import import import_reference  # noqa: E402

import_reference()
import make_goldens as MG  # noqa: E402

SEED = 4101


def collate(seqs, pad, eos, shift=False):
    out = torch.full((len(seqs), max(len(s) for s in seqs)), pad, dtype=torch.long)
    for i, s in enumerate(seqs):
        s = torch.as_tensor(s, dtype=torch.long)
        if shift:
            s = torch.cat([torch.tensor([eos]), s[:-1]])
        out[i, :len(s)] = s
    return out


def main():
    from fairseq.models.chimera.w2v2_transformer_interlingua import S2TTransformerInterlinguaModelW2V2
    from fairseq.sequence_scorer import SequenceScorer

    g = np.load(os.path.join(MG.OUT, "decode_tiny.npz"), allow_pickle=False)
    rec = np.load(os.path.join(MG.OUT, "decode_recipe_tiny.npz"), allow_pickle=False)
    ens = np.load(os.path.join(MG.OUT, "decode_ensemble_tiny.npz"), allow_pickle=False)
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
    members = [m0]
    for k in (1, 2):
        m = copy.deepcopy(m0)
        pre = "member%d/param/" % k
        own = {name[len(pre):]: torch.from_numpy(ens[name].astype(np.float32)) for name in ens.files if name.startswith(pre)}
        dst = m.state_dict()
        assert own and all(name in dst for name in own)
        with torch.no_grad():  # (copied tensor by tensor: the model's load_state_dict would take a partial dict for an old checkpoint
            for name, v in own.items():  # and drop the decoder's final LayerNorm)
                dst[name].copy_(v)
        members.append(m.eval())

    pad, eos, V = d.pad(), d.eos(), len(d)
    gen = torch.Generator().manual_seed(SEED)
    out = {"meta/seed": np.int64(SEED)}
    wrong_len = 0.0
    for tag in ("a", "b"):
        src, lens = torch.from_numpy(rec["in/%s/src_tokens" % tag]), torch.from_numpy(rec["in/%s/src_lengths" % tag])
        seqs = []
        for i in range(src.size(0)):
            best = rec["gen/recipe/%s/b%d/r0/tokens" % (tag, i)].tolist()
            assert best[-1] == eos
            n = len(best) + 2 + i % 3
            seqs += [best, torch.randint(4, V, (n - 1,), generator=gen).tolist() + [eos]]
        target, prev = collate(seqs, pad, eos), collate(seqs, pad, eos, shift=True)
        assert bool(target.eq(pad).any()), ("no pad position", tag)
        net = {"src_tokens": src.repeat_interleave(2, 0), "src_lengths": lens.repeat_interleave(2, 0), "prev_output_tokens": prev}
        B, T = target.shape
        out["%s/target" % tag], out["%s/prev_output_tokens" % tag] = target.numpy(), prev.numpy()
        with torch.no_grad():
            lg = [m(**net)[0].float() for m in members]
        lps = torch.stack([torch.log_softmax(x, -1).gather(2, target.unsqueeze(-1)).squeeze(-1) for x in lg], 0)  # [3, B, T]
        for k, x in enumerate(lg):
            assert x.shape == (B, T, V)
            out["%s/logits/m%d" % (tag, k)] = x.numpy()
        live = target.ne(pad)
        for N in (1, 2, 3):
            sample = {"net_input": net, "target": target}
            with torch.no_grad():
                hyps = SequenceScorer(d).generate(members[:N], sample)
            pos, score, length = torch.zeros(B, T), torch.zeros(B), torch.zeros(B, dtype=torch.long)
            for b, h in enumerate(hyps):
                assert len(h) == 1 and h[0]["attention"] is None and h[0]["alignment"] is None
                n = h[0]["tokens"].numel()
                assert h[0]["tokens"].tolist() == seqs[b] and h[0]["positional_scores"].numel() == n
                pos[b, :n], score[b], length[b] = h[0]["positional_scores"].float(), float(h[0]["score"]), n
                wrong_len = max(wrong_len, abs(float(h[0]["positional_scores"].sum()) / T - float(h[0]["score"])))
            assert bool(torch.isfinite(pos).all()) and bool(torch.isfinite(score).all()), ("a probability underflowed", tag, N)
            if N > 1:
                d0 = float((pos - lps[0])[live].abs().max())
                dm = float((pos - lps[:N].mean(0))[live].abs().max())
                print(tag, "N", N, "max |ensemble - member 0| %.4f, max |ensemble - mean of log-probabilities| %.4f" % (d0, dm))
                assert d0 > 1e-3, ("the ensemble's scores equal member 0's", tag, N)
                assert dm > 1e-3, ("the ensemble's scores equal the mean of the log-probabilities", tag, N)
            key = "n%d/%s/" % (N, tag)
            out[key + "pos_scores"], out[key + "score"], out[key + "len"] = pos.numpy(), score.numpy(), length.numpy()
            print(tag, "N", N, "len", length.tolist(), "score", ["%.4f" % s for s in score.tolist()], "min token score %.3f" % float(pos.min()))
    assert wrong_len > 1e-3, ("no sentence's score tells sum / len from sum / T", wrong_len)
    path = os.path.join(MG.OUT, "decode_score_tiny.npz")
    np.savez_compressed(path, **out)
    print("wrote decode_score_tiny.npz: %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
