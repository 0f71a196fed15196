#!/usr/bin/env python3
"""tests/golden/w2v_pretrain_tiny.npz — wav2vec2 pre-training as the REAL reference computes it (imported through ref_import.py), on the
CPU in fp32: Wav2Vec2Model (fairseq/models/wav2vec/wav2vec2.py) over tests/golden/w2v_quant_tiny.pt (final_dim 16, V = 8, G = 2) under
Wav2vecCriterion (fairseq/criterions/wav2vec_criterion.py) with --infonce and --loss-weights [0.1, 10], train mode with every dropout
and layerdrop at 0, on 3 cropped utterances.

Build container only:   python tools/ref_harness/make_w2v_pretrain_goldens.py
Holds data only, never reference source.  The draws are recorded so that another implementation can replay them: the time mask
(compute_mask_indices under np.random.seed(SEED)), the indices sample_negatives returned, and the Gumbel noise — F.gumbel_softmax is
replaced by a function with torch's own formula that keeps the noise it drew.

Keys (case = train | eval | cross; cross: cross_sample_negatives = 2 on top of num_negatives):
  meta/seed, meta/num_negatives, meta/cross_sample_negatives, meta/loss_weights, meta/keys (the state-dict keys, newline-joined)
  in/source [B, S] float32
  <case>/mask [B, T] bool, <case>/neg_idx [B * M, K'] int64 (flat rows into [B * M], as the reference's view(bsz, num, K') reads them),
  <case>/noise [B * M, G, V] float32 (train, cross), <case>/logits [B, M, K' + 1] (positive first; -inf where a negative equals it),
  <case>/loss, <case>/loss_0..2, <case>/correct, <case>/count, <case>/prob_perplexity, <case>/code_perplexity, <case>/temp,
  <case>/features_pen, <case>/sample_size
  grad/<key>  d loss / d parameter of the train case"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ref_import import import_reference  # noqa: E402

import_reference()
import fairseq.models.wav2vec.wav2vec2 as W  # noqa: E402
from fairseq.criterions.wav2vec_criterion import Wav2vecCriterion  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SEED = 7311
REC = {}


def recording_gumbel_softmax(logits, tau=1, hard=False, eps=1e-10, dim=-1):
    """torch.nn.functional.gumbel_softmax's formula, with the noise kept."""
    gumbels = -torch.empty_like(logits).exponential_().log()
    REC["noise"] = gumbels.detach().clone()
    g = (logits + gumbels) / tau
    top2 = (logits + gumbels).topk(2, dim=dim).values
    REC["margin"] = float((top2[..., 0] - top2[..., 1]).min())
    y_soft = g.softmax(dim)
    index = y_soft.max(dim, keepdim=True)[1]
    y_hard = torch.zeros_like(logits).scatter_(dim, index, 1.0)
    return y_hard - y_soft.detach() + y_soft if hard else y_soft


def main():
    torch.nn.functional.gumbel_softmax = recording_gumbel_softmax
    real_masks = W.compute_mask_indices

    def recording_masks(*a, **k):
        m = real_masks(*a, **k)
        REC.setdefault("mask", m)
        return m
    W.compute_mask_indices = recording_masks

    ck = torch.load(os.path.join(GOLDEN, "w2v_quant_tiny.pt"), map_location="cpu")
    args = ck["args"]
    args.mask_prob, args.mask_length, args.num_negatives = 0.3, 3, 5
    model = W.Wav2Vec2Model.build_model(args, None)
    model.load_state_dict(ck["model"], strict=True)
    model.encoder.pos_conv.register_forward_pre_hook(lambda m, i: (i[0].contiguous(),))  # (torch >= 2, as in make_ctc_goldens.py)
    real_neg = model.sample_negatives

    def recording_neg(y, num):
        negs, idx = real_neg(y, num)
        REC["neg_idx"] = idx.reshape(y.shape[0] * num, -1).clone()
        return negs, idx
    model.sample_negatives = recording_neg

    out = {"meta/seed": np.int64(SEED), "meta/num_negatives": np.int64(args.num_negatives), "meta/cross_sample_negatives": np.int64(2),
           "meta/loss_weights": np.array([0.1, 10.0]), "meta/keys": np.array("\n".join(model.state_dict().keys())),
           "meta/mask_prob": np.float64(args.mask_prob), "meta/mask_length": np.int64(args.mask_length)}
    g = torch.Generator().manual_seed(SEED)
    source = 0.1 * torch.randn(3, 3000, generator=g)
    out["in/source"] = source.numpy()
    sample = {"id": torch.arange(3), "net_input": {"source": source, "padding_mask": None}}
    task = None
    crit = Wav2vecCriterion(task, True, "[0.1, 10]", '["prob_perplexity","code_perplexity","temp"]')

    def run(case, train):
        REC.clear()
        np.random.seed(SEED)
        torch.manual_seed(SEED)
        model.train(train)
        model.zero_grad()
        net = model(**sample["net_input"])
        np.random.seed(SEED)
        torch.manual_seed(SEED)
        REC.pop("mask")
        loss, sample_size, log = crit(model, sample)  # the same draws again: what the criterion sees is what `net` holds
        B, T = REC["mask"].shape
        M = sample_size // B
        logits = model.get_logits(net).float()  # [M * B, K' + 1], time-major rows
        out[case + "/logits"] = logits.view(M, B, -1).transpose(0, 1).detach().numpy().copy()
        out[case + "/mask"] = np.asarray(REC["mask"])
        out[case + "/neg_idx"] = REC["neg_idx"].numpy()
        if train:
            out[case + "/noise"] = REC["noise"].view(B * M, model.quantizer.groups, -1).numpy()
            assert REC["margin"] >= 1e-3, "a hard choice of the fixture hangs on %g: change the seed" % REC["margin"]
        else:
            l = model.quantizer.weight_proj(model.layer_norm(model.feature_extractor(source).transpose(1, 2)))
            top2 = l.view(B, T, model.quantizer.groups, -1).topk(2, dim=-1).values
            assert float((top2[..., 0] - top2[..., 1]).min()) >= 1e-3
        for k in ("loss", "loss_0", "loss_1", "loss_2", "correct", "count", "prob_perplexity", "code_perplexity", "temp", "sample_size"):
            out[case + "/" + k] = np.float64(log[k])
        out[case + "/features_pen"] = np.float64(float(net["features_pen"]))
        assert M >= 4 and bool(torch.isinf(logits).any()), "no negative carries its positive's codes: change the seed or the mask options"
        return loss

    loss = run("train", True)
    loss.backward()
    for k, p in model.named_parameters():
        out["grad/" + k] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy().copy()
    run("eval", False)
    model.cross_sample_negatives = 2
    run("cross", True)
    path = os.path.join(GOLDEN, "w2v_pretrain_tiny.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; loss", float(out["train/loss"]), "M", int(out["train/sample_size"]) // 3,
          "correct", out["train/correct"], "-inf logits", int(np.isinf(out["train/logits"]).sum()))


if __name__ == "__main__":
    main()
