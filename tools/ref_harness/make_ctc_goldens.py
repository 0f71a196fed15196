#!/usr/bin/env python3
"""tests/golden/ctc_tiny.npz — CTC fine-tuning as the REAL reference computes it (imported through ref_import.py), on the CPU in fp32:
a tiny Wav2VecCtc (fairseq/models/wav2vec/wav2vec2_asr.py) over tests/golden/w2v_quant_tiny.pt with a letter dictionary of 32 symbols
under CtcCriterion (fairseq/criterions/ctc.py), and the pure functions compute_mask_indices / post_process of data/data_utils.py.

Build container only:   python tools/ref_harness/make_ctc_goldens.py
Holds data only, never reference source.  `editdistance` is the stub of tools/ref_harness/stubs.

Keys:
  meta/dict            the dictionary's symbols behind the four specials, one string;  meta/seed: the numpy seed of the mask cases
  meta/keys            the model's state-dict keys, newline-joined (w2v_encoder.w2v_model.* WITHOUT the pre-training heads, w2v_encoder.proj.*)
  in/source [B, S] float32, in/padding_mask [B, S] bool, in/target [B, L] int64 (pad 1), in/target_lengths [B]
  param/<key>          the projection's parameters (the wav2vec2 weights are those of w2v_quant_tiny.pt, not stored again)
  out/logits [T, B, V], out/nll [B], out/loss (reduction sum), out/frame_padding_mask [B, T]
  grad/<key>           d loss / d parameter (train mode, every dropout 0, no masking)
  eval/<name>          the eval-mode logging output: c_errors, c_total, w_errors, wv_errors, w_total
  mask/<case>/...      compute_mask_indices for np.random.seed(SEED) at two (B, T) shapes, with and without a padding mask:
                       lengths (real frames per row; absent without padding), args (mask_prob, mask_length, min_masks), mask [B, T] bool;
                       the time mask and then a channel mask are drawn from ONE seeded stream, as apply_mask draws them
  post/<symbol>/in|out post_process outputs for a few strings"""
import os
import sys
from argparse import Namespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ref_import import import_reference  # noqa: E402

import_reference()
from fairseq.criterions.ctc import CtcCriterion  # noqa: E402
from fairseq.data import Dictionary  # noqa: E402
from fairseq.data.data_utils import compute_mask_indices, post_process  # noqa: E402
from fairseq.models.wav2vec.wav2vec2_asr import Wav2VecCtc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SEED = 5204
LETTERS = "|ETAONIHSRDLUMWCFGYPBVK'XJQZ"  # 28 symbols + 4 specials = the 32 classes of the published letter dictionary


def main():
    out = {}
    d = Dictionary()
    for c in LETTERS:
        d.add_symbol(c)
    out["meta/dict"] = np.array(LETTERS)
    out["meta/seed"] = np.int64(SEED)

    ck = torch.load(os.path.join(GOLDEN, "w2v_quant_tiny.pt"), map_location="cpu")
    w2v_args = ck["args"]
    w2v_args.task, w2v_args.arch, w2v_args.normalize, w2v_args.labels = "audio_pretraining", "wav2vec2", False, None
    w2v_args.criterion = "wav2vec"
    w2v_args.sample_rate, w2v_args.max_sample_size, w2v_args.min_sample_size, w2v_args.enable_padding = 16000, None, None, False
    args = Namespace(w2v_path=None, w2v_args=w2v_args, normalize=False, data="/tmp", criterion="ctc", zero_infinity=False, post_process="letter",
                     wer_args=None, sentence_avg=False, final_dropout=0.0)
    task = Namespace(target_dictionary=d)
    torch.manual_seed(SEED)
    model = Wav2VecCtc.build_model(args, task)
    sd = {"w2v_encoder.w2v_model." + k: v for k, v in ck["model"].items()
          if not k.startswith(("quantizer.", "project_q.", "final_proj.", "target_glu."))}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("w2v_encoder.proj.") for k in missing), (missing, unexpected)
    # (torch >= 2: the conv must not see the view that `x += x_conv` then modifies in place, as in make_goldens.py — values unchanged)
    model.w2v_encoder.w2v_model.encoder.pos_conv.register_forward_pre_hook(lambda m, i: (i[0].contiguous(),))
    out["meta/keys"] = np.array("\n".join(model.state_dict().keys()))
    with torch.no_grad():  # wide logit margins: the eval counts must not hinge on an argmax decided in the last fp32 bits
        model.w2v_encoder.proj.weight.mul_(20.0)
    for k, v in model.state_dict().items():  # (the wav2vec2 weights are w2v_quant_tiny.pt's and are not stored again)
        if k.startswith("w2v_encoder.proj."):
            out["param/" + k] = v.detach().numpy().copy()

    g = torch.Generator().manual_seed(SEED)
    lens = [4000, 3100, 2300]
    B, S = len(lens), max(lens)
    source = torch.zeros(B, S)
    pm = torch.zeros(B, S, dtype=torch.bool)
    for b, n in enumerate(lens):
        source[b, :n] = 0.1 * torch.randn(n, generator=g)
        pm[b, n:] = True
    texts = ["THE|CAT|", "A|DOG", "IT"]
    target = torch.full((B, max(len(t) for t in texts)), d.pad(), dtype=torch.long)
    for b, t in enumerate(texts):
        target[b, :len(t)] = torch.tensor([d.index(c) for c in t])
    tl = torch.tensor([len(t) for t in texts])
    sample = {"id": torch.arange(B), "net_input": {"source": source, "padding_mask": pm}, "target": target, "target_lengths": tl,
              "ntokens": int(tl.sum())}
    out.update({"in/source": source.numpy(), "in/padding_mask": pm.numpy(), "in/target": target.numpy(), "in/target_lengths": tl.numpy()})

    crit = CtcCriterion(args, task)
    model.train()
    loss, sample_size, log = crit(model, sample)
    loss.backward()
    assert sample_size == int(tl.sum()) and np.isfinite(float(loss))
    for k, p in model.named_parameters():
        out["grad/" + k] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy().copy()
    with torch.no_grad():
        net = model(**sample["net_input"])
        lp = model.get_normalized_probs(net, log_probs=True)
        in_len = (~net["padding_mask"]).long().sum(-1)
        nll = torch.nn.functional.ctc_loss(lp, target[target != d.pad()], in_len, tl, blank=d.bos(), reduction="none")
    assert abs(float(nll.sum()) - float(loss)) < 1e-4 * abs(float(loss))
    out.update({"out/logits": net["encoder_out"].numpy(), "out/nll": nll.numpy(), "out/loss": np.float32(float(loss)),
                "out/frame_padding_mask": net["padding_mask"].numpy()})
    model.eval()
    with torch.no_grad():
        _, _, elog = crit(model, sample)
    for k in ("c_errors", "c_total", "w_errors", "wv_errors", "w_total"):
        out["eval/" + k] = np.int64(elog[k])
    assert elog["c_total"] == int(tl.sum()) and elog["w_total"] == 5
    top2 = net["encoder_out"].transpose(0, 1)[~net["padding_mask"]].topk(2, dim=-1).values
    margin = float((top2[:, 0] - top2[:, 1]).min())
    assert margin > 0.02, "a best-path decision of the fixture hangs on %g: change the seed" % margin

    for name, (B_, T_), lens_ in (("pad_3x50", (3, 50), [50, 31, 40]), ("nopad_3x50", (3, 50), None),
                                  ("pad_2x137", (2, 137), [137, 90]), ("nopad_2x137", (2, 137), None)):
        np.random.seed(SEED)
        pmask = None
        if lens_ is not None:
            pmask = torch.arange(T_)[None, :] >= torch.tensor(lens_)[:, None]
            out["mask/%s/lengths" % name] = np.array(lens_)
        m = compute_mask_indices((B_, T_), pmask, 0.5, 10, "static", 0, min_masks=2, no_overlap=False, min_space=1)
        c = compute_mask_indices((B_, 64), None, 0.25, 8, "static", 0, no_overlap=False, min_space=1)
        out["mask/%s/time" % name], out["mask/%s/channel" % name] = m, c
        assert m.any() and c.any()
    for sym, strings in (("letter", ["T H E | C A T |", "A | D O G", ""]), ("sentencepiece", ["▁the ▁ca t", "▁a"]),
                         ("none", ["a b"]), ("@@ ", ["he@@ llo wor@@ ld"])):
        out["post/%s/in" % sym] = np.array(strings)
        out["post/%s/out" % sym] = np.array([post_process(s, sym) for s in strings])
    path = os.path.join(GOLDEN, "ctc_tiny.npz")
    np.savez_compressed(path, **out)
    print("min argmax margin", margin)
    print("wrote", path, os.path.getsize(path), "bytes; loss", float(loss), "eval", {k: int(out["eval/" + k]) for k in
          ("c_errors", "c_total", "w_errors", "wv_errors", "w_total")})


if __name__ == "__main__":
    main()
