#!/usr/bin/env python3
"""Fixtures of the large-style wav2vec2 layout (extractor_mode=layer_norm, conv_bias=True, layer_norm_first=True) at the harness's
tiny dimensions, produced by running the REAL reference (imported through ref_import.py) on CPU fp32.

Build container only:   python tools/ref_harness/make_w2v_large_goldens.py
Holds data only (inputs, parameters, activations, logits, loss terms, gradients, generator output), never reference source.
Dropout and layerdrop are 0 everywhere: nothing draws a random number after the parameters are initialised.

  w2v_large_tiny.pt                 the wav2vec2 checkpoint ({"args", "model"}) the reference saved; --w2v2-model-path takes it
  w2v_large_tiny.npz                ragged 3-utterance batch (one much shorter): inputs, stage activations of the wav2vec2 model
                                    (act/conv0, act/cnn, act/proj, act/last_layer, act/final_ln, act/out) and its padding mask
  w2v_large_s2t_tiny.npz            s2t_transformer_w2v2 + label_smoothed_cross_entropy over that checkpoint: the key layout of
  w2v_large_s2t_tiny_grads.npz      s2t_w2v2_tiny.npz, the grad/ keys in a file of their own (every committed file stays < 1 MiB)
  w2v_large_chimera_tiny.npz        s2t_transformer_w2v2_interlingua + triplet criterion: the key layout of chimera_tiny.npz,
  w2v_large_chimera_tiny_grads.npz  plus gen/beam{1,5}/... from the reference's SequenceGenerator on the model as initialised
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ref_import import import_reference  # noqa: E402

import_reference()
import make_goldens as MG  # noqa: E402

W2V_LARGE_TINY = dict(MG.W2V_TINY, extractor_mode="layer_norm", conv_bias=True, layer_norm_first=True)
S = (3600, 3000, 900)  # samples per utterance: the last one is much shorter (padding, and the zeroing of padded frames)


def build_w2v_ckpt(path, seed):
    from argparse import Namespace

    from fairseq.models.wav2vec.wav2vec2 import Wav2Vec2Model

    torch.manual_seed(seed)
    ns = Namespace(**W2V_LARGE_TINY)
    w2v = Wav2Vec2Model.build_model(ns, task=None)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():  # biases and LayerNorm affines start at 0 / 1: move them so that parity sees them
        for n, p in w2v.named_parameters():
            if n.endswith("bias") or "layer_norm" in n or n.endswith("2.1.weight"):
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    torch.save({"args": ns, "model": w2v.state_dict()}, path)
    return ns


def save(name, out):
    path = os.path.join(MG.OUT, name)
    np.savez_compressed(path, **out)
    print(name, os.path.getsize(path))


def split_save(stem, out):
    save(stem + ".npz", {k: v for k, v in out.items() if not k.startswith("grad/")})
    save(stem + "_grads.npz", {k: v for k, v in out.items() if k.startswith("grad/")})


def common(out, model, sample, args):
    for n, p in model.named_parameters():
        out["grad/" + n] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy()
    out.update(MG.np_state(model))
    for k in out:  # (uninitialised one-element buffers of the positional embeddings: never read; zeroed so that the files regenerate bit for bit)
        if k.endswith("._float_tensor"):
            out[k] = np.zeros_like(out[k])
    for k in ("src_tokens", "src_lengths", "prev_output_tokens"):
        out["in/" + k] = sample["net_input"][k].numpy()
    for k in ("target", "target_lengths", "src_text", "src_text_lengths"):
        out["in/" + k] = sample[k].numpy()
    out["in/ntokens"] = np.int64(sample["ntokens"])
    out["meta/w2v_args"] = np.array(repr(W2V_LARGE_TINY))
    out["meta/model_args"] = np.array(repr({k: v for k, v in vars(args).items() if k != "w2v2_model_path"}))


def gen_w2v_stages(w2v_path, sample):
    from fairseq.models.wav2vec.wav2vec2 import Wav2Vec2Model

    ck = torch.load(w2v_path, map_location="cpu", weights_only=False)
    w2v = Wav2Vec2Model.build_model(ck["args"], task=None)
    w2v.load_state_dict(ck["model"])
    w2v.eval()
    w2v.encoder.pos_conv.register_forward_pre_hook(lambda m, i: (i[0].contiguous(),))
    names = {"conv0": "feature_extractor.conv_layers.0", "cnn": "feature_extractor", "proj": "post_extract_proj",
             "last_layer": "encoder.layers.%d" % (len(w2v.encoder.layers) - 1), "final_ln": "encoder.layer_norm"}
    acts, hooks = MG.capture(w2v, names)
    wav, lens = sample["net_input"]["src_tokens"], sample["net_input"]["src_lengths"]
    pm = torch.arange(wav.size(1)).view(1, -1) >= lens.view(-1, 1)
    with torch.no_grad():
        x, fpm = w2v.extract_features(wav, pm, mask=False)
    for h in hooks:
        h.remove()
    out = {"act/" + k: v[0] for k, v in acts.items()}  # conv0 / cnn [B,C,T]; proj [B,T,C]; last_layer [T,B,C]; final_ln [B,T,C]
    out["act/out"] = x.numpy()
    out["out/padding_mask"] = fpm.numpy()
    out["in/src_tokens"], out["in/src_lengths"] = wav.numpy(), lens.numpy()
    out["meta/w2v_args"] = np.array(repr(W2V_LARGE_TINY))
    save("w2v_large_tiny.npz", out)


def main():
    from fairseq.criterions.label_smoothed_cross_entropy import LabelSmoothedCrossEntropyCriterion
    from fairseq.criterions.triplet_st_mt_contrastive import TripletSTMTContrastiveCriterion
    from fairseq.models.chimera.w2v2_transformer import S2TTransformerModelW2V2
    from fairseq.models.chimera.w2v2_transformer_interlingua import S2TTransformerInterlinguaModelW2V2
    from fairseq.sequence_generator import SequenceGenerator

    torch.set_num_threads(1)  # one summation order: the fixtures regenerate bit-identically
    d = MG.make_dictionary()
    task = MG.TaskStub(d)
    w2v_path = os.path.join(MG.OUT, "w2v_large_tiny.pt")
    build_w2v_ckpt(w2v_path, seed=31)
    print("w2v_large_tiny.pt", os.path.getsize(w2v_path))
    sample = MG.make_sample(d, seed=34, B=3, S=S, U=(6, 9, 4), L=(5, 7, 3))
    gen_w2v_stages(w2v_path, sample)

    # ---- s2t_transformer_w2v2 ----
    torch.manual_seed(32)
    args = MG.model_args(w2v_path, encoder_layers=1, decoder_layers=1)
    model = S2TTransformerModelW2V2.build_model(args, task)
    MG.randomize_small_params(model, 33)
    model.encoder.wav2vec_model.encoder.pos_conv.register_forward_pre_hook(lambda m, i: (i[0].contiguous(),))
    model.train()
    crit = LabelSmoothedCrossEntropyCriterion(task, False, 0.1)
    model.zero_grad()
    loss, sample_size, log = crit(model, sample)
    loss.backward()
    out = {}
    with torch.no_grad():
        logits, _ = model(**sample["net_input"])
        enc = model.encoder(sample["net_input"]["src_tokens"], sample["net_input"]["src_lengths"])
    out["out/logits"] = logits.numpy()
    out["out/encoder_out"] = enc.encoder_out.numpy()
    out["out/encoder_padding_mask"] = (enc.encoder_padding_mask.numpy() if enc.encoder_padding_mask is not None else np.zeros((0,), dtype=bool))
    out["loss/loss"] = np.float64(loss.item())
    out["loss/nll_loss"] = np.float64(float(log["nll_loss"]))
    out["loss/sample_size"] = np.int64(sample_size)
    common(out, model, sample, args)
    split_save("w2v_large_s2t_tiny", out)
    print("s2t: loss", loss.item())

    # ---- Chimera ----
    torch.manual_seed(35)
    args = MG.model_args(w2v_path, encoder_layers=1, decoder_layers=1, interlingua_layers=1, encoder_ffn_embed_dim=64)
    model = S2TTransformerInterlinguaModelW2V2.build_model(args, task)
    MG.randomize_small_params(model, 36)
    model.encoder.wav2vec_model.encoder.pos_conv.register_forward_pre_hook(lambda m, i: (i[0].contiguous(),))
    model.train()
    crit = TripletSTMTContrastiveCriterion(task, False, 0.1, [1.0, 1.0, 1.0], 0.1, 0, False, None, [None, None])
    model.zero_grad()
    loss, sample_size, log = crit(model, sample)
    loss.backward()
    out = {}
    with torch.no_grad():
        (st_logits, _), mem_a = model.forward_with_internal(**sample["net_input"])
        (mt_logits, _), mem_t = model.forward_with_internal(
            src_tokens=sample["src_text"], src_lengths=sample["src_text_lengths"],
            prev_output_tokens=sample["net_input"]["prev_output_tokens"], mask=False)
    out.update({"out/st_logits": st_logits.numpy(), "out/mt_logits": mt_logits.numpy(), "out/memory_audio": mem_a.numpy(),
                "out/memory_text": mem_t.numpy(), "loss/loss": np.float64(loss.item()), "loss/sample_size": np.int64(sample_size)})
    for k in ("nll_loss", "st_loss", "st_nll_loss", "mt_loss", "mt_nll_loss", "contrastive_loss"):
        out["loss/" + k] = np.float64(float(log[k]))
    common(out, model, sample, args)
    model.eval()
    for beam in (1, 5):
        gen = SequenceGenerator([model], d, beam_size=beam, max_len_a=0, max_len_b=12, min_len=1)
        with torch.no_grad():
            hyps = gen.generate([model], sample)
        for b, h in enumerate(hyps):
            for r, hyp in enumerate(h[: min(beam, 3)]):
                out["gen/beam%d/b%d/r%d/tokens" % (beam, b, r)] = hyp["tokens"].numpy()
                out["gen/beam%d/b%d/r%d/score" % (beam, b, r)] = np.float64(float(hyp["score"]))
    split_save("w2v_large_chimera_tiny", out)
    print("chimera: loss", loss.item(), {k: float(v) for k, v in log.items() if "loss" in k})


if __name__ == "__main__":
    main()
