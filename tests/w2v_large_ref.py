"""The large-style wav2vec2 feature path, restated from its formulas in plain torch (the role fbank_ref.py plays for filter banks):
extractor_mode="layer_norm" (every conv layer: Conv1d with bias -> LayerNorm over the channels of a frame, fp32 statistics -> GELU),
pre-norm Transformer layers (x = x + attn(LN(x)); x = x + fc2(gelu(fc1(LN(x))))), and the LayerNorm behind the last layer instead
of in front of the first.  Everything runs in the dtype of the parameters it is given: fp64 parameters give the fp64 reference.

The checker only: nothing here is imported by the product.  The primitives shared with the default-mode oracle (attention, linear,
storage-rounding points) are the oracle's, so `patched_oracle()` lets the whole-model oracle functions (lsce_criterion,
triplet_criterion, with or without bf16 storage emulation) run over a large-style wav2vec2."""
import contextlib

import torch
import torch.nn.functional as F

from oracle import chimera_oracle as O


def ln_gelu(u, w, b, eps=1e-5):
    """u [..., C]: GELU(LayerNorm over the last axis).  The HIP kernels keep the normalised value in registers: one storage point."""
    mu = u.mean(-1, keepdim=True)
    var = ((u - mu) ** 2).mean(-1, keepdim=True)
    z = (u - mu) * torch.rsqrt(var + eps) * w + b
    return O._st(0.5 * z * (1.0 + torch.erf(z * 0.7071067811865476)))


def conv_feature_extractor(p, pre, wav, conv_layers):
    """wav [B,S] -> [B,C,T]; keys conv_layers.N.0.{weight,bias}, conv_layers.N.2.1.{weight,bias}."""
    x = wav.unsqueeze(1)
    for i, (dim, k, s) in enumerate(conv_layers):
        x = F.conv1d(x, p["%sconv_layers.%d.0.weight" % (pre, i)], p.get("%sconv_layers.%d.0.bias" % (pre, i)), stride=s)
        if i > 0:
            x = O._st(x)  # (layer 0 goes conv -> LayerNorm -> GELU in registers; layers 1.. store the conv GEMM's output)
        x = ln_gelu(x.transpose(1, 2), p["%sconv_layers.%d.2.1.weight" % (pre, i)], p["%sconv_layers.%d.2.1.bias" % (pre, i)]).transpose(1, 2)
    return x


def sentence_layer_pre_norm(p, pre, x, padding_mask, heads):
    """x [T,B,C]."""
    h = O.layer_norm(x, p[pre + "self_attn_layer_norm.weight"], p[pre + "self_attn_layer_norm.bias"])
    x = O._st(x + O.mha(p, pre + "self_attn.", h, h, h, heads, key_padding_mask=padding_mask))
    h = O.layer_norm(x, p[pre + "final_layer_norm.weight"], p[pre + "final_layer_norm.bias"])
    h = O.gelu(O.linear(h, p[pre + "fc1.weight"], p[pre + "fc1.bias"]))
    return O._st(x + O.linear(h, p[pre + "fc2.weight"], p[pre + "fc2.bias"]))


def extract_features(p, pre, wav, padding_mask, cfg):
    """-> x [B,T,C], frame padding mask [B,T] (or None), {stage: tensor}.  cfg: conv_layers, conv_pos, conv_pos_groups, w2v_layers,
    w2v_heads, feature_grad_mult."""
    inter = {}
    feats = conv_feature_extractor(p, pre + "feature_extractor.", wav, cfg["conv_layers"])
    if cfg.get("feature_grad_mult", 1.0) != 1.0:
        feats = O._GradMultiply.apply(feats, cfg["feature_grad_mult"])
    inter["w2v_cnn"] = feats
    feats = O.layer_norm(feats.transpose(1, 2), p[pre + "layer_norm.weight"], p[pre + "layer_norm.bias"])
    pm = O.downsample_padding_mask(padding_mask, feats.size(1)) if padding_mask is not None else None
    if (pre + "post_extract_proj.weight") in p:
        feats = O.linear(feats, p[pre + "post_extract_proj.weight"], p[pre + "post_extract_proj.bias"])
    inter["w2v_proj"] = feats
    x = feats
    e = pre + "encoder."
    if pm is not None:
        x = x.masked_fill(pm.unsqueeze(-1), 0.0)
    kpos = cfg["conv_pos"]
    xc = F.conv1d(x.transpose(1, 2), O.pos_conv_weight(p, e), p[e + "pos_conv.0.bias"], padding=kpos // 2, groups=cfg["conv_pos_groups"])
    if kpos % 2 == 0:
        xc = xc[:, :, :-1]
    x = O._st(x + O.gelu(xc).transpose(1, 2))
    x = x.transpose(0, 1)  # (no LayerNorm in front of a pre-norm stack)
    for i in range(cfg["w2v_layers"]):
        x = sentence_layer_pre_norm(p, "%slayers.%d." % (e, i), x, pm, cfg["w2v_heads"])
    inter["w2v_last_layer"] = x
    x = O.layer_norm(x.transpose(0, 1), p[e + "layer_norm.weight"], p[e + "layer_norm.bias"])
    inter["w2v_out"] = x
    return x, pm, inter


@contextlib.contextmanager
def patched_oracle():
    """Inside: the oracle's audio front end runs the large-style wav2vec2 above."""
    prev = O.w2v2_extract_features
    O.w2v2_extract_features = extract_features
    try:
        yield O
    finally:
        O.w2v2_extract_features = prev
