"""Shared by test_w2v_pretrain_ref_cpu.py: wav2vec2 pre-training restated on the oracle's wav2vec2 building blocks (the way
wav2vec_ctc_util.ctc_oracle composes the CTC stage with the trunk) — Wav2Vec2Model.forward (wav2vec2.py:527-641) with replayed masks,
negative indices and Gumbel noise, then Wav2vecCriterion's InfoNCE loss and extra losses.  Plain torch on the CPU with autograd."""
import argparse

import torch
import torch.nn.functional as F

import wav2vec_ctc_util as U


def params(requires_grad=True):
    torch.serialization.add_safe_globals([argparse.Namespace])
    ck = torch.load(U.W2V, map_location="cpu")
    return {k: v.clone().requires_grad_(requires_grad and v.is_floating_point()) for k, v in ck["model"].items()}, ck["args"]


def pretrain_oracle(p, a, source, mask, neg_idx, noise, training=True, loss_weights=(0.1, 10.0), choices=None):
    """dict(loss, loss_0, loss_1, loss_2, logits [B, M, K' + 1], correct, count, prob_perplexity, code_perplexity, features_pen, and
    the quantizer's logits `vq_logits` [B M, G, V], its decision values `vq_scores` (logits + noise in training) and `choices`
    [B M, G]).  choices: hard choices to replay instead of the argmax (another evaluation's, where a reduced-precision run decided a
    near-tie the other way); the soft path and every gradient formula are unchanged."""
    from oracle import chimera_oracle as O
    cfg = dict(conv_layers=eval(a.conv_feature_layers), conv_pos=a.conv_pos, conv_pos_groups=a.conv_pos_groups, w2v_layers=a.encoder_layers,
               w2v_heads=a.encoder_attention_heads, feature_grad_mult=a.feature_grad_mult)
    feats = O.conv_feature_extractor(p, "feature_extractor.", source, cfg["conv_layers"])
    feats = O._GradMultiply.apply(feats, cfg["feature_grad_mult"])
    pen = feats.float().pow(2).mean()
    feats = O.layer_norm(feats.transpose(1, 2), p["layer_norm.weight"], p["layer_norm.bias"])
    unmasked = feats
    feats = O.linear(feats, p["post_extract_proj.weight"], p["post_extract_proj.bias"])
    mask = torch.as_tensor(mask)
    B, T = mask.shape
    x = torch.where(mask.unsqueeze(-1), p["mask_emb"], feats)
    y = unmasked[mask].view(B, -1, unmasked.size(-1))
    M = y.size(1)
    kpos = cfg["conv_pos"]
    xc = F.conv1d(x.transpose(1, 2), O.pos_conv_weight(p, "encoder."), p["encoder.pos_conv.0.bias"], padding=kpos // 2, groups=cfg["conv_pos_groups"])
    if kpos % 2 == 0:
        xc = xc[:, :, :-1]
    x = O._st(x + O.gelu(xc).transpose(1, 2))
    x = O.layer_norm(x, p["encoder.layer_norm.weight"], p["encoder.layer_norm.bias"]).transpose(0, 1)
    for i in range(cfg["w2v_layers"]):
        x = O.w2v2_sentence_layer(p, "encoder.layers.%d." % i, x, None, cfg["w2v_heads"])
    x = x.transpose(0, 1)[mask].view(B, M, -1)
    # quantizer (modules/gumbel_vector_quantizer.py:138-199)
    G, V = a.latent_groups, a.latent_vars
    l = O.linear(y.reshape(B * M, -1), p["quantizer.weight_proj.weight"], p["quantizer.weight_proj.bias"]).view(B * M * G, V)
    k = l.argmax(-1, keepdim=True)
    hard = torch.zeros_like(l).scatter_(-1, k, 1.0)
    hp = hard.view(B * M, G, V).mean(0)
    code_ppl = torch.exp(-(hp * torch.log(hp + 1e-7)).sum(-1)).sum()
    avg = torch.softmax(l.view(B * M, G, V), -1).mean(0)
    prob_ppl = torch.exp(-(avg * torch.log(avg + 1e-7)).sum(-1)).sum()
    if training:
        tau = eval(a.latent_temp)[0] if isinstance(a.latent_temp, str) else a.latent_temp[0]
        scores = l + torch.as_tensor(noise).reshape(B * M * G, V)
        ys = (scores / tau).softmax(-1)
        pick = ys.argmax(-1, keepdim=True) if choices is None else torch.as_tensor(choices).long().reshape(-1, 1)
        oh = torch.zeros_like(l).scatter_(-1, pick, 1.0) - ys.detach() + ys
    else:
        scores = l
        oh = hard if choices is None else torch.zeros_like(l).scatter_(-1, torch.as_tensor(choices).long().reshape(-1, 1), 1.0)
    # under oracle.STORAGE the one-hot's gradient (gy, the K = d product's output) and q's are stored tensors of the HIP path: rounded
    # in backward; forward they are exact in any storage type (0 / 1, copies of codebook rows)
    oh = O._st(oh)
    q = O._st((oh.view(B * M, G * V, 1) * p["quantizer.vars"]).view(B * M, G, V, -1).sum(-2).view(B * M, -1))
    yq = O.linear(q, p["project_q.weight"], p["project_q.bias"])
    xf = O.linear(x.reshape(B * M, -1), p["final_proj.weight"], p["final_proj.bias"])
    negs = yq[torch.as_tensor(neg_idx).long().reshape(-1)].view(B * M, -1, yq.size(-1))
    targets = torch.cat([yq.unsqueeze(1), negs], 1)
    logits = torch.cosine_similarity(xf.unsqueeze(1), targets, dim=-1) / a.logit_temp
    eq = (negs == yq.unsqueeze(1)).all(-1)
    logits = torch.cat([logits[:, :1], logits[:, 1:].masked_fill(eq, float("-inf"))], 1)
    n = B * M
    l0 = F.cross_entropy(logits, torch.zeros(n, dtype=torch.long), reduction="sum")
    nv = G * V
    l1 = loss_weights[0] * ((nv - prob_ppl) / nv) * n
    l2 = loss_weights[1] * pen * n
    mx, mn = logits.argmax(-1) == 0, logits.argmin(-1) == 0
    return dict(loss=l0 + l1 + l2, loss_0=l0, loss_1=l1, loss_2=l2, logits=logits.view(B, M, -1), choices=oh.detach().view(n, G, V).argmax(-1),
                vq_logits=l.detach().view(n, G, V), vq_scores=scores.detach().view(n, G, V), correct=int(mx.sum()) - int((mx & mn).sum()),
                count=n, prob_perplexity=prob_ppl, code_perplexity=code_ppl, features_pen=pen)


def pretrain_oracle_fn(p, sample, cfg):
    """pretrain_oracle in the calling convention of parity_util.run_oracle (which sets oracle.STORAGE and rounds the leaves):
    sample = dict(source, mask, neg_idx, noise, training, choices), cfg = the checkpoint's arguments."""
    return pretrain_oracle(p, cfg, sample["source"], sample["mask"], sample["neg_idx"], sample.get("noise"), training=sample.get("training", True),
                           choices=sample.get("choices"))
