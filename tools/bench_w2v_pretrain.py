#!/usr/bin/env python3
"""The contrastive head of wav2vec2 pre-training, CF.sample_negatives + CF.infonce_loss (cst_w2v_negatives, cst_infonce_fwd, cst_infonce_bwd_x,
cst_infonce_bwd_y), against the calls it replaces on the same device: sample_negatives + compute_preds of the reference model
(torch.randint, the gathered [K + 1, N, D] targets, torch.cosine_similarity, the -inf mask) and the criterion's
F.cross_entropy(reduction="sum"), forward + backward.  The shape is the base recipe's: B = 8 utterances of 250 000 samples (T = 781
frames), about 380 masked frames each, D = final_dim = 256, K = 100 negatives, temperature 0.1, bf16, seeded.  The targets are
codebook-like (each y row is one of 4096 distinct rows), so some negatives equal their positive and the mask is exercised.

A second line times the Gumbel quantizer after its projection, CF.gumbel_vector_quantize (cst_gumbel_vq_fwd, cst_gumbel_vq_bwd and the two
GEMMs of its backward), against GumbelVectorQuantizer.forward's own operations (modules/gumbel_vector_quantizer.py:148-199) at N = 8 x 781
frames, G = 2, V = 320, d = 128, tau = 2, forward + backward of sum(q * dq) + 0.1 * prob_perplexity.

Prints one JSON line per part: milliseconds per forward + backward from device events over a window of calls (host launch cost included), the
windows alternating between the two sides; the median window and the spread (max - min) of each side; the peak device memory of one
call of each side above what the operands hold; and the largest difference of the two losses and gradients on the SAME indices (they
must agree: faster and different is not faster).  Needs a GPU; there is no fallback.

  python tools/bench_w2v_pretrain.py [--windows 5] [--calls 400]   (a window of 400 calls is 0.2 s on our side, 1.3 - 1.8 s on torch's)"""
import argparse
import importlib
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPE = dict(B=8, M=380, D=256, K=100, temp=0.1, codes=4096)


def device_window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def stats(v):
    v = sorted(v)
    return {"median_ms": round(v[len(v) // 2], 4), "spread_ms": round(v[-1] - v[0], 4)}


def torch_negatives(B, M, K):
    """sample_negatives (models/wav2vec/wav2vec2.py:454-510) with the draws made on the device: [B * M, K] flat row indices."""
    tszs = torch.arange(M, device="cuda").unsqueeze(-1).expand(-1, K).flatten()
    neg = torch.randint(0, M - 1, (B, K * M), device="cuda")
    neg[neg >= tszs] += 1
    neg += torch.arange(B, device="cuda")[:, None] * M
    return neg.view(B * M, K)


def torch_head(x, y, idx, temp):
    """compute_preds (:512-525) + the criterion's cross entropy on the logits' float() (criterions/wav2vec_criterion.py:64-77)."""
    N, D = x.shape
    negs = y[idx.reshape(-1)].view(N, -1, D).permute(1, 0, 2)
    neg_is_pos = (y.unsqueeze(0) == negs).all(-1)
    targets = torch.cat([y.unsqueeze(0), negs], dim=0)
    logits = torch.cosine_similarity(x.unsqueeze(0).float(), targets.float(), dim=-1).type_as(x)
    logits = logits / temp
    logits[1:][neg_is_pos] = float("-inf")  # (the reference tests neg_is_pos.any() on the host first: one synchronisation spared here)
    return F.cross_entropy(logits.transpose(0, 1).float(), torch.zeros(N, dtype=torch.long, device=x.device), reduction="sum")


def torch_quantizer(x, vars_, G, tau):
    """GumbelVectorQuantizer.forward from the projection's output on (:148-199), training mode."""
    N, GV = x.shape
    xg = x.view(N * G, -1)
    _, k = xg.max(-1)
    hard_x = xg.new_zeros(*xg.shape).scatter_(-1, k.view(-1, 1), 1.0).view(N, G, -1)
    hard_probs = torch.mean(hard_x.float(), dim=0)
    code_ppl = torch.exp(-torch.sum(hard_probs * torch.log(hard_probs + 1e-7), dim=-1)).sum()
    avg_probs = torch.softmax(xg.view(N, G, -1).float(), dim=-1).mean(dim=0)
    prob_ppl = torch.exp(-torch.sum(avg_probs * torch.log(avg_probs + 1e-7), dim=-1)).sum()
    y = F.gumbel_softmax(xg.float(), tau=tau, hard=True).type_as(xg).view(N, -1)
    q = (y.unsqueeze(-1) * vars_).view(N, G, GV // G, -1).sum(-2).view(N, -1)
    return q, prob_ppl, code_ppl


def peak_above(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=400)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_w2v_pretrain.py measures on the GPU; there is no fallback"
    CF = importlib.import_module("chimera-st_amd.functional")
    rng = importlib.import_module("chimera-st_amd.rng")
    c = SHAPE
    B, M, D, K, temp = c["B"], c["M"], c["D"], c["K"], c["temp"]
    N = B * M
    g = torch.Generator().manual_seed(1)
    codebook = torch.randn(c["codes"], D, generator=g)
    x0 = torch.randn(N, D, generator=g).to(torch.bfloat16).cuda()
    y0 = codebook[torch.randint(c["codes"], (N,), generator=g)].to(torch.bfloat16).cuda()
    xa, ya = x0.clone().requires_grad_(True), y0.clone().requires_grad_(True)
    xb, yb = x0.clone().requires_grad_(True), y0.clone().requires_grad_(True)
    rng.reseed(1)
    fixed = CF.sample_negatives(B, M, K)

    def ours(idx=None):
        xa.grad = ya.grad = None
        loss, _, _ = CF.infonce_loss(xa, ya, CF.sample_negatives(B, M, K) if idx is None else idx, temp)
        loss.backward()
        return loss

    def theirs(idx=None):
        xb.grad = yb.grad = None
        loss = torch_head(xb, yb, torch_negatives(B, M, K) if idx is None else idx.long(), temp)
        loss.backward()
        return loss

    la, lb = float(ours(fixed)), float(theirs(fixed))  # the same indices on both sides (also the warm-up of every shape)
    dxd = float((xa.grad.float() - xb.grad.float()).abs().max() / xb.grad.float().abs().max())
    dyd = float((ya.grad.float() - yb.grad.float()).abs().max() / yb.grad.float().abs().max())
    ours(), theirs()
    mem = {"ours_peak_mib": round(peak_above(ours), 1), "torch_peak_mib": round(peak_above(theirs), 1)}
    t = {"ours": [], "torch": []}
    for _ in range(args.windows):  # alternate the sides inside one process
        t["ours"].append(device_window(ours, args.calls))
        t["torch"].append(device_window(theirs, args.calls))
    print(json.dumps({"head": "negatives + logits + loss, forward + backward", **c, "N": N, "dtype": "bf16", "windows": args.windows,
                      "calls": args.calls, "loss_rel_diff": abs(la - lb) / abs(lb), "dx_rel_diff": dxd, "dy_rel_diff": dyd, **mem,
                      **{k: stats(v) for k, v in t.items()}}), flush=True)
    quantizer_part(args, CF)


def quantizer_part(args, CF):
    N, G, V, d, tau = 8 * 781, 2, 320, 128, 2.0
    g = torch.Generator().manual_seed(2)
    l0 = (torch.randn(N, G * V, generator=g) * 2).to(torch.bfloat16).cuda()
    v0 = torch.rand(G * V, d, generator=g).to(torch.bfloat16).cuda()
    dq = torch.randn(N, G * d, generator=g).to(torch.bfloat16).cuda()
    la, va = l0.clone().requires_grad_(True), v0.clone().requires_grad_(True)
    lb, vb = l0.clone().requires_grad_(True), v0.clone().requires_grad_(True)

    def ours():
        la.grad = va.grad = None
        q, ppl, _, _, _ = CF.gumbel_vector_quantize(la, va, G, tau)
        ((q.float() * dq).sum() + 0.1 * ppl).backward()
        return ppl

    def theirs():
        lb.grad = vb.grad = None
        q, ppl, _ = torch_quantizer(lb, vb.unsqueeze(0), G, tau)
        ((q.float() * dq).sum() + 0.1 * ppl).backward()
        return ppl

    pa, pb = float(ours().detach()), float(theirs().detach())  # (different noise on the two sides: prob_perplexity does not depend on it)
    mem = {"ours_peak_mib": round(peak_above(ours), 1), "torch_peak_mib": round(peak_above(theirs), 1)}
    t = {"ours": [], "torch": []}
    for _ in range(args.windows):
        t["ours"].append(device_window(ours, args.calls))
        t["torch"].append(device_window(theirs, args.calls))
    print(json.dumps({"part": "gumbel quantizer after its projection, forward + backward", "N": N, "G": G, "V": V, "d": d, "tau": tau,
                      "dtype": "bf16", "windows": args.windows, "calls": args.calls, "prob_perplexity_rel_diff": abs(pa - pb) / abs(pb), **mem,
                      **{k: stats(v) for k, v in t.items()}}), flush=True)


if __name__ == "__main__":
    main()
