#!/usr/bin/env python3
"""CF.ctc_loss (cst_ctc_fwd + cst_ctc_bwd) against the calls it replaces, F.ctc_loss(F.log_softmax(x.float(), -1), ...) of the installed
torch on the same device, forward + backward; and CF.ctc_greedy (one transfer of B*T + B int32) against the reference criterion's
validation loop (the fp32 [B, T, V] log-probabilities copied to the host, argmax().unique_consecutive() per utterance).  bf16 logits,
seeded.  Two batches: letters (B = 12, T = 800, V = 32, L ~ 250) and sentencepiece (B = 12, T = 800, V = 10000, L ~ 60), input lengths
spread over [T/2, T].

Prints one JSON line per batch: milliseconds per call from device events over a window of calls (host launch cost included; the
greedy decodes, which end on the host, by a host clock around the transfer), the windows alternating between the two sides; the median
window and the spread (max - min) of each side; and the largest difference of the two losses and gradients (they must agree: faster and
different is not faster).  Needs a GPU; there is no fallback.

  python tools/bench_ctc.py [--windows 5] [--calls 20]"""
import argparse
import importlib
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BATCHES = {"letter": dict(B=12, T=800, V=32, L=250), "sentencepiece": dict(B=12, T=800, V=10000, L=60)}


def make(name, seed=1):
    c = BATCHES[name]
    B, T, V, L = c["B"], c["T"], c["V"], c["L"]
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(T, B, V, generator=g) * 3).to(torch.bfloat16)
    in_len = torch.linspace(T / 2, T, B).round().long()
    tl = torch.minimum(torch.randint(int(0.8 * L), int(1.2 * L) + 1, (B,), generator=g), in_len // 3)  # feasible with room for repeats
    tg = torch.randint(1, V, (B, int(tl.max())), generator=g)
    return x.cuda(), tg.cuda(), tl.cuda(), in_len.cuda()


def device_window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def host_window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def stats(v):
    v = sorted(v)
    return {"median_ms": round(v[len(v) // 2], 4), "spread_ms": round(v[-1] - v[0], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ctc.py measures on the GPU; there is no fallback"
    CF = importlib.import_module("chimera-st_amd.functional")
    for name in BATCHES:
        x, tg, tl, il = make(name)
        mask = torch.arange(tg.shape[1], device="cuda")[None, :] < tl[:, None]
        flat = tg[mask]
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)

        def ours():
            xa.grad = None
            loss, _ = CF.ctc_loss(xa, tg, tl, il, 0, True)
            loss.backward()
            return loss

        def theirs():
            xb.grad = None
            loss = F.ctc_loss(F.log_softmax(xb.float(), -1), flat, il, tl, blank=0, reduction="sum", zero_infinity=True)
            loss.backward()
            return loss

        def greedy_ours():
            return CF.ctc_greedy(x, il, 0)[2].cpu()

        def greedy_theirs():
            lp = F.log_softmax(x.float(), -1).transpose(0, 1).contiguous().cpu()
            out = []
            for row, n in zip(lp, il_host):
                toks = row[:n].argmax(dim=-1).unique_consecutive()
                out.append(toks[toks != 0].tolist())
            return out

        il_host = il.tolist()
        la, lb = float(ours()), float(theirs())  # (also the warm-up of every shape)
        gdiff = float((xa.grad.float() - xb.grad.float()).abs().max())
        packed, ref = greedy_ours(), greedy_theirs()
        B, T = x.shape[1], x.shape[0]
        same = all(packed[b * T:b * T + int(packed[B * T + b])].tolist() == ref[b] for b in range(B))
        t = {"ours": [], "torch": [], "greedy_ours": [], "greedy_host_loop": []}
        for _ in range(args.windows):  # alternate the sides inside one process
            t["ours"].append(device_window(ours, args.calls))
            t["torch"].append(device_window(theirs, args.calls))
            t["greedy_ours"].append(host_window(greedy_ours, args.calls))
            t["greedy_host_loop"].append(host_window(greedy_theirs, max(args.calls // 4, 1)))
        print(json.dumps({"batch": name, **BATCHES[name], "dtype": "bf16", "windows": args.windows, "calls": args.calls,
                          "loss_rel_diff": abs(la - lb) / abs(lb), "grad_max_abs_diff": gdiff, "greedy_equal": same,
                          **{k: stats(v) for k, v in t.items()}}), flush=True)


if __name__ == "__main__":
    main()
