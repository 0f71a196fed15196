#!/usr/bin/env python3
"""CTC prefix beam search on the device (CF.ctc_prefix_beam_search: cst_ctc_topn + cst_ctc_beam, one transfer of the packed result)
against the host route on the same emissions (ctc_decoder.prefix_beam_search_host, numpy), with the best-path decode (CF.ctc_greedy)
beside them.  bf16 logits, seeded, B = 12, T = 800, input lengths spread over [T/2, T].  Two batches: letters (V = 32, K = 50, every
class listed) and sentencepiece (V = 10000, K = 50, N = 100).

Prints one JSON line per batch: milliseconds per call by a host clock around the call (every route ends on the host), the median of the
windows and their spread; the host route runs once (it takes seconds); and whether the two routes' top hypotheses agree.  Needs a GPU;
there is no fallback.

  python tools/bench_ctc_beam.py [--windows 5] [--calls 5]"""
import argparse
import importlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BATCHES = {"letter": dict(B=12, T=800, V=32, K=50, N=31), "sentencepiece": dict(B=12, T=800, V=10000, K=50, N=100)}


def make(name, seed=1):
    c = BATCHES[name]
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(c["T"], c["B"], c["V"], generator=g) * 3).to(torch.bfloat16)
    return x.cuda(), torch.linspace(c["T"] / 2, c["T"], c["B"]).round().long().cuda()


def windows(fn, n, calls):
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / calls)
    out.sort()
    return out[len(out) // 2], out[-1] - out[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    CF = importlib.import_module("chimera-st_amd.functional")
    CD = importlib.import_module("chimera-st_amd.ctc_decoder")
    for name, c in BATCHES.items():
        x, il = make(name)
        beam = lambda: CF.ctc_prefix_beam_search(x, il, 0, c["K"], c["N"], 25.0, 1)
        greedy = lambda: CF.ctc_greedy(x, il, 0)[2].cpu()
        beam(), greedy()  # warm-up
        b_ms, b_sp = windows(beam, a.windows, a.calls)
        g_ms, g_sp = windows(greedy, a.windows, a.calls)
        t0 = time.perf_counter()
        host = CD.prefix_beam_search_host(x, il, 0, c["K"], c["N"], 25.0, 1)
        h_ms = (time.perf_counter() - t0) * 1e3
        dev = beam()
        same = sum(d[0][0] == h[0][0] for d, h in zip(dev, host))
        print(json.dumps({"batch": name, **c, "device_beam_ms": round(b_ms, 3), "device_beam_spread_ms": round(b_sp, 3),
                          "host_beam_ms": round(h_ms, 1), "greedy_ms": round(g_ms, 3), "greedy_spread_ms": round(g_sp, 3),
                          "top_hypotheses_equal": "%d/%d" % (same, c["B"])}), flush=True)


if __name__ == "__main__":
    main()
