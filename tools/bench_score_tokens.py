#!/usr/bin/env python3
"""cst_score_tokens (kernels.score_tokens) against the torch composition it replaces (sequence_scorer.score_tokens_torch on the
device: per member a float32 [B, T, V] log-softmax, a gather, logsumexp over the members) for bf16 logits, 32 x 64 target positions
with one third of them padding (right-padded sentences), V = 10 000, N = 1 and N = 3 members.  Seeded.

Prints one JSON line per N: per call, the device-event time of a window of calls (host launch cost included) for both, the kernel
time the library's profiling table records for cst_score_tokens' two launches, the bytes of the NON-PAD rows (each read once: N *
live rows * V * 2) and that byte count over kernel time as a fraction of the 8 TB/s HBM peak.  The calls of a window rotate
through enough input sets (--footprint-mb) that no set is still in the 256 MB last-level cache when its turn comes again.

  python tools/bench_score_tokens.py [--windows 5] [--calls 2000] [--torch-calls 50] [--footprint-mb 768]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BPS = 8e12
B, T, V, PAD = 32, 64, 10000, 1


def targets(seed=1):
    """Right-padded [B, T]: sentence lengths spread evenly so that a third of the positions is padding."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(4, V, (B, T), generator=g)
    lens = torch.linspace(T / 3, T, B).round().long()  # mean 2T/3
    t[torch.arange(T).unsqueeze(0) >= lens.unsqueeze(1)] = PAD
    return t


def window(fn, sets, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(calls):
        fn(sets[i % len(sets)])
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls  # ms per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--torch-calls", type=int, default=50)
    ap.add_argument("--footprint-mb", type=int, default=768)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU: there is no CPU fallback and no CPU number"
    K = importlib.import_module("chimera-st_amd.kernels")
    L = importlib.import_module("chimera-st_amd.lib")
    SS = importlib.import_module("chimera-st_amd.sequence_scorer")
    t = targets().cuda()
    live = int(t.ne(PAD).sum())
    g = torch.Generator(device="cuda").manual_seed(2)
    for N in (1, 3):
        nsets = max(2, -(-args.footprint_mb * (1 << 20) // (N * B * T * V * 2)))
        sets = [[(torch.randn(B, T, V, generator=g, device="cuda") * 2.0).to(torch.bfloat16) for _ in range(N)] for _ in range(nsets)]
        fused = lambda xs: K.score_tokens(xs, t, PAD)            # noqa: E731
        plain = lambda xs: SS.score_tokens_torch(xs, t, PAD)     # noqa: E731
        got, ref = fused(sets[0]), plain(sets[0])
        err = float((got[0] - ref[0]).abs().max())
        assert err < 1e-4 and torch.equal(got[2], ref[2]), err  # the two compute the same thing (fp32 evaluations of one formula)
        window(fused, sets, 50), window(plain, sets, 5)
        wf, wt = [], []
        for _ in range(args.windows):  # alternating, so that a drift of the clock meets both
            wf.append(window(fused, sets, args.calls))
            wt.append(window(plain, sets, args.torch_calls))
        L.prof_enable(True)
        window(fused, sets, args.calls)
        rec = L.prof_query()["loss"]
        L.prof_enable(False)
        kernel_ms = rec["ms"] / (rec["launches"])  # one record per cst_score_tokens call (both launches inside it)
        nbytes = N * live * V * 2
        print(json.dumps({"bench": "score_tokens", "dtype": "bf16", "rows": B * T, "live_rows": live, "V": V, "members": N,
                          "input_sets": nsets, "fused_ms_per_call_median": float(np.median(wf)), "fused_ms_per_call_windows": wf,
                          "torch_ms_per_call_median": float(np.median(wt)), "torch_ms_per_call_windows": wt,
                          "speedup_median": float(np.median(wt) / np.median(wf)), "kernel_ms_prof_table": kernel_ms,
                          "live_bytes": nbytes, "hbm_fraction_of_8TBps": nbytes / (kernel_ms * 1e-3) / HBM_BPS,
                          "max_abs_diff_to_torch": err}), flush=True)
        del sets


if __name__ == "__main__":
    main()
