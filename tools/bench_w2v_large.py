#!/usr/bin/env python3
"""Times the layer-norm feature-extractor kernels and one training update over a large-layout wav2vec2 (random weights).

  python tools/bench_w2v_large.py [--batch 32] [--seconds 10 30] [--update-batch 8] [--out profiles/w2v_large_bench.jsonl]

Per shape (bf16 storage, B utterances of `seconds` at 16 kHz): cst_conv0_ln_gelu_fwd / _bwd next to cst_conv0_gn_gelu_fwd / _bwd on the
same samples, and cst_ln_gelu_fwd / _bwd next to cst_layernorm_fwd / _bwd at the rows x 512 of conv layer 1; byte floors are the
bytes each entry has to move (samples in + B L C out; two or three passes over rows x C).  Then one s2t_transformer_w2v2 update
(forward + backward, bf16) over the 7 x 512 layer-norm CNN + 24 x 1024 x 16 encoder: ms per update, utterances per second and the
GEMM-class share of the kernel time (cst_prof).  Warm-up, then the median of `--iters` timed calls, each between two events."""
import argparse
import json
import os
import statistics
import sys
from argparse import Namespace
from importlib import import_module

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def kernels(K, B, seconds, iters):
    dt, C, k, st = torch.bfloat16, 512, 10, 5
    S = 16000 * seconds
    g = torch.Generator().manual_seed(1)
    wav = (0.1 * torch.randn(B, S, generator=g)).cuda()
    w = (0.5 * torch.randn(C, k, generator=g)).to(dt).cuda()
    bias, beta = ((0.1 * torch.randn(C, generator=g)).to(dt).cuda() for _ in range(2))
    gamma = (1 + 0.1 * torch.randn(C, generator=g)).to(dt).cuda()
    L = (S - k) // st + 1
    y, mean, rstd = K.conv0_ln_fwd(wav, w, bias, gamma, beta, k, st)
    dy = torch.randn(B, L, C, dtype=dt, device="cuda")
    yg, gmean, grstd, gram = K.conv0_fwd(wav, w, gamma, beta, k, st)
    floor = B * S * 4 + B * L * C * 2
    r = dict(what="conv0", B=B, seconds=seconds, frames=B * L, floor_bytes=floor,
             ln_fwd_ms=timed(lambda: K.conv0_ln_fwd(wav, w, bias, gamma, beta, k, st), iters),
             gn_fwd_ms=timed(lambda: K.conv0_fwd(wav, w, gamma, beta, k, st), iters),
             ln_bwd_ms=timed(lambda: K.conv0_ln_bwd(dy, wav, w, bias, gamma, beta, mean, rstd, k, st), iters),
             gn_bwd_ms=timed(lambda: K.conv0_bwd(dy, wav, w, gamma, beta, gmean, grstd, gram, k, st), iters))
    for key in ("ln_fwd", "gn_fwd", "ln_bwd", "gn_bwd"):
        r[key + "_GBps"] = round(floor / (r[key + "_ms"] * 1e-3) / 1e9, 1)
    out = [r]
    del y, yg, dy
    L1 = (L - 3) // 2 + 1  # conv layer 1 of the published layouts: k = 3, stride 2
    u = torch.randn(B, L1, C, dtype=dt, device="cuda")
    d1 = torch.randn(B, L1, C, dtype=dt, device="cuda")
    _, m1, r1 = K.ln_gelu_fwd(u, gamma, beta)
    u2 = u.view(B * L1, C)
    _, _, m2, r2 = K.layernorm_fwd(u2, None, gamma, beta, 1e-5)
    q = dict(what="ln_gelu", B=B, seconds=seconds, rows=B * L1, cols=C, fwd_floor_bytes=2 * B * L1 * C * 2, bwd_floor_bytes=3 * B * L1 * C * 2,
             ln_gelu_fwd_ms=timed(lambda: K.ln_gelu_fwd(u, gamma, beta), iters),
             layernorm_fwd_ms=timed(lambda: K.layernorm_fwd(u2, None, gamma, beta, 1e-5), iters),
             ln_gelu_bwd_ms=timed(lambda: K.ln_gelu_bwd(d1, u, gamma, beta, m1, r1, want_colsum=True), iters),
             layernorm_bwd_ms=timed(lambda: K.layernorm_bwd(d1.view(B * L1, C), u2, gamma, m2, r2), iters))
    q["fwd_ratio"] = round(q["ln_gelu_fwd_ms"] / q["layernorm_fwd_ms"], 3)
    q["bwd_ratio"] = round(q["ln_gelu_bwd_ms"] / q["layernorm_bwd_ms"], 3)
    q["ln_gelu_fwd_GBps"] = round(q["fwd_floor_bytes"] / (q["ln_gelu_fwd_ms"] * 1e-3) / 1e9, 1)
    q["ln_gelu_bwd_GBps"] = round(q["bwd_floor_bytes"] / (q["ln_gelu_bwd_ms"] * 1e-3) / 1e9, 1)
    out.append(q)
    return out


def update(B, seconds, iters):
    W = import_module("chimera-st_amd.wav2vec2")
    w2t = import_module("chimera-st_amd.w2v2_transformer")
    tasks = import_module("chimera-st_amd.tasks")
    crit_mod = import_module("chimera-st_amd.criterions")
    lib = import_module("chimera-st_amd.lib")
    w2t.SYNTHETIC_W2V["large_layout"] = W.wav2vec_small_args(
        extractor_mode="layer_norm", conv_bias=True, layer_norm_first=True, encoder_layers=24, encoder_embed_dim=1024,
        encoder_ffn_embed_dim=4096, encoder_attention_heads=16, final_dim=768, quantize_targets=False, encoder_layerdrop=0.0)
    task = tasks.TripletTask(Namespace(data=None, synthetic_vocab_size=10000))
    args = Namespace(w2v2_model_path="synthetic:large_layout", arch="s2t_transformer_w2v2")
    import_module("chimera-st_amd.registry").ARCH_CONFIG_REGISTRY["s2t_transformer_w2v2"](args)
    torch.manual_seed(1)
    model = w2t.S2TTransformerModelW2V2.build_model(args, task).to("cuda", torch.bfloat16).train()
    crit = crit_mod.LabelSmoothedCrossEntropyCriterion(task, False, 0.1)
    lens = [int(16000 * seconds * (1.0 - 0.5 * i / max(1, B - 1))) for i in range(B)]
    sample = tasks.synthetic_sample(task.target_dictionary, B, lens, [20 + i % 7 for i in range(B)], [12] * B, seed=3, device="cuda")

    def step():
        model.zero_grad(set_to_none=True)
        loss, _, _ = crit(model, sample)
        loss.backward()

    ms = timed(step, iters, warmup=3)
    lib.prof_enable(True)
    step()
    torch.cuda.synchronize()
    prof = lib.prof_query()
    lib.prof_enable(False)
    tot = sum(v["ms"] for v in prof.values())
    return dict(what="update", arch="s2t_transformer_w2v2", B=B, seconds_longest=seconds, fwd_bwd_ms=round(ms, 2), utterances_per_s=round(B / (ms * 1e-3), 1),
                gemm_share_of_kernel_ms=round(prof["gemm"]["ms"] / tot, 3) if tot > 0 else None,
                class_ms={k: round(v["ms"], 2) for k, v in prof.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=int, nargs="+", default=[10, 30])
    ap.add_argument("--update-batch", type=int, default=8)
    ap.add_argument("--update-seconds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--no-update", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "w2v_large_bench.jsonl"))
    a = ap.parse_args()
    K = import_module("chimera-st_amd.kernels")
    rows = []
    for s in a.seconds:
        rows += kernels(K, a.batch, s, a.iters)
        torch.cuda.empty_cache()
    if not a.no_update:
        rows.append(update(a.update_batch, a.update_seconds, max(5, a.iters // 3)))
    with open(a.out, "w") as f:
        for r in rows:
            r = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}
            print(json.dumps(r))
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
