#!/usr/bin/env python3
"""Batch assembly of the `language_modeling` task, per batch, both routes of the same commit, on the GPU:

  host route      MonolingualDataset's host collater (per-block slices of the memory-mapped corpus, the shifted source, the two padded
                  tensors), pinning, and the three H2D copies — what EpochBatchIterator's background thread and
                  Trainer._prepare_sample do between them;
  resident route  the collater's record (block indices, width, lengths from the sizes), the index copy and cst_collate_blocks.

The corpus is synthetic with WMT-like sentence lengths (log-normal, median ~26 tokens, clipped to 1 .. 250; a uint16 stream, a
vocabulary of 10 000), written as .bin/.idx files and read back through the reader; batches are drawn as the trainer draws them:
--tokens-per-sample 512, --max-tokens 8192 (16 blocks of 512 tokens in `none` mode), shuffled.  Each figure is the median over a window
of batches, every batch timed on its own from a host clock to the device synchronise that ends it; the two routes alternate batch by
batch, so a drift meets both.  The parts are timed too: what runs on the background thread (collate + pin / the record) and what the
trainer's thread pays (copies / copy + launch), and the kernel alone from device events.

  python tools/bench_collate_blocks.py [--sentences 200000] [--modes none,complete] [--window 300] [--out profiles/collate_blocks_bench_mi355x.jsonl]"""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VOCAB = 10000


def make_corpus(d, n, seed=1):
    ID = importlib.import_module("chimera-st_amd.indexed_dataset")
    r = np.random.RandomState(seed)
    sizes = np.clip(np.exp(r.normal(3.25, 0.6, n)).astype(np.int64), 1, 250)
    stream = r.randint(4, VOCAB, int(sizes.sum())).astype(np.uint16)
    stream[np.cumsum(sizes) - 1] = 2  # every sentence ends in eos
    ID.write_dataset(os.path.join(d, "train"), stream, sizes)
    return int(sizes.sum())


def sync_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def host_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def to_device(sample):
    mv = lambda x: x.to("cuda", non_blocking=True) if torch.is_tensor(x) else ({k: mv(v) for k, v in x.items()} if isinstance(x, dict) else x)
    return mv(sample)


def measure(args, tmp, ntok, mode, d):
    M = importlib.import_module("chimera-st_amd.monolingual_dataset")
    ID = importlib.import_module("chimera-st_amd.indexed_dataset")
    D = importlib.import_module("chimera-st_amd.data")
    K = importlib.import_module("chimera-st_amd.kernels")
    corpus = ID.MMapIndexedDataset(os.path.join(tmp, "train"))
    tb = M.TokenBlockDataset(corpus, corpus.sizes, args.tokens_per_sample, d.pad(), d.eos(), break_mode=mode)
    ds = M.MonolingualDataset(tb, tb.sizes, d, shuffle=True)
    with D.numpy_seed(1):
        idx = ds.ordered_indices()
    batches = ds.batch_by_size(idx, max_tokens=args.max_tokens, required_batch_size_multiple=8)
    with D.numpy_seed(2):
        np.random.shuffle(batches)
    batches = batches[:args.warmup + args.window]
    assert len(batches) == args.warmup + args.window, "corpus too small for the window"
    os.environ.pop("CST_BLOCK_COLLATE", None)
    assert ds.enable_resident()
    rb = ds.resident
    t = {k: [] for k in ("host_total", "host_collate_pin", "host_h2d", "res_total", "res_record", "res_copy_launch", "res_kernel")}
    words, rows = [], []
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for n, batch in enumerate(batches):
        # host route: whole, then its two halves on a second pass over the same batch
        ms_total, dev_h = sync_ms(lambda: to_device(D._pin(ds.host_batch(batch))))
        ms_cp, pinned = host_ms(lambda: D._pin(ds.host_batch(batch)))
        ms_h2d, _ = sync_ms(lambda: to_device(pinned))
        # resident route
        ms_rtotal, dev_r = sync_ms(lambda: rb.materialize(ds.record(batch)))
        ms_rec, rec = host_ms(lambda: ds.record(batch))
        ms_cl, _ = sync_ms(lambda: rb.materialize(rec))
        T = rec["net_input"]["block_width"]
        dev_idx = rec["net_input"]["block_idx"].cuda()
        torch.cuda.synchronize()
        a.record()
        for _ in range(10):
            rb_out = K.collate_blocks(rb._dev[0], rb.tok_dtype, rb._dev[1], dev_idx, T, rb.pad, rb.eos)
        b.record()
        b.synchronize()
        for k in ("src_tokens", "src_lengths"):  # the two routes build the same batch
            assert torch.equal(dev_h["net_input"][k], dev_r["net_input"][k]), k
        assert torch.equal(dev_h["target"], dev_r["target"]) and torch.equal(rb_out[2], dev_r["target"])
        if n < args.warmup:
            continue
        for k, v in (("host_total", ms_total), ("host_collate_pin", ms_cp), ("host_h2d", ms_h2d), ("res_total", ms_rtotal),
                     ("res_record", ms_rec), ("res_copy_launch", ms_cl), ("res_kernel", a.elapsed_time(b) / 10)):
            t[k].append(v)
        words.append(len(batch) * (2 * T + 1))
        rows.append(len(batch))
    med = {k + "_ms_median": float(np.median(v)) for k, v in t.items()}
    p90 = {k + "_ms_p90": float(np.percentile(v, 90)) for k, v in t.items()}
    return {"bench": "collate_blocks", "sample_break_mode": mode, "tokens_per_sample": args.tokens_per_sample, "sentences": args.sentences,
            "corpus_tokens": ntok, "blocks": len(ds), "resident_mb": rb.nbytes / 2 ** 20, "max_tokens": args.max_tokens,
            "window_batches": args.window, "rows_per_batch_median": float(np.median(rows)),
            "int64_words_per_batch_median": float(np.median(words)), **med, **p90,
            "host_over_resident_total": med["host_total_ms_median"] / med["res_total_ms_median"],
            "trainer_thread_host_over_resident": med["host_h2d_ms_median"] / med["res_copy_launch_ms_median"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, default=200000)
    ap.add_argument("--tokens-per-sample", type=int, default=512)
    ap.add_argument("--max-tokens", type=int, default=8192)
    ap.add_argument("--modes", default="none,complete")
    ap.add_argument("--window", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "collate_blocks_bench_mi355x.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU: there is no CPU number"
    d = importlib.import_module("chimera-st_amd.dictionary").Dictionary.synthetic(VOCAB)
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        ntok = make_corpus(tmp, args.sentences)
        for mode in args.modes.split(","):
            line = measure(args, tmp, ntok, mode, d)
            lines.append(line)
            print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("".join(json.dumps(l) + "\n" for l in lines))


if __name__ == "__main__":
    main()
