#!/usr/bin/env python3
"""Batch assembly of the `translation` task, per batch, both routes of the same commit, on the GPU:

  host route      LanguagePairDataset's host collater (per-sentence slices of the memory-mapped corpus, the three padded tensors), pinning,
                  and the four H2D copies — what EpochBatchIterator's background thread and Trainer._prepare_sample do between them;
  resident route  the collater's record (indices, widths, lengths from the sizes), the index copy and cst_collate_pairs.

The corpus is synthetic with WMT-like lengths (log-normal, median ~26 sentencepiece tokens, clipped to 1 .. 250; uint16 streams, a
vocabulary of 10 000), written as .bin/.idx files and read back through the reader; batches are drawn as the trainer draws them
(--max-tokens 4096, batch sizes a multiple of 8, shuffled).  Each figure is the median over a window of batches, every batch timed on its
own from a host clock to the device synchronise that ends it; the two routes alternate batch by batch, so a drift meets both.  The parts
are timed too: what runs on the background thread (collate + pin / the record) and what the trainer's thread pays (copies / copy + launch),
and the kernel alone from device events.

With --update it also times the MT update itself (one micro-batch per update, median) at the tiny test dimensions and at the script's
(train-en2any-MT.sh: 6 encoder layers, 512 wide, 64 memory slots, wav2vec_small in the model but idle), so the share is known.

  python tools/bench_collate_pairs.py [--sentences 200000] [--window 300] [--update] [--out profiles/collate_pairs_bench_mi355x.jsonl]"""
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
    src = np.clip(np.exp(r.normal(3.25, 0.6, n)).astype(np.int64), 1, 250)
    tgt = np.clip((src * r.uniform(0.8, 1.25, n)).astype(np.int64) + 1, 1, 250)
    for lang, sizes in (("en", src), ("de", tgt)):
        stream = r.randint(4, VOCAB, int(sizes.sum())).astype(np.uint16)
        stream[np.cumsum(sizes) - 1] = 2  # every sentence ends in eos
        ID.write_dataset(os.path.join(d, "train.en-de." + lang), stream, sizes)
    return int(src.sum() + tgt.sum())


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, default=200000)
    ap.add_argument("--max-tokens", type=int, default=4096)
    ap.add_argument("--window", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--update", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "collate_pairs_bench_mi355x.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU: there is no CPU number"
    P = importlib.import_module("chimera-st_amd.language_pair_dataset")
    D = importlib.import_module("chimera-st_amd.data")
    Dictionary = importlib.import_module("chimera-st_amd.dictionary").Dictionary
    d = Dictionary.synthetic(VOCAB)
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        ntok = make_corpus(tmp, args.sentences)
        ds = P.load_langpair_dataset(tmp, "train", "en", d, "de", d)
        with D.numpy_seed(1):
            idx = ds.ordered_indices()
        batches = ds.batch_by_size(idx, max_tokens=args.max_tokens, required_batch_size_multiple=8)
        with D.numpy_seed(2):
            np.random.shuffle(batches)
        batches = batches[:args.warmup + args.window]
        assert len(batches) == args.warmup + args.window, "corpus too small for the window"
        os.environ.pop("CST_PAIR_COLLATE", None)
        assert ds.enable_resident()
        rp = ds.resident
        K = importlib.import_module("chimera-st_amd.kernels")
        t = {k: [] for k in ("host_total", "host_collate_pin", "host_h2d", "res_total", "res_record", "res_copy_launch", "res_kernel")}
        words, rows = [], []
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for n, batch in enumerate(batches):
            # host route: whole, then its two halves on a second pass over the same batch
            ms_total, dev_h = sync_ms(lambda: to_device(D._pin(ds.host_batch(batch))))
            ms_cp, pinned = host_ms(lambda: D._pin(ds.host_batch(batch)))
            ms_h2d, _ = sync_ms(lambda: to_device(pinned))
            # resident route
            ms_rtotal, dev_r = sync_ms(lambda: rp.materialize(ds.record(batch)))
            ms_rec, rec = host_ms(lambda: ds.record(batch))
            ms_cl, _ = sync_ms(lambda: rp.materialize(rec))
            S, T = rec["net_input"]["pair_widths"]
            dev_idx = rec["net_input"]["pair_idx"].cuda()
            torch.cuda.synchronize()
            a.record()
            for _ in range(10):
                rp_out = K.collate_pairs(rp._dev[0], rp._dev[2], rp.tok_dtype, rp._dev[1], rp._dev[3], dev_idx, S, T, rp.pad, rp.eos,
                                         rp.left_pad_source, rp.left_pad_target)
            b.record()
            b.synchronize()
            for k in ("src_tokens", "src_lengths", "prev_output_tokens"):  # the two routes build the same batch
                assert torch.equal(dev_h["net_input"][k], dev_r["net_input"][k]), k
            assert torch.equal(dev_h["target"], dev_r["target"]) and torch.equal(rp_out[3], dev_r["target"])
            if n < args.warmup:
                continue
            for k, v in (("host_total", ms_total), ("host_collate_pin", ms_cp), ("host_h2d", ms_h2d), ("res_total", ms_rtotal),
                         ("res_record", ms_rec), ("res_copy_launch", ms_cl), ("res_kernel", a.elapsed_time(b) / 10)):
                t[k].append(v)
            words.append(len(batch) * (S + 2 * T + 1))
            rows.append(len(batch))
        med = {k + "_ms_median": float(np.median(v)) for k, v in t.items()}
        p90 = {k + "_ms_p90": float(np.percentile(v, 90)) for k, v in t.items()}
        line = {"bench": "collate_pairs", "sentences": args.sentences, "corpus_tokens": ntok, "resident_mb": rp.nbytes / 2 ** 20,
                "max_tokens": args.max_tokens, "window_batches": args.window, "rows_per_batch_median": float(np.median(rows)),
                "int64_words_per_batch_median": float(np.median(words)), **med, **p90,
                "host_over_resident_total": med["host_total_ms_median"] / med["res_total_ms_median"],
                "trainer_thread_host_over_resident": med["host_h2d_ms_median"] / med["res_copy_launch_ms_median"]}
        lines.append(line)
        print(json.dumps(line), flush=True)
        if args.update:
            for name, flags in (("tiny", ["--encoder-layers", "2", "--encoder-embed-dim", "64", "--encoder-ffn-embed-dim", "128",
                                          "--encoder-attention-heads", "2", "--decoder-attention-heads", "2", "--decoder-layers", "2",
                                          "--conv-channels", "64", "--interlingua-length", "8", "--interlingua-layers", "2",
                                          "--w2v2-model-path", "synthetic:golden_tiny"]),
                                ("script", ["--encoder-layers", "6", "--encoder-embed-dim", "512", "--interlingua-length", "64",
                                            "--w2v2-model-path", "synthetic:wav2vec_small"])):
                line = time_update(name, flags, ds, rp, batches[args.warmup:], d, med)
                lines.append(line)
                print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("".join(json.dumps(l) + "\n" for l in lines))


def time_update(name, arch_flags, ds, rp, batches, d, med):
    """Median wall time of one MT update (one micro-batch, bf16, dropout 0.1) fed from the resident route, batch in hand; then the
    training loop as the driver runs it — EpochBatchIterator's background thread eight batches ahead, pinning on the host route — over
    windows of 100 updates per route, the routes alternating (host, resident, host, resident)."""
    import ast
    from argparse import Namespace
    reg = importlib.import_module("chimera-st_amd.registry")
    tasks = importlib.import_module("chimera-st_amd.tasks")
    importlib.import_module("chimera-st_amd.cli")  # (registers models and criteria)
    w2t = importlib.import_module("chimera-st_amd.w2v2_transformer")
    if name == "tiny":
        g = np.load(os.path.join(ROOT, "tests", "golden", "chimera_tiny.npz"), allow_pickle=False)
        w2t.SYNTHETIC_W2V["golden_tiny"] = Namespace(**ast.literal_eval(str(g["meta/w2v_args"])))
    args = reg.parse_args_and_arch(["/nowhere", "--task", "translation", "--criterion", "label_smoothed_cross_entropy", "--label-smoothing", "0.1",
                                    "--arch", "s2t_transformer_w2v2_interlingua_base", "--share-decoder-input-output-embed", "--dropout", "0.1",
                                    "--optimizer", "adam", "--adam-betas", "(0.9, 0.98)", "--clip-norm", "0.0", "--lr", "5e-4",
                                    "--weight-decay", "0.0001", "--warmup-updates", "4000", "--bf16"] + arch_flags)
    task = tasks.TranslationTask(args, d, d)
    model = task.build_model(args)
    trainer = importlib.import_module("chimera-st_amd.trainer").Trainer(args, task, model, task.build_criterion(args), device="cuda")
    times = []
    D = importlib.import_module("chimera-st_amd.data")
    for n, batch in enumerate(batches[:40]):
        rec = ds.record(batch)
        ms, out = sync_ms(lambda: trainer.train_step([rec]))
        assert out is not None and np.isfinite(out["loss"])
        if n >= 10:
            times.append(ms)
    upd = float(np.median(times))
    loop = {"host": [], "resident": []}
    for w, route in enumerate(("host", "resident", "host", "resident")):
        ds.resident = rp if route == "resident" else None
        chunk = batches[40 + (w % 2) * 110:40 + (w % 2) * 110 + 110]  # (both routes see the same two chunks of batches)
        assert len(chunk) == 110, "--window too small for the loop measurement (260 needed)"
        it = D.EpochBatchIterator(ds, chunk, pin_memory=True).next_epoch_itr(shuffle=False, buffer_size=8)
        for n, sample in enumerate(it):
            if n == 10:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            trainer.train_step([sample])
        torch.cuda.synchronize()
        loop[route].append((time.perf_counter() - t0) * 1e3 / 100)
    ds.resident = rp
    return {"loop_ms_per_update_host_windows": loop["host"], "loop_ms_per_update_resident_windows": loop["resident"],
            "loop_host_over_resident": float(np.mean(loop["host"]) / np.mean(loop["resident"])),"bench": "mt_update", "dims": name, "params": sum(p.numel() for p in model.parameters()), "dtype": "bf16",
            "update_ms_median": upd, "updates_timed": len(times),
            "host_h2d_share_of_update": med["host_h2d_ms_median"] / upd, "host_total_share_of_update": med["host_total_ms_median"] / upd,
            "resident_copy_launch_share_of_update": med["res_copy_launch_ms_median"] / upd}


if __name__ == "__main__":
    main()
