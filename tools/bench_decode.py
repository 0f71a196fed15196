#!/usr/bin/env python3
"""Decode throughput of BASELINE config 5 (SURVEY §8d "Decode"): s2t_transformer_l (d 1024, ffn 4096, 16 heads, 12 encoder +
6 decoder layers, 10 000-way tied vocabulary), filter-bank input, beam 5, incremental-state decode, 1 x MI355X, bf16.

  python tools/bench_decode.py [--batch 32] [--frames 3000] [--beam 5] [--max-len 200] [--reps 3] [--mirror] [--ensemble N]
                               [--no-repeat-ngram-size N] [--sampling [--sampling-topk K] [--sampling-topp P]]
                               [--diverse-beam-groups G [--diverse-beam-strength S]] [--diversity-rate R]
                               [--lm-layers L [--lm-weight W]] [--constraints {ordered,unordered}]

Prints one JSON line: utterances/s and generated tokens/s of the device-resident loop (decode_engine.py: one captured HIP
graph per step), the per-step time, the encoder time, and — with --mirror — the same numbers for the host-driven
module-by-module loop (fused=False).  Random-init weights emit eos only when forced, so every sentence runs the full
max_len + 1 steps: the reported rate is the worst case for the configured max_len.
--ensemble N decodes N independently seeded copies of the model as a checkpoint ensemble (every member's encoder and decoder run;
one beam step over the N logits matrices) and adds "models" and "nodes_per_step" to the line.
--sampling decodes with the Sampling strategy (every hypothesis an independent sample) on the same engine; --diverse-beam-groups and
--diversity-rate with DiverseBeamSearch / DiverseSiblingsSearch (both inside the beam step's merge kernel).
--lm-layers L adds shallow fusion with a random pre-norm language model of the decoder's width, heads and ffn size, L layers deep
(weight --lm-weight): the engine runs it as a member without cross attention and fuses it inside the beam step's row kernel.
--constraints R decodes the batch a second time with LexicallyConstrainedBeamSearch (representation R) and synthetic constraints — two
one-token phrases and one two-token phrase per sentence — and adds "lexical": its ms_per_step beside the plain-beam figure of the same
run (same models, batch and step count; the constraint code lives in the two search kernels, so nodes_per_step is the same)."""
import argparse
import importlib
import json
import os
import sys
import time
from argparse import Namespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=3000, help="max filter-bank frames (10 ms each)")
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--max-len", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--arch", default="s2t_transformer_l")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--mirror", action="store_true", help="also time the host-driven loop (fused=False)")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--cross-kernel", default="flash", choices=["flash", "flash_hm", "shared"])
    ap.add_argument("--ensemble", type=int, default=1, help="decode N independently seeded copies of the model as an ensemble")
    ap.add_argument("--no-repeat-ngram-size", type=int, default=0, help="decode with n-gram blocking (0 = off)")
    ap.add_argument("--sampling", action="store_true", help="sample instead of beam search")
    ap.add_argument("--sampling-topk", type=int, default=-1)
    ap.add_argument("--sampling-topp", type=float, default=-1.0)
    ap.add_argument("--diverse-beam-groups", type=int, default=-1, help="diverse beam search with this many groups (--beam divisible)")
    ap.add_argument("--diverse-beam-strength", type=float, default=0.5)
    ap.add_argument("--diversity-rate", type=float, default=-1.0, help="diverse siblings search with this rate (negative = off)")
    ap.add_argument("--lm-layers", type=int, default=0, help="fuse a random language model of this depth (0 = off)")
    ap.add_argument("--lm-weight", type=float, default=0.3)
    ap.add_argument("--constraints", default=None, choices=["ordered", "unordered"],
                    help="also time lexically constrained beam search with synthetic constraints (three phrases per sentence)")
    ap.add_argument("--attention", action="store_true", help="decode with return_attention (--print-alignment): every step also records the "
                    "last layer's head-averaged cross attention; with --profile the mean time of that launch and of the cross-attention "
                    "launch in front of it are reported")
    ap.add_argument("--profile", action="store_true", help="per-class GPU time of one eager decode loop (hipEvent pairs)")
    args = ap.parse_args()
    if sum((args.sampling, args.diverse_beam_groups > 0, args.diversity_rate > 0)) > 1:
        ap.error("--sampling, --diverse-beam-groups and --diversity-rate are mutually exclusive")
    if args.diverse_beam_groups > 0 and args.beam % args.diverse_beam_groups != 0:
        ap.error("--beam must be divisible by --diverse-beam-groups")
    if args.constraints and (args.sampling or args.diverse_beam_groups > 0 or args.diversity_rate > -1):
        ap.error("--constraints times lexically constrained beam search against PLAIN beam search")

    importlib.import_module("chimera-st_amd")
    s2t = importlib.import_module("chimera-st_amd.s2t_transformer")
    tasks = importlib.import_module("chimera-st_amd.tasks")
    reg = importlib.import_module("chimera-st_amd.registry")
    lib = importlib.import_module("chimera-st_amd.lib")
    SG = importlib.import_module("chimera-st_amd.sequence_generator").SequenceGenerator
    sg_mod = importlib.import_module("chimera-st_amd.sequence_generator")
    Sampling, DiverseBeamSearch, DiverseSiblingsSearch = sg_mod.Sampling, sg_mod.DiverseBeamSearch, sg_mod.DiverseSiblingsSearch
    lib.load()
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    torch.manual_seed(1)
    task = tasks.SpeechToTextTask(Namespace(data=None, synthetic_vocab_size=10000))
    ns = Namespace(share_decoder_input_output_embed=True, dropout=0.0)
    reg.ARCH_CONFIG_REGISTRY[args.arch](ns)
    model = s2t.S2TTransformerModel.build_model(ns, task).to("cuda", dt).eval()
    models = [model]
    for k in range(1, args.ensemble):
        torch.manual_seed(1 + k)
        models.append(s2t.S2TTransformerModel.build_model(ns, task).to("cuda", dt).eval())

    lm = None
    if args.lm_layers > 0:
        tlm = importlib.import_module("chimera-st_amd.transformer_lm")
        cu = importlib.import_module("chimera-st_amd.checkpoint_utils")
        torch.manual_seed(101)
        lm_ns = Namespace(decoder_layers=args.lm_layers, decoder_embed_dim=ns.decoder_embed_dim, decoder_ffn_embed_dim=ns.decoder_ffn_embed_dim,
                          decoder_attention_heads=ns.decoder_attention_heads, dropout=0.0, share_decoder_input_output_embed=True)
        lm = tlm.TransformerLanguageModel.build_model(lm_ns, cu._DictTask(task.target_dictionary)).to("cuda", dt).eval()
    lm_kw = dict(lm_model=lm, lm_weight=args.lm_weight) if lm is not None else {}
    if args.attention:
        lm_kw["return_attention"] = True

    g = torch.Generator().manual_seed(1)
    lens = torch.randint(args.frames // 3, args.frames + 1, (args.batch,), generator=g).sort(descending=True)[0]
    lens[0] = args.frames
    src = torch.randn(args.batch, args.frames, 80, generator=g).to(dt).cuda()
    sample = {"net_input": {"src_tokens": src, "src_lengths": lens.cuda()}}

    def timed(gen, **kw):
        hyps = gen.generate(models, sample, **kw)  # warm-up (graph capture, code objects)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            hyps = gen.generate(models, sample, **kw)
        torch.cuda.synchronize()
        dt_ = (time.perf_counter() - t0) / args.reps
        ntok = sum(len(h[0]["tokens"]) for h in hyps)
        return dt_, ntok

    with torch.no_grad():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            for m in models:
                m.encoder(src, sample["net_input"]["src_lengths"])
        torch.cuda.synchronize()
        enc_s = (time.perf_counter() - t0) / args.reps

    def strategy():
        if args.sampling:
            return Sampling(task.target_dictionary, args.sampling_topk, args.sampling_topp)
        if args.diverse_beam_groups > 0:
            return DiverseBeamSearch(task.target_dictionary, args.diverse_beam_groups, args.diverse_beam_strength)
        if args.diversity_rate > -1:
            return DiverseSiblingsSearch(task.target_dictionary, args.diversity_rate)
        return None

    fused = SG(models, task.target_dictionary, beam_size=args.beam, max_len_a=0, max_len_b=args.max_len, use_graph=not args.no_graph,
               cross_kernel=args.cross_kernel, no_repeat_ngram_size=args.no_repeat_ngram_size, search_strategy=strategy(), **lm_kw)
    t_f, ntok = timed(fused)
    steps = args.max_len + 1
    out = {"metric": "decode utterances/sec, s2t_transformer_l beam 5, 1 MI355X", "config": {"arch": args.arch, "batch": args.batch,
           "beam": args.beam, "max_frames": args.frames, "max_len": args.max_len, "dtype": args.dtype, "graph": not args.no_graph},
           "utterances_per_s": args.batch / t_f, "tokens_per_s": ntok / t_f, "best_hyp_tokens": ntok, "s_per_batch": t_f,
           "encoder_s": enc_s, "ms_per_step": (t_f - enc_s) / steps * 1e3, "hyp_rows_per_step": args.batch * args.beam}
    if args.sampling:
        out["config"].update(sampling=True, sampling_topk=args.sampling_topk, sampling_topp=args.sampling_topp)
        out["nodes_per_step"] = fused._engine.nodes_per_step(dt, args.batch * args.beam)
    if args.diverse_beam_groups > 0:
        out["config"].update(diverse_beam_groups=args.diverse_beam_groups, diverse_beam_strength=args.diverse_beam_strength)
        out["nodes_per_step"] = fused._engine.nodes_per_step(dt, args.batch * args.beam)
    elif args.diversity_rate > -1 and not args.sampling:
        out["config"].update(diversity_rate=args.diversity_rate)
        out["nodes_per_step"] = fused._engine.nodes_per_step(dt, args.batch * args.beam)
    if args.no_repeat_ngram_size:
        out["config"]["no_repeat_ngram_size"] = args.no_repeat_ngram_size
        out["nodes_per_step"] = fused._engine.nodes_per_step(dt, args.batch * args.beam)
    if args.ensemble > 1:
        out["models"] = args.ensemble
        out["nodes_per_step"] = fused._engine.nodes_per_step(dt, args.batch * args.beam)
    if lm is not None:
        out["config"].update(lm_layers=args.lm_layers, lm_weight=args.lm_weight)
        out["nodes_per_step"] = fused._engine.nodes_per_step(dt, args.batch * args.beam)
    if args.attention:
        out["config"]["attention"] = True
        out["nodes_per_step"] = fused._engine.nodes_per_step(dt, args.batch * args.beam)
    if args.constraints:
        lc = importlib.import_module("chimera-st_amd.lexical_constraints")
        gc = torch.Generator().manual_seed(7)
        toks = torch.randint(4, 10000, (args.batch, 4), generator=gc).tolist()  # per sentence: [a], [b], [c d]
        packed = lc.pack_constraints([[[a], [b], [c, d]] for a, b, c, d in toks], pad=task.target_dictionary.pad(), eos=task.target_dictionary.eos())
        lex = SG(models, task.target_dictionary, beam_size=args.beam, max_len_a=0, max_len_b=args.max_len, use_graph=not args.no_graph,
                 cross_kernel=args.cross_kernel, no_repeat_ngram_size=args.no_repeat_ngram_size,
                 search_strategy=sg_mod.LexicallyConstrainedBeamSearch(task.target_dictionary, args.constraints), **lm_kw)
        t_x, ntok_x = timed(lex, constraints=packed)
        assert lex._engine is not None
        out["lexical"] = {"representation": args.constraints, "phrases_per_sentence": 3, "ms_per_step": (t_x - enc_s) / steps * 1e3,
                          "utterances_per_s": args.batch / t_x, "best_hyp_tokens": ntok_x,
                          "nodes_per_step": lex._engine.nodes_per_step(dt, args.batch * args.beam)}
        out["nodes_per_step"] = fused._engine.nodes_per_step(dt, args.batch * args.beam)
    if args.mirror:
        mirror = SG(models, task.target_dictionary, beam_size=args.beam, max_len_a=0, max_len_b=args.max_len, fused=False,
                    search_strategy=strategy(), **lm_kw)
        t_m, ntok_m = timed(mirror)
        out["mirror_host_loop"] = {"utterances_per_s": args.batch / t_m, "tokens_per_s": ntok_m / t_m, "s_per_batch": t_m,
                                   "ms_per_step": (t_m - enc_s) / steps * 1e3}
        out["speedup_vs_host_loop"] = t_m / t_f
    if args.profile:
        eager = SG(models, task.target_dictionary, beam_size=args.beam, max_len_a=0, max_len_b=args.max_len, use_graph=False,
                   cross_kernel=args.cross_kernel, return_attention=args.attention)
        eager.generate(models, sample)
        lib.prof_enable(True)
        eager.generate(models, sample)
        torch.cuda.synchronize()
        table = lib.prof_query()
        lib.prof_enable(False)
        out["per_class_ms_per_step"] = {k: round(v["ms"] / steps, 4) for k, v in table.items() if v["launches"]}
        out["launches_per_step"] = sum(v["launches"] for v in table.values()) / steps
        if args.attention:  # the attn_fwd launches in order: every cst_attn_avg_probs follows the last layer's cross attention
            recs = lib.prof_dump(lib.K_ATTN_FWD)
            at = [i for i, r in enumerate(recs) if r[3].startswith("avg_probs")]
            if at:
                out["attention_probs_us"] = round(1e3 * sum(recs[i][0] for i in at) / len(at), 2)
                out["last_cross_attn_us"] = round(1e3 * sum(recs[i - 1][0] for i in at if i > 0) / len(at), 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
