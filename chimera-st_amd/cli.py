"""Command-line drivers — the part of fairseq_cli/train.py (:44-330) and fairseq_cli/generate.py (:57-390) that sits
around the hot path, so that the flag sets of chimera/scripts/train-en2any-ST.sh and chimera/generate/generate-mustc-final.sh
drive this build unchanged:

  python fairseq_train.py <data> --task triplet --arch s2t_transformer_w2v2_interlingua_base --config-yaml config_wave.yaml ...
  python fairseq_generate.py <data> --task triplet --path ckpt.pt --gen-subset tst-COMMON_wave --beam 10 --lenpen 1.5 ...
  python fairseq_interactive.py <data> --task triplet --config-yaml config_wave.yaml --path ckpt.pt   (fairseq_cli/interactive.py:42-307,
                                chimera/scripts/interactive-en2any-ST.sh: typed audio paths; sentences and LM prompts on those checkpoints)

`--fp16` selects the reduced-precision path of this hardware: bf16 storage with fp32 accumulation (no loss scaling).  One
process per GPU (torchrun-style env: RANK / WORLD_SIZE / LOCAL_RANK); each rank reads its own shard of the epoch's batches."""
import argparse
import json
import math
import os
import sys
import time

import torch

from . import checkpoint_utils, criterions, fbank, registry, s2t_transformer, tasks, transformer_lm, w2v2_transformer, w2v2_transformer_interlingua, wav2vec2_asr  # noqa: F401
from .distributed import distributed_init, launch_ranks, needs_self_launch
from .hostcfg import limit_host_threads
from .trainer import Trainer


def _log(rank, **kw):
    if rank == 0:
        print(json.dumps(kw), flush=True)


def _extra_train_flags(argv):
    """Flags of the reference scripts that configure subsystems outside this build (or have a fixed meaning here)."""
    p = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    p.add_argument("--best-checkpoint-metric", default="loss")
    p.add_argument("--maximize-best-checkpoint-metric", action="store_true")
    p.add_argument("--validate-interval", type=int, default=1)
    p.add_argument("--no-epoch-checkpoints", action="store_true")
    p.add_argument("--no-save", action="store_true")
    p.add_argument("--restore-file", default="checkpoint_last.pt")
    p.add_argument("--disable-validation", action="store_true")
    p.add_argument("--data-buffer-size", type=int, default=8)
    p.add_argument("--label-smoothing-placeholder", default=None, help=argparse.SUPPRESS)
    return p.parse_known_args(argv)


def validate(trainer, task, args, subset, rank, world):
    ds = task.load_dataset(subset) if subset not in task.datasets else task.dataset(subset)
    itr = task.get_batch_iterator(ds, max_tokens=args.max_tokens, max_sentences=args.batch_size, max_positions=task.max_positions(),
                                  ignore_invalid_inputs=True, seed=args.seed, num_shards=world, shard_id=rank)
    totals = {}
    for sample in itr.next_epoch_itr(shuffle=False):
        log = trainer.valid_step(sample)
        for k, v in (log or {}).items():
            totals[k] = totals.get(k, 0.0) + torch.as_tensor(v, dtype=torch.float64, device=trainer.device)
    # every rank takes part in the SAME collectives with the SAME vector layout, whatever its shard held: a rank whose shard had
    # no batch (fewer validation batches than ranks) contributes zeros instead of returning before the all-reduce
    keys = sorted(totals)
    if world > 1:
        gathered = [None] * world
        torch.distributed.all_gather_object(gathered, keys)
        keys = sorted(set(k for ks in gathered for k in ks))
    if not keys:
        return {}
    zero = torch.zeros((), dtype=torch.float64, device=trainer.device)
    vec = torch.stack([totals.get(k, zero) for k in keys])
    if world > 1:
        torch.distributed.all_reduce(vec)
    out = dict(zip(keys, vec.tolist()))
    ss = max(out.get("sample_size", 1.0), 1.0)
    res = {k: (v / ss / math.log(2) if k.endswith("loss") else v) for k, v in out.items()}  # per-token, base 2 (criterions reduce_metrics)
    derived = getattr(trainer.criterion, "derived_metrics", None)  # criterion `ctc`: uer / wer / raw_wer from the summed error counts
    if derived is not None:
        res.update(derived(out))
    derived = getattr(task, "derived_metrics", None)  # task `translation` with --eval-bleu: bleu from the summed n-gram statistics
    if derived is not None:
        res.update(derived(out))
    return res


def train_main(argv=None):
    # Self-launch (below) is the SCRIPT entry's behaviour (fairseq_train.py's __main__ calls train_main() with no argument list); a
    # programmatic caller that passes argv wants the Trainer back from THIS process and gets ranks only by asking for them
    # (--distributed-world-size N > 1).
    from_script = argv is None
    argv = list(sys.argv[1:] if argv is None else argv)
    extra, rest = _extra_train_flags(argv)
    args = registry.parse_args_and_arch(rest)
    for k, v in vars(extra).items():
        setattr(args, k, v)
    if args.fp16 or getattr(args, "memory_efficient_fp16", False):
        args.fp16, args.memory_efficient_fp16, args.bf16 = False, False, True
    # Started plainly on a multi-GPU node, fairseq-train spawns one process per GPU itself (fairseq/distributed_utils.py:286-303,
    # nprocs = min(device_count, distributed_world_size); the flag's default is the device count, options.py:310).  Same here: this
    # process has not touched the GPU yet (device_count() does not initialise it) and becomes the launcher of the rank processes.
    if "WORLD_SIZE" not in os.environ and "RANK" not in os.environ:
        ndev = torch.cuda.device_count()
        want = args.distributed_world_size if args.distributed_world_size is not None else (max(ndev, 1) if from_script else 1)
        nproc = want if os.environ.get("CST_DIST_BACKEND") else min(max(ndev, 1), want)  # (gloo: ranks may share a GPU — tests)
        if needs_self_launch(nproc):
            entry = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fairseq_train.py")
            code = launch_ranks(nproc, [sys.executable, entry] + argv)
            if code != 0:
                raise SystemExit(code)
            return None
    rank, world = distributed_init()
    limit_host_threads(int(os.environ.get("LOCAL_WORLD_SIZE", world)))
    device = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(args.seed)
    import numpy as np
    np.random.seed(args.seed)  # (fairseq_cli/train.py:52: the draws made before the first update — the first batch's crops — follow --seed)
    task = registry.setup_task(args)
    train_ds = task.load_dataset(args.train_subset)
    model = task.build_model(args)
    criterion = task.build_criterion(args)
    trainer = Trainer(args, task, model, criterion, device=device)
    _log(rank, event="start", arch=args.arch, task=args.task, criterion=args.criterion, world_size=world,
         params=sum(p.numel() for p in model.parameters()), train_examples=len(train_ds), dtype=str(trainer.dtype))
    os.makedirs(args.save_dir, exist_ok=True)
    start_epoch, skip = 1, 0
    restore = args.restore_file if os.path.isabs(args.restore_file) else os.path.join(args.save_dir, args.restore_file)
    extra_state = trainer.load_checkpoint(restore, reset_optimizer=args.reset_optimizer)
    if extra_state is not None:
        if not args.reset_dataloader and extra_state.get("train_iterator"):
            start_epoch, skip = extra_state["train_iterator"]["epoch"], extra_state["train_iterator"]["iterations_in_epoch"]
        _log(rank, event="loaded_checkpoint", path=restore, num_updates=trainer.num_updates, epoch=start_epoch, iterations_in_epoch=skip)
    itr = task.get_batch_iterator(train_ds, max_tokens=args.max_tokens, max_sentences=args.batch_size, max_positions=task.max_positions(),
                                  ignore_invalid_inputs=True, required_batch_size_multiple=8 if args.batch_size is None else 1,
                                  seed=args.seed, num_shards=world, shard_id=rank, epoch=start_epoch)
    itr.pin_memory = True
    best = extra_state.get("best") if extra_state is not None else None  # checkpoint_utils.py:47-55: save_checkpoint.best survives a restart
    max_update = args.max_update or math.inf
    max_epoch = args.max_epoch or math.inf
    epoch = start_epoch

    def save(tag_files, epoch_, it_in_epoch, val):
        # `args.no_save` is the same on every rank, so this return is rank-agreed.  With --zero-sharding os the optimizer's moments
        # live in every rank's shards and Trainer.save_checkpoint assembles them with an all-gather: EVERY rank must enter it (only
        # rank 0 writes, trainer.py save_checkpoint); the file copies stay rank 0's.
        if args.no_save or (rank != 0 and not trainer.zero):
            return
        extra_ = {"train_iterator": {"epoch": epoch_, "iterations_in_epoch": it_in_epoch}, "val_loss": val, "best": best}
        first = os.path.join(args.save_dir, tag_files[0])
        trainer.save_checkpoint(first, extra_)
        if rank != 0:
            return
        for f in tag_files[1:]:
            import shutil
            shutil.copyfile(first, os.path.join(args.save_dir, f))

    while epoch <= max_epoch and trainer.num_updates < max_update:
        uf = args.update_freq[min(epoch - 1, len(args.update_freq) - 1)]
        t0, group, n_it, agg = time.time(), [], 0, {}
        for i, sample in enumerate(itr.next_epoch_itr(shuffle=True, buffer_size=max(getattr(args, "data_buffer_size", 8), 0))):
            if epoch == start_epoch and i < skip:
                continue
            group.append(sample)
            n_it = i + 1
            if len(group) < uf:
                continue
            out = trainer.train_step(group)
            group = []
            if out is None:  # a rank ran out of memory: every rank dropped this update (trainer.py:564-570)
                _log(rank, event="oom_skipped_update", epoch=epoch, num_updates=trainer.num_updates)
                continue
            if out.get("overflow"):  # NaN / Inf gradients: every rank dropped this update (trainer.py:629-646)
                _log(rank, event="nonfinite_gradient_skipped_update", epoch=epoch, num_updates=trainer.num_updates)
                continue
            for k, v in out.items():
                agg[k] = agg.get(k, 0.0) + (v if k not in ("lr", "gnorm") else 0.0)
            if trainer.num_updates % max(args.log_interval, 1) == 0:
                ss = max(out.get("sample_size", 1.0), 1.0)
                _log(rank, event="train_inner", epoch=epoch, num_updates=trainer.num_updates, loss=out["loss"] / ss / math.log(2),
                     gnorm=out["gnorm"], lr=out["lr"], ntokens=out.get("ntokens"))
            if args.save_interval_updates > 0 and trainer.num_updates % args.save_interval_updates == 0:
                save(["checkpoint_%d_%d.pt" % (epoch, trainer.num_updates), "checkpoint_last.pt"], epoch, n_it, None)
            if trainer.num_updates >= max_update:
                break
        if group and trainer.num_updates < max_update:  # the epoch's tail group is a (smaller) update of its own (iterators.py GroupedIterator)
            out = trainer.train_step(group)
            if out is not None and out.get("overflow"):
                out = None
            for k, v in (out or {}).items():
                agg[k] = agg.get(k, 0.0) + (v if k not in ("lr", "gnorm") else 0.0)
        ss = max(agg.get("sample_size", 1.0), 1.0)
        derived = trainer.criterion.derived_metrics(agg) if getattr(trainer.criterion, "derives_from_train_log", False) else {}  # (cross_entropy: ppl)
        _log(rank, event="train", epoch=epoch, num_updates=trainer.num_updates, loss=agg.get("loss", 0.0) / ss / math.log(2),
             wall=time.time() - t0, nsentences=agg.get("nsentences"), **derived)
        val = None
        if not args.disable_validation and epoch % args.validate_interval == 0:
            stats = validate(trainer, task, args, args.valid_subset.split(",")[0], rank, world)
            val = stats.get(args.best_checkpoint_metric, stats.get("loss"))
            # (keys with a leading underscore are summed statistics behind a derived metric, as in the reference's progress bar)
            _log(rank, event="valid", epoch=epoch, num_updates=trainer.num_updates, **{k: v for k, v in stats.items() if not k.startswith("_")})
        files = [] if args.no_epoch_checkpoints else ["checkpoint%d.pt" % epoch]
        better = val is not None and (best is None or (val > best if args.maximize_best_checkpoint_metric else val < best))
        if better:
            best = val
            files.append("checkpoint_best.pt")
        files.append("checkpoint_last.pt")
        save(files, epoch + 1, 0, val)
        epoch += 1
        skip = 0
    _log(rank, event="done", num_updates=trainer.num_updates, best=best)
    if world > 1:
        torch.distributed.destroy_process_group()
    return trainer


# --------------------------------------------------------------------------------------------------------------------
def corpus_bleu(hyps, refs, max_n=4):
    """Corpus BLEU-4 with brevity penalty over whitespace tokens (the reference scores with sacrebleu's 13a tokeniser,
    fairseq_cli/generate.py:352-376 — sacrebleu is not in this image; numbers are comparable between runs of THIS tool only)."""
    from collections import Counter
    match, total, hl, rl = [0] * max_n, [0] * max_n, 0, 0
    for h, r in zip(hyps, refs):
        h, r = h.split(), r.split()
        hl, rl = hl + len(h), rl + len(r)
        for n in range(1, max_n + 1):
            hc = Counter(tuple(h[i:i + n]) for i in range(len(h) - n + 1))
            rc = Counter(tuple(r[i:i + n]) for i in range(len(r) - n + 1))
            match[n - 1] += sum(min(c, rc[g]) for g, c in hc.items())
            total[n - 1] += max(len(h) - n + 1, 0)
    if min(total) == 0 or min(match) == 0:
        return 0.0
    logp = sum(math.log(m / t) for m, t in zip(match, total)) / max_n
    bp = 1.0 if hl > rl else math.exp(1 - rl / max(hl, 1))
    return 100.0 * bp * math.exp(logp)


def generate_parser():
    """The options of fairseq_generate.py (a subset of fairseq-generate's, same names and defaults)."""
    p = argparse.ArgumentParser(allow_abbrev=False)
    p.add_argument("data")
    p.add_argument("--path", required=True, help="checkpoint(s), colon separated: several files are decoded as an ensemble "
                   "(the members' next-token distributions are averaged at every step)")
    p.add_argument("--task", default="triplet")
    p.add_argument("--config-yaml", default="config.yaml")
    p.add_argument("--gen-subset", default="test")
    p.add_argument("--max-tokens", type=int, default=None)
    p.add_argument("--max-sentences", "--batch-size", type=int, default=None, dest="batch_size")
    p.add_argument("--max-source-positions", type=int, default=2000000)
    p.add_argument("--max-target-positions", type=int, default=1024)
    p.add_argument("--beam", type=int, default=5)
    p.add_argument("--max-len-a", type=float, default=0)
    p.add_argument("--max-len-b", type=int, default=200)
    p.add_argument("--min-len", type=int, default=1)
    p.add_argument("--lenpen", type=float, default=1.0)
    p.add_argument("--unkpen", type=float, default=0.0)
    p.add_argument("--temperature", type=float, default=1.0)
    p.add_argument("--unnormalized", action="store_true")
    p.add_argument("--no-repeat-ngram-size", type=int, default=0, help="no n-gram of this size may occur twice in a hypothesis (0 = off)")
    p.add_argument("--prefix-size", type=int, default=0, help="force the first K target tokens of every sentence to the reference's")
    p.add_argument("--sampling", action="store_true", help="draw every token from the model's distribution instead of beam search: each of "
                   "the --beam hypotheses of a sentence is an independent sample (--seed selects the stream of draws)")
    p.add_argument("--sampling-topk", type=int, default=-1, help="draw among the k most probable tokens only (requires --sampling)")
    p.add_argument("--sampling-topp", type=float, default=-1.0, help="draw from the smallest set of tokens with probability mass p "
                   "(nucleus sampling; requires --sampling, wins over --sampling-topk)")
    p.add_argument("--diverse-beam-groups", type=int, default=-1, help="diverse beam search: the --beam hypotheses are dealt to this many "
                   "groups, and a group is penalised for tokens the groups before it chose at the same step (--beam must be divisible)")
    p.add_argument("--diverse-beam-strength", type=float, default=0.5, help="the penalty per earlier choice of a token (diverse beam search)")
    p.add_argument("--diversity-rate", type=float, default=-1.0, help="diverse siblings search: the p-th best continuation of a hypothesis "
                   "loses p times this rate (0 equals beam search; negative = off)")
    p.add_argument("--constraints", nargs="?", const="ordered", default=None, choices=["ordered", "unordered"],
                   help="lexically constrained decoding: the phrases of --constraints-file must appear in the translation, in the given "
                   "order (ordered, the default) or in any order")
    p.add_argument("--constraints-file", default=None, help="one line per utterance: id<TAB>phrase<TAB>phrase... (the id of the manifest; "
                   "phrases are tokenised like target text; utterances without a line are unconstrained)")
    p.add_argument("--score-reference", action="store_true", help="just score the reference translation")
    p.add_argument("--lm-path", default=None, help="a transformer_lm checkpoint over the TARGET dictionary: its next-token log-probabilities "
                   "are added to the model's at every step (shallow fusion)")
    p.add_argument("--lm-weight", type=float, default=0.0, help="the weight of the language model's log-probabilities (requires --lm-path)")
    p.add_argument("--nbest", type=int, default=1, help="hypotheses printed per sentence (at most --beam)")
    p.add_argument("--print-alignment", action="store_true", help="after every hypothesis an A- line: per target token the source position "
                   "(encoder frame; memory slot for Chimera models) its last-layer cross attention, averaged over the heads, is largest at")
    p.add_argument("--remove-bpe", "--post-process", nargs="?", const="@@ ", default=None, dest="post_process")
    p.add_argument("--scoring", default="bleu")
    p.add_argument("--results-path", default=None)
    p.add_argument("--fp16", action="store_true")
    p.add_argument("--bf16", action="store_true")
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--quiet", action="store_true")
    return p


def check_generate_args(args):
    """The combinations fairseq-generate refuses (fairseq_cli/generate.py:49-54, fairseq_task.py:343-344), before anything is loaded."""
    if args.nbest < 1 or args.nbest > args.beam:
        raise ValueError("--nbest %d must be between 1 and --beam %d" % (args.nbest, args.beam))
    if args.sampling_topk >= 0 and not args.sampling:
        raise ValueError("--sampling-topk requires --sampling")
    if args.sampling_topp >= 0 and not args.sampling:
        raise ValueError("--sampling-topp requires --sampling")
    if sum(int(bool(c)) for c in (args.sampling, args.diverse_beam_groups > 0, args.diversity_rate > 0)) > 1:
        raise ValueError("Provided Search parameters are mutually exclusive.")
    if args.diverse_beam_groups > 0 and args.beam % args.diverse_beam_groups != 0:
        raise ValueError("DiverseBeamSearch requires --beam to be divisible by the number of groups")
    if (args.constraints is None) != (args.constraints_file is None):
        raise ValueError("--constraints and --constraints-file go together")
    if args.constraints is not None:
        if args.sampling or args.diverse_beam_groups > 0 or args.diversity_rate > -1:
            raise ValueError("Provided Search parameters are mutually exclusive: --constraints with sampling or a diverse strategy.")
        if args.prefix_size > 0:
            raise ValueError("--constraints cannot be combined with --prefix-size")
        if args.score_reference:
            raise ValueError("--constraints cannot be combined with --score-reference: nothing is searched")
    if args.lm_weight != 0.0 and args.lm_path is None:
        raise ValueError("--lm-weight requires --lm-path")
    if args.print_alignment and args.score_reference:
        raise ValueError("--print-alignment cannot be combined with --score-reference: the scorer returns no attention")
    if args.lm_path is not None and args.score_reference:
        raise ValueError("--lm-path cannot be combined with --score-reference: the scorer has no language model")
    return args


def hard_alignment(attention, tokens, pad, eos):
    """The (source, target) pairs of the A- line of --print-alignment (fairseq_cli/generate.py:296-305 over utils.extract_hard_alignment
    with the generator's attention): attention [src_len, tgt_len] as a hypothesis carries it, tokens its tgt_len token ids.  Per target
    position that is neither pad nor eos — the final eos is dropped — the source position with the largest weight, ties to the smallest
    index; both 0-based.  Padded source positions have weight exactly 0 and so never win."""
    attention = torch.as_tensor(attention).float().cpu()
    tokens = torch.as_tensor(tokens).long().cpu()
    if attention.dim() != 2 or attention.size(1) != tokens.numel():
        raise ValueError("attention %s does not match %d tokens" % (tuple(attention.shape), tokens.numel()))
    best = attention.max(dim=0, keepdim=True).values
    src = torch.where(attention == best, torch.arange(attention.size(0)).unsqueeze(1), torch.full((1, 1), attention.size(0))).amin(dim=0)
    return [(int(src[t]), t) for t in range(tokens.numel()) if int(tokens[t]) not in (pad, eos)]


def read_constraints_file(path):
    """{utterance id: [phrase, ...]} of a constraints file: one line per utterance, id<TAB>phrase<TAB>phrase... (the tab-separated
    phrases fairseq-interactive takes after the source, keyed by the manifest's id).  An id with no phrase has no constraints."""
    table = {}
    with open(path, encoding="utf-8") as f:
        for n, line in enumerate(f, 1):
            line = line.rstrip("\n")
            if not line.strip():
                continue
            uid, *phrases = line.split("\t")
            if uid in table:
                raise ValueError("%s:%d: utterance id %r occurs twice" % (path, n, uid))
            if any(not ph.strip() for ph in phrases):
                raise ValueError("%s:%d: an empty phrase" % (path, n))
            table[uid] = [ph.strip() for ph in phrases]
    return table


def encode_constraints(dataset, table, tgt_dict):
    """Per item of `dataset` (one manifest) its constraints as lists of token ids: every phrase is encoded exactly like target text
    (tokenize_text(..., "target"), then encode_line without new symbols and without eos).  Ids of the file the manifest does not have
    are an error."""
    manifests = getattr(dataset, "datasets", [dataset])
    if len(manifests) != 1:
        raise ValueError("--constraints-file names utterances by the id of ONE manifest; the subset has %d" % len(manifests))
    ds = manifests[0]
    if getattr(ds, "ids", None) is None:
        raise ValueError("--constraints-file needs the manifest's id column")
    unknown = sorted(set(table) - set(ds.ids))
    if unknown:
        raise ValueError("--constraints-file: ids that are not in the manifest: %s" % ", ".join(map(repr, unknown[:8])))
    out = []
    for uid in ds.ids:
        out.append([tgt_dict.encode_line(ds.tokenize_text(ph, "target"), add_if_not_exist=False, append_eos=False).long().tolist()
                    for ph in table.get(uid, [])])
    return out


def generate_main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    args, ignored = generate_parser().parse_known_args(argv)
    check_generate_args(args)
    limit_host_threads()
    overrides = {"data": args.data, "config_yaml": args.config_yaml, "max_source_positions": args.max_source_positions,
                 "max_target_positions": args.max_target_positions}
    models, margs, task = checkpoint_utils.load_model_ensemble_and_task(args.path.split(":"), arg_overrides=overrides)
    if getattr(margs, "task", None) == "language_modeling":
        raise NotImplementedError("generation from a language model (fairseq-generate --task language_modeling) is not built: score it with "
                                  "fairseq_eval_lm.py, or fuse it into a translation model's decode with --lm-path")
    dtype = torch.bfloat16 if (args.fp16 or args.bf16) else torch.float32
    models = [m.to("cuda", dtype).eval() for m in models]
    ds = task.load_dataset(args.gen_subset)
    itr = task.get_batch_iterator(ds, max_tokens=args.max_tokens, max_sentences=args.batch_size,
                                  max_positions=(args.max_source_positions, args.max_target_positions), ignore_invalid_inputs=True)
    if args.score_reference and any(getattr(d, "tgt_texts", getattr(d, "tgt", None)) is None for d in getattr(ds, "datasets", [ds])):  # before any batch is decoded
        raise ValueError("--score-reference needs the references of subset %s: it has no target text" % args.gen_subset)
    lm = None
    if args.lm_path is not None:  # fairseq_cli/generate.py:112-128: one LM over the target dictionary
        lm = checkpoint_utils.load_language_model(args.lm_path, task.target_dictionary).to("cuda", dtype).eval()
    gen = task.build_generator(models, args, extra_gen_cls_kwargs={"lm_model": lm, "lm_weight": args.lm_weight})
    tgt_dict, src_dict = task.target_dictionary, task.source_dictionary
    lexical = None
    if args.constraints is not None:
        from .lexical_constraints import pack_constraints
        lexical = encode_constraints(ds, read_constraints_file(args.constraints_file), tgt_dict)
    if args.results_path:
        os.makedirs(args.results_path, exist_ok=True)
    out = open(os.path.join(args.results_path, "generate-%s.txt" % args.gen_subset), "w") if args.results_path else sys.stdout

    def detok(s):
        if args.post_process == "sentencepiece":
            return s.replace(" ", "").replace("▁", " ").strip()
        if args.post_process:
            return (s + " ").replace(args.post_process, "").rstrip()
        return s

    hyps, refs, nsent, ntok, t0 = [], [], 0, 0, time.time()
    for sample in itr.next_epoch_itr(shuffle=False):
        if not sample:
            continue
        ni = sample["net_input"]
        if "pair_idx" in ni:  # translation task, device-resident corpus (language_pair_dataset.py): the batch from its indices
            dev = ni["pair_corpus"].materialize(sample)
            ni, sample = dev["net_input"], dict(sample, target=dev["target"].cpu(), net_input=dev["net_input"])
        if "src_audio" in ni:  # fbank route (data.py): filter banks of the audio batch, computed on the device
            ni = fbank.materialize({k: (v.cuda() if torch.is_tensor(v) else v) for k, v in ni.items()},
                                   max_frames=int(ni["src_lengths"].max()))
        src = ni["src_tokens"]
        # raw waveforms [B, S] stay fp32 as in training (Trainer._prepare_sample: conv0 reads fp32 samples); only feature
        # inputs [B, T, F] take the model's storage dtype
        src = src.to("cuda", dtype) if (src.dim() == 3 and src.is_floating_point()) else src.cuda()
        s = {"net_input": {"src_tokens": src, "src_lengths": ni["src_lengths"].cuda()}}
        prefix = None
        if args.prefix_size > 0:  # fairseq_cli/generate.py:189-191
            if sample.get("target") is None:
                raise ValueError("--prefix-size needs the references of the subset (no target in this batch)")
            prefix = sample["target"][:, :args.prefix_size].cuda()
        if args.score_reference:  # fairseq_cli/generate.py hands the scorer the collater's whole sample
            if sample.get("target") is None:
                raise ValueError("--score-reference needs the references of the subset (no target in this batch)")
            s["net_input"]["prev_output_tokens"] = sample["net_input"]["prev_output_tokens"].cuda()
            s["target"] = sample["target"].cuda()
        packed = None
        if lexical is not None:  # interactive.py:188-197: the batch's constraints, packed
            packed = pack_constraints([lexical[i] for i in sample["id"].tolist()], pad=tgt_dict.pad(), eos=tgt_dict.eos())
        results = task.inference_step(gen, models, s, prefix_tokens=prefix, constraints=packed)
        src_text = None
        if not args.quiet and src_dict is not None and not src.is_floating_point():  # text input: the S- lines of fairseq-generate
            src_text = [src_dict.string(row) for row in src.tolist()]
        for i, sid in enumerate(sample["id"].tolist()):
            ref = tgt_dict.string(sample["target"][i]) if sample.get("target") is not None else None
            if src_text is not None:
                print("S-%d\t%s" % (sid, src_text[i]), file=out)
            if not args.quiet and ref is not None:
                print("T-%d\t%s" % (sid, ref), file=out)
            if not args.quiet and lexical is not None:  # interactive.py:257-260
                for c in lexical[sid]:
                    print("C-%d\t%s" % (sid, tgt_dict.string(torch.tensor(c))), file=out)
            for j, hj in enumerate(results[i][:args.nbest]):  # fairseq_cli/generate.py: hypos[i][:args.nbest]
                hyp_j = tgt_dict.string(hj["tokens"].cpu())
                if not args.quiet:
                    print("H-%d\t%.6f\t%s" % (sid, float(hj["score"]) / math.log(2), hyp_j), file=out)
                    print("D-%d\t%.6f\t%s" % (sid, float(hj["score"]) / math.log(2), detok(hyp_j)), file=out)
                    print("P-%d\t%s" % (sid, " ".join("%.4f" % (x / math.log(2)) for x in hj["positional_scores"].tolist())), file=out)
                    if args.print_alignment:
                        pairs = hard_alignment(hj["attention"], hj["tokens"], tgt_dict.pad(), tgt_dict.eos())
                        print("A-%d\t%s" % (sid, " ".join("%d-%d" % st for st in pairs)), file=out)
                if j == 0:  # BLEU and the token count come from the best hypothesis
                    h, hyp = hj, hyp_j
            hyps.append(detok(hyp))
            refs.append(detok(ref) if ref is not None else "")
            ntok += len(h["tokens"])
        nsent += len(results)
    torch.cuda.synchronize()
    dt = time.time() - t0
    summary = {"event": "generate", "subset": args.gen_subset, "sentences": nsent, "tokens": ntok, "seconds": dt,
               "sentences_per_s": nsent / max(dt, 1e-9), "tokens_per_s": ntok / max(dt, 1e-9), "beam": args.beam, "models": len(models),
               "sampling": bool(args.sampling), "nbest": args.nbest, "seed": args.seed,
               "diverse_beam_groups": args.diverse_beam_groups, "diverse_beam_strength": args.diverse_beam_strength,
               "diversity_rate": args.diversity_rate, "score_reference": bool(args.score_reference),
               "lm_path": args.lm_path, "lm_weight": args.lm_weight, "constraints": args.constraints,
               "print_alignment": bool(args.print_alignment),
               "bleu4_whitespace": corpus_bleu(hyps, refs) if any(refs) else None, "ignored_flags": ignored}
    print(json.dumps(summary), file=out, flush=True)
    if out is not sys.stdout:
        out.close()
        print(json.dumps(summary))
    return summary


# --------------------------------------------------------------------------------------------------------------------
def eval_lm_parser():
    """The options of fairseq_eval_lm.py (a subset of fairseq-eval-lm's, same names and defaults)."""
    p = argparse.ArgumentParser(allow_abbrev=False)
    p.add_argument("data")
    p.add_argument("--path", required=True, help="the language model's checkpoint")
    p.add_argument("--task", default="language_modeling")
    p.add_argument("--gen-subset", default="test")
    p.add_argument("--max-tokens", type=int, default=None)
    p.add_argument("--max-sentences", "--batch-size", type=int, default=None, dest="batch_size")
    p.add_argument("--tokens-per-sample", type=int, default=None, help="(default: the checkpoint's)")
    p.add_argument("--sample-break-mode", default=None, choices=["none", "complete", "complete_doc", "eos"], help="(default: the checkpoint's)")
    p.add_argument("--remove-bpe", "--post-process", nargs="?", const="@@ ", default=None, dest="post_process")
    p.add_argument("--output-word-probs", action="store_true", help="if set, outputs words and their predicted log probabilities")
    p.add_argument("--output-word-stats", action="store_true", help="if set, outputs word statistics such as word count, average probability, etc")
    p.add_argument("--context-window", type=int, default=0, help="(values above 0 are not built)")
    p.add_argument("--softmax-batch", type=int, default=sys.maxsize, help="accepted, without effect: no fp32 [B, T, V] tensor is materialised")
    p.add_argument("--fp16", action="store_true")
    p.add_argument("--bf16", action="store_true")
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--quiet", action="store_true")
    return p


def check_eval_lm_args(args):
    if args.context_window > 0:
        raise NotImplementedError("--context-window %d is not built: every block is scored from its own first token" % args.context_window)
    if args.post_process == "sentencepiece":  # (fairseq_cli/eval_lm.py:163-164 refuses it too)
        raise NotImplementedError("--post-process sentencepiece (--remove-bpe sentencepiece) is not built: the reference's eval-lm "
                                  "raises on it as well; pass the continuation marker itself, e.g. --remove-bpe '@@ '")
    return args


def bpe_continuation_tokens(dictionary, post_process):
    """(ids of the symbols that end in the continuation marker, the marker's length) — fairseq_cli/eval_lm.py:162-175."""
    if post_process is None:
        return None, 0
    bpe_cont = post_process.rstrip()
    return {i for i in range(len(dictionary)) if dictionary[i].endswith(bpe_cont)}, len(bpe_cont)


def lm_score_stats(tokens, pos_scores, bpe_toks=None):
    """One sample's share of eval-lm's totals (fairseq_cli/eval_lm.py:195-220): a BPE continuation token's score moves onto the next
    token and is not counted; +-inf scores are dropped.  tokens: the ids [n]; pos_scores: float [n] natural-log scores.
    -> (score sum, count, the merged scores [n] before the infinite ones are dropped, the number of infinite scores)."""
    tokens = [int(t) for t in (tokens.tolist() if torch.is_tensor(tokens) else tokens)]
    pos = torch.as_tensor(pos_scores).detach().float().cpu().clone()
    skipped = 0
    if bpe_toks is not None:
        for i in range(len(tokens) - 1):
            if tokens[i] in bpe_toks:
                skipped += 1
                pos[i + 1] += pos[i]
                pos[i] = 0
    inf = torch.isinf(pos)
    kept = pos[~inf]
    return float(kept.sum()), int(kept.numel()) - skipped, pos, int(inf.sum())


class WordStat:
    """fairseq_cli/eval_lm.py:37-66."""

    def __init__(self, word, is_bpe):
        self.word, self.is_bpe = word, is_bpe
        self.log_prob, self.next_word_prob, self.count, self.missing_next_words = 0, 0, 0, 0

    def add(self, log_prob, next_word_prob):
        if next_word_prob is not None:
            self.next_word_prob += next_word_prob
        else:
            self.missing_next_words += 1
        self.log_prob += log_prob
        self.count += 1

    def __str__(self):
        return "{}\t{}\t{}\t{}\t{}\t{}".format(self.word, self.count, self.log_prob, self.is_bpe, self.next_word_prob,
                                               self.count - self.missing_next_words)


def eval_lm_main(argv=None):
    """fairseq_cli/eval_lm.py:69-276: the perplexity of a language model on a binarised split.  Every batch is scored by the
    SequenceScorer (cst_score_tokens: no fp32 [B, T, V] tensor, one transfer of the scores per batch)."""
    from .sequence_scorer import SequenceScorer
    argv = list(sys.argv[1:] if argv is None else argv)
    args, ignored = eval_lm_parser().parse_known_args(argv)
    check_eval_lm_args(args)
    limit_host_threads()
    overrides = {"data": args.data}
    if args.tokens_per_sample is not None:
        overrides["tokens_per_sample"] = args.tokens_per_sample
    if args.sample_break_mode is not None:
        overrides["sample_break_mode"] = args.sample_break_mode
    models, margs, task = checkpoint_utils.load_model_ensemble_and_task([args.path], arg_overrides=overrides)
    if not hasattr(task, "dictionary") or getattr(margs, "task", None) != "language_modeling":
        raise ValueError("%s was trained by task %r: eval-lm scores a language_modeling checkpoint" % (args.path, getattr(margs, "task", None)))
    dtype = torch.bfloat16 if (args.fp16 or args.bf16) else torch.float32
    models = [m.to("cuda", dtype).eval() for m in models]
    ds = task.load_dataset(args.gen_subset)
    limits = [task.max_positions()] + [m.max_positions() for m in models]
    itr = task.get_batch_iterator(ds, max_tokens=args.max_tokens or 36000, max_sentences=args.batch_size,
                                  max_positions=min(int(v) for v in limits if v is not None), ignore_invalid_inputs=True, seed=args.seed)
    d = task.target_dictionary
    scorer = SequenceScorer(d)
    bpe_toks, bpe_len = bpe_continuation_tokens(task.source_dictionary, args.post_process)
    score_sum, count, ntokens, word_stats, t0 = 0.0, 0, 0, {}, time.time()
    for sample in itr.next_epoch_itr(shuffle=False):
        if not sample or "net_input" not in sample:
            continue
        ni = sample["net_input"]
        if "block_idx" in ni:  # device-resident corpus (monolingual_dataset.py): the batch from its block indices, one launch
            dev = ni["block_corpus"].materialize(sample)
        else:
            dev = {"net_input": {k: v.cuda() for k, v in ni.items()}, "target": sample["target"].cuda()}
        hypos = scorer.generate(models, {"net_input": dev["net_input"], "target": dev["target"]})
        ntokens += sample["ntokens"]
        for i, sid in enumerate(sample["id"].tolist()):
            hypo = hypos[i][0]
            tokens = hypo["tokens"].tolist()
            s, c, pos, n_inf = lm_score_stats(tokens, hypo["positional_scores"], bpe_toks)
            if n_inf:
                print("skipping tokens with inf scores: " + d.string(torch.tensor([t for t, x in zip(tokens, pos.tolist()) if math.isinf(x)])))
            score_sum += s
            count += c
            if args.output_word_probs or args.output_word_stats:  # :222-257
                w, word_prob, is_bpe = "", [], False
                for k, w_ind in enumerate(tokens):
                    w += task.source_dictionary[w_ind]
                    if bpe_toks is not None and w_ind in bpe_toks:
                        w, is_bpe = w[:-bpe_len], True
                        continue
                    word_prob.append((w, float(pos[k])))
                    next_prob = next((float(pos[j]) for j in range(k + 1, len(tokens)) if float(pos[j]) != 0), None)
                    word_stats.setdefault(w, WordStat(w, is_bpe)).add(float(pos[k]), next_prob)
                    w, is_bpe = "", False
                if args.output_word_probs:
                    print(str(int(sid)) + " " + "\t".join("{} [{:2f}]".format(x[0], x[1]) for x in word_prob))
    torch.cuda.synchronize()
    dt = time.time() - t0
    if count <= 0:
        raise ValueError("subset %s of %s holds no token to score" % (args.gen_subset, args.data))
    loss = -score_sum / count / math.log(2)  # base 2
    print("Evaluated {} tokens in {:.1f}s ({:.2f} tokens/s)".format(ntokens, dt, ntokens / max(dt, 1e-9)))
    print("Loss (base 2): {:.4f}, Perplexity: {:.2f}".format(loss, 2 ** loss))
    if args.output_word_stats:
        for ws in sorted(word_stats.values(), key=lambda x: x.count, reverse=True):
            print(ws)
    summary = {"event": "eval_lm", "subset": args.gen_subset, "tokens": ntokens, "count": count, "score_sum": score_sum, "loss": loss,
               "ppl": 2 ** loss, "seconds": dt, "sample_break_mode": getattr(margs, "sample_break_mode", None),
               "tokens_per_sample": getattr(margs, "tokens_per_sample", None), "ignored_flags": ignored}
    print(json.dumps(summary), flush=True)
    return summary


# --------------------------------------------------------------------------------------------------------------------
def buffered_read(input, buffer_size):
    """fairseq_cli/interactive.py:42-52: the stripped lines of `input` ("-": stdin) in lists of buffer_size; the last may be shorter."""
    buffer = []
    h = sys.stdin if input == "-" else open(input, encoding="utf-8")
    try:
        for src_str in h:
            buffer.append(src_str.strip())
            if len(buffer) >= buffer_size:
                yield buffer
                buffer = []
    finally:
        if h is not sys.stdin:
            h.close()
    if len(buffer) > 0:
        yield buffer


def interactive_parser():
    """The options of fairseq_interactive.py: the decoding flags of generate_parser() under the same names and defaults, and
    fairseq-interactive's own.  --max-source-positions / --max-target-positions default to the checkpoint's here: the limits of a
    language model are its training run's."""
    p = generate_parser()
    p.set_defaults(max_source_positions=None, max_target_positions=None)
    p.add_argument("--buffer-size", type=int, default=0, help="read this many sentences before processing them")
    p.add_argument("--input", default="-", help="file to read from; use - for stdin")
    p.add_argument("--bpe", default=None, help="the BPE of a text task's lines (sentencepiece); the speech tasks take theirs from the config YAML")
    p.add_argument("--sentencepiece-model", default=None, help="path to the sentencepiece model (--bpe sentencepiece)")
    p.add_argument("--tokenizer", default=None, help="the pre-tokenizer of a text task's lines")
    p.add_argument("--skip-invalid-size-inputs-valid-test", action="store_true", help="ignore lines beyond the model's positions")
    return p


def check_interactive_args(args):
    """fairseq_cli/interactive.py:117-128 and what this driver refuses by name — before any checkpoint is read."""
    if args.buffer_size < 1:
        args.buffer_size = 1
    if args.max_tokens is None and args.batch_size is None:
        args.batch_size = 1
    assert not args.sampling or args.nbest == args.beam, "--sampling requires --nbest to be equal to --beam"
    assert not args.batch_size or args.batch_size <= args.buffer_size, "--batch-size cannot be larger than --buffer-size"
    if args.score_reference:
        raise NotImplementedError("--score-reference is not built for typed input: a typed line has no reference (fairseq_generate.py scores a subset's)")
    if args.prefix_size > 0:
        raise NotImplementedError("--prefix-size %d is not built for typed input: a typed line has no reference to take a prefix from" % args.prefix_size)
    if args.constraints_file is not None:
        raise ValueError("--constraints-file belongs to fairseq_generate.py: here the phrases follow the source on its line, after a tab")
    from . import data as D
    D.build_tokenizer({"tokenizer": args.tokenizer})  # (refuses by name what is not built)
    if args.bpe not in (None, "none", "sentencepiece"):
        D.build_bpe({"bpe": args.bpe})
    if args.bpe == "sentencepiece" and not args.sentencepiece_model:
        raise ValueError("--bpe sentencepiece needs --sentencepiece-model")
    generic = argparse.Namespace(**vars(args))
    generic.constraints_file = "-" if args.constraints is not None else None  # (the pairing rule of fairseq_generate.py does not apply)
    check_generate_args(generic)
    return args


def resolve_max_positions(*limits):
    """utils.resolve_max_positions for ints and (source, target) pairs: the element-wise minimum, None = no limit."""
    out = None
    for v in limits:
        if v is None:
            continue
        if out is None:
            out = v
        elif isinstance(v, (int, float)) and isinstance(out, (int, float)):
            out = min(out, v)
        else:
            a = out if isinstance(out, (tuple, list)) else (out, out)
            b = v if isinstance(v, (tuple, list)) else (v, v)
            out = tuple(x if y is None else y if x is None else min(x, y) for x, y in zip(a, b))
    return out


def split_constraints(lines, tgt_dict, encode_fn):
    """fairseq_cli/interactive.py:59-76: (the sources, per line its constraints as lists of token ids) of lines
    `source<TAB>phrase<TAB>phrase...`; a phrase is encoded like target text, without new symbols and without eos."""
    sources, lists = [], []
    for line in lines:
        src, *phrases = line.split("\t") if "\t" in line else [line]
        sources.append(src)
        lists.append([tgt_dict.encode_line(encode_fn(ph), append_eos=False, add_if_not_exist=False).long().tolist() for ph in phrases])
    return sources, lists


def lm_prompt_limit(n, max_len_a, max_len_b, max_decoder_positions):
    """Whether a prompt of n tokens fits the generator's step limit in ANY batch: max_len of a batch is computed from its width, at least
    this prompt's own 1 + n (sequence_generator.py:228-232), and the forced prefix may be exactly max_len wide."""
    return n <= min(int(max_len_a * (n + 1) + max_len_b), max_decoder_positions - 1)


def make_batches(lines, args, task, max_positions, encode_fn, start_id=0, err=None, prompt_ok=None):
    """fairseq_cli/interactive.py:55-105 — yields (ids, the collated batch, its constraints as lists or None): the task's
    get_interactive_tokens_and_lengths, build_dataset_for_inference and get_batch_iterator(shuffle=False); ids are positions in `lines`.
    DIFFERENCES to the reference: a line the task cannot read (a missing, unreadable or non-PCM audio file) is named on `err` with its id
    and left out instead of ending the session; prompt_ok (language models): a predicate on a prompt's token count — a prompt that fails
    it is reported the same way, and EMPTY prompts (eos alone) are batched apart from the others: they decode without a prefix."""
    err = sys.stderr if err is None else err
    lists = None
    if args.constraints:
        lines, lists = split_constraints(lines, task.target_dictionary, encode_fn)
    groups = {}
    for pos, line in enumerate(lines):
        try:
            tokens, lengths = task.get_interactive_tokens_and_lengths([line], encode_fn)
        except (FileNotFoundError, ValueError, OSError) as e:
            print("input %d skipped: %s" % (start_id + pos, e), file=err, flush=True)
            continue
        key = 0
        beyond = isinstance(max_positions, (int, float)) and lengths[0] > max_positions  # (the iterator raises on it, or skips it)
        if prompt_ok is not None and not beyond:
            n = int(lengths[0]) - 1  # (without the eos encode_line appended)
            if not prompt_ok(n):
                print("input %d skipped: a prompt of %d tokens exceeds the step limit max_len (--max-len-a, --max-len-b, the model's "
                      "positions)" % (start_id + pos, n), file=err, flush=True)
                continue
            key = int(n == 0)
        g = groups.setdefault(key, ([], [], []))
        g[0].append(pos), g[1].append(tokens[0]), g[2].append(lengths[0])
    for key in sorted(groups):
        positions, tokens, lengths = groups[key]
        itr = task.get_batch_iterator(dataset=task.build_dataset_for_inference(tokens, lengths), max_tokens=args.max_tokens,
                                      max_sentences=args.batch_size, max_positions=max_positions,
                                      ignore_invalid_inputs=args.skip_invalid_size_inputs_valid_test).next_epoch_itr(shuffle=False)
        for batch in itr:
            if not batch:
                continue
            ids = [positions[i] for i in batch["id"].tolist()]
            yield ids, batch, (None if lists is None else [lists[i] for i in ids])


def print_translations(results, args, src_dict, tgt_dict, decode_fn, strip=(), out=None):
    """fairseq_cli/interactive.py:250-298, the lines of one buffer in input order.  results: (id, src_tokens or None, hypos, info) with
    info = {"constraints": lists of token ids, "time": seconds}; src_tokens None (a float source: audio) prints no S-/W-/C- line.  Scores
    are divided by ln 2 in fp32 on the host, as the reference's tensors are, and printed with `{}`; P- with %.4f."""
    out = sys.stdout if out is None else out
    ntok = 0
    for id_, src_tokens, hypos, info in sorted(results, key=lambda x: x[0]):
        if src_dict is not None and src_tokens is not None:
            print("S-{}\t{}".format(id_, src_dict.string(src_tokens, args.post_process)), file=out)
            print("W-{}\t{:.3f}\tseconds".format(id_, info["time"]), file=out)
            for constraint in info["constraints"]:
                print("C-{}\t{}".format(id_, tgt_dict.string(constraint, args.post_process)), file=out)
        for j, hypo in enumerate(hypos[:min(len(hypos), args.nbest)]):
            tokens = torch.as_tensor(hypo["tokens"]).int().cpu()
            hypo_str = tgt_dict.string(tokens, args.post_process, extra_symbols_to_ignore=strip)
            detok_hypo_str = decode_fn(hypo_str).replace("<unk>", " ")
            score = torch.as_tensor(hypo["score"]).detach().float().cpu() / math.log(2)  # convert to base 2
            print("H-{}\t{}\t{}".format(id_, score, hypo_str), file=out)
            print("D-{}\t{}\t{}".format(id_, score, detok_hypo_str), file=out)
            pos = torch.as_tensor(hypo["positional_scores"]).detach().float().cpu().div(math.log(2)).tolist()
            print("P-{}\t{}".format(id_, " ".join(map(lambda x: "{:.4f}".format(x), pos))), file=out)
            if args.print_alignment:
                pairs = hard_alignment(hypo["attention"], hypo["tokens"], tgt_dict.pad(), tgt_dict.eos())
                print("A-{}\t{}".format(id_, " ".join("{}-{}".format(s, t) for s, t in pairs)), file=out)
            if j == 0:
                ntok += len(tokens)
    out.flush()
    return ntok


def interactive_main(argv=None):
    """fairseq_cli/interactive.py:108-307: translate typed audio paths (tasks speech_to_text / triplet), sentences (translation) or
    language-model prompts (language_modeling), one buffer at a time.  Stdout carries the S-/W-/C-/H-/D-/P-/A- lines and nothing else;
    skipped lines and the closing JSON summary go to stderr."""
    argv = list(sys.argv[1:] if argv is None else argv)
    args, ignored = interactive_parser().parse_known_args(argv)
    check_interactive_args(args)
    limit_host_threads()
    start_time, total_translate_time = time.time(), 0.0
    overrides = {"data": args.data, "config_yaml": args.config_yaml}
    if args.max_source_positions is not None:
        overrides["max_source_positions"] = args.max_source_positions
    if args.max_target_positions is not None:
        overrides["max_target_positions"] = args.max_target_positions
    models, margs, task = checkpoint_utils.load_model_ensemble_and_task(args.path.split(":"), arg_overrides=overrides)
    kind = getattr(margs, "task", None)
    is_lm, is_speech = kind == "language_modeling", hasattr(task, "data_cfg")
    if args.constraints is not None and (is_lm or is_speech):
        raise NotImplementedError("--constraints is not built for task %s: a typed line is an audio path or a prompt, and the phrases "
                                  "of --constraints follow a source SENTENCE after a tab" % kind)
    if is_lm and args.print_alignment:
        raise ValueError("--print-alignment needs cross attention: the model of %s is a language model" % args.path)
    if is_lm and args.lm_path is not None:
        raise ValueError("--lm-path: the model of %s is itself a language model; decode the two as an ensemble (--path a.pt:b.pt)" % args.path)
    dtype = torch.bfloat16 if (args.fp16 or args.bf16) else torch.float32
    models = [m.to("cuda", dtype).eval() for m in models]
    src_dict, tgt_dict = task.source_dictionary, task.target_dictionary
    lm = None
    if args.lm_path is not None:
        lm = checkpoint_utils.load_language_model(args.lm_path, tgt_dict).to("cuda", dtype).eval()
    generator = task.build_generator(models, args, extra_gen_cls_kwargs={"lm_model": lm, "lm_weight": args.lm_weight})
    tokenizer, bpe = task.build_tokenizer(args), task.build_bpe(args)

    def encode_fn(x):
        if tokenizer is not None:
            x = tokenizer.encode(x)
        if bpe is not None:
            x = bpe.encode(x)
        return x

    def decode_fn(x):
        if bpe is not None:
            x = bpe.decode(x)
        if tokenizer is not None:
            x = tokenizer.decode(x)
        return x

    max_positions = resolve_max_positions(task.max_positions(), *[m.max_positions() for m in models])
    prompt_ok = None
    if is_lm:
        limit = min(m.max_decoder_positions() for m in models)
        prompt_ok = lambda n: lm_prompt_limit(n, args.max_len_a, args.max_len_b, limit)
    strip = ()
    if is_speech:  # speech_to_text.py:130-135: language tags are not printed
        from .data import SpeechToTextDataset
        strip = {i for s, i in tgt_dict.indices.items() if SpeechToTextDataset.is_lang_tag(s)}
    start_id, nsent, ntok = 0, 0, 0
    for inputs in buffered_read(args.input, args.buffer_size):
        results = []
        for ids, batch, lists in make_batches(inputs, args, task, max_positions, encode_fn, start_id, sys.stderr, prompt_ok):
            ni = batch["net_input"]
            if "src_audio" in ni:  # fbank route (data.py): filter banks of the audio batch, computed on the device
                ni = fbank.materialize({k: (v.cuda() if torch.is_tensor(v) else v) for k, v in ni.items()},
                                       max_frames=int(ni["src_lengths"].max()))
            src = ni["src_tokens"]
            text = not src.is_floating_point()
            src_host = src.cpu() if text else None
            src = src.to("cuda", dtype) if (src.dim() == 3 and src.is_floating_point()) else src.cuda()
            sample = {"net_input": {"src_tokens": src, "src_lengths": ni["src_lengths"].cuda()}}
            packed = None
            if lists is not None:
                from .lexical_constraints import pack_constraints
                packed = pack_constraints(lists, pad=tgt_dict.pad(), eos=tgt_dict.eos())
            t0 = time.time()
            translations = task.inference_step(generator, models, sample, constraints=packed)
            torch.cuda.synchronize()
            translate_time = time.time() - t0
            total_translate_time += translate_time
            for i, (pos, hypos) in enumerate(zip(ids, translations)):
                src_i = src_host[i][src_host[i].ne(tgt_dict.pad())] if text else None  # utils.strip_pad
                results.append((start_id + pos, src_i, hypos, {"constraints": lists[i] if lists is not None else [],
                                                                "time": translate_time / len(translations)}))
        ntok += print_translations(results, args, src_dict, tgt_dict, decode_fn, strip)
        nsent += len(results)
        start_id += len(inputs)
    summary = {"event": "interactive", "sentences": nsent, "tokens": ntok, "seconds": time.time() - start_time,
               "translate_seconds": total_translate_time, "beam": args.beam, "models": len(models), "ignored_flags": ignored}
    print(json.dumps(summary), file=sys.stderr, flush=True)
    return summary


# --------------------------------------------------------------------------------------------------------------------
def infer_parser():
    """The options of fairseq_infer.py: examples/speech_recognition/infer.py:31-86 and the generation group, same names and defaults."""
    p = argparse.ArgumentParser(allow_abbrev=False)
    p.add_argument("data")
    p.add_argument("--task", default="audio_pretraining")
    p.add_argument("--labels", default=None, help="extension of the label file (e.g. ltr)")
    p.add_argument("--path", default=None, help="the wav2vec_ctc checkpoint (not needed with --load-emissions)")
    p.add_argument("--gen-subset", default="test")
    p.add_argument("--criterion", default="ctc")
    p.add_argument("--w2l-decoder", default="viterbi", choices=["viterbi", "beam", "kenlm", "fairseqlm"],
                   help="viterbi: best path; beam: CTC prefix beam search (kenlm / fairseqlm need bindings this build does not have)")
    p.add_argument("--beam", type=int, default=5)
    p.add_argument("--nbest", type=int, default=1)
    p.add_argument("--beam-threshold", type=float, default=25.0)
    p.add_argument("--beam-size-token", type=int, default=100)
    p.add_argument("--lm-model", "--kenlm-model", default=None, dest="lm_model", help="a transformer_lm checkpoint over the target dictionary")
    p.add_argument("--lm-weight", type=float, default=0.2)
    p.add_argument("--word-score", type=float, default=1.0)
    p.add_argument("--unk-weight", type=float, default=-math.inf)
    p.add_argument("--sil-weight", type=float, default=0.0)
    p.add_argument("--lexicon", default=None)
    p.add_argument("--dump-features", default=None)
    p.add_argument("--post-process", "--remove-bpe", default="letter", dest="post_process")
    p.add_argument("--results-path", default=None)
    p.add_argument("--max-tokens", type=int, default=None)
    p.add_argument("--max-sentences", "--batch-size", type=int, default=None, dest="batch_size")
    p.add_argument("--sample-rate", type=int, default=16000)
    p.add_argument("--normalize", action="store_true")
    p.add_argument("--dump-emissions", default=None, help="write the fp32 log-probabilities of every utterance to this file and stop")
    p.add_argument("--load-emissions", default=None, help="decode these emissions instead of running a model")
    p.add_argument("--fp16", action="store_true")
    p.add_argument("--bf16", action="store_true")
    p.add_argument("--quiet", action="store_true")
    p.add_argument("--seed", type=int, default=1)
    return p


def check_infer_args(args):
    """Everything infer.py offers that this build does not is refused by name, before any file is opened."""
    if args.task != "audio_pretraining":
        raise NotImplementedError("--task %s: fairseq_infer.py transcribes with the audio_pretraining task" % args.task)
    if not args.labels:
        raise ValueError("--labels is required: the references and the dictionary dict.<labels>.txt are found by it")
    if args.criterion == "asg_loss":
        raise NotImplementedError("--criterion asg_loss is not built (its transitions come from the wav2letter bindings): use --criterion ctc")
    if args.criterion != "ctc":
        raise NotImplementedError("--criterion %s: fairseq_infer.py decodes models trained with --criterion ctc" % args.criterion)
    if args.w2l_decoder in ("kenlm", "fairseqlm"):
        raise NotImplementedError("--w2l-decoder %s needs the flashlight / KenLM bindings, which are not in this build: use --w2l-decoder beam "
                                  "(CTC prefix beam search; --lm-model rescores its n best with a transformer_lm)" % args.w2l_decoder)
    if args.lexicon is not None:
        raise NotImplementedError("--lexicon (lexicon-constrained decoding) needs the flashlight bindings, which are not in this build: use "
                                  "--w2l-decoder beam, which is lexicon-free")
    if args.sil_weight != 0:
        raise NotImplementedError("--sil-weight %g is not built: the beam decoder has no silence score" % args.sil_weight)
    if args.unk_weight != -math.inf:
        raise NotImplementedError("--unk-weight %g is not built: the beam decoder has no lexicon and so no unknown word" % args.unk_weight)
    if args.dump_features is not None:
        raise NotImplementedError("--dump-features is not built: --dump-emissions writes the log-probabilities")
    if args.path is not None and len(args.path.split(":")) > 1:
        raise NotImplementedError("--path with several checkpoints is not built: infer.py decodes with models[0] only; pass one file")
    if args.path is None and args.load_emissions is None:
        raise ValueError("--path is required (or --load-emissions, which needs no checkpoint)")
    if args.lm_model is not None and args.w2l_decoder != "beam":
        raise ValueError("--lm-model rescores the n best of --w2l-decoder beam; %s has one hypothesis" % args.w2l_decoder)
    if args.max_tokens is None and args.batch_size is None:
        args.max_tokens = 4000000
    return args


def infer_result_files(args):
    """infer.py:184-207: {kind: path} of the four result files, or None without --results-path."""
    if not args.results_path:
        return None
    stem = os.path.basename(args.path if args.path is not None else args.load_emissions)
    return {k: os.path.join(args.results_path, "%s-%s-%s.txt" % (k, stem, args.gen_subset)) for k in ("hypo.word", "hypo.units", "ref.word", "ref.units")}


def word_errors(hyp_words, ref_words):
    """(Levenshtein distance of the two word lists — cst_edit_distance over word ids —, the reference's length)."""
    from . import kernels as K
    ids = {}
    enc = lambda ws: [ids.setdefault(w, len(ids)) for w in ws]
    return K.edit_distance(enc(hyp_words), enc(ref_words)), len(ref_words)


def process_predictions(args, hypos, tgt_dict, target_tokens, files, speaker, sid):
    """infer.py:115-178: writes the nbest hypotheses and the reference of one utterance as "<text> (<speaker>-<id>)" lines; returns
    (word errors, reference words, unit errors, reference units) of the TOP hypothesis."""
    from . import kernels as K
    from .dictionary import post_process
    tgt_pieces = tgt_dict.string(target_tokens)
    tgt_words = post_process(tgt_pieces, args.post_process)
    first = None
    for hypo in hypos[:min(len(hypos), args.nbest)]:
        toks = [int(t) for t in hypo["tokens"].tolist()]
        hyp_pieces = tgt_dict.string(toks)
        hyp_words = post_process(hyp_pieces, args.post_process)
        if first is None:
            first = (toks, hyp_words)
        if files is not None:
            print("{} ({}-{})".format(hyp_pieces, speaker, sid), file=files["hypo.units"])
            print("{} ({}-{})".format(hyp_words, speaker, sid), file=files["hypo.word"])
            print("{} ({}-{})".format(tgt_pieces, speaker, sid), file=files["ref.units"])
            print("{} ({}-{})".format(tgt_words, speaker, sid), file=files["ref.word"])
        if not args.quiet:
            print("HYPO:" + hyp_words)
            print("TARGET:" + tgt_words)
            print("___________________")
    toks, hyp_words = first if first is not None else ([], "")
    w_err, w_len = word_errors(hyp_words.split(), tgt_words.split())
    return w_err, w_len, K.edit_distance(toks, list(target_tokens)), len(target_tokens)


def infer_main(argv=None):
    """examples/speech_recognition/infer.py:211-454 for a wav2vec_ctc checkpoint: transcribes a subset, writes hypothesis / reference
    files, reports WER.  Returns (task, wer)."""
    import numpy as np

    from . import ctc_decoder as CD
    argv = list(sys.argv[1:] if argv is None else argv)
    args, ignored = infer_parser().parse_known_args(argv)
    check_infer_args(args)
    limit_host_threads()
    host = CD.host_route()
    targs = argparse.Namespace(data=args.data, labels=args.labels, criterion="ctc", sample_rate=args.sample_rate, normalize=args.normalize,
                               max_sample_size=None, min_sample_size=None, enable_padding=False, task="audio_pretraining")
    task = tasks.AudioPretrainingTask.setup_task(targs)
    tgt_dict = task.target_dictionary
    dtype = torch.bfloat16 if (args.fp16 or args.bf16) else torch.float32
    models, emissions = None, None
    if args.load_emissions is not None:
        emissions = np.load(args.load_emissions, allow_pickle=True)
    else:
        models, _, _ = checkpoint_utils.load_model_ensemble_and_task([args.path], arg_overrides={"data": args.data}, task=task)
        models = [m.to("cuda", dtype).eval() for m in models]
    lm = lm_dict = None
    if args.lm_model is not None:
        from .dictionary import Dictionary
        lm_data = getattr(checkpoint_utils.load_checkpoint_to_cpu(args.lm_model).get("args"), "data", None)
        lm_dict_path = os.path.join(str(lm_data).split(":")[0], "dict.txt") if lm_data else None
        lm_dict = Dictionary.load(lm_dict_path) if lm_dict_path and os.path.exists(lm_dict_path) else tgt_dict
        CD.check_lm_dictionary(lm_dict, tgt_dict)
        lm = checkpoint_utils.load_language_model(args.lm_model, tgt_dict).to("cuda", dtype).eval()
    if args.w2l_decoder == "viterbi":
        decoder = CD.CtcViterbiDecoder(args, tgt_dict)
    else:
        decoder = CD.CtcBeamDecoder(args, tgt_dict, lm_model=lm, lm_dict=lm_dict)
    ds = task.load_dataset(args.gen_subset)
    itr = task.get_batch_iterator(ds, max_tokens=args.max_tokens, max_sentences=args.batch_size, max_positions=(sys.maxsize, sys.maxsize),
                                  ignore_invalid_inputs=True, seed=args.seed)
    names = infer_result_files(args) if args.dump_emissions is None else None
    files = None
    if names is not None:
        os.makedirs(args.results_path, exist_ok=True)
        files = {k: open(v, "w") for k, v in names.items()}
    errs_t = lengths_t = c_err_t = c_len_t = nsent = 0
    dumped, t0 = {}, time.time()
    for sample in itr.next_epoch_itr(shuffle=False):
        if not sample or "net_input" not in sample:
            continue
        ids = sample["id"].tolist()
        if emissions is not None:  # infer.py:283-294, 360-365: the stored log-probabilities stand in for the model
            rows = [torch.from_numpy(np.asarray(emissions[i], dtype=np.float32)) for i in ids]
            lens = torch.tensor([r.shape[0] for r in rows], dtype=torch.int64)
            em = torch.zeros(int(lens.max()), len(rows), rows[0].shape[1], dtype=torch.float32)
            for b, r in enumerate(rows):
                em[:r.shape[0], b] = r
            hypos = decoder.decode(em if host else em.cuda(), lens if host else lens.cuda())
        else:
            ni = {k: (v.to("cuda", dtype) if v.is_floating_point() else v.cuda()) for k, v in sample["net_input"].items()}
            logits, lens = decoder.get_emissions(models, {"net_input": ni})
            if args.dump_emissions is not None:
                lp = torch.log_softmax(logits.float(), dim=-1).cpu()
                for b, (i, n) in enumerate(zip(ids, lens.tolist())):
                    dumped[i] = lp[:n, b].numpy().copy()
                continue
            hypos = decoder.decode(logits, lens)
        for b, sid in enumerate(ids):
            toks = sample["target"][b]
            target_tokens = toks[(toks != tgt_dict.pad()) & (toks != tgt_dict.eos())].tolist()
            w_err, w_len, c_err, c_len = process_predictions(args, hypos[b], tgt_dict, target_tokens, files, None, sid)
            errs_t, lengths_t, c_err_t, c_len_t = errs_t + w_err, lengths_t + w_len, c_err_t + c_err, c_len_t + c_len
        nsent += len(ids)
    if files is not None:
        for f in files.values():
            f.close()
    if args.dump_emissions is not None:  # infer.py:421-427: the list indexed by sample id
        out = np.empty(len(dumped), dtype=object)
        for i in range(len(dumped)):
            out[i] = dumped[i]
        with open(args.dump_emissions, "wb") as f:
            np.save(f, out, allow_pickle=True)
        print("saved %d emissions to %s" % (len(dumped), args.dump_emissions))
        return task, None
    dt = time.time() - t0
    wer = errs_t * 100.0 / lengths_t if lengths_t > 0 else None
    print("WER: {}".format(wer))
    print("| Processed {} sentences ({} tokens) in {:.1f}s ({:.2f} sentences/s, {:.2f} tokens/s)".format(
        nsent, c_len_t, dt, nsent / max(dt, 1e-9), c_len_t / max(dt, 1e-9)))
    print("| Generate {} with beam={}".format(args.gen_subset, args.beam))
    print(json.dumps({"event": "infer", "subset": args.gen_subset, "decoder": args.w2l_decoder, "route": "host" if host else getattr(decoder, "last_route", None) or "device",
                      "wer": wer, "w_errors": errs_t, "w_total": lengths_t, "c_errors": c_err_t, "c_total": c_len_t, "sentences": nsent,
                      "result_files": names, "ignored_flags": ignored}), flush=True)
    return task, wer
