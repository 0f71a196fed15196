#!/usr/bin/env python3
"""Golden fixtures of the `language_modeling` task, made by the REAL reference:

  tests/golden/lm_tiny/       a synthetic monolingual corpus (written HERE: 30 train / 8 valid / 6 test lines over the 56 words of the
                              tiny fixtures' dictionary; a one-word line, empty lines — eos alone once binarised, the document separators
                              of `complete_doc` — and a line longer than either block size) binarised by the reference's
                              fairseq_cli/preprocess.py --only-source: {train,valid,test}.{bin,idx} (uint16 streams), dict.txt; and one
                              more split `noeos` written through the reference's MMapIndexedDatasetBuilder with vocab_size=None (int32
                              stream) whose sentences do NOT end in eos; the text itself is kept beside them (corpus/*.txt)
  tests/golden/lm_tiny.npz    what the reference's LanguageModelingTask / TokenBlockDataset (over the Cython token_block_utils_fast,
                              compiled from the reference's .pyx into a temp dir) / MonolingualDataset / EpochBatchIterator make of it:
                              per break mode and block size (7 and 16: blocks begin inside sentences and at their first tokens) the
                              slice indices, the block-to-sentence index, the sizes, every (source, target) item, ordered_indices under
                              a seed, the size filter and the --max-tokens batches; the `noeos` split in `none` and `complete` modes;
                              every collated batch of one epoch for `none` and `eos`; a 2-layer transformer_lm (the LM_ARGS of
                              make_decode_lm_goldens.py, fitted for a few Adam steps, parameters rounded to values float16 holds
                              exactly and stored as float32); for two batches — one full-width from `none`, one padded from `eos` —
                              the reference `cross_entropy` criterion's loss, sample_size, logits, every parameter gradient and, per fc1
                              neuron, the smallest |pre-activation| (where two fp32 evaluations of ReLU' may differ); and the
                              eval-lm totals on `valid` in `none` and `eos` modes.

eval_lm.main itself cannot run under the harness's omegaconf stub (it needs hydra's ConfigStore and convert_namespace_to_omegaconf).
The totals are therefore formed HERE from the reference SequenceScorer's positional scores per sample, by the formula of
fairseq_cli/eval_lm.py:191-220 and :262 (no BPE marker: nothing is merged; +-inf scores dropped; count = what remains;
loss = -sum / count / ln 2); the positional scores themselves are stored too.

Build container only:   python tools/ref_harness/make_lm_goldens.py
The fixtures hold data only (what the reference's programs wrote and computed), never reference source."""
import importlib.util
import math
import os
import shutil
import subprocess
import sys
import tempfile
from argparse import Namespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ref_import import REF, import_reference  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.abspath(os.path.join(HERE, "..", "..", "tests", "golden"))
ROOT = os.path.join(GOLDEN, "lm_tiny")
OUT = os.path.join(GOLDEN, "lm_tiny.npz")
WORDS = ["w%d" % i for i in range(56)]   # the tiny fixtures' dictionary: 4 specials + 56 words = 60 symbols
MODES = ("none", "complete", "complete_doc", "eos")
BLOCK_SIZES = (7, 16)
LIMIT = 12         # the position limit the tests filter with
MAX_TOKENS = 48
LM_ARGS = dict(arch="transformer_lm", decoder_layers=2, decoder_embed_dim=64, decoder_ffn_embed_dim=128, decoder_attention_heads=2,
               dropout=0.0, attention_dropout=0.0, share_decoder_input_output_embed=True, max_target_positions=1024, tokens_per_sample=1024)
LM_SEED, FIT_STEPS, FIT_LR = 41, 12, 3e-3


def make_corpus(tmp):
    """{split: [lines]}; the special cases: a one-word line, empty lines (two of them document separators in the middle of train), a
    line longer than both block sizes."""
    r = np.random.RandomState(9)

    def line(n):
        return " ".join(r.choice(WORDS, size=n))

    splits = {}
    for split, n in (("train", 30), ("valid", 8), ("test", 6)):
        lines = [line(int(r.randint(2, 10))) for _ in range(n)]
        lines[1] = line(1)          # a one-word line
        lines[3] = ""               # an empty line: eos alone
        if split == "train":
            lines[6] = line(21)     # longer than either block size
            lines[11] = ""          # a document separator
            lines[19] = ""          # another one
            lines[20] = line(1)     # a one-sentence document of 2 tokens
            lines[24] = line(12)
        if split == "valid":
            lines[5] = line(18)
        splits[split] = lines
    text = os.path.join(ROOT, "corpus")
    os.makedirs(text, exist_ok=True)
    for split, lines in splits.items():
        for path in (os.path.join(tmp, split), os.path.join(text, split + ".txt")):
            with open(path, "w", encoding="utf-8") as f:
                f.write("".join(l + "\n" for l in lines))
    with open(os.path.join(tmp, "dict.txt"), "w", encoding="utf-8") as f:
        for i, w in enumerate(WORDS):
            f.write("%s %d\n" % (w, 1000 - i))
    return splits


def binarise(tmp):
    """fairseq-preprocess --only-source --trainpref .. --validpref .. --testpref .. --srcdict D (one worker)."""
    from fairseq import options
    from fairseq_cli import preprocess
    parser = options.get_preprocessing_parser()
    args = parser.parse_args(["--only-source", "--trainpref", os.path.join(tmp, "train"), "--validpref", os.path.join(tmp, "valid"),
                              "--testpref", os.path.join(tmp, "test"), "--destdir", ROOT, "--thresholdsrc", "0",
                              "--srcdict", os.path.join(tmp, "dict.txt"), "--workers", "1"])
    preprocess.main(args)
    log = os.path.join(ROOT, "preprocess.log")  # (names the temp directory: not a fixture)
    if os.path.exists(log):
        os.remove(log)


def write_noeos_split():
    """The train split's first sentences once more as `noeos`, through the reference's builder with vocab_size=None (int32), every
    sentence WITHOUT its final eos (sentences that were eos alone are left out: a sentence holds at least one token)."""
    from fairseq.data import indexed_dataset
    ds = indexed_dataset.MMapIndexedDataset(os.path.join(ROOT, "train"))
    prefix = os.path.join(ROOT, "noeos")
    b = indexed_dataset.make_builder(prefix + ".bin", impl="mmap", vocab_size=None)
    for i in range(14):
        if len(ds[i]) > 1:
            assert int(ds[i][-1]) == 2
            b.add_item(ds[i][:-1])
    b.finalize(prefix + ".idx")
    out = indexed_dataset.MMapIndexedDataset(prefix)
    assert out._index.dtype == np.int32 and all(int(out[i][-1]) != 2 for i in range(len(out)))


def build_cython_token_blocks(tmp):
    """Compile the reference's token_block_utils_fast.pyx (unmodified, read in place) into `tmp` and register it under its package name."""
    import sysconfig
    src = os.path.join(REF, "fairseq", "data", "token_block_utils_fast.pyx")
    cpp = os.path.join(tmp, "token_block_utils_fast.cpp")
    subprocess.check_call([sys.executable, "-m", "cython", "--cplus", "-3", src, "-o", cpp])
    so = os.path.join(tmp, "token_block_utils_fast" + sysconfig.get_config_var("EXT_SUFFIX"))
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-w", "-I" + sysconfig.get_paths()["include"], "-I" + np.get_include(),
                           cpp, "-o", so])
    spec = importlib.util.spec_from_file_location("fairseq.data.token_block_utils_fast", so)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sys.modules["fairseq.data.token_block_utils_fast"] = mod


def task_args(mode, block_size):
    return Namespace(data=ROOT, sample_break_mode=mode, tokens_per_sample=block_size, output_dictionary_size=-1, self_target=False,
                     future_target=False, past_target=False, add_bos_token=False, max_target_positions=None, shorten_method="none",
                     shorten_data_split_list="", dataset_impl="mmap", seed=1, train_subset="train")


def load(mode, block_size, split):
    from fairseq.tasks.language_modeling import LanguageModelingTask
    task = LanguageModelingTask.setup_task(task_args(mode, block_size))
    task.load_dataset(split)
    return task, task.dataset(split)


def put_batch(out, key, s):
    out[key + "/id"] = s["id"].numpy()
    out[key + "/ntokens"] = np.int64(s["ntokens"])
    out[key + "/nsentences"] = np.int64(s["nsentences"])
    out[key + "/target"] = s["target"].numpy()
    out[key + "/src_tokens"] = s["net_input"]["src_tokens"].numpy()
    out[key + "/src_lengths"] = s["net_input"]["src_lengths"].numpy()


def record_data(out):
    from fairseq.data import data_utils, iterators
    for split in ("train", "valid", "noeos"):
        for mode in MODES if split != "noeos" else ("none", "complete"):
            for bs in BLOCK_SIZES:
                task, ds = load(mode, bs, split)
                tb = ds.dataset
                key = "%s/%s/%d" % (split, mode, bs)
                out[key + "/slice_indices"] = np.asarray(tb.slice_indices)
                out[key + "/block_to_dataset_index"] = np.asarray(tb.block_to_dataset_index)
                out[key + "/sizes"] = np.asarray(ds.sizes)
                items = [ds[i] for i in range(len(ds))]
                out[key + "/src_flat"] = np.concatenate([it["source"].numpy() for it in items])
                out[key + "/tgt_flat"] = np.concatenate([it["target"].numpy() for it in items])
                assert all(len(it["source"]) == len(it["target"]) == int(ds.sizes[i]) for i, it in enumerate(items))
                with data_utils.numpy_seed(1):
                    idx = ds.ordered_indices()
                out[key + "/ordered"] = np.asarray(idx)
                idx_f, ignored = ds.filter_indices_by_size(idx, LIMIT)
                out[key + "/filtered"] = np.asarray(idx_f)
                out[key + "/ignored"] = np.asarray(ignored, dtype=np.int64)
                batches = ds.batch_by_size(idx, max_tokens=MAX_TOKENS)
                out[key + "/batches/sizes"] = np.array([len(b) for b in batches])
                out[key + "/batches/flat"] = np.concatenate([np.asarray(b) for b in batches])
                if mode in ("none", "eos") and bs == 16 and split != "valid":  # every collated batch of one epoch
                    it = iterators.EpochBatchIterator(ds, ds.collater, batches, seed=1, num_shards=1, shard_id=0, epoch=1)
                    samples = list(it.next_epoch_itr(shuffle=(split == "train")))
                    out[key + "/collated/n"] = np.int64(len(samples))
                    for j, s in enumerate(samples):
                        put_batch(out, "%s/collated/%d" % (key, j), s)
        print(split, "sizes", np.asarray(out["%s/none/16/sizes" % split]).tolist())
    out["dict_len"] = np.int64(len(task.source_dictionary))
    out["meta/limit"], out["meta/max_tokens"] = np.int64(LIMIT), np.int64(MAX_TOKENS)
    # the fixture must be able to tell the two readings of "the token before the block" apart
    tb = load("complete", 7, "noeos")[1].dataset
    later = [i for i in range(1, len(tb)) if tb.block_to_dataset_index[i][1] == 0]
    assert later and all(int(tb[i][0][0]) == 2 for i in later)
    inside = [i for i in range(len(load("none", 7, "noeos")[1].dataset)) if load("none", 7, "noeos")[1].dataset.block_to_dataset_index[i][1] > 0]
    assert inside, "no block of the noeos split begins inside a sentence"


def build_lm(task, out):
    from fairseq.models.transformer_lm import TransformerLanguageModel
    torch.manual_seed(LM_SEED)
    lm = TransformerLanguageModel.build_model(Namespace(**LM_ARGS), task)
    n = int(out["train/none/16/collated/n"])
    opt = torch.optim.Adam(lm.parameters(), lr=FIT_LR)
    lm.train()
    for step in range(FIT_STEPS):
        key = "train/none/16/collated/%d" % (step % n)
        opt.zero_grad()
        logits = lm(torch.from_numpy(out[key + "/src_tokens"]))[0]
        loss = torch.nn.functional.cross_entropy(logits.reshape(-1, logits.size(-1)), torch.from_numpy(out[key + "/target"]).reshape(-1),
                                                 ignore_index=task.source_dictionary.pad())
        loss.backward()
        opt.step()
    with torch.no_grad():
        for v in lm.parameters():
            v.copy_(v.half().float())
    print("LM fitted: loss %.3f after %d steps" % (float(loss.detach()), FIT_STEPS))
    out["meta/lm_args"] = np.array(repr(LM_ARGS))
    out["meta/lm_keys"] = np.array(sorted(lm.state_dict().keys()))
    for name, v in lm.state_dict().items():
        if v.is_floating_point() and "_float_tensor" not in name and name != "decoder.version":
            assert torch.equal(v.half().float(), v), name
            out["lm/param/" + name] = v.detach().float().numpy()
    return lm


def record_criterion(out, task, lm):
    """The reference cross_entropy criterion on two batches: one full-width from `none`, one padded from `eos`."""
    from fairseq.criterions.cross_entropy import CrossEntropyCriterion
    crit = CrossEntropyCriterion(task, sentence_avg=False)
    pad = task.source_dictionary.pad()

    def pick(mode, want_padding):
        for j in range(int(out["train/%s/16/collated/n" % mode])):
            key = "train/%s/16/collated/%d" % (mode, j)
            tgt = out[key + "/target"]
            if tgt.shape[0] > 1 and bool((tgt == pad).any()) == want_padding and (want_padding or tgt.shape[1] == 16):
                return key
        raise AssertionError("no such batch: %s padding=%s" % (mode, want_padding))

    for tag, key in (("full", pick("none", False)), ("padded", pick("eos", True))):
        sample = {"id": torch.from_numpy(out[key + "/id"]), "nsentences": int(out[key + "/nsentences"]), "ntokens": int(out[key + "/ntokens"]),
                  "net_input": {"src_tokens": torch.from_numpy(out[key + "/src_tokens"]), "src_lengths": torch.from_numpy(out[key + "/src_lengths"])},
                  "target": torch.from_numpy(out[key + "/target"])}
        lm.train()
        lm.zero_grad()
        taps, hooks = {}, []
        for i, layer in enumerate(lm.decoder.layers):  # per fc1 neuron the smallest |pre-activation| over the batch's tokens: where ReLU' may tie
            hooks.append(layer.fc1.register_forward_hook(
                lambda m, a, z, i=i: taps.__setitem__("decoder.layers.%d.fc1" % i, z.detach().abs().reshape(-1, z.size(-1)).amin(dim=0))))
        loss, sample_size, log = crit(lm, sample)
        for h in hooks:
            h.remove()
        loss.backward()
        for name, v in taps.items():
            out["crit/%s/relu_min_abs/%s" % (tag, name)] = v.float().numpy()
        with torch.no_grad():
            logits = lm(**sample["net_input"])[0]
        out["crit/%s/batch" % tag] = np.array(key)
        out["crit/%s/loss" % tag] = np.float64(float(loss.detach()))
        out["crit/%s/sample_size" % tag] = np.int64(sample_size)
        out["crit/%s/log_ntokens" % tag] = np.int64(log["ntokens"])
        out["crit/%s/log_nsentences" % tag] = np.int64(log["nsentences"])
        out["crit/%s/logits" % tag] = logits.float().numpy()
        for name, p in lm.named_parameters():
            out["crit/%s/grad/%s" % (tag, name)] = p.grad.detach().float().numpy()
        print("criterion", tag, key, "loss %.4f" % float(loss.detach()), "sample_size", sample_size, "shape", tuple(sample["target"].shape))


def record_eval_lm(out, lm):
    """The totals of fairseq_cli/eval_lm.py on `valid` (tokens-per-sample 16), formed from the reference scorer's positional scores."""
    from fairseq.sequence_scorer import SequenceScorer
    lm.eval()
    for mode in ("none", "eos"):
        task, ds = load(mode, 16, "valid")
        itr = task.get_batch_iterator(dataset=ds, max_tokens=MAX_TOKENS, max_sentences=None, max_positions=lm.max_positions(),
                                      ignore_invalid_inputs=True).next_epoch_itr(shuffle=False)
        scorer = SequenceScorer(task.target_dictionary)
        score_sum, count, ids, flat = 0.0, 0, [], []
        for sample in itr:
            if "net_input" not in sample:
                continue
            with torch.no_grad():
                hypos = scorer.generate([lm], sample)
            for i, h in enumerate(hypos):
                pos = h[0]["positional_scores"].float()
                inf = pos.eq(float("inf")) | pos.eq(float("-inf"))
                pos = pos[~inf]
                score_sum += float(pos.sum())
                count += pos.numel()
                ids.append(int(sample["id"][i]))
                flat.append(h[0]["positional_scores"].float().numpy())
        loss = -score_sum / count / math.log(2)
        key = "eval_lm/valid/%s" % mode
        out[key + "/score_sum"], out[key + "/count"], out[key + "/loss"] = np.float64(score_sum), np.int64(count), np.float64(loss)
        out[key + "/ids"] = np.array(ids)
        out[key + "/pos_sizes"] = np.array([len(f) for f in flat])
        out[key + "/pos_flat"] = np.concatenate(flat)
        print("eval-lm valid", mode, "sum %.4f count %d loss %.4f ppl %.2f" % (score_sum, count, loss, 2 ** loss))


def main():
    if os.path.isdir(ROOT):
        shutil.rmtree(ROOT)
    os.makedirs(ROOT)
    import_reference()
    import make_data_goldens as DG
    tmp = tempfile.mkdtemp()
    DG.build_cython_batcher(tmp)
    build_cython_token_blocks(tmp)
    make_corpus(tmp)
    binarise(tmp)
    write_noeos_split()
    out = {}
    record_data(out)
    task, _ = load("none", 16, "train")
    lm = build_lm(task, out)
    record_criterion(out, task, lm)
    record_eval_lm(out, lm)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(out), "arrays;", sorted(os.listdir(ROOT)))


if __name__ == "__main__":
    main()
