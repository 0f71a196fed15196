"""The `translation` task on the host (no GPU): the binarised-corpus reader, LanguagePairDataset and its host collater against the
fixture the reference made (tests/golden/translation_tiny/, translation_tiny.npz: tools/ref_harness/make_translation_goldens.py), the
resident route's record, BLEU statistics and score, the string decoding of --eval-bleu, the refused options, and the flag set of
chimera/scripts/train-en2any-MT.sh."""
import math
import os
import shutil
import struct
from argparse import Namespace
from importlib import import_module

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, load_pkg

load_pkg()
ID = import_module("chimera-st_amd.indexed_dataset")
P = import_module("chimera-st_amd.language_pair_dataset")
D = import_module("chimera-st_amd.data")
B = import_module("chimera-st_amd.bleu")
tasks = import_module("chimera-st_amd.tasks")
reg = import_module("chimera-st_amd.registry")
Dictionary = import_module("chimera-st_amd.dictionary").Dictionary

ROOT = os.path.join(GOLDEN, "translation_tiny")
LIMIT, MAX_TOKENS = (20, 20), 40


@pytest.fixture(autouse=True)
def host_route(monkeypatch):
    """These tests state the batch on the host, also where a GPU is present."""
    monkeypatch.setenv("CST_PAIR_COLLATE", "host")


@pytest.fixture(scope="module")
def g():
    return load_golden("translation_tiny.npz")


def task_args(**over):
    a = Namespace(data=ROOT, source_lang=None, target_lang=None, left_pad_source="True", left_pad_target="False", max_source_positions=1024,
                  max_target_positions=1024, required_seq_len_multiple=1, dataset_impl=None, eval_bleu=False)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def load(split, **over):
    t = tasks.TranslationTask.setup_task(task_args(**over))
    return t, t.load_dataset(split)


# ---- the reader ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split,dtype", [("train", np.uint16), ("valid", np.uint16), ("test", np.uint16), ("valid32", np.int32)])
def test_reader_reproduces_sizes_and_every_sentence(g, split, dtype):
    for col, lang, flat in ((0, "en", "src_flat"), (1, "de", "tgt_flat")):
        ds = ID.MMapIndexedDataset(os.path.join(ROOT, "%s.en-de.%s" % (split, lang)))
        assert ds.dtype == np.dtype(dtype) and str(g[split + "/dtype"]) == np.dtype(dtype).name
        np.testing.assert_array_equal(np.asarray(ds.sizes), g[split + "/sizes"][:, col])
        items = [ds[i] for i in range(len(ds))]
        assert all(it.dtype == torch.int64 for it in items)
        np.testing.assert_array_equal(torch.cat(items).numpy(), g[split + "/" + flat])
        assert ds.offsets[0] == 0 and ds.offsets[-1] == len(ds.stream) and np.array_equal(np.diff(ds.offsets), ds.sizes)
        with pytest.raises(IndexError):
            ds[len(ds)]
    assert (g["train/sizes"] == 1).any()  # the empty line is kept as eos alone


def test_int64_and_uint8_streams_are_read(tmp_path):
    for code, dt in ((5, np.int64), (1, np.uint8)):
        sents = [np.array([7, 9, 2], dt), np.array([2], dt), np.array([4, 5, 6, 8, 2], dt)]
        prefix = str(tmp_path / ("x%d" % code))
        with open(prefix + ".bin", "wb") as f:
            f.write(b"".join(s.tobytes() for s in sents))
        sizes = np.array([len(s) for s in sents], np.int32)
        ptrs = np.concatenate([[0], np.cumsum(sizes[:-1])]).astype(np.int64) * np.dtype(dt).itemsize
        with open(prefix + ".idx", "wb") as f:
            f.write(ID.MMAP_MAGIC + struct.pack("<Q", 1) + struct.pack("<B", code) + struct.pack("<Q", len(sents)) + sizes.tobytes() + ptrs.tobytes())
        ds = ID.MMapIndexedDataset(prefix)
        assert ds.dtype == np.dtype(dt) and [ds[i].tolist() for i in range(3)] == [s.tolist() for s in sents]
        ID.write_dataset(prefix + "w", np.concatenate(sents), sizes)  # the package's own writer leaves the same two files
        for ext in (".bin", ".idx"):
            assert open(prefix + "w" + ext, "rb").read() == open(prefix + ext, "rb").read()


def test_other_implementations_are_refused_by_name(tmp_path):
    legacy = str(tmp_path / "train.en-de.en")
    with open(legacy + ".idx", "wb") as f:
        f.write(ID.LEGACY_MAGIC + struct.pack("<Q", 1))
    open(legacy + ".bin", "wb").close()
    with pytest.raises(NotImplementedError, match="lazy.*cached"):
        ID.MMapIndexedDataset(legacy)
    raw = str(tmp_path / "valid.en-de.en")
    with open(raw + ".txt", "w") as f:
        f.write("w1 w2\n")
    with pytest.raises(NotImplementedError, match="raw"):
        ID.MMapIndexedDataset(raw)
    for impl in ("raw", "lazy", "cached"):
        with pytest.raises(NotImplementedError, match="--dataset-impl %s" % impl):
            load("train", dataset_impl=impl)
    floats = str(tmp_path / "f")
    with open(floats + ".idx", "wb") as f:
        f.write(ID.MMAP_MAGIC + struct.pack("<Q", 1) + struct.pack("<B", 6) + struct.pack("<Q", 0))
    open(floats + ".bin", "wb").close()
    with pytest.raises(NotImplementedError, match="dtype code 6"):
        ID.MMapIndexedDataset(floats)


# ---- the task's data ----------------------------------------------------------------------------------------------------------
def test_language_pair_is_inferred_and_dictionaries_load(g):
    t, ds = load("train")
    assert [t.args.source_lang, t.args.target_lang] == list(g["pair"]) == ["en", "de"]
    assert len(t.source_dictionary) == len(t.target_dictionary) == int(g["dict_len"]) == 60
    assert t.args.left_pad_source is True and t.args.left_pad_target is False
    assert t.max_positions() == (1024, 1024)
    np.testing.assert_array_equal(ds.sizes, g["train/sizes"])
    assert ds.num_tokens(5) == 28 and ds.size(5) == (28, 25) and len(ds) == 25
    # the reverse pair finds the same files (translation.py:66-70) with source and target swapped
    t2, ds2 = load("valid", source_lang="de", target_lang="en")
    np.testing.assert_array_equal(ds2.sizes, g["valid/sizes"][:, ::-1])


@pytest.mark.parametrize("split", ["train", "valid", "test", "valid32"])
def test_order_filter_batches_and_epochs_equal_the_reference(g, split):
    t, ds = load(split)
    with D.numpy_seed(1):
        idx = ds.ordered_indices()
    np.testing.assert_array_equal(idx, g[split + "/ordered"])  # ties between equal lengths fall as the reference's mergesorts put them
    idx_f, ignored = ds.filter_indices_by_size(idx, LIMIT)
    np.testing.assert_array_equal(idx_f, g[split + "/filtered"])
    assert ignored == g[split + "/ignored"].tolist()
    for tag, kw in (("tok40", dict(max_tokens=MAX_TOKENS)), ("sent3", dict(max_sentences=3)),
                    ("tok64_mult8", dict(max_tokens=64, required_batch_size_multiple=8))):
        batches = ds.batch_by_size(idx_f, **kw)
        assert [len(b) for b in batches] == g["%s/batches/%s/sizes" % (split, tag)].tolist(), tag
        assert sum(batches, []) == g["%s/batches/%s/flat" % (split, tag)].tolist(), tag
    for num_shards in (1, 2):
        for shard in range(num_shards):
            it = t.get_batch_iterator(ds, max_tokens=MAX_TOKENS, max_positions=LIMIT, ignore_invalid_inputs=True, seed=1,
                                      num_shards=num_shards, shard_id=shard)
            for ep in (1, 2):
                ids = [s["id"].tolist() if s else [] for s in it.next_epoch_itr(shuffle=(split == "train"))]
                key = "%s/epoch%d/shards%d/%d/" % (split, ep, num_shards, shard)
                assert [len(i) for i in ids] == g[key + "sizes"].tolist(), key
                assert sum(ids, []) == g[key + "ids"].tolist(), key
    if split == "train":  # an over-long pair is an error unless it may be skipped (fairseq_task.py get_batch_iterator)
        with pytest.raises(Exception, match="max_positions"):
            t.get_batch_iterator(ds, max_tokens=MAX_TOKENS, max_positions=LIMIT, ignore_invalid_inputs=False)


def assert_batch(s, g, key):
    assert s["id"].tolist() == g[key + "/id"].tolist()
    assert s["ntokens"] == int(g[key + "/ntokens"]) and s["nsentences"] == int(g[key + "/nsentences"])
    for k in ("src_tokens", "src_lengths", "prev_output_tokens"):
        assert s["net_input"][k].dtype == torch.int64
        np.testing.assert_array_equal(s["net_input"][k].numpy(), g[key + "/" + k], err_msg=key + "/" + k)
    np.testing.assert_array_equal(s["target"].numpy(), g[key + "/target"], err_msg=key)
    assert list(s["net_input"]) == ["src_tokens", "src_lengths", "prev_output_tokens"]


@pytest.mark.parametrize("split", ["train", "valid", "test", "valid32"])
def test_every_collated_batch_of_an_epoch_equals_the_reference(g, split):
    t, ds = load(split)
    it = t.get_batch_iterator(ds, max_tokens=MAX_TOKENS, max_positions=LIMIT, ignore_invalid_inputs=True, seed=1)
    samples = list(it.next_epoch_itr(shuffle=(split == "train")))
    assert len(samples) == int(g[split + "/collated/n"])
    for j, s in enumerate(samples):
        assert_batch(s, g, "%s/collated/%d" % (split, j))


@pytest.mark.parametrize("lps,lpt", [("True", "True"), ("False", "False"), ("False", "True")])
def test_left_pad_combinations_and_width_multiple_equal_the_reference(g, lps, lpt):
    t, ds = load("train", left_pad_source=lps, left_pad_target=lpt, required_seq_len_multiple=8)
    keys = sorted(k for k in g if k.startswith("train/padded/src%s_tgt%s/" % (lps, lpt)) and k.endswith("/batch"))
    assert len(keys) == 3
    for k in keys:
        s = ds.collater([ds[int(i)] for i in g[k]])
        assert_batch(s, g, k[:-len("/batch")])
        assert s["net_input"]["src_tokens"].size(1) % 8 == 0 and s["target"].size(1) % 8 == 0


def test_the_resident_record_states_the_host_batch_without_tokens(g):
    """The record of the device route (indices in row order, widths, lengths, token count) agrees with the host collater's batch,
    ties included, and is built from the sizes alone."""
    for kw in (dict(), dict(required_seq_len_multiple=8, left_pad_target="True")):
        t, ds = load("train", **kw)
        assert ds.resident is None and "source" in ds[0]
        with D.numpy_seed(1):
            idx, _ = ds.filter_indices_by_size(ds.ordered_indices(), LIMIT)
        for b in ds.batch_by_size(idx, max_tokens=MAX_TOKENS) + [[3, 15, 0, 4, 8, 12]]:  # (the last: six sources of 6 and 7 tokens)
            host = ds.host_batch(b)
            ds.resident = marker = object()
            try:
                assert ds[b[0]] == {"id": b[0]}
                rec = ds.collater([ds[i] for i in b])
            finally:
                ds.resident = None
            ni = rec["net_input"]
            assert rec["id"].tolist() == host["id"].tolist() == ni["pair_idx"].tolist()
            assert ni["pair_widths"] == (host["net_input"]["src_tokens"].size(1), host["target"].size(1))
            assert ni["src_lengths"].tolist() == host["net_input"]["src_lengths"].tolist()
            assert (rec["ntokens"], rec["nsentences"]) == (host["ntokens"], host["nsentences"]) and ni["pair_corpus"] is marker
            assert P.is_pair_record(rec) and not P.is_pair_record(host)


# ---- refused options ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("over,name", [(dict(upsample_primary=2), "--upsample-primary"), (dict(truncate_source=True), "--truncate-source"),
                                       (dict(load_alignments=True), "--load-alignments"), (dict(num_batch_buckets=4), "--num-batch-buckets")])
def test_each_refused_flag_raises_with_its_own_name(over, name):
    with pytest.raises(NotImplementedError, match=name):
        load("train", **over)


def test_several_data_paths_and_shards_are_refused_by_name(tmp_path):
    with pytest.raises(NotImplementedError, match="colon-separated data paths"):
        tasks.TranslationTask.setup_task(task_args(data=ROOT + os.pathsep + ROOT))
    d = str(tmp_path / "bin")
    shutil.copytree(ROOT, d)
    for lang in ("en", "de"):
        for ext in (".bin", ".idx"):
            shutil.copyfile(os.path.join(d, "valid.en-de.%s%s" % (lang, ext)), os.path.join(d, "train1.en-de.%s%s" % (lang, ext)))
    with pytest.raises(NotImplementedError, match="train1"):
        load("train", data=d)
    with pytest.raises(FileNotFoundError, match="Dataset not found: dev"):
        load("dev")


# ---- BLEU ---------------------------------------------------------------------------------------------------------------------
def stats_of(hyps, refs):
    s = B.corpus_stats(hyps, refs)
    return ([s["_bleu_counts_%d" % i] for i in range(4)], [s["_bleu_totals_%d" % i] for i in range(4)], s["_bleu_sys_len"], s["_bleu_ref_len"])


def test_bleu_statistics_and_score_by_hand():
    assert stats_of(["a b c d e"], ["a b c d e"]) == ([5, 4, 3, 2], [5, 4, 3, 2], 5, 5)
    assert B.bleu_from_stats([5, 4, 3, 2], [5, 4, 3, 2], 5, 5) == pytest.approx(100.0, abs=1e-9)
    assert stats_of(["a a a"], ["a b"])[0] == [1, 0, 0, 0]  # clipped to the reference's multiplicity
    # one zero 4-gram count under `exp` smoothing: precisions 4/5, 2/4, 1/3 and (1/2)/2
    c, t, sl, rl = stats_of(["a b c d x"], ["a b c e x"])
    assert (c, t, sl, rl) == ([4, 2, 1, 0], [5, 4, 3, 2], 5, 5)
    assert B.bleu_from_stats(c, t, sl, rl) == pytest.approx(100.0 * (0.8 * 0.5 * (1.0 / 3.0) * 0.25) ** 0.25, rel=1e-12)
    # two zero counts: the k-th takes 1 / 2^k
    c, t, sl, rl = stats_of(["a b x y z"], ["a b c d e"])
    assert (c, t) == ([2, 1, 0, 0], [5, 4, 3, 2])
    assert B.bleu_from_stats(c, t, sl, rl) == pytest.approx(100.0 * ((2 / 5) * (1 / 4) * (0.5 / 3) * (0.25 / 2)) ** 0.25, rel=1e-12)
    # a short system output: brevity penalty exp(1 - 6/4), all precisions 1
    c, t, sl, rl = stats_of(["a b c d"], ["a b c d e f"])
    assert (c, t, sl, rl) == ([4, 3, 2, 1], [4, 3, 2, 1], 4, 6)
    assert B.bleu_from_stats(c, t, sl, rl) == pytest.approx(100.0 * math.exp(-0.5), rel=1e-12)
    assert B.bleu_from_stats([6, 5, 4, 3], [6, 5, 4, 3], 6, 4) == pytest.approx(100.0)  # a long one is not rewarded
    # the empty hypothesis, and an output too short for a 4-gram: a total of 0 gives 0
    assert stats_of([""], ["a b"]) == ([0, 0, 0, 0], [0, 0, 0, 0], 0, 2)
    assert B.bleu_from_stats([0, 0, 0, 0], [0, 0, 0, 0], 0, 2) == 0.0
    assert B.bleu_from_stats(*stats_of(["a b c"], ["a b c"])) == 0.0


def test_bleu_statistics_add_over_halves_and_derive_the_logged_value():
    hyps = ["a b c d x", "the cat sat on the mat today", "", "w1 w2 w3 w4 w5 w6", "a b"]
    refs = ["a b c e x", "the cat sat on a mat today", "x y", "w1 w2 w3 w9 w5 w6", "a b"]
    whole, h1, h2 = B.corpus_stats(hyps, refs), B.corpus_stats(hyps[:2], refs[:2]), B.corpus_stats(hyps[2:], refs[2:])
    assert set(whole) == {"_bleu_sys_len", "_bleu_ref_len"} | {"_bleu_%s_%d" % (k, i) for k in ("counts", "totals") for i in range(4)}
    summed = {k: float(h1[k] + h2[k]) for k in whole}  # (what cli.validate hands over: float64 sums over batches and ranks)
    assert summed == {k: float(v) for k, v in whole.items()}
    t = tasks.TranslationTask(Namespace(eval_bleu=True), None, None)
    c, tt, sl, rl = stats_of(hyps, refs)
    assert t.derived_metrics(dict(summed, loss=1.0)) == {"bleu": round(B.bleu_from_stats(c, tt, sl, rl), 2)}
    assert 0.0 < t.derived_metrics(summed)["bleu"] < 100.0
    assert t.derived_metrics({"loss": 1.0}) == {} and tasks.TranslationTask(Namespace(eval_bleu=False), None, None).derived_metrics(summed) == {}


# ---- string decoding ----------------------------------------------------------------------------------------------------------
def bleu_task(symbols, **over):
    d = Dictionary()
    for s in symbols:
        d.add_symbol(s)
    a = Namespace(eval_bleu=True, eval_bleu_remove_bpe=None, eval_bleu_detok="space")
    for k, v in over.items():
        setattr(a, k, v)
    return tasks.TranslationTask(a, d, d), d


def test_decoding_removes_bpe_and_names_unknown_tokens():
    t, d = bleu_task(["he@@", "llo", "wor@@", "ld"])
    ids = torch.tensor([4, 5, 3, 6, 7, d.eos(), d.pad()])
    assert t.decode_for_bleu(ids) == "he@@ llo UNKNOWNTOKENINHYP wor@@ ld"
    t.args.eval_bleu_remove_bpe = "@@ "  # the flag without a value (its const)
    assert t.decode_for_bleu(ids) == "hello UNKNOWNTOKENINHYP world"
    assert t.decode_for_bleu(ids, escape_unk=True) == "hello UNKNOWNTOKENINREF world"
    t2, _ = bleu_task(["▁he", "llo", "▁wor", "ld"], eval_bleu_remove_bpe="sentencepiece")  # the flag with a value
    assert t2.decode_for_bleu([d.bos(), 4, 5, 6, 7, 3, 2]) == "hello worldUNKNOWNTOKENINHYP"
    hyps, refs = t.bleu_strings([[4, 5, 3, 2]], torch.tensor([[4, 5, 3, 2, 1, 1]]))
    assert (hyps, refs) == (["hello UNKNOWNTOKENINHYP"], ["hello UNKNOWNTOKENINREF"])  # an unknown word never counts as a match
    assert stats_of(hyps, refs)[0] == [1, 0, 0, 0]
    assert d.string(ids) == "he@@ llo <unk> wor@@ ld"  # the default is unchanged


def test_sentencepiece_round_trip_and_detokenisers(tmp_path):
    import logging

    import sentencepiece as spm
    text = ["the cat sat on the mat", "a dog ran to the house", "the house is on the hill", "cats and dogs run", "this is a small test"]
    corpus = tmp_path / "c.txt"
    corpus.write_text("\n".join(text * 4) + "\n")
    spm.SentencePieceTrainer.train(input=str(corpus), model_prefix=str(tmp_path / "sp"), vocab_size=48, hard_vocab_limit=False,
                                   minloglevel=2)
    bpe = D.build_bpe({"bpe": "sentencepiece", "sentencepiece_model": str(tmp_path / "sp.model")})
    pieces = sorted({p for s in text for p in bpe.encode(s).split()})
    t, d = bleu_task(pieces)
    t.bpe, t.tokenizer = bpe, B.build_detokenizer("space", logging.getLogger("t"))
    for s in text:
        ids = d.encode_line(bpe.encode(s), add_if_not_exist=False, append_eos=True)
        assert int((ids == d.unk()).sum()) == 0
        assert t.decode_for_bleu(ids) == s
    moses = B.build_detokenizer("moses", logging.getLogger("t"))  # sacremoses where it imports, else `space` with a note
    assert moses.decode("a b") in ("a b",)
    with pytest.raises(NotImplementedError, match="--eval-bleu-detok nltk"):
        B.build_detokenizer("nltk", logging.getLogger("t"))


# ---- the script's command line ------------------------------------------------------------------------------------------------
def test_the_mt_script_flag_set_parses():
    """chimera/scripts/train-en2any-MT.sh:38-64, unchanged."""
    cli = import_module("chimera-st_amd.cli")
    argv = [ROOT, "--task", "translation", "--train-subset", "train", "--valid-subset", "valid", "--save-dir", "/tmp/mt", "--max-tokens", "4096",
            "--criterion", "label_smoothed_cross_entropy", "--label-smoothing", "0.1",
            "--eval-bleu-args", '{"beam": 5, "max_len_a": 1.2, "max_len_b": 10}',
            "--eval-bleu", "--eval-bleu-detok", "moses", "--eval-bleu-remove-bpe", "--eval-bleu-bpe", "sentencepiece",
            "--eval-bleu-bpe-path", "/data/spm.model", "--eval-bleu-print-samples",
            "--best-checkpoint-metric", "bleu", "--maximize-best-checkpoint-metric",
            "--arch", "s2t_transformer_w2v2_interlingua_base", "--share-decoder-input-output-embed",
            "--w2v2-model-path", "/w2v/wav2vec_small.pt", "--encoder-layers", "6", "--encoder-embed-dim", "512", "--interlingua-length", "64",
            "--dropout", "0.1", "--optimizer", "adam", "--adam-betas", "(0.9, 0.98)", "--clip-norm", "0.0",
            "--lr", "5e-4", "--lr-scheduler", "inverse_sqrt", "--weight-decay", "0.0001", "--max-update", "100000", "--warmup-updates", "4000",
            "--fp16", "--update-freq", "8", "--num-workers", "1", "--ddp-backend", "no_c10d", "--seed", "1"]
    extra, rest = cli._extra_train_flags(argv)
    args = reg.parse_args_and_arch(rest)
    assert extra.best_checkpoint_metric == "bleu" and extra.maximize_best_checkpoint_metric
    assert args.task == "translation" and args.data == ROOT and args.max_tokens == 4096 and args.update_freq == [8]
    assert args.eval_bleu and args.eval_bleu_detok == "moses" and args.eval_bleu_remove_bpe == "@@ " and args.eval_bleu_print_samples
    assert args.eval_bleu_bpe == "sentencepiece" and args.eval_bleu_bpe_path == "/data/spm.model" and not args.eval_tokenized_bleu
    assert args.eval_bleu_args == '{"beam": 5, "max_len_a": 1.2, "max_len_b": 10}'
    assert args.source_lang is None and args.left_pad_source == "True" and args.max_source_positions == 1024
    assert args.interlingua_length == 64 and args.encoder_embed_dim == 512 and args.share_decoder_input_output_embed
    t = reg.setup_task(args)
    assert isinstance(t, tasks.TranslationTask) and (args.source_lang, args.target_lang) == ("en", "de") and args.left_pad_source is True
    assert "translation" in reg.TASK_REGISTRY


def test_a_checkpoint_without_a_task_maps_to_translation():
    """checkpoint_utils._upgrade_state_dict names `translation` for old checkpoints; the task now exists and sets up without its data."""
    cu = import_module("chimera-st_amd.checkpoint_utils")
    state = cu._upgrade_state_dict({"args": Namespace(arch="x"), "model": {}, "optimizer_history": [{"num_updates": 0}], "extra_state": {}})
    assert state["args"].task == "translation"
    state["args"].data, state["args"].synthetic_vocab_size = None, 60
    t = reg.setup_task(state["args"])
    assert isinstance(t, tasks.TranslationTask) and len(t.target_dictionary) == 60 and t.source_dictionary is t.target_dictionary
