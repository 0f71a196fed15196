"""The `language_modeling` task on the host (no GPU): the two block natives, TokenBlockDataset / MonolingualDataset and the host
collater against the fixture the reference made (tests/golden/lm_tiny/, lm_tiny.npz: tools/ref_harness/make_lm_goldens.py), the
resident route's record, the refused options, and eval-lm's aggregation."""
import ctypes
import math
import os
import shutil
from argparse import Namespace
from importlib import import_module

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, load_pkg

load_pkg()
ID = import_module("chimera-st_amd.indexed_dataset")
M = import_module("chimera-st_amd.monolingual_dataset")
D = import_module("chimera-st_amd.data")
cli = import_module("chimera-st_amd.cli")
tasks = import_module("chimera-st_amd.tasks")
reg = import_module("chimera-st_amd.registry")
criterions = import_module("chimera-st_amd.criterions")
import_module("chimera-st_amd.transformer_lm")
Dictionary = import_module("chimera-st_amd.dictionary").Dictionary

ROOT = os.path.join(GOLDEN, "lm_tiny")
MODES = ("none", "complete", "complete_doc", "eos")
BLOCK_SIZES = (7, 16)
CASES = [("train", m, b) for m in MODES for b in BLOCK_SIZES] + [("valid", m, b) for m in MODES for b in BLOCK_SIZES] + \
        [("noeos", m, b) for m in ("none", "complete") for b in BLOCK_SIZES]
PAD, EOS = 1, 2


@pytest.fixture(autouse=True)
def host_route(monkeypatch):
    """These tests state the batch on the host, also where a GPU is present."""
    monkeypatch.setenv("CST_BLOCK_COLLATE", "host")


@pytest.fixture(scope="module")
def g():
    return load_golden("lm_tiny.npz")


def task_args(mode="none", block_size=16, **over):
    a = Namespace(data=ROOT, sample_break_mode=mode, tokens_per_sample=block_size, max_target_positions=None, dataset_impl=None)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def load(split, mode="none", block_size=16, **over):
    t = tasks.LanguageModelingTask.setup_task(task_args(mode, block_size, **over))
    return t, t.load_dataset(split)


# ---- the natives --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split,mode,bs", CASES)
def test_block_natives_equal_the_reference(g, split, mode, bs):
    key = "%s/%s/%d" % (split, mode, bs)
    sizes = np.asarray(ID.MMapIndexedDataset(os.path.join(ROOT, split)).sizes)
    slices = M.token_block_slices(sizes, mode, bs, 1)
    assert slices.dtype == np.int64
    np.testing.assert_array_equal(slices, g[key + "/slice_indices"])
    np.testing.assert_array_equal(M.token_block_index(sizes, slices), g[key + "/block_to_dataset_index"])


def test_the_fixture_exercises_every_rule(g):
    sizes = np.asarray(ID.MMapIndexedDataset(os.path.join(ROOT, "train")).sizes)
    assert (sizes == 1).sum() >= 3 and (sizes == 2).any() and sizes.max() > max(BLOCK_SIZES)  # eos alone, a one-word line, a long line
    for bs in BLOCK_SIZES:
        assert (g["train/none/%d/block_to_dataset_index" % bs][:, 1] > 0).any()        # blocks that begin inside a sentence
        assert (g["train/none/%d/block_to_dataset_index" % bs][1:, 1] == 0).any()      # and at a later sentence's first token
        assert g["train/complete/%d/sizes" % bs].max() > bs                            # a sentence longer than the block
        doc, full = g["train/complete_doc/%d/slice_indices" % bs], g["train/complete/%d/slice_indices" % bs]
        assert doc[:, 1].max() <= full[:, 1].max() and (doc[1:, 0] > doc[:-1, 1]).any()  # separators belong to no block
        assert g["train/complete_doc/%d/sizes" % bs].min() > 1
    assert g["train/none/7/sizes"][-1] < 7 or g["train/none/16/sizes"][-1] < 16          # a short last block
    noeos = ID.MMapIndexedDataset(os.path.join(ROOT, "noeos"))
    assert noeos.dtype == np.int32 and all(int(noeos[i][-1]) != EOS for i in range(len(noeos)))


def test_block_natives_properties_and_bad_arguments():
    sizes = np.array([3, 1, 5, 1, 9, 2], dtype=np.int64)
    total = int(sizes.sum())
    s = M.token_block_slices(sizes, "none", 4)
    assert len(s) == math.ceil(total / 4) and s[-1].tolist() == [20, 21] and np.all(s[:-1, 1] - s[:-1, 0] == 4)
    assert M.token_block_slices(sizes, None, 4).tolist() == s.tolist()  # (None is `none`)
    np.testing.assert_array_equal(M.token_block_slices(sizes, "eos", None), np.stack([np.cumsum(sizes) - sizes, np.cumsum(sizes)], 1))
    c = M.token_block_slices(sizes, "complete", 4)
    assert c.tolist() == [[0, 4], [4, 9], [9, 10], [10, 19], [19, 21]]
    d = M.token_block_slices(sizes, "complete_doc", 4, 1)
    assert d.tolist() == [[0, 3], [4, 9], [10, 19], [19, 21]]
    assert M.token_block_slices(np.array([1, 1, 1]), "complete_doc", 4, 1).shape == (0, 2)  # nothing but separators
    np.testing.assert_array_equal(M.token_block_index(sizes, s), [[0, 0, 1], [2, 0, 2], [2, 4, 4], [4, 2, 4], [4, 6, 5], [5, 1, 5]])
    np.testing.assert_array_equal(M.token_block_index(sizes, np.array([[4, 4]])), [[2, 0, 2]])  # an empty block ends where it begins
    np.testing.assert_array_equal(M.token_block_index(sizes, np.array([[10, 12], [0, 2]])), [[4, 0, 4], [0, 0, 0]])  # not rising
    lib = import_module("chimera-st_amd.lib").load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    out = np.zeros((2, 2), dtype=np.int64)
    assert lib.cst_token_block_slices(p(sizes), len(sizes), 0, 4, 1, p(out), 2) == -3          # more blocks than the capacity
    assert lib.cst_token_block_slices(p(sizes), len(sizes), 0, 4, 1, None, 0) == 6             # the count alone
    with pytest.raises(ValueError, match="Invalid break_mode"):
        M.token_block_slices(sizes, "sentence", 4)
    with pytest.raises(ValueError):
        M.token_block_slices(sizes, "none", 0)
    with pytest.raises(ValueError):
        M.token_block_slices(np.array([3, -1]), "none", 4)
    with pytest.raises(ValueError):
        M.token_block_index(np.array([3, 0, 2]), np.array([[0, 2]]))   # an empty sentence
    with pytest.raises(ValueError):
        M.token_block_index(sizes, np.array([[0, 22]]))                # beyond the corpus


def test_a_zero_length_sentence_is_refused_when_the_split_is_loaded(tmp_path):
    ID.write_dataset(str(tmp_path / "train"), np.array([5, 6, 2, 7, 2], dtype=np.uint16), [3, 0, 2])
    shutil.copyfile(os.path.join(ROOT, "dict.txt"), str(tmp_path / "dict.txt"))
    t = tasks.LanguageModelingTask.setup_task(task_args(data=str(tmp_path)))
    with pytest.raises(ValueError, match="sentence 1 .*no token"):
        t.load_dataset("train")


# ---- datasets -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split,mode,bs", CASES)
def test_items_order_filter_and_batches(g, split, mode, bs):
    key = "%s/%s/%d" % (split, mode, bs)
    task, ds = load(split, mode, bs)
    assert ds.resident is None and len(ds) == len(g[key + "/sizes"])
    np.testing.assert_array_equal(ds.sizes, g[key + "/sizes"])
    np.testing.assert_array_equal(ds.dataset.slice_indices, g[key + "/slice_indices"])
    np.testing.assert_array_equal(ds.dataset.block_to_dataset_index, g[key + "/block_to_dataset_index"])
    items = [ds[i] for i in range(len(ds))]
    assert all(it["id"] == i and it["source"].dtype == torch.int64 and it["target"].dtype == torch.int64 for i, it in enumerate(items))
    np.testing.assert_array_equal(torch.cat([it["source"] for it in items]).numpy(), g[key + "/src_flat"])
    np.testing.assert_array_equal(torch.cat([it["target"] for it in items]).numpy(), g[key + "/tgt_flat"])
    assert [ds.num_tokens(i) for i in range(len(ds))] == [ds.size(i) for i in range(len(ds))] == g[key + "/sizes"].tolist()
    with D.numpy_seed(1):
        idx = ds.ordered_indices()
    np.testing.assert_array_equal(idx, g[key + "/ordered"])
    idx_f, ignored = ds.filter_indices_by_size(idx, int(g["meta/limit"]))
    np.testing.assert_array_equal(idx_f, g[key + "/filtered"])
    assert list(ignored) == g[key + "/ignored"].tolist()
    batches = ds.batch_by_size(idx, max_tokens=int(g["meta/max_tokens"]))
    assert [len(b) for b in batches] == g[key + "/batches/sizes"].tolist()
    assert [i for b in batches for i in b] == g[key + "/batches/flat"].tolist()
    ds.shuffle = False
    np.testing.assert_array_equal(ds.ordered_indices(), np.argsort(ds.sizes, kind="stable"))


def test_source_starts_with_the_dictionary_eos_at_a_sentence_start_only(g):
    """The one place the batch can be subtly wrong: on a corpus whose sentences do not end in eos, a block at a later sentence's first
    token still begins its source with eos, a block inside a sentence with the token before it."""
    _, ds = load("noeos", "none", 7)
    stream = np.asarray(ds.dataset.dataset.stream)
    seen = set()
    for i in range(len(ds)):
        start, off = int(ds.dataset.slice_indices[i, 0]), int(ds.dataset.block_to_dataset_index[i, 1])
        first = int(ds[i]["source"][0])
        if off == 0:
            assert first == EOS and (start == 0 or int(stream[start - 1]) != EOS)
            seen.add("later" if start else "zero")
        else:
            assert first == int(stream[start - 1]) != EOS
            seen.add("inside")
    assert {"zero", "inside"} <= seen
    _, ds = load("noeos", "complete", 7)
    assert all(int(ds[i]["source"][0]) == EOS for i in range(len(ds))) and len(ds) > 1
    np.testing.assert_array_equal(ds.dataset.blocks[:, 2], -1)
    _, ds = load("train", "none", 7)
    b = ds.dataset.blocks
    inside = ds.dataset.block_to_dataset_index[:, 1] > 0
    np.testing.assert_array_equal(b[inside, 2], b[inside, 0] - 1)
    np.testing.assert_array_equal(b[~inside, 2], -1)
    np.testing.assert_array_equal(b[:, 1], ds.sizes)


@pytest.mark.parametrize("split,mode", [("train", "none"), ("train", "eos"), ("noeos", "none")])
def test_host_collater_equals_the_reference(g, split, mode):
    key = "%s/%s/16" % (split, mode)
    task, ds = load(split, mode, 16)
    it = task.get_batch_iterator(ds, max_tokens=int(g["meta/max_tokens"]), seed=1)
    samples = list(it.next_epoch_itr(shuffle=(split == "train")))
    assert len(samples) == int(g[key + "/collated/n"])
    padded = False
    for j, s in enumerate(samples):
        k = "%s/collated/%d" % (key, j)
        np.testing.assert_array_equal(s["id"].numpy(), g[k + "/id"])
        assert s["ntokens"] == int(g[k + "/ntokens"]) and s["nsentences"] == int(g[k + "/nsentences"])
        np.testing.assert_array_equal(s["net_input"]["src_tokens"].numpy(), g[k + "/src_tokens"])
        np.testing.assert_array_equal(s["net_input"]["src_lengths"].numpy(), g[k + "/src_lengths"])
        np.testing.assert_array_equal(s["target"].numpy(), g[k + "/target"])
        assert sorted(s) == ["id", "net_input", "nsentences", "ntokens", "target"] and sorted(s["net_input"]) == ["src_lengths", "src_tokens"]
        padded = padded or bool((s["target"] == PAD).any())
        assert not (s["target"][:, 0] == PAD).any()  # right padding only
    assert padded or mode == "none"
    assert ds.collater([]) == {}


def test_record_equals_the_host_batch(g, monkeypatch):
    _, ds = load("train", "eos", 16)
    with D.numpy_seed(1):
        batches = ds.batch_by_size(ds.ordered_indices(), max_tokens=48)
    ds.resident = object()  # the record route: __getitem__ reads no token (no device is needed to build a record)
    assert ds[3] == {"id": 3}
    for b in batches:
        rec = ds.collater([ds[i] for i in b])
        host = ds.host_batch(b)
        ni = rec["net_input"]
        assert M.is_block_record(rec) and not M.is_block_record(host) and rec["target"] is None
        assert ni["block_width"] == host["target"].size(1) == host["net_input"]["src_tokens"].size(1)
        assert torch.equal(ni["src_lengths"], host["net_input"]["src_lengths"]) and ni["src_lengths"].dtype == torch.int64
        assert torch.equal(ni["block_idx"], host["id"]) and torch.equal(rec["id"], host["id"])
        assert rec["ntokens"] == host["ntokens"] == int(host["target"].ne(PAD).sum()) and rec["nsentences"] == host["nsentences"]
        assert ni["block_corpus"] is ds.resident


def test_block_collate_switch_is_validated(monkeypatch):
    _, ds = load("valid")
    for mode in ("host", "device"):
        monkeypatch.setenv("CST_BLOCK_COLLATE", mode)
        assert ds.enable_resident(budget_mb=64) in (False, True) and (mode == "device" or ds.resident is None)
    monkeypatch.setenv("CST_BLOCK_COLLATE", "gpu")
    with pytest.raises(ValueError, match="CST_BLOCK_COLLATE"):
        ds.enable_resident()
    monkeypatch.setenv("CST_BLOCK_COLLATE", "host")
    with pytest.raises(ValueError, match="outside the stream"):
        M.ResidentBlocks(np.zeros(10, np.uint16), np.array([[8, 4, -1]]), PAD, EOS)
    with pytest.raises(TypeError):
        M.ResidentBlocks(np.zeros(10, np.float32), np.array([[0, 4, -1]]), PAD, EOS)


# ---- the task's surface -------------------------------------------------------------------------------------------------------
def test_task_dictionaries_positions_and_registration():
    t, ds = load("valid", "eos", 16)
    assert t.source_dictionary is t.target_dictionary and len(t.source_dictionary) == 60
    assert t.max_positions() == 16 and tasks.LanguageModelingTask.setup_task(task_args(max_target_positions=33)).max_positions() == 33
    assert reg.TASK_REGISTRY["language_modeling"] is tasks.LanguageModelingTask
    assert reg.CRITERION_REGISTRY["cross_entropy"] is criterions.CrossEntropyCriterion
    assert t.dataset("valid") is ds
    with pytest.raises(FileNotFoundError):
        t.load_dataset("nosuchsplit")
    args = reg.parse_args_and_arch([ROOT, "--task", "language_modeling", "--arch", "transformer_lm", "--criterion", "cross_entropy",
                                    "--sample-break-mode", "complete", "--tokens-per-sample", "32", "--share-decoder-input-output-embed"])
    assert args.sample_break_mode == "complete" and args.tokens_per_sample == 32 and args.max_target_positions is None
    model = reg.setup_task(args).build_model(args)
    assert model.max_positions() == 32 and model.supported_targets == {"future"}


@pytest.mark.parametrize("over,name", [
    (dict(output_dictionary_size=40), "--output-dictionary-size"), (dict(self_target=True), "--self-target"),
    (dict(past_target=True), "--past-target"), (dict(add_bos_token=True), "--add-bos-token"),
    (dict(shorten_method="truncate"), "--shorten-method"), (dict(shorten_method="random_crop"), "--shorten-method"),
    (dict(data=ROOT + os.pathsep + ROOT), "colon-separated"), (dict(dataset_impl="lazy"), "--dataset-impl lazy"),
    (dict(dataset_impl="raw"), "--dataset-impl raw"), (dict(dataset_impl="cached"), "--dataset-impl cached")])
def test_refused_options_raise_by_name(over, name):
    with pytest.raises(NotImplementedError) as e:
        tasks.LanguageModelingTask.setup_task(task_args(**over))
    assert name in str(e.value)


def test_unsupported_target_and_break_mode_are_errors(monkeypatch):
    t, _ = load("valid")

    class SelfTargetModel:
        supported_targets = {"self"}

        @classmethod
        def build_model(cls, args, task):
            return cls()

    monkeypatch.setitem(reg.ARCH_MODEL_REGISTRY, "_lm_stub", SelfTargetModel)
    with pytest.raises(ValueError, match="Unsupported language modeling target: future"):
        t.build_model(Namespace(arch="_lm_stub"))
    with pytest.raises(ValueError, match="sample-break-mode"):
        tasks.LanguageModelingTask.setup_task(task_args(mode="sentence"))


def test_cross_entropy_criterion_surface():
    t, _ = load("valid")
    c = criterions.CrossEntropyCriterion.build_criterion(Namespace(sentence_avg=False), t)
    assert c.single_pass and c.padding_idx == PAD and not c.sentence_avg
    assert sorted(c.logging_keys()) == ["loss", "nsentences", "ntokens", "sample_size"] and c.logging_outputs_can_be_summed()
    d = c.derived_metrics({"loss": 3.0 * math.log(2) * 10, "ntokens": 10.0, "sample_size": 10.0, "nsentences": 2.0})
    assert d == {"ppl": 8.0}
    d = c.derived_metrics({"loss": 3.0 * math.log(2) * 10, "ntokens": 10.0, "sample_size": 2.0, "nsentences": 2.0})  # --sentence-avg
    assert d["ppl"] == 8.0 and abs(d["nll_loss"] - 3.0) < 1e-12


# ---- eval-lm's aggregation ----------------------------------------------------------------------------------------------------
def test_eval_lm_aggregation_bpe_merge_inf_and_count():
    d = Dictionary.load(os.path.join(ROOT, "dict.txt"))
    for w in ("ab@@", "c@@", "x"):
        d.add_symbol(w)
    a, c, x = d.index("ab@@"), d.index("c@@"), d.index("x")
    toks, n = cli.bpe_continuation_tokens(d, "@@ ")
    assert toks == {a, c} and n == 2 and cli.bpe_continuation_tokens(d, None) == (None, 0)
    tokens = [a, c, x, 5, a, EOS]
    pos = torch.tensor([-1.0, -2.0, -4.0, -0.5, -3.0, -0.25])
    s, count, merged, n_inf = cli.lm_score_stats(tokens, pos, toks)
    assert merged.tolist() == [0.0, 0.0, -7.0, -0.5, 0.0, -3.25] and n_inf == 0
    assert s == -10.75 and count == 3   # six positions, three continuation tokens moved on
    s, count, merged, n_inf = cli.lm_score_stats(tokens, pos, None)
    assert s == float(pos.sum()) and count == 6 and torch.equal(merged, pos)
    # a continuation token in the LAST place has nothing to move onto: counted as it is
    s, count, _, _ = cli.lm_score_stats([5, a], torch.tensor([-1.0, -2.0]), toks)
    assert (s, count) == (-3.0, 2)
    # infinite scores are dropped from the sum and from the count; a continuation's -inf moves on first
    s, count, merged, n_inf = cli.lm_score_stats([5, 6, 7], torch.tensor([-1.0, float("-inf"), -2.0]), None)
    assert (s, count, n_inf) == (-3.0, 2, 1)
    s, count, merged, n_inf = cli.lm_score_stats([a, x, 7], torch.tensor([float("-inf"), -1.0, -2.0]), toks)
    assert (s, count, n_inf) == (-2.0, 1, 1) and merged[0] == 0
    s, count, _, n_inf = cli.lm_score_stats([5, 6], torch.tensor([float("inf"), -1.5]), None)
    assert (s, count, n_inf) == (-1.5, 1, 1)
    assert pos.tolist() == [-1.0, -2.0, -4.0, -0.5, -3.0, -0.25]  # the caller's scores are not written


def test_eval_lm_fixture_totals_follow_the_formula(g):
    for mode in ("none", "eos"):
        k = "eval_lm/valid/%s" % mode
        flat, sizes = g[k + "/pos_flat"], g[k + "/pos_sizes"]
        s = c = 0
        for chunk in np.split(flat, np.cumsum(sizes)[:-1]):
            a, b, _, _ = cli.lm_score_stats([5] * len(chunk), torch.from_numpy(chunk), None)
            s, c = s + a, c + b
        assert c == int(g[k + "/count"]) == int(np.asarray(ID.MMapIndexedDataset(os.path.join(ROOT, "valid")).sizes).sum())
        assert abs(s - float(g[k + "/score_sum"])) < 1e-3 and abs(-s / c / math.log(2) - float(g[k + "/loss"])) < 1e-5


def test_eval_lm_refusals_by_name():
    p = cli.eval_lm_parser()
    with pytest.raises(NotImplementedError, match="--context-window"):
        cli.check_eval_lm_args(p.parse_args([ROOT, "--path", "x.pt", "--context-window", "4"]))
    with pytest.raises(NotImplementedError, match="sentencepiece"):
        cli.check_eval_lm_args(p.parse_args([ROOT, "--path", "x.pt", "--post-process", "sentencepiece"]))
    a = cli.check_eval_lm_args(p.parse_args([ROOT, "--path", "x.pt", "--softmax-batch", "1024", "--remove-bpe", "--gen-subset", "valid",
                                             "--batch-size", "3", "--output-word-probs", "--output-word-stats"]))
    assert a.post_process == "@@ " and a.batch_size == 3 and a.softmax_batch == 1024 and a.output_word_probs and a.output_word_stats


def test_generate_refuses_a_language_model_checkpoint_by_name(tmp_path):
    cu = import_module("chimera-st_amd.checkpoint_utils")
    args = reg.parse_args_and_arch([ROOT, "--task", "language_modeling", "--arch", "transformer_lm", "--criterion", "cross_entropy",
                                    "--decoder-layers", "1", "--decoder-embed-dim", "16", "--decoder-ffn-embed-dim", "16",
                                    "--decoder-attention-heads", "2", "--tokens-per-sample", "16", "--share-decoder-input-output-embed"])
    args.no_save_optimizer_state = True
    model = reg.setup_task(args).build_model(args)
    path = str(tmp_path / "lm.pt")
    cu.save_state(path, args, model.state_dict(), None, None, 0)
    assert cu.load_language_model(path, Dictionary.load(os.path.join(ROOT, "dict.txt"))).max_positions() == 16  # what --lm-path does with it
    with pytest.raises(NotImplementedError, match="language_modeling"):
        cli.generate_main([ROOT, "--path", path])
