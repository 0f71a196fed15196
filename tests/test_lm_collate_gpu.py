"""cst_collate_blocks on a real MI355X: one launch against the host collater of monolingual_dataset.py, bit for bit (integers, no
tolerance), every word written; the fixture's batches of `none` and `eos` through record() -> materialize()."""
import ctypes
import os
from argparse import Namespace
from importlib import import_module

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, load_pkg

pytestmark = pytest.mark.gpu

ROOT = os.path.join(GOLDEN, "lm_tiny")
PAD, EOS = 1, 2
SENTINEL = -7777
DTYPES = [np.uint8, np.uint16, np.int32, np.int64]
# sentence lengths: odd ones first, so that later uint16 sentences start on odd element offsets; none of the sentences ends in eos
SENT_LENS = [3, 1, 9, 2, 17, 5, 1, 4, 6]     # 48 tokens: blocks of 7 -> six full blocks and a short last one of 6
BLOCK = 7


def mods():
    load_pkg()
    return import_module("chimera-st_amd.monolingual_dataset"), import_module("chimera-st_amd.kernels"), import_module("chimera-st_amd.lib")


class Corpus:
    """What TokenBlockDataset reads of an MMapIndexedDataset."""

    def __init__(self, sents):
        self.stream = np.concatenate(sents)
        self.sizes = np.array([len(s) for s in sents], dtype=np.int32)
        self.offsets = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)

    def __len__(self):
        return len(self.sizes)


class Vocab:
    def pad(self):
        return PAD

    def eos(self):
        return EOS


def dataset(dtype, mode="none", block=BLOCK, seed=3):
    M, _, _ = mods()
    r = np.random.RandomState(seed)
    hi = 250 if dtype == np.uint8 else 60000
    corpus = Corpus([r.randint(4, hi, size=n).astype(dtype) for n in SENT_LENS])  # (no eos anywhere in the stream)
    tb = M.TokenBlockDataset(corpus, corpus.sizes, block, PAD, EOS, break_mode=mode)
    ds = M.MonolingualDataset(tb, tb.sizes, Vocab(), shuffle=False)
    return ds, M.ResidentBlocks(corpus.stream, tb.blocks, PAD, EOS)


def host_rows(ds, idx, T):
    """The host collater's batch of the blocks `idx` at width T: rows longer than T are cut, an index outside the blocks is a pad row."""
    src = torch.full((len(idx), T), PAD, dtype=torch.int64)
    tgt = torch.full((len(idx), T), PAD, dtype=torch.int64)
    lens = torch.zeros(len(idx), dtype=torch.int64)
    for b, i in enumerate(idx):
        if 0 <= i < len(ds):
            it = ds.item(i)
            n = min(len(it["target"]), T)
            src[b, :n], tgt[b, :n], lens[b] = it["source"][:n], it["target"][:n], n
    return src, lens, tgt


def check(rb, ds, idx, T):
    src, lens, tgt = host_rows(ds, idx, T)
    B = len(idx)
    if all(0 <= i < len(ds) for i in idx) and T == max(int(ds.sizes[i]) for i in idx):  # the collater's own width: its own batch
        host = ds.host_batch(idx)
        assert torch.equal(host["net_input"]["src_tokens"], src) and torch.equal(host["target"], tgt)
        assert torch.equal(host["net_input"]["src_lengths"], lens)
    out = torch.full((2 * B * T + B,), SENTINEL, dtype=torch.int64, device="cuda")
    st, sl, target = rb.collate(torch.tensor(idx, dtype=torch.int64), T, out=out)
    torch.cuda.synchronize()
    assert int((out == SENTINEL).sum()) == 0  # every word written
    assert st.dtype == sl.dtype == target.dtype == torch.int64 and st.shape == target.shape == (B, T) and sl.shape == (B,)
    assert torch.equal(st.cpu(), src), (idx, T)
    assert torch.equal(target.cpu(), tgt), (idx, T)
    assert torch.equal(sl.cpu(), lens), (idx, T)


@pytest.mark.parametrize("T", [1, 2, 7, 13])
@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("dtype", DTYPES)
def test_collate_blocks_equals_the_host_collater(dtype, B, T):
    ds, rb = dataset(dtype)
    n = len(ds)
    assert n == 7 and int(ds.sizes[-1]) == 6
    for start in range(0, n, B):  # every block takes its turn, at every row position modulo B
        check(rb, ds, [(start + k * 3) % n for k in range(B)], T)
    if dtype == np.uint16:
        assert any(int(s) % 2 for s in ds.dataset.slice_indices[:, 0])  # blocks that start on odd element offsets


def test_collate_blocks_named_cases():
    ds, rb = dataset(np.uint16)
    tb = ds.dataset
    stream = np.asarray(tb.dataset.stream).astype(np.int64)
    blocks = tb.blocks
    off = tb.block_to_dataset_index[:, 1]
    # a block at stream element 0: eos first
    assert blocks[0].tolist() == [0, 7, -1]
    check(rb, ds, [0], 7)
    assert int(rb.collate(torch.tensor([0]), 7)[0][0, 0]) == EOS
    # a block beginning inside a sentence: the token before it
    inside = int(np.nonzero(off > 0)[0][0])
    assert blocks[inside, 2] == blocks[inside, 0] - 1
    check(rb, ds, [inside, 0], 7)
    assert int(rb.collate(torch.tensor([inside]), 7)[0][0, 0]) == stream[blocks[inside, 0] - 1] != EOS
    # a block beginning at a later sentence's first token of a corpus without eos: eos although stream[start - 1] is not eos
    later = [i for i in range(1, len(ds)) if off[i] == 0]
    assert later and all(stream[blocks[i, 0] - 1] != EOS and blocks[i, 2] == -1 for i in later)
    check(rb, ds, later + [inside], 7)
    assert int(rb.collate(torch.tensor(later[:1]), 7)[0][0, 0]) == EOS
    ds_c, rb_c = dataset(np.int32, mode="complete")  # every block of `complete` begins at a sentence's first token
    assert len(ds_c) > 3 and bool((ds_c.dataset.blocks[:, 2] == -1).all())
    check(rb_c, ds_c, list(range(len(ds_c))), int(ds_c.sizes.max()))
    ds_e, rb_e = dataset(np.uint8, mode="eos")
    check(rb_e, ds_e, [4, 1, 6, 0], 17)
    # a short last block beside full ones
    check(rb, ds, [len(ds) - 1, 1], 7)
    check(rb, ds, [len(ds) - 1], 6)
    # T larger than every block
    check(rb, ds, [2, 6, 0], 13)
    # T smaller than a block: truncation, lengths = T
    check(rb, ds, [2, 6, 0], 4)
    assert rb.collate(torch.tensor([2, 6, 0]), 4)[1].tolist() == [4, 4, 4]
    # an odd total word count (the lone tail store) and an even one (no tail)
    assert (2 * 3 * 7 + 3) % 2 == 1 and (2 * 2 * 7 + 2) % 2 == 0
    check(rb, ds, [1, 2, 3], 7)
    check(rb, ds, [1, 2], 7)
    # an out-of-range index: an all-pad row of length 0, the rows beside it untouched by it
    check(rb, ds, [1, len(ds), -1, 5, 2 ** 40], 7)
    st, sl, target = rb.collate(torch.tensor([len(ds), -1]), 7)
    assert sl.tolist() == [0, 0] and bool((st == PAD).all()) and bool((target == PAD).all())
    # more than one workgroup (512 words each): 40 rows of 13
    check(rb, ds, [i % len(ds) for i in range(40)], 13)
    # bit-reproducible
    idx = torch.tensor([3, 0, 6, 2, 5])
    assert torch.equal(torch.cat([t.reshape(-1) for t in rb.collate(idx, 7)]), torch.cat([t.reshape(-1) for t in rb.collate(idx, 7)]))


def test_collate_blocks_guards_its_arguments():
    M, K, L = mods()
    ds, rb = dataset(np.uint16)
    rb.collate(torch.tensor([0]), 7)  # uploads
    tok, blocks = rb._dev
    idx = torch.tensor([0, 1, 2], device="cuda")
    BAD_ARG = -1
    lib = L.load()

    def raw(tok_p, dt, blocks_p, N, idx_p, B, T, out_p):
        return lib.cst_collate_blocks(tok_p, dt, blocks_p, N, idx_p, B, T, PAD, EOS, out_p, L.stream_ptr())

    out = torch.full((2 * 3 * 7 + 3 + 2,), SENTINEL, dtype=torch.int64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    good = (p(tok), rb.tok_dtype, p(blocks), blocks.size(0), p(idx), 3, 7, p(out))
    assert raw(*good) == 0
    for pos in (0, 2, 4, 7):  # a null operand
        a = list(good)
        a[pos] = None
        assert raw(*a) == BAD_ARG, pos
    for dt in (-1, 4, 9):
        assert raw(p(tok), dt, p(blocks), blocks.size(0), p(idx), 3, 7, p(out)) == BAD_ARG
    assert raw(p(tok), rb.tok_dtype, p(blocks), 0, p(idx), 3, 7, p(out)) == BAD_ARG        # n_blocks < 1
    assert raw(p(tok), rb.tok_dtype, p(blocks), blocks.size(0), p(idx), 0, 7, p(out)) == BAD_ARG   # B < 1
    assert raw(p(tok), rb.tok_dtype, p(blocks), blocks.size(0), p(idx), 3, 0, p(out)) == BAD_ARG   # T < 1
    assert raw(p(tok), rb.tok_dtype, p(blocks), blocks.size(0), p(idx), 3, -7, p(out)) == BAD_ARG
    assert raw(p(tok), rb.tok_dtype, p(blocks), blocks.size(0), p(idx), 1, 2 ** 30, p(out)) == BAD_ARG   # B (2T + 1) = 2^31 + 1
    assert raw(p(tok), rb.tok_dtype, p(blocks), blocks.size(0), p(idx), 2 ** 31, 1, p(out)) == BAD_ARG
    assert raw(p(tok), rb.tok_dtype, p(blocks), blocks.size(0), p(idx), 3, 7, ctypes.c_void_p(out.data_ptr() + 8)) == BAD_ARG  # misaligned out
    assert raw(ctypes.c_void_p(tok.data_ptr() + 1), rb.tok_dtype, p(blocks), blocks.size(0), p(idx), 3, 7, p(out)) == BAD_ARG  # misaligned stream
    torch.cuda.synchronize()
    assert int((out[45:] == SENTINEL).sum()) == 2  # (the one good call wrote its 45 words and nothing else; the refused ones nothing)
    with pytest.raises(RuntimeError, match="bad token dtype"):
        K.collate_blocks(tok, 9, blocks, idx, 7, PAD, EOS)
    with pytest.raises(RuntimeError, match="bad shape"):
        K.collate_blocks(tok, rb.tok_dtype, blocks, idx, 0, PAD, EOS)
    with pytest.raises(ValueError, match="out must be"):
        K.collate_blocks(tok, rb.tok_dtype, blocks, idx, 7, PAD, EOS, out=torch.empty(5, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match=r"\[n_blocks, 3\]"):
        K.collate_blocks(tok, rb.tok_dtype, blocks.reshape(-1), idx, 7, PAD, EOS)
    with pytest.raises(ValueError, match="bytes"):
        K.collate_blocks(tok.view(torch.int16), rb.tok_dtype, blocks, idx, 7, PAD, EOS)


@pytest.mark.parametrize("split,mode", [("train", "none"), ("train", "eos"), ("noeos", "none")])
def test_fixture_batches_through_record_and_materialize(split, mode, monkeypatch):
    load_pkg()
    tasks = import_module("chimera-st_amd.tasks")
    M, _, _ = mods()
    g = load_golden("lm_tiny.npz")
    monkeypatch.setenv("CST_BLOCK_COLLATE", "device")
    monkeypatch.setenv("CST_RESIDENT_CORPUS_MB", "64")
    t = tasks.LanguageModelingTask.setup_task(Namespace(data=ROOT, sample_break_mode=mode, tokens_per_sample=16, max_target_positions=None,
                                                        dataset_impl=None))
    ds = t.load_dataset(split)
    assert ds.resident is not None and ds.resident.tok_dtype == (2 if split == "noeos" else 1)
    key = "%s/%s/16" % (split, mode)
    it = t.get_batch_iterator(ds, max_tokens=int(g["meta/max_tokens"]), seed=1)
    samples = list(it.next_epoch_itr(shuffle=(split == "train")))
    assert len(samples) == int(g[key + "/collated/n"])
    for j, rec in enumerate(samples):
        k = "%s/collated/%d" % (key, j)
        assert M.is_block_record(rec) and rec["target"] is None
        dev = rec["net_input"]["block_corpus"].materialize(rec)
        np.testing.assert_array_equal(dev["id"].numpy(), g[k + "/id"])
        assert dev["ntokens"] == int(g[k + "/ntokens"]) and dev["nsentences"] == int(g[k + "/nsentences"])
        assert dev["target"].is_cuda and dev["net_input"]["src_tokens"].is_cuda
        np.testing.assert_array_equal(dev["net_input"]["src_tokens"].cpu().numpy(), g[k + "/src_tokens"])
        np.testing.assert_array_equal(dev["net_input"]["src_lengths"].cpu().numpy(), g[k + "/src_lengths"])
        np.testing.assert_array_equal(dev["target"].cpu().numpy(), g[k + "/target"])
    # a corpus beyond the budget, or the switch, takes the host route
    assert ds.enable_resident(budget_mb=1e-6) is False and ds.resident is None
    monkeypatch.setenv("CST_BLOCK_COLLATE", "host")
    assert ds.enable_resident() is False and "source" in ds[0]
