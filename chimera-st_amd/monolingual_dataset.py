"""Monolingual text of the `language_modeling` task — mirror of
  fairseq/data/token_block_dataset.py        TokenBlockDataset :11-168 (include_targets=True, the "future" target only)
  fairseq/data/token_block_utils_fast.pyx    the block cuts and their sentence index -> cst_token_block_slices / cst_token_block_index
  fairseq/data/monolingual_dataset.py        collate :12-53, MonolingualDataset :56-230
over the binarised corpora indexed_dataset.py reads.

A block is a run [start, end) of the split's ONE token stream; its target is that run, its source the run shifted right by one: the
token before the block when the block begins inside a sentence, the DICTIONARY's eos when it begins at a sentence's first token
(token_block_dataset.py:137-138 — not the previous sentence's last token: the two differ on a corpus whose sentences do not end in eos).

Two routes build a batch, as for the translation task:
  * host: `collater` — per-block slices, the two right-padded tensors.  The CPU-testable statement of the batch, and the route of a
    corpus that is not device-resident (CST_BLOCK_COLLATE=host, or larger than CST_RESIDENT_CORPUS_MB).
  * resident: the stream and the block table (start, length, prev) live on the device (ResidentBlocks, uploaded once, on first use,
    from the trainer's thread); the collater builds a RECORD only — the block indices in row order, the width, the lengths and token
    count from the host-side sizes — touching no token and making no HIP call, and `ResidentBlocks.materialize` (called by
    Trainer._prepare_sample / eval_lm_main) copies the index vector and launches cst_collate_blocks on the current stream.

Not built (refused by name in tasks.LanguageModelingTask): self / past targets, --add-bos-token, --output-dictionary-size."""
import ctypes
import logging
import os

import numpy as np
import torch

from .language_pair_dataset import _TOK_CODE, ResidentPairs, collate_tokens, default_resident_budget_mb

logger = logging.getLogger(__name__)

BREAK_MODES = {"none": 0, "complete": 1, "complete_doc": 2, "eos": 3}  # include/cst.h: cst_break_mode


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def token_block_slices(sizes, break_mode, block_size, document_sep_len=1):
    """int64 [n_blocks, 2]: (first stream element, one past the last) of every block (_get_slice_indices_fast)."""
    from . import lib as L
    break_mode = "none" if break_mode is None else str(break_mode)
    if break_mode not in BREAK_MODES:
        raise ValueError("Invalid break_mode: " + break_mode)
    sizes = np.ascontiguousarray(sizes, dtype=np.int64)
    block_size = 0 if block_size is None else int(block_size)  # (`eos` does not read it)
    lib = L.load()
    n = lib.cst_token_block_slices(_p(sizes), len(sizes), BREAK_MODES[break_mode], block_size, int(document_sep_len), None, 0)
    if n < 0:
        raise ValueError(lib.cst_last_error().decode())
    out = np.zeros((n, 2), dtype=np.int64)
    if n and lib.cst_token_block_slices(_p(sizes), len(sizes), BREAK_MODES[break_mode], block_size, int(document_sep_len), _p(out), n) != n:
        raise ValueError(lib.cst_last_error().decode())
    return out


def token_block_index(sizes, slices):
    """int64 [n_blocks, 3]: per block (first sentence, offset inside it, last sentence) (_get_block_to_dataset_index_fast)."""
    from . import lib as L
    sizes = np.ascontiguousarray(sizes, dtype=np.int64)
    slices = np.ascontiguousarray(slices, dtype=np.int64)
    out = np.zeros((len(slices), 3), dtype=np.int64)
    lib = L.load()
    if lib.cst_token_block_index(_p(sizes), len(sizes), _p(slices), len(slices), _p(out)) != 0:
        raise ValueError(lib.cst_last_error().decode())
    return out


class TokenBlockDataset(torch.utils.data.Dataset):
    """token_block_dataset.py:11-168 with include_targets=True, over an MMapIndexedDataset (`stream`, `offsets`, `sizes`).  Items
    are (source, target) int64 tensors; `blocks` is the table the device route uploads."""

    def __init__(self, dataset, sizes, block_size, pad, eos, break_mode=None, include_targets=True, document_sep_len=1):
        if not include_targets:
            raise NotImplementedError("TokenBlockDataset without targets is not built: the language_modeling task always asks for them")
        if not hasattr(dataset, "stream") or not hasattr(dataset, "offsets"):
            raise TypeError("TokenBlockDataset reads a binarised corpus (indexed_dataset.MMapIndexedDataset)")
        sizes = np.asarray(sizes).astype(np.int64)
        assert len(dataset) == len(sizes)
        assert len(dataset) > 0
        if np.any(sizes < 1):  # (the reference's sentence searcher asserts on it)
            raise ValueError("sentence %d of %s has no token: a binarised sentence holds at least its eos"
                             % (int(np.argmax(sizes < 1)), getattr(dataset, "prefix", "the corpus")))
        self.dataset, self.pad, self.eos = dataset, int(pad), int(eos)
        self.break_mode = "none" if break_mode is None else str(break_mode)
        self.slice_indices = token_block_slices(sizes, self.break_mode, block_size, document_sep_len)
        self.sizes = self.slice_indices[:, 1] - self.slice_indices[:, 0]
        self.block_to_dataset_index = token_block_index(sizes, self.slice_indices)

    @property
    def blocks(self):
        """int64 [n_blocks, 3] = (start element, length, prev): prev = start - 1 inside a sentence, -1 at a sentence's first token."""
        start = self.slice_indices[:, 0]
        prev = np.where(self.block_to_dataset_index[:, 1] > 0, start - 1, -1)
        return np.ascontiguousarray(np.stack([start, self.sizes, prev], axis=1), dtype=np.int64)

    def __len__(self):
        return len(self.slice_indices)

    def __getitem__(self, index):
        s, e = (int(v) for v in self.slice_indices[index])
        stream = self.dataset.stream

        def run(a, b):
            return torch.from_numpy(np.asarray(stream[a:b]).astype(np.int64))

        target = run(s, e)
        if self.block_to_dataset_index[index, 1] == 0:
            source = torch.cat([target.new([self.eos]), run(s, max(e - 1, s))])
        else:
            source = run(s - 1, e - 1)
        return source, target


def collate(samples, pad_idx, eos_idx):
    """monolingual_dataset.py:12-53 (one target)."""
    if len(samples) == 0:
        return {}
    return {"id": torch.LongTensor([s["id"] for s in samples]), "nsentences": len(samples),
            "ntokens": sum(len(s["source"]) for s in samples),
            "net_input": {"src_tokens": collate_tokens([s["source"] for s in samples], pad_idx, eos_idx, left_pad=False),
                          "src_lengths": torch.LongTensor([s["source"].numel() for s in samples])},
            "target": collate_tokens([s["target"] for s in samples], pad_idx, eos_idx, left_pad=False)}


# --------------------------------------------------------------------------------------------------------------------
class ResidentBlocks:
    """A split's token stream (stored dtype) and its block table on the device, and the batch assembly over them."""
    RING = ResidentPairs.RING
    _index_to_device = ResidentPairs._index_to_device  # the pinned index ring of the pair route, unchanged

    def __init__(self, stream, blocks, pad, eos):
        stream = np.asarray(stream)
        if stream.dtype not in _TOK_CODE:
            raise TypeError("the token stream must be uint8 / uint16 / int32 / int64, got %s" % stream.dtype)
        blocks = np.ascontiguousarray(blocks, dtype=np.int64)
        if blocks.ndim != 2 or blocks.shape[1] != 3 or len(blocks) < 1:
            raise ValueError("blocks must be int64 [n_blocks, 3] with at least one block, got %s" % (blocks.shape,))
        start, length, prev = blocks[:, 0], blocks[:, 1], blocks[:, 2]
        if np.any(start < 0) or np.any(length < 0) or np.any(start + length > len(stream)) or np.any(prev >= len(stream)):
            raise ValueError("a block lies outside the stream of %d tokens" % len(stream))
        self.tok_dtype = _TOK_CODE[stream.dtype]
        self._host = (stream, blocks)
        self.pad, self.eos = int(pad), int(eos)
        self._dev = None
        self._slots, self._events, self._next = None, None, 0

    @property
    def nbytes(self):
        return sum(a.nbytes for a in self._host)

    def _upload(self, device):
        stream, blocks = self._host
        tok = torch.from_numpy(np.array(stream, copy=True).reshape(-1).view(np.uint8)).to(device) if stream.size else \
            torch.zeros(8, dtype=torch.uint8, device=device)
        self._dev = (tok, torch.from_numpy(blocks.copy()).to(device))
        self._device = device

    def collate(self, idx, T, device="cuda", out=None):
        """(src_tokens, src_lengths, target) of the blocks `idx` (host int64 tensor, row order), width T."""
        from . import kernels as K
        if self._dev is None:
            self._upload(torch.device(device))
        tok, blocks = self._dev
        st, sl, target, _ = K.collate_blocks(tok, self.tok_dtype, blocks, self._index_to_device(idx), T, self.pad, self.eos, out=out)
        return st, sl, target

    def materialize(self, sample, device="cuda"):
        """The collater's record -> the batch the host collater would have built, on the device."""
        ni = sample["net_input"]
        st, sl, target = self.collate(ni["block_idx"], ni["block_width"], device)
        return {"id": sample["id"], "nsentences": sample["nsentences"], "ntokens": sample["ntokens"],
                "net_input": {"src_tokens": st, "src_lengths": sl}, "target": target}


def is_block_record(sample):
    ni = sample.get("net_input") if isinstance(sample, dict) else None
    return bool(ni) and "block_idx" in ni


# --------------------------------------------------------------------------------------------------------------------
class MonolingualDataset(torch.utils.data.Dataset):
    """monolingual_dataset.py:56-230 over a TokenBlockDataset, targets = ["future"], one vocabulary."""

    def __init__(self, dataset, sizes, vocab, shuffle=True):
        self.dataset, self.sizes, self.vocab, self.shuffle = dataset, np.array(sizes), vocab, shuffle
        self.resident = None  # a ResidentBlocks once enable_resident() has decided for the device route

    # ---- the resident route -----------------------------------------------------------------------------------------
    def enable_resident(self, budget_mb=None):
        """Decide the route of this split (call from the trainer's thread, before batches are drawn): resident unless
        CST_BLOCK_COLLATE=host, no GPU, or the stream exceeds the budget.  Nothing is uploaded here."""
        self.resident = None
        mode = os.environ.get("CST_BLOCK_COLLATE", "device")
        if mode not in ("host", "device"):
            raise ValueError("CST_BLOCK_COLLATE must be `host` or `device`, got %r" % mode)
        if mode == "host" or not torch.cuda.is_available() or len(self.dataset) == 0:
            return False
        blocks = ResidentBlocks(self.dataset.dataset.stream, self.dataset.blocks, self.vocab.pad(), self.vocab.eos())
        budget = default_resident_budget_mb() if budget_mb is None else budget_mb
        if blocks.nbytes > budget * 2 ** 20:
            logger.info("corpus of %.1f MB exceeds the resident budget of %.1f MB (CST_RESIDENT_CORPUS_MB): host batch assembly",
                        blocks.nbytes / 2 ** 20, budget)
            return False
        self.resident = blocks
        return True

    def __getitem__(self, index):
        if self.resident is not None:
            return {"id": index}  # the record route reads no token
        return self.item(index)

    def item(self, index):
        """The block's (source, target), whatever the route."""
        source, target = self.dataset[index]
        return {"id": index, "source": source, "target": target}

    def __len__(self):
        return len(self.dataset)

    def collater(self, samples):
        if len(samples) == 0:
            return {}
        if "source" not in samples[0]:
            return self.record([s["id"] for s in samples])
        return collate(samples, self.vocab.pad(), self.vocab.eos())

    def host_batch(self, indices):
        """The host collater's batch of the blocks `indices` (the reference batch of either route)."""
        return collate([self.item(int(i)) for i in indices], self.vocab.pad(), self.vocab.eos())

    def record(self, indices):
        """What the resident route needs of a batch, from the host-side sizes alone: the block indices in the collater's row order
        (the given one: this collater does not sort), the width, the lengths and the token count."""
        ids = torch.LongTensor(indices)
        lengths = torch.from_numpy(self.sizes[ids.numpy()].astype(np.int64))
        return {"id": ids, "nsentences": len(indices), "ntokens": int(lengths.sum()),
                "net_input": {"block_idx": ids, "block_width": int(lengths.max()), "block_corpus": self.resident, "src_lengths": lengths},
                "target": None}

    # ---- sizes, order, filter, batches ------------------------------------------------------------------------------
    def num_tokens(self, index):
        return self.sizes[index]

    def size(self, index):
        return self.sizes[index]

    def ordered_indices(self):
        """:215-223 — by size; equal sizes in the order of a random permutation's values (under the caller's numpy_seed) when
        shuffling, of the indices otherwise."""
        order = [np.random.permutation(len(self)) if self.shuffle else np.arange(len(self))]
        order.append(self.sizes)
        return np.lexsort(order)

    def filter_indices_by_size(self, indices, max_sizes):
        """fairseq_dataset.py filter_indices_by_size with one size per item."""
        if max_sizes is None:
            return indices, []
        if not isinstance(max_sizes, (int, float)):
            max_sizes = min(m for m in max_sizes if m is not None)
        indices = np.asarray(indices, dtype=np.int64)
        bad = self.sizes[indices] > max_sizes
        return indices[~bad], indices[bad].tolist()

    def batch_by_size(self, indices, max_tokens=None, max_sentences=None, required_batch_size_multiple=1):
        from . import data as D
        return D.batch_by_size(indices, None, max_tokens, max_sentences, required_batch_size_multiple,
                               sizes=self.sizes[np.asarray(indices, dtype=np.int64)])


class PromptDataset(torch.utils.data.Dataset):
    """The inference dataset of the `language_modeling` task (language_modeling.py:246-289: TokenBlockDataset in "eos" mode, eos stripped,
    eos prepended; NestedDictionaryDataset with sizes = [src_lengths]) over typed prompts.  src_tokens: one int64 tensor per prompt as
    encode_line returns it (its final eos included), src_lengths: their lengths.  A batch is {"id", "net_input": {"src_tokens":
    [B, 1 + longest prompt] = eos + prompt, right-padded, "src_lengths"}, "target": prompt + pad, right-padded}, rows in the given order
    (this collater does not sort, and the items keep input order: fairseq_dataset.py ordered_indices)."""

    def __init__(self, src_tokens, src_lengths, vocab):
        assert len(src_tokens) == len(src_lengths)
        pad, eos = vocab.pad(), vocab.eos()
        self.vocab = vocab
        self.prompts = [torch.as_tensor(t, dtype=torch.long) for t in src_tokens]
        self.prompts = [t[t.ne(eos)] for t in self.prompts]  # (StripTokenDataset: every eos, not just the last)
        self.sizes = np.array(src_lengths, dtype=np.int64)
        self.pad, self.eos = pad, eos

    def __len__(self):
        return len(self.prompts)

    def __getitem__(self, index):
        p = self.prompts[index]
        return {"id": index, "source": torch.cat([p.new_tensor([self.eos]), p]), "target": torch.cat([p, p.new_tensor([self.pad])])}

    def collater(self, samples):
        if len(samples) == 0:
            return {}
        src = [s["source"] for s in samples]
        return {"id": torch.tensor([s["id"] for s in samples]),
                "net_input": {"src_tokens": collate_tokens(src, self.pad, self.eos, left_pad=False),
                              "src_lengths": torch.LongTensor([s.numel() for s in src])},
                "target": collate_tokens([s["target"] for s in samples], self.pad, self.eos, left_pad=False)}

    def num_tokens(self, index):
        return self.sizes[index]

    def size(self, index):
        return self.sizes[index]

    def ordered_indices(self):
        return np.arange(len(self), dtype=np.int64)

    filter_indices_by_size = MonolingualDataset.filter_indices_by_size
    batch_by_size = MonolingualDataset.batch_by_size
