"""Parallel text of the `translation` task — mirror of
  fairseq/tasks/translation.py               load_langpair_dataset :34-161
  fairseq/data/language_pair_dataset.py      collate :16-165, LanguagePairDataset :168-470
  fairseq/data/data_utils.py                 infer_language_pair :24-31, collate_tokens :34-64 (pad_to_multiple :46-47),
                                             filter_paired_dataset_indices_by_size :240-273
over the binarised corpora indexed_dataset.py reads.

Two routes build a batch:
  * host: `collater` — per-sentence slices, the three padded tensors, pinned and copied by the trainer.  The CPU-testable statement of
    the batch, and the route of a corpus that is not device-resident (CST_PAIR_COLLATE=host, or larger than CST_RESIDENT_CORPUS_MB).
  * resident: the split's two token streams and their offsets live on the device (ResidentPairs, uploaded once, on first use, from the
    trainer's thread); the collater then builds a RECORD only — the sentence indices in the batch's row order, the widths, the lengths
    and token count from the host-side sizes — touching no token and making no HIP call, and `ResidentPairs.materialize` (called by
    Trainer._prepare_sample / generate_main) copies the index vector and launches cst_collate_pairs on the current stream."""
import logging
import os

import numpy as np
import torch

from . import indexed_dataset as ID

logger = logging.getLogger(__name__)


def infer_language_pair(path):
    """data_utils.py:24-31: the pair of the first `<split>.<l1>-<l2>.*` file name in `path` (directory order, as the reference)."""
    for filename in os.listdir(path):
        parts = filename.split(".")
        if len(parts) >= 3 and len(parts[1].split("-")) == 2:
            return parts[1].split("-")
    return None, None


def padded_width(size, pad_to_multiple=1):
    """data_utils.py:46-47."""
    if pad_to_multiple != 1 and size % pad_to_multiple != 0:
        size = int(((size - 0.1) // pad_to_multiple + 1) * pad_to_multiple)
    return size


def collate_tokens(values, pad_idx, eos_idx=None, left_pad=False, move_eos_to_beginning=False, pad_to_multiple=1):
    """data_utils.py:34-64."""
    size = padded_width(max(v.size(0) for v in values), pad_to_multiple)
    res = values[0].new(len(values), size).fill_(pad_idx)
    for i, v in enumerate(values):
        dst = res[i][size - len(v):] if left_pad else res[i][:len(v)]
        if move_eos_to_beginning:
            dst[0] = v[-1] if eos_idx is None else eos_idx
            dst[1:] = v[:-1]
        else:
            dst.copy_(v)
    return res


def collate(samples, pad_idx, eos_idx, left_pad_source=True, left_pad_target=False, input_feeding=True, pad_to_multiple=1):
    """language_pair_dataset.py:16-126 (no alignments, no constraints)."""
    if len(samples) == 0:
        return {}

    def merge(key, left_pad, move_eos_to_beginning=False):
        return collate_tokens([s[key] for s in samples], pad_idx, eos_idx, left_pad, move_eos_to_beginning, pad_to_multiple)

    ids = torch.LongTensor([s["id"] for s in samples])
    src_tokens = merge("source", left_pad_source)
    src_lengths = torch.LongTensor([s["source"].ne(pad_idx).long().sum() for s in samples])
    src_lengths, sort_order = src_lengths.sort(descending=True)  # sort by descending source length
    ids = ids.index_select(0, sort_order)
    src_tokens = src_tokens.index_select(0, sort_order)
    prev_output_tokens = target = None
    if samples[0].get("target", None) is not None:
        target = merge("target", left_pad_target).index_select(0, sort_order)
        tgt_lengths = torch.LongTensor([s["target"].ne(pad_idx).long().sum() for s in samples]).index_select(0, sort_order)
        ntokens = tgt_lengths.sum().item()
        if input_feeding:
            prev_output_tokens = merge("target", left_pad_target, move_eos_to_beginning=True)
    else:
        ntokens = src_lengths.sum().item()
    batch = {"id": ids, "nsentences": len(samples), "ntokens": ntokens,
             "net_input": {"src_tokens": src_tokens, "src_lengths": src_lengths}, "target": target}
    if prev_output_tokens is not None:
        batch["net_input"]["prev_output_tokens"] = prev_output_tokens.index_select(0, sort_order)
    return batch


# --------------------------------------------------------------------------------------------------------------------
_TOK_CODE = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.int32): 2, np.dtype(np.int64): 3}


def default_resident_budget_mb():
    """CST_RESIDENT_CORPUS_MB, or 1/16 of the device memory that is free when the split is loaded (the models of this recipe need a few
    GB of the 288; a corpus that takes more than a sixteenth of what is left is not the small-corpus case this route is for)."""
    v = os.environ.get("CST_RESIDENT_CORPUS_MB")
    if v is not None:
        return float(v)
    free, _ = torch.cuda.mem_get_info()
    return free / 16.0 / 2 ** 20


class ResidentPairs:
    """A split's two token streams (stored dtype) and their int64 element offsets on the device, and the batch assembly over them."""
    RING = 64  # pinned index slots; a slot is reused only after the copy that read it has completed (checked with its event)

    def __init__(self, src_stream, src_offsets, tgt_stream, tgt_offsets, pad, eos, left_pad_source=True, left_pad_target=False):
        src_stream, tgt_stream = np.asarray(src_stream), np.asarray(tgt_stream)
        if src_stream.dtype not in _TOK_CODE or tgt_stream.dtype not in _TOK_CODE:
            raise TypeError("token streams must be uint8 / uint16 / int32 / int64, got %s and %s" % (src_stream.dtype, tgt_stream.dtype))
        if src_stream.dtype != tgt_stream.dtype:  # one element type per launch: the narrower side is widened once, here
            wide = max(src_stream.dtype, tgt_stream.dtype, key=lambda d: _TOK_CODE[d])
            src_stream, tgt_stream = src_stream.astype(wide), tgt_stream.astype(wide)
        self.tok_dtype = _TOK_CODE[src_stream.dtype]
        self._host = (src_stream, np.ascontiguousarray(src_offsets, dtype=np.int64), tgt_stream, np.ascontiguousarray(tgt_offsets, dtype=np.int64))
        for stream, off, name in ((self._host[0], self._host[1], "source"), (self._host[2], self._host[3], "target")):
            if off.ndim != 1 or len(off) < 2 or off[0] != 0 or off[-1] != len(stream) or np.any(np.diff(off) < 0):
                raise ValueError("%s offsets must rise from 0 to the stream's length %d" % (name, len(stream)))
        if len(self._host[1]) != len(self._host[3]):
            raise ValueError("source and target must contain the same number of examples")
        self.pad, self.eos, self.left_pad_source, self.left_pad_target = int(pad), int(eos), bool(left_pad_source), bool(left_pad_target)
        self._dev = None
        self._slots, self._events, self._next = None, None, 0

    @property
    def nbytes(self):
        return sum(a.nbytes for a in self._host)

    def _upload(self, device):
        def up(a):
            return torch.from_numpy(np.array(a, copy=True).reshape(-1).view(np.uint8)).to(device)

        src, so, tgt, to = self._host
        # an empty stream still needs an address for the launch's null check: one pad byte
        self._dev = (up(src) if src.size else torch.zeros(8, dtype=torch.uint8, device=device), torch.from_numpy(so.copy()).to(device),
                     up(tgt) if tgt.size else torch.zeros(8, dtype=torch.uint8, device=device), torch.from_numpy(to.copy()).to(device))
        self._device = device

    def _index_to_device(self, idx):
        """The index vector through a pinned slot, asynchronously: no pageable copy (which would drain the stream), no host wait."""
        B = idx.numel()
        if self._slots is None or self._slots.size(1) < B:
            self._slots = torch.empty(self.RING, max(B, 256), dtype=torch.int64).pin_memory()
            self._events = [None] * self.RING
        k, self._next = self._next, (self._next + 1) % self.RING
        if self._events[k] is not None:
            self._events[k].synchronize()  # (done long ago in any loop that reads a result every 64 batches; a wait only otherwise)
        slot = self._slots[k, :B]
        slot.copy_(idx)
        dev = slot.to(self._device, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._events[k] = ev
        return dev

    def collate(self, idx, S, T, device="cuda", out=None):
        """(src_tokens, src_lengths, prev_output_tokens, target) of the sentences `idx` (host int64 tensor, row order), widths S / T."""
        from . import kernels as K
        if self._dev is None:
            self._upload(torch.device(device))
        src, so, tgt, to = self._dev
        st, sl, prev, target, _ = K.collate_pairs(src, tgt, self.tok_dtype, so, to, self._index_to_device(idx), S, T, self.pad, self.eos,
                                                  self.left_pad_source, self.left_pad_target, out=out)
        return st, sl, prev, target

    def materialize(self, sample, device="cuda"):
        """The collater's record -> the batch the host collater would have built, on the device."""
        ni = sample["net_input"]
        S, T = ni["pair_widths"]
        st, sl, prev, target = self.collate(ni["pair_idx"], S, T, device)
        net_input = {"src_tokens": st, "src_lengths": sl, "prev_output_tokens": prev}
        # (id: the sentence indices in row order ARE the index vector; the consumers of ids read the host record)
        return {"id": sample["id"], "nsentences": sample["nsentences"], "ntokens": sample["ntokens"], "net_input": net_input, "target": target}


def is_pair_record(sample):
    ni = sample.get("net_input") if isinstance(sample, dict) else None
    return bool(ni) and "pair_idx" in ni


# --------------------------------------------------------------------------------------------------------------------
class LanguagePairDataset(torch.utils.data.Dataset):
    """language_pair_dataset.py:168-470 over two MMapIndexedDatasets (or any pair of sequences of int64 tensors with `sizes`)."""

    def __init__(self, src, src_sizes, src_dict, tgt=None, tgt_sizes=None, tgt_dict=None, left_pad_source=True, left_pad_target=False,
                 shuffle=True, input_feeding=True, pad_to_multiple=1):
        if tgt_dict is not None:
            assert src_dict.pad() == tgt_dict.pad()
            assert src_dict.eos() == tgt_dict.eos()
            assert src_dict.unk() == tgt_dict.unk()
        if tgt is not None:
            assert len(src) == len(tgt), "Source and target must contain the same number of examples"
        self.src, self.tgt = src, tgt
        self.src_sizes = np.array(src_sizes)
        self.tgt_sizes = np.array(tgt_sizes) if tgt_sizes is not None else None
        self.sizes = np.vstack((self.src_sizes, self.tgt_sizes)).T if self.tgt_sizes is not None else self.src_sizes
        self.src_dict, self.tgt_dict = src_dict, tgt_dict
        self.left_pad_source, self.left_pad_target = left_pad_source, left_pad_target
        self.shuffle, self.input_feeding, self.pad_to_multiple = shuffle, input_feeding, pad_to_multiple
        self.eos = src_dict.eos()
        self.resident = None  # a ResidentPairs once enable_resident() has decided for the device route

    # ---- the resident route -----------------------------------------------------------------------------------------
    def enable_resident(self, budget_mb=None):
        """Decide the route of this split (call from the trainer's thread, before batches are drawn): resident unless
        CST_PAIR_COLLATE=host, no GPU, no target side, or the streams exceed the budget.  Nothing is uploaded here."""
        self.resident = None
        mode = os.environ.get("CST_PAIR_COLLATE", "device")
        if mode not in ("host", "device"):
            raise ValueError("CST_PAIR_COLLATE must be `host` or `device`, got %r" % mode)
        if mode == "host" or self.tgt is None or not torch.cuda.is_available() or not hasattr(self.src, "stream") or not hasattr(self.tgt, "stream"):
            return False
        pairs = ResidentPairs(self.src.stream, self.src.offsets, self.tgt.stream, self.tgt.offsets, self.src_dict.pad(), self.eos,
                              self.left_pad_source, self.left_pad_target)
        budget = default_resident_budget_mb() if budget_mb is None else budget_mb
        if pairs.nbytes > budget * 2 ** 20:
            logger.info("corpus of %.1f MB exceeds the resident budget of %.1f MB (CST_RESIDENT_CORPUS_MB): host batch assembly",
                        pairs.nbytes / 2 ** 20, budget)
            return False
        self.resident = pairs
        return True

    def __getitem__(self, index):
        if self.resident is not None:
            return {"id": index}  # the record route reads no token
        return {"id": index, "source": self.src[index], "target": self.tgt[index] if self.tgt is not None else None}

    def item(self, index):
        """The sentence pair itself, whatever the route."""
        return {"id": index, "source": self.src[index], "target": self.tgt[index] if self.tgt is not None else None}

    def __len__(self):
        return len(self.src)

    def collater(self, samples):
        if len(samples) == 0:
            return {}
        if "source" not in samples[0]:
            return self.record([s["id"] for s in samples])
        return collate(samples, self.src_dict.pad(), self.eos, self.left_pad_source, self.left_pad_target, self.input_feeding,
                       self.pad_to_multiple)

    def host_batch(self, indices):
        """The host collater's batch of the sentences `indices` (the reference batch of either route)."""
        return collate([self.item(int(i)) for i in indices], self.src_dict.pad(), self.eos, self.left_pad_source, self.left_pad_target,
                       self.input_feeding, self.pad_to_multiple)

    def record(self, indices):
        """What the resident route needs of a batch, from the host-side sizes alone: the indices in the collater's row order (the same
        torch sort of the same lengths, so ties fall as in the host collater), the widths, the lengths and the token count."""
        ids = torch.LongTensor(indices)
        src_lengths, order = torch.from_numpy(self.src_sizes[ids.numpy()].astype(np.int64)).sort(descending=True)
        ids = ids.index_select(0, order)
        tgt_sizes = self.tgt_sizes[ids.numpy()]
        S = padded_width(int(src_lengths[0]), self.pad_to_multiple)
        T = padded_width(int(tgt_sizes.max()), self.pad_to_multiple)
        return {"id": ids, "nsentences": len(indices), "ntokens": int(tgt_sizes.sum()),
                "net_input": {"pair_idx": ids, "pair_widths": (S, T), "pair_corpus": self.resident, "src_lengths": src_lengths},
                "target": None}

    # ---- sizes, order, filter, batches ------------------------------------------------------------------------------
    def num_tokens(self, index):
        return max(self.src_sizes[index], self.tgt_sizes[index] if self.tgt_sizes is not None else 0)

    def size(self, index):
        return (self.src_sizes[index], self.tgt_sizes[index] if self.tgt_sizes is not None else 0)

    def ordered_indices(self):
        """:420-437 — a random permutation (under the caller's numpy_seed), then the two stable sorts: by target, then source length."""
        if self.shuffle:
            indices = np.random.permutation(len(self)).astype(np.int64)
        else:
            indices = np.arange(len(self), dtype=np.int64)
        if self.tgt_sizes is not None:
            indices = indices[np.argsort(self.tgt_sizes[indices], kind="mergesort")]
        return indices[np.argsort(self.src_sizes[indices], kind="mergesort")]

    def filter_indices_by_size(self, indices, max_sizes):
        """data_utils.py:240-273."""
        if max_sizes is None:
            return indices, []
        if type(max_sizes) in (int, float):
            max_src, max_tgt = max_sizes, max_sizes
        else:
            max_src, max_tgt = max_sizes
        bad = self.src_sizes[indices] > max_src
        if self.tgt_sizes is not None:
            bad = bad | (self.tgt_sizes[indices] > max_tgt)
        return indices[~bad], indices[bad].tolist()

    def batch_by_size(self, indices, max_tokens=None, max_sentences=None, required_batch_size_multiple=1):
        from . import data as D
        sizes = np.maximum(self.src_sizes, self.tgt_sizes) if self.tgt_sizes is not None else self.src_sizes
        return D.batch_by_size(indices, None, max_tokens, max_sentences, required_batch_size_multiple,
                               sizes=sizes[np.asarray(indices, dtype=np.int64)])


# --------------------------------------------------------------------------------------------------------------------
def split_paths(paths):
    """utils.split_paths: colon-separated data directories (a URL-like `://` path is one)."""
    return paths.split(os.pathsep) if "://" not in paths else paths.split("|")


def load_langpair_dataset(data_path, split, src, src_dict, tgt, tgt_dict, combine=False, dataset_impl=None, upsample_primary=1,
                          left_pad_source=True, left_pad_target=False, max_source_positions=1024, max_target_positions=1024,
                          load_alignments=False, truncate_source=False, num_buckets=0, shuffle=True, pad_to_multiple=1):
    """translation.py:34-161: `<split>.<src>-<tgt>.<lang>.{bin,idx}`, tried in both pair orders.  Refused by name: what the Chimera MT
    stage does not use."""
    ID.check_dataset_impl(dataset_impl)
    if upsample_primary != 1:
        raise NotImplementedError("--upsample-primary %s: upsampling a primary corpus over shards is not built" % upsample_primary)
    if truncate_source:
        raise NotImplementedError("--truncate-source is not built")
    if load_alignments:
        raise NotImplementedError("--load-alignments is not built")
    if num_buckets > 0:
        raise NotImplementedError("--num-batch-buckets %d: length buckets (a TPU measure) are not built" % num_buckets)

    def prefix_of(name):
        for a, b in ((src, tgt), (tgt, src)):
            p = os.path.join(data_path, "%s.%s-%s." % (name, a, b))
            if ID.dataset_exists(p + src):
                return p
            if os.path.exists(p + src + ".txt"):
                raise NotImplementedError("%s%s.txt: the `raw` dataset implementation is not built; binarise with --dataset-impl mmap" % (p, src))
        return None

    prefix = prefix_of(split)
    if prefix is None:
        raise FileNotFoundError("Dataset not found: {} ({})".format(split, data_path))
    if prefix_of(split + "1") is not None:
        raise NotImplementedError("%s1: sharded splits (train, train1, ...) are not built; binarise the corpus as one split" % split)
    src_ds = ID.MMapIndexedDataset(prefix + src)
    tgt_ds = ID.MMapIndexedDataset(prefix + tgt) if ID.dataset_exists(prefix + tgt) else None
    logger.info("%s %s %s-%s %d examples", data_path, split, src, tgt, len(src_ds))
    return LanguagePairDataset(src_ds, src_ds.sizes, src_dict, tgt_ds, tgt_ds.sizes if tgt_ds is not None else None, tgt_dict,
                               left_pad_source=left_pad_source, left_pad_target=left_pad_target, shuffle=shuffle,
                               pad_to_multiple=pad_to_multiple)
