"""Reader of the binarised corpora `fairseq-preprocess` writes — the `mmap` implementation of fairseq/data/indexed_dataset.py
(MMapIndexedDataset :365-517, its Index :366-459; dtype codes :98-107).

`<prefix>.idx`: magic b"MMIDIDX\\x00\\x00" (9 bytes) | version uint64 LE (= 1) | dtype code uint8 | sentence count uint64 LE |
int32 sizes [count] | int64 BYTE pointers [count].   `<prefix>.bin`: the sentences' tokens, back to back, in the coded dtype.

Streams of uint8, uint16 (what the binariser writes for a vocabulary below 65 500), int32 and int64 are read; the other implementations
(`raw`, `lazy`, `cached`: the legacy b"TNTIDX\\x00\\x00" index) are refused by name."""
import os
import struct

import numpy as np
import torch

MMAP_MAGIC = b"MMIDIDX\x00\x00"
LEGACY_MAGIC = b"TNTIDX\x00\x00"
# indexed_dataset.py:98-107 — the codes of the integer streams (6 / 7 are float / double: not token streams)
DTYPES = {1: np.uint8, 4: np.int32, 5: np.int64, 8: np.uint16}
REFUSED_IMPLS = ("raw", "lazy", "cached", "fasta")


def index_file_path(prefix):
    return prefix + ".idx"


def data_file_path(prefix):
    return prefix + ".bin"


def dataset_exists(prefix):
    return os.path.exists(index_file_path(prefix)) and os.path.exists(data_file_path(prefix))


def check_dataset_impl(impl):
    """--dataset-impl: None / "mmap" pass; every other implementation of the reference is refused by name."""
    if impl in (None, "mmap"):
        return
    if impl in REFUSED_IMPLS:
        raise NotImplementedError("--dataset-impl %s is not built: binarise with --dataset-impl mmap (fairseq-preprocess's default)" % impl)
    raise ValueError("unknown --dataset-impl %r" % (impl,))


def write_dataset(prefix, stream, sizes):
    """`<prefix>.bin/.idx` of a token stream (its dtype is the stored one) cut into sentences of `sizes` tokens — the files
    MMapIndexedDatasetBuilder.finalize leaves (:534-561).  For tools and tests that need a corpus of their own."""
    stream, sizes = np.ascontiguousarray(stream), np.asarray(sizes, dtype=np.int32)
    code = {v: k for k, v in DTYPES.items()}[stream.dtype.type]
    assert int(sizes.sum()) == len(stream)
    pointers = (np.concatenate([[0], np.cumsum(sizes[:-1], dtype=np.int64)]) * stream.dtype.itemsize).astype(np.int64)
    with open(data_file_path(prefix), "wb") as f:
        f.write(stream.tobytes(order="C"))
    with open(index_file_path(prefix), "wb") as f:
        f.write(MMAP_MAGIC + struct.pack("<Q", 1) + struct.pack("<B", code) + struct.pack("<Q", len(sizes)))
        f.write(sizes.tobytes(order="C") + pointers.tobytes(order="C"))


class MMapIndexedDataset(torch.utils.data.Dataset):
    """indexed_dataset.py:365-517.  Items are int64 tensors (copies); `stream` is the whole token stream as stored (a numpy.memmap) and
    `offsets` the int64 ELEMENT offsets [len + 1] of the sentences in it — what the device-resident route uploads."""

    def __init__(self, prefix):
        self.prefix = prefix
        if not os.path.exists(index_file_path(prefix)) and os.path.exists(prefix + ".txt"):
            raise NotImplementedError("%s.txt: the `raw` dataset implementation (text files) is not built; binarise with fairseq-preprocess "
                                      "--dataset-impl mmap" % prefix)
        with open(index_file_path(prefix), "rb") as f:
            magic = f.read(9)
            if magic[:8] == LEGACY_MAGIC:
                raise NotImplementedError("%s: a `lazy` / `cached` (legacy TNTIDX) index; only the `mmap` implementation is built — binarise "
                                          "with fairseq-preprocess --dataset-impl mmap" % index_file_path(prefix))
            if magic != MMAP_MAGIC:
                raise ValueError("%s: not an mmap index file (magic %r)" % (index_file_path(prefix), magic))
            (version,) = struct.unpack("<Q", f.read(8))
            if version != 1:
                raise ValueError("%s: index version %d (1 expected)" % (index_file_path(prefix), version))
            (code,) = struct.unpack("<B", f.read(1))
            if code not in DTYPES:
                raise NotImplementedError("%s: dtype code %d is not a token stream this build reads (uint8 1, int32 4, int64 5, uint16 8)"
                                          % (index_file_path(prefix), code))
            (count,) = struct.unpack("<Q", f.read(8))
            header = f.tell()
        self.dtype = np.dtype(DTYPES[code])
        self._index = np.memmap(index_file_path(prefix), mode="r", order="C")
        self._sizes = np.frombuffer(self._index, dtype=np.int32, count=count, offset=header)
        self._pointers = np.frombuffer(self._index, dtype=np.int64, count=count, offset=header + self._sizes.nbytes)
        nbytes = os.path.getsize(data_file_path(prefix))
        if nbytes % self.dtype.itemsize:
            raise ValueError("%s: %d bytes is not a whole number of %s tokens" % (data_file_path(prefix), nbytes, self.dtype))
        self.stream = np.memmap(data_file_path(prefix), mode="r", order="C", dtype=self.dtype) if nbytes else np.zeros(0, self.dtype)
        if np.any(self._pointers % self.dtype.itemsize):
            raise ValueError("%s: a sentence pointer is not a multiple of the token size" % index_file_path(prefix))
        self.offsets = np.empty(count + 1, dtype=np.int64)
        self.offsets[:count] = self._pointers // self.dtype.itemsize
        self.offsets[count] = (self.offsets[count - 1] + self._sizes[count - 1]) if count else 0
        if count and (np.any(np.diff(self.offsets) != self._sizes) or self.offsets[0] != 0 or self.offsets[count] != len(self.stream)):
            raise ValueError("%s: sizes and pointers do not describe one contiguous stream of %d tokens" % (index_file_path(prefix), len(self.stream)))

    def __len__(self):
        return len(self._sizes)

    def __getitem__(self, i):
        if i < 0 or i >= len(self):
            raise IndexError(i)
        return torch.from_numpy(np.asarray(self.stream[self.offsets[i]:self.offsets[i + 1]]).astype(np.int64))

    @property
    def sizes(self):
        return self._sizes
