"""The host-side rules of the conv section of functional.py that need no GPU.

The K-block stamp rule (functional.posconv_k_block_stamps: one body for the host row counts, numpy, and the device row counts, torch)
against its independent restatement posconv_ref.k_block_stamps — a Python loop over the blocks — on every case of posconv_ref.CASES and
the row vectors: nothing live, everything live, two seeded random vectors in [0, T], and the limits the GPU tests use for that case."""
import importlib
import zlib

import numpy as np
import pytest
import torch

import posconv_ref as R
from conftest import load_pkg


@pytest.fixture(scope="module")
def CF():
    load_pkg()
    return importlib.import_module("chimera-st_amd.functional")


def row_vectors(name):
    B, T, _, _ = R.CASES[name]
    rng = np.random.RandomState(zlib.crc32(name.encode()))
    out = [(0,) * B, (T,) * B] + [tuple(int(v) for v in rng.randint(0, T + 1, size=B)) for _ in range(2)]
    if name in R.LIMITS:
        out.append(tuple(R.LIMITS[name]))
    if name == "past_list":
        out.append(tuple(R.PAST_LIST_ROWS))
    return out


@pytest.mark.parametrize("name", list(R.CASES))
def test_k_block_stamps_equal_the_reference_from_numpy_and_from_torch(CF, name):
    B, T, G, k = R.CASES[name]
    geo = R.geometry(B, T, G, k)
    assert CF._posconv_geometry(B, T, k) == (geo["padl"], geo["lp"], geo["Tp"], geo["Kr"])
    for rows in row_vectors(name):
        assert len(rows) == B
        ref = R.k_block_stamps(B, T, k, rows)
        host = CF.posconv_k_block_stamps(np.asarray(rows), B, geo["Tp"], geo["Kr"])
        dev = CF.posconv_k_block_stamps(torch.tensor(rows, dtype=torch.int32), B, geo["Tp"], geo["Kr"])
        assert isinstance(host, np.ndarray) and host.dtype == np.int32 and host.shape == ((geo["Kr"] + 63) // 64,)
        assert isinstance(dev, torch.Tensor) and dev.dtype == torch.int32 and tuple(dev.shape) == ((geo["Kr"] + 63) // 64,)
        assert torch.equal(torch.from_numpy(host), ref), "%s rows %s: numpy stamps differ from the reference" % (name, rows)
        assert torch.equal(dev, ref), "%s rows %s: torch stamps differ from the reference" % (name, rows)
        assert torch.equal(torch.from_numpy(CF.posconv_k_block_stamps(list(rows), B, geo["Tp"], geo["Kr"])), ref)  # (the plan's list)
