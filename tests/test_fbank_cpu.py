"""The filter-bank input route without a GPU: the fp64 restatement of Kaldi fbank (fbank_ref.py), the .npy / stored-zip routes
with the host feature transforms and the audio route's collater (SpecAugment draws, order, frame counts) against the REAL
reference's outputs (tools/ref_harness/make_fbank_goldens.py -> tests/golden/fbank_pipeline_tiny.npz), and the rejections."""
import os
import shutil
import wave
import zipfile
from argparse import Namespace
from importlib import import_module

import numpy as np
import pytest
import torch

import fbank_ref as R
from conftest import GOLDEN, load_golden, load_pkg

FIX = os.path.join(GOLDEN, "fbank_tiny")
LB = {"time_warp_W": 0, "freq_mask_N": 1, "freq_mask_F": 27, "time_mask_N": 1, "time_mask_T": 100, "time_mask_p": 1.0}


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    load_pkg()
    lib = import_module("chimera-st_amd.lib")
    if not os.path.exists(lib.LIB_PATH):
        ge.build()
    return import_module("chimera-st_amd.data"), import_module("chimera-st_amd.fbank"), import_module("chimera-st_amd.tasks")


def fixture_task(pkg, tmp_path, cfg_name):
    _, _, tasks = pkg
    root = tmp_path / cfg_name
    root.mkdir()
    for f in os.listdir(FIX):
        if f.endswith((".tsv", ".txt")):
            shutil.copy(os.path.join(FIX, f), root / f)
    (root / "config.yaml").write_text(open(os.path.join(FIX, "config_%s.yaml" % cfg_name)).read().replace("AUDIO_ROOT", FIX))
    return tasks.TripletTask(Namespace(data=str(root), config_yaml="config.yaml", seed=1))


def write_wav(path, x, sr=16000, ch=1):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(ch); w.setsampwidth(2); w.setframerate(sr)
        w.writeframes(np.asarray(x, dtype="<i2").tobytes())


def small_task(pkg, tmp_path, audio_entries, transforms=None, normalize=False, spec=LB):
    """A one-split manifest root in tmp_path over the given `audio` column entries (relative to tmp_path)."""
    _, _, tasks = pkg
    shutil.copy(os.path.join(FIX, "dict.txt"), tmp_path / "dict.txt")
    cfg = "audio_root: %s\nvocab_filename: dict.txt\nsrc_vocab_filename: dict.txt\nuse_audio_input: false\n" % tmp_path
    if transforms is not None:
        cfg += "transforms:\n  _train: [%s]\nspecaugment: %s\n" % (", ".join(transforms), dict(spec))
    (tmp_path / "config.yaml").write_text(cfg)
    with open(tmp_path / "train_x.tsv", "w") as f:
        f.write("id\taudio\tn_frames\ttgt_text\tsrc_text\tspeaker\n")
        for i, a in enumerate(audio_entries):
            f.write("u%d\t%s\t10\t▁the ▁cat\t▁a\tspk0\n" % (i, a))
    t = tasks.TripletTask(Namespace(data=str(tmp_path), config_yaml="config.yaml", seed=1, normalize=normalize))
    return t.load_dataset("train_x")


# ---------------------------------------------------------------------------------------------------------------- restatement
def test_mel_matrix_anchors():
    W = R.mel_matrix()
    assert W.shape == (80, 257)
    assert (W[:, 256] == 0).all()
    left, center, right = R.band_edges()
    inv = lambda m: 700.0 * (np.exp(m / 1127.0) - 1.0)
    np.testing.assert_allclose(np.diag(R.mel_weights(inv(center))), 1.0, atol=1e-9)  # each triangle peaks at 1, at its centre
    np.testing.assert_allclose(inv(left[0]), 20.0, rtol=1e-12)
    np.testing.assert_allclose(inv(right[-1]), 8000.0, rtol=1e-12)
    np.testing.assert_allclose(np.diff(center), (R.mel(8000.0) - R.mel(20.0)) / 81, rtol=1e-9)
    assert (W >= 0).all() and W.max() <= 1.0
    assert (W[:, 0] == 0).all()  # 0 Hz is below the 20 Hz low edge
    # each interior bin feeds at most two adjacent filters
    nz = W[:, :256] > 0
    assert nz.sum(axis=0).max() <= 2
    for k in np.nonzero(nz.sum(axis=0) == 2)[0]:
        a, b = np.nonzero(nz[:, k])[0]
        assert b == a + 1


@pytest.mark.parametrize("n,frames", [(399, 0), (400, 1), (401, 1), (560, 2)])
def test_frame_counts(pkg, n, frames):
    assert R.n_frames(n) == frames == pkg[1].num_frames(n)
    assert R.fbank(np.zeros(n)).shape == (frames, 80)


def test_zero_audio_gives_log_eps():
    f = R.fbank(np.zeros(16000))
    assert (f == np.log(np.float64(np.float32(1.1920929e-07)))).all()
    assert abs(f[0, 0] - (-15.942385)) < 1e-6


@pytest.mark.parametrize("m", [5, 30, 60])
def test_tone_peaks_in_its_filter(m):
    _, center, _ = R.band_edges()
    f0 = 700.0 * (np.exp(center[m] / 1127.0) - 1.0)
    t = np.arange(8000) / 16000.0
    f = R.fbank(0.3 * np.sin(2 * np.pi * f0 * t))
    assert (np.argmax(f, axis=1) == m).all()


# ---------------------------------------------------------------------------------------------------------------- vs the reference
@pytest.mark.parametrize("cfg_name,kind", [("prep", "zip"), ("ucmvn_sa", "npy"), ("ucmvn_sa", "zip"), ("gcmvn_sa", "npy")])
def test_feature_routes_match_reference(pkg, tmp_path, cfg_name, kind):
    """.npy and stored-zip entries with the host transforms, under the reference's np.random state: bit for bit."""
    g = load_golden("fbank_pipeline_tiny.npz")
    ds = fixture_task(pkg, tmp_path, cfg_name).load_dataset("train_" + kind)
    np.random.seed(1)
    s = ds.collater([ds[i] for i in range(len(ds))])
    key = "%s/%s/" % (cfg_name, kind)
    assert s["id"].tolist() == g[key + "id"].tolist()
    assert s["net_input"]["src_lengths"].tolist() == g[key + "src_lengths"].tolist()
    assert s["net_input"]["src_tokens"].dtype == torch.float32
    assert np.array_equal(s["net_input"]["src_tokens"].numpy(), g[key + "src_tokens"])


@pytest.mark.parametrize("cfg_name", ["ucmvn_sa", "gcmvn_sa"])
def test_audio_route_collater_matches_reference(pkg, tmp_path, cfg_name):
    """.wav entries: the reference's draws, in its order, with its early returns; its sort order and frame counts."""
    D, FB, _ = pkg
    g = load_golden("fbank_pipeline_tiny.npz")
    key = "%s/wav/" % cfg_name
    ds = fixture_task(pkg, tmp_path, cfg_name).load_dataset("train_wav")
    np.random.seed(1)
    items = [ds[i] for i in range(len(ds))]
    draws = np.split(g[key + "draws"], np.cumsum(g[key + "draws_len"])[:-1])
    for it, want in zip(items, draws):
        a = it[1]
        assert isinstance(a, D.FbankAudio)
        got = [v for f0, f in a.fmask for v in (f, f0)] + [v for t0, t in a.tmask for v in (t, t0)]
        assert got == want.tolist()
    s = ds.collater(items)
    ni = s["net_input"]
    assert "src_tokens" not in ni
    assert s["id"].tolist() == g[key + "id"].tolist()
    assert ni["src_lengths"].tolist() == g[key + "src_lengths"].tolist()
    order = s["id"].tolist()
    lens = [items[i][1].wave.numel() for i in order]
    assert ni["src_audio_lengths"].tolist() == lens
    assert ni["src_audio"].shape == (len(order), (max(lens) + 3) // 4 * 4) and ni["src_audio"].dtype == torch.float32
    for r, i in enumerate(order):
        assert torch.equal(ni["src_audio"][r, :lens[r]], items[i][1].wave)
        assert (ni["src_audio"][r, lens[r]:] == 0).all()
        assert ni["src_audio_fmask"][r].tolist() == [list(x) for x in items[i][1].fmask]
        assert ni["src_audio_tmask"][r].tolist() == [list(x) for x in items[i][1].tmask]
    # the reference's wave-route features hold one value over each drawn frequency band (the fixture is self-consistent)
    ref = g[key + "src_tokens"]
    for r, i in enumerate(order):
        for f0, f in items[i][1].fmask:
            band = ref[r, :ni["src_lengths"][r], f0:f0 + f]
            assert (band == band.flat[0]).all()


def test_wav_segment_route_is_the_slice(pkg, tmp_path):
    """x.wav:<offset>:<count> (the reference asserts there) takes the fbank route over that slice of the file."""
    x = np.round(np.random.RandomState(2).randn(6000) * 1000).astype(np.int16)
    write_wav(tmp_path / "a.wav", x)
    ds = small_task(pkg, tmp_path, ["a.wav:1000:2000", "a.wav"])
    a, b = ds[0][1], ds[1][1]
    assert a.n_frames == R.n_frames(2000) and b.n_frames == R.n_frames(6000)
    assert torch.equal(a.wave, torch.from_numpy(x[1000:3000].astype(np.float32) / 32768.0))
    assert a.fmask == [] and a.tmask == []  # no transforms configured


def test_host_transform_order_is_free_on_feature_route(pkg, tmp_path):
    np.save(tmp_path / "f.npy", np.random.RandomState(0).randn(50, 80).astype(np.float32))
    ds = small_task(pkg, tmp_path, ["f.npy"], ["specaugment", "utterance_cmvn"])
    np.random.seed(3)
    assert ds[0][1].shape == (50, 80)


# ---------------------------------------------------------------------------------------------------------------- rejections
def test_rejects_time_warp(pkg, tmp_path):
    np.save(tmp_path / "f.npy", np.zeros((20, 80), np.float32))
    with pytest.raises(ValueError, match="time warping"):
        small_task(pkg, tmp_path, ["f.npy"], ["specaugment"], spec=dict(LB, time_warp_W=5))


def test_rejects_flac(pkg, tmp_path):
    (tmp_path / "a.flac").write_bytes(b"fLaC" + bytes(100))
    ds = small_task(pkg, tmp_path, ["a.flac"])
    with pytest.raises(ValueError, match="FLAC"):
        ds[0]


def test_rejects_wav_in_zip(pkg, tmp_path):
    write_wav(tmp_path / "a.wav", np.zeros(1000, np.int16))
    with zipfile.ZipFile(tmp_path / "z.zip", "w", zipfile.ZIP_STORED) as z:
        z.write(tmp_path / "a.wav", "a.wav")
    with zipfile.ZipFile(tmp_path / "z.zip") as z:
        i = z.infolist()[0]
        off, size = i.header_offset + 30 + len(i.filename), i.file_size
    ds = small_task(pkg, tmp_path, ["z.zip:%d:%d" % (off, size)])
    with pytest.raises(ValueError, match="inside a zip"):
        ds[0]


def test_rejects_multichannel(pkg, tmp_path):
    write_wav(tmp_path / "a.wav", np.zeros(2000, np.int16), ch=2)
    with pytest.raises(ValueError, match="multi-channel"):
        small_task(pkg, tmp_path, ["a.wav"])[0]


def test_rejects_other_sample_rates(pkg, tmp_path):
    write_wav(tmp_path / "a.wav", np.zeros(2000, np.int16), sr=8000)
    with pytest.raises(ValueError, match="sample rate"):
        small_task(pkg, tmp_path, ["a.wav"])[0]


def test_rejects_short_utterances(pkg, tmp_path):
    write_wav(tmp_path / "a.wav", np.zeros(399, np.int16))
    with pytest.raises(ValueError, match="shorter than one"):
        small_task(pkg, tmp_path, ["a.wav"])[0]


def test_rejects_normalize_on_fbank_route(pkg, tmp_path):
    write_wav(tmp_path / "a.wav", np.zeros(2000, np.int16))
    with pytest.raises(ValueError, match="--normalize"):
        small_task(pkg, tmp_path, ["a.wav"], normalize=True)[0]


def test_rejects_other_transform_order_on_device_route(pkg, tmp_path):
    write_wav(tmp_path / "a.wav", np.zeros(2000, np.int16))
    ds = small_task(pkg, tmp_path, ["a.wav"], ["specaugment", "utterance_cmvn"])
    with pytest.raises(ValueError, match="followed by at most one specaugment"):
        ds[0]


def test_rejects_mixed_batches(pkg, tmp_path):
    write_wav(tmp_path / "a.wav", np.zeros(2000, np.int16))
    np.save(tmp_path / "f.npy", np.zeros((11, 80), np.float32))
    ds = small_task(pkg, tmp_path, ["a.wav", "f.npy"])
    with pytest.raises(ValueError, match="mixes"):
        ds.collater([ds[0], ds[1]])


def test_device_stage_needs_gpu_tensors(pkg):
    FB = pkg[1]
    with pytest.raises(RuntimeError, match="not on the GPU"):
        FB.fbank(torch.zeros(1, 800), torch.tensor([800]))


def test_cst_fbank_validates_before_any_hip_call(pkg):
    import ctypes
    L = import_module("chimera-st_amd.lib")
    lib = L.load()
    d = L.FbankDesc()
    assert lib.cst_fbank(ctypes.byref(d), None) == -1
    assert b"null operand" in lib.cst_last_error()
    d.wave, d.n_samples, d.out, d.B, d.S, d.T = 16, 16, 16, 2, 1000, 4
    d.specaugment, d.n_fmask = 1, 9
    assert lib.cst_fbank(ctypes.byref(d), None) == -1
    assert b"at most 8" in lib.cst_last_error()
    d.n_fmask, d.utterance_cmvn = 1, 1
    assert lib.cst_fbank(ctypes.byref(d), None) == -1
    assert b"mask intervals" in lib.cst_last_error()
    assert lib.cst_fbank_workspace_bytes(2, 33) == 2 * 2 * 2 * 80 * 8
