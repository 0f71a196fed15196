"""Filter-bank input from audio (the reference's fbank route):
  feature_transforms/utterance_cmvn.py, global_cmvn.py, specaugment.py, __init__.py (CompositeAudioFeatureTransform) — restated in
  numpy for the feature route (.npy / stored-zip entries), where __getitem__ applies them on the host as the reference does;
  fbank() — the device feature stage of the audio route (.wav entries): collated 16 kHz audio in, Kaldi filter banks with the
  configured transforms out, computed by cst_fbank (csrc/fbank.hip).  SpecAugment's intervals are drawn on the host, in
  __getitem__, with the reference's np.random calls; only the values are computed on the device."""
import ctypes
import math
import numbers

import numpy as np
import torch

from . import lib as L

NMEL, WIN, SHIFT, SAMPLE_RATE = 80, 400, 160, 16000


def num_frames(num_samples: int) -> int:
    """Frames of Kaldi's snip_edges framing: 400-sample windows every 160 samples."""
    return 0 if num_samples < WIN else 1 + (num_samples - WIN) // SHIFT


# --------------------------------------------------------------------------------------------------------------------
class UtteranceCMVN:
    """feature_transforms/utterance_cmvn.py:8-37."""
    name = "utterance_cmvn"

    def __init__(self, norm_means=True, norm_vars=True):
        self.norm_means, self.norm_vars = norm_means, norm_vars

    @classmethod
    def from_config_dict(cls, config=None):
        c = config or {}
        return cls(c.get("norm_means", True), c.get("norm_vars", True))

    def __call__(self, x):
        mean = x.mean(axis=0)
        square_sums = (x ** 2).sum(axis=0)
        if self.norm_means:
            x = np.subtract(x, mean)
        if self.norm_vars:
            var = square_sums / x.shape[0] - mean ** 2
            std = np.sqrt(np.maximum(var, 1e-10))
            x = np.divide(x, std)
        return x

    def draw(self, num_frames):
        return None


class GlobalCMVN:
    """feature_transforms/global_cmvn.py:8-23."""
    name = "global_cmvn"

    def __init__(self, stats_npz_path):
        stats = np.load(stats_npz_path)
        self.mean, self.std = stats["mean"], stats["std"]

    @classmethod
    def from_config_dict(cls, config=None):
        return cls((config or {}).get("stats_npz_path"))

    def __call__(self, x):
        return np.divide(np.subtract(x, self.mean), self.std)

    def draw(self, num_frames):
        return None


class SpecAugment:
    """feature_transforms/specaugment.py:12-133 without time warping (its cv2 resize is not available: time_warp_W > 0 is
    rejected).  draw() makes the np.random calls of __call__, in the same order and with the same early returns, and returns the
    intervals; __call__ is draw() plus the masking."""
    name = "specaugment"

    def __init__(self, time_warp_w=0, freq_mask_n=0, freq_mask_f=0, time_mask_n=0, time_mask_t=0, time_mask_p=0.0, mask_value=0.0):
        assert mask_value is None or isinstance(mask_value, numbers.Number), \
            f"mask_value (type: {type(mask_value)}) must be None or a number"
        if freq_mask_n > 0:
            assert freq_mask_f > 0, f"freq_mask_F ({freq_mask_f}) must be larger than 0 when doing freq masking."
        if time_mask_n > 0:
            assert time_mask_t > 0, f"time_mask_T ({time_mask_t}) must be larger than 0 when doing time masking."
        if time_warp_w > 0:
            raise ValueError("specaugment: time warping (time_warp_W = %d > 0) is not supported (the reference needs cv2 for it); "
                             "set time_warp_W: 0" % time_warp_w)
        self.time_warp_w, self.freq_mask_n, self.freq_mask_f = time_warp_w, freq_mask_n, freq_mask_f
        self.time_mask_n, self.time_mask_t, self.time_mask_p, self.mask_value = time_mask_n, time_mask_t, time_mask_p, mask_value

    @classmethod
    def from_config_dict(cls, config=None):
        c = config or {}
        return cls(c.get("time_warp_W", 0), c.get("freq_mask_N", 0), c.get("freq_mask_F", 0), c.get("time_mask_N", 0),
                   c.get("time_mask_T", 0), c.get("time_mask_p", 0.0), c.get("mask_value", None))

    def draw(self, num_frames, num_freqs=NMEL):
        """([(f0, f)], [(t0, t)]): the frequency and time intervals __call__ masks (width 0 = nothing masked)."""
        freq, time = [], []
        if num_frames == 0 or num_freqs < self.freq_mask_f:
            return freq, time
        for _ in range(self.freq_mask_n):
            f = np.random.randint(0, self.freq_mask_f)
            f0 = np.random.randint(0, num_freqs - f)
            freq.append((f0, f))
        max_time_mask_t = min(self.time_mask_t, math.floor(num_frames * self.time_mask_p))
        if max_time_mask_t < 1:
            return freq, time
        for _ in range(self.time_mask_n):
            t = np.random.randint(0, max_time_mask_t)
            t0 = np.random.randint(0, num_frames - t)
            time.append((t0, t))
        return freq, time

    def __call__(self, spectrogram):
        assert len(spectrogram.shape) == 2, "spectrogram must be a 2-D tensor."
        distorted = spectrogram.copy()
        num_frames, num_freqs = spectrogram.shape
        mask_value = spectrogram.mean() if self.mask_value is None else self.mask_value
        freq, time = self.draw(num_frames, num_freqs)
        if num_frames == 0 or num_freqs < self.freq_mask_f:
            return spectrogram
        for f0, f in freq:
            if f != 0:
                distorted[:, f0:f0 + f] = mask_value
        for t0, t in time:
            if t != 0:
                distorted[t0:t0 + t, :] = mask_value
        return distorted


TRANSFORMS = {c.name: c for c in (UtteranceCMVN, GlobalCMVN, SpecAugment)}


class CompositeTransform:
    """feature_transforms/__init__.py CompositeAudioFeatureTransform: the configured transforms, applied in config order."""

    def __init__(self, transforms):
        self.transforms = [t for t in transforms if t is not None]

    def __call__(self, x):
        for t in self.transforms:
            x = t(x)
        return x

    def draw(self, num_frames):
        """SpecAugment's intervals for an utterance of `num_frames` frames (the audio route), drawn as __call__ would."""
        out = ([], [])
        for t in self.transforms:
            d = t.draw(num_frames)
            if d is not None:
                out = d
        return out


def build_transforms(config):
    """CompositeAudioFeatureTransform.from_config_dict: config = the data config with "transforms" = the split's list."""
    names = (config or {}).get("transforms")
    if names is None:
        return None
    for n in names:
        if n not in TRANSFORMS:
            raise ValueError("unknown feature transform %r (known: %s)" % (n, ", ".join(sorted(TRANSFORMS))))
    return CompositeTransform([TRANSFORMS[n].from_config_dict(config.get(n)) for n in names])


# --------------------------------------------------------------------------------------------------------------------
class DeviceTransforms:
    """The transform list in the form cst_fbank applies it: CMVN steps (utterance and / or global, in config order), then at most
    one SpecAugment.  Any other order is rejected (the device epilogue fuses exactly that shape)."""

    def __init__(self, composite):
        ts = composite.transforms if composite is not None else []
        names = [t.name for t in ts]
        cmvn = [t for t in ts if t.name != "specaugment"]
        ok = len(set(names)) == len(names) and all(t.name != "specaugment" for t in ts[:len(cmvn)])
        if not ok:
            raise ValueError("on the device fbank route the feature transforms must be CMVN (utterance_cmvn and / or global_cmvn, "
                             "each at most once) followed by at most one specaugment; got %s" % names)
        self.utt = next((t for t in ts if t.name == "utterance_cmvn"), None)
        self.glob = next((t for t in ts if t.name == "global_cmvn"), None)
        self.spec = next((t for t in ts if t.name == "specaugment"), None)
        self.global_first = self.glob is not None and self.utt is not None and names.index("global_cmvn") < names.index("utterance_cmvn")
        self.composite = composite
        self._dev = {}

    @property
    def empty(self):
        return self.utt is None and self.glob is None and self.spec is None

    @property
    def n_fmask(self):
        return self.spec.freq_mask_n if self.spec is not None else 0

    @property
    def n_tmask(self):
        return self.spec.time_mask_n if self.spec is not None else 0

    def draw(self, num_frames):
        return self.composite.draw(num_frames) if self.composite is not None else ([], [])

    def global_stats(self, device):
        key = str(device)
        if key not in self._dev:
            m = torch.as_tensor(np.asarray(self.glob.mean, dtype=np.float32).reshape(-1)).to(device)
            s = torch.as_tensor(np.asarray(self.glob.std, dtype=np.float32).reshape(-1)).to(device)
            if m.numel() != NMEL or s.numel() != NMEL:
                raise ValueError("global_cmvn: mean / std must have %d entries, got %d / %d" % (NMEL, m.numel(), s.numel()))
            self._dev[key] = (m, s)
        return self._dev[key]


def intervals_tensor(rows, n):
    """[B, n, 2] int32 of per-utterance interval lists (shorter lists padded with empty intervals)."""
    out = torch.zeros(len(rows), n, 2, dtype=torch.int32)
    for i, r in enumerate(rows):
        for j, (a, w) in enumerate(r[:n]):
            out[i, j, 0], out[i, j, 1] = int(a), int(w)
    return out


_ws = {}


def fbank(audio, lengths, transforms=None, fmask=None, tmask=None, max_frames=None):
    """Device filter banks of a collated audio batch.
    audio: fp32 [B, S] on the GPU, samples in [-1, 1); lengths: int64 [B] sample counts (CPU or GPU); transforms: a
    DeviceTransforms or None; fmask / tmask: int32 [B, n, 2] intervals (SpecAugment only); max_frames: the padded frame count
    (default: from `lengths`, which costs a device read when they live on the GPU).
    Returns (features fp32 [B, T, 80], n_frames int64 [B] on the GPU); rows beyond an utterance's frames are 0."""
    if not torch.is_tensor(audio) or audio.dim() != 2 or audio.dtype != torch.float32:
        raise ValueError("fbank: audio must be a float32 [B, S] tensor, got %s" % (
            "%s %s" % (tuple(audio.shape), audio.dtype) if torch.is_tensor(audio) else type(audio)))
    if not audio.is_cuda:
        raise RuntimeError("chimera-st_amd: fbank audio is not on the GPU — the HIP path has no CPU fallback")
    B, S = audio.shape
    if not torch.is_tensor(lengths) or lengths.shape != (B,) or lengths.dtype != torch.int64:
        raise ValueError("fbank: lengths must be an int64 [B=%d] tensor" % B)
    if max_frames is None:
        max_frames = num_frames(int(lengths.max()))
    if max_frames < 1:
        raise ValueError("fbank: no utterance has a frame (%d samples are needed for one)" % WIN)
    dev = audio.device
    audio = audio.contiguous()
    lengths = lengths.to(dev, non_blocking=True)
    out = torch.empty(B, max_frames, NMEL, dtype=torch.float32, device=dev)
    nfr = torch.empty(B, dtype=torch.int64, device=dev)
    d = L.FbankDesc()
    d.B, d.S, d.T = B, S, max_frames
    d.wave, d.n_samples, d.out, d.n_frames = audio.data_ptr(), lengths.data_ptr(), out.data_ptr(), nfr.data_ptr()
    keep = []  # device copies of the intervals: alive until the launch is enqueued (a freed block would be reused by the next copy)
    if transforms is not None and not transforms.empty:
        if transforms.utt is not None:
            d.utterance_cmvn, d.norm_means, d.norm_vars = 1, int(bool(transforms.utt.norm_means)), int(bool(transforms.utt.norm_vars))
        if transforms.glob is not None:
            gm, gs = transforms.global_stats(dev)
            d.global_mean, d.global_std = gm.data_ptr(), gs.data_ptr()
        d.global_first = int(transforms.global_first)
        if transforms.spec is not None:
            d.specaugment = 1
            for name, m, n in (("fmask", fmask, transforms.n_fmask), ("tmask", tmask, transforms.n_tmask)):
                if n == 0:
                    continue
                if not torch.is_tensor(m) or m.shape != (B, n, 2) or m.dtype != torch.int32:
                    raise ValueError("fbank: %s must be an int32 [%d, %d, 2] tensor of SpecAugment intervals" % (name, B, n))
                m = m.to(dev, non_blocking=True).contiguous()
                keep.append(m)
                setattr(d, name, m.data_ptr())
            d.n_fmask, d.n_tmask = transforms.n_fmask, transforms.n_tmask
            d.mask_mean = int(transforms.spec.mask_value is None)
            d.mask_value = 0.0 if transforms.spec.mask_value is None else float(transforms.spec.mask_value)
        nbytes = int(L.load().cst_fbank_workspace_bytes(B, max_frames))
        key = (dev.index, L.stream_ptr().value)
        ws = _ws.get(key)
        if ws is None or ws.numel() < nbytes:
            ws = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, device=dev)
            _ws[key] = ws
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    L.check(L.load().cst_fbank(ctypes.byref(d), L.stream_ptr()), "cst_fbank")
    return out, nfr


AUDIO_KEYS = ("src_audio", "src_audio_lengths", "src_audio_transforms", "src_audio_fmask", "src_audio_tmask")


def materialize(net_input, max_frames=None):
    """A collated audio-route `net_input` (keys AUDIO_KEYS, tensors already on the GPU) -> the same dict with the device features
    as `src_tokens` and their frame counts as `src_lengths`; anything else is returned unchanged."""
    if not net_input or "src_audio" not in net_input:
        return net_input
    ni = dict(net_input)
    audio, alen = ni.pop("src_audio"), ni.pop("src_audio_lengths")
    tr, fm, tm = ni.pop("src_audio_transforms", None), ni.pop("src_audio_fmask", None), ni.pop("src_audio_tmask", None)
    feats, nfr = fbank(audio, alen, tr, fm, tm, max_frames=max_frames)
    ni.pop("src_lengths", None)
    return {"src_tokens": feats, "src_lengths": nfr, **ni}
