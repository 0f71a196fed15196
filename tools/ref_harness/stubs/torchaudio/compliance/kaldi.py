"""torchaudio.compliance.kaldi.fbank at the reference's call (num_mel_bins=80, sample_frequency=16000, other arguments at their
defaults, dither 0 as the reference's prep uses it) -> tests/fbank_ref.fbank, returned as float32 like torchaudio's."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..", "..", "..", "..", "tests")))
import fbank_ref  # noqa: E402


def fbank(waveform, num_mel_bins=23, sample_frequency=16000.0, **kw):
    assert num_mel_bins == 80 and sample_frequency == 16000 and not kw, "stub covers the reference's call only"
    x = waveform.numpy().astype(np.float64)
    assert x.ndim == 2 and x.shape[0] == 1
    return torch.from_numpy(fbank_ref.fbank(x[0] / 32768.0).astype(np.float32))
