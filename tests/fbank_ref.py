"""fp64 numpy restatement of torchaudio.compliance.kaldi.fbank at the reference's call (fairseq/data/audio/audio_utils.py:80-93:
fbank(wave * 2^15, num_mel_bins=80, sample_frequency=16000), defaults otherwise, no dither).  Used by the tests and by
tools/ref_harness only; the product computes filter banks on the device (csrc/fbank.hip)."""
import numpy as np

SR, WIN, SHIFT, NFFT, NMEL = 16000, 400, 160, 512, 80
LOW_HZ, HIGH_HZ = 20.0, 8000.0
EPS = float(np.finfo(np.float32).eps)  # 1.1920929e-07


def mel(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def band_edges():
    """(left, center, right) of the 80 filters on the mel axis: mel(20) + (m, m + 1, m + 2) * delta."""
    lo, hi = mel(LOW_HZ), mel(HIGH_HZ)
    delta = (hi - lo) / (NMEL + 1)
    left = lo + np.arange(NMEL) * delta
    return left, left + delta, left + 2 * delta


def mel_weights(freqs_hz):
    """[80, len(freqs)]: max(0, min(up, down)) on the mel axis."""
    left, center, right = band_edges()
    m = mel(freqs_hz)[None, :]
    up = (m - left[:, None]) / (center - left)[:, None]
    down = (right[:, None] - m) / (right - center)[:, None]
    return np.maximum(0.0, np.minimum(up, down))


def mel_matrix():
    """[80, 257]: the weight of FFT bin k (frequency 31.25 k) in filter m; the Nyquist bin has weight 0."""
    w = mel_weights(SR / NFFT * np.arange(NFFT // 2))
    return np.concatenate([w, np.zeros((NMEL, 1))], axis=1)


def povey_window():
    n = np.arange(WIN, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2 * np.pi * n / (WIN - 1))) ** 0.85


def n_frames(num_samples):
    return 0 if num_samples < WIN else 1 + (num_samples - WIN) // SHIFT


def power_spectrum(wave):
    """[T, 257] |rfft|^2 of the processed frames of a [-1, 1) waveform."""
    x = np.asarray(wave, dtype=np.float64) * 32768.0
    T = n_frames(len(x))
    if T == 0:
        return np.zeros((0, NFFT // 2 + 1))
    idx = np.arange(T)[:, None] * SHIFT + np.arange(WIN)[None, :]
    fr = x[idx]
    fr = fr - fr.mean(axis=1, keepdims=True)
    prev = np.concatenate([fr[:, :1], fr[:, :-1]], axis=1)
    fr = (fr - 0.97 * prev) * povey_window()[None, :]
    spec = np.fft.rfft(fr, n=NFFT, axis=1)
    return spec.real ** 2 + spec.imag ** 2


def mel_energies(wave):
    return power_spectrum(wave) @ mel_matrix().T


def fbank(wave):
    """[T, 80] fp64 log mel energies."""
    return np.log(np.maximum(mel_energies(wave), EPS))
