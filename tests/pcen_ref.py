"""Float64 restatement of the PCEN front end (TEST INFRASTRUCTURE ONLY).

PARITY UNPINNED: the reference's ``pcen`` package (``StreamingPCENTransform``,
utils/manage_audio.py:28,44-47) is not installed and the reference holds no PCEN
fixtures, so this restates the published algorithm (Wang et al. 2017) only, with the
defaults of include/honk_hip.h:

    STFT as the MFCC's (centre reflect padding, periodic Hann, n_fft, hop)
    E[t][m] = sum_k melw[m][k] |X_t[k]|^power          (Slaney mel basis, area-normalised)
    M[0] = E[0];  M[t] = (1 - s) M[t-1] + s E[t]       (per band, reset for every clip)
    out[t][m] = (E / (M + eps)^alpha + delta)^r - delta^r

The DFT is an explicit complex-exponential matrix product, the mel basis is
oracle.mfcc_ref.mel_basis and the recurrence a plain Python loop: no code shared with
honk_amd/audio.py.  Also the shared inputs of the PCEN tests.
"""
import functools

import numpy as np

from oracle import mfcc_ref
from test_mfcc_service import _speechlike as speechlike

DEFAULTS = dict(eps=1e-6, s=0.025, alpha=0.98, delta=2.0, r=0.5, power=1)


def window(n_fft=480):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)


def pcen(y, sr=16000, n_fft=480, hop=160, n_mels=40, fmin=20.0, fmax=4000.0, **params):
    """y: [S] float -> [frames, n_mels] float64."""
    p = dict(DEFAULTS, **params)
    y = np.asarray(y, dtype=np.float64)
    pad = n_fft // 2
    yp = np.concatenate([y[1:pad + 1][::-1], y, y[-pad - 1:-1][::-1]])
    frames = 1 + (len(yp) - n_fft) // hop
    n = np.arange(n_fft)
    k = np.arange(1 + n_fft // 2)
    basis = np.exp(-2j * np.pi * np.outer(n, k) / n_fft)
    fr = np.stack([yp[t * hop:t * hop + n_fft] * window(n_fft) for t in range(frames)])
    E = (np.abs(fr @ basis) ** p["power"]) @ mfcc_ref.mel_basis(sr, n_fft, n_mels, fmin, fmax).T
    out = np.zeros_like(E)
    for m in range(n_mels):
        M = E[0][m]
        for t in range(frames):
            if t > 0:
                M = (1.0 - p["s"]) * M + p["s"] * E[t][m]
            out[t][m] = (E[t][m] / (M + p["eps"]) ** p["alpha"] + p["delta"]) ** p["r"] - p["delta"] ** p["r"]
    return out


def clips(n=16000):
    """The inputs of the PCEN checks, [8][n] float32: five speech-like clips, an all-zero clip,
    an onset clip (8000 zeros, then speech: PCEN's largest gain) and a quiet one (1e-3 x)."""
    ys = [speechlike(s, n) for s in range(5)]
    onset = speechlike(5, n)
    onset[:min(8000, n // 2)] = 0.0
    return np.stack(ys + [np.zeros(n, np.float32), onset, (1e-3 * speechlike(6, n)).astype(np.float32)])


ZERO_CLIP = 5


@functools.lru_cache(maxsize=None)
def _ref_cached(n, n_fft, n_mels, items):
    out = np.stack([pcen(y, n_fft=n_fft, n_mels=n_mels, **dict(items)) for y in clips(n)])
    out.setflags(write=False)
    return out


def ref_clips(n=16000, n_fft=480, n_mels=40, **params):
    """pcen() of clips(n), computed once per argument set and shared (read-only)."""
    return _ref_cached(n, n_fft, n_mels, tuple(sorted(params.items())))


def check(got, ref, rel):
    """Per clip: |got - ref| <= rel * max(max|ref clip|, 1e-6); returns the largest error / scale."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all()
    worst = 0.0
    for i in range(len(ref)):
        scale = max(np.abs(ref[i]).max(), 1e-6)
        err = np.abs(got[i] - ref[i]).max() / scale
        worst = max(worst, err)
        assert err <= rel, (i, err, rel)
    return worst
