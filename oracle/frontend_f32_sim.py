"""A float32 restatement of the audio front ends (TEST INFRASTRUCTURE ONLY).

What the error of "the same chain in float32" is, so that a test of the HIP front ends
(csrc/mfcc.hip, csrc/pcen.hip, csrc/mfcc_stream.hip) and of the numpy path can ask for a
bound that follows from the number format and not from what the code under test gives:

    e32(case) = max over the case's clips of  max|f32 chain - float64 oracle| / max(max|oracle clip|, 1e-6)

with the float64 oracles oracle/mfcc_ref.py and tests/pcen_ref.py.  Every stage is rounded to
float32 as a straightforward implementation would: the clip, the periodic Hann window and the
mel / DCT tables as float32 tables; cos and sin of the float32 angle 2*pi*t/N as float32; the
direct DFT as two float32 matrix products over the table entry (n*k) mod N; |X|^2 (or its
square root), the mel product, ``log`` and the DCT in float32; PCEN's recurrence as a float32
loop and its powers as float32 ``np.power``.  This is one legitimate order of float32
arithmetic.  The kernels use others (fmaf chains, k in steps of 4 on the MFMA, LDS-atomic
arrival order, the device's sincosf / logf / exp2f), which is what the factor between e32 and
the asserted bound is for (tests/frontend_geometry_cases.py).

No code shared with honk_amd/audio.py and none with the kernels; the tables come from
oracle/mfcc_ref.py (float64, rounded once).
"""
import numpy as np

from oracle import mfcc_ref

F = np.float32
FACTOR = 16.0   # e32 -> asserted bound: an order of magnitude for the kernels' other orders of fp32 arithmetic
CAP = 1e-4      # ... and never above this: ten times under the smallest effect of a real mistake found (1.4e-3)
PCEN_DEFAULTS = dict(eps=1e-6, s=0.025, alpha=0.98, delta=2.0, r=0.5, power=1)


def _frames(y, n_fft, hop):
    """Centre reflect padding and framing of a float32 clip: [frames][n_fft] float32 (exact)."""
    y = np.asarray(y, dtype=F)
    pad = n_fft // 2
    idx = np.arange(-pad, len(y) + pad)
    idx = np.where(idx < 0, -idx, np.where(idx >= len(y), 2 * len(y) - 2 - idx, idx))
    yp = y[idx]
    n = 1 + (len(yp) - n_fft) // hop
    return yp[np.arange(n_fft)[None, :] + hop * np.arange(n)[:, None]]


def spectrum(y, n_fft, hop):
    """(re, im) of the windowed frames' rDFT, [frames][n_fft//2+1] float32 each."""
    t = np.arange(n_fft)
    win = (0.5 - 0.5 * np.cos(2.0 * np.pi * t / n_fft)).astype(F)
    ang = F(6.283185307179586) * t.astype(F) / F(n_fft)
    cos_t, sin_t = np.cos(ang), np.sin(ang)
    assert ang.dtype == F and cos_t.dtype == F and sin_t.dtype == F
    nk = (t[:, None] * np.arange(1 + n_fft // 2)[None, :]) % n_fft
    fr = _frames(y, n_fft, hop) * win[None, :]
    re, im = fr @ cos_t[nk], fr @ (-sin_t[nk])
    assert re.dtype == F and im.dtype == F
    return re, im


def mfcc(y, sr=16000, n_fft=480, hop=160, n_mels=40, n_dct=40, fmin=20.0, fmax=4000.0):
    """y: [S] -> [frames][n_dct] float32, every stage in float32."""
    re, im = spectrum(y, n_fft, hop)
    power = re * re + im * im
    mel = power @ mfcc_ref.mel_basis(sr, n_fft, n_mels, fmin, fmax).astype(F).T
    pos = mel > 0
    mel[pos] = np.log(mel[pos])
    out = mel @ mfcc_ref.dct_basis(n_dct, n_mels).astype(F).T
    assert out.dtype == F
    return out


def pcen(y, sr=16000, n_fft=480, hop=160, n_mels=40, fmin=20.0, fmax=4000.0, **params):
    """y: [S] -> [frames][n_mels] float32, every stage in float32."""
    p = dict(PCEN_DEFAULTS, **params)
    re, im = spectrum(y, n_fft, hop)
    mag = re * re + im * im
    if p["power"] == 1:
        mag = np.sqrt(mag)
    E = mag @ mfcc_ref.mel_basis(sr, n_fft, n_mels, fmin, fmax).astype(F).T
    s, a = F(p["s"]), F(1.0) - F(p["s"])
    M = np.empty_like(E)
    M[0] = E[0]
    for t in range(1, len(E)):
        M[t] = a * M[t - 1] + s * E[t]
    delta, r = F(p["delta"]), F(p["r"])
    out = np.power(E * np.power(M + F(p["eps"]), -F(p["alpha"])) + delta, r) - np.power(delta, r)
    assert out.dtype == F
    return out


def rel_err(got, ref):
    """max|got - ref| / max(max|ref|, 1e-6) of one clip."""
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / max(np.abs(ref).max(), 1e-6))


def e32(front, clips, refs, **shape):
    """e32 of a case: ``front`` "mfcc" or "pcen", ``clips`` [n][S], ``refs`` the float64 oracle's
    outputs for them, ``shape`` the keywords of mfcc() / pcen()."""
    fn = {"mfcc": mfcc, "pcen": pcen}[front]
    return max(rel_err(fn(y, **shape), ref) for y, ref in zip(clips, refs))


def bound(e, factor=FACTOR):
    """The bound a front-end test asserts for a case whose restatement error is e: factor * e, never
    above CAP, relative to max(max|ref clip|, 1e-6), rtol = 0."""
    return min(factor * e, CAP)
