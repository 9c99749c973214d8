"""The audio front ends off 16000/480/160/40: one table for the host-only plan tests
(test_frontend_geometry_plan.py) and the GPU tests (test_gpu_frontend_geometry.py).

A batch case is a shape (S samples, n_fft, hop, n_mels, n_dct) of honk_mfcc_f32 / honk_pcen_f32
with the route the table claims for each (csrc/mfcc_spectrum.h front_plan: "mfma" needs frames <= 112,
n_fft % 16 == 0, hop % 4 == 0 and an LDS plan within 160 KiB; "valu" is every other shape and every
shape under HONK_MFCC_VALU=1) and the reason it is in the table.  A windows case is a shape of
honk_mfcc_windows_i16 (csrc/mfcc_stream.hip) with one shared and one unshared stride.

Inputs of a case: four clips of pcen_ref.clips(S) -- speech-like, all-zero, an onset after zeros and
1e-3 x speech-like (three where a case says why).  Reference: the float64 oracles oracle/mfcc_ref.py
and tests/pcen_ref.py.

Bound of a case (bound()): 16 * e32(case), never above 1e-4, relative to max(max|ref clip|, 1e-6),
rtol = 0.  e32 is the error of oracle/frontend_f32_sim.py -- the chain restated in float32, one
legitimate order of fp32 arithmetic -- against the float64 oracle on the case's own clips.  The kernels
use other orders (fmaf chains, k in steps of 4 on the MFMA, LDS-atomic arrival order, device sincosf /
logf); the factor 16 leaves an order of magnitude for that.  The cap keeps the bound ten times under
the smallest effect of a real mistake found so far (a symmetric Hann window: 1.4e-3).  No route needs
a factor of its own ("The audio front ends off 16000 / 480 / 160 / 40").
"""
import functools

import numpy as np

import pcen_ref
from oracle import frontend_f32_sim as sim
from oracle import mfcc_ref

SR, FMIN, FMAX = 16000, 20.0, 4000.0
FACTOR, CAP = sim.FACTOR, sim.CAP  # 16 and 1e-4
CLIPS = (0, pcen_ref.ZERO_CLIP, 6, 7)  # of pcen_ref.clips: speech-like, all-zero, onset, 1e-3 x speech-like
ZERO = 1                               # the all-zero clip's place among a case's clips
FRONTS = ("mfcc", "pcen")
MAX_BATCH = 65535                      # clips per C call (the Python paths loop over chunks of it)


class Case:
    def __init__(self, id, S, n_fft, hop, n_mels, n_dct, mfcc, pcen, why, clips=None):
        self.clips = CLIPS if clips is None else clips  # places in pcen_ref.clips(S); the all-zero one second
        self.id, self.S, self.n_fft, self.hop, self.n_mels, self.n_dct = id, S, n_fft, hop, n_mels, n_dct
        self.route = {"mfcc": mfcc, "pcen": pcen}
        self.why = why
        self.n_bins = n_fft // 2 + 1
        self.frames = 1 + (S + 2 * (n_fft // 2) - n_fft) // hop  # of the centre-padded clip

    @property
    def shape(self):
        return dict(n_fft=self.n_fft, hop=self.hop, n_mels=self.n_mels)

    @property
    def expressible(self):
        """AudioPreprocessor makes hop = 16 * hop_ms only; other hops go through the C ABI."""
        return self.hop % 16 == 0

    def __repr__(self):
        return self.id


def _c(id, S, n_fft, hop, n_mels, n_dct, mfcc, pcen, why, clips=None):
    return Case(id, S, n_fft, hop, n_mels, n_dct, mfcc, pcen, why, clips)


M, V = "mfma", "valu"

# every distinct (H, W) with (H - 1) * 160 > 240 of res_geometry_cases, cnn_geometry_cases and
# train_geometry_cases (CASES and STEPS); test_frontend_geometry_plan checks the list against them
NETWORK_HW = [
    (3, 4), (3, 220), (3, 224), (3, 260), (4, 4), (4, 8), (4, 12), (5, 5), (5, 7), (5, 8), (5, 256), (6, 44), (7, 8),
    (7, 12), (7, 40), (9, 33), (9, 42), (14, 20), (16, 33), (16, 40), (17, 5), (19, 11), (21, 16), (21, 17), (25, 13),
    (25, 20), (26, 20), (30, 26), (32, 34), (33, 37), (34, 20), (35, 20), (37, 27), (37, 41), (37, 42), (37, 43),
    (45, 40), (48, 41), (49, 20), (50, 20), (51, 39), (52, 40), (61, 40), (70, 40), (72, 40), (98, 40), (100, 40),
    (101, 38), (101, 39), (101, 41), (102, 40), (103, 40), (112, 40)]
# at n_fft 480 / hop 160 the MFMA MFCC plan takes 59 bands in 160 KiB and the fused PCEN 48 (pinned by
# test_lds_boundaries); every H here is within the 112-frame limit
# 3 x 4 takes three clips: on 3 frames of 4 bands the 1e-3 x clip's MFCC is all offset (max|ref| 32 from
# log 1e-6), and a one-sample shift of its stationary signal moves it by 7 bounds only, under the 10 the
# separation condition asks of every clip of a case
NETWORK_CLIPS = {(3, 4): (0, pcen_ref.ZERO_CLIP, 6)}
NETWORK = [_c(f"net-{H}x{W}", (H - 1) * 160, 480, 160, W, W, M if W <= 59 else V, M if W <= 48 else V,
              f"a model input of {H} x {W}", NETWORK_CLIPS.get((H, W))) for H, W in NETWORK_HW]

BATCH = [
    _c("default", 16000, 480, 160, 40, 40, M, M, "the reference shape: 101 frames, VALU's last workgroup holds one"),
    _c("51x20", 8000, 480, 160, 20, 20, M, M, "the 51 x 20 model input"),
    _c("frames112", 17760, 480, 160, 40, 40, M, M, "frame limit: 112 frames, the last MFMA shape"),
    _c("frames113", 17920, 480, 160, 40, 40, V, V, "frame limit: 113 frames, the first VALU shape"),
    _c("frames100", 15840, 480, 160, 40, 40, M, M, "100 frames: under HONK_MFCC_VALU=1 every workgroup is full"),
    _c("mfcc-lds-in", 16000, 512, 160, 56, 56, M, V, "160 KiB MFCC plan: 162916 B, the most bands at n_fft 512"),
    _c("mfcc-lds-out", 16000, 512, 160, 57, 57, V, V, "160 KiB MFCC plan: one band more"),
    _c("pcen-lds-in", 16000, 512, 160, 45, 45, M, M, "160 KiB PCEN plan: the most bands PCEN fuses at n_fft 512"),
    _c("pcen-lds-out", 16000, 512, 160, 46, 46, M, V, "160 KiB PCEN plan: one band more"),
    _c("under64k", 4000, 256, 64, 20, 20, M, M, "MFCC plan under 64 KiB: no shared-memory opt-in call"),
    _c("nfft400", 16000, 400, 160, 40, 40, M, M, "librosa's other usual n_fft; 400 = 25 * 16, so the MFMA route"),
    _c("nfft488", 16000, 488, 160, 40, 40, V, V, "n_fft % 16 != 0 (n_fft % 8 == 0)"),
    _c("hop50", 16000, 480, 50, 40, 40, V, V, "hop % 4 != 0 (321 frames)"),
    _c("hop100", 8050, 480, 100, 40, 40, M, M, "hop % 4 == 0, hop % 16 != 0, S % hop != 0 (81 frames)"),
    _c("nfft128-hop160", 8000, 128, 160, 20, 20, M, M, "n_fft < hop: samples between the frames are never read"),
    _c("odd481", 16000, 481, 160, 40, 40, V, V, "odd n_fft: 100 frames, not 1 + S / hop"),
    _c("odd255", 4000, 255, 64, 20, 20, V, V, "odd n_fft, small"),
    _c("shortest", 241, 480, 160, 40, 40, M, M, "the shortest legal clip: 2 frames, both reflections in one frame"),
    _c("dct13", 16000, 480, 160, 40, 13, M, M, "fewer DCT rows than bands"),
    _c("dct1", 16000, 480, 160, 40, 1, M, M, "one DCT row"),
    _c("oneband", 16000, 480, 160, 1, 1, M, M, "one mel band"),
    _c("emptybands", 4000, 256, 128, 80, 13, M, M, "3 all-zero mel rows: their log-mel entries are exactly 0"),
    _c("nfft1024", 16000, 1024, 160, 40, 40, V, V, "n_fft % 16 == 0 but past the MFMA LDS plan at any band count"),
    _c("chunk", 64, 32, 16, 4, 4, M, M, "the Python chunk loop: B = 65537 clips of 64 samples"),
] + NETWORK
BY_ID = {c.id: c for c in BATCH}
assert len(BY_ID) == len(BATCH)
CHUNK_B = MAX_BATCH + 2
CHUNK_ROWS = (0, MAX_BATCH - 1, MAX_BATCH, MAX_BATCH + 1)

# boundary -> (case inside, case outside, front the boundary belongs to)
BOUNDARIES = {
    "112 frames": ("frames112", "frames113", "mfcc"),
    "160 KiB MFCC plan": ("mfcc-lds-in", "mfcc-lds-out", "mfcc"),
    "160 KiB PCEN plan": ("pcen-lds-in", "pcen-lds-out", "pcen"),
    "n_fft % 16": ("nfft400", "nfft488", "mfcc"),
    "hop % 4": ("hop100", "hop50", "mfcc"),
    "64 KiB opt-in": ("under64k", "default", "mfcc"),
    "full last VALU workgroup": ("frames100", "default", "mfcc"),
    "even n_fft": ("default", "odd481", "mfcc"),
}
# lds_bytes the plan query must report (the arithmetic of mfcc_spectrum.h front_plan, by hand)
PINNED_LDS = {("mfcc-lds-in", "mfcc"): 162916, ("pcen-lds-in", "pcen"): 162544, ("under64k", "mfcc"): 52308,
              ("default", "mfcc"): 136164}


class WinCase:
    """window samples per window at n_fft / hop; strides (shared: a multiple of hop, unshared: not);
    kernel False: honk_mfcc_windows_plan / _i16 refuse the shape and compute_mfccs_windows falls back
    to the per-window kernel."""

    def __init__(self, id, window, n_fft, hop, n_mels, n_dct, n_windows, why, kernel=True, shared=True):
        self.id, self.window, self.n_fft, self.hop, self.n_mels, self.n_dct = id, window, n_fft, hop, n_mels, n_dct
        self.n_windows, self.why, self.kernel, self.shared = n_windows, why, kernel, shared
        q = max(1, (window // hop) // 4)
        self.strides = (q * hop, q * hop + 7)
        self.frames = 1 + window // hop

    def __repr__(self):
        return self.id


WINDOWS = [
    WinCase("win8000", 8000, 480, 160, 40, 40, 5, "window = 8000: 51 frames"),
    WinCase("win16077", 16077, 480, 160, 40, 40, 4, "window % hop != 0"),
    WinCase("512-160", 16000, 512, 160, 40, 40, 3, "n_fft = 512: 2 head and 2 tail frames, pad 256"),
    WinCase("320-80", 8000, 320, 80, 40, 40, 5, "hop = 80: the LDS slot stride is 88 floats"),
    WinCase("640-320", 16000, 640, 320, 40, 40, 4, "hop = 320: one edge frame per side"),
    WinCase("256-64", 4000, 256, 64, 20, 20, 9, "window = 4000 at 256 / 64"),
    WinCase("128-160", 8000, 128, 160, 20, 20, 5, "n_fft < hop"),
    WinCase("dct13", 8000, 480, 160, 40, 13, 4, "n_dct = 13"),
    WinCase("80bands", 4000, 256, 64, 80, 13, 5, "80 bands at n_fft 256: the empty rows of mel_range_kernel"),
    WinCase("128bands", 8000, 480, 160, 128, 40, 3, "128 bands, the most the kernel takes"),
    WinCase("129bands", 8000, 480, 160, 129, 40, 3, "129 bands: the Python fallback", kernel=False),
    WinCase("2048-16", 4000, 2048, 16, 40, 40, 3, "more than 32 edge frames per side: plan refusal, then fallback",
            kernel=False),
    WinCase("win300", 300, 480, 160, 40, 40, 9, "no interior frame: unshared at either stride", shared=False),
    WinCase("800-160", 16000, 800, 160, 40, 40, 3, "3 edge frames per side: 10 groups per edge tile, FT % gs != 0"),
    WinCase("1024-128", 8192, 1024, 128, 40, 40, 3, "4 edge frames per side, 65 frames"),
    WinCase("win16240", 16240, 480, 160, 40, 40, 3, "2 head and 1 tail edge frame: 102 frames, fhi = 100"),
]
WIN_BY_ID = {c.id: c for c in WINDOWS}


# ---- inputs and references (computed once, read-only) ------------------------------------------------
@functools.lru_cache(maxsize=None)
def _clips(S, which):
    ys = np.ascontiguousarray(pcen_ref.clips(S)[list(which)])
    ys.setflags(write=False)
    return ys


def clips(case):
    return _clips(case.S, tuple(case.clips))


def oracle(front, y, case, n_dct=None):
    if front == "mfcc":
        return mfcc_ref.mfcc(y, SR, case.n_fft, case.hop, case.n_mels, case.n_dct if n_dct is None else n_dct,
                             FMIN, FMAX)
    return pcen_ref.pcen(y, SR, case.n_fft, case.hop, case.n_mels, FMIN, FMAX)


@functools.lru_cache(maxsize=None)
def refs(case_id, front):
    """The float64 oracle on the case's clips: [clips][frames][n_dct | n_mels]."""
    case = BY_ID[case_id]
    out = np.stack([oracle(front, y, case) for y in clips(case)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def e32(case_id, front):
    case = BY_ID[case_id]
    kw = dict(case.shape, sr=SR, fmin=FMIN, fmax=FMAX)
    if front == "mfcc":
        kw["n_dct"] = case.n_dct
    return sim.e32(front, clips(case), refs(case_id, front), **kw)


def bound_of(e):
    return sim.bound(e)


def bound(case_id, front):
    return bound_of(e32(case_id, front))


def errors(got, ref):
    """Per clip max|got - ref| / max(max|ref clip|, 1e-6)."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return [sim.rel_err(g, r) for g, r in zip(got, ref)]


def chunk_clips():
    """[CHUNK_B][64]: the chunk case's four clips in turn, each row at a gain of its own."""
    ys = clips(BY_ID["chunk"])
    i = np.arange(CHUNK_B)
    return (ys[i % len(ys)] * (0.5 + 0.5 * (i % 1000) / 1000.0).astype(np.float32)[:, None]).astype(np.float32)


# ---- the float64 oracle in stages, for named mutations (the separation condition) --------------------
MUTATIONS = ("symmetric_pad", "symmetric_hann", "late_frames", "mel_shift", "bin_dropped")


def staged(front, y, case, mutation=None):
    """oracle(front, y, case) restated stage by stage (equal to it for mutation None, which the plan
    test checks), with one named mistake applied:
      symmetric_pad   numpy 'symmetric' padding (the edge sample repeated) instead of 'reflect'
      symmetric_hann  the symmetric Hann window (denominator n_fft - 1) instead of the periodic one
      late_frames     every frame starts one sample late
      mel_shift       the mel basis shifted up by one bin
      bin_dropped     one in-band bin (the middle one of those with a weight) left out of the mel product"""
    assert mutation is None or mutation in MUTATIONS
    N, hop = case.n_fft, case.hop
    y = np.asarray(y, dtype=np.float64)
    pad = N // 2
    if mutation == "symmetric_pad":
        yp = np.concatenate([y[:pad][::-1], y, y[-pad:][::-1]])
    else:
        yp = np.concatenate([y[1:pad + 1][::-1], y, y[-pad - 1:-1][::-1]])
    frames = 1 + (len(yp) - N) // hop
    n = np.arange(N)
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / (N - 1 if mutation == "symmetric_hann" else N))
    if mutation == "late_frames":
        yp = np.append(yp, 0.0)[1:]
    basis = np.exp(-2j * np.pi * np.outer(n, np.arange(1 + N // 2)) / N)
    fr = np.stack([yp[t * hop:t * hop + N] * win for t in range(frames)])
    mel = mfcc_ref.mel_basis(SR, N, case.n_mels, FMIN, FMAX)
    if mutation == "mel_shift":
        mel = np.concatenate([np.zeros((case.n_mels, 1)), mel[:, :-1]], axis=1)
    if mutation == "bin_dropped":
        inband = np.flatnonzero(mel.any(axis=0))
        mel = mel.copy()
        mel[:, inband[len(inband) // 2]] = 0.0
    if front == "mfcc":
        e = (np.abs(fr @ basis) ** 2) @ mel.T
        logmel = np.where(e > 0, np.log(np.where(e > 0, e, 1.0)), e)
        return logmel @ mfcc_ref.dct_basis(case.n_dct, case.n_mels).T
    p = pcen_ref.DEFAULTS
    E = (np.abs(fr @ basis) ** p["power"]) @ mel.T
    out = np.zeros_like(E)
    Mt = E[0].copy()
    for t in range(frames):
        if t > 0:
            Mt = (1.0 - p["s"]) * Mt + p["s"] * E[t]
        out[t] = (E[t] / (Mt + p["eps"]) ** p["alpha"] + p["delta"]) ** p["r"] - p["delta"] ** p["r"]
    return out


# ---- windows cases -----------------------------------------------------------------------------------
def recording(case, stride):
    """An int16 recording of exactly case.n_windows windows at this stride (speech-like, seeded by the
    case's place in the table)."""
    n = case.window + (case.n_windows - 1) * stride
    y = pcen_ref.speechlike(40 + WINDOWS.index(case), n)
    return (np.clip(y, -1, 1) * 32767).astype(np.int16)


def window_refs(case, x, stride):
    return [mfcc_ref.mfcc(x[w * stride:w * stride + case.window] / 32768., SR, case.n_fft, case.hop, case.n_mels,
                          case.n_dct, FMIN, FMAX) for w in range(case.n_windows)]


def window_e32(case, x, stride, refs_):
    kw = dict(sr=SR, n_fft=case.n_fft, hop=case.hop, n_mels=case.n_mels, n_dct=case.n_dct, fmin=FMIN, fmax=FMAX)
    ys = [(x[w * stride:w * stride + case.window].astype(np.float32) / np.float32(32768.))
          for w in range(case.n_windows)]
    return sim.e32("mfcc", ys, refs_, **kw)
