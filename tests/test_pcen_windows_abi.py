"""honk_pcen_windows_plan / honk_pcen_windows_i16 (csrc/mfcc_stream.hip), host-only: the surface, the
plan's counts (honk_mfcc_windows_plan's for the same geometry), the argument contract (every call here
returns before it would touch the GPU: the pointers are never dereferenced), and the CPU side of the
Python surface (compute_pcen_windows, the PCEN label_stream)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from honk_amd import _native
from honk_amd import model as hm
from honk_amd import service as hs
from honk_amd.audio import AudioPreprocessor
from test_mfcc_windows_abi import _pcm, _same

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -2, -3
P = 0x1000  # a non-null stand-in for a device pointer
WIN, NFFT, HOP, NMELS = 16000, 480, 160, 40
COUNTS = ("windows", "shared", "shared_frames", "edge_frames", "frames_computed", "frames")


@pytest.fixture()
def lib():
    from honk_amd import build
    build.build()
    return _native.load()


def _n(samples, stride, window=WIN):
    return 0 if samples < window else 1 + (samples - window) // stride


def _plans(lib, samples, stride, first=0, n=None, window=WIN, n_fft=NFFT, hop=HOP, n_mels=NMELS):
    """(status, plan) of honk_pcen_windows_plan and of honk_mfcc_windows_plan for the same geometry."""
    n = _n(samples, stride, window) if n is None else n
    p, m = _native.MfccWindowsPlan(), _native.MfccWindowsPlan()
    rp = lib.honk_pcen_windows_plan(samples, window, stride, n_fft, hop, n_mels, first, n, ctypes.addressof(p))
    rm = lib.honk_mfcc_windows_plan(samples, window, stride, n_fft, hop, first, n, ctypes.addressof(m))
    return rp, p, rm, m


def _call(lib, samples=48000, window=WIN, stride=8000, first=0, n=5, n_fft=NFFT, hop=HOP, n_mels=NMELS, params=None,
          ptrs=(P,) * 5, ws_bytes=1 << 24):
    pcm, win, mel, out, ws = ptrs
    pp = ctypes.addressof(params) if params is not None else None
    return lib.honk_pcen_windows_i16(pcm, samples, window, stride, first, n, win, n_fft, hop, mel, n_mels, pp, out, ws,
                                     ws_bytes, None)


def test_symbols_exist_and_header_agrees(lib):
    src = open(os.path.join(REPO, "include", "honk_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("honk_pcen_windows_plan", "honk_pcen_windows_i16"):
        assert hasattr(lib, name) and name in _native.EXPORTS
        assert re.search(r"\b%s\s*\(" % name, src), name
    # no translation unit of its own: the frame-tile kernel is mfcc_stream.hip's, with another epilogue
    from honk_amd import build
    assert "mfcc_stream.hip" in build.SOURCES
    for s in build.SOURCES:
        assert os.path.exists(os.path.join(build.CSRC, s)), s


PLAN_INPUTS = [(15999, 160), (16000, 160), (16000 + 20 * 160, 160), (48000, 8000), (48000, 16000), (56000, 24000),
               (20000, 400)]


def test_plan_counts_equal_the_mfcc_plan(lib):
    for samples, stride in PLAN_INPUTS:
        rp, p, rm, m = _plans(lib, samples, stride)
        assert rp == 0 and rm == 0, (samples, stride)
        assert [getattr(p, k) for k in COUNTS] == [getattr(m, k) for k in COUNTS], (samples, stride)
        assert p.workspace_bytes > 0
    _, p, _, _ = _plans(lib, 16000 + 20 * 160, 160)
    assert (p.windows, p.shared_frames, p.edge_frames) == (21, 117, 84)
    # the overlapping route's workspace holds the mel-range table and one row of E per frame computed
    assert p.workspace_bytes >= (117 + 84) * NMELS * 4
    _, p, _, _ = _plans(lib, 20000, 400)
    assert p.windows == 11 and p.shared == 0 and p.frames_computed == 11 * 101
    # workspace_bytes is the call's own: it grows with n_mels on the overlapping route
    _, p20, _, _ = _plans(lib, 48000, 8000, n_mels=20)
    _, p40, _, _ = _plans(lib, 48000, 8000, n_mels=40)
    assert 0 < p20.workspace_bytes < p40.workspace_bytes


@pytest.mark.parametrize("first,n", [(0, 3), (3, 3), (18, 3), (5, 1), (0, 21), (7, 0)])
def test_plan_sub_range_counts_distinct_frames(lib, first, n):
    rp, p, rm, m = _plans(lib, 16000 + 20 * 160, 160, first, n)
    assert rp == 0 and rm == 0 and p.windows == 21
    distinct = {w + f for w in range(first, first + n) for f in range(2, 99)}
    assert p.shared_frames == len(distinct) == m.shared_frames
    assert p.edge_frames == 4 * n and p.frames_computed == len(distinct) + 4 * n
    assert p.workspace_bytes > 0
    rp, p, rm, m = _plans(lib, 48000, 8000, 1, 3)
    assert p.shared_frames == len({w * 50 + f for w in range(1, 4) for f in range(2, 99)}) == m.shared_frames


def test_argument_errors(lib):
    for null in range(5):
        ptrs = tuple(0 if i == null else P for i in range(5))
        assert _call(lib, ptrs=ptrs) == ERR_ARG
        assert b"null pointer" in lib.honk_last_error()
    assert _call(lib, samples=-1, n=0) == ERR_ARG
    assert _call(lib, first=-1) == ERR_ARG
    assert _call(lib, n=-1) == ERR_ARG
    assert b"negative" in lib.honk_last_error()
    assert _call(lib, stride=0) == ERR_ARG
    assert _call(lib, window=240) == ERR_ARG  # window <= n_fft/2: no reflect padding
    assert b"n_fft/2" in lib.honk_last_error()
    assert _call(lib, n=6) == ERR_ARG  # 48000 samples at stride 8000: 5 windows
    assert _call(lib, first=5, n=1) == ERR_ARG
    assert b"5 windows" in lib.honk_last_error()
    assert _call(lib, n_mels=0) == ERR_ARG
    assert _call(lib, n_mels=0, n=0, ptrs=(0,) * 5) == ERR_ARG  # the shape is checked before n_windows == 0
    rp, _, _, _ = _plans(lib, 48000, 8000, 0, 6)
    assert rp == ERR_ARG
    assert lib.honk_pcen_windows_plan(48000, WIN, 8000, NFFT, HOP, NMELS, 0, 5, None) == ERR_ARG
    assert lib.honk_pcen_windows_plan(48000, WIN, 8000, NFFT, HOP, 0, 0, 5, ctypes.addressof(
        _native.MfccWindowsPlan())) == ERR_ARG


def test_short_workspace_and_unsupported(lib):
    for samples, stride in [(48000, 8000), (56000, 24000), (20000, 400)]:  # overlapping, gapped, unshared
        _, p, _, _ = _plans(lib, samples, stride)
        n = _n(samples, stride)
        assert _call(lib, samples=samples, stride=stride, n=n, ws_bytes=p.workspace_bytes - 1) == ERR_WORKSPACE
        assert b"workspace" in lib.honk_last_error()
    assert _call(lib, hop=150) == ERR_UNSUPPORTED  # hop not a multiple of 16
    assert lib.honk_last_error()
    assert _call(lib, n_fft=500, window=16000) == ERR_UNSUPPORTED
    assert _call(lib, n_mels=129) == ERR_UNSUPPORTED
    assert b"mel" in lib.honk_last_error()
    assert _call(lib, samples=3 * 4000, window=4000, stride=4000, n=3, n_fft=2048, hop=16) == ERR_UNSUPPORTED
    assert b"edge frames" in lib.honk_last_error()
    assert _call(lib, n_fft=65536, hop=16384, window=40000, samples=48000, stride=8000, n=2) == ERR_UNSUPPORTED
    assert b"LDS" in lib.honk_last_error()
    # stage 2's own LDS refusal: a window of 1 + 160000 / 16 frames of 40 bands is a 1.6 MB tile
    assert _call(lib, samples=320000, window=160000, stride=160000, n=2, n_fft=32, hop=16) == ERR_UNSUPPORTED
    assert b"LDS" in lib.honk_last_error() and b"tile" in lib.honk_last_error()
    rp, _, rm, _ = _plans(lib, 48000, 8000, hop=150)
    assert rp == ERR_UNSUPPORTED and rm == ERR_UNSUPPORTED
    rp, _, _, _ = _plans(lib, 48000, 8000, n_mels=129)
    assert rp == ERR_UNSUPPORTED


BAD_PARAMS = [dict(s=0.0), dict(s=1.5), dict(eps=0.0), dict(alpha=-0.1), dict(delta=-1.0), dict(r=0.0),
              dict(power=3), dict(s=math.nan), dict(eps=math.nan), dict(alpha=math.inf), dict(delta=math.nan),
              dict(r=math.nan)]


@pytest.mark.parametrize("bad", BAD_PARAMS, ids=lambda d: "%s=%s" % next(iter(d.items())))
def test_bad_parameters_as_honk_pcen_f32(lib, bad):
    """The status and the honk_last_error text honk_pcen_f32 gives for the same parameter."""
    kw = dict(eps=1e-6, s=0.025, alpha=0.98, delta=2.0, r=0.5, power=1)
    kw.update(bad)
    params = _native.PcenParams(kw["eps"], kw["s"], kw["alpha"], kw["delta"], kw["r"], kw["power"])
    assert lib.honk_pcen_f32(P, 1, 16000, P, NFFT, HOP, P, NMELS, ctypes.addressof(params), P, None) == ERR_ARG
    want = lib.honk_last_error()
    assert want.startswith(b"pcen:")
    assert _call(lib, params=params) == ERR_ARG
    assert lib.honk_last_error() == want
    assert _call(lib, params=params, n=0, ptrs=(0,) * 5) == ERR_ARG  # checked before n_windows == 0


def test_empty_range_enqueues_nothing(lib):
    assert _call(lib, n=0, ptrs=(0,) * 5, ws_bytes=0) == 0
    assert _call(lib, samples=100, n=0, ptrs=(0,) * 5, ws_bytes=0) == 0  # shorter than a window: W = 0


# ---- the Python surface on the CPU -----------------------------------------------------------
def _service(tmp_path, no_cuda, labels=("_silence_", "_unknown_", "yes", "no")):
    torch.manual_seed(0)
    m = hm.SpeechModel(dict(hm.find_config("cnn-trad-pool2"), n_labels=len(labels)))
    fn = str(tmp_path / "m.pt")
    m.save(fn)
    return hs.TorchLabelService(fn, no_cuda=no_cuda, labels=list(labels), audio_preprocess_type="PCEN")


@pytest.mark.parametrize("params", [None, dict(power=2, s=0.1)], ids=["defaults", "power2"])
def test_cpu_compute_pcen_windows_equals_per_slice(params):
    ap = AudioPreprocessor(pcen_params=params)
    x = _pcm(3, 16000 + 2 * 4000 + 17)
    out = ap.compute_pcen_windows(torch.from_numpy(x), 4000)
    assert out.shape == (3, 101, 40) and out.dtype == torch.float32
    for w in range(3):
        ref = ap.compute_pcen(x[w * 4000:w * 4000 + 16000].astype(np.float32) / 32768.)[0]
        assert np.array_equal(out[w].numpy(), ref.numpy())
    sub = ap.compute_pcen_windows(torch.from_numpy(x), 4000, first=1, count=2)
    assert np.array_equal(sub.numpy(), out[1:].numpy())
    assert ap.compute_pcen_windows(torch.from_numpy(x), 4000, first=3, count=0).shape == (0, 101, 40)
    assert ap.compute_pcen_windows(torch.from_numpy(x[:15999]), 4000).shape == (0, 101, 40)
    with pytest.raises(ValueError):
        ap.compute_pcen_windows(torch.from_numpy(x), 4000, first=2, count=2)
    with pytest.raises(ValueError):
        ap.compute_pcen_windows(torch.from_numpy(x).float(), 4000)
    with pytest.raises(ValueError):
        ap.compute_pcen_windows(torch.from_numpy(x)[None], 4000)
    with pytest.raises(ValueError):
        ap.compute_pcen_windows(torch.from_numpy(x), 0)


def test_python_plan_query(lib):
    rc, plan = AudioPreprocessor().pcen_windows_plan(16000 + 20 * 160, 160, count=21)
    assert rc == 0 and (plan.windows, plan.shared, plan.shared_frames, plan.edge_frames) == (21, 1, 117, 84)
    rc, _ = AudioPreprocessor(n_mels=129).pcen_windows_plan(48000, 8000, count=5)
    assert rc == ERR_UNSUPPORTED


def test_cpu_pcen_label_stream_equals_label_batch(tmp_path):
    svc = _service(tmp_path, no_cuda=True)
    wav = _pcm(5, 40000).tobytes()  # 2.5 s: 4 windows at 0.5 s
    assert svc.label_stream(wav) == svc.label_batch(list(hs.stride(wav, 16000, 32000)))
    _same(svc.label_stream(wav, 100, max_windows=3), svc.label_batch(list(hs.stride(wav, 3200, 32000))))
    assert svc.listen_stream(wav) == svc.listen(wav)
