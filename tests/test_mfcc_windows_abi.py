"""honk_mfcc_windows_plan / honk_mfcc_windows_i16 (csrc/mfcc_stream.hip), host-only: the plan's
counts, the argument contract (every call here returns before it would touch the GPU: the pointers
are never dereferenced), and the CPU side of the Python surface (compute_mfccs_windows,
label_stream, listen_stream, StreamListener)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from honk_amd import _native
from honk_amd import model as hm
from honk_amd import service as hs
from honk_amd.audio import AudioPreprocessor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -2, -3
P = 0x1000  # a non-null stand-in for a device pointer
WIN, NFFT, HOP = 16000, 480, 160


@pytest.fixture()
def lib():
    from honk_amd import build
    build.build()
    return _native.load()


def _plan(lib, samples, stride, first=0, n=None, window=WIN, n_fft=NFFT, hop=HOP):
    p = _native.MfccWindowsPlan()
    if n is None:
        n = 0 if samples < window else 1 + (samples - window) // stride
    rc = lib.honk_mfcc_windows_plan(samples, window, stride, n_fft, hop, first, n, ctypes.addressof(p))
    return rc, p


def _call(lib, samples=48000, window=WIN, stride=8000, first=0, n=5, n_fft=NFFT, hop=HOP, n_mels=40, n_dct=40,
          ptrs=(P,) * 6, ws_bytes=1 << 20):
    pcm, win, mel, dct, out, ws = ptrs
    return lib.honk_mfcc_windows_i16(pcm, samples, window, stride, first, n, win, n_fft, hop, mel, n_mels, dct, n_dct,
                                     out, ws, ws_bytes, None)


def test_symbols_exist_and_header_agrees(lib):
    src = open(os.path.join(REPO, "include", "honk_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("honk_mfcc_windows_plan", "honk_mfcc_windows_i16"):
        assert hasattr(lib, name) and name in _native.EXPORTS
        assert re.search(r"\b%s\s*\(" % name, src), name
    assert "honk_mfcc_windows_plan_t" in src
    # the struct the binding mirrors: five int64 counts, two int32
    assert ctypes.sizeof(_native.MfccWindowsPlan) == 5 * 8 + 2 * 4
    from honk_amd import build
    assert "mfcc_stream.hip" in build.SOURCES


def test_plan_counts(lib):
    rc, p = _plan(lib, 15999, 160)
    assert rc == 0 and p.windows == 0 and p.frames_computed == 0
    rc, p = _plan(lib, 16000, 160)
    assert rc == 0 and (p.windows, p.shared, p.shared_frames, p.edge_frames, p.frames_computed) == (1, 1, 97, 4, 101)
    assert p.frames == 101
    rc, p = _plan(lib, 16000 + 20 * 160, 160)
    assert rc == 0 and (p.windows, p.shared_frames, p.edge_frames) == (21, 20 + 97, 84)
    assert p.frames_computed == 20 + 97 + 84
    rc, p = _plan(lib, 48000, 8000)
    assert rc == 0 and (p.windows, p.shared_frames, p.edge_frames) == (5, 4 * 50 + 97, 20)
    rc, p = _plan(lib, 48000, 16000)
    assert rc == 0 and (p.windows, p.shared, p.shared_frames, p.edge_frames) == (3, 1, 3 * 97, 12)
    rc, p = _plan(lib, 56000, 24000)  # gapped: samples 16000..23999 belong to no window
    assert rc == 0 and (p.windows, p.shared, p.shared_frames, p.edge_frames) == (2, 1, 2 * 97, 8)
    rc, p = _plan(lib, 20000, 400)
    assert rc == 0 and p.windows == 11 and p.shared == 0 and p.shared_frames == 0 and p.edge_frames == 0
    assert p.frames_computed == p.windows * 101
    assert p.workspace_bytes > 0


@pytest.mark.parametrize("first,n", [(0, 3), (3, 3), (18, 3), (5, 1), (0, 21), (7, 0)])
def test_plan_sub_range_counts_distinct_frames(lib, first, n):
    """The shared count of a window range = the distinct global frames j = w q + f (f in 2..98) it uses."""
    rc, p = _plan(lib, 16000 + 20 * 160, 160, first, n)
    assert rc == 0 and p.windows == 21
    distinct = {w * 1 + f for w in range(first, first + n) for f in range(2, 99)}
    assert p.shared_frames == len(distinct)
    assert p.edge_frames == 4 * n and p.frames_computed == len(distinct) + 4 * n
    rc, p = _plan(lib, 48000, 8000, 1, 3)
    assert p.shared_frames == len({w * 50 + f for w in range(1, 4) for f in range(2, 99)})


def test_argument_errors(lib):
    for null in range(6):
        ptrs = tuple(0 if i == null else P for i in range(6))
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
    assert _call(lib, n_mels=0) == ERR_ARG and _call(lib, n_dct=0) == ERR_ARG
    rc, _ = _plan(lib, 48000, 8000, 0, 6)
    assert rc == ERR_ARG
    assert lib.honk_mfcc_windows_plan(48000, WIN, 8000, NFFT, HOP, 0, 5, None) == ERR_ARG


def test_short_workspace_and_unsupported(lib):
    rc, p = _plan(lib, 48000, 8000)
    assert _call(lib, ws_bytes=p.workspace_bytes - 1) == ERR_WORKSPACE
    assert b"workspace" in lib.honk_last_error()
    assert _call(lib, hop=150) == ERR_UNSUPPORTED  # hop not a multiple of 16
    assert lib.honk_last_error()
    assert _call(lib, n_fft=500, window=16000) == ERR_UNSUPPORTED
    assert _call(lib, n_mels=129) == ERR_UNSUPPORTED
    assert b"mel" in lib.honk_last_error()
    assert _call(lib, n_fft=65536, hop=16384, window=40000, samples=48000, stride=8000, n=2) == ERR_UNSUPPORTED
    assert b"LDS" in lib.honk_last_error()
    rc, _ = _plan(lib, 48000, 8000, hop=150)
    assert rc == ERR_UNSUPPORTED


def test_empty_range_enqueues_nothing(lib):
    assert _call(lib, n=0, ptrs=(0,) * 6, ws_bytes=0) == 0
    assert _call(lib, samples=100, n=0, ptrs=(0,) * 6, ws_bytes=0) == 0  # shorter than a window: W = 0


# ---- the Python surface on the CPU -----------------------------------------------------------
def _speechlike(seed, n=16000):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    y = 0.05 * rng.standard_normal(n)
    for f in rng.uniform(100, 3500, 6):
        y += rng.uniform(0.02, 0.2) * np.sin(2 * np.pi * f * t + rng.uniform(0, 6.3))
    return np.clip(y, -1, 1).astype(np.float32)


def _pcm(seed, n):
    return (np.clip(_speechlike(seed, n), -1, 1) * 32767).astype(np.int16)


def _service(tmp_path, no_cuda, labels=("_silence_", "_unknown_", "yes", "no")):
    torch.manual_seed(0)
    cfg = dict(hm.find_config("cnn-trad-pool2"), n_labels=len(labels))
    m = hm.SpeechModel(cfg)
    fn = str(tmp_path / "m.pt")
    m.save(fn)
    return hs.TorchLabelService(fn, no_cuda=no_cuda, labels=list(labels))


def _same(got, want, tol=1e-6):
    assert [g[0] for g in got] == [w[0] for w in want]
    assert all(abs(g[1] - w[1]) <= tol for g, w in zip(got, want))


def test_cpu_compute_mfccs_windows_equals_per_slice():
    ap = AudioPreprocessor()
    x = _pcm(3, 16000 + 2 * 4000 + 17)
    out = ap.compute_mfccs_windows(torch.from_numpy(x), 4000)
    assert out.shape == (3, 101, 40) and out.dtype == torch.float32
    for w in range(3):
        ref = ap.compute_mfccs(x[w * 4000:w * 4000 + 16000].astype(np.float32) / 32768.).squeeze(2)
        assert np.array_equal(out[w].numpy(), ref)
    sub = ap.compute_mfccs_windows(torch.from_numpy(x), 4000, first=1, count=2)
    assert np.array_equal(sub.numpy(), out[1:].numpy())
    assert ap.compute_mfccs_windows(torch.from_numpy(x[:15999]), 4000).shape == (0, 101, 40)
    with pytest.raises(ValueError):
        ap.compute_mfccs_windows(torch.from_numpy(x), 4000, first=2, count=2)
    with pytest.raises(ValueError):
        ap.compute_mfccs_windows(torch.from_numpy(x).float(), 4000)


def test_cpu_label_stream_and_listen_stream(tmp_path):
    svc = _service(tmp_path, no_cuda=True)
    wav = _pcm(5, 40000).tobytes()  # 2.5 s: 4 windows at 0.5 s
    assert svc.label_stream(wav) == svc.label_batch(list(hs.stride(wav, 16000, 32000)))
    _same(svc.label_stream(wav, 100, max_windows=3), svc.label_batch(list(hs.stride(wav, 3200, 32000))))
    assert svc.label_stream(wav[:31998]) == []
    assert svc.listen_stream(wav) == svc.listen(wav)
    for kw in ("yes", "no", "_unknown_", "_silence_"):
        assert svc.listen_stream(wav, method="command_tagging", keyword=kw, min_keyword_prob=0.2) == \
            svc.listen(wav, method="command_tagging", keyword=kw, min_keyword_prob=0.2)


@pytest.mark.parametrize("stride_ms", [500, 100, 1250])
def test_cpu_stream_listener_any_chunking(tmp_path, stride_ms):
    svc = _service(tmp_path, no_cuda=True)
    wav = _pcm(6, 52000).tobytes()
    want = svc.label_stream(wav, stride_ms)
    assert len(want) == len(list(hs.stride(wav, 32 * stride_ms, 32000))) > 0
    whole = hs.StreamListener(svc, stride_ms).feed(wav)
    assert whole == want
    sl = hs.StreamListener(svc, stride_ms)
    got = []
    for i in range(0, len(wav), 2 * 1234):
        got += sl.feed(wav[i:i + 2 * 1234])
        assert len(sl._buf) < 32000 + 32 * stride_ms
    _same(got, want)  # (other batch compositions: the forward's rounding may differ in the last bit)
