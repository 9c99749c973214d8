"""The PCEN front end without a GPU: the numpy path (AudioPreprocessor.compute_pcen) against the
float64 restatement tests/pcen_ref.py (PARITY UNPINNED: the reference's ``pcen`` package is absent),
honk_pcen_f32's argument contract (every call here returns before it would touch the GPU: the
pointers are never dereferenced), and the serving surface on the CPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pcen_ref
from honk_amd import _native
from honk_amd import model as hm
from honk_amd import service as hs
from honk_amd.audio import AudioPreprocessor
from test_mfcc_windows_abi import _pcm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
P = 0x1000  # a non-null stand-in for a device pointer
CPU_REL = 1e-4  # of the clip's maximum; a float32 numpy version of the definition measured <= 1.6e-6


@pytest.fixture()
def lib():
    from honk_amd import build
    build.build()
    return _native.load()


# ---- numpy path ---------------------------------------------------------------------------------
def test_compute_pcen_matches_reference():
    ys, ref = pcen_ref.clips(), pcen_ref.ref_clips()
    out = AudioPreprocessor().compute_pcen(ys)
    assert out.dtype == torch.float32 and tuple(out.shape) == (len(ys), 101, 40)
    got = out.numpy()
    for i in range(len(ys)):
        np.testing.assert_allclose(got[i], ref[i], atol=CPU_REL * np.abs(ref[i]).max(), rtol=0)
    assert np.all(got[pcen_ref.ZERO_CLIP] == 0.0)
    assert np.abs(ref[6]).max() > 2 * np.abs(ref[0]).max()  # the onset clip is the high-gain one


def test_compute_pcen_shapes_and_dtypes():
    ap = AudioPreprocessor()
    ys = pcen_ref.clips()[:3]
    whole = ap.compute_pcen(ys)
    for data in (ys[1], ys[1:2], torch.from_numpy(ys[1]), torch.from_numpy(ys[1:2]), ys[1].astype(np.float64)):
        one = ap.compute_pcen(data)
        assert isinstance(one, torch.Tensor) and one.dtype == torch.float32 and tuple(one.shape) == (1, 101, 40)
        assert torch.equal(one[0], whole[1])
    assert torch.equal(ap.compute_pcen_batch(torch.from_numpy(ys)), whole)  # a CPU tensor: the numpy path
    assert tuple(ap.compute_pcen(ys[:, :16077]).shape) == (3, 101, 40)
    assert tuple(ap.compute_pcen(ys[:, :1600]).shape) == (3, 11, 40)
    with pytest.raises(ValueError):
        ap.compute_pcen(ys[None])
    assert ap.pcen_params == dict(eps=1e-6, s=0.025, alpha=0.98, delta=2.0, r=0.5, power=1)


@pytest.mark.parametrize("params", [dict(power=2), dict(s=0.1), dict(s=0.1, alpha=0.8, delta=1.0, r=0.25)])
def test_compute_pcen_parameters(params):
    ys, ref = pcen_ref.clips(), pcen_ref.ref_clips(**params)
    got = AudioPreprocessor(pcen_params=params).compute_pcen(ys).numpy()
    for i in range(len(ys)):
        np.testing.assert_allclose(got[i], ref[i], atol=CPU_REL * np.abs(ref[i]).max(), rtol=0)
    assert np.abs(ref - pcen_ref.ref_clips()).max() > 1e-2  # the parameters are taken


# ---- the C ABI, host-only -------------------------------------------------------------------------
def _call(lib, batch=2, samples=16000, n_fft=480, hop=160, n_mels=40, ptrs=(P,) * 4, params=None, **kw):
    pcm, win, mel, out = ptrs
    if kw:
        d = dict(eps=1e-6, s=0.025, alpha=0.98, delta=2.0, r=0.5, power=1)
        d.update(kw)
        params = _native.PcenParams(d["eps"], d["s"], d["alpha"], d["delta"], d["r"], d["power"])
    pp = ctypes.addressof(params) if params is not None else None
    return lib.honk_pcen_f32(pcm, batch, samples, win, n_fft, hop, mel, n_mels, pp, out, None)


def test_symbol_header_and_binding_agree(lib):
    src = open(os.path.join(REPO, "include", "honk_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert hasattr(lib, "honk_pcen_f32") and "honk_pcen_f32" in _native.EXPORTS
    assert re.search(r"\bhonk_pcen_f32\s*\(", src)
    assert re.search(r"float eps, s, alpha, delta, r;\s*int32_t power;\s*}\s*honk_pcen_params_t", src)
    assert ctypes.sizeof(_native.PcenParams) == 6 * 4
    from honk_amd import build
    assert "pcen.hip" in build.SOURCES


def test_argument_errors(lib):
    for null in range(4):
        assert _call(lib, ptrs=tuple(0 if i == null else P for i in range(4))) == ERR_ARG
        assert b"null pointer" in lib.honk_last_error()
    assert _call(lib, samples=240) == ERR_ARG  # samples <= n_fft/2: no reflect padding
    assert b"n_fft/2" in lib.honk_last_error()
    assert _call(lib, samples=100) == ERR_ARG
    inf, nan = float("inf"), float("nan")
    for bad in (dict(s=0.0), dict(s=-0.1), dict(s=1.5), dict(eps=0.0), dict(eps=-1e-6), dict(alpha=-0.1),
                dict(delta=-1.0), dict(r=0.0), dict(r=-0.5), dict(power=0), dict(power=3),
                dict(eps=inf), dict(s=nan), dict(alpha=inf), dict(delta=nan), dict(r=inf), dict(alpha=nan)):
        assert _call(lib, **bad) == ERR_ARG, bad
        assert b"pcen" in lib.honk_last_error()
    assert _call(lib, batch=-1) == ERR_ARG
    assert _call(lib, batch=65536) == ERR_ARG
    assert _call(lib, n_mels=0) == ERR_ARG


def test_empty_batch_enqueues_nothing(lib):
    assert _call(lib, batch=0, ptrs=(0,) * 4) == 0
    assert _call(lib, batch=0, ptrs=(0,) * 4, s=1.0, power=2) == 0  # (s = 1 is inside (0, 1])


# ---- the serving surface on the CPU ------------------------------------------------------------------
def _service(tmp_path, **kw):
    labels = ["_silence_", "_unknown_", "yes", "no"]
    torch.manual_seed(0)
    m = hm.SpeechModel(dict(hm.find_config("cnn-trad-pool2"), n_labels=len(labels)))
    fn = str(tmp_path / "m.pt")
    m.save(fn)
    return hs.TorchLabelService(fn, no_cuda=True, labels=labels, **kw)


def _same(got, want, tol=1e-6):
    assert [g[0] for g in got] == [w[0] for w in want]
    assert all(abs(g[1] - w[1]) <= tol for g, w in zip(got, want))


def test_cpu_service_pcen(tmp_path):
    svc = _service(tmp_path, audio_preprocess_type="PCEN")
    wav = _pcm(5, 40000).tobytes()  # 2.5 s: 4 windows at 0.5 s
    wins = list(hs.stride(wav, 16000, 32000))
    assert len(wins) == 4
    x = svc._model_input(wins[:1])
    want = AudioPreprocessor().compute_pcen(np.frombuffer(wins[0], np.int16).astype(np.float32) / 32768.)
    assert torch.equal(x, want)  # the model sees PCEN, each window with its own smoother
    many = svc.label_batch(wins)
    _same([svc.label(w) for w in wins], many)
    assert svc.label_stream(wav) == many
    _same(svc.label_stream(wav, 100, max_windows=3), svc.label_batch(list(hs.stride(wav, 3200, 32000))))
    assert svc.listen_stream(wav) == svc.listen(wav)
    want = svc.label_stream(wav, 100)
    sl, got = hs.StreamListener(svc, 100), []
    for i in range(0, len(wav), 2 * 1234):
        got += sl.feed(wav[i:i + 2 * 1234])
    assert len(got) == len(want) > 0
    _same(got, want)
    with pytest.raises(ValueError):
        _service(tmp_path, audio_preprocess_type="bogus")


def test_cpu_service_default_is_mfcc(tmp_path):
    wav = _pcm(7, 40000).tobytes()
    wins = list(hs.stride(wav, 16000, 32000))
    default, mfcc, pcen = _service(tmp_path), _service(tmp_path, audio_preprocess_type="MFCCs"), \
        _service(tmp_path, audio_preprocess_type="PCEN")
    assert default.audio_preprocess_type == "MFCCs"
    assert torch.equal(default._model_input(wins), mfcc._model_input(wins))
    assert default.label_batch(wins) == mfcc.label_batch(wins)
    assert default.label(wins[0]) == mfcc.label(wins[0])
    assert default.label_stream(wav) == mfcc.label_stream(wav)
    assert not torch.equal(default._model_input(wins), pcen._model_input(wins))
