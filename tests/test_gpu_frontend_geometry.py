"""honk_mfcc_f32, honk_pcen_f32 and honk_mfcc_windows_i16 on the GPU at every shape of
frontend_geometry_cases.py, against the float64 oracles (oracle/mfcc_ref.py, tests/pcen_ref.py) at the
case's bound: 16 * e32(case), never above 1e-4, relative to max(max|ref clip|, 1e-6), where e32 is the
error of the float32 restatement oracle/frontend_f32_sim.py on the same clips.  Every case runs on the
route the table names (proved by the host-only plan query) and on the VALU route too where that is the
MFMA one.  Each test prints e32, the device error and their ratio (the table of DESIGN.md)."""
import random

import numpy as np
import pytest
import torch

import frontend_geometry_cases as fg
import pcen_ref
from honk_amd import _native
from honk_amd import data as hdata
from honk_amd import model as hm
from honk_amd.audio import AudioPreprocessor, dct_filters, mel_filterbank

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV)


def _call(front, case, ys, dct=None):
    """The C ABI on clips ys [B][S], the tables from honk_amd.audio, the output pre-filled with NaN."""
    pcm = _dev(ys)
    win = _dev(pcen_ref.window(case.n_fft))
    mel = _dev(mel_filterbank(fg.SR, case.n_fft, case.n_mels, fg.FMIN, fg.FMAX))
    lib, stream = _native.load(), _native.stream_handle(pcm.device)
    if front == "mfcc":
        dct = _dev(dct_filters(case.n_dct, case.n_mels) if dct is None else dct)
        out = torch.full((len(ys), case.frames, dct.shape[0]), float("nan"), device=DEV)
        rc = lib.honk_mfcc_f32(pcm.data_ptr(), len(ys), case.S, win.data_ptr(), case.n_fft, case.hop, mel.data_ptr(),
                               case.n_mels, dct.data_ptr(), dct.shape[0], out.data_ptr(), stream)
    else:
        out = torch.full((len(ys), case.frames, case.n_mels), float("nan"), device=DEV)
        rc = lib.honk_pcen_f32(pcm.data_ptr(), len(ys), case.S, win.data_ptr(), case.n_fft, case.hop, mel.data_ptr(),
                               case.n_mels, None, out.data_ptr(), stream)
    _native.check(rc, f"honk_{front}_f32")
    return out.cpu().numpy()


def _preprocessor(case):
    return AudioPreprocessor(n_fft=case.n_fft, hop_ms=case.hop // 16, n_mels=case.n_mels, n_dct_filters=case.n_dct)


def _python(front, ap, ys):
    fn = ap.compute_mfccs_batch if front == "mfcc" else ap.compute_pcen_batch
    return fn(torch.from_numpy(np.array(ys, dtype=np.float32)).to(DEV)).cpu().numpy()


def _routes(case, front):
    return [case.route[front]] + (["valu"] if case.route[front] == "mfma" else [])


def _set_route(monkeypatch, case, front, route):
    """Force the VALU route where the table names the MFMA one; prove the route with the plan query."""
    if route != case.route[front]:
        monkeypatch.setenv("HONK_MFCC_VALU", "1")
    else:
        monkeypatch.delenv("HONK_MFCC_VALU", raising=False)
    rc, plan = _native.front_plan(case.S, case.n_fft, case.hop, case.n_mels, case.n_dct if front == "mfcc" else None)
    assert rc == 0 and _native.FRONT_ROUTES[plan.route] == route and plan.frames == case.frames


def _check(what, got, ref, e, b):
    assert got.shape == ref.shape and got.dtype == np.float32, (got.shape, ref.shape)
    assert np.isfinite(got).all()
    errs = fg.errors(got, ref)
    print(f"FRONT {what}: e32 {e:.2e}  device {max(errs):.2e}  ratio {max(errs) / e:.2f}  bound {b:.2e}")
    assert max(errs) <= b, (what, errs, b)


@pytest.mark.parametrize("front", fg.FRONTS)
@pytest.mark.parametrize("case_id", [c.id for c in fg.BATCH])
def test_batch_case(monkeypatch, case_id, front):
    _gpu()
    case = fg.BY_ID[case_id]
    ys, ref, e = fg.clips(case), fg.refs(case_id, front), fg.e32(case_id, front)
    for route in _routes(case, front):
        _set_route(monkeypatch, case, front, route)
        got = _call(front, case, ys)
        _check(f"{case_id} {front} {route}", got, ref, e, fg.bound_of(e))
        assert not got[fg.ZERO].any()  # log / the root compression of zero energy pass through: exact zeros
        if case.expressible:
            py = _python(front, _preprocessor(case), ys)
            _check(f"{case_id} {front} {route} (audio.py)", py, ref, e, fg.bound_of(e))


@pytest.mark.parametrize("route", ["mfma", "valu"])
def test_empty_bands_give_the_oracles_exact_value(monkeypatch, route):
    """80 bands at n_fft 256: three mel rows hold no bin.  Their energy is an empty sum, so the log-mel
    entry (read through an identity in place of the DCT) and the PCEN value are exactly the oracle's 0."""
    _gpu()
    case = fg.BY_ID["emptybands"]
    mel = mel_filterbank(fg.SR, case.n_fft, case.n_mels, fg.FMIN, fg.FMAX)
    empty = np.flatnonzero(~mel.any(axis=1))
    assert len(empty) == 3
    ys = fg.clips(case)
    _set_route(monkeypatch, case, "mfcc", route)
    logmel = _call("mfcc", case, ys, dct=np.eye(case.n_mels, dtype=np.float32))
    assert logmel.shape == (len(ys), case.frames, case.n_mels) and np.isfinite(logmel).all()
    assert not logmel[:, :, empty].any() and np.abs(logmel[0]).max() > 1
    _set_route(monkeypatch, case, "pcen", route)
    got = _call("pcen", case, ys)
    assert not got[:, :, empty].any() and not fg.refs("emptybands", "pcen")[:, :, empty].any()


@pytest.mark.parametrize("route", ["mfma", "valu"])
def test_pcen_twice_gives_the_same_bits(monkeypatch, route):
    """PCEN's fixed-order claim (no float atomics on either route) at 51 x 20."""
    _gpu()
    case = fg.BY_ID["51x20"]
    _set_route(monkeypatch, case, "pcen", route)
    ys = fg.clips(case)
    assert np.array_equal(_call("pcen", case, ys), _call("pcen", case, ys))


@pytest.mark.parametrize("front", fg.FRONTS)
def test_python_chunk_loop(monkeypatch, front):
    """65537 clips: compute_*_batch makes two C calls, of 65535 and 2 clips."""
    _gpu()
    monkeypatch.delenv("HONK_MFCC_VALU", raising=False)
    case = fg.BY_ID["chunk"]
    ys = fg.chunk_clips()
    got = _python(front, _preprocessor(case), ys)
    assert got.shape == (fg.CHUNK_B, case.frames, case.n_dct) and np.isfinite(got).all()
    rows = list(fg.CHUNK_ROWS)
    ref = np.stack([fg.oracle(front, ys[r], case) for r in rows])
    e = max(fg.e32("chunk", front),
            fg.sim.e32(front, ys[rows], ref, sr=fg.SR, fmin=fg.FMIN, fmax=fg.FMAX, **case.shape,
                       **({"n_dct": case.n_dct} if front == "mfcc" else {})))
    _check(f"chunk rows {rows} {front}", got[rows], ref, e, fg.bound_of(e))
    assert not got[1::4].any()  # every fourth clip is the all-zero one


# ---- the windows kernel ------------------------------------------------------------------------------
def _windows(case, x, stride):
    return np.stack([x[w * stride:w * stride + case.window] for w in range(case.n_windows)]).astype(np.float32) / 32768.


@pytest.mark.parametrize("which", ["shared", "unshared"])
@pytest.mark.parametrize("case_id", [c.id for c in fg.WINDOWS])
def test_windows_case(monkeypatch, case_id, which):
    _gpu()
    monkeypatch.delenv("HONK_MFCC_VALU", raising=False)
    case = fg.WIN_BY_ID[case_id]
    stride = case.strides[which == "unshared"]
    ap = _preprocessor(case)
    x = fg.recording(case, stride)
    rc, plan = ap.windows_plan(len(x), stride, case.window)
    if rc == 0:
        assert plan.shared == int(case.shared and which == "shared") and plan.windows == case.n_windows
    else:
        assert rc == -2 and not case.kernel
    got = ap.compute_mfccs_windows(torch.from_numpy(x).to(DEV), stride, window=case.window).cpu().numpy()
    old = ap.compute_mfccs_batch(torch.from_numpy(_windows(case, x, stride)).to(DEV)).cpu().numpy()
    refs = fg.window_refs(case, x, stride)
    e = fg.window_e32(case, x, stride, refs)
    b = fg.bound_of(e)
    assert got.shape == old.shape == (case.n_windows, case.frames, case.n_dct)
    _check(f"windows {case_id} {which}", got, np.stack(refs), e, b)
    _check(f"windows {case_id} {which} (per-window kernel)", old, np.stack(refs), e, b)
    scale = [max(np.abs(r).max(), 1e-6) for r in refs]
    assert max(np.abs(got[w] - old[w]).max() / scale[w] for w in range(case.n_windows)) <= b
    if not case.kernel:
        # the fallback is the per-window kernel on the same float windows, here on its VALU route (129 bands,
        # n_fft 2048: past the MFMA plan), which sums in a fixed order: the same bits
        assert _native.front_plan(case.window, case.n_fft, case.hop, case.n_mels, case.n_dct)[1].route == 2
        assert np.array_equal(got, old)


@pytest.mark.parametrize("which", ["shared", "unshared"])
def test_windows_runs_and_ranges_are_bitwise(which):
    """At 320 / 80, window 8000: two runs give the same bits, and ranges concatenate to the whole."""
    _gpu()
    case = fg.WIN_BY_ID["320-80"]
    stride = case.strides[which == "unshared"]
    ap, pcm = _preprocessor(case), torch.from_numpy(fg.recording(case, stride)).to(DEV)
    whole = ap.compute_mfccs_windows(pcm, stride, window=case.window)
    assert whole.shape[0] == case.n_windows == 5
    assert torch.equal(ap.compute_mfccs_windows(pcm, stride, window=case.window), whole)
    parts = [ap.compute_mfccs_windows(pcm, stride, window=case.window, first=f, count=n) for f, n in ((0, 2), (2, 3))]
    assert torch.equal(torch.cat(parts), whole)


# ---- the data path at 51 x 20 --------------------------------------------------------------------------
@pytest.mark.parametrize("front_end", ["MFCCs", "PCEN"])
def test_device_dataset_at_51x20(monkeypatch, front_end):
    """DeviceSpeechDataset with input_length 8000 and 20 bands: device_batch is the front end applied to
    augment_batch on the same seed, it meets the oracle on what augment_batch gave, and a res and a cnn
    model built from that config run forward on it."""
    _gpu()
    monkeypatch.delenv("HONK_MFCC_VALU", raising=False)
    g = np.random.default_rng(8)
    clips = {f"c{i}.wav": (pcen_ref.clips(8000)[i % 8][:8000 - 13 * i], 2 + i % 3) for i in range(10)}
    bg = [(g.standard_normal(30000) * 0.1).astype(np.float32)]
    cfg = dict(input_length=8000, timeshift_ms=100, noise_prob=0.8, silence_prob=0.1, cache_size=32,
               n_mels=20, n_dct_filters=20, audio_preprocess_type=front_end)
    a, b = (hdata.DeviceSpeechDataset(clips, hdata.DatasetType.TRAIN, cfg, device=DEV, rng=random.Random(5),
                                      bg_noise_audio=bg) for _ in range(2))
    idx = torch.tensor([3, 0, 10, 7, 9, 3])  # (10: a silence item)
    x = hdata.batch_input(a, idx)
    pcm = b.augment_batch(idx)
    ap = b.audio_processor
    want = ap.compute_pcen_batch(pcm) if front_end == "PCEN" else ap.compute_mfccs_batch(pcm)
    assert x.is_cuda and tuple(x.shape) == tuple(want.shape) == (6, 51, 20) and torch.isfinite(x).all()
    case, front = fg.BY_ID["51x20"], "pcen" if front_end == "PCEN" else "mfcc"
    ys = pcm.cpu().numpy()
    ref = np.stack([fg.oracle(front, y, case) for y in ys])
    e = fg.sim.e32(front, ys, ref, sr=fg.SR, fmin=fg.FMIN, fmax=fg.FMAX, **case.shape,
                   **({"n_dct": case.n_dct} if front == "mfcc" else {}))
    b_ = fg.bound_of(e)
    _check(f"dataset 51x20 {front}", x.cpu().numpy(), ref, e, b_)
    _check(f"dataset 51x20 {front} (front end on augment_batch)", want.cpu().numpy(), ref, e, b_)
    if front_end == "PCEN":
        assert torch.equal(x, want)  # (the same draws, and the fused kernel sums in a fixed order)
    else:
        scale = torch.from_numpy(np.maximum(np.abs(ref).max(axis=(1, 2)), 1e-6)).to(DEV)[:, None, None]
        assert float(((x - want).abs() / scale).max()) <= b_  # (the MFMA MFCC's atomic sums: equal to rounding)
    torch.manual_seed(0)
    for name in ("res8-narrow", "cnn-trad-pool2"):
        mcfg = dict(hm.find_config(name), n_labels=4, height=51, width=20)
        model = hm.find_model(name)(mcfg).eval().to(DEV)
        with torch.no_grad():
            y = model(x)
        assert tuple(y.shape) == (6, 4) and torch.isfinite(y).all()
