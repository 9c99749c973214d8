"""compute_pcen_segments on the device (honk_pcen_segments_i16, csrc/mfcc_stream.hip): the batches and
the properties of tests/test_gpu_mfcc_segments.py under PCEN -- recording r's rows equal, bit for bit,
compute_pcen_windows of that recording alone -- plus PCEN's own: a silent recording between two loud
ones gives exact zeros (nothing leaks across a recording boundary, each window has its own smoother),
and a non-default parameter set.  Oracle of ragged_q1: the float64 tests/pcen_ref.pcen at the front-end
bound, used exactly as tests/test_gpu_pcen_windows.py uses it (16 x the float32 restatement's error on
the same windows, never above 1e-4, relative to max(max|ref window|, 1e-6))."""
import functools

import numpy as np
import pytest
import torch

import pcen_ref
import poison_util as pu
import segments_cases as sc
from honk_amd import model as hm
from honk_amd import service as hs
from honk_amd.audio import AudioPreprocessor
from oracle import frontend_f32_sim as sim
from test_gpu_mfcc_segments import _capture, _pool_against_listeners
from test_mfcc_windows_abi import _pcm, _same

pytestmark = pytest.mark.gpu
DEV, WIN = sc.DEV, sc.WIN
WHICH = "pcen"
ALT = dict(s=0.1, alpha=0.8, delta=1.0, r=0.25, power=2)
SEEDS = (35, 93, 275)  # three 3 s recordings; under PCEN no window of theirs is a near tie at 500 or 100 ms


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def _case(name):
    out, blocks = sc.check_rows(WHICH, AudioPreprocessor(), name)
    out.setflags(write=False)
    return out, blocks


@pytest.mark.parametrize("name", list(sc.BATCHES))
def test_rows_equal_the_single_recording_call(name):
    _gpu()
    out, blocks = _case(name)
    assert len(out) >= 2 and out.any()


@pytest.mark.parametrize("name", list(sc.BATCHES))
def test_two_runs_are_bitwise_equal(name):
    _gpu()
    out, _ = _case(name)
    pcm, off, stride, _ = sc.batch(name)
    again, _ = sc.segments(WHICH, AudioPreprocessor(), pcm, off, stride)
    assert again.tobytes() == out.tobytes()


@pytest.mark.parametrize("name", list(sc.BATCHES))
def test_reversed_order_permutes_the_row_blocks(name):
    _gpu()
    _, blocks = _case(name)
    _, rev = sc.check_rows(WHICH, AudioPreprocessor(), name, reverse=True)
    assert len(rev) == len(blocks)
    for a, b in zip(rev, blocks[::-1]):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()


def test_unowned_samples_are_never_read():
    _gpu()
    out, _ = _case("holes")
    pcm, off, stride, _ = sc.batch("holes")
    y = pcm.copy()
    y[sc.unowned("holes")] = 12345
    got, _ = sc.segments(WHICH, AudioPreprocessor(), y, off, stride)
    assert got.tobytes() == out.tobytes()
    plain, _ = _case("ragged_q1")
    assert plain.tobytes() == out.tobytes()


def _oracle(out, rows, stride, **kw):
    wins = [rec[w * stride:w * stride + WIN] for rec, _ in rows for w in range(sc.n_windows(len(rec), stride))]
    assert len(wins) == len(out)
    ys = np.stack(wins).astype(np.float32) / np.float32(32768.)
    refs = [pcen_ref.pcen(y.astype(np.float64), **kw) for y in ys]
    b = sim.bound(sim.e32("pcen", ys, refs, **kw))
    assert b <= 1e-4
    e = max(np.abs(np.asarray(out[w], np.float64) - r).max() / max(np.abs(r).max(), 1e-6) for w, r in enumerate(refs))
    print(f"pcen segments {kw}: max|segments - oracle| / max|ref window| = {e:.3e} (bound {b:.1e})")
    for w, ref in enumerate(refs):
        np.testing.assert_allclose(out[w], ref, atol=b * max(np.abs(ref).max(), 1e-6), rtol=0)


def test_ragged_q1_within_the_front_end_bound_of_the_oracle():
    _gpu()
    out, _ = _case("ragged_q1")
    _, _, stride, rows = sc.batch("ragged_q1")
    _oracle(out, rows, stride)


def test_a_non_default_parameter_set():
    """ones_9 (the pool's tick) under other parameters and power 2: the single-recording call's bits, and
    the oracle's bound."""
    _gpu()
    ap = AudioPreprocessor(pcen_params=ALT)
    out, blocks = sc.check_rows(WHICH, ap, "ones_9")
    default, _ = _case("ones_9")
    assert out.tobytes() != default.tobytes()
    _, _, stride, rows = sc.batch("ones_9")
    _oracle(out, rows, stride, **ALT)


def test_a_silent_recording_between_two_loud_ones_is_exactly_zero():
    """Three recordings of 24000 samples at stride 8000 (two windows each), the middle one all zeros and
    loud speech up to the last sample before it and from the first after it: a frame, a reflected edge or
    a smoother that crossed a recording boundary would leave something other than 0."""
    _gpu()
    loud = [_pcm(70, 24000), _pcm(71, 24000)]
    x = np.concatenate([loud[0], np.zeros(24000, np.int16), loud[1]])
    assert np.abs(x[23000:24000]).max() > 1000 and np.abs(x[48000:49000]).max() > 1000
    off = np.asarray([0, 24000, 48000, 72000], np.int64)
    out, w0 = sc.segments(WHICH, AudioPreprocessor(), x, off, 8000)
    assert w0.tolist() == [0, 2, 4, 6] and out.shape == (6, 101, 40)
    assert not out[2:4].any()
    assert out[0].any() and out[1].any() and out[4].any() and out[5].any()
    for r in (0, 1):
        want = sc.alone(WHICH, AudioPreprocessor(), loud[r], 8000)
        assert out[4 * r:4 * r + 2].tobytes() == want.tobytes()


@pytest.mark.parametrize("name", ["ragged_q1", "ones_9"])
def test_memory_contract(name):
    """out and the workspace (the mel-range table, then the E rows) poisoned and guard-banded, for every
    fill: the unpoisoned result, every guard intact, every element of out written; pcm and the table
    unchanged."""
    _gpu()
    want, _ = _case(name)
    pcm_np, off, stride, _ = sc.batch(name)
    pcm = torch.from_numpy(pcm_np).to(DEV)
    for fill in pu.FILLS:
        a = pu.arena(fill)
        out = sc.native_segments(a, WHICH, AudioPreprocessor(), pcm, off, stride, pu.frozen)
        a.check()
        assert out.cpu().numpy().tobytes() == want.tobytes(), hex(fill)
        if fill == 0xFF:
            assert not a.untouched(out)


def test_capturable():
    _gpu()
    _capture(WHICH)


# ---- the service ---------------------------------------------------------------------------------
def _service(tmp_path, no_cuda, labels=("_silence_", "_unknown_", "yes", "no")):
    torch.manual_seed(0)
    m = hm.SpeechModel(dict(hm.find_config("cnn-trad-pool2"), n_labels=len(labels)))
    fn = str(tmp_path / "m.pt")
    m.save(fn)
    return hs.TorchLabelService(fn, no_cuda=no_cuda, labels=list(labels), audio_preprocess_type="PCEN")


def _no_ties(logits_fn, wav, stride_ms):
    """No window's top two probabilities (CPU, numpy PCEN) within 2e-4 of each other."""
    wins = list(hs.stride(wav, 32 * stride_ms, 32000))
    pcm = np.stack([np.frombuffer(w, np.int16) for w in wins]).astype(np.float32) / 32768.
    x = AudioPreprocessor().compute_pcen(pcm)
    with torch.no_grad():
        p = torch.softmax(logits_fn(x), 1).numpy()
    top = np.sort(p, 1)
    assert (top[:, -1] - top[:, -2] > 2e-4).all()
    return len(wins)


@pytest.mark.parametrize("stride_ms", [500, 100])
def test_label_streams_equals_label_stream_per_recording(tmp_path, stride_ms):
    _gpu()
    wavs = [_pcm(s, 48000).tobytes() for s in SEEDS]
    cpu = _service(tmp_path, no_cuda=True)
    for w in wavs:
        _no_ties(cpu.model, w, stride_ms)
    svc = _service(tmp_path, no_cuda=False)
    want = [svc.label_stream(w, stride_ms) for w in wavs]
    for got in (svc.label_streams(wavs, stride_ms), svc.label_streams(wavs, stride_ms, max_windows=3),
                svc.label_streams(wavs, stride_ms, max_windows=12)):
        assert len(got) == 3
        for g, w in zip(got, want):
            assert len(g) == len(w) > 0
            _same(g, w, 1e-6)


def test_stream_pool_equals_stream_listeners(tmp_path):
    _gpu()
    cpu = _service(tmp_path, no_cuda=True)
    for s in SEEDS:
        _no_ties(cpu.model, _pcm(s, 48000).tobytes(), 500)
    _pool_against_listeners(_service(tmp_path, no_cuda=False), 500, SEEDS)
