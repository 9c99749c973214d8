"""StreamBank on the device (honk_mfcc_bank_tick_i16, csrc/mfcc_stream.hip): streams fed tick after tick,
their tails and the finished rows their next window reuses resident on the device, and
StreamPool(device_state=True) over it.

The defining property: a stream's rows, concatenated over its ticks, are byte-equal to compute_mfccs_windows
of the whole recording alone -- calls the project already pins to its float64 oracle
(tests/test_gpu_mfcc_windows.py), so no tolerance is invented here.  The schedules
(tests/stream_bank_cases.py) are the smallest that reach each way the cache, the tails or the per-stream
lookup can go wrong.  Service results are compared under _same(..., 1e-6): the tolerance the existing pool
tests use for the same windows in another batch composition of the forward."""
import functools

import pytest
import torch

import poison_util as pu
import stream_bank_cases as bc
from honk_amd.audio import AudioPreprocessor
from test_gpu_mfcc_segments import CHUNKS, SEEDS, _wavs
from test_gpu_mfcc_windows import _no_ties
from test_mfcc_windows_abi import _pcm, _same, _service

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FRONT, WHICH = "MFCCs", "mfcc"
NINE = range(60, 69)   # nine 1.5 s recordings; neither window of theirs is a near tie at 500 ms (checked below)


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def _case(name):
    """({stream: rows}, stats) of a schedule on a bank grown from 2 slots, every stream checked against the
    whole recording's windows; computed once, read-only."""
    got, bank = bc.check(AudioPreprocessor(), name, FRONT, DEV)
    for rows in got.values():
        rows.setflags(write=False)
    return got, dict(bank.stats)


@pytest.mark.parametrize("name", list(bc.CASES))
def test_ticks_add_up_to_the_whole_recording(name):
    _gpu()
    got, stats = _case(name)
    assert all(r.any() for r in got.values()) and stats["ticks"] == len(bc.CASES[name][1])
    if name == "ragged":   # the closed stream and the key that took its slot
        assert len(got["d"]) == 1 and len(got["g"]) == 2


@pytest.mark.parametrize("name", list(bc.CASES))
def test_two_runs_are_bitwise_equal(name):
    _gpu()
    got, _ = _case(name)
    again, _ = bc.run(AudioPreprocessor(), name, FRONT, DEV)
    assert set(again) == set(got)
    for k in got:
        assert again[k].tobytes() == got[k].tobytes(), k


def test_feed_order_does_not_matter():
    _gpu()
    got, _ = _case("ragged")
    rev, _ = bc.run(AudioPreprocessor(), "ragged", FRONT, DEV, reverse=True)
    for k in got:
        assert rev[k].shape == got[k].shape and rev[k].tobytes() == got[k].tobytes(), k


def test_a_stream_alone_in_a_bank_of_one_slot():
    """Alone in a bank of 1 slot, or among the others in a bank that grew from 2 slots during the schedule."""
    _gpu()
    got, _ = _case("ragged")
    for k in got:
        alone, bank = bc.run(AudioPreprocessor(), "ragged", FRONT, DEV, slots=1, only={k})
        assert bank.slots == 1 and list(alone) == [k]
        assert alone[k].shape == got[k].shape and alone[k].tobytes() == got[k].tobytes(), k


@pytest.mark.parametrize("name", ["ones_9", "q1"])
def test_memory_contract(name):
    _gpu()
    got, _ = _case(name)
    bc.memory_contract(FRONT, name, got, DEV, pu)


@pytest.mark.parametrize("name", ["ones_9", "q1"])
def test_counters_equal_the_cpu_banks(name):
    _gpu()
    _, stats = _case(name)
    _, cpu = bc.run(AudioPreprocessor(), name, FRONT, "cpu")
    assert stats == cpu.stats and stats["frames_reused"] > 0


def test_an_unsupported_shape_raises():
    _gpu()
    with pytest.raises(ValueError):
        AudioPreprocessor(n_fft=500).stream_bank(8000, device=DEV)


# ---- the service ---------------------------------------------------------------------------------
@pytest.mark.parametrize("stride_ms", [500, 100])
def test_pool_with_device_state_equals_the_plain_pool(tmp_path, stride_ms):
    _gpu()
    wavs = _wavs()
    cpu_model = _service(tmp_path, no_cuda=True).model
    for w in wavs:
        assert _no_ties(cpu_model, w, stride_ms) == {500: 5, 100: 21}[stride_ms]
    bc.pools_agree(_service(tmp_path, no_cuda=False), stride_ms, wavs, CHUNKS, _same)


def test_one_tick_of_nine_streams_is_one_bank_tick_and_one_forward(tmp_path, monkeypatch):
    _gpu()
    wavs = {k: _pcm(s, 24000).tobytes() for k, s in enumerate(NINE)}
    cpu = _service(tmp_path, no_cuda=True)
    for w in wavs.values():
        assert _no_ties(cpu.model, w, 500) == 2
    bc.nine_streams_one_tick(_service(tmp_path, no_cuda=False), wavs, WHICH, monkeypatch, _same)
