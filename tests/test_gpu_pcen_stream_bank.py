"""StreamBank under PCEN on the device (honk_pcen_bank_tick_i16, csrc/mfcc_stream.hip): the cache holds a
frame's mel energies before the smoother, which still restarts per window; stage 2 gathers a window's tile
from the slot's cached rows, the tick's rows in the workspace and the window's edge rows.

The defining property: a stream's rows, concatenated over its ticks, are byte-equal to compute_pcen_windows
of the whole recording alone (pinned to its float64 oracle in tests/test_gpu_pcen_windows.py).  The
schedules and the shared checks are tests/stream_bank_cases.py's; the service recordings and their near-tie
check are tests/test_gpu_pcen_segments.py's (the seeds chosen there for PCEN), the chunkings
tests/test_gpu_mfcc_segments.py's; service results under _same(..., 1e-6) as the existing pool tests."""
import functools

import pytest
import torch

import poison_util as pu
import stream_bank_cases as bc
from honk_amd.audio import AudioPreprocessor
from test_gpu_mfcc_segments import CHUNKS
from test_gpu_pcen_segments import SEEDS, _no_ties, _service
from test_mfcc_windows_abi import _pcm, _same

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FRONT, WHICH = "PCEN", "pcen"
# nine 1.5 s recordings; under PCEN neither window of theirs is a near tie at 500 ms (checked below)
NINE = (61, 64, 65, 66, 68, 69, 70, 72, 75)


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def _case(name):
    got, bank = bc.check(AudioPreprocessor(), name, FRONT, DEV)
    for rows in got.values():
        rows.setflags(write=False)
    return got, dict(bank.stats)


@pytest.mark.parametrize("name", list(bc.CASES))
def test_ticks_add_up_to_the_whole_recording(name):
    _gpu()
    got, stats = _case(name)
    assert all(r.any() for r in got.values()) and stats["ticks"] == len(bc.CASES[name][1])


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
    _gpu()
    got, _ = _case("ragged")
    for k in got:
        alone, bank = bc.run(AudioPreprocessor(), "ragged", FRONT, DEV, slots=1, only={k})
        assert bank.slots == 1 and list(alone) == [k]
        assert alone[k].shape == got[k].shape and alone[k].tobytes() == got[k].tobytes(), k


def test_power_2_goes_through_its_own_instantiation():
    _gpu()
    ap = AudioPreprocessor(pcen_params=dict(power=2))
    bc.check(ap, "steady_q50", FRONT, DEV)


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


# ---- the service ---------------------------------------------------------------------------------
@pytest.mark.parametrize("stride_ms", [500, 100])
def test_pool_with_device_state_equals_the_plain_pool(tmp_path, stride_ms):
    _gpu()
    wavs = [_pcm(s, 48000).tobytes() for s in SEEDS]
    cpu = _service(tmp_path, no_cuda=True)
    for w in wavs:
        assert _no_ties(cpu.model, w, stride_ms) == {500: 5, 100: 21}[stride_ms]
    bc.pools_agree(_service(tmp_path, no_cuda=False), stride_ms, wavs, CHUNKS, _same)


def test_one_tick_of_nine_streams_is_one_bank_tick_and_one_forward(tmp_path, monkeypatch):
    _gpu()
    wavs = {k: _pcm(s, 24000).tobytes() for k, s in enumerate(NINE)}
    cpu = _service(tmp_path, no_cuda=True)
    for w in wavs.values():
        assert _no_ties(cpu.model, w, 500) == 2
    bc.nine_streams_one_tick(_service(tmp_path, no_cuda=False), wavs, WHICH, monkeypatch, _same)
