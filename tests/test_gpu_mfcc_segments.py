"""compute_mfccs_segments on the device (honk_mfcc_segments_i16, csrc/mfcc_stream.hip): a batch of
recordings of ragged length in one call, and the serving surface over it (label_streams, StreamPool).

The defining property: recording r's rows equal, bit for bit, compute_mfccs_windows of that recording
alone in a buffer of its own.  The batches (tests/segments_cases.py) are the smallest that reach each
way the per-recording lookup or the tiling can go wrong.  ragged_q1 is also held to the front-end bound
of its float64 oracle (oracle.mfcc_ref), used exactly as tests/test_gpu_mfcc_windows.py uses it: 16 x the
error of the float32 restatement oracle/frontend_f32_sim.py on the same windows, never above 1e-4,
relative to max|ref window|.  Service results are compared under _same(..., 1e-6): the tolerance the
project already uses for the same windows in another batch composition of the forward."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import poison_util as pu
import segments_cases as sc
from honk_amd import _native
from honk_amd import model as hm
from honk_amd import service as hs
from honk_amd.audio import AudioPreprocessor
from oracle import frontend_f32_sim as sim
from oracle import mfcc_ref
from test_gpu_mfcc_windows import _no_ties
from test_mfcc_windows_abi import _pcm, _same, _service

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEV, WIN = sc.DEV, sc.WIN
WHICH = "mfccs"


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def _case(name):
    """(out, [rows of each recording]) of a batch, each block checked against the single-recording call;
    computed once, read-only."""
    out, blocks = sc.check_rows(WHICH, AudioPreprocessor(), name)
    out.setflags(write=False)
    return out, blocks


def test_the_plans_reach_what_the_batches_are_for():
    """Host-only: the tiles of each batch (FT = 32 slots, 16 edge groups per tile)."""
    ap = AudioPreprocessor()
    tiles = {}
    for name in sc.BATCHES:
        _, off, stride, _ = sc.batch(name)
        rc, plan, w0, _ = ap.segments_plan(off, stride)
        assert rc == 0
        tiles[name] = (int(plan.windows), int(plan.shared_frames), int(plan.tiles))
    # 1 / 33 / 0 / 2 windows: 97 + 129 + 98 shared frames in 4 + 5 + 4 tiles; 72 edge groups in 5 tiles
    assert tiles["ragged_q1"] == (36, 97 + 129 + 98, 13 + 5) == tiles["holes"]
    assert tiles["ones_9"] == (9, 9 * 97, 9 * 4 + 2)          # 18 edge groups: the second edge tile has 2
    assert tiles["gapped"] == (2 + 1 + 2, 5 * 97, 5 * 4 + 1)
    assert tiles["unshared"] == (11 + 1 + 2, 0, 14 * 4)
    assert tiles["empty_ends"] == (2, 50 + 97, 5 + 1)


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
    mask = sc.unowned("holes")
    assert off[0] == 1000 and mask.sum() == 5 * 1000 and mask[:1000].all() and mask[-1000:].all()
    y = pcm.copy()
    y[mask] = 12345
    got, _ = sc.segments(WHICH, AudioPreprocessor(), y, off, stride)
    assert got.tobytes() == out.tobytes()
    plain, _ = _case("ragged_q1")    # the same recordings without the holes
    assert plain.tobytes() == out.tobytes()


def test_ragged_q1_within_the_front_end_bound_of_the_oracle():
    _gpu()
    out, _ = _case("ragged_q1")
    pcm, off, stride, rows = sc.batch("ragged_q1")
    wins = [rec[w * stride:w * stride + WIN] for rec, _ in rows for w in range(sc.n_windows(len(rec), stride))]
    assert len(wins) == len(out) == 36
    refs = [mfcc_ref.mfcc(w / 32768.) for w in wins]
    ys = np.stack(wins).astype(np.float32) / 32768.
    b = sim.bound(sim.e32("mfcc", ys, refs))
    assert b <= 1e-4
    e = max(np.abs(out[w] - r).max() / max(np.abs(r).max(), 1e-30) for w, r in enumerate(refs))
    print(f"ragged_q1: max|segments - oracle| / max|ref| = {e:.3e} (bound {b:.1e})")
    for w, ref in enumerate(refs):
        np.testing.assert_allclose(out[w], ref, atol=b * np.abs(ref).max(), rtol=0)


@pytest.mark.parametrize("name", ["ragged_q1", "ones_9"])
def test_memory_contract(name):
    """out and the workspace poisoned and guard-banded, for every fill: the unpoisoned result, every
    guard intact, every element of out written; pcm and the table unchanged."""
    _gpu()
    want, _ = _case(name)
    pcm_np, off, stride, _ = sc.batch(name)
    pcm = torch.from_numpy(pcm_np).to(DEV)
    for fill in pu.FILLS:
        a = pu.arena(fill)
        out = sc.native_segments(a, WHICH, AudioPreprocessor(), pcm, off, stride, pu.frozen)
        a.check()
        assert out.cpu().numpy().tobytes() == want.tobytes(), hex(fill)
        if fill == 0xFF:   # (NaN as fp32: no finite result keeps it)
            assert not a.untouched(out)


def _capture(which, rows=36):
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "child.npz")
        try:
            p = subprocess.run([sys.executable, os.path.join(HERE, "mfcc_segments_graph_child.py"), which, out],
                               capture_output=True, text=True, timeout=120)
        except subprocess.TimeoutExpired:
            pytest.exit("tests/mfcc_segments_graph_child.py (graph capture / replay) hung: stopping the GPU run", 1)
        if p.returncode < 0 or p.returncode in (134, 139):
            pytest.exit(f"tests/mfcc_segments_graph_child.py died with status {p.returncode}: stopping the GPU run\n"
                        f"{p.stderr[-3000:]}", 1)
        assert p.returncode == 0, p.stderr[-3000:]
        z = np.load(out)
        assert z["replay"].shape == (rows, 101, 40) and z["replay"].tobytes() == z["eager"].tobytes()
        assert z["replay"].any()


def test_capturable():
    """The call inside torch.cuda.graph on fixed buffers; pcm refilled with other recordings of the same
    lengths, one replay: the eager result on the second batch, bit for bit.  In a child under a timeout."""
    _gpu()
    _capture(WHICH)


# ---- the service ---------------------------------------------------------------------------------
SEEDS = (31, 36, 37)  # three 3 s recordings; no window of theirs is a near tie at 500 or 100 ms (checked below)
CHUNKS = (2 * 1234, 2 * 777, None)   # bytes per tick of the three streams (None: whole); the third opens 2 ticks late


def _wavs(seeds=SEEDS):
    return [_pcm(s, 48000).tobytes() for s in seeds]


def _res8(svc):
    torch.manual_seed(1)
    return hm.find_model("res8")(dict(hm.find_config("res8"), n_labels=len(svc.labels))).eval()


@pytest.mark.parametrize("net", ["cnn-trad-pool2", "res8"])
@pytest.mark.parametrize("stride_ms", [500, 100])
def test_label_streams_equals_label_stream_per_recording(tmp_path, stride_ms, net):
    _gpu()
    wavs = _wavs()
    svc = _service(tmp_path, no_cuda=False)
    if net == "res8":
        m = _res8(svc)
        cpu_model = m
    else:
        cpu_model = _service(tmp_path, no_cuda=True).model
    for w in wavs:
        assert _no_ties(cpu_model, w, stride_ms) == {500: 5, 100: 21}[stride_ms]
    if net == "res8":
        svc.model = m.to(DEV)
    want = [svc.label_stream(w, stride_ms) for w in wavs]
    got = svc.label_streams(wavs, stride_ms)
    assert len(got) == 3
    for g, w in zip(got, want):
        assert len(g) == len(w) > 0
        _same(g, w, 1e-6)
    small = svc.label_streams(wavs, stride_ms, max_windows=3)   # every recording through label_stream itself
    # 500 ms: batches of 5 + 5 and 5 windows; 100 ms: 21 > 12, label_stream itself in chunks of 12
    mixed = svc.label_streams(wavs + [b"", wavs[0][:31998]], stride_ms, max_windows=12)
    assert mixed[3:] == [[], []]
    for g, s, x, w in zip(got, small, mixed, want):
        _same(s, w, 1e-6)
        _same(x, w, 1e-6)


def _pool_against_listeners(svc, stride_ms, seeds=SEEDS):
    wavs = _wavs(seeds)
    pool = hs.StreamPool(svc, stride_ms)
    listeners = [hs.StreamListener(svc, stride_ms) for _ in wavs]
    got, want = [[] for _ in wavs], [[] for _ in wavs]
    start = (0, 0, 2)
    size = [c or len(w) for c, w in zip(CHUNKS, wavs)]
    ticks = max(s + -(-len(w) // c) for s, w, c in zip(start, wavs, size))
    for t in range(ticks):
        fed = {}
        for k, w in enumerate(wavs):
            i = (t - start[k]) * size[k]
            if t >= start[k] and i < len(w):
                fed[k] = w[i:i + size[k]]
        res = pool.feed(fed)
        assert set(res) == set(fed)
        for k, chunk in fed.items():
            got[k] += res[k]
            want[k] += listeners[k].feed(chunk)
    for g, w in zip(got, want):
        assert len(g) == len(w) > 0
        _same(g, w, 1e-6)


def test_stream_pool_equals_stream_listeners(tmp_path):
    _gpu()
    svc = _service(tmp_path, no_cuda=False)
    _pool_against_listeners(svc, 500)
    _pool_against_listeners(svc, 100)


def test_one_tick_of_nine_streams_is_one_call_and_one_forward(tmp_path, monkeypatch):
    """Nine streams that each complete one window in the same tick: one honk_mfcc_segments_i16, no
    honk_mfcc_windows_i16, one forward of the model."""
    _gpu()
    svc = _service(tmp_path, no_cuda=False)
    wavs = {k: _pcm(60 + k, 16000).tobytes() for k in range(9)}
    cpu = _service(tmp_path, no_cuda=True)
    for w in wavs.values():
        assert _no_ties(cpu.model, w, 500) == 1
    want = {k: svc.label_stream(w) for k, w in wavs.items()}
    pool = hs.StreamPool(svc)
    assert pool.feed({k: w[:20000] for k, w in wavs.items()}) == {k: [] for k in wavs}
    lib, calls = _native.load(), dict(segments=0, windows=0, forward=0)
    real_seg, real_win = lib.honk_mfcc_segments_i16, lib.honk_mfcc_windows_i16

    def seg(*a):
        calls["segments"] += 1
        return real_seg(*a)

    def win(*a):
        calls["windows"] += 1
        return real_win(*a)

    monkeypatch.setattr(lib, "honk_mfcc_segments_i16", seg)
    monkeypatch.setattr(lib, "honk_mfcc_windows_i16", win)
    hook = svc.model.register_forward_hook(lambda *a: calls.__setitem__("forward", calls["forward"] + 1))
    try:
        got = pool.feed({k: w[20000:] for k, w in wavs.items()})
    finally:
        hook.remove()
    assert calls == dict(segments=1, windows=0, forward=1)
    for k in wavs:
        assert len(got[k]) == 1
        _same(got[k], want[k], 1e-6)
    assert sorted(pool.keys()) == list(range(9))


def test_label_streams_on_the_latency_schedule(tmp_path):
    """honk_latency with a res8 model in the service: its latency schedule gives a SpeechResModel's logits
    bit for bit whatever the batch, so the 1e-6 of the other service tests holds here as well."""
    _gpu()
    wavs = _wavs()
    svc = _service(tmp_path, no_cuda=False)
    m = _res8(svc)
    for w in wavs:
        _no_ties(m, w, 500)
    svc.model = m.to(DEV)
    want = [svc.label_stream(w, 500) for w in wavs]
    svc.honk_latency = True
    got = svc.label_streams(wavs, 500)
    assert svc.model.honk_schedule == "latency"
    for g, w in zip(got, want):
        _same(g, w, 1e-6)
