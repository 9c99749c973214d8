"""honk_mfcc_segments_plan / _i16 and honk_pcen_segments_plan / _i16 (csrc/mfcc_stream.hip), host-only:
the batch plan's counts against the sums of the single-recording plans, window0, the tile formula, the
argument contract (every call here returns before it would touch the GPU: the pointers are never
dereferenced), and the CPU side of the Python surface (compute_mfccs_segments, compute_pcen_segments,
label_streams, StreamPool)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from honk_amd import _native
from honk_amd import service as hs
from honk_amd.audio import AudioPreprocessor
from test_mfcc_windows_abi import _pcm, _same, _service

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -2, -3
P = 0x1000  # a non-null stand-in for a device pointer
WIN, NFFT, HOP, NMELS = 16000, 480, 160, 40
FT = 32     # frame slots per workgroup
ROW = 48    # bytes of a table row: six int64
COUNTS = ("windows", "shared_frames", "edge_frames", "frames_computed")

# stride -> the lengths of a batch: 0 samples, 15999, exactly one window, one sample short of a second
# window, and a few longer ones
BATCHES = {
    160: [16000, 0, 16000 + 32 * 160, 15999, 16000 + 160 - 1, 16000 + 160],
    8000: [0, 48000, 15999, 16000, 16000 + 8000 - 1, 24000, 0],
    24000: [56000, 16000, 15999, 16000 + 24000 - 1, 40000, 0],
    400: [20000, 0, 16399, 16400, 15999, 16000],
}


@pytest.fixture()
def lib():
    from honk_amd import build
    build.build()
    return _native.load()


def _off(lens, first=0):
    return np.concatenate([[first], first + np.cumsum(lens)]).astype(np.int64)


def _plan(lib, off, stride, pcen=False, window=WIN, n_fft=NFFT, hop=HOP, n_mels=NMELS, table=True, cap=None,
          plan=True):
    off = np.ascontiguousarray(off, dtype=np.int64)
    n_rec = len(off) - 1
    p = _native.MfccSegmentsPlan()
    w0 = np.full(max(n_rec, 0) + 1, -1, np.int64)
    tbl = np.zeros(ROW // 8 * (max(n_rec, 0) + 1), np.int64)
    extra = (n_mels,) if pcen else ()
    fn = lib.honk_pcen_segments_plan if pcen else lib.honk_mfcc_segments_plan
    rc = fn(off.ctypes.data, n_rec, window, stride, n_fft, hop, *extra, w0.ctypes.data,
            tbl.ctypes.data if table else None, tbl.nbytes if cap is None else cap,
            ctypes.addressof(p) if plan else None)
    return rc, p, w0, tbl


def _single(lib, samples, stride):
    p = _native.MfccWindowsPlan()
    n = 0 if samples < WIN else 1 + (samples - WIN) // stride
    assert lib.honk_mfcc_windows_plan(samples, WIN, stride, NFFT, HOP, 0, n, ctypes.addressof(p)) == 0
    return p


def _call(lib, lens=(48000, 16000), total=None, off=None, window=WIN, stride=8000, n_fft=NFFT, hop=HOP, n_mels=NMELS,
          n_dct=40, pcen=False, params=None, ptrs=(P,) * 7, ws_bytes=1 << 24, table_bytes=1 << 16, n_rec=None):
    off = _off(lens) if off is None else np.ascontiguousarray(off, dtype=np.int64)
    n_rec = len(off) - 1 if n_rec is None else n_rec
    total = int(off[-1]) if total is None else total
    pcm, tbl, win, mel, dct, out, ws = ptrs
    head = (pcm, total, off.ctypes.data, n_rec, tbl, table_bytes, window, stride, win, n_fft, hop, mel, n_mels)
    if pcen:
        pp = ctypes.addressof(params) if params is not None else None
        return lib.honk_pcen_segments_i16(*head, pp, out, ws, ws_bytes, None)
    return lib.honk_mfcc_segments_i16(*head, dct, n_dct, out, ws, ws_bytes, None)


def test_symbols_exist_and_header_agrees(lib):
    src = open(os.path.join(REPO, "include", "honk_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("honk_mfcc_segments_plan", "honk_mfcc_segments_i16", "honk_pcen_segments_plan",
                 "honk_pcen_segments_i16"):
        assert hasattr(lib, name) and name in _native.EXPORTS
        assert re.search(r"\b%s\s*\(" % name, src), name
    assert "honk_mfcc_segments_plan_t" in src
    # the struct the binding mirrors: seven int64 counts, two int32
    assert ctypes.sizeof(_native.MfccSegmentsPlan) == 7 * 8 + 2 * 4


@pytest.mark.parametrize("first", [0, 1000])
@pytest.mark.parametrize("stride", sorted(BATCHES))
def test_plan_is_the_sum_of_the_single_recording_plans(lib, stride, first):
    lens = BATCHES[stride]
    rc, p, w0, tbl = _plan(lib, _off(lens, first), stride)
    assert rc == 0
    singles = [_single(lib, n, stride) for n in lens]
    for k in COUNTS:
        assert getattr(p, k) == sum(getattr(s, k) for s in singles), k
    W = [s.windows for s in singles]
    assert W.count(0) >= 2 and 1 in W and max(W) >= 2
    assert w0.tolist() == np.concatenate([[0], np.cumsum(W)]).tolist()
    assert p.frames == 101 and p.shared == int(stride % HOP == 0) and p.table_bytes == ROW * (len(lens) + 1)
    # the tiles: per recording as the single call lays them out, the edge tiles over the batch's windows
    if stride in (160, 8000):    # overlapping: runs of 32 shared frames of a recording
        seg = [-(-s.shared_frames // FT) for s in singles]
    else:                        # gapped (97 interior frames) / unshared (101): 4 tiles per window
        seg = [4 * w for w in W]
    edge = -(-2 * sum(W) // 16) if stride != 400 else 0   # 2 edge frames per side: 16 groups per tile
    assert p.tiles == sum(seg) + edge
    # the table: first tile, first window, first shared row, sample0, n, G per recording, then the totals
    t = tbl.reshape(-1, 6)
    assert t[:, 0].tolist() == np.concatenate([[0], np.cumsum(seg)]).tolist()
    assert t[:, 1].tolist() == w0.tolist()
    assert t[:, 3].tolist() == _off(lens, first).tolist()
    assert t[:-1, 4].tolist() == W
    if stride in (160, 8000):
        assert t[:-1, 5].tolist() == [s.shared_frames for s in singles]
        assert t[:, 2].tolist() == np.concatenate([[0], np.cumsum([s.shared_frames for s in singles])]).tolist()
    # sizes only
    rc2, p2, _, _ = _plan(lib, _off(lens, first), stride, table=False, cap=0)
    assert rc2 == 0 and bytes(p2) == bytes(p)


@pytest.mark.parametrize("stride", sorted(BATCHES))
def test_pcen_plan_same_counts_own_workspace(lib, stride):
    off = _off(BATCHES[stride])
    rc, p, w0, tbl = _plan(lib, off, stride, pcen=True)
    rm, m, w0m, tblm = _plan(lib, off, stride)
    assert rc == 0 and rm == 0
    for k in COUNTS + ("tiles", "table_bytes", "shared", "frames"):
        assert getattr(p, k) == getattr(m, k), k
    assert np.array_equal(w0, w0m) and np.array_equal(tbl, tblm)
    assert m.workspace_bytes == 2 * 128 * 4
    if stride in (160, 8000):   # the overlapping route keeps one row of E per frame computed
        assert p.workspace_bytes == m.workspace_bytes + p.frames_computed * NMELS * 4
        _, p20, _, _ = _plan(lib, off, stride, pcen=True, n_mels=20)
        assert p20.workspace_bytes == m.workspace_bytes + p.frames_computed * 20 * 4
    else:
        assert p.workspace_bytes == m.workspace_bytes


@pytest.mark.parametrize("pcen", [False, True])
def test_argument_errors(lib, pcen):
    n_ptrs = 7
    for null in range(n_ptrs):
        if pcen and null == 4:
            continue  # (no dct)
        ptrs = tuple(0 if i == null else P for i in range(n_ptrs))
        assert _call(lib, pcen=pcen, ptrs=ptrs) == ERR_ARG, null
        assert b"null pointer" in lib.honk_last_error()
    assert _plan(lib, _off([48000]), 8000, pcen=pcen, plan=False)[0] == ERR_ARG
    assert b"null pointer" in lib.honk_last_error()
    fn = lib.honk_pcen_segments_plan if pcen else lib.honk_mfcc_segments_plan
    extra = (NMELS,) if pcen else ()
    plan = _native.MfccSegmentsPlan()
    assert fn(None, 1, WIN, 8000, NFFT, HOP, *extra, None, None, 0, ctypes.addressof(plan)) == ERR_ARG
    assert fn(_off([48000]).ctypes.data, -1, WIN, 8000, NFFT, HOP, *extra, None, None, 0,
              ctypes.addressof(plan)) == ERR_ARG
    assert b"negative" in lib.honk_last_error()
    assert _call(lib, pcen=pcen, n_rec=-1) == ERR_ARG
    assert _call(lib, pcen=pcen, total=-1, off=[0, 0]) == ERR_ARG
    for bad in ([0, 48000, 47999], [-1, 48000], [5, 4]):
        assert _plan(lib, bad, 8000, pcen=pcen)[0] == ERR_ARG, bad
        assert b"offset" in lib.honk_last_error()
        assert _call(lib, pcen=pcen, off=bad, total=1 << 20) == ERR_ARG, bad
    assert _call(lib, pcen=pcen, lens=(48000, 16000), total=63999) == ERR_ARG  # offsets past total_samples
    assert b"past" in lib.honk_last_error()
    assert _call(lib, pcen=pcen, stride=0) == ERR_ARG
    assert _plan(lib, _off([48000]), 0, pcen=pcen)[0] == ERR_ARG
    assert _call(lib, pcen=pcen, window=240) == ERR_ARG
    assert b"n_fft/2" in lib.honk_last_error()
    assert _call(lib, pcen=pcen, n_mels=0) == ERR_ARG
    assert _call(lib, pcen=pcen, n_mels=0, lens=(), ptrs=(0,) * 7) == ERR_ARG  # the shape is checked first
    if not pcen:
        assert _call(lib, n_dct=0) == ERR_ARG
    else:
        assert _plan(lib, _off([48000]), 8000, pcen=True, n_mels=0)[0] == ERR_ARG


@pytest.mark.parametrize("pcen", [False, True])
def test_short_table_short_workspace_and_unsupported(lib, pcen):
    for lens, stride in [((48000, 16000, 0), 8000), ((56000, 16000), 24000), ((20000, 16400), 400)]:
        off = _off(lens)
        rc, p, _, _ = _plan(lib, off, stride, pcen=pcen)
        assert rc == 0 and p.table_bytes == ROW * (len(lens) + 1)
        assert _plan(lib, off, stride, pcen=pcen, cap=p.table_bytes - 1)[0] == ERR_WORKSPACE
        assert b"table" in lib.honk_last_error()
        assert _call(lib, lens=lens, stride=stride, pcen=pcen, table_bytes=p.table_bytes - 1,
                     ws_bytes=p.workspace_bytes) == ERR_WORKSPACE
        assert b"table" in lib.honk_last_error()
        assert _call(lib, lens=lens, stride=stride, pcen=pcen, table_bytes=p.table_bytes,
                     ws_bytes=p.workspace_bytes - 1) == ERR_WORKSPACE
        assert b"workspace" in lib.honk_last_error()
    for n_fft in (500, 408):  # n_fft not a multiple of 16
        assert _call(lib, pcen=pcen, n_fft=n_fft) == ERR_UNSUPPORTED
        assert b"multiples of 16" in lib.honk_last_error()
        assert _plan(lib, _off([48000]), 8000, pcen=pcen, n_fft=n_fft)[0] == ERR_UNSUPPORTED
    # (n_fft = 400 = 25 * 16 is inside the plan, as for the single-recording calls: host-only query)
    assert _plan(lib, _off([48000]), 8000, pcen=pcen, n_fft=400)[0] == 0
    assert _call(lib, pcen=pcen, hop=150) == ERR_UNSUPPORTED
    assert _call(lib, pcen=pcen, n_mels=129) == ERR_UNSUPPORTED
    assert b"mel" in lib.honk_last_error()
    assert _call(lib, pcen=pcen, lens=(48000,), n_fft=65536, hop=16384, window=40000) == ERR_UNSUPPORTED
    assert b"LDS" in lib.honk_last_error()
    if pcen:  # stage 2's own LDS refusal
        assert _call(lib, pcen=True, lens=(320000,), window=160000, stride=160000, n_fft=32, hop=16) == ERR_UNSUPPORTED
        assert b"tile" in lib.honk_last_error()
        assert _plan(lib, _off([48000]), 8000, pcen=True, n_mels=129)[0] == ERR_UNSUPPORTED


BAD_PARAMS = [dict(s=0.0), dict(s=1.5), dict(eps=0.0), dict(alpha=-0.1), dict(delta=-1.0), dict(r=0.0),
              dict(power=3), dict(s=math.nan), dict(eps=math.nan), dict(alpha=math.inf), dict(delta=math.nan),
              dict(r=math.nan)]


@pytest.mark.parametrize("bad", BAD_PARAMS, ids=lambda d: "%s=%s" % next(iter(d.items())))
def test_bad_pcen_parameters_as_honk_pcen_f32(lib, bad):
    kw = dict(eps=1e-6, s=0.025, alpha=0.98, delta=2.0, r=0.5, power=1)
    kw.update(bad)
    params = _native.PcenParams(kw["eps"], kw["s"], kw["alpha"], kw["delta"], kw["r"], kw["power"])
    assert lib.honk_pcen_f32(P, 1, 16000, P, NFFT, HOP, P, NMELS, ctypes.addressof(params), P, None) == ERR_ARG
    want = lib.honk_last_error()
    assert _call(lib, pcen=True, params=params) == ERR_ARG
    assert lib.honk_last_error() == want
    assert _call(lib, pcen=True, params=params, lens=(), ptrs=(0,) * 7) == ERR_ARG  # checked before n_rec == 0


@pytest.mark.parametrize("pcen", [False, True])
def test_empty_batches_enqueue_nothing(lib, pcen):
    assert _call(lib, pcen=pcen, lens=(), ptrs=(0,) * 7, ws_bytes=0, table_bytes=0) == 0          # n_rec == 0
    assert _call(lib, pcen=pcen, lens=(0, 15999, 100), ptrs=(0,) * 7, ws_bytes=0, table_bytes=0) == 0  # all short
    rc, p, w0, _ = _plan(lib, _off(()), 8000, pcen=pcen)
    assert rc == 0 and p.windows == 0 and p.tiles == 0 and w0.tolist() == [0]
    rc, p, w0, _ = _plan(lib, _off((0, 15999, 100)), 8000, pcen=pcen)
    assert rc == 0 and p.windows == 0 and p.tiles == 0 and p.frames_computed == 0 and w0.tolist() == [0, 0, 0, 0]


# ---- the Python surface on the CPU -----------------------------------------------------------
def test_python_plans():
    ap = AudioPreprocessor()
    off = _off(BATCHES[160], 7)
    rc, plan, w0, table = ap.segments_plan(off, 160)
    assert rc == 0 and plan.windows == 1 + 33 + 1 + 2 and w0.tolist() == [0, 1, 1, 34, 34, 35, 37]
    assert table.dtype == np.int64 and table.nbytes == plan.table_bytes
    rc, pp, w0p, tp = ap.pcen_segments_plan(list(off), 160)
    assert rc == 0 and pp.windows == plan.windows and pp.workspace_bytes > plan.workspace_bytes
    assert np.array_equal(w0p, w0) and np.array_equal(tp, table)
    assert ap.segments_plan([0, 5, 4], 160)[0] == ERR_ARG


@pytest.mark.parametrize("which", ["mfccs", "pcen"])
def test_cpu_segments_equal_the_per_recording_windows(which):
    ap = AudioPreprocessor()
    lens = [16000 + 2 * 4000, 0, 15999, 16000, 16000 + 4000 + 17]
    hole = 100
    x = _pcm(41, hole + sum(lens) + hole)
    off = _off(lens, hole)
    pcm = torch.from_numpy(x)
    segments = getattr(ap, f"compute_{which}_segments")
    windows = getattr(ap, f"compute_{which}_windows")
    out, w0 = segments(pcm, off, 4000)
    assert w0.tolist() == [0, 3, 3, 3, 4, 6] and out.shape == (6, 101, 40) and out.dtype == torch.float32
    for r in range(len(lens)):
        ref = windows(torch.from_numpy(x[off[r]:off[r + 1]].copy()), 4000)
        assert np.array_equal(out[w0[r]:w0[r + 1]].numpy(), ref.numpy()), r
    out, w0 = segments(pcm, [0, 15999, 15999], 4000)
    assert out.shape == (0, 101, 40) and w0.tolist() == [0, 0, 0]
    out, w0 = segments(pcm, [3], 4000)
    assert out.shape == (0, 101, 40) and w0.tolist() == [0]
    for bad in ([0, 20000, 19999], [-1, 20000], [0, len(x) + 1], [], [[0, 1]], [0.0, 16000.0]):
        with pytest.raises(ValueError):
            segments(pcm, bad, 4000)
    with pytest.raises(ValueError):
        segments(pcm.float(), off, 4000)


def test_cpu_label_streams(tmp_path):
    svc = _service(tmp_path, no_cuda=True)
    recs = [_pcm(5, 40000).tobytes(), b"", _pcm(6, 15999).tobytes(), _pcm(7, 16000).tobytes()]
    for ms in (500, 100):
        assert svc.label_streams(recs, ms) == [svc.label_stream(r, ms) for r in recs]
    assert svc.label_streams([]) == []
    assert [len(r) for r in svc.label_streams(recs)] == [4, 0, 0, 1]


@pytest.mark.parametrize("stride_ms", [100, 500, 1500])
def test_cpu_stream_pool_equals_stream_listeners(tmp_path, stride_ms):
    """Three streams, fed in chunks of 2*1234 bytes, 2*777 bytes and whole, the third opened two ticks
    late: per key, the concatenation over the ticks is what a StreamListener fed the same bytes returns."""
    svc = _service(tmp_path, no_cuda=True)
    wavs = {"a": _pcm(6, 52000).tobytes(), "b": _pcm(7, 40000).tobytes(), "c": _pcm(8, 52000).tobytes()}
    chunk = {"a": 2 * 1234, "b": 2 * 777, "c": len(wavs["c"])}
    start = {"a": 0, "b": 0, "c": 2}
    pool = hs.StreamPool(svc, stride_ms)
    listeners = {k: hs.StreamListener(svc, stride_ms) for k in wavs}
    got, want = {k: [] for k in wavs}, {k: [] for k in wavs}
    calls = []
    real = svc.label_streams
    svc.label_streams = lambda recs, *a, **kw: (calls.append(len(recs)), real(recs, *a, **kw))[1]
    ticks = max(start[k] + -(-len(wavs[k]) // chunk[k]) for k in wavs)
    for t in range(ticks):
        fed = {}
        for k in wavs:
            i = (t - start[k]) * chunk[k]
            if t >= start[k] and i < len(wavs[k]):
                fed[k] = wavs[k][i:i + chunk[k]]
        before = len(calls)
        res = pool.feed(fed)
        assert set(res) == set(fed) and len(calls) - before <= 1   # one label_streams call per tick at most
        for k, chunk_bytes in fed.items():
            got[k] += res[k]
            want[k] += listeners[k].feed(chunk_bytes)
            assert pool._streams[k]._buf == listeners[k]._buf and pool._streams[k]._skip == listeners[k]._skip
        if t == 0:
            assert sorted(pool.keys()) == ["a", "b"]
    assert sorted(pool.keys()) == ["a", "b", "c"] and calls and max(calls) >= 1
    for k in wavs:
        assert len(want[k]) == len(list(hs.stride(wavs[k], 32 * stride_ms, 32000))) > 0
        _same(got[k], want[k], 1e-6)
    pool.close("b")
    assert sorted(pool.keys()) == ["a", "c"]
    assert pool.feed({"b": wavs["b"][:100]}) == {"b": []} and "b" in pool.keys()   # reopened, empty tail
    assert len(pool._streams["b"]._buf) == 100
