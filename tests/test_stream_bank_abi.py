"""honk_stream_bank_plan, honk_{mfcc,pcen}_bank_tick_plan / _i16 (csrc/mfcc_stream.hip), host-only: the
slot geometry and every tick's counts against the arithmetic of the definitions (stream_bank_cases.Model),
the argument contract (every call here returns before it would touch the GPU: the pointers are never
dereferenced), and the CPU side of the Python surface (StreamBank on a CPU device,
StreamPool(device_state=True) on a CPU service)."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch

import stream_bank_cases as bc
from honk_amd import _native
from honk_amd import service as hs
from honk_amd.audio import BANK_TABLE_ROW, AudioPreprocessor
from test_mfcc_windows_abi import _pcm, _same, _service

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -2, -3
P = 0x1000  # a non-null stand-in for a device pointer
WIN, NFFT, HOP, NMELS = 16000, 480, 160, 40
NAMES = ("honk_stream_bank_plan", "honk_mfcc_bank_tick_plan", "honk_pcen_bank_tick_plan",
         "honk_mfcc_bank_tick_i16", "honk_pcen_bank_tick_i16")


@pytest.fixture()
def lib():
    from honk_amd import build
    build.build()
    return _native.load()


def _slots(n, **kw):
    s = np.zeros(n, _native.BANK_SLOT_DTYPE)
    for k, v in kw.items():
        s[k] = v
    return s


def _bank(lib, stride, rows=40, window=WIN, n_fft=NFFT, hop=HOP, plan=True):
    p = _native.StreamBankPlan()
    return lib.honk_stream_bank_plan(window, stride, n_fft, hop, rows, ctypes.addressof(p) if plan else None), p


def _tick_plan(lib, slots, ids, off, stride, pcen=False, window=WIN, n_fft=NFFT, hop=HOP, cols=40, table=True,
               cap=None, plan=True, n_fed=None, n_slots=None):
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    off = np.ascontiguousarray(off, dtype=np.int64)
    n = len(ids) if n_fed is None else n_fed
    p = _native.BankTickPlan()
    w0 = np.full(max(n, 0) + 1, -1, np.int64)
    nxt = np.full(max(n, 0), -1, np.int32).repeat(4).view(_native.BANK_SLOT_DTYPE)
    tbl = np.zeros(BANK_TABLE_ROW * (max(n, 0) + 1), np.uint8)
    fn = lib.honk_pcen_bank_tick_plan if pcen else lib.honk_mfcc_bank_tick_plan
    rc = fn(slots.ctypes.data if slots is not None else None, len(slots) if n_slots is None else n_slots,
            ids.ctypes.data, off.ctypes.data, n, window, stride, n_fft, hop, cols, w0.ctypes.data, nxt.ctypes.data,
            tbl.ctypes.data if table else None, tbl.nbytes if cap is None else cap,
            ctypes.addressof(p) if plan else None)
    return rc, p, w0, nxt, tbl


def _call(lib, slots=None, ids=(0, 1), off=(0, 16000, 24000), stride=8000, pcen=False, window=WIN, n_fft=NFFT,
          hop=HOP, n_mels=NMELS, n_dct=40, params=None, ptrs=(P,) * 8, ws_bytes=1 << 24, table_bytes=1 << 16,
          state_bytes=1 << 24, n_slots=None):
    """The _i16 call with stand-in pointers: (chunks, table, state, window table, mel, dct, out, workspace)."""
    slots = _slots(4) if slots is None else slots
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    off = np.ascontiguousarray(off, dtype=np.int64)
    chunks, tbl, state, win, mel, dct, out, ws = ptrs
    head = (chunks, slots.ctypes.data, len(slots) if n_slots is None else n_slots, ids.ctypes.data, off.ctypes.data,
            len(ids), tbl, table_bytes, state, state_bytes, window, stride, win, n_fft, hop, mel, n_mels)
    if pcen:
        pp = ctypes.addressof(params) if params is not None else None
        return lib.honk_pcen_bank_tick_i16(*head, pp, out, ws, ws_bytes, None)
    return lib.honk_mfcc_bank_tick_i16(*head, dct, n_dct, out, ws, ws_bytes, None)


def test_symbols_exist_and_header_agrees(lib):
    src = open(os.path.join(REPO, "include", "honk_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NAMES:
        assert hasattr(lib, name) and name in _native.EXPORTS
        assert re.search(r"\b%s\s*\(" % name, src), name
    for t in ("honk_bank_slot_t", "honk_stream_bank_plan_t", "honk_bank_tick_plan_t"):
        assert t in src
    assert ctypes.sizeof(_native.BankSlot) == 16 == np.dtype(_native.BANK_SLOT_DTYPE).itemsize
    assert ctypes.sizeof(_native.StreamBankPlan) == 8 + 8 * 4
    assert ctypes.sizeof(_native.BankTickPlan) == 8 * 8


@pytest.mark.parametrize("stride,route", [(160, 1), (8000, 1), (15360, 1), (15520, 1), (24000, 2), (400, 0)])
def test_bank_plan_geometry(lib, stride, route):
    rc, p = _bank(lib, stride)
    assert rc == 0
    assert p.cache_rows == bc.cache_rows(stride) == {160: 96, 8000: 47, 15360: 1}.get(stride, 0)
    assert (p.route, p.frames, p.flo, p.fhi, p.tail_capacity, p.row_floats) == (route, 101, 2, 98, WIN - 1, 40)
    # the tail, then two halves of cache_rows rows
    assert p.slot_bytes >= 2 * (WIN - 1) + 2 * p.cache_rows * 40 * 4 and p.slot_bytes % 16 == 0
    assert p.slot_bytes < 2 * (WIN - 1) + 2 * p.cache_rows * 40 * 4 + 64
    rc20, p20 = _bank(lib, stride, rows=20)
    assert rc20 == 0 and p20.cache_rows == p.cache_rows and p20.slot_bytes <= p.slot_bytes


def test_q97_is_the_overlapping_route_without_a_cache(lib):
    """q = 97 = the interior frames of a window: consecutive windows abut, the plan keeps the overlapping
    route's layout and the cache has no row -- the case's cached = 0."""
    assert bc.cache_rows(15520) == 0 and bc.cache_rows(15360) == 1
    assert _bank(lib, 15520)[1].route == 1 and _bank(lib, 15680)[1].route == 2


@pytest.mark.parametrize("pcen", [False, True])
@pytest.mark.parametrize("name", list(bc.CASES))
def test_tick_plans_follow_the_definitions(lib, name, pcen):
    stride, ticks = bc.CASES[name]
    keys = list(bc.streams(name))
    slot = {k: i for i, k in enumerate(keys)}        # (a slot of its own per stream: the bookkeeping alone)
    slots = _slots(len(keys))
    models = {k: bc.Model(stride) for k in keys}
    total = dict(samples_in=0, windows=0, frames_computed=0, frames_reused=0)
    for feed, _, descending in ticks:
        if descending:
            feed = sorted(feed, key=lambda kn: -slot[kn[0]])
        ids = [slot[k] for k, _ in feed]
        lens = []
        for k, n in feed:   # the caller's part of the skip contract: drop before the upload
            drop = min(int(slots["skip"][slot[k]]), n)
            slots["skip"][slot[k]] -= drop
            lens.append(n - drop)
        off = np.concatenate([[0], np.cumsum(lens)])
        before = slots.copy()
        rc, p, w0, nxt, tbl = _tick_plan(lib, slots, ids, off, stride, pcen=pcen)
        assert rc == 0, lib.honk_last_error()
        assert np.array_equal(slots, before)           # the plan commits nothing
        want = [models[k].feed(n) for k, n in feed]
        assert w0.tolist() == np.concatenate([[0], np.cumsum([w[0] for w in want])]).tolist()
        assert p.windows == sum(w[0] for w in want)
        assert p.frames_computed == sum(w[1] for w in want)
        assert p.frames_reused == sum(w[2] for w in want)
        assert p.samples_in == sum(lens) and p.table_bytes == BANK_TABLE_ROW * (len(feed) + 1)
        for j, (k, _) in enumerate(feed):
            tail, cached, skip = models[k].state()
            assert (int(nxt["tail"][j]), int(nxt["cached"][j]), int(nxt["skip"][j])) == (tail, cached, skip), (k, j)
            flips = want[j][0] > 0 and bc.cache_rows(stride) > 0
            assert int(nxt["parity"][j]) == int(before["parity"][slot[k]]) ^ int(flips)
        slots[ids] = nxt
        for k in total:
            total[k] += int(getattr(p, k))
    if name == "ones_9":   # the second tick
        assert (p.samples_in, p.frames_computed, p.frames_reused, p.windows) == (9 * 8000, 9 * (50 + 4), 9 * 47, 9)
        assert p.tiles == 9 * 2 + 2      # 50 frames: a full tile + 18 per stream; 18 edge groups in 2 tiles
    if name == "q1":
        assert total["windows"] == 1 + 3 + 33 + 0 + 1 and total["frames_reused"] == 96 * (3 + 1 + 1)
    if name == "steady_q50":
        assert total["frames_computed"] == 101 + 3 * 54 and total["frames_reused"] == 3 * 47
    if name == "gapped":
        assert total["windows"] == 4 and total["samples_in"] == 96000 - 6000   # 6000 samples dropped in the gap


@pytest.mark.parametrize("pcen", [False, True])
def test_pcen_plan_has_its_own_workspace(lib, pcen):
    slots = _slots(2, tail=[8000, 0], cached=[47, 0], parity=[1, 0])
    rc, p, w0, nxt, _ = _tick_plan(lib, slots, [0, 1], [0, 8000, 8000 + 24000], 8000, pcen=pcen)
    assert rc == 0 and w0.tolist() == [0, 1, 3]
    pcm = 2 * (8000 + 8000 + 24000)
    e_rows = p.frames_computed * NMELS * 4 if pcen else 0
    assert 1024 + e_rows + pcm <= p.workspace_bytes < 1024 + e_rows + pcm + 16
    assert p.frames_computed == (50 + 4) + (50 + 97 + 8) and p.frames_reused == 47


@pytest.mark.parametrize("pcen", [False, True])
def test_argument_errors(lib, pcen):
    for null in range(8):
        if pcen and null == 5:
            continue  # (no dct)
        ptrs = tuple(0 if i == null else P for i in range(8))
        assert _call(lib, pcen=pcen, ptrs=ptrs) == ERR_ARG, null
        assert b"null pointer" in lib.honk_last_error()
    # a tick without a window needs no front-end table and no out, but still its chunks, table, state, workspace
    for null in range(8):
        ptrs = tuple(0 if i == null else P for i in range(8))
        rc = _call(lib, pcen=pcen, ptrs=ptrs, off=(0, 100, 200), ws_bytes=0)
        assert rc == (ERR_ARG if null in (0, 1, 2, 7) else ERR_WORKSPACE), null
    slots = _slots(4)
    assert _tick_plan(lib, slots, [0], [0, 100], 8000, pcen=pcen, plan=False)[0] == ERR_ARG
    assert b"null pointer" in lib.honk_last_error()
    assert _tick_plan(lib, None, [0], [0, 100], 8000, pcen=pcen, n_slots=4)[0] == ERR_ARG
    assert _tick_plan(lib, slots, [0], [0, 100], 8000, pcen=pcen, n_fed=-1)[0] == ERR_ARG
    assert b"negative" in lib.honk_last_error()
    assert _tick_plan(lib, slots, [0], [0, 100], 8000, pcen=pcen, n_slots=-1)[0] == ERR_ARG
    for bad in ([0, 100, 99], [-1, 100, 200], [5, 4, 4]):
        assert _tick_plan(lib, slots, [0, 1], bad, 8000, pcen=pcen)[0] == ERR_ARG, bad
        assert b"offset" in lib.honk_last_error()
        assert _call(lib, pcen=pcen, off=bad) == ERR_ARG, bad
    for ids in ([0, 4], [-1, 0]):        # a slot id out of range
        assert _tick_plan(lib, slots, ids, [0, 100, 200], 8000, pcen=pcen)[0] == ERR_ARG
        assert b"slot" in lib.honk_last_error()
        assert _call(lib, pcen=pcen, ids=ids) == ERR_ARG
    rc, _, w0, nxt, _ = _tick_plan(lib, slots, [2, 2], [0, 100, 200], 8000, pcen=pcen)   # fed twice
    assert rc == ERR_ARG and b"twice" in lib.honk_last_error()
    assert (w0 == -1).all() and (nxt["tail"] == -1).all()   # a refused tick writes nothing
    assert _call(lib, pcen=pcen, ids=[2, 2]) == ERR_ARG
    # a state no tick can have left
    for bad in (dict(tail=WIN), dict(tail=-1), dict(cached=5), dict(parity=2), dict(skip=-1), dict(skip=3, tail=1)):
        s = _slots(2, **bad)
        assert _tick_plan(lib, s, [0], [0, 100], 8000, pcen=pcen)[0] == ERR_ARG, bad
        assert b"state" in lib.honk_last_error()
    # the skip contract of stride > window: the caller drops the samples before the upload
    s = _slots(2, skip=[6000, 0])
    assert _tick_plan(lib, s, [0], [0, 0], 24000, pcen=pcen)[0] == 0
    assert _tick_plan(lib, s, [0], [0, 1], 24000, pcen=pcen)[0] == ERR_ARG
    assert b"skip" in lib.honk_last_error()
    assert _call(lib, pcen=pcen, slots=s, ids=[0], off=[0, 1], stride=24000) == ERR_ARG
    assert _call(lib, pcen=pcen, stride=0) == ERR_ARG
    assert _call(lib, pcen=pcen, window=240) == ERR_ARG
    assert b"n_fft/2" in lib.honk_last_error()
    assert _call(lib, pcen=pcen, n_mels=0) == ERR_ARG
    assert _call(lib, pcen=pcen, n_mels=0, ids=[], off=[0], ptrs=(0,) * 8) == ERR_ARG  # the shape is checked first
    if not pcen:
        assert _call(lib, n_dct=0) == ERR_ARG
    assert _bank(lib, 8000, plan=False)[0] == ERR_ARG
    assert _bank(lib, 0)[0] == ERR_ARG and _bank(lib, 8000, rows=0)[0] == ERR_ARG


@pytest.mark.parametrize("pcen", [False, True])
def test_short_buffers_and_unsupported(lib, pcen):
    slots = _slots(4)
    for stride in (8000, 24000, 400):
        ids, off = [3, 0], [0, 40000, 56000]
        rc, p, _, _, _ = _tick_plan(lib, slots, ids, off, stride, pcen=pcen)
        assert rc == 0 and p.windows > 0
        assert _tick_plan(lib, slots, ids, off, stride, pcen=pcen, cap=p.table_bytes - 1)[0] == ERR_WORKSPACE
        assert b"table" in lib.honk_last_error()
        kw = dict(pcen=pcen, ids=ids, off=off, stride=stride, slots=slots)
        assert _call(lib, table_bytes=p.table_bytes - 1, ws_bytes=p.workspace_bytes, **kw) == ERR_WORKSPACE
        assert b"table" in lib.honk_last_error()
        assert _call(lib, table_bytes=p.table_bytes, ws_bytes=p.workspace_bytes - 1, **kw) == ERR_WORKSPACE
        assert b"workspace" in lib.honk_last_error()
        bank = _bank(lib, stride)[1]
        assert _call(lib, table_bytes=p.table_bytes, ws_bytes=p.workspace_bytes, state_bytes=4 * bank.slot_bytes - 1,
                     **kw) == ERR_WORKSPACE
        assert b"state" in lib.honk_last_error()
    for n_fft in (500, 408):  # exactly the shapes the segments calls refuse
        assert _call(lib, pcen=pcen, n_fft=n_fft) == ERR_UNSUPPORTED
        assert b"multiples of 16" in lib.honk_last_error()
        assert _tick_plan(lib, slots, [0], [0, 100], 8000, pcen=pcen, n_fft=n_fft)[0] == ERR_UNSUPPORTED
        assert _bank(lib, 8000, n_fft=n_fft)[0] == ERR_UNSUPPORTED
    assert _tick_plan(lib, slots, [0], [0, 100], 8000, pcen=pcen, n_fft=400)[0] == 0
    assert _call(lib, pcen=pcen, hop=150) == ERR_UNSUPPORTED
    assert _call(lib, pcen=pcen, n_mels=129) == ERR_UNSUPPORTED
    assert b"mel" in lib.honk_last_error()
    big = _slots(1)
    assert _call(lib, pcen=pcen, slots=big, ids=[0], off=[0, 48000], n_fft=65536, hop=16384, window=40000,
                 stride=16384) == ERR_UNSUPPORTED
    assert b"LDS" in lib.honk_last_error()
    assert _bank(lib, 16384, n_fft=65536, hop=16384, window=40000)[0] == ERR_UNSUPPORTED
    if pcen:
        assert _tick_plan(lib, slots, [0], [0, 100], 8000, pcen=True, cols=129)[0] == ERR_UNSUPPORTED


@pytest.mark.parametrize("pcen", [False, True])
def test_empty_ticks_enqueue_nothing(lib, pcen):
    assert _call(lib, pcen=pcen, ids=[], off=[0], ptrs=(0,) * 8, ws_bytes=0, table_bytes=0, state_bytes=0) == 0
    assert _call(lib, pcen=pcen, ids=[1, 0], off=[7, 7, 7], ptrs=(0,) * 8, ws_bytes=0, table_bytes=0,
                 state_bytes=0) == 0                                   # fed, but no new sample
    rc, p, w0, nxt, _ = _tick_plan(lib, _slots(4, tail=100), [1, 0], [7, 7, 7], 8000, pcen=pcen)
    assert rc == 0 and p.windows == 0 and p.tiles == 0 and p.samples_in == 0 and w0.tolist() == [0, 0, 0]
    assert nxt["tail"].tolist() == [100, 100]
    rc, p, w0, nxt, _ = _tick_plan(lib, _slots(4, tail=100), [1, 0], [0, 15899, 15999], 8000, pcen=pcen)
    assert rc == 0 and p.windows == 0 and p.tiles == 0 and nxt["tail"].tolist() == [15999, 200]   # tails advance


# ---- the Python surface on the CPU -----------------------------------------------------------
@pytest.mark.parametrize("front", ["MFCCs", "PCEN"])
@pytest.mark.parametrize("name", list(bc.CASES))
def test_cpu_bank_adds_up_to_the_whole_recording(name, front):
    ap = AudioPreprocessor()
    got, bank = bc.check(ap, name, front, "cpu")
    assert bank.device.type == "cpu" and bank.stats["ticks"] == len(bc.CASES[name][1])
    assert bank.stats["windows"] == sum(len(r) for r in got.values())
    if name == "ragged":
        assert bank.slots == 8 and len(got) == 6 and len(got["d"]) == 1 and len(got["g"]) == 2   # grown from 2
    if name == "ones_9":
        assert bank.slots == 16 and bank.stats["samples_in"] == 9 * 24000
        assert bank.stats["frames_computed"] == 9 * 101 + 9 * 54 and bank.stats["frames_reused"] == 9 * 47


def test_cpu_bank_surface():
    ap = AudioPreprocessor()
    bank = ap.stream_bank(8000, device="cpu", slots=1)
    assert (bank.route, bank.plan.cache_rows, bank.slots) == ("overlap", 47, 1)
    a = bank.open()
    b = bank.open()
    assert (a, b, bank.slots) == (0, 1, 2)
    x = torch.from_numpy(_pcm(9, 16000))
    out, w0 = bank.tick([b], x, [0, 16000])
    assert out.shape == (1, 101, 40) and w0.tolist() == [0, 1]
    out, w0 = bank.tick([], x[:0], [0])
    assert out.shape == (0, 101, 40) and w0.tolist() == [0]
    bank.close(b)
    assert bank.open() == b and bank._slots[b].tolist() == (0, 0, 0, 0)    # reused: tail 0, cached 0, skip 0
    for bad in (lambda: bank.tick([a, a], x, [0, 1, 2]), lambda: bank.tick([5], x, [0, 1]),
                lambda: bank.tick([a], x.float(), [0, 1]), lambda: bank.tick([a], x, [0, 1, 2]),
                lambda: bank.tick([a], x, [0, 16001]), lambda: bank.close(7)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ValueError):
        AudioPreprocessor(n_fft=500).stream_bank(8000, device="cpu")     # unsupported: n_fft % 16
    with pytest.raises(ValueError):
        ap.stream_bank(8000, front="mel", device="cpu")


@pytest.mark.parametrize("stride_ms", [100, 500, 1500])
def test_cpu_pool_with_device_state_warns_once_and_equals_the_plain_pool(tmp_path, stride_ms):
    svc = _service(tmp_path, no_cuda=True)
    wavs = {"a": _pcm(6, 40000).tobytes(), "b": _pcm(7, 33000).tobytes()}
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        pool = hs.StreamPool(svc, stride_ms, device_state=True)
        plain = hs.StreamPool(svc, stride_ms)
        assert pool.bank is None and plain.bank is None
        for i in range(0, 80000, 2 * 2345):
            fed = {k: w[i:i + 2 * 2345] for k, w in wavs.items() if i < len(w)}
            got, want = pool.feed(fed), plain.feed(fed)
            assert set(got) == set(want)
            for k in got:
                _same(got[k], want[k], 1e-6)
    assert len([w for w in seen if "device_state" in str(w.message)]) == 1
    assert sorted(pool.keys()) == ["a", "b"]
    pool.close("a")
    assert pool.keys() == ["b"]
