"""The schedules of tests/test_stream_bank_abi.py, tests/test_gpu_stream_bank.py and
tests/test_gpu_pcen_stream_bank.py (StreamBank, honk_*_bank_tick_i16; csrc/mfcc_stream.hip) and what the
three files share.  A case is (stride, ticks); a tick is (feed, close, descending): ``feed`` the
(stream, new samples) pairs in feed order, ``close`` the streams closed after the tick, ``descending``:
feed in descending slot order.  A stream is opened at its first feed and owns the recording
``_pcm(SEED + index, its total length)``.

At n_fft 480 / hop 160 / window 16000: FT = 32 frame slots per workgroup, interior frames [flo, fhi] =
[2, 98], 2 + 2 edge frames; q = stride / 160 and the cache holds 97 - q rows on the overlapping route
(q <= 96)."""
import numpy as np
import torch

from test_mfcc_windows_abi import _pcm

WIN, HOP, FLO, FHI, FRAMES = 16000, 160, 2, 98, 101
NINT = FHI - FLO + 1
SEED = 300


def _single(stride, chunks):
    return stride, [([("s0", c)], [], False) for c in chunks]


def _ragged():
    """Five streams and a late key: chunks of 2468 / 1554 samples, 8000 (closed after two ticks: one window
    emitted, a tail and a cache left behind), a new key that opens in the next tick and takes that slot,
    8000 skipping every third tick, and a whole recording opened two ticks late."""
    total = 24000
    plan = [("a", 2468, 0), ("b", 1554, 0), ("d", 8000, 0), ("g", 8000, 2), ("f", 8000, 0), ("c", total, 2)]
    pos = {k: 0 for k, _, _ in plan}
    ticks, t = [], 0
    while any(pos[k] < total for k, _, _ in plan if k != "d"):
        feed = []
        for k, c, start in plan:
            if t < start or pos[k] >= total or (k == "d" and t >= 2) or (k == "f" and t % 3 == 2):
                continue
            n = min(c, total - pos[k])
            feed.append((k, n))
            pos[k] += n
        ticks.append((feed, ["d"] if t == 1 else [], t % 2 == 1))
        t += 1
    return 8000, ticks


CASES = {
    # cached 47; 50 new frames = one full tile + 18; the cache refilled from computed frames only
    "steady_q50": _single(8000, [16000, 8000, 8000, 8000]),
    # cached 96; one new frame per tick (95 rows move cache -> cache); 33 windows in one tick (the computed
    # run starts off a tile boundary, 2 tiles); a chunk that completes nothing; one sample that completes one
    "q1": _single(160, [16000, 160, 160, 160, 33 * 160, 159, 1]),
    "q96": _single(15360, [16000, 15360, 15360]),        # the smallest cache: 1 row
    "q97": _single(15520, [16000, 15520, 15520]),        # the overlapping route's arithmetic with cached = 0
    # 5 windows in a tick: only the first uses the cache, nothing of the old cache survives
    "long_chunk": _single(8000, [16000, 40000, 8000]),
    "gapped": _single(24000, [56000, 10000, 30000]),     # no cache, the host's skip, a tick inside a gap
    "unshared": _single(400, [20000, 399, 401]),         # stride % hop != 0: tails only
    "ragged": _ragged(),
    # the pool's tick: nine streams primed with one window, then one tick of 8000 samples each
    "ones_9": (8000, [([(f"s{i}", 16000) for i in range(9)], [], False),
                      ([(f"s{i}", 8000) for i in range(9)], [], False)]),
}


# The helpers below take the shape by keyword -- window, hop, the interior frames [flo, fhi], frames and cols
# of a row, seed, and case: a (stride, ticks) schedule that is not in CASES -- with the reference shape the
# schedules above are written for as the default.  tests/stream_geometry_cases.py has the shapes off it.
def streams(name, case=None):
    """{stream: total samples} in order of first appearance."""
    total = {}
    for feed, _, _ in (CASES[name] if case is None else case)[1]:
        for k, n in feed:
            total[k] = total.get(k, 0) + n
    return total


def recordings(name, case=None, seed=SEED):
    return {k: _pcm(seed + i, n) for i, (k, n) in enumerate(streams(name, case).items())}


def cache_rows(stride, hop=HOP, flo=FLO, fhi=FHI):
    """The issue's formula: fhi - flo + 1 - q on the overlapping route, else 0."""
    q = stride // hop
    return fhi - flo + 1 - q if stride % hop == 0 and q <= fhi - flo else 0


class Model:
    """The issue's arithmetic for one stream, written from the definitions: N samples received, E windows
    emitted."""

    def __init__(self, stride, window=WIN, hop=HOP, flo=FLO, fhi=FHI, frames=FRAMES):
        self.stride, self.N, self.E = stride, 0, 0
        self.window, self.hop, self.nint, self.frames = window, hop, fhi - flo + 1, frames
        self.rows = cache_rows(stride, hop, flo, fhi)
        self.shared = stride % hop == 0
        self.overlap = self.shared and stride // hop <= fhi - flo

    def cached(self):
        return self.rows if self.E > 0 else 0

    def feed(self, c):
        """-> (n windows, frames_computed, frames_reused) of the tick; advances the stream."""
        cached, q = self.cached(), self.stride // self.hop
        self.N += c
        E = 0 if self.N < self.window else 1 + (self.N - self.window) // self.stride
        n, self.E = E - self.E, E
        if n == 0:
            return 0, 0, 0
        if self.overlap:
            return n, (n - 1) * q + self.nint - cached + n * (self.frames - self.nint), cached
        return n, n * self.frames, 0

    def state(self):
        """(tail, cached, skip)."""
        nxt = self.E * self.stride
        return max(0, self.N - nxt), self.cached(), max(0, nxt - self.N)


def run(ap, name, front, device, slots=2, only=None, reverse=False, before_tick=None, window=WIN, frames=FRAMES,
        cols=40, case=None, seed=SEED):
    """Play a schedule on a fresh bank -> ({stream: its rows over the ticks, concatenated}, bank).
    only: feed these streams alone; reverse: every tick's feed order reversed; before_tick(bank, ids, pcm,
    off) -> a context manager around each tick (the memory-contract tests)."""
    stride, ticks = CASES[name] if case is None else case
    bank = ap.stream_bank(stride, window, front, device, slots)
    recs, pos, slot = recordings(name, case, seed), {}, {}
    rows = {}
    for feed, close, descending in ticks:
        feed = [(k, n) for k, n in feed if only is None or k in only]
        for k, _ in feed:
            if k not in pos:
                slot[k], pos[k], rows[k] = bank.open(), 0, []
        if descending:
            feed.sort(key=lambda kn: -slot[kn[0]])
        if reverse:
            feed = feed[::-1]
        chunks = [recs[k][pos[k]:pos[k] + n] for k, n in feed]
        pcm = torch.from_numpy(np.concatenate(chunks + [np.zeros(0, np.int16)]))
        off = np.concatenate([[0], np.cumsum([n for _, n in feed])]).astype(np.int64)
        ids = [slot[k] for k, _ in feed]
        if before_tick is None:
            x, w0 = bank.tick(ids, pcm, off)
        else:
            x, w0 = before_tick(bank, ids, pcm, off)
        assert x.dtype == torch.float32 and x.shape[1:] == (frames, cols) and x.device.type == torch.device(device).type
        assert w0[0] == 0 and w0[-1] == x.shape[0]
        x = x.cpu().numpy()
        for j, (k, n) in enumerate(feed):
            rows[k].append(x[w0[j]:w0[j + 1]])
            pos[k] += n
        for k in close:
            if k in slot:
                bank.close(slot.pop(k))
    return {k: np.concatenate(v) for k, v in rows.items()}, bank


def whole(ap, name, front, device, window=WIN, case=None, seed=SEED):
    """{stream: compute_{mfccs,pcen}_windows of its whole recording in a buffer of its own}: what the
    ticks' rows must add up to, byte for byte."""
    stride = (CASES[name] if case is None else case)[0]
    windows = ap.compute_pcen_windows if front == "PCEN" else ap.compute_mfccs_windows
    return {k: windows(torch.from_numpy(np.ascontiguousarray(r)).to(device), stride, window).cpu().numpy()
            for k, r in recordings(name, case, seed).items()}


def check(ap, name, front, device, **kw):
    got, bank = run(ap, name, front, device, **kw)
    want = whole(ap, name, front, device, **{k: kw[k] for k in ("window", "case", "seed") if k in kw})
    for k, rows in got.items():
        ref = want[k]
        assert rows.shape == ref.shape and len(ref) > 0 and rows.tobytes() == ref.tobytes(), (name, k)
    return got, bank


# ---- what the two GPU files share --------------------------------------------------------------
def native_tick(arena, bank, ids, pcm, off, frozen):
    """One tick through the C call itself on buffers of the test's own: out and the workspace from ``arena``
    (poisoned, guard-banded), the bank's state (allocated under the same arena), chunks and table uploaded
    here and wrapped in ``frozen``.  Checks the guards, that out is fully written and that no byte of a slot
    that was not fed has changed; commits the bookkeeping as StreamBank.tick does.  -> (out, window0)."""
    import ctypes

    from honk_amd import _native
    ap, dev = bank.ap, bank.device
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    rc, plan, w0, nxt, table = bank._plan(ids, off, bank._slots)
    assert rc == 0
    win, mel, dct = ap._device_tables(dev)
    chunks, table_dev = pcm.to(dev), torch.from_numpy(table).to(dev)
    out = arena.buffer((int(plan.windows), bank.frames, bank.cols), torch.float32, dev, "out")
    ws = arena.buffer((int(plan.workspace_bytes),), torch.uint8, dev, "workspace")
    state = bank._state
    assert any(raw.data_ptr() <= state.data_ptr() < raw.data_ptr() + raw.numel() for raw, _, _ in arena.allocations)
    before = state.clone()
    head = (chunks.data_ptr(), bank._slots.ctypes.data, len(bank._slots), ids.ctypes.data, off.ctypes.data, len(ids),
            table_dev.data_ptr(), table.nbytes, state.data_ptr(), state.numel(), bank.window, bank.stride,
            win.data_ptr(), ap.n_fft, ap.hop_length, mel.data_ptr(), mel.shape[0])
    tail = (out.data_ptr(), ws.data_ptr(), ws.numel(), _native.stream_handle(dev))
    lib = _native.load()
    with frozen(chunks, table_dev):
        if bank.pcen:
            p = ap.pcen_params
            params = _native.PcenParams(p["eps"], p["s"], p["alpha"], p["delta"], p["r"], int(p["power"]))
            rc = lib.honk_pcen_bank_tick_i16(*head, ctypes.addressof(params), *tail)
        else:
            rc = lib.honk_mfcc_bank_tick_i16(*head, dct.data_ptr(), bank.cols, *tail)
        _native.check(rc, "honk_*_bank_tick_i16")
        torch.cuda.synchronize()
    arena.check()
    if arena.fill == 0xFF:   # (NaN as fp32: no finite result keeps it)
        assert not arena.untouched(out)
    sb = int(bank.plan.slot_bytes)
    unfed = [s for s in range(len(bank._slots)) if s not in set(ids.tolist())]
    a, b = state.view(-1, sb), before.view(-1, sb)
    assert torch.equal(a[unfed], b[unfed]), "a slot that was not fed has changed"
    bank._slots[ids] = nxt
    return out, w0


def memory_contract(front, name, want, device, pu, preprocessor=None, **kw):
    """The schedule with the bank's state, every tick's out and workspace poisoned and guard-banded, for
    every fill: the unpoisoned rows.  preprocessor: makes the front end of each fill (None: the default
    one); kw: run()'s shape keywords."""
    from honk_amd.audio import AudioPreprocessor
    for fill in pu.FILLS:
        a = pu.arena(fill)
        with a:
            got, bank = run((preprocessor or AudioPreprocessor)(), name, front, device, slots=2,
                            before_tick=lambda bank, ids, pcm, off: native_tick(a, bank, ids, pcm, off, pu.frozen),
                            **kw)
        a.check()
        assert set(got) == set(want)
        for k in got:
            assert got[k].tobytes() == want[k].tobytes(), (hex(fill), k)


def pools_agree(svc, stride_ms, wavs, chunks, same):
    """StreamPool(svc, ms, device_state=True) against StreamPool(svc, ms), tick by tick on the same bytes:
    three streams, the third opened two ticks late."""
    from honk_amd import service as hs
    bank_pool, plain = hs.StreamPool(svc, stride_ms, device_state=True), hs.StreamPool(svc, stride_ms)
    assert bank_pool.bank is not None and bank_pool.bank.device.type == "cuda"
    start = (0, 0, 2)
    size = [c or len(w) for c, w in zip(chunks, wavs)]
    ticks = max(s + -(-len(w) // c) for s, w, c in zip(start, wavs, size))
    n = [0] * len(wavs)
    for t in range(ticks):
        fed = {}
        for k, w in enumerate(wavs):
            i = (t - start[k]) * size[k]
            if t >= start[k] and i < len(w):
                fed[k] = w[i:i + size[k]]
        got, want = bank_pool.feed(fed), plain.feed(fed)
        assert set(got) == set(want) == set(fed)
        for k in fed:
            assert len(got[k]) == len(want[k])
            same(got[k], want[k], 1e-6)
            n[k] += len(got[k])
    assert min(n) > 0
    assert sorted(bank_pool.keys()) == sorted(plain.keys())
    # only the fed bytes were uploaded
    assert bank_pool.bank.stats["samples_in"] == sum(len(w) // 2 for w in wavs)
    return bank_pool


def nine_streams_one_tick(svc, wavs, which, monkeypatch, same):
    """Nine streams primed with 16000 samples, then 8000 each in one tick: one bank tick call, no segments
    or windows call, one forward; 9 x 8000 samples uploaded."""
    from honk_amd import _native
    from honk_amd import service as hs
    want = {k: svc.label_stream(w) for k, w in wavs.items()}
    pool = hs.StreamPool(svc, device_state=True)
    first = pool.feed({k: w[:32000] for k, w in wavs.items()})
    lib, calls = _native.load(), dict(tick=0, segments=0, windows=0, forward=0)
    names = {"tick": f"honk_{which}_bank_tick_i16", "segments": f"honk_{which}_segments_i16",
             "windows": f"honk_{which}_windows_i16"}
    for kind, name in names.items():
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _k=kind, _r=real: (calls.__setitem__(_k, calls[_k] + 1), _r(*a))[1])
    hook = svc.model.register_forward_hook(lambda *a: calls.__setitem__("forward", calls["forward"] + 1))
    before = dict(pool.bank.stats)
    try:
        got = pool.feed({k: w[32000:] for k, w in wavs.items()})
    finally:
        hook.remove()
    assert calls == dict(tick=1, segments=0, windows=0, forward=1)
    st = pool.bank.stats
    assert st["ticks"] - before["ticks"] == 1 and st["samples_in"] - before["samples_in"] == 9 * 8000
    assert st["frames_computed"] - before["frames_computed"] == 9 * 54
    assert st["frames_reused"] - before["frames_reused"] == 9 * 47
    for k in wavs:
        assert len(first[k]) == len(got[k]) == 1 and len(want[k]) == 2
        same(first[k] + got[k], want[k], 1e-6)
    assert sorted(pool.keys()) == sorted(wavs)
    pool.close(0)
    assert 0 not in pool.keys() and not pool.bank._open[0]
