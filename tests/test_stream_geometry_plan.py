"""The host side of tests/stream_geometry_cases.py: the batched and the resident front ends off
16000 / 480 / 160 / 40 without a GPU.  The plan queries (honk_stream_bank_plan, honk_*_bank_tick_plan,
honk_*_segments_plan) against the arithmetic of the definitions as stream_geometry_cases derives it, the
schedule's own coverage at every (shape, stride), the CPU bank against the CPU whole-recording call, and the
refusals: construction refuses what a tick refuses, found by an empty tick (no pointer read, nothing
enqueued), so all of it runs here."""
import ctypes

import numpy as np
import pytest

import stream_bank_cases as bc
import stream_geometry_cases as sg
from honk_amd import _native
from honk_amd.audio import BANK_TABLE_ROW, AudioPreprocessor
from test_stream_bank_abi import ERR_UNSUPPORTED, _bank, _call, _slots, _tick_plan

ROUTES = {"unshared": 0, "overlap": 1, "gapped": 2}
IDS = [f"{g}-{s}" for g, s in sg.COMBOS]


@pytest.fixture()
def lib():
    from honk_amd import build
    build.build()
    return _native.load()


def _cdiv(a, b):
    return -(-a // b)


def test_the_table_reaches_what_it_is_for():
    """The shapes by their derived constants: every gs from 1 to 4, head != tail, rows of 13, 20, 40, 80 and
    128 floats, an odd tail capacity, no interior frame, and every route at the six shapes with more strides."""
    g = sg.BY_ID
    assert {x.gs for x in sg.GEOS} == {1, 2, 3, 4}
    assert (g["800-160"].head, g["800-160"].tail, g["800-160"].frames, g["800-160"].nint) == (3, 3, 101, 95)
    assert (g["1024-128"].head, g["1024-128"].tail, g["1024-128"].frames, g["1024-128"].nint) == (4, 4, 65, 57)
    assert (g["win16240"].head, g["win16240"].tail, g["win16240"].frames, g["win16240"].fhi) == (2, 1, 102, 100)
    assert (g["win800"].frames, g["win800"].nint) == (6, 2) and g["win300"].nint <= 0
    assert g["win16077"].slot_bytes(8000, "MFCCs")[0] == 16076
    assert g["dct13"].slot_bytes(1920, "MFCCs")[1:] == (35, 19648)     # 16000 + two halves of 1820 bytes, up to 16
    assert {x.cols(f) for x in sg.GEOS for f in sg.FRONTS} == {13, 20, 40, 80, 128}
    for id in sg.MORE_STRIDES:
        x = g[id]
        assert [x.route(s) for s, _ in x.strides] == ["overlap", "unshared", "overlap", "overlap", "gapped", "gapped"]
        assert [x.cache_rows(s) for s, _ in x.strides][2:4] == [x.nint - 1, 0] and x.strides[5][0] > x.window
    assert [g["win800"].route(s) for s, _ in g["win800"].strides] == ["overlap", "overlap", "gapped", "unshared"]
    assert len(sg.COMBOS) == 14 * 2 + 6 * 4 + 4
    assert all(x.why for x in sg.GEOS) and all(why for x in sg.GEOS for _, why in x.strides)


@pytest.mark.parametrize("geo_id,stride", sg.COMBOS, ids=IDS)
def test_the_schedule_covers_its_ways_to_go_wrong(geo_id, stride):
    seen = sg.coverage(sg.BY_ID[geo_id], stride)
    assert seen == dict(many=True, none=True, one_sample=True, reused=True, grew=True)


@pytest.mark.parametrize("geo_id,stride", sg.COMBOS, ids=IDS)
def test_bank_plan_follows_the_definitions(lib, geo_id, stride):
    geo = sg.BY_ID[geo_id]
    for front in sg.FRONTS:
        rc, p = _bank(lib, stride, rows=geo.cols(front), window=geo.window, n_fft=geo.n_fft, hop=geo.hop)
        assert rc == 0, lib.honk_last_error()
        assert (p.frames, p.flo, p.fhi, p.route, p.row_floats) == (geo.frames, geo.flo, geo.fhi,
                                                                   ROUTES[geo.route(stride)], geo.cols(front))
        assert (p.tail_capacity, p.cache_rows, p.slot_bytes) == geo.slot_bytes(stride, front)
        assert p.q == (stride // geo.hop if geo.shared(stride) else 0)


@pytest.mark.parametrize("pcen", [False, True], ids=["mfcc", "pcen"])
@pytest.mark.parametrize("geo_id,stride", sg.COMBOS, ids=IDS)
def test_tick_plans_follow_the_definitions(lib, geo_id, stride, pcen):
    """tests/test_stream_bank_abi.py's check of every tick's counts and next states, at this shape."""
    geo = sg.BY_ID[geo_id]
    _, ticks = sg.schedule(geo, stride)
    keys = list(bc.streams(None, (stride, ticks)))
    slot = {k: i for i, k in enumerate(keys)}        # (a slot of its own per stream: the bookkeeping alone)
    slots = _slots(len(keys))
    models = {k: geo.model(stride) for k in keys}
    rows = geo.cache_rows(stride)
    kw = dict(pcen=pcen, window=geo.window, n_fft=geo.n_fft, hop=geo.hop, cols=geo.cols("PCEN" if pcen else "MFCCs"))
    edge = geo.head + geo.tail
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
        rc, p, w0, nxt, _ = _tick_plan(lib, slots, ids, off, stride, **kw)
        assert rc == 0, lib.honk_last_error()
        assert np.array_equal(slots, before)
        want = [models[k].feed(n) for k, n in feed]
        assert w0.tolist() == np.concatenate([[0], np.cumsum([w[0] for w in want])]).tolist()
        assert p.windows == sum(w[0] for w in want)
        assert p.frames_computed == sum(w[1] for w in want)
        assert p.frames_reused == sum(w[2] for w in want)
        assert p.samples_in == sum(lens) and p.table_bytes == BANK_TABLE_ROW * (len(feed) + 1)
        # the tiles: per stream its computed shared frames in tiles of FT (overlapping) or its windows' own
        # segment tiles, then the edge groups of all the tick's windows, FT // gs to a tile
        if geo.route(stride) == "overlap":
            tiles = sum(_cdiv(w[1] - w[0] * edge, sg.FT) for w in want if w[0])
        else:
            nfw = geo.nint if geo.route(stride) == "gapped" else geo.frames
            tiles = p.windows * _cdiv(nfw, sg.FT)
        if geo.route(stride) != "unshared":
            assert p.edge_frames == p.windows * edge
            tiles += _cdiv(2 * p.windows, sg.FT // geo.gs)
        assert p.tiles == tiles
        for j, (k, _) in enumerate(feed):
            tail, cached, skip = models[k].state()
            assert (int(nxt["tail"][j]), int(nxt["cached"][j]), int(nxt["skip"][j])) == (tail, cached, skip), (k, j)
            assert tail <= geo.window - 1
            flips = want[j][0] > 0 and rows > 0
            assert int(nxt["parity"][j]) == int(before["parity"][slot[k]]) ^ int(flips)
        slots[ids] = nxt


@pytest.mark.parametrize("geo_id,stride", sg.COMBOS, ids=IDS)
def test_segments_plans_follow_the_definitions(geo_id, stride):
    geo = sg.BY_ID[geo_id]
    ap = geo.ap()
    edge, route = geo.head + geo.tail, geo.route(stride)
    for name, (lens, _, hole) in sg.batches(geo, stride).items():
        import segments_cases as sc
        _, off, _, _ = sc.batch(name, seed=sg.batch_seed(geo, stride, name), window=geo.window, spec=(lens, stride, hole))
        W = [sc.n_windows(int(b - a), stride, geo.window) for a, b in zip(off[:-1], off[1:])]
        for fn in (ap.segments_plan, ap.pcen_segments_plan):
            rc, plan, w0, _ = fn(off, stride, geo.window)
            assert rc == 0
            assert w0.tolist() == np.concatenate([[0], np.cumsum(W)]).tolist() and plan.frames == geo.frames
            q = stride // geo.hop
            if route == "overlap":
                G = [(w - 1) * q + geo.nint if w else 0 for w in W]
                tiles, shared = sum(_cdiv(x, sg.FT) for x in G), sum(G)
            else:
                nfw = geo.nint if route == "gapped" else geo.frames
                tiles, shared = sum(W) * _cdiv(nfw, sg.FT), sum(W) * geo.nint if route == "gapped" else 0
            if route != "unshared":
                tiles += _cdiv(2 * sum(W), sg.FT // geo.gs)
                assert (plan.shared_frames, plan.edge_frames) == (shared, sum(W) * edge)
            assert (plan.windows, plan.tiles) == (sum(W), tiles)
        if name == "ragged":
            assert W == [1, 5, 0, 0, 2]
        if name == "holes":
            assert len(W) == 9 and sum(W) == 8 and off[0] == hole > 0


@pytest.mark.parametrize("front", sg.FRONTS)
@pytest.mark.parametrize("geo_id,stride", sg.COMBOS, ids=IDS)
def test_cpu_bank_adds_up_to_the_whole_recording(geo_id, stride, front):
    geo = sg.BY_ID[geo_id]
    got, bank = bc.check(geo.ap(), None, front, "cpu", case=sg.schedule(geo, stride), seed=sg.bank_seed(geo, stride),
                         **geo.shape(front))
    assert bank.device.type == "cpu" and bank.slots == 4
    assert [len(got[k]) for k in "abcde"] == [7, 7, 7, 1, 7]
    assert bank.stats == sg.expected_stats(geo, stride)
    assert (bank.plan.tail_capacity, bank.plan.cache_rows, bank.plan.slot_bytes) == geo.slot_bytes(stride, front)


# ---- refusals ------------------------------------------------------------------------------------
def _empty_tick(lib, pcen, geo=None, **kw):
    """The _i16 call with no fed stream and null pointers: the shape checks alone."""
    if geo is not None:
        kw = dict(dict(window=geo.window, n_fft=geo.n_fft, hop=geo.hop, n_mels=geo.n_mels, n_dct=geo.n_dct), **kw)
    params = None
    if pcen:
        p = AudioPreprocessor().pcen_params
        params = _native.PcenParams(p["eps"], p["s"], p["alpha"], p["delta"], p["r"], int(p["power"]))
    return _call(lib, slots=_slots(1), ids=[], off=[0], pcen=pcen, params=params, ptrs=(0,) * 8, ws_bytes=0,
                 table_bytes=0, state_bytes=0, n_slots=0, **kw)


@pytest.mark.parametrize("pcen", [False, True], ids=["mfcc", "pcen"])
def test_an_empty_tick_takes_every_shape_of_the_table(lib, pcen):
    for geo_id, stride in sg.COMBOS:
        assert _empty_tick(lib, pcen, sg.BY_ID[geo_id], stride=stride) == 0, (geo_id, stride, lib.honk_last_error())


@pytest.mark.parametrize("pcen", [False, True], ids=["mfcc", "pcen"])
def test_an_empty_tick_refuses_what_a_tick_with_a_window_refuses(lib, pcen):
    """The mel bands (the MFCC plan calls never see them) and the frame-tile kernel's LDS plan with the
    epilogue's tiles and the group table (honk_stream_bank_plan has neither): the status and the reason of
    the tick that completes a window, before any sample is fed."""
    slots = _slots(1)
    # (a tick that completes a window, with an empty workspace: a shape it takes stops at HONK_ERR_WORKSPACE,
    # before anything is enqueued)
    full = dict(slots=slots, ids=[0], pcen=pcen, ws_bytes=0)
    if pcen:
        p = AudioPreprocessor().pcen_params
        full["params"] = _native.PcenParams(p["eps"], p["s"], p["alpha"], p["delta"], p["r"], int(p["power"]))
    assert _empty_tick(lib, pcen, n_mels=129, stride=8000) == ERR_UNSUPPORTED
    assert b"mel bands" in lib.honk_last_error()
    assert _call(lib, off=[0, 16000], n_mels=129, stride=8000, **full) == ERR_UNSUPPORTED
    if not pcen:   # honk_stream_bank_plan and the MFCC tick plan pass: nothing but the tick refuses
        assert _bank(lib, 8000)[0] == 0 and _tick_plan(lib, slots, [0], [0, 16000], 8000)[0] == 0
    # the first n_fft from 1600 up, at hop 160 and an unshared stride, whose slot plan passes and whose tick
    # does not: the LDS instance
    found = None
    for n_fft in range(1600, 2400, 16):
        kw = dict(window=16000, n_fft=n_fft, hop=160, stride=8007)
        if _bank(lib, 8007, n_fft=n_fft)[0] != 0:
            break
        rc_full = _call(lib, off=[0, 16000], **kw, **full)
        rc_empty = _empty_tick(lib, pcen, **kw)
        assert rc_empty == (ERR_UNSUPPORTED if rc_full == ERR_UNSUPPORTED else 0), n_fft
        if rc_full == ERR_UNSUPPORTED:
            assert b"LDS" in lib.honk_last_error()
            found = n_fft
            break
        assert rc_full == -3
    print(f"first n_fft the tick refuses and honk_stream_bank_plan takes ({'pcen' if pcen else 'mfcc'}): {found}")
    assert found is not None


def test_a_cpu_mfcc_bank_takes_129_bands():
    """On a CPU device a tick is compute_mfccs_windows per stream, which has no such limit: the empty tick is
    the device bank's check."""
    import torch
    from test_mfcc_windows_abi import _pcm
    ap = AudioPreprocessor(n_mels=129)
    bank = ap.stream_bank(4000, 8000, "MFCCs", "cpu")
    x = torch.from_numpy(_pcm(11, 12000))
    out, w0 = bank.tick([bank.open()], x, [0, 12000])
    assert out.shape == (2, 51, 40) and w0.tolist() == [0, 2]
    assert np.array_equal(out.numpy(), ap.compute_mfccs_windows(x, 4000, 8000).numpy())
