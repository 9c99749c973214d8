"""compute_{mfccs,pcen}_segments and StreamBank on the device off 16000 / 480 / 160 / 40: every shape and
stride of tests/stream_geometry_cases.py, both front ends (honk_*_segments_i16, honk_*_bank_tick_i16;
csrc/mfcc_stream.hip).

The defining properties are the ones of tests/test_gpu_*_segments.py and tests/test_gpu_*_stream_bank.py --
a recording's rows of a batch, and a stream's rows over its ticks, are byte-equal to compute_*_windows of the
whole recording alone -- through the same helpers (segments_cases, stream_bank_cases) with the shape passed
in.  The oracle pin ties that reference to the float64 oracles at the project's front-end rule, used as
tests/test_gpu_frontend_geometry.py and tests/test_gpu_pcen_windows.py use it: atol = sim.bound(e32) *
max(max|ref window|, 1e-6), rtol = 0, e32 the error of oracle/frontend_f32_sim.py on the same windows; no
tolerance is invented here, and no recording's bound may sit at the 1e-4 cap (the seeds are chosen so:
stream_geometry_cases.RESEED) but three groups at 128 bands, where no seed does and the cap is the bound.  It
prints e32, the device error and their ratio per (shape, stride, front): the table of DESIGN.md."""
import functools
import warnings

import numpy as np
import pytest
import torch

import poison_util as pu
import segments_cases as sc
import stream_bank_cases as bc
import stream_geometry_cases as sg
from honk_amd import service as hs
from honk_amd.audio import AudioPreprocessor
from oracle import frontend_f32_sim as sim
from test_mfcc_windows_abi import _pcm, _service

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = [f"{g}-{s}" for g, s in sg.COMBOS]
combos = pytest.mark.parametrize("geo_id,stride", sg.COMBOS, ids=IDS)
fronts = pytest.mark.parametrize("front", sg.FRONTS)


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _windows_call(geo, front, rec, stride):
    ap = geo.ap()
    fn = ap.compute_pcen_windows if front == "PCEN" else ap.compute_mfccs_windows
    return fn(torch.from_numpy(np.array(rec)).to(DEV), stride, geo.window).cpu().numpy()   # (a writable copy)


# ---- the reference of everything below, against the float64 oracle -------------------------------------
@fronts
@combos
def test_whole_recording_calls_meet_the_oracle(geo_id, stride, front):
    _gpu()
    geo = sg.BY_ID[geo_id]
    which = "pcen" if front == "PCEN" else "mfcc"
    worst = (0.0, 0.0)
    for name, rec in sg.pinned_recordings(geo_id, stride).items():
        wins = sg.windows_of(geo, rec, stride)
        if not wins:
            continue
        refs = [sg.oracle(geo, front, w) for w in wins]
        ys = np.stack(wins).astype(np.float32) / np.float32(32768.)
        e = sim.e32(which, ys, refs, **sg.sim_kw(geo, front))
        b = sim.bound(e)
        assert 0 < e <= sg.e32_max(geo, stride, name), (name, e)     # 16 x e32 under the cap (but sg.AT_CAP)
        got = _windows_call(geo, front, rec, stride)
        assert got.shape == (len(wins), geo.frames, geo.cols(front)) and np.isfinite(got).all()
        dev = max(sim.rel_err(got[w], r) for w, r in enumerate(refs))
        if dev / e >= worst[1] / max(worst[0], 1e-30):
            worst = (e, dev)
        for w, ref in enumerate(refs):
            np.testing.assert_allclose(got[w], ref, atol=b * max(np.abs(ref).max(), 1e-6), rtol=0, err_msg=name)
    e, dev = worst
    print(f"STREAM {geo_id} stride {stride} {which}: e32 {e:.2e}  device {dev:.2e}  ratio {dev / e:.2f}  "
          f"bound {sim.bound(e):.2e}")


# ---- segments ----------------------------------------------------------------------------------------------
@fronts
@combos
def test_segments_rows_equal_the_single_recording_call(geo_id, stride, front):
    """Every batch of the shape: rows per recording, window0 = the cumulative counts, the ranges that are no
    recording own no row and are never read, the reversed batch gives the same rows per recording."""
    _gpu()
    geo = sg.BY_ID[geo_id]
    which, kw = sg.WHICH[front], geo.shape(front)
    outs = {}
    for name, spec in sg.batches(geo, stride).items():
        ap, seed = geo.ap(), sg.batch_seed(geo, stride, name)
        out, blocks = sc.check_rows(which, ap, name, spec=spec, seed=seed, **kw)
        assert out.any() and len(out) == {"ragged": 8, "holes": 8, "ones": 9, "long": 42}[name]
        _, rev = sc.check_rows(which, ap, name, reverse=True, spec=spec, seed=seed, **kw)
        assert len(rev) == len(blocks)
        for a, b in zip(rev, blocks[::-1]):
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), name
        outs[name] = out
    assert outs["holes"].tobytes() == outs["ragged"].tobytes()     # the same recordings without the holes
    spec, seed = sg.batches(geo, stride)["holes"], sg.batch_seed(geo, stride, "holes")
    pcm, off, _, _ = sc.batch("holes", seed=seed, window=geo.window, spec=spec)
    mask = sc.unowned("holes", seed=seed, window=geo.window, spec=spec)
    assert off[0] == spec[2] > 0 and mask.sum() == 6 * spec[2] and mask[:spec[2]].all() and mask[-spec[2]:].all()
    y = pcm.copy()
    y[mask] = 12345
    got, _ = sc.segments(which, geo.ap(), y, off, stride, geo.window)
    assert got.tobytes() == outs["holes"].tobytes()


# ---- the bank ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bank_case(geo_id, stride, front):
    """({stream: rows}, stats, plan fields) of the schedule on a bank grown from 2 slots, every stream checked
    against the whole recording's windows; computed once, read-only."""
    geo = sg.BY_ID[geo_id]
    got, bank = bc.check(geo.ap(), None, front, DEV, **_run_kw(geo, stride, front))
    for rows in got.values():
        rows.setflags(write=False)
    p = bank.plan
    return got, dict(bank.stats), (p.tail_capacity, p.cache_rows, p.slot_bytes), bank.slots


def _run_kw(geo, stride, front):
    return dict(case=sg.schedule(geo, stride), seed=sg.bank_seed(geo, stride), **geo.shape(front))


@fronts
@combos
def test_bank_ticks_add_up_to_the_whole_recording(geo_id, stride, front):
    """... over the schedule; two runs give the same bits; the reversed feed order the same rows; each stream
    alone in a bank of one slot the same bytes; the counters are the CPU bank's and the Model's; the slot
    geometry is the header's formulas."""
    _gpu()
    geo = sg.BY_ID[geo_id]
    kw = _run_kw(geo, stride, front)
    got, stats, plan, slots = _bank_case(geo_id, stride, front)
    assert [len(got[k]) for k in "abcde"] == [7, 7, 7, 1, 7] and all(r.any() for r in got.values())
    assert slots == 4 and plan == geo.slot_bytes(stride, front)
    again, _ = bc.run(geo.ap(), None, front, DEV, **kw)
    rev, _ = bc.run(geo.ap(), None, front, DEV, reverse=True, **kw)
    assert set(again) == set(rev) == set(got)
    for k in got:
        assert again[k].tobytes() == got[k].tobytes(), k
        assert rev[k].shape == got[k].shape and rev[k].tobytes() == got[k].tobytes(), k
        alone, bank = bc.run(geo.ap(), None, front, DEV, slots=1, only={k}, **kw)
        assert bank.slots == 1 and list(alone) == [k]
        assert alone[k].shape == got[k].shape and alone[k].tobytes() == got[k].tobytes(), k
    _, cpu = bc.run(geo.ap(), None, front, "cpu", **kw)
    assert stats == cpu.stats == sg.expected_stats(geo, stride)
    assert (stats["frames_reused"] > 0) == (geo.cache_rows(stride) > 0)


# ---- memory contract ---------------------------------------------------------------------------------------
@fronts
@pytest.mark.parametrize("geo_id,stride", [("dct13", 160), ("win16077", 4000)], ids=["dct13-q1", "win16077-shared"])
def test_bank_memory_contract(geo_id, stride, front):
    """dct13 at q = 1: 46 rows of 13 floats, halves of 2392 bytes (the second one 8-byte aligned only, odd row
    strides); win16077: a tail of 16 076 samples in 32 160 bytes.  State, out and workspace poisoned and
    guard-banded under every fill, no unfed slot changes, out fully written."""
    _gpu()
    geo = sg.BY_ID[geo_id]
    assert (geo_id, stride) in sg.COMBOS and geo.cache_rows(stride) > 0
    got, _, _, _ = _bank_case(geo_id, stride, front)
    bc.memory_contract(front, None, got, DEV, pu, preprocessor=geo.ap, **_run_kw(geo, stride, front))


@fronts
def test_segments_memory_contract(front):
    """800-160 (10 groups per edge tile), the ragged batch with holes, at the table's shared stride."""
    _gpu()
    geo = sg.BY_ID["800-160"]
    stride = geo.strides[0][0]
    which, spec, seed = sg.WHICH[front], sg.batches(geo, stride)["holes"], sg.batch_seed(geo, stride, "holes")
    want, _ = sc.check_rows(which, geo.ap(), "holes", spec=spec, seed=seed, **geo.shape(front))
    pcm_np, off, _, _ = sc.batch("holes", seed=seed, window=geo.window, spec=spec)
    pcm = torch.from_numpy(pcm_np).to(DEV)
    for fill in pu.FILLS:
        a = pu.arena(fill)
        out = sc.native_segments(a, which, geo.ap(), pcm, off, stride, pu.frozen, window=geo.window)
        a.check()
        assert out.cpu().numpy().tobytes() == want.tobytes(), hex(fill)
        if fill == 0xFF:   # (NaN as fp32: no finite result keeps it)
            assert not a.untouched(out)


# ---- refusals ----------------------------------------------------------------------------------------------
REFUSED = {
    "129bands": dict(n_mels=129),                    # the MFCC bank: no plan call sees the mel bands
    "2048-16": dict(n_fft=2048, hop_ms=1),           # more than 32 edge frames per side / the LDS plan
    "1760-160": dict(n_fft=1760),                    # the frame-tile LDS plan within FT * sizeof(Group) of 160 KiB
}
REFUSED_STRIDES = {"129bands": (1920, 1927), "2048-16": (992, 999), "1760-160": (8007,)}   # the windows table's
REFUSED_WINDOW = {"129bands": 8000, "2048-16": 4000, "1760-160": 16000}


@fronts
@pytest.mark.parametrize("name", list(REFUSED))
def test_construction_refuses_what_a_tick_refuses(name, front):
    """ValueError at construction, which StreamPool's fallback relies on -- not RuntimeError from the first
    tick that completes a window."""
    _gpu()
    for stride in REFUSED_STRIDES[name]:
        with pytest.raises(ValueError):
            AudioPreprocessor(**REFUSED[name]).stream_bank(stride, REFUSED_WINDOW[name], front, DEV)
    # the shape next to it is taken, and its first window-completing tick passes
    near = dict(REFUSED[name])
    if name == "129bands":
        near["n_mels"] = 128
    elif name == "2048-16":
        near = dict(n_fft=1024, hop_ms=2)
    else:
        near["n_fft"] = 1744
    ap = AudioPreprocessor(**near)
    W, s = REFUSED_WINDOW[name], REFUSED_STRIDES[name][-1]
    bank = ap.stream_bank(s, W, front, DEV, slots=1)
    x = torch.from_numpy(_pcm(5, W + s))
    out, w0 = bank.tick([bank.open()], x, [0, W + s])
    fn = ap.compute_pcen_windows if front == "PCEN" else ap.compute_mfccs_windows
    assert w0.tolist() == [0, 2] and out.cpu().numpy().tobytes() == fn(x.to(DEV), s, W).cpu().numpy().tobytes()


@fronts
@pytest.mark.parametrize("name", list(REFUSED))
def test_segments_at_the_refused_shapes_equal_the_per_recording_fallback(name, front):
    _gpu()
    ap = AudioPreprocessor(**REFUSED[name])
    W, which = REFUSED_WINDOW[name], sg.WHICH[front]
    windows = ap.compute_pcen_windows if front == "PCEN" else ap.compute_mfccs_windows
    for stride in REFUSED_STRIDES[name]:
        lens = [W + stride, 0, W, W - 1, W + 2 * stride + 1]
        recs = [_pcm(70 + i, n) for i, n in enumerate(lens)]
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        pcm = torch.from_numpy(np.concatenate(recs)).to(DEV)
        out, w0 = getattr(ap, f"compute_{which}_segments")(pcm, off, stride, W)
        assert w0.tolist() == [0, 2, 2, 3, 3, 6] and out.shape[0] == 6 and out.is_cuda
        want = torch.cat([windows(torch.from_numpy(r).to(DEV), stride, W) for r in recs if len(r) >= W])
        assert out.cpu().numpy().tobytes() == want.cpu().numpy().tobytes() and out.cpu().numpy().any()


def test_pool_over_a_refused_preprocessor_warns_once_and_equals_the_plain_pool(tmp_path):
    """129 mel bands under 40 DCT rows: the model input stays 101 x 40, the device bank is refused at
    construction, and the pool works with host tails."""
    _gpu()
    svc = _service(tmp_path, no_cuda=False)
    svc.audio_processor = AudioPreprocessor(n_mels=129)
    wavs = {"a": _pcm(6, 40000).tobytes(), "b": _pcm(7, 33000).tobytes()}
    n = 0
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        pool = hs.StreamPool(svc, 500, device_state=True)
        plain = hs.StreamPool(svc, 500)
        assert pool.bank is None and plain.bank is None
        for i in range(0, 80000, 2 * 2345):
            fed = {k: w[i:i + 2 * 2345] for k, w in wavs.items() if i < len(w)}
            got, want = pool.feed(fed), plain.feed(fed)
            assert set(got) == set(want)
            for k in got:
                assert got[k] == want[k]
                n += len(got[k])
    assert n == 4 + 3
    assert len([w for w in seen if "device_state" in str(w.message) and "mel bands" in str(w.message)]) == 1
