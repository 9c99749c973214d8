"""Every native call on poisoned, guard-banded device buffers ("Memory contract";
tests/poison_util.py).

The library's scratch, output and packed-weight buffers come from torch.empty: fresh pages are
zero and recycled blocks hold the previous test's data in the same layout, so a kernel that reads
a pad / ring slot / partial-sum slot nothing wrote in this call, leaves the tail of an output
unwritten, or writes a few bytes past its workspace passes every other test.  Here each cell runs
the same call on the same inputs four times -- every buffer the library allocates filled with
0x00, 0x00 again, 0xFF (NaN in every float format, -1 as an integer) and 0x3C (a small finite
value: fmaxf, v_max and the f16x2 admission swallow NaN) -- and asserts

* the two 0x00 runs are bit-equal (the determinism the project claims);
* every fill gives the same bits: the named results (logits, gradients, running statistics, the
  flagged-clip count) and EVERY typed buffer the library allocated during the call (so an output
  element left unwritten shows as the fill it still holds);
* the 0xFF result meets the oracle bar of the case's existing table, unchanged;
* both 4096-byte guards of every allocation still hold the fill (poison_util.arena.check);
* inputs, packed weights and parameters are bit-equal to their clones on entry (frozen).

Cases, inputs, plans and bars are the existing tables' (res_geometry_cases, cnn_geometry_cases,
frontend_geometry_cases, train_geometry_cases, test_gpu_cnn_train, test_gpu_head,
test_gpu_augment, test_gpu_train); the launch plan is asserted on the device before a run counts.

Left out of the bit comparison, each a row of DESIGN.md's table (3 exclusions):
1. honk_mfcc_f32 on its MFMA route sums the mel energies with LDS float atomics (arrival order):
   not bit-repeatable by design.  Every fill is held to the oracle bound and to the other fills
   within that bound; the VALU route of the same cases is compared bit for bit.
2. the pad floats between the regions of the packed weight buffer (res.hip make_layout, round64):
   written by nothing, read by nothing.  The bytes that hold the fill under BOTH poisoned fills are
   masked; everything else of the buffer is compared.
3. the folded BatchNorm's zero-storage placeholder y (conv3x3.py, _ResTail.forward): deliberately
   never written; asserted to still hold the fill.

On the first call that reports a HIP error the session ends (pytest.exit), as in
test_gpu_res_geometry._run."""
import contextlib
import random
import types
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cnn_geometry_cases as cgeo
import decision_replay as dr
import frontend_geometry_cases as fg
import poison_util as pu
import res_geometry_cases as rgeo
import test_gpu_train_geometry as tg   # (its inputs, float64 references and bars)
import train_geometry_cases as tgeo
from golden_util import load_fixture
from honk_amd import _native
from honk_amd import augment as aug
from honk_amd import cnn_train as ct
from honk_amd import conv3x3 as hc
from honk_amd import head_train as ht
from honk_amd import model as hm
from honk_amd import optim
from honk_amd.audio import AudioPreprocessor, dct_filters, mel_filterbank
from oracle import ref_numpy as orc
import pcen_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILLS = (0x00, 0x00, 0xFF, 0x3C)
PACKED_SITE = "honk_amd/model.py:345"      # SpeechResModel._packed: exclusion 2


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _native.load()


ENV_VARS = rgeo.ENV_VARS + cgeo.ENV_VARS + tgeo.ENV_VARS + ("HONK_MFCC_VALU", "HONK_PRECISION")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for v in ENV_VARS:
        monkeypatch.delenv(v, raising=False)


def _setenv(monkeypatch, env):
    for v in ENV_VARS:
        monkeypatch.delenv(v, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ---- the harness ---------------------------------------------------------------------------------
@contextlib.contextmanager
def _device_errors_end_the_run(what):
    try:
        yield
    except RuntimeError as e:
        if "hip" in str(e).lower() or "illegal" in str(e).lower():
            # a device error: nothing more runs on the GPU in this session
            pytest.exit(f"GPU error in {what}: {e}", returncode=3)
        raise


def _bytes(t):
    if not torch.is_tensor(t):
        return np.asarray(t).tobytes()
    return t.detach().contiguous().view(-1).view(torch.uint8).cpu().numpy().tobytes()


def _placeholder(site, t):
    """Exclusion 3: the folded tail's 0-dim y (the only 0-dim allocation of conv3x3.py)."""
    return site.startswith("honk_amd/conv3x3.py:") and t.dim() == 0


def _snapshot(a, ret):
    typed = []
    for site, t in a.typed():
        if _placeholder(site, t):
            assert a.untouched(t) == [0], f"{site}: the folded tail's placeholder y was written"
            continue
        typed.append((site, str(t.dtype), tuple(t.shape), _bytes(t)))
    named = {k: (str(getattr(v, "dtype", type(v))), _bytes(v)) for k, v in ret.items() if v is not None}
    return typed, named


def _first_diff(x, y):
    u, v = np.frombuffer(x, np.uint8), np.frombuffer(y, np.uint8)
    return "sizes differ" if len(u) != len(v) else f"first differing byte {int(np.flatnonzero(u != v)[0])} of {len(u)}"


def _same(what, why, s0, s1, fills):
    (t0, n0), (t1, n1) = s0, s1
    assert sorted(n0) == sorted(n1), (what, why)
    for k in n0:
        assert n0[k] == n1[k], f"{what}: {why}: result '{k}': {_first_diff(n0[k][1], n1[k][1])}"
    assert [e[:3] for e in t0] == [e[:3] for e in t1], f"{what}: {why}: the calls allocated differently"
    for (site, _, shape, b0), (_, _, _, b1) in zip(t0, t1):
        if b0 == b1:
            continue
        if site == PACKED_SITE and 0x00 not in fills:
            # exclusion 2: bytes that hold the fill under both poisoned fills were written by nothing
            u, v = np.frombuffer(b0, np.uint8), np.frombuffer(b1, np.uint8)
            stale = (u == fills[0]) & (v == fills[1])
            assert np.array_equal(u[~stale], v[~stale]), f"{what}: {why}: packed weights differ outside the pads"
            print(f"{what}: {int(stale.sum())} of {len(u)} packed bytes are pads nothing writes")
            assert stale.sum() < 0.02 * len(u), (what, int(stale.sum()), len(u))
            continue
        if site == PACKED_SITE:
            continue   # (against the 0x00 run a pad cannot be told from a written zero: the poisoned pair decides)
        raise AssertionError(f"{what}: {why}: buffer {site} {shape}: {_first_diff(b0, b1)}")


def four_fills(what, call, frozen=(), before=None, bitwise=True, own_buffers=False):
    """`call() -> {name: tensor | number}` under each fill; the checks of the module docstring but
    the oracle's.  Returns the 0xFF run's named results (bitwise=False, exclusion 1: all four runs'),
    as float / int numpy arrays.  own_buffers: `call(arena)`, for a call that hands the C ABI
    buffers of the test's own (arena.buffer)."""
    snaps, rets = [], []
    for fill in FILLS:
        if before is not None:
            before()
        with _device_errors_end_the_run(what):
            with pu.arena(fill) as a:
                with pu.frozen(*frozen):
                    ret = call(a) if own_buffers else call()
                    torch.cuda.synchronize()
            a.check()
            assert a.allocations, f"{what}: no allocation of the library's was intercepted"
            snaps.append(_snapshot(a, ret))
            rets.append({k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v))
                         for k, v in ret.items() if v is not None})
    if not bitwise:
        return rets
    _same(what, "the two 0x00 runs differ (determinism)", snaps[0], snaps[1], (0x00, 0x00))
    _same(what, "the 0xFF fill changed the result", snaps[0], snaps[2], (0x00, 0xFF))
    _same(what, "the 0x3C fill changed the result", snaps[0], snaps[3], (0x00, 0x3C))
    _same(what, "the 0xFF and 0x3C fills differ", snaps[2], snaps[3], (0xFF, 0x3C))
    return rets[2]


def test_the_arena_on_the_device():
    """The interception itself on device tensors: a library allocation (conv3x3._ws) comes back
    poisoned between its guards, and a byte written into a guard (inside the test's own raw
    allocation) is reported with the allocation site."""
    with pu.arena(0x3C) as a:
        ws = hc._ws(100, torch.device(DEV))
        mine = torch.empty(4, device=DEV)
    (raw, nbytes, site), = a.allocations
    assert site.startswith("honk_amd/conv3x3.py:") and nbytes == 100 and raw.is_cuda and mine.storage_offset() == 0
    assert ws.data_ptr() == raw.data_ptr() + pu.G and ws.data_ptr() % 512 == 0 and bool((raw == 0x3C).all())
    a.check()
    raw[pu.G + 100] = 0
    with pytest.raises(AssertionError, match=r"conv3x3\.py:\d+: 100-byte buffer, byte 100 "):
        a.check()


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def n_cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


# ---- res forward ---------------------------------------------------------------------------------
RES_CASES = [rgeo.BY_ID[i] for i in ("res15-1x40", "res15-33x37", "res15-19x11", "res15-5x5", "res8-51x39",
                                     "res26-n_layers6-6x44")]
RES_PRECS = ("f32",) + rgeo.PRECS
_RES = {}


def _res_module(case, prec):
    key = (case.id, prec)
    if key not in _RES:
        cfg, params, _ = rgeo.build(case)
        m = hm.find_model(case.model)(cfg)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
        m = m.eval().to(DEV)
        m.honk_precision = prec
        m.honk_reroute = False   # the kernels of `prec` themselves, whatever the policy
        _RES[key] = m
    return _RES[key]


def _res_inputs(m, x):
    """(device clips, everything the forward must leave alone): the weights are packed here, on
    ordinary memory, so a forward cell poisons the workspace and the outputs only."""
    xd = torch.tensor(np.asarray(x)).to(DEV)
    with torch.cuda.device(xd.device):
        packed = m._packed(xd)
    torch.cuda.synchronize()
    return xd, [xd, packed] + [t for t in m._pack_tensors()]


def _res_fwd(m, xd, schedule="throughput", ordered=False, capacity=None):
    m.honk_schedule, m.honk_stream_ordered, m.honk_rerun_capacity = schedule, ordered, capacity
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)   # no silent fallback to the fp32 layer path
            with torch.no_grad():
                out = m(xd)
        torch.cuda.synchronize()
        n = int(m.honk_last_rerun_dev) if (ordered or schedule == "latency") else int(m.honk_last_rerun)
        return dict(logits=out, flagged=n)
    finally:
        m.honk_schedule, m.honk_stream_ordered, m.honk_rerun_capacity = "throughput", False, None


def _raw(prec, env=None):
    e = dict(env or {})
    if prec == "f16x2":
        e["HONK_F16X2_RERUN"] = "0"   # the kernels' own logits: the admission would replace a wrong clip
    return e


def _res_plan(m, case, B):
    return _native.res_launch_plan(m._desc(case.H, case.W), B)


def _res_oracle(case, clips):
    return np.stack([rgeo.reference(case)[i] for i in clips])


@pytest.mark.parametrize("prec", RES_PRECS)
@pytest.mark.parametrize("case", RES_CASES, ids=repr)
def test_res_forward(monkeypatch, case, prec):
    """honk_res_forward: the default plan, forced-p, w and r at 3 and BMAX clips (at BMAX the
    streams take several clips and the ring slots are reused); f16x2 with the admission off."""
    m = _res_module(case, prec)
    L = rgeo.config(case)["n_layers"]
    if prec == "f32":
        runs = {"default": ({}, ["block_kernel"] * L)}
    else:
        runs = {"default": ({}, case.plan(prec)), "forced-p": (rgeo.FORCED_P, case.plan(prec, forced=True)),
                "w": (dict(HONK_RES_KERNEL="w"), ["block16w_kernel"] * L)}
        if prec != "f16x2":
            runs["r"] = (dict(HONK_RES_KERNEL="r"), ["block16r_kernel"] * L)
    for B in case.batches:
        xd, keep = _res_inputs(m, rgeo.build(case)[2][:B])
        idx, ref, bar = rgeo.compared(B), rgeo.oracle(case, B), rgeo.bar(case, prec)
        for name, (env, want) in runs.items():
            _setenv(monkeypatch, _raw(prec, env))
            assert _res_plan(m, case, B) == want, name
            r = four_fills(f"{case} {prec} {name} B={B}", lambda: _res_fwd(m, xd), keep)
            err = float(np.abs(r["logits"][idx] - ref).max())
            print(f"{case} {prec} {name} B={B}: max|logit - oracle| {err:.2e} (bar {bar:.2e})")
            assert np.isfinite(r["logits"]).all() and err <= bar, (name, B, err, bar)


@pytest.mark.parametrize("prec", RES_PRECS)
@pytest.mark.parametrize("case", RES_CASES, ids=repr)
def test_res_forward_chunked(monkeypatch, case, prec):
    """HONK_RES_CHUNK=4 at 7 clips: a ragged second chunk over the first chunk's leftovers, bit-equal
    to the unchunked run (the table's oracle covers clips 0..2; the identity covers the rest)."""
    m = _res_module(case, prec)
    xd, keep = _res_inputs(m, rgeo.build(case)[2][:7])
    _setenv(monkeypatch, _raw(prec))
    with _device_errors_end_the_run(f"{case} {prec} unchunked"):
        whole = _res_fwd(m, xd)["logits"].cpu().numpy()
    _setenv(monkeypatch, _raw(prec, dict(HONK_RES_CHUNK="4")))
    want = ["block_kernel"] * rgeo.config(case)["n_layers"] if prec == "f32" else case.plan(prec)
    assert _res_plan(m, case, 7) == want
    r = four_fills(f"{case} {prec} chunks of 4", lambda: _res_fwd(m, xd), keep)
    assert pu.bits_equal(r["logits"], whole), float(np.abs(r["logits"] - whole).max())
    assert float(np.abs(r["logits"][:3] - _res_oracle(case, range(3))).max()) <= rgeo.bar(case, prec)


def _scaled(case, B):
    """The first B clips with two of them (one of a single clip) scaled by 3000, out of the f16x2
    calibration as in test_gpu_res_latency: flags, list, gather, re-run and scatter all run.
    -> (clips, the scaled ones, the clips the admission must flag).

    The admission flags a clip whose BatchNorm'd last-layer channel means leave HONK_F16X2_Z_MAX = 8
    (tail_sum_body).  On a map of 25 pixels, calibrated on two clips, a clip of the table's own can
    do that unscaled (res15-5x5 at 17 clips: two do), so the expected flags are the float64 oracle's
    |z| > 8 -- the scaled clips, and nothing else wherever the unscaled clips stay in calibration;
    no clip may sit within 1e-3 of the threshold, where f16x2's rounding could decide."""
    cfg, params, clips = rgeo.build(case)
    x = np.array(clips[:B])
    which = [1, 2] if B >= 3 else [0]
    x[which] *= 3000
    trace = []
    orc.res_forward(params, cfg, x, trace=trace)
    z = np.abs(trace[-1].reshape(B, trace[-1].shape[1], -1).mean(axis=2)).max(axis=1)
    assert not ((z > 8 * (1 - 1e-3)) & (z < 8 * (1 + 1e-3))).any(), z
    flagged = [int(i) for i in np.flatnonzero(z > 8)]
    assert set(which) <= set(flagged)
    return x, which, flagged


@pytest.mark.parametrize("case", RES_CASES, ids=repr)
def test_res_f16x2_admission(monkeypatch, case):
    """f16x2 with the admission on: honk_res_forward, honk_res_forward_ordered with and without a
    capacity below the flagged count, and the latency schedule at 1, 3 and 17 clips.  The flagged
    count is the same under every fill and exactly the number of clips out of calibration (the
    scaled ones: _scaled); the clips left alone meet the table's bar; the paths agree bit for bit
    as test_gpu_ordered / test_gpu_res_latency state."""
    m = _res_module(case, "f16x2")
    bar = rgeo.bar(case, "f16x2")
    got = {}
    for path, B, cap in (("sync", 3, None), ("ordered", 3, None), ("ordered", 3, 1), ("latency", 1, None),
                         ("latency", 3, None), ("latency", 3, 1), ("latency", 17, None)):
        x, which, flagged = _scaled(case, B)
        xd, keep = _res_inputs(m, x)
        assert _res_plan(m, case, B) == case.plan("f16x2")
        kw = dict(sync={}, ordered=dict(ordered=True, capacity=cap), latency=dict(schedule="latency", capacity=cap))[path]
        r = four_fills(f"{case} f16x2 admission {path} B={B} cap={cap}", lambda: _res_fwd(m, xd, **kw), keep)
        print(f"{case} f16x2 admission {path} B={B} cap={cap}: flagged {int(r['flagged'])}, out of calibration {flagged}")
        assert int(r["flagged"]) == len(flagged), (path, B, cap, int(r["flagged"]), flagged)
        kept = flagged[cap:] if cap else []   # (a flagged clip past the capacity keeps its f16x2 logits)
        assert np.isfinite(r["logits"][[i for i in range(B) if i not in kept]]).all()
        alone = [i for i in range(min(B, 3)) if i not in which and i not in kept]
        if alone:
            assert float(np.abs(r["logits"][alone] - _res_oracle(case, alone)).max()) <= bar
        got[path, B, cap] = r["logits"]
    monkeypatch.setenv("HONK_F16X2_RERUN", "0")
    x3, which, flagged = _scaled(case, 3)
    with _device_errors_end_the_run(f"{case} raw f16x2"):
        raw = _res_fwd(m, torch.tensor(x3).to(DEV))["logits"].cpu().numpy()
    sync = got["sync", 3, None]
    assert pu.bits_equal(got["ordered", 3, None], sync) and pu.bits_equal(got["latency", 3, None], sync)
    redone = [i for i in range(3) if i not in flagged[1:]]
    for path in ("ordered", "latency"):   # capacity 1: the flagged clips past the first keep their f16x2 logits
        one = got[path, 3, 1]
        assert pu.bits_equal(one[redone], sync[redone]) and pu.bits_equal(one[flagged[1:]], raw[flagged[1:]])
    assert pu.bits_equal(got["latency", 17, None][:3], sync)   # (a clip's logits do not depend on the batch around it)


@pytest.mark.parametrize("prec", rgeo.PRECS)
@pytest.mark.parametrize("case", RES_CASES, ids=repr)
def test_res_latency_schedule(monkeypatch, case, prec):
    """honk_res_forward_latency (its value buffer behind the throughput workspace) at 1, 3 and 17
    clips: bit-equal to the throughput schedule's ordered forward, clips 0..2 at the table's bar."""
    m = _res_module(case, prec)
    _setenv(monkeypatch, _raw(prec))
    split = 0
    for B in (1, 3, 17):
        xd, keep = _res_inputs(m, rgeo.build(case)[2][:B])
        split += [k for k, _ in _native.res_latency_plan(m._desc(case.H, case.W), B, n_cus())].count("block16s_kernel")
        with _device_errors_end_the_run(f"{case} {prec} ordered B={B}"):
            thr = _res_fwd(m, xd, ordered=True)["logits"].cpu().numpy()
        r = four_fills(f"{case} {prec} latency B={B}", lambda: _res_fwd(m, xd, schedule="latency"), keep)
        assert pu.bits_equal(r["logits"], thr) and int(r["flagged"]) == 0
        k = min(B, 3)
        assert float(np.abs(r["logits"][:k] - _res_oracle(case, range(k))).max()) <= rgeo.bar(case, prec)
    assert split > 0 or prec == "f16x2"   # (test_gpu_res_latency: every case splits in some mode)


# one model per channel-tile count: 19 maps (NT = 2), 33 (NT = 3, 15 pad channels), 45 (NT = 3, 3 pads).
# 33 maps has no table row: built as res_geometry_cases builds one, its simulated errors (rgeo.simulate,
# oracle/res_round_sim.py) and max |logit| written down here so that rgeo.bar applies unchanged.
C33 = rgeo.Case("res15", dict(n_feature_maps=33), 16, 40, 91, {}, {"bf16x3": 5.67e-06, "f16x2": 9.92e-05, "bf16": 3.33e-03},
                0.66)


def _pack_model(which):
    """(module, clips, {precision: (reference logits, bar)})"""
    if which == 19:   # the res15-narrow fixture at 101 x 40: the reference's own logits, the project's 1e-4
        cfg, params, x, logits, meta = load_fixture("res15-narrow-mfcc")
        model, refs = meta["model"], {"f32": (logits, 1e-4), "bf16x3": (logits, 1e-4)}
    else:
        case = C33 if which == 33 else rgeo.BY_ID["res15-33x37"]
        cfg, params, x = rgeo.build(case)
        model, x = case.model, x[:3]
        refs = {p: (rgeo.oracle(case, 3), rgeo.bar(case, p)) for p in RES_PRECS}
    m = hm.find_model(model)(cfg)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
    m = m.eval().to(DEV)
    m.honk_reroute = False
    return m, np.asarray(x, dtype=np.float32), refs


@pytest.mark.parametrize("which", [19, 33, 45])
def test_res_pack_into_poisoned_buffer(monkeypatch, which):
    """honk_res_pack into a poisoned `packed`: the numerics record and the forward of every
    precision from it are the same bits under every fill (each precision reads fragment regions of
    its own), within the bars where a reference exists; the pads between regions: exclusion 2."""
    monkeypatch.setenv("HONK_F16X2_RERUN", "0")
    m, x, refs = _pack_model(which)
    xd = torch.tensor(x).to(DEV)

    def unpack():
        m._honk_packed = m._honk_key = None

    def call():
        out = {}
        for prec in RES_PRECS:
            m.honk_precision = prec
            out[prec] = _res_fwd(m, xd)["logits"]
        rec = _native.res_numerics(m._desc(xd.shape[1], xd.shape[2], "f32"), m._packed(xd), xd.device)[1]
        out["record"] = np.array(list(rec), dtype=np.float32)
        return out

    r = four_fills(f"pack {which} maps", call, [xd] + list(m._pack_tensors()), before=unpack)
    assert np.isfinite(r["record"]).all()
    for prec, (ref, bar) in refs.items():
        err = float(np.abs(r[prec] - ref).max())
        print(f"pack {which} maps {prec}: max|logit - reference| {err:.2e} (bar {bar:.2e})")
        assert err <= bar, (prec, err, bar)
    assert all(np.isfinite(r[p]).all() for p in RES_PRECS)


# ---- cnn forward ---------------------------------------------------------------------------------
CNN_CASES = [cgeo.BY_ID[i] for i in ("trad-101x39", "trad-101x38", "trad-72x40-c2out33", "trad-70x40",
                                     "one-lin6510-37x42", "labels5")]
_CNN = {}


def _cnn_module(case, prec):
    key = (case.id, prec)
    if key not in _CNN:
        cfg, params, _ = cgeo.build(case)
        m = hm.find_model(case.model)(cfg)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
        m = m.eval().to(DEV)
        m.honk_precision = prec
        _CNN[key] = m
    return _CNN[key]


def _cnn_fwd(m, xd):
    with torch.no_grad():
        return dict(logits=m(xd))


@pytest.mark.parametrize("prec", cgeo.PRECS)
@pytest.mark.parametrize("case", CNN_CASES, ids=repr)
def test_cnn_forward(monkeypatch, case, prec):
    """honk_cnn_forward (NHWC intermediates, split weight fragments in the workspace) at 1, 3 and
    300 clips, and 5 clips in chunks of 2 bit-equal to unchunked."""
    m = _cnn_module(case, prec)
    desc = _native.CnnDesc(**m._honk_desc, precision=_native.PRECISIONS[prec])
    assert _native.cnn_launch_plan(desc) == case.plan(prec)
    keep = [p for p in m.parameters()]
    for B in cgeo.BATCHES:
        xd = torch.tensor(cgeo.build(case)[2][:B]).to(DEV)
        r = four_fills(f"{case} {prec} B={B}", lambda: _cnn_fwd(m, xd), [xd] + keep)
        err = float(np.abs(r["logits"][cgeo.compared(B)] - cgeo.oracle(case, B)).max())
        print(f"{case} {prec} B={B}: max|logit - oracle| {err:.2e}")
        assert np.isfinite(r["logits"]).all() and err <= cgeo.ATOL
    xd = torch.tensor(cgeo.build(case)[2][:5]).to(DEV)
    with _device_errors_end_the_run(f"{case} {prec} unchunked"):
        whole = _cnn_fwd(m, xd)["logits"].cpu().numpy()
    monkeypatch.setenv("HONK_CNN_CHUNK", "2")
    r = four_fills(f"{case} {prec} chunks of 2", lambda: _cnn_fwd(m, xd), [xd] + keep)
    assert pu.bits_equal(r["logits"], whole)
    assert float(np.abs(r["logits"][:3] - np.stack([cgeo.reference(case)[i] for i in range(3)])).max()) <= cgeo.ATOL


# ---- the audio front ends ------------------------------------------------------------------------
FRONT_CASES = ("default", "frames113", "hop50", "shortest", "emptybands", "pcen-lds-out")


def _front_call(front, case, pcm, arena=None):
    """audio.py's batch path where AudioPreprocessor can express the shape (the library allocates the
    output); else the C ABI on a poisoned output of the test's own (hop 50)."""
    if case.expressible:
        ap = AudioPreprocessor(n_fft=case.n_fft, hop_ms=case.hop // 16, n_mels=case.n_mels, n_dct_filters=case.n_dct)
        return (ap.compute_mfccs_batch if front == "mfcc" else ap.compute_pcen_batch)(pcm)
    dev = lambda a: torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV)   # noqa: E731
    win, mel = dev(pcen_ref.window(case.n_fft)), dev(mel_filterbank(fg.SR, case.n_fft, case.n_mels, fg.FMIN, fg.FMAX))
    lib, st, B = _native.load(), _native.stream_handle(pcm.device), pcm.shape[0]
    if front == "mfcc":
        dct = dev(dct_filters(case.n_dct, case.n_mels))
        out = arena.buffer((B, case.frames, case.n_dct), torch.float32, DEV)
        rc = lib.honk_mfcc_f32(pcm.data_ptr(), B, case.S, win.data_ptr(), case.n_fft, case.hop, mel.data_ptr(),
                               case.n_mels, dct.data_ptr(), case.n_dct, out.data_ptr(), st)
    else:
        out = arena.buffer((B, case.frames, case.n_mels), torch.float32, DEV)
        rc = lib.honk_pcen_f32(pcm.data_ptr(), B, case.S, win.data_ptr(), case.n_fft, case.hop, mel.data_ptr(),
                               case.n_mels, None, out.data_ptr(), st)
    _native.check(rc, f"honk_{front}_f32")
    return out


@pytest.mark.parametrize("front", fg.FRONTS)
@pytest.mark.parametrize("case_id", FRONT_CASES)
def test_front_end(monkeypatch, case_id, front):
    """honk_mfcc_f32 / honk_pcen_f32 on the table's route and, where that is the MFMA one, on the
    VALU route (pcen-lds-out: PCEN's long route scans the output in place)."""
    case = fg.BY_ID[case_id]
    pcm = torch.from_numpy(np.array(fg.clips(case), dtype=np.float32)).to(DEV)
    ref, e = fg.refs(case_id, front), fg.e32(case_id, front)
    b = fg.bound_of(e)
    for route in [case.route[front]] + (["valu"] if case.route[front] == "mfma" else []):
        _setenv(monkeypatch, {"HONK_MFCC_VALU": "1"} if route != case.route[front] else {})
        rc, plan = _native.front_plan(case.S, case.n_fft, case.hop, case.n_mels, case.n_dct if front == "mfcc" else None)
        assert rc == 0 and _native.FRONT_ROUTES[plan.route] == route and plan.frames == case.frames
        bitwise = not (front == "mfcc" and route == "mfma")   # exclusion 1
        what = f"{case_id} {front} {route}"
        r = four_fills(what, lambda a: dict(out=_front_call(front, case, pcm, a)), [pcm], bitwise=bitwise,
                       own_buffers=True)
        runs = [r] if bitwise else r
        for got in runs:
            got = got["out"]
            assert got.shape == ref.shape and np.isfinite(got).all()
            errs = fg.errors(got, ref)
            assert max(errs) <= b, (what, errs, b)
            assert not got[fg.ZERO].any()   # zero energy passes through log / the root compression: exact zeros
        if not bitwise:
            scale = np.maximum(np.abs(ref).max(axis=(1, 2)), 1e-6)[:, None, None]
            for got in runs[1:]:
                assert float((np.abs(got["out"] - runs[0]["out"]) / scale).max()) <= b
        print(f"FRONT {what}: device {max(fg.errors(runs[-1]['out'], ref)):.2e} bound {b:.2e}")


@pytest.mark.parametrize("which", ["shared", "unshared"])
@pytest.mark.parametrize("case_id", ["win16077", "320-80"])
def test_front_end_windows(case_id, which):
    """honk_mfcc_windows_i16: the output and the (cached) mel-range workspace, a fresh preprocessor
    per fill; then a long recording first and a shorter one on the same cached workspace, bit-equal
    to the shorter one on a fresh preprocessor."""
    case = fg.WIN_BY_ID[case_id]
    stride = case.strides[which == "unshared"]
    x = fg.recording(case, stride)
    pcm = torch.from_numpy(x).to(DEV)
    short = pcm[:case.window + stride].contiguous()   # two windows
    ap = lambda: AudioPreprocessor(n_fft=case.n_fft, hop_ms=case.hop // 16, n_mels=case.n_mels,   # noqa: E731
                                   n_dct_filters=case.n_dct)
    rc, plan = ap().windows_plan(len(x), stride, case.window)
    assert rc == 0 and plan.shared == int(case.shared and which == "shared") and plan.windows == case.n_windows

    def call():
        a = ap()
        whole = a.compute_mfccs_windows(pcm, stride, window=case.window)
        again = a.compute_mfccs_windows(short, stride, window=case.window)    # on the workspace `whole` left
        fresh = ap().compute_mfccs_windows(short, stride, window=case.window)
        assert len(a._dev_ws) == 1
        return dict(whole=whole, again=again, fresh=fresh)

    r = four_fills(f"windows {case_id} {which}", call, [pcm, short])
    assert pu.bits_equal(r["again"], r["fresh"])
    refs = fg.window_refs(case, x, stride)
    b = fg.bound_of(fg.window_e32(case, x, stride, refs))
    assert r["whole"].shape == (case.n_windows, case.frames, case.n_dct) and np.isfinite(r["whole"]).all()
    assert max(fg.errors(r["whole"], np.stack(refs))) <= b


# ---- res training --------------------------------------------------------------------------------
TRAIN_CASES = [tgeo.BY_ID[i] for i in ("19-1x4-d1", "19-7x12-d3", "19-49x20-d1", "19-17x5-d1", "19-3x260-d1",
                                       "45-5x7-d2", "19-2x286-d1")]


def _train_batches(case):
    """2 clips; 19-49x20-d1 (both fixed instances) also past one tile per workgroup of the conv and
    of the weight gradient (train_geometry_cases.many_tile_batches on its fewer bands)."""
    return [2] + ([tgeo.many_tile_batches(min(case.nband()), n_cus())[0]] if case.id == "19-49x20-d1" else [])


@pytest.mark.parametrize("case", TRAIN_CASES, ids=repr)
def test_train_convs(case):
    """Conv forward, input gradient and weight gradient (per-split partials in the workspace; the
    same-conv path pads its input there) under every environment of ENVS, at the 1e-5 of
    test_kernels_match_float64."""
    C, H, W, d = case.shape
    for B in _train_batches(case):
        t = tg._data(case, B)
        idx = tg._clips(B)
        refs = (tg._ref_conv(t["x"], t["w"], d, False, idx), tg._ref_conv(t["dy"], t["w"], d, True, idx),
                tg._ref_wgrad(t["x"], t["dy"], d))
        for env in tgeo.ENVS:
            with tgeo.environment(env):
                if case.family() is not None:
                    assert tgeo.signature(B, C, H, W, d, n_cus())[0] == case.sigs[env], env
                else:
                    assert not hc._dedicated(C, H, W, d)
                r = four_fills(f"{case} {env} B={B}", lambda: dict(
                    y=hc._conv(t["x"], t["w"], flip=False, d=d), dx=hc._conv(t["dy"], t["w"], flip=True, d=d),
                    dw=hc._wgrad(t["x"], t["dy"], d=d)), [t["x"], t["dy"], t["w"]])
            errs = (_rel(r["y"][idx], refs[0]), _rel(r["dx"][idx], refs[1]), _rel(r["dw"], refs[2]))
            print(case, env, "B", B, "fwd / dgrad / wgrad vs float64: %.2e %.2e %.2e" % errs)
            assert max(errs) < 1e-5, (env, errs)


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("case", [c for c in TRAIN_CASES if "s" in c.flags()], ids=repr)
def test_train_epilogue_chain(case, fold):
    """The statistics epilogue, the mask words and the fused / folded / masked tails: two blocks
    chained as the model chains them (test_gpu_train_geometry._chain) under the four fills; then
    test_fused_epilogue_chain itself, with every bar it has, on 0xFF buffers."""
    for bi, B in enumerate(_train_batches(case)):
        assert tg._batches(case)[bi] == B
        t = tg._data(case, B)
        assert "f" in case.flags()
        four_fills(f"{case} chain fold={fold} B={B}", lambda: tg._chain(case, t, fold=fold)[0], list(t.values()))
        if not fold:
            with _device_errors_end_the_run(f"{case} test_fused_epilogue_chain"):
                with pu.arena(0xFF) as a:
                    tg.test_fused_epilogue_chain(case, bi)
                    torch.cuda.synchronize()
                a.check()


@pytest.mark.parametrize("case", TRAIN_CASES, ids=repr)
def test_train_tail_and_batchnorm(case):
    """honk_res_tail_fwd / bwd_f32 and honk_bn_train_fwd / bwd_f32 on a workspace of their own
    ([c][S][2] double partials, then 4 c floats): y within 1e-6, running statistics rtol 1e-5 /
    atol 1e-6, gradients within 1e-5 of float64 (the bars of test_gpu_train_geometry and
    test_batchnorm_train_matches_torch)."""
    C, H, W, d = case.shape
    t = tg._data(case, 2)
    h, old, gy, gs = t["x"], t["old"], t["dy"], t["gs"]
    x = t["x"] * 3 + 1.5
    def call():
        hh, oo = h.clone().requires_grad_(True), old.clone().requires_grad_(True)
        bn, bn2 = (torch.nn.BatchNorm2d(C, affine=False).to(DEV).train() for _ in range(2))
        y, s = hc.res_tail(hh, oo, bn, keep_s=True)
        gh, gold = torch.autograd.grad([y, s], [hh, oo], [gy, gs])
        xx = x.clone().requires_grad_(True)
        assert hc.bn_supported(xx, bn2)
        yb = hc.batch_norm_train(xx, bn2)
        (dxb,) = torch.autograd.grad(yb, xx, gy)
        return dict(y=y.detach(), s=s.detach(), gh=gh, gold=gold, rm=bn.running_mean, rv=bn.running_var,
                    yb=yb.detach(), dxb=dxb, rm2=bn2.running_mean, rv2=bn2.running_var)

    r = four_fills(f"{case} tail / batchnorm", call, [h, old, gy, gs, x])
    assert pu.bits_equal(r["s"], (torch.relu(h) + old).cpu().numpy())
    stats = types.SimpleNamespace(running_mean=torch.from_numpy(r["rm"]), running_var=torch.from_numpy(r["rv"]))
    y64, _, var = tg._check_tail_forward(f"{case} tail", torch.from_numpy(r["s"]), torch.from_numpy(r["y"]), stats)
    g64, gh64 = tg._bn_bwd64(gy, y64, var, mask=~(h <= 0), gs=gs)
    assert _rel(r["gold"], g64) < 1e-5 and _rel(r["gh"], gh64) < 1e-5
    # BatchNorm alone: float64 on the CPU, and torch's own fp32 as the yardstick of the gradient
    x64 = x.double().cpu().requires_grad_(True)
    bn64 = torch.nn.BatchNorm2d(C, affine=False).double()
    yb64 = bn64(x64)
    (dx64,) = torch.autograd.grad(yb64, x64, gy.double().cpu())
    bnt = torch.nn.BatchNorm2d(C, affine=False).to(DEV)
    xt = x.clone().requires_grad_(True)
    (dxt,) = torch.autograd.grad(bnt(xt), xt, gy)
    assert _rel(r["yb"], yb64) < 1e-6 and _rel(r["dxb"], dx64) <= max(_rel(dxt, dx64), 1e-5)
    torch.testing.assert_close(torch.from_numpy(r["rm2"]), bnt.running_mean.cpu(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(torch.from_numpy(r["rv2"]), bnt.running_var.cpu(), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("B,C,H,W,pool", [(3, 19, 9, 7, (2, 3)), (2, 8, 180, 200, (4, 3))])
def test_train_stem(B, C, H, W, pool):
    """honk_res_stem_fwd_f32 / wgrad_f32 (per-workgroup partials in the workspace): the bars of
    test_res_stem_matches_float64."""
    g = torch.Generator(device=DEV).manual_seed(B + C + H + W)
    x = torch.randn(B, H, W, device=DEV, generator=g)
    conv0 = torch.nn.Conv2d(1, C, (3, 3), padding=(1, 1), bias=False).to(DEV)
    pm = torch.nn.AvgPool2d(pool)
    assert hc.stem_supported(x, conv0, pm)
    gy = torch.randn(B, C, H // pool[0], W // pool[1], device=DEV, generator=g)

    def call():
        y = hc.stem(x, conv0, pm)
        (dw,) = torch.autograd.grad(y, conv0.weight, gy)
        return dict(y=y.detach(), dw=dw)

    r = four_fills(f"stem {(B, C, H, W, pool)}", call, [x, conv0.weight, gy])
    w64 = conv0.weight.detach().double().cpu().requires_grad_(True)
    ref = F.avg_pool2d(F.relu(F.conv2d(x.double().cpu().unsqueeze(1), w64, padding=1)), pool)
    (dw64,) = torch.autograd.grad(ref, w64, gy.double().cpu())
    assert r["y"].shape == tuple(ref.shape) and _rel(r["y"], ref.detach()) < 1e-6 and _rel(r["dw"], dw64) < 1e-5


@pytest.mark.parametrize("step", tgeo.STEPS[:2], ids=repr)
def test_train_step(step):
    """One native training step (every allocation of the forward and the backward poisoned):
    loss, gradients and running statistics the same bits under every fill, and within the bounds of
    the decision-matched float64 replay (test_train_step_vs_decision_matched_float64)."""
    cfg = tg._cfg(step)
    torch.manual_seed(11)
    m = hm.find_model(step.model)(cfg)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    m = m.to(DEV).train()
    g = torch.Generator().manual_seed(12 + step.B)
    x = torch.randn(step.B, step.H, step.W, generator=g)
    y = torch.randint(0, cfg["n_labels"], (step.B,), generator=g)
    xd, yd = x.to(DEV), y.to(DEV)
    decs = []

    def reset():
        m.load_state_dict(state)
        for p in m.parameters():
            p.grad = None

    def call():
        dec = dr.Decisions()
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)   # no fallback to PyTorch / MIOpen
            with dr.record(dec):
                loss = F.cross_entropy(m(xd), yd)
            loss.backward()
        decs.append(dec)
        out = dict(loss=loss.detach())
        out.update({"g:" + k: p.grad for k, p in m.named_parameters()})
        out.update({"b:" + k: v for k, v in m.state_dict().items() if "running_" in k})
        return out

    r = four_fills(f"{step} step", call, [xd, yd] + list(m.parameters()), before=reset)
    ref = dr.replay_step(cfg, step.model, state, x.numpy(), y.numpy(), decs[2], dict(lr=0.1, momentum=0.9))
    got = (max(dr.rel_err(r["g:" + k], ref["g"][k]) for k in ref["g"]), abs(float(r["loss"]) - ref["loss"]),
           max(dr.rel_err(r["b:" + k], ref["b"][k]) for k in ref["b"]))
    print(step, "grad rel %.2e loss abs %.2e running-stat rel %.2e" % got)
    assert ref["ambiguous"] == 0 and decs[2].count() > 0
    for v, bound, what in zip(got, (1e-4, 1e-5, 1e-5), ("grad", "loss", "running stats")):
        assert v <= bound, f"{what}: {v:.3e} > {bound:.0e} vs the decision-matched float64 step"


# ---- cnn training, the head, the augmentation, the optimizer ---------------------------------------
@pytest.mark.parametrize("B,C,H,W,N,KH,KW,stride,xgrad", [(7, 5, 11, 9, 3, 3, 2, (1, 1), True),
                                                          (4, 3, 17, 13, 70, 4, 3, (2, 3), False),
                                                          (3, 64, 41, 16, 64, 10, 4, (1, 1), True)])
def test_cnn_conv_relu(B, C, H, W, N, KH, KW, stride, xgrad):
    """conv_relu forward and backward (the weight gradient's per-split partials; conv2's input
    gradient pads g' and flips the weights in the workspace): test_conv_relu_grads_vs_float64's bars."""
    g = torch.Generator().manual_seed(B * 1000 + C)
    x = torch.randn(B, C, H, W, generator=g)
    conv = torch.nn.Conv2d(C, N, (KH, KW), stride=stride)
    with torch.no_grad():
        conv.bias.normal_(0, 0.1, generator=g)
    conv = conv.to(DEV)
    xd = x.to(DEV)
    gy = torch.randn(B, N, (H - KH) // stride[0] + 1, (W - KW) // stride[1] + 1, generator=g).to(DEV)

    def call():
        xx = xd.clone().requires_grad_(xgrad)
        assert ct.conv_supported(xx, conv)
        y = ct.conv_relu(xx, conv)
        gr = torch.autograd.grad(y, [conv.weight, conv.bias] + ([xx] if xgrad else []), gy)
        return dict(y=y.detach(), dw=gr[0], db=gr[1], dx=gr[2] if xgrad else None)

    r = four_fills(f"conv_relu {(B, C, H, W, N, KH, KW, stride)}", call, [xd, gy, conv.weight, conv.bias])
    w64, b64 = conv.weight.detach().cpu().double(), conv.bias.detach().cpu().double()
    pre = F.conv2d(x.double(), w64, b64, stride=stride)
    np.testing.assert_allclose(r["y"].astype(np.float64), pre.clamp_min(0).numpy(), atol=2e-5, rtol=1e-5)
    gp = gy.cpu().double() * torch.from_numpy(r["y"] > 0).double()
    assert dr.rel_err(r["dw"], torch.nn.grad.conv2d_weight(x.double(), w64.shape, gp, stride=stride).numpy()) <= 1e-5
    assert dr.rel_err(r["db"], gp.sum((0, 2, 3)).numpy()) <= 1e-5
    if xgrad:
        assert dr.rel_err(r["dx"], torch.nn.grad.conv2d_input(x.shape, w64, gp, stride=stride).numpy()) <= 1e-5


def test_cnn_max_pool():
    """max_pool (2, 3) forward and backward on test_maxpool_bwd_bitwise_vs_torch's input: torch's bits."""
    k = (2, 3)
    g = torch.Generator().manual_seed(k[0] * 10 + k[1])
    x = torch.randint(-3, 4, (4, 6, 25, 17), generator=g).float()
    x[0, 0, :4, :4] = float("-inf")
    x[1, 2, 3:6, 3:6] = float("nan")
    x[2, 3, 0, 1] = float("nan")
    x[3, 1, 7, 2] = -float("nan")
    x[3, 1, 8, 2] = float("nan")
    gy = torch.randn(4, 6, 25 // k[0], 17 // k[1], generator=g)
    xr = x.clone().requires_grad_(True)
    F.max_pool2d(xr, k).backward(gy)
    xd, gyd, pool = x.to(DEV), gy.to(DEV), torch.nn.MaxPool2d(k)

    def call():
        xx = xd.clone().requires_grad_(True)
        assert ct.pool_supported(xx, pool)
        out = ct.max_pool(xx, pool)
        (gx,) = torch.autograd.grad(out, xx, gyd)
        return dict(out=out.detach(), gx=gx)

    r = four_fills("max_pool (2, 3)", call, [xd, gyd])
    ref = F.max_pool2d(x, k)
    out = torch.from_numpy(r["out"])
    assert torch.equal(out.nan_to_num(7.5), ref.nan_to_num(7.5)) and torch.equal(out.isnan(), ref.isnan())
    assert torch.equal(torch.from_numpy(r["gx"]), xr.grad)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("B,K,N", [(5, 7, 3), (7, 2496, 32)])
def test_head_linear(B, K, N, relu):
    g = torch.Generator().manual_seed(B + K + N)
    lin = torch.nn.Linear(K, N)
    x, gy = torch.randn(B, K, generator=g), torch.randn(B, N, generator=g)
    lin_d = torch.nn.Linear(K, N).to(DEV)
    lin_d.load_state_dict(lin.state_dict())
    xd, gyd = x.to(DEV), gy.to(DEV)

    def call():
        xx = xd.clone().requires_grad_(True)
        y = ht.linear_relu(xx, lin_d) if relu else ht.linear(xx, lin_d)
        gx, gw, gb = torch.autograd.grad(y, (xx, lin_d.weight, lin_d.bias), gyd)
        return dict(y=y.detach(), gx=gx, gw=gw, gb=gb)

    r = four_fills(f"linear {(B, K, N, relu)}", call, [xd, gyd, lin_d.weight, lin_d.bias])
    lin64, x64 = lin.double(), x.double().requires_grad_(True)
    y64 = F.relu(lin64(x64)) if relu else lin64(x64)
    refs = (y64,) + torch.autograd.grad(y64, (x64, lin64.weight, lin64.bias), gy.double())
    for k, ref in zip(("y", "gx", "gw", "gb"), refs):
        assert _rel(r[k], ref.detach()) < 1e-5, k


@pytest.mark.parametrize("shape", [(5, 7, 25, 13), (2, 3, 1, 1)])
def test_head_spatial_mean(shape):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(*shape, generator=g)
    gz = torch.randn(shape[0], shape[1], generator=g)
    xd, gzd = x.to(DEV), gz.to(DEV)

    def call():
        xx = xd.clone().requires_grad_(True)
        z = ht.spatial_mean(xx)
        (gx,) = torch.autograd.grad(z, xx, gzd)
        return dict(z=z.detach(), gx=gx)

    r = four_fills(f"spatial_mean {shape}", call, [xd, gzd])
    x64 = x.double().requires_grad_(True)
    z64 = x64.view(shape[0], shape[1], -1).mean(2)
    (gx64,) = torch.autograd.grad(z64, x64, gz.double())
    assert _rel(r["z"], z64.detach()) < 1e-6 and _rel(r["gx"], gx64) < 1e-6


@pytest.mark.parametrize("B,N,scale", [(3, 4, 1.0), (1000, 35, 0.5)])
def test_head_cross_entropy(B, N, scale):
    g = torch.Generator().manual_seed(B + N)
    z = torch.randn(B, N, generator=g) * 3
    y = torch.randint(0, N, (B,), generator=g)
    zd, yd = z.to(DEV), y.to(DEV)

    def call():
        zz = zd.clone().requires_grad_(True)
        loss = ht.CrossEntropyLoss()(zz, yd)
        (gz,) = torch.autograd.grad(loss * scale, zz)
        return dict(loss=loss.detach(), gz=gz)

    r = four_fills(f"cross entropy {(B, N)}", call, [zd, yd])
    z64 = z.double().requires_grad_(True)
    loss64 = torch.nn.CrossEntropyLoss()(z64, y)
    (gz64,) = torch.autograd.grad(loss64 * scale, z64)
    assert abs(float(r["loss"]) - float(loss64)) <= 1e-6 * max(1.0, abs(float(loss64)))
    assert _rel(r["gz"], gz64) < 1e-5


def test_device_augment_edges():
    """honk_augment_f32 on test_kernel_edges_vs_oracle's parameters: the CPU oracle's bits."""
    L, B = 3000, 9
    g = np.random.default_rng(5)
    audio = (g.standard_normal((B, L)) * 2).astype(np.float32)
    audio[3, 17] = np.nan
    bank = g.standard_normal(L + 50).astype(np.float32)
    a = aug.DeviceAugment([bank], dict(input_length=L, timeshift_ms=100), device=DEV, rng=random.Random(0))
    params = [(0, 0, 0.05, 2), (50, -1600, 0.099, 2), (49, 1600, 0.0, 0), (10, 3, 0.03, 2), (0, -2999, 0.07, 2),
              (0, 2999, 0.01, 0), (25, 0, 0.08, 3), (0, 0, 0.0, 1), (5, -7, 0.02, 2)]
    src = torch.from_numpy(audio).to(DEV)
    r = four_fills("DeviceAugment edges", lambda: dict(out=a._apply(src, params)), [src, a.bank])
    for b, (off, shift, amp, flags) in enumerate(params):
        want = orc.augment_clip(audio[b], bank[off:off + L], shift, amp, bool(flags & 1), bool(flags & 2), L)
        np.testing.assert_array_equal(r["out"][b], want.astype(np.float32))


def test_flat_sgd_step():
    """FlatParams' bucket and gradient bucket between guards (the step is in place, so their
    contents are the data; 58 floats: a ragged last float4) around FlatSGD.step with momentum:
    test_sgd_kernel_matches_torch's bar against torch.optim.SGD, nothing outside the buckets touched."""
    torch.manual_seed(3)
    proto = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Linear(5, 3))
    n = sum(p.numel() for p in proto.parameters())
    assert n % 4 == 2
    grads = [torch.randn(n, generator=torch.Generator().manual_seed(s)).to(DEV) for s in (1, 2)]

    def call():
        mod = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Linear(5, 3))
        mod.load_state_dict(proto.state_dict())
        flat = optim.FlatParams(mod.to(DEV))
        sgd = optim.FlatSGD(flat, lr=0.1, momentum=0.9, weight_decay=1e-3)
        for gr in grads:
            flat.grad.copy_(gr)
            sgd.step()
        return dict(data=flat.data, buf=sgd.buf)

    r = four_fills("FlatSGD.step", call, grads)
    ref = torch.nn.Parameter(torch.cat([p.detach().reshape(-1) for p in proto.parameters()]).to(DEV))
    opt = torch.optim.SGD([ref], lr=0.1, momentum=0.9, weight_decay=1e-3)
    for gr in grads:
        ref.grad = gr.clone()
        opt.step()
    torch.testing.assert_close(torch.from_numpy(r["data"]), ref.detach().cpu(), rtol=1e-6, atol=1e-7)
