"""The audio front ends off 16000/480/160/40, host-only: honk_mfcc_plan / honk_pcen_plan against the
table of frontend_geometry_cases.py (route, frames, launches, LDS bytes; every boundary with a case on
each side), the refusals (every call here returns before it would touch the GPU: the stand-in pointers
are never dereferenced), the numpy paths at the case's bound, and the separation condition: each named
mistake applied to the float64 oracle moves every non-zero clip of every case by at least ten bounds."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import frontend_geometry_cases as fg
from honk_amd import _native
from honk_amd.audio import AudioPreprocessor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED = -1, -2
P = 0x1000  # a non-null stand-in for a device pointer
IDS = [c.id for c in fg.BATCH]
EXPRESSIBLE = [c.id for c in fg.BATCH if c.expressible]
SEPARATION = 10.0


@pytest.fixture()
def lib():
    from honk_amd import build
    build.build()
    return _native.load()


def _plan(case, front):
    return _native.front_plan(case.S, case.n_fft, case.hop, case.n_mels, case.n_dct if front == "mfcc" else None)


def _preprocessor(case):
    return AudioPreprocessor(n_fft=case.n_fft, hop_ms=case.hop // 16, n_mels=case.n_mels, n_dct_filters=case.n_dct)


def _last_error(lib):
    return lib.honk_last_error().decode(errors="replace")


def test_symbols_exist_and_header_agrees(lib):
    src = open(os.path.join(REPO, "include", "honk_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("honk_mfcc_plan", "honk_pcen_plan"):
        assert hasattr(lib, name) and name in _native.EXPORTS
        assert re.search(r"\b%s\s*\(" % name, src), name
    assert "honk_front_plan_t" in src
    assert ctypes.sizeof(_native.FrontPlan) == 4 * 4 + 8
    for name, value in (("HONK_FRONT_ROUTE_MFMA", "mfma"), ("HONK_FRONT_ROUTE_VALU", "valu")):
        m = re.search(r"#define\s+%s\s+(\d+)" % name, src)
        assert m and _native.FRONT_ROUTES[int(m.group(1))] == value


def test_network_cases_cover_the_network_tables():
    import cnn_geometry_cases
    import res_geometry_cases
    import train_geometry_cases
    hw = {(c.H, c.W) for c in (res_geometry_cases.CASES + cnn_geometry_cases.CASES + train_geometry_cases.CASES
                               + train_geometry_cases.STEPS) if (c.H - 1) * 160 > 240}
    assert sorted(hw) == fg.NETWORK_HW
    for H, W in fg.NETWORK_HW:
        case = fg.BY_ID[f"net-{H}x{W}"]
        assert (case.frames, case.n_dct) == (H, W)


@pytest.mark.parametrize("valu_env", [False, True], ids=["default", "HONK_MFCC_VALU"])
@pytest.mark.parametrize("case_id", IDS)
def test_plan_matches_table(lib, monkeypatch, case_id, valu_env):
    case = fg.BY_ID[case_id]
    if valu_env:
        monkeypatch.setenv("HONK_MFCC_VALU", "1")
    else:
        monkeypatch.delenv("HONK_MFCC_VALU", raising=False)
    for front in fg.FRONTS:
        rc, p = _plan(case, front)
        assert rc == 0, _last_error(lib)
        route = "valu" if valu_env else case.route[front]
        assert _native.FRONT_ROUTES[p.route] == route, (front, case.why)
        assert (p.frames, p.n_bins) == (case.frames, case.n_bins)
        assert p.launches == (2 if (front, route) == ("pcen", "valu") else 1)
        assert 0 < p.lds_bytes <= (160 if route == "mfma" else 64) * 1024


def test_every_boundary_has_a_case_on_each_side(lib, monkeypatch):
    monkeypatch.delenv("HONK_MFCC_VALU", raising=False)
    plan = lambda cid, front: _plan(fg.BY_ID[cid], front)[1]  # noqa: E731
    for name in ("112 frames", "160 KiB MFCC plan", "160 KiB PCEN plan", "n_fft % 16", "hop % 4"):
        inside, outside, front = fg.BOUNDARIES[name]
        assert _native.FRONT_ROUTES[plan(inside, front).route] == "mfma", name
        assert _native.FRONT_ROUTES[plan(outside, front).route] == "valu", name
    assert (fg.BY_ID["frames112"].frames, fg.BY_ID["frames113"].frames) == (112, 113)
    for cid in ("mfcc-lds-in", "mfcc-lds-out", "pcen-lds-in", "pcen-lds-out"):
        assert fg.BY_ID[cid].frames <= 112 and fg.BY_ID[cid].n_fft % 16 == 0 and fg.BY_ID[cid].hop % 4 == 0
    assert fg.BY_ID["nfft488"].n_fft % 16 and fg.BY_ID["hop50"].hop % 4
    assert fg.BY_ID["hop100"].hop % 4 == 0 and fg.BY_ID["hop100"].hop % 16 and fg.BY_ID["hop100"].S % 100
    inside, outside, front = fg.BOUNDARIES["64 KiB opt-in"]
    assert plan(inside, front).lds_bytes <= 64 * 1024 < plan(outside, front).lds_bytes
    inside, outside, _ = fg.BOUNDARIES["full last VALU workgroup"]
    assert fg.BY_ID[inside].frames % 4 == 0 and fg.BY_ID[outside].frames % 4 == 1   # FPB = 4 frames per workgroup
    inside, outside, _ = fg.BOUNDARIES["even n_fft"]
    assert fg.BY_ID[inside].frames == 1 + fg.BY_ID[inside].S // fg.BY_ID[inside].hop
    assert fg.BY_ID[outside].frames == 100 == fg.BY_ID[outside].S // fg.BY_ID[outside].hop
    for (cid, front), lds in fg.PINNED_LDS.items():
        assert plan(cid, front).lds_bytes == lds, (cid, front)


@pytest.mark.parametrize("n_fft,mfcc_bands,pcen_bands", [(512, 56, 45), (480, 59, 48)])
def test_lds_boundaries(lib, monkeypatch, n_fft, mfcc_bands, pcen_bands):
    """The claimed boundary values: the most bands each MFMA route takes at 16000 / n_fft / 160."""
    monkeypatch.delenv("HONK_MFCC_VALU", raising=False)
    for front, most in (("mfcc", mfcc_bands), ("pcen", pcen_bands)):
        routes = [_native.front_plan(16000, n_fft, 160, m, m if front == "mfcc" else None)[1].route
                  for m in range(1, 2 * most)]
        assert routes == [1] * most + [2] * (most - 1), front
    assert fg.BY_ID["mfcc-lds-in"].n_mels == 56 and fg.BY_ID["mfcc-lds-out"].n_mels == 57
    assert fg.BY_ID["pcen-lds-in"].n_mels == 45 and fg.BY_ID["pcen-lds-out"].n_mels == 46


# ---- refusals --------------------------------------------------------------------------------------
BAD = [  # (samples, n_fft, hop, n_mels, n_dct, status)
    (240, 480, 160, 40, 40, ERR_ARG),    # S = n_fft / 2: the reflection needs one sample more
    (0, 480, 160, 40, 40, ERR_ARG),
    (16000, 1, 160, 40, 40, ERR_ARG),
    (16000, 480, 0, 40, 40, ERR_ARG),
    (16000, 480, 160, 0, 40, ERR_ARG),
    (16000, 480, 160, 40, 0, ERR_ARG),   # (the MFCC only)
    (16000, 4096, 160, 40, 40, ERR_UNSUPPORTED),
]


def _mfcc(lib, batch, S, n_fft, hop, n_mels, n_dct, ptrs=(P,) * 5):
    pcm, win, mel, dct, out = ptrs
    return lib.honk_mfcc_f32(pcm, batch, S, win, n_fft, hop, mel, n_mels, dct, n_dct, out, None)


def _pcen(lib, batch, S, n_fft, hop, n_mels, ptrs=(P,) * 4):
    pcm, win, mel, out = ptrs
    return lib.honk_pcen_f32(pcm, batch, S, win, n_fft, hop, mel, n_mels, None, out, None)


@pytest.mark.parametrize("bad", BAD, ids=lambda b: "-".join(map(str, b[:5])))
def test_refusals(lib, bad):
    """The plan queries and the launches refuse the same shapes with the same status and a reason; the
    launches return from their host checks (no pointer read, nothing enqueued)."""
    S, n_fft, hop, n_mels, n_dct, status = bad
    calls = [lambda: _native.front_plan(S, n_fft, hop, n_mels, n_dct)[0],
             lambda: _mfcc(lib, 4, S, n_fft, hop, n_mels, n_dct)]
    if n_dct >= 1:
        calls += [lambda: _native.front_plan(S, n_fft, hop, n_mels)[0], lambda: _pcen(lib, 4, S, n_fft, hop, n_mels)]
    reasons = []
    for call in calls:
        assert call() == status
        reasons.append(_last_error(lib))
        assert reasons[-1]
    assert reasons[0] == reasons[1] and reasons[2:3] == reasons[3:4]  # the query's reason is the launch's


def test_batch_limits_and_null_pointers(lib):
    shape = (16000, 480, 160, 40)
    null4, null5 = (None,) * 4, (None,) * 5
    for rc in (_mfcc(lib, -1, *shape, 40, ptrs=null5), _pcen(lib, -1, *shape, ptrs=null4),  # (checked first)
               _mfcc(lib, 65536, *shape, 40), _pcen(lib, 65536, *shape),
               _mfcc(lib, 4, *shape, 40, ptrs=null5), _pcen(lib, 4, *shape, ptrs=null4),
               lib.honk_mfcc_plan(*shape, 40, None), lib.honk_pcen_plan(*shape, None)):
        assert rc == ERR_ARG and _last_error(lib)
    assert _pcen(lib, 65536, *shape) == ERR_ARG and "65535" in _last_error(lib)
    assert _mfcc(lib, 65535, 240, 480, 160, 40, 40) == ERR_ARG  # the largest batch: on to the shape checks
    assert _mfcc(lib, 0, *shape, 40, ptrs=null5) == 0 and _pcen(lib, 0, *shape, ptrs=null4) == 0
    # (the shape is checked ahead of the empty batch's return)
    assert _mfcc(lib, 0, 240, 480, 160, 40, 40, ptrs=null5) == ERR_ARG and _pcen(lib, 0, 16000, 4096, 160, 40) == ERR_UNSUPPORTED


# ---- the numpy paths -------------------------------------------------------------------------------
def test_frame_count_helper():
    assert AudioPreprocessor().n_frames(16000) == 101
    assert AudioPreprocessor(n_fft=481).n_frames(16000) == 100
    assert AudioPreprocessor(n_fft=481).n_frames(16001) == 101
    assert AudioPreprocessor(n_fft=255, hop_ms=4).n_frames(4000) == 63


@pytest.mark.parametrize("case_id", EXPRESSIBLE)
def test_numpy_paths_meet_the_bound(case_id):
    case = fg.BY_ID[case_id]
    ap, ys = _preprocessor(case), fg.clips(case)
    assert ap.hop_length == case.hop and ap.n_frames(case.S) == case.frames
    got = {"mfcc": np.stack([ap.compute_mfccs(y).squeeze(2) for y in ys]),
           "pcen": ap.compute_pcen(ys).numpy()}
    cpu = {"mfcc": ap.compute_mfccs_batch(torch.from_numpy(ys.copy())).numpy(),
           "pcen": ap.compute_pcen_batch(torch.from_numpy(ys.copy())).numpy()}
    for front in fg.FRONTS:
        ref, b = fg.refs(case_id, front), fg.bound(case_id, front)
        assert got[front].shape == (len(ys), case.frames, case.n_dct if front == "mfcc" else case.n_mels)
        assert got[front].dtype == np.float32 and np.array_equal(got[front], cpu[front])
        errs = fg.errors(got[front], ref)
        print(f"{case_id} numpy {front}: e32 {fg.e32(case_id, front):.2e}  err {max(errs):.2e}  bound {b:.2e}")
        assert max(errs) <= b, (front, errs, b)
        assert not got[front][fg.ZERO].any()


def test_numpy_paths_at_odd_n_fft():
    """compute_pcen allocated 1 + S // hop rows: 101 for the 100 frames of 16000 / 481 / 160."""
    ap = AudioPreprocessor(n_fft=481)
    y = fg.clips(fg.BY_ID["odd481"]).copy()
    assert ap.compute_mfccs(y[0]).shape == (100, 40, 1)
    assert tuple(ap.compute_pcen(y).shape) == (len(y), 100, 40)
    assert tuple(ap.compute_mfccs_batch(torch.from_numpy(y)).shape) == (len(y), 100, 40)
    x = torch.from_numpy((y[0] * 32767).astype(np.int16))
    assert tuple(ap.compute_mfccs_windows(x, 8000, window=8000).shape) == (2, 50, 40)


# ---- the reference side: restatement, bound, separation --------------------------------------------
def test_f32_restatement_shares_no_code_with_the_product():
    src = open(os.path.join(REPO, "oracle", "frontend_f32_sim.py")).read()
    imports = [ln for ln in src.splitlines() if re.match(r"\s*(import|from)\s", ln)]
    assert imports == ["import numpy as np", "from oracle import mfcc_ref"]


@pytest.mark.parametrize("case_id", IDS)
def test_bound_and_separation(case_id):
    """16 * e32 under the cap where the restatement is sound; the staged oracle is the oracle; every named
    mistake moves every non-zero clip by at least ten bounds (a condition on the case's inputs)."""
    case = fg.BY_ID[case_id]
    ys = fg.clips(case)
    assert not ys[fg.ZERO].any() and all(ys[i].any() for i in range(len(ys)) if i != fg.ZERO)
    for front in fg.FRONTS:
        ref, e, b = fg.refs(case_id, front), fg.e32(case_id, front), fg.bound(case_id, front)
        assert 0 < e and b == min(fg.FACTOR * e, fg.CAP) and b <= 1e-4
        assert ref.shape[1] == case.frames and not ref[fg.ZERO].any()
        for i, y in enumerate(ys):
            np.testing.assert_allclose(fg.staged(front, y, case), ref[i], rtol=0,
                                       atol=1e-12 * max(np.abs(ref[i]).max(), 1e-6))
        for mutation in fg.MUTATIONS:
            for i, y in enumerate(ys):
                if i == fg.ZERO:
                    continue
                moved = fg.sim.rel_err(fg.staged(front, y, case, mutation), ref[i])
                assert moved >= SEPARATION * b, (front, mutation, i, moved / b)


def test_empty_bands_are_exact_zeros_in_the_oracle():
    from honk_amd.audio import mel_filterbank
    case = fg.BY_ID["emptybands"]
    mel = mel_filterbank(fg.SR, case.n_fft, case.n_mels, fg.FMIN, fg.FMAX)
    empty = np.flatnonzero(~mel.any(axis=1))
    assert len(empty) == 3
    full = fg.oracle("mfcc", fg.clips(case)[0], case, n_dct=case.n_mels)  # an orthonormal DCT: invert it
    logmel = full @ fg.mfcc_ref.dct_basis(case.n_mels, case.n_mels)
    assert np.abs(logmel[:, empty]).max() < 1e-12 and np.abs(logmel).max() > 1
    assert not fg.refs("emptybands", "pcen")[:, :, empty].any()


# ---- the windows cases -----------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", [c.id for c in fg.WINDOWS])
def test_windows_plan_matches_table(lib, case_id):
    case = fg.WIN_BY_ID[case_id]
    for stride, shared in zip(case.strides, (case.shared, False)):
        assert (stride % case.hop == 0) == (stride == case.strides[0])
        x = fg.recording(case, stride)
        plan = _native.MfccWindowsPlan()
        rc = lib.honk_mfcc_windows_plan(len(x), case.window, stride, case.n_fft, case.hop, 0, case.n_windows,
                                        ctypes.addressof(plan))
        if case.id == "2048-16" and stride % case.hop == 0:
            assert rc == ERR_UNSUPPORTED and "edge frames" in _last_error(lib)
            continue
        assert rc == 0, _last_error(lib)
        assert 3 <= plan.windows == case.n_windows <= 9
        assert (plan.frames, plan.shared) == (case.frames, int(shared))
        # a shape the kernel takes stops at its empty workspace (HONK_ERR_WORKSPACE); one it refuses is given
        # a workspace and stops at the refusal (the band count, or the LDS plan: 171072 B for 2048 / 16)
        rc = lib.honk_mfcc_windows_i16(P, len(x), case.window, stride, 0, case.n_windows, P, case.n_fft, case.hop, P,
                                       case.n_mels, P, case.n_dct, P, P, 0 if case.kernel else plan.workspace_bytes,
                                       None)
        assert rc == (-3 if case.kernel else ERR_UNSUPPORTED) and _last_error(lib)
