"""The SpeechModel (cnn-*) forward at input geometries other than 101 x 40
(cnn_geometry_cases.py): the four hand-scheduled cnn-trad-pool2 kernels at every bound of
their predicates -- heights 72 .. 101, W = 39, odd conv1 outputs, conv2 from 221 to 416
pixels with a ragged last m-tile, pitches of 15 and 18 pixels, an odd tap count, 33 and 12
out channels -- and every variant of the generic GEMM (precision x fused pool x epilogue,
K around the 4096-entry offset table, scalar weight loads, N tails), the unfused max-pool and
the GEMV instances up to the switch to the GEMM.

a. per case, precision and batch (the first B clips; 300 is past a 256-CU persistent grid):
   the launch plan names the kernels the case is about, and the logits are within 1e-4 of
   the float64 oracle;
b. bitwise batch invariance of the fast-path cases: 300 clips = the same clips as 1 + 2 + 256
   + 41, and 5 clips in chunks of 2 = unchunked;
c. each fast path switched off agrees with the default plan at the same geometry, both held
   to the oracle;
d. through the C ABI with a workspace of exactly honk_cnn_workspace_bytes: sentinel tails of
   the workspace and of the logits come back untouched, every logit is written."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from honk_amd import _native
from honk_amd import model as hm
import cnn_geometry_cases as geo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = geo.CASES
FAST_CASES = [pytest.param(c, p, id=f"{c}-{p}") for c in CASES for p in geo.PRECS if c.fast(p)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _native.load()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for v in geo.ENV_VARS:
        monkeypatch.delenv(v, raising=False)


_MODULES = {}


def _module(case, prec):
    key = (case.id, prec)
    if key not in _MODULES:
        cfg, params, _ = geo.build(case)
        m = hm.find_model(case.model)(cfg)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
        m = m.eval().to(DEV)
        m.honk_precision = prec
        _MODULES[key] = m
    return _MODULES[key]


def _desc(m, prec):
    return _native.CnnDesc(**m._honk_desc, precision=_native.PRECISIONS[prec])


@contextlib.contextmanager
def _device_errors_end_the_run(what):
    try:
        yield
    except RuntimeError as e:
        if "hip" in str(e).lower() or "illegal" in str(e).lower():
            # an untested geometry that faulted the device: nothing more runs on it
            pytest.exit(f"GPU error in {what}: {e}", returncode=3)
        raise


def _run(m, x):
    with _device_errors_end_the_run(f"{m.honk_precision} on {tuple(x.shape)}"):
        with torch.no_grad():
            out = m(torch.tensor(x).to(DEV))   # (a copy: the shared clips are read-only)
        torch.cuda.synchronize()
        return out.cpu().numpy()


def _clips(case, B):
    return geo.build(case)[2][:B]


@pytest.mark.parametrize("B", geo.BATCHES)
@pytest.mark.parametrize("prec", geo.PRECS)
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_kernels_vs_oracle(case, prec, B):
    """(a)"""
    m = _module(case, prec)
    assert _native.cnn_launch_plan(_desc(m, prec)) == case.plan(prec)
    out = _run(m, _clips(case, B))
    assert out.shape == (B, geo.config(case)["n_labels"]) and np.isfinite(out).all()
    ref = geo.oracle(case, B)
    err = float(np.abs(out[geo.compared(B)] - ref).max())
    print(f"{case} {prec} B={B}: max|logit - oracle| {err:.2e} (max|logit| {np.abs(ref).max():.2f}, "
          f"float32 oracle {case.f32_err:.1e}; {'+'.join(case.fast(prec)) or 'generic'})")
    assert err <= geo.ATOL


@pytest.mark.parametrize("case,prec", FAST_CASES)
def test_batch_invariance(monkeypatch, case, prec):
    """(b) a clip's logits do not depend on the batch around it, nor on the chunking."""
    m = _module(case, prec)
    x = _clips(case, geo.BMAX)
    whole = _run(m, x)
    pieces = np.concatenate([_run(m, x[a:b]) for a, b in ((0, 1), (1, 3), (3, 259), (259, 300))])
    assert np.array_equal(whole, pieces), float(np.abs(whole - pieces).max())
    monkeypatch.setenv("HONK_CNN_CHUNK", "2")   # 2 + 2 + a ragged last chunk of 1
    assert np.array_equal(_run(m, x[:5]), whole[:5])


@pytest.mark.parametrize("case,prec", FAST_CASES)
def test_fast_vs_generic(monkeypatch, case, prec):
    """(c) each of the case's fast kernels switched off (its plan then has one fast kernel
    fewer) against the default plan, on all 300 clips; both against the oracle."""
    m = _module(case, prec)
    x = _clips(case, geo.BMAX)
    idx, ref = geo.compared(geo.BMAX), geo.oracle(case, geo.BMAX)
    fast = _run(m, x)
    assert float(np.abs(fast[idx] - ref).max()) <= geo.ATOL
    for k in case.fast(prec):
        monkeypatch.setenv(geo.SWITCH_OF[k], "0")
        plan = _native.cnn_launch_plan(_desc(m, prec))
        assert k not in plan and plan != case.plan(prec)
        out = _run(m, x)
        monkeypatch.delenv(geo.SWITCH_OF[k])
        d, e = float(np.abs(out - fast).max()), float(np.abs(out[idx] - ref).max())
        print(f"{case} {prec} {geo.SWITCH_OF[k]}=0: vs default {d:.2e}, vs oracle {e:.2e}")
        assert d <= geo.ATOL and e <= geo.ATOL, (k, d, e)
    for k, v in geo.ALL_OFF.items():
        monkeypatch.setenv(k, v)
    assert _native.cnn_launch_plan(_desc(m, prec)) == case.plan(prec, off=True)
    out = _run(m, x)
    d, e = float(np.abs(out - fast).max()), float(np.abs(out[idx] - ref).max())
    print(f"{case} {prec} all off: vs default {d:.2e}, vs oracle {e:.2e}")
    assert d <= geo.ATOL and e <= geo.ATOL, (d, e)


TAIL = 4096


@pytest.mark.parametrize("prec", geo.PRECS)
@pytest.mark.parametrize("cid", ["trad-100x40", "trad-61x40-c1k10x4", "k4160"])
def test_honest_sizes(cid, prec):
    """(d) honk_cnn_forward keeps to the workspace honk_cnn_workspace_bytes asks for and to
    B * n_labels logits."""
    case, B = geo.BY_ID[cid], 3
    m = _module(case, prec)
    lib = _native.load()
    d = _desc(m, prec)
    n_labels = geo.config(case)["n_labels"]
    need = lib.honk_cnn_workspace_bytes(ctypes.byref(d), B)
    assert need > 0
    ws = torch.full((need + TAIL,), 0xA5, dtype=torch.uint8, device=DEV)
    logits = torch.full((B * n_labels + TAIL // 4,), float("nan"), device=DEV)
    logits[B * n_labels:] = 12345.0
    x = torch.tensor(_clips(case, B)).to(DEV)
    ts = [t.detach().contiguous() if t is not None else None for t in m._native_tensors()]
    with _device_errors_end_the_run(f"{cid} {prec} through the C ABI"), torch.cuda.device(DEV):
        _native.check(lib.honk_cnn_forward(ctypes.byref(d), _native.ptr_array(ts), x.data_ptr(), logits.data_ptr(), B,
                                           ws.data_ptr(), need, _native.stream_handle(torch.device(DEV))),
                      "honk_cnn_forward")
        torch.cuda.synchronize()
    assert bool((ws[need:] == 0xA5).all()), "workspace tail written"
    assert bool((logits[B * n_labels:] == 12345.0).all()), "logits tail written"
    out = logits[:B * n_labels].cpu().numpy().reshape(B, n_labels)
    assert not np.isnan(out).any(), "a logit was not written"
    assert float(np.abs(out - geo.oracle(case, B)).max()) <= geo.ATOL
    # one byte short is refused, not overrun
    rc = lib.honk_cnn_forward(ctypes.byref(d), _native.ptr_array(ts), x.data_ptr(), logits.data_ptr(), B,
                              ws.data_ptr(), need - 1, _native.stream_handle(torch.device(DEV)))
    assert rc != 0 and b"workspace" in lib.honk_last_error()
