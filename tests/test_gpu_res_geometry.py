"""The res block kernels at input geometries other than 101 x 40 (res_geometry_cases.py):
one-row and few-row maps (streams shorter than a 64-pixel step, heights below the dilation,
dilation classes with no rows), heights that are multiples of every dilation, widths at both
ends of each DMA pieces-per-row class of the pair kernel, widths below the dilation, pooled
maps off 25 x 13 / 50 x 20, and the two `auto` -> f16x2 contract sizes off 101 x 40.

For every case, precision and batch (a batch is the first B clips):
a. the launch plan on the device is the table's (so each run below is of the kernel it names);
b. the default plan, forced-p, w and r against the float64 oracle, at the bar of
   res_geometry_cases.bar (f16x2 with the per-clip admission off: it would replace a wrong
   f16x2 clip with its bf16x3 re-run; once per case with it on);
c. the cross-kernel identities: the pairs bit for bit the weight-stationary layers, the
   last-layer kernel within fp32 summation rounding of them, bf16's DMA / stream variants
   bit for bit the default;
d. bitwise batch invariance of the default plan;
e. the fp32 kernel (plan_block at new H and W);
f. the `auto` policy at the contract sizes.
The bf16 oracle bar is loose by nature; the bitwise checks are its sharp ones, and bf16x3's
1e-4 is the tight oracle check of the geometry code the three formats share."""
import warnings

import numpy as np
import pytest
import torch

from honk_amd import _native
from honk_amd import model as hm
import res_geometry_cases as geo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = geo.CASES
CASE_BATCH = [pytest.param(c, B, id=f"{c}-B{B}") for c in CASES for B in c.batches]


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


def _module(case, prec, reroute=False):
    key = (case.id, prec, reroute)
    if key not in _MODULES:
        cfg, params, _ = geo.build(case)
        m = hm.find_model(case.model)(cfg)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
        m = m.eval().to(DEV)
        m.honk_precision = prec
        m.honk_reroute = reroute   # False: the kernels of `prec` themselves, whatever the policy
        _MODULES[key] = m
    return _MODULES[key]


def _run(m, x):
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)   # no silent fallback to the fp32 layer path
            with torch.no_grad():
                out = m(torch.tensor(x).to(DEV))   # (a copy: the shared clips are read-only)
        torch.cuda.synchronize()
        out = out.cpu().numpy()
    except RuntimeError as e:
        if "hip" in str(e).lower() or "illegal" in str(e).lower():
            # an untested geometry that faulted the device: nothing more runs on it
            pytest.exit(f"GPU error in {m.honk_precision} on {tuple(x.shape)}: {e}", returncode=3)
        raise
    assert np.isfinite(out).all()
    return out


def _setenv(monkeypatch, env):
    for v in geo.ENV_VARS:
        monkeypatch.delenv(v, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _plan(m, case, B):
    return _native.res_launch_plan(m._desc(case.H, case.W), B)


def _clips(case, B):
    return geo.build(case)[2][:B]


def _raw(prec, env=None):
    """The environment of a kernel run: f16x2 without the admission's bf16x3 re-run."""
    e = dict(env or {})
    if prec == "f16x2":
        e["HONK_F16X2_RERUN"] = "0"
    return e


@pytest.mark.parametrize("prec", geo.PRECS)
@pytest.mark.parametrize("case,B", CASE_BATCH)
def test_plan_on_device(monkeypatch, case, B, prec):
    """(a) with the device's own CU count (n_cus = 0), as the forward plans."""
    m = _module(case, prec)
    assert _plan(m, case, B) == case.plan(prec)
    _setenv(monkeypatch, geo.FORCED_P)
    assert _plan(m, case, B) == case.plan(prec, forced=True)


@pytest.mark.parametrize("prec", geo.PRECS)
@pytest.mark.parametrize("case,B", CASE_BATCH)
def test_kernels_vs_oracle(monkeypatch, case, B, prec):
    """(b) and (c): every dispatch of the mode against the float64 oracle, and against each
    other where the contracts are exact."""
    m = _module(case, prec)
    x = _clips(case, B)
    idx = geo.compared(B)
    ref = geo.oracle(case, B)
    bar = geo.bar(case, prec)
    L = geo.config(case)["n_layers"]
    runs = {"default": {}, "forced-p": geo.FORCED_P, "w": dict(HONK_RES_KERNEL="w")}
    if prec != "f16x2":
        runs["r"] = dict(HONK_RES_KERNEL="r")
    want = {"default": case.plan(prec), "forced-p": case.plan(prec, forced=True), "w": ["block16w_kernel"] * L,
            "r": ["block16r_kernel"] * L}
    outs, errs = {}, {}
    for name, env in runs.items():
        _setenv(monkeypatch, _raw(prec, env))
        assert _plan(m, case, B) == want[name], name
        outs[name] = _run(m, x)
        errs[name] = float(np.abs(outs[name][idx] - ref).max())
    print(f"{case} {prec} B={B}: max|logit - oracle| " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) +
          f" (bar {bar:.2e}, max|logit| {np.abs(ref).max():.2f})")
    for name, e in errs.items():
        assert e <= bar, (name, e, bar)
    # the pairs compute what two weight-stationary launches compute: same products, same
    # order, same roundings (where the last layer is the weight-stationary kernel's in both: a
    # bf16 even stack's last pair stores its output for tail_act_kernel, other sums)
    fp = want["forced-p"]
    if "block16p_kernel" in fp and fp[-1] == "block16w_kernel":
        assert np.array_equal(outs["forced-p"], outs["w"]), float(np.abs(outs["forced-p"] - outs["w"]).max())
    # the last-layer kernel adds the channel sums in another (fixed) order
    if want["default"][-1] == "block16l_kernel":
        _setenv(monkeypatch, _raw(prec, dict(HONK_LAST_KERNEL="w")))
        assert _plan(m, case, B) == want["default"][:-1] + ["block16w_kernel"]
        outw = _run(m, x)
        assert np.abs(outs["default"] - outw).max() <= 2e-5 * max(1.0, float(np.abs(outw).max()))
    # bf16's pair variants move the same bytes: one stream per workgroup, the row-table walk
    # for the tap-step instances, row pieces for the linear DMA
    if prec == "bf16" and "block16p_kernel" in want["default"]:
        for var, val in (("HONK_PAIR_STREAMS", "1"), ("HONK_PAIR_IMM2", "0"), ("HONK_PAIR_LIN", "0")):
            _setenv(monkeypatch, {var: val})
            if "block16p_kernel" not in _plan(m, case, B):   # (one stream may not plan: nothing to compare)
                continue
            out = _run(m, x)
            assert np.array_equal(out, outs["default"]), (var, float(np.abs(out - outs["default"]).max()))


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_f16x2_with_the_admission(case):
    """(b) f16x2 as it ships: the per-clip admission on, at the same bar."""
    B = max(case.batches)
    m = _module(case, "f16x2")
    out = _run(m, _clips(case, B))
    err = float(np.abs(out[geo.compared(B)] - geo.oracle(case, B)).max())
    print(f"{case} f16x2 B={B} with the admission: max|logit - oracle| {err:.2e} (bar {geo.bar(case, 'f16x2'):.2e}), "
          f"honk_last_rerun = {m.honk_last_rerun}")
    assert err <= geo.bar(case, "f16x2")


@pytest.mark.parametrize("prec", geo.PRECS)
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_batch_invariance(monkeypatch, case, prec):
    """(d) a clip's logits do not depend on the batch around it: clip 1 alone, clips 0..2, and
    the same clips last in a 600-clip batch (several clips per workgroup stream), bit for bit."""
    _setenv(monkeypatch, _raw(prec))
    m = _module(case, prec)
    x = _clips(case, max(case.batches))
    three = _run(m, x[:3])
    assert np.array_equal(_run(m, x[1:2])[0], three[1])
    if not case.contract:
        big = _run(m, np.concatenate([x[3:], x[:3]]))
        assert len(big) == geo.BMAX
        assert np.array_equal(big[-3:], three), float(np.abs(big[-3:] - three).max())


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_f32(case):
    """(e) block_kernel under plan_block's tiling of the case's map."""
    B = max(case.batches)
    m = _module(case, "f32")
    assert _plan(m, case, B) == ["block_kernel"] * geo.config(case)["n_layers"]
    out = _run(m, _clips(case, B))
    err = float(np.abs(out[geo.compared(B)] - geo.oracle(case, B)).max())
    print(f"{case} f32 B={B}: max|logit - oracle| {err:.2e}")
    assert err <= geo.bar(case, "f32")


@pytest.mark.parametrize("cid,want", [("res15-112x40", "f16x2"), ("res15-101x41", "f16x2"), ("res15-33x37", "bf16x3")])
def test_auto_policy(cid, want):
    """(f) include/honk_hip.h: auto runs f16x2 where its 1e-4 contract holds -- unpooled maps
    of >= 4040 pixels (112 x 40 = 4480, 101 x 41 = 4141) -- else bf16x3 (33 x 37 = 1221)."""
    case = geo.BY_ID[cid]
    m = _module(case, "auto", reroute=True)
    out = _run(m, _clips(case, 3))
    assert m.honk_last_precision == want
    err = float(np.abs(out - geo.oracle(case, 3)).max())
    print(f"{case} auto -> {m.honk_last_precision}: max|logit - oracle| {err:.2e}")
    assert err <= 1e-4
