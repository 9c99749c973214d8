"""The case table of the input-geometry tests (res_geometry_cases.py) against the library's
host-only planner, and against the rounding simulation its bars derive from.

test_gpu_res_geometry.py names the kernel each of its runs is about; this is the guard that
the name is true: honk_res_launch_plan (a function of H, W, the dilations and the batch) gives
the table's plan for every case, precision and batch, under the default environment and under
forced-p.  A pair or last-layer entry that disappears from a plan here is a finding, not a
row to re-pin: that geometry would no longer be tested on the kernel the table names."""
import ctypes

import numpy as np
import pytest

from honk_amd import _native
import res_geometry_cases as geo

N_CUS = 256


@pytest.fixture()
def lib(monkeypatch):
    from honk_amd import build
    build.build()
    for v in geo.ENV_VARS:
        monkeypatch.delenv(v, raising=False)
    return _native.load()


@pytest.mark.parametrize("prec", geo.PRECS)
@pytest.mark.parametrize("case", geo.CASES, ids=repr)
def test_launch_plan_is_the_tables(lib, monkeypatch, case, prec):
    d = geo.desc(case, prec)
    for B in (3, geo.BMAX):
        assert _native.res_launch_plan(d, B, N_CUS) == case.plan(prec), (B, "default")
    for k, v in geo.FORCED_P.items():
        monkeypatch.setenv(k, v)
    for B in (3, geo.BMAX):
        assert _native.res_launch_plan(d, B, N_CUS) == case.plan(prec, forced=True), (B, "forced-p")
    # the single-kernel plans the GPU file compares them with
    L = geo.config(case)["n_layers"]
    monkeypatch.setenv("HONK_RES_KERNEL", "w")
    assert _native.res_launch_plan(d, geo.BMAX, N_CUS) == ["block16w_kernel"] * L
    if prec != "f16x2":
        monkeypatch.setenv("HONK_RES_KERNEL", "r")
        assert _native.res_launch_plan(d, geo.BMAX, N_CUS) == ["block16r_kernel"] * L


def test_table_covers_what_it_claims():
    """Every kernel family at an off-101x40 geometry in every mode it has: pairs at each
    pieces-per-row class, the last-layer kernel at heights other than 101, a mixed plan."""
    by = {p: [c for c in geo.CASES if "P" in c.plans[p][0]] for p in geo.PRECS}
    for p in geo.PRECS:
        widths = {c.W // (geo.config(c).get("res_pool") or (1, 1))[1] for c in by[p]}
        assert {40, 41, 37} <= widths and widths & {11, 13} and widths & {17, 20, 22}, (p, widths)
        assert {c.H for c in geo.CASES if c.plans[p][0].endswith("L")} >= {1, 7, 16, 112}
    assert geo.BY_ID["res15-33x37"].plans["bf16x3"][0] == "PWWPPWWPW"
    assert len(geo.BY_ID) == len(geo.CASES)


def test_no_pair_below_its_dilation():
    """The pair kernel's walk takes every dilation class of its A layer to hold a row: a map
    of fewer rows than that dilation stays on the single-layer kernels (1 x 40 and 7 x 40
    lose the pairs at dilations >= 2 and 8; a B layer's dilation past the height is fine)."""
    seen = set()
    for case in geo.CASES:
        cfg = geo.config(case)
        H = case.H // (cfg.get("res_pool") or (1, 1))[0]
        for prec in geo.PRECS:
            for plan in case.plans[prec]:
                layer = 1
                for k in plan:
                    if k == "P":
                        dA, dB = (2 ** ((i - 1) // 3) if cfg["use_dilation"] else 1 for i in (layer, layer + 1))
                        assert H >= dA, (case, prec, plan, layer)
                        seen.add((H >= dB, dA > 1))
                    layer += 2 if k == "P" else 1
                assert layer == cfg["n_layers"] + 1
    assert (False, True) in seen   # 7 x 40: the (4, 8) pair


@pytest.mark.parametrize("case", geo.CASES, ids=repr)
def test_workspace_accepts_every_case(lib, case):
    for prec in geo.PRECS + ("f32",):
        d = geo.desc(case, prec)
        for B in case.batches:
            assert lib.honk_res_workspace_bytes(ctypes.byref(d), B) != 0, (prec, B, lib.honk_last_error())
        assert _native.res_launch_plan(geo.desc(case, "f32"), 3, N_CUS) == ["block_kernel"] * d.n_layers


def test_f16x2_refuses_64_pixel_rows(lib):
    """The weight-stationary / pair kernels' m-tile walk carries at most one row per 64-pixel
    step: rows of 64 pixels and more are outside f16x2 (its only kernels), with the
    documented message; bf16x3 and bf16 fall to the row-band kernel there."""
    wide = geo.Case("res15", {}, 9, 64, 0, {}, {}, 1.0)
    d = geo.desc(wide, "f16x2")
    assert lib.honk_res_workspace_bytes(ctypes.byref(d), 3) == 0
    msg = lib.honk_last_error().decode()
    assert msg.startswith("f16x2 runs on the weight-stationary / pair kernels only") and "9x64" in msg, msg
    with pytest.raises(RuntimeError, match="f16x2: outside the weight-stationary / pair kernels' envelope"):
        _native.res_launch_plan(d, 3, N_CUS)
    for prec in ("bf16x3", "bf16"):
        d = geo.desc(wide, prec)
        assert lib.honk_res_workspace_bytes(ctypes.byref(d), 3) != 0
        assert _native.res_launch_plan(d, 3, N_CUS) == ["block16r_kernel"] * 13
    narrow = geo.Case("res15", {}, 9, 63, 0, {}, {}, 1.0)
    assert lib.honk_res_workspace_bytes(ctypes.byref(geo.desc(narrow, "f16x2")), 3) != 0


def _simulated(case):
    ref = geo.reference(case)
    got = {p: geo.simulate(case, p) for p in geo.PRECS}
    got["max_logit"] = max(float(np.abs(v).max()) for v in ref.values())
    return got


def _check_recorded(case):
    got = _simulated(case)
    print(case, {k: f"{v:.3g}" for k, v in got.items()})
    for p in geo.PRECS:
        assert abs(case.sim[p] - got[p]) <= 0.1 * got[p], (p, case.sim[p], got[p])
    assert abs(case.max_logit - got["max_logit"]) <= 0.1 * got["max_logit"]
    # the oracle's own headroom under the 1e-4 bar of bf16x3 / f32 / contract-size f16x2:
    # the number formats alone stay 5x below it, on logits of O(1)
    assert got["bf16x3"] <= 2.0e-5 and got["max_logit"] <= 2.2
    # a bar is never below the mode's floor, nor below 3x what its formats explain
    assert geo.bar(case, "bf16x3") == geo.bar(case, "f32") == 1e-4
    assert geo.bar(case, "bf16") >= max(geo.BF16_BOUND, 2.7 * got["bf16"])
    if not case.contract:
        assert geo.bar(case, "f16x2") >= max(1e-4, 2.7 * got["f16x2"])


@pytest.mark.parametrize("case", [c for c in geo.CASES if not c.contract], ids=repr)
def test_recorded_simulated_errors(case):
    """The table's simulated errors are what oracle/res_round_sim.py gives for the case's own
    clips (+-10 %: they are recorded to three digits), so no bar can be loosened by hand."""
    _check_recorded(case)


@pytest.mark.slow
@pytest.mark.parametrize("case", [c for c in geo.CASES if c.contract], ids=repr)
def test_recorded_simulated_errors_contract_sizes(case):
    _check_recorded(case)


@pytest.mark.slow
def test_bf16_scheme_matches_the_measured_mode():
    """The one-bf16-per-operand scheme on the shape everything else is measured at: res15 on
    101 x 40 simulates to what DESIGN.md measures for the bf16 kernels there (<= 3.4e-3;
    within a factor of two either way: the simulation has the operand roundings only, the
    measurement other weights and clips), so the scheme is a credible source of the bf16
    bars at the other geometries."""
    case = geo.Case("res15", {}, 101, 40, 71, {}, {}, 1.0, contract=True)
    e = geo.simulate(case, "bf16")
    print(f"res15 101x40 bf16 simulated {e:.2e}")
    assert 3.4e-3 / 2 <= e <= 3.4e-3 * 2
