"""The latency schedule of the res forward on the host (honk_res_latency_plan,
honk_res_latency_workspace_bytes; no GPU call): for a chunk of fewer clips than CUs every block
layer of the 16-bit modes is one launch of the split band kernel whose tiles reach the CU count
where the map has that many; for larger chunks and f32 the plan is honk_res_launch_plan's.

The tile bound of a step, for a chunk of n clips of an H x W (pooled) map with NT out-tiles on
n_cus CUs: tiles >= min(n_cus, n * ceil(H W / 16) * NT) -- the 16-pixel m-tiles x out-tile
groups of the batch -- or tiles == n * H * NT, the most the geometry allows (a band is at
least one class row, and the class rows of a map are its H rows).

The row-band family (block16r_kernel: bf16 on the 19 x 11, 21 x 17, 5 x 5 and 3 x 22 cases) is
split too, with that kernel's arithmetic (the plan reports HONK_KERNEL_SPLIT for both)."""
import ctypes
import re
import os

import pytest

from honk_amd import _native
from golden_util import ref_configs
import res_geometry_cases as geo

N_CUS = 256
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLIT, SYMBOLS = "block16s_kernel", ("honk_res_forward_latency", "honk_res_latency_workspace_bytes",
                                     "honk_res_latency_plan")


@pytest.fixture()
def lib(monkeypatch):
    from honk_amd import build
    build.build()
    for v in geo.ENV_VARS:
        monkeypatch.delenv(v, raising=False)
    return _native.load()


def test_symbols_and_header(lib):
    src = open(os.path.join(REPO, "include", "honk_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _native.EXPORTS
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert re.search(r"#define\s+HONK_KERNEL_SPLIT\s+8\b", src)
    assert _native.KERNEL_NAMES[8] == SPLIT and 6 not in _native.KERNEL_NAMES and 7 not in _native.KERNEL_NAMES


def _res15(prec, H=101, W=40, **over):
    cfg = dict(ref_configs()["res15"])
    cfg.update(over)
    return _native.ResDesc(n_labels=int(cfg["n_labels"]), n_maps=int(cfg["n_feature_maps"]),
                           n_layers=int(cfg["n_layers"]), use_dilation=int(bool(cfg["use_dilation"])), pool_h=0,
                           pool_w=0, height=H, width=W, precision=_native.PRECISIONS[prec])


def _bound(d, n):
    ph, pw = max(d.pool_h, 1), max(d.pool_w, 1)
    H, W, NT = d.height // ph, d.width // pw, (d.n_maps + 15) // 16
    return min(N_CUS, n * -(-H * W // 16) * NT), n * H * NT


@pytest.mark.parametrize("prec", geo.PRECS)
def test_res15_batch_1_is_all_split(lib, prec):
    d = _res15(prec)
    plan = _native.res_latency_plan(d, 1, N_CUS)
    assert [k for k, _ in plan] == [SPLIT] * 13, plan
    need, most = _bound(d, 1)
    for k, tiles in plan:
        assert tiles >= need or tiles == most, plan


@pytest.mark.parametrize("prec", geo.PRECS)
@pytest.mark.parametrize("case", geo.CASES, ids=repr)
def test_tiles_reach_the_cu_count(lib, case, prec):
    d = geo.desc(case, prec)
    for B in (1, 3, N_CUS - 1):
        plan = _native.res_latency_plan(d, B, N_CUS)
        assert len(plan) >= d.n_layers // 2
        need, most = _bound(d, B)
        for i, (k, tiles) in enumerate(plan):
            assert tiles >= need or tiles == most, (B, i, k, tiles, need, most)


@pytest.mark.parametrize("case", geo.CASES, ids=repr)
def test_split_covers_every_16_bit_family(lib, case):
    """Where the throughput plan is pairs / weight-stationary / last-layer / row-band launches, the
    latency plan is one split launch per layer; an fp32 plan is unchanged."""
    for prec in geo.PRECS + ("f32",):
        d = geo.desc(case, prec)
        for B in (1, 3, N_CUS - 1):
            default = _native.res_launch_plan(d, B, N_CUS)
            kinds = [k for k, _ in _native.res_latency_plan(d, B, N_CUS)]
            if prec == "f32":
                assert kinds == default == ["block_kernel"] * d.n_layers, B
            else:
                assert kinds == [SPLIT] * d.n_layers, (prec, B, default, kinds)


@pytest.mark.parametrize("case", geo.CASES, ids=repr)
def test_at_and_past_the_cu_count_is_the_throughput_plan(lib, case):
    for prec in geo.PRECS + ("f32",):
        d = geo.desc(case, prec)
        for B in (N_CUS, 4 * N_CUS):
            assert [k for k, _ in _native.res_latency_plan(d, B, N_CUS)] == _native.res_launch_plan(d, B, N_CUS)
    d = geo.desc(case, "f32")
    for B in (1, 3, N_CUS - 1):
        assert [k for k, _ in _native.res_latency_plan(d, B, N_CUS)] == _native.res_launch_plan(d, B, N_CUS)


def _refusal(fn):
    with pytest.raises(RuntimeError) as e:
        fn()
    return str(e.value).split(": ", 1)[1]


def test_refused_descriptors_are_refused_with_the_same_reason(lib):
    wide = geo.Case("res15", {}, 9, 200, 0, {}, {}, 1.0)
    for d in (_res15("f16x2", n_feature_maps=48), geo.desc(wide, "bf16x3")):
        why = _refusal(lambda: _native.res_launch_plan(d, 1, N_CUS))
        assert _refusal(lambda: _native.res_latency_plan(d, 1, N_CUS)) == why
        assert lib.honk_res_workspace_bytes(ctypes.byref(d), 1) == 0
        why_ws = lib.honk_last_error().decode()
        assert lib.honk_res_latency_workspace_bytes(ctypes.byref(d), 1) == 0
        assert lib.honk_last_error().decode() == why_ws


@pytest.mark.parametrize("case", geo.CASES, ids=repr)
def test_workspace_accepts_every_case(lib, case):
    for prec in geo.PRECS + ("f32",):
        d = geo.desc(case, prec)
        for B in (1, 3, N_CUS - 1, N_CUS, 4 * N_CUS):
            lat, thr = (f(ctypes.byref(d), B) for f in (lib.honk_res_latency_workspace_bytes,
                                                        lib.honk_res_workspace_bytes))
            assert lat != 0 and lat >= thr, (prec, B, lib.honk_last_error())
