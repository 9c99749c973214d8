"""The case table of the training-conv geometry tests (train_geometry_cases.py) against the
library's host-only plan query.

test_gpu_train_geometry.py names the kernel each of its runs is about; this is the guard that
the name is true: honk_conv3x3_plan -- what honk_conv3x3_f32, the statistics-epilogue convs
and honk_conv3x3_wgrad_f32 read at every launch -- gives the table's signature for every
case, at 2 clips and at the many-tile batches, under the default environment and under
HONK_TRAIN_CONV=m|v, HONK_WGRAD=d|h and HONK_TD_FIXED=0; and the older yes/no queries agree
with it on a sweep of shapes.  A case whose kernel changes is a finding, not a row to re-pin:
that geometry would no longer be tested on the kernel the table names."""
import itertools

import pytest

from honk_amd import _native
from honk_amd import model as hm
import train_geometry_cases as geo

N_CUS = geo.N_CUS


@pytest.fixture()
def lib(monkeypatch):
    from honk_amd import build
    build.build()
    for v in geo.ENV_VARS:
        monkeypatch.delenv(v, raising=False)
    return _native.load()


def _batches(case, env):
    if case.family(env) is None or not case.many:
        return (2,)
    return (2,) + tuple(b for nb in set(case.nband(env)) for b in geo.many_tile_batches(nb, N_CUS))


@pytest.mark.parametrize("env", list(geo.ENVS))
@pytest.mark.parametrize("case", geo.CASES, ids=repr)
def test_plan_is_the_tables(lib, case, env):
    with geo.environment(env):
        for B in _batches(case, env):
            sig, grids = geo.signature(B, *case.shape)
            assert sig == case.sigs[env], (B, env)
            if grids is None:
                assert lib.honk_conv3x3_check(*case.shape) != 0
                continue
            # the DMA kernels: one workgroup per CU; the others two (train.hip: tc_grid)
            fam, nb = case.family(env), case.nband(env)
            want = tuple(min(B * n, N_CUS * (1 if f == "d" else 2)) for f, n in zip(fam, nb))
            assert grids == want, (B, env)


def test_table_covers_what_it_claims():
    """Every family with its edge geometries, both ends of both compile-time instances, and a
    many-tile case of d = 1, d = 4 and the fixed instances."""
    c = geo.BY_ID
    assert c["19-25x20-d1"].sigs["default"].startswith("d:25x1F ") and c["19-49x20-d1"].sigs["default"].startswith("d:25x2F ")
    assert "F" not in c["19-26x20-d1"].sigs["default"]
    assert " dq:17x2F" in c["19-34x20-d1"].sigs["default"] and " dq:17x3F" in c["19-50x20-d1"].sigs["default"]
    assert "F" not in c["19-35x20-d1"].sigs["default"]
    assert all("F" not in x.sigs["nofix"] for x in geo.CASES)
    many = [x for x in geo.CASES if x.many]
    assert {x.d for x in many} == {1, 4} and any("F" in x.sigs["default"] for x in many)
    assert all(x.family() == ("d", "d") for x in many)
    fams = {x.family() for x in geo.CASES}
    assert {("d", "d"), ("d", "v"), ("m", "m"), ("m", "v"), ("v", "v"), None} <= fams
    # the VALU conv's pixels per thread: 1 .. 3 at 19 maps (HONK_TRAIN_CONV=v), 1 and 2 at 45
    assert {x.sigs["v"][:2] for x in geo.CASES if x.C == 19 and x.family("v")} >= {"v1", "v2", "v3"}
    assert {x.sigs["default"][:2] for x in geo.CASES if x.C == 45 and x.family()} == {"v1", "v2"}
    # H < d and H == d on the DMA kernels, H < d on the m and the 45-map kernels
    assert any(x.H < x.d and x.family() == ("d", "d") for x in geo.CASES)
    assert any(x.H == x.d and x.family() == ("d", "d") for x in geo.CASES)
    assert any(x.H < x.d and x.family() == ("m", "m") for x in geo.CASES)
    assert any(x.H < x.d and x.C == 45 for x in geo.CASES)
    # one past the widest accepted row goes to the same-conv path
    for C, W in ((19, 285), (45, 119)):
        assert c[f"{C}-2x{W}-d1"].family() == ("v", "v") and c[f"{C}-2x{W + 1}-d1"].family() is None


@pytest.mark.parametrize("step", geo.STEPS, ids=repr)
def test_steps_land_on_the_table(step):
    cfg = dict(hm.find_config(step.model))
    cfg.update(step.override)
    pool = cfg.get("res_pool") or (1, 1)
    assert (step.H // pool[0], step.W // pool[1]) == step.maps
    cases = geo.step_cases(step, cfg)    # KeyError: a block conv off the table
    assert len(cases) == cfg["n_layers"]
    if step.many:
        assert any(x.family() == ("d", "d") for x in cases)


@pytest.mark.parametrize("env", ["default", "m", "v"])
def test_yes_no_queries_agree_with_the_plan(lib, env):
    """honk_conv3x3_check, _stats_bytes, _bn_fold_check and _wgrad_workspace_bytes against the
    plan (at the CU count they see: n_cus = 0) over a few thousand (C, H, W, d, B)."""
    Hs = (1, 2, 3, 4, 7, 17, 25, 26, 49, 101)
    Ws = (1, 3, 4, 5, 8, 12, 20, 40, 119, 120, 252, 256, 257, 260, 285, 286)
    ds = (1, 2, 3, 4, 5, 8, 16)
    n = 0
    with geo.environment(env):
        for C, H, W, d, B in itertools.product((19, 45, 20), Hs, Ws, ds, (2, 300)):
            if C == 20 and (H > 4 or W > 8):
                continue
            p = _native.conv3x3_plan(B, C, H, W, d, 0)
            n += 1
            at = (C, H, W, d, B)
            assert (p is not None) == (lib.honk_conv3x3_check(C, H, W, d) == 0), at
            sb = int(lib.honk_conv3x3_stats_bytes(B, C, H, W, d))
            fold = lib.honk_conv3x3_bn_fold_check(B, C, H, W, d) == 0
            wb = int(lib.honk_conv3x3_wgrad_workspace_bytes(B, C, H, W, d))
            if p is None:
                assert (sb, fold, wb) == (0, False, 0), at
                continue
            assert (sb > 0) == p["stats"] and fold == p["fold"], at
            if p["stats"]:
                assert p["conv"]["family"] == "d" and C == 19, at
                # [C][grid][2] doubles of partial sums + 4 C floats
                assert sb == C * p["conv"]["grid"] * 2 * 8 + 4 * C * 4, at
            if p["fold"]:
                assert p["stats"] and p["wgrad"]["family"] == "d", at
            # one partial dW per workgroup of whichever kernel the environment selects
            assert wb >= p["wgrad"]["grid"] * C * C * 9 * 4 > 0, at
            for k in ("conv", "wgrad"):
                assert 1 <= p[k]["grid"] <= B * p[k]["nband"] and p[k]["th"] >= 1, at
    assert n > 4000


def test_plan_argument_errors(lib):
    with pytest.raises(RuntimeError):
        _native.conv3x3_plan(0, 19, 5, 4, 1, 256)
    with pytest.raises(RuntimeError):
        _native.conv3x3_plan(2, 19, 0, 4, 1, 256)
    with pytest.raises(RuntimeError):
        _native.conv3x3_plan(2, 19, 5, 4, 65, 256)
    assert _native.conv3x3_plan(2, 7, 5, 4, 1, 256) is None   # other widths: the same-conv path
