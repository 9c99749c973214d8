"""The training ABI's host side (honk_amd/csrc/train.hip behind honk_sgd_step_f32 ..
honk_res_stem_wgrad_f32) against its pinned refusals and byte counts
(train_abi_refusal_cases.py).

The refusals run only where the process sees no GPU: every pointer of a refused call is null
or a host buffer, and should a later change lose a check, a device would be handed host
pointers.  The byte-count queries run everywhere, as relations that hold at any CU count."""
import ctypes

import pytest
import torch

from honk_amd import _native
import train_abi_refusal_cases as abi
import train_geometry_cases as geo


@pytest.fixture()
def lib(monkeypatch):
    from honk_amd import build
    build.build()
    for v in geo.ENV_VARS:
        monkeypatch.delenv(v, raising=False)
    return _native.load()


_HOST = (ctypes.c_double * 8192)()   # 64 KiB: every size a row passes fits, were it ever read


def _call(lib, fn, change):
    base = abi.BASE[fn]
    assert set(change) <= set(base), (fn, change)
    args = [ctypes.addressof(_HOST) if v is abi.P else v for v in dict(base, **change).values()]
    rc = getattr(lib, fn)(*args)
    return rc, lib.honk_last_error().decode()


def test_table_covers_every_training_entry_point():
    named = {r[0] for r in abi.REFUSALS}
    assert named == set(abi.BASE)
    ids = [abi.row_id(r) for r in abi.REFUSALS]
    assert len(set(ids)) == len(ids)
    queries = {"honk_conv3x3_check", "honk_conv3x3_plan", "honk_conv3x3_wgrad_workspace_bytes",
               "honk_bn_train_workspace_bytes", "honk_conv3x3_stats_bytes", "honk_conv3x3_bn_fold_check",
               "honk_res_stem_wgrad_workspace_bytes"}
    training = {n for n in _native.EXPORTS if n.startswith(("honk_conv3x3_", "honk_bn_", "honk_res_tail_",
                                                              "honk_res_stem_", "honk_sgd_"))}
    assert training - queries == named
    for fn, base in abi.BASE.items():
        assert len(base) == len(_native._PROTOS[fn][1]), fn


@pytest.mark.parametrize("row", abi.REFUSALS, ids=abi.row_id)
def test_refusal_is_the_pinned_one(lib, row):
    if torch.cuda.is_available():
        pytest.skip("the refusal table runs only in a process that sees no GPU (its pointers are host buffers)")
    fn, change, code, text = row
    assert code in (abi.ARG, abi.UNSUPPORTED, abi.WORKSPACE)
    assert _call(lib, fn, change) == (code, text)


def test_count_scale_refusal_keeps_the_scale(lib):
    """(host-only at any device count: honk_bn_count_scale launches nothing)"""
    assert lib.honk_bn_count_scale(2.0) == 0
    assert lib.honk_bn_count_scale(0.5) == abi.ARG
    assert lib.honk_last_error().decode() == "BatchNorm count scale 0.5 outside [1, 65536]"
    assert lib.honk_bn_count_scale(1.0) == 0


# two batches past the grid cap of every family (two workgroups per CU at the most) on any
# device of up to 512 CUs, every case having at least one band per clip
BATCHES = (2, 1100, 2300)


@pytest.mark.parametrize("case", geo.CASES, ids=repr)
def test_statistics_bytes_and_fold_check_follow_the_plan(lib, case):
    C = case.C
    for B in BATCHES:
        p = _native.conv3x3_plan(B, *case.shape, n_cus=0)
        sb = int(lib.honk_conv3x3_stats_bytes(B, *case.shape))
        fold = lib.honk_conv3x3_bn_fold_check(B, *case.shape)
        if p is None or not p["stats"]:
            assert sb == 0, B
        else:
            assert sb == C * p["conv"]["grid"] * 16 + 16 * C, B
        assert (fold == 0) == bool(p and p["fold"]), B
        if fold:
            assert fold == abi.UNSUPPORTED
            assert lib.honk_last_error().decode() == "conv3x3: no folded BatchNorm for this shape"
    assert (case.family() is None) == (p is None)
    if p is not None:
        assert (p["stats"], p["fold"]) == ("s" in case.flags(), "f" in case.flags())


@pytest.mark.parametrize("case", geo.CASES, ids=repr)
def test_wgrad_workspace_is_the_largest_family_grid(lib, case):
    """B = 2: every tile count is far below any device's CU count, so the grid is the tile
    count -- of the family with the most bands, whichever kernel the environment selects."""
    bands = abi.WGRAD_BANDS[case.id]
    for env in ("default", "m", "v"):
        with geo.environment(env):
            assert int(lib.honk_conv3x3_wgrad_workspace_bytes(2, *case.shape)) == 2 * bands * case.C * case.C * 9 * 4
        if bands:
            assert case.nband(env)[1] <= bands
    if bands:   # ... and it is some family's
        assert bands == max(case.nband(env)[1] for env in ("default", "m", "v"))
    else:
        assert case.family() is None
    for bad in ((0, *case.shape), (2, 32, *case.shape[1:]), (2, case.C, 0, case.W, case.d),
                (2, case.C, case.H, case.W, 65)):
        assert int(lib.honk_conv3x3_wgrad_workspace_bytes(*bad)) == 0


def test_bn_workspace_bytes(lib):
    assert len(abi.BN_WORKSPACE) >= 6
    for (B, C, HW), n in abi.BN_WORKSPACE.items():
        assert int(lib.honk_bn_train_workspace_bytes(B, C, HW)) == n, (B, C, HW)
    for bad in ((0, 19, 84), (2, 0, 84), (2, 19, 0), (-1, 19, 84)):
        assert int(lib.honk_bn_train_workspace_bytes(*bad)) == 0
