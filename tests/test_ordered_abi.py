"""honk_res_forward_ordered's argument contract and honk_res_rerun_clips, host-only: every
call here returns before it would touch the GPU (the pointers are never dereferenced)."""
import pytest

from honk_amd import _native

ERR_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -2, -3
P = 0x1000  # a non-null stand-in for a device pointer


def _desc(prec="f16x2", **ov):
    kw = dict(n_labels=12, n_maps=45, n_layers=13, use_dilation=1, pool_h=0, pool_w=0, height=101, width=40)
    kw.update(ov)
    return _native.ResDesc(precision=_native.PRECISIONS[prec], **kw)


@pytest.fixture()
def lib(monkeypatch):
    from honk_amd import build
    build.build()
    for v in ("HONK_F16X2_RERUN", "HONK_RES_CHUNK", "HONK_RES_KERNEL", "HONK_LAST_KERNEL"):
        monkeypatch.delenv(v, raising=False)
    return _native.load()


def test_symbols_exist(lib):
    assert hasattr(lib, "honk_res_forward_ordered") and hasattr(lib, "honk_res_rerun_clips")
    assert "honk_res_forward_ordered" in _native.EXPORTS and "honk_res_rerun_clips" in _native.EXPORTS


@pytest.mark.parametrize("prec", ["f32", "bf16x3", "f16x2"])
def test_null_pointers_and_negative_batch(lib, prec):
    d = _desc(prec)
    ws = lib.honk_res_workspace_bytes(d, 3)
    assert ws > 0
    for null in range(4):
        packed, x, logits, wsp = [0 if i == null else P for i in range(4)]
        assert lib.honk_res_forward_ordered(d, packed, x, logits, 3, wsp, ws, None, 0, None) == ERR_ARG
        assert b"null pointer" in lib.honk_last_error()
    assert lib.honk_res_forward_ordered(d, P, P, P, -1, P, ws, None, 0, None) == ERR_ARG
    assert b"negative batch" in lib.honk_last_error()
    assert lib.honk_res_rerun_count() == 0


@pytest.mark.parametrize("prec", ["f32", "bf16x3", "f16x2"])
def test_workspace_too_small(lib, prec):
    d = _desc(prec)
    ws = lib.honk_res_workspace_bytes(d, 3)
    assert lib.honk_res_forward_ordered(d, P, P, P, 3, P, ws - 1, None, 0, None) == ERR_WORKSPACE
    assert lib.honk_res_forward(d, P, P, P, 3, P, ws - 1, None) == ERR_WORKSPACE
    assert lib.honk_res_rerun_count() == 0


def test_unsupported_shapes_as_the_synchronous_entry(lib):
    """More maps than the kernels take, a bf16x3 map wider than the staging plan: the status
    honk_res_forward gives, and nothing enqueued."""
    for d in (_desc("f32", n_maps=65), _desc("bf16x3", width=67), _desc("f16x2", width=67)):
        want = lib.honk_res_forward(d, P, P, P, 3, P, 1 << 40, None)
        assert want == ERR_UNSUPPORTED
        assert lib.honk_res_forward_ordered(d, P, P, P, 3, P, 1 << 40, None, 0, None) == want
        assert lib.honk_last_error()
    bad = _desc("f32", n_maps=0)
    assert lib.honk_res_forward_ordered(bad, P, P, P, 3, P, 1 << 40, None, 0, None) == \
        lib.honk_res_forward(bad, P, P, P, 3, P, 1 << 40, None) == ERR_ARG
    assert lib.honk_res_rerun_count() == 0


def test_empty_batch_without_a_count_pointer(lib):
    assert lib.honk_res_forward_ordered(_desc(), P, P, P, 0, P, 0, None, 0, None) == 0
    assert lib.honk_res_rerun_count() == 0


def test_rerun_clips_query(lib, monkeypatch):
    """The clips per re-run round, as f16_check_plan sizes them: half the chunk (4096 clips for
    res15), the batch's half below that; 0 where there is no admission."""
    d = _desc()
    assert lib.honk_res_rerun_clips(d, 6) == 3
    assert lib.honk_res_rerun_clips(d, 1) == 1
    assert lib.honk_res_rerun_clips(d, 131072) == 2048
    monkeypatch.setenv("HONK_RES_CHUNK", "4")
    assert lib.honk_res_rerun_clips(d, 6) == 2
    monkeypatch.delenv("HONK_RES_CHUNK")
    assert lib.honk_res_rerun_clips(_desc("bf16x3"), 6) == 0
    assert lib.honk_res_rerun_clips(_desc("f16x2", width=67), 6) == 0
    monkeypatch.setenv("HONK_F16X2_RERUN", "0")
    assert lib.honk_res_rerun_clips(d, 6) == 0
