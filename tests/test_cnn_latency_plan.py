"""The latency schedule of the cnn forward, host-only: honk_cnn_latency_plan /
honk_cnn_latency_workspace_bytes / honk_cnn_latency_threshold over the geometries of
cnn_geometry_cases x both precisions x batches 1, 3, 17 x devices of 8 and 256 CUs.

What "tiles the chunk yields" means per split kernel (the bound a launch's workgroup count is
held to): conv2, split -- one tile per (clip, 16-pixel m-tile, non-empty 16-channel out tile);
conv1, split -- one per (clip, band of 4 pooled m-tiles, n-group of 2 out tiles), a band being at
least one m-tile per wave; split-K Linear -- one per (K slice, group of 4 rows, group of 8
outputs)."""
import ctypes

import pytest

from honk_amd import _native
import cnn_geometry_cases as cgeo

BATCHES = (1, 3, 17)
CUS = (8, 256)
SPLIT_OF = _native.CNN_SPLIT_OF
SPLIT_KINDS = tuple(SPLIT_OF.values())
SK, SKS = "linear_splitk_kernel", "linear_splitk_sum_kernel"
NEW = SPLIT_KINDS + (SK, SKS)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for v in cgeo.ENV_VARS + ("HONK_CNN_SPLITK_SLICE",):
        monkeypatch.delenv(v, raising=False)


def _cdiv(a, b):
    return -(-a // b)


def _linears(case):
    """[(K, n)] of the case's Linear layers in order."""
    cfg = cgeo.config(case)
    oh1, ow1, ph1, pw1, oh2, ow2 = cgeo.geometry(case)
    d = cgeo.desc(case, "f32")
    if d.has_conv2:
        width = d.c2_out * (oh2 // d.p2_h) * (ow2 // d.p2_w)
    else:
        width = d.c1_out * ph1 * pw1
    out = []
    for n in ([32] if d.has_lin else []) + [v for v in (d.dnn1, d.dnn2) if v] + [int(cfg["n_labels"])]:
        out.append((width, n))
        width = n
    return out


def _yield(case, kind, B):
    """Tiles a chunk of B clips yields for a split conv (see the module docstring)."""
    oh1, ow1, ph1, pw1, oh2, ow2 = cgeo.geometry(case)
    d = cgeo.desc(case, "f32")
    if kind in ("conv2xs_kernel", "conv2fs_kernel"):
        return B * _cdiv(oh2 * ow2, 16) * _cdiv(d.c2_out, 16)
    return B * _cdiv(ph1 * pw1 // 4, 4) * 2


def test_abi_surface():
    lib = _native.load()
    for name in ("honk_cnn_forward_latency", "honk_cnn_latency_workspace_bytes", "honk_cnn_latency_plan",
                 "honk_cnn_latency_threshold", "honk_cnn_features_f32", "honk_linear_splitk_f32",
                 "honk_linear_splitk_slices", "honk_linear_splitk_workspace_bytes"):
        assert hasattr(lib, name) and name in _native.EXPORTS
    assert [_native.cnn_kernel_name(k) for k in (13, 14, 15, 32, 33, 34)] == [
        "conv1xs_kernel", "conv1fs_kernel", "conv2xs_kernel", "conv2fs_kernel", SK, SKS]
    # fewer clips than CUs, and no more than the measured cap of the precision
    for prec in cgeo.PRECS:
        d = cgeo.desc(cgeo.BY_ID["trad-72x40"], prec)
        assert _native.cnn_latency_threshold(d, 8) == 8
        assert max(BATCHES) < _native.cnn_latency_threshold(d, 256) <= 256
        assert _native.cnn_latency_threshold(d, 1 << 20) == _native.cnn_latency_threshold(d, 256)
    d.precision = 1
    assert lib.honk_cnn_latency_threshold(ctypes.byref(d), 256) == lib.honk_cnn_launch_plan(ctypes.byref(d), None, 0) < 0


def test_python_surface():
    from honk_amd import model as hm
    m = hm.find_model("cnn-trad-pool2")(dict(hm.find_config("cnn-trad-pool2")))
    assert m.honk_schedule == "throughput" and callable(m.honk_capture)
    with pytest.raises(RuntimeError):
        m.honk_capture(None)  # (training mode, and no tensor)


@pytest.mark.parametrize("prec", cgeo.PRECS)
@pytest.mark.parametrize("case", cgeo.CASES, ids=repr)
def test_latency_plan(case, prec):
    lib = _native.load()
    d = cgeo.desc(case, prec)
    thr_plan = _native.cnn_launch_plan(d)
    assert thr_plan == case.plan(prec)
    linears = _linears(case)
    n_lin = len(linears)
    slices = {}
    for cus in CUS:
        thr = _native.cnn_latency_threshold(d, cus)
        assert [k for k, _ in _native.cnn_latency_plan(d, thr, cus)] == thr_plan  # at the threshold: throughput
        for B in BATCHES:
            plan = _native.cnn_latency_plan(d, B, cus)
            kinds = [k for k, _ in plan]
            assert all(t > 0 for _, t in plan), plan
            ws, ws_thr = (getattr(lib, q)(ctypes.byref(d), B) for q in
                          ("honk_cnn_latency_workspace_bytes", "honk_cnn_workspace_bytes"))
            assert ws >= ws_thr > 0
            if B >= thr:  # the throughput plan, step for step
                assert kinds == thr_plan, (cus, B)
                continue
            # the convs, pools and packs: the throughput plan's, each dedicated kernel as its split kind
            head, lat_head = thr_plan[:len(thr_plan) - n_lin], []
            it = iter(plan)
            for k, t in it:
                if k in (SK, SKS) or k.startswith("linear_"):
                    break
                lat_head.append((k, t))
            assert [k for k, _ in lat_head] == [SPLIT_OF.get(k, k) for k in head], (cus, B, kinds)
            for k, t in lat_head:
                if k in SPLIT_KINDS:
                    assert t >= min(cus, _yield(case, k, B)), (k, t, cus, B)
            # the Linears: split-K + sum exactly where K spans at least two slices
            tail, thr_tail = plan[len(lat_head):], thr_plan[len(thr_plan) - n_lin:]
            i = 0
            for (K, n), thr_kind in zip(linears, thr_tail):
                S = lib.honk_linear_splitk_slices(K, n)
                if S:
                    assert S >= 2 and [tail[i][0], tail[i + 1][0]] == [SK, SKS], (K, n, tail)
                    assert tail[i][1] == S * _cdiv(B, 4) * _cdiv(n, 8) and tail[i][1] % S == 0
                    # the slice count does not depend on the batch or on the device
                    assert slices.setdefault((K, n), tail[i][1] // (_cdiv(B, 4) * _cdiv(n, 8))) == S
                    i += 2
                else:
                    assert tail[i][0] == thr_kind, (K, n, tail)
                    i += 1
            assert i == len(tail)
    # a Linear's slices: a function of (K, n) that grows with K, at least two where it splits
    for K, n in linears:
        S = lib.honk_linear_splitk_slices(K, n)
        assert S == 0 or S >= 2
        assert lib.honk_linear_splitk_slices(2 * K, n) >= S


@pytest.mark.parametrize("prec", cgeo.PRECS)
@pytest.mark.parametrize("case", [c for c in cgeo.CASES if c.fast("f32") or c.fast("bf16x3")], ids=repr)
def test_switched_off_kernels_have_no_split_form(monkeypatch, case, prec):
    d = cgeo.desc(case, prec)
    for k, v in cgeo.ALL_OFF.items():
        monkeypatch.setenv(k, v)
    for cus in CUS:
        for B in BATCHES:
            kinds = [k for k, _ in _native.cnn_latency_plan(d, B, cus)]
            assert not any(k in SPLIT_KINDS for k in kinds), kinds
            n_lin = len(_linears(case))
            off = case.plan(prec, off=True)
            assert [k for k in kinds if not k.startswith("linear_")] == off[:len(off) - n_lin]
    # one switch at a time: the plan of ONE_OFF with its remaining dedicated kernels split
    if case.id == cgeo.ONE_OFF_CASE:
        for k in cgeo.ALL_OFF:
            monkeypatch.delenv(k)
        for switch, plans in cgeo.ONE_OFF.items():
            monkeypatch.setenv(switch, "0")
            kinds = [k for k, _ in _native.cnn_latency_plan(d, 3, 256)]
            want = [SPLIT_OF.get(k, k) for k in plans[prec] if not k.startswith("linear_")]
            assert [k for k in kinds if not k.startswith("linear_")] == want, (switch, kinds)
            monkeypatch.delenv(switch)


def test_refusals_match_the_launch_plan():
    lib = _native.load()
    case = cgeo.BY_ID["trad-72x40"]
    kinds, tiles = (ctypes.c_int32 * 16)(), (ctypes.c_int64 * 16)()
    bad = []
    for field, value in (("height", 0), ("width", 0), ("n_labels", 0), ("c1_out", 0), ("c1_kh", 200), ("c1_sh", 0),
                         ("p1_h", 500), ("c2_kh", 100), ("c2_out", 0), ("p2_h", 500), ("precision", 1),
                         ("precision", 3), ("precision", 9)):
        d = cgeo.desc(case, "f32")
        setattr(d, field, value)
        bad.append(d)
    for d in bad:
        want = lib.honk_cnn_launch_plan(ctypes.byref(d), kinds, 16)
        assert want < 0
        assert lib.honk_cnn_latency_plan(ctypes.byref(d), 3, 256, kinds, tiles, 16) == want
    d = cgeo.desc(case, "f32")
    assert lib.honk_cnn_latency_plan(ctypes.byref(d), 0, 256, kinds, tiles, 16) < 0
    assert lib.honk_cnn_latency_plan(ctypes.byref(d), 3, -1, kinds, tiles, 16) < 0
    assert lib.honk_cnn_latency_workspace_bytes(ctypes.byref(d), 0) == 0
    # NULL outputs: the count alone
    assert lib.honk_cnn_latency_plan(ctypes.byref(d), 3, 256, None, None, 0) == len(_native.cnn_latency_plan(d, 3, 256))
