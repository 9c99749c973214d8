"""The case table of the cnn input-geometry tests (cnn_geometry_cases.py) against the library's
host-only planner, and against the conditioning of its own inputs.

test_gpu_cnn_geometry.py names the kernel each of its runs is about; this is the guard that
the name is true: honk_cnn_launch_plan (the list honk_cnn_forward itself runs) gives the
table's plan for every case and precision, under the default environment, with every fast
path off, and with each one off alone.  A fast-kernel entry that disappears from a plan here
is a finding, not a row to re-pin: that geometry would no longer be tested on the kernel the
table names."""
import ctypes

import numpy as np
import pytest

from honk_amd import _native
from oracle import ref_numpy as orc
import cnn_geometry_cases as geo


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
    assert _native.cnn_launch_plan(d) == case.plan(prec), "default"
    for k, v in geo.ALL_OFF.items():
        monkeypatch.setenv(k, v)
    assert _native.cnn_launch_plan(d) == case.plan(prec, off=True), "all off"
    assert not set(case.plan(prec, off=True)) & set(geo.FAST + (geo.PKX, geo.PKF))


def test_reference_configs_at_101x40(lib):
    """The workload the table stays off: cnn-trad-pool2 itself plans all four dedicated
    kernels, no other reference config plans any."""
    from golden_util import ref_configs
    for name in (n for n in ref_configs() if n.startswith("cnn")):
        case = geo.Case(name, name, {}, 101, 40, 0, {}, 0.0, 0.0)
        for prec in geo.PRECS:
            plan = _native.cnn_launch_plan(geo.desc(case, prec))
            if name == geo.T:
                assert plan == geo.ALL_FAST[prec][0]
            else:
                assert plan and not set(plan) & set(geo.FAST + (geo.PKX, geo.PKF)), (name, prec, plan)


def test_module_descriptor_is_the_tables():
    """The descriptor SpeechModel derives from a case's config (what the GPU tests run) is the
    one planned here (cnn_geometry_cases.desc)."""
    from honk_amd import model as hm
    for case in geo.CASES:
        m = hm.find_model(case.model)(geo.config(case))
        for prec in geo.PRECS:
            d = _native.CnnDesc(**m._honk_desc, precision=_native.PRECISIONS[prec])
            assert bytes(d) == bytes(geo.desc(case, prec)), case


@pytest.mark.parametrize("switch", geo.SWITCHES)
def test_each_switch_alone(lib, monkeypatch, switch):
    """72 x 40 under each HONK_CNN_* switch: the plan function honours the forward's switches."""
    case = geo.BY_ID[geo.ONE_OFF_CASE]
    monkeypatch.setenv(switch, "0")
    for prec in geo.PRECS:
        assert _native.cnn_launch_plan(geo.desc(case, prec)) == geo.ONE_OFF[switch][prec], prec
    monkeypatch.setenv(switch, "1")   # any other value leaves the path on
    for prec in geo.PRECS:
        assert _native.cnn_launch_plan(geo.desc(case, prec)) == case.plan(prec), prec


def _with(prec, kernel):
    return [c for c in geo.CASES if kernel in c.plan(prec)]


def orc_flat(case):
    return orc.cnn_geometry(geo.config(case))["flat"]


def _conv2_px(case):
    g = geo.geometry(case)
    return g[4] * g[5]


def test_table_covers_what_it_claims():
    """In each precision: each of the four fast kernels at three or more geometries; both sides
    of each bound of their predicates (208 and 416 conv2 pixels, C1X3_HMAX, W = 39); each
    variant of the generic GEMM (precision x fused pool x epilogue); each linear_small
    instance and the Linear GEMM; K > KTAB in a conv."""
    assert len(geo.BY_ID) == len(geo.CASES)
    conv1 = {"f32": geo.C1F, "bf16x3": geo.C1X}
    conv2 = {"f32": geo.C2F, "bf16x3": geo.C2X}
    pack = {"f32": geo.PKF, "bf16x3": geo.PKX}
    for p in geo.PRECS:
        other = [q for q in geo.PRECS if q != p][0]
        for k in (conv1[p], conv2[p]):
            assert len({geo.geometry(c) for c in _with(p, k)}) >= 3, (p, k)
            assert not _with(other, k)            # a kernel of one precision never plans in the other
        for c in geo.CASES:                        # the pack launch goes with its conv2 kernel, conv1's kernel
            plan = c.plan(p)                       # only ahead of it
            assert (pack[p] in plan) == (conv2[p] in plan)
            assert conv1[p] not in plan or conv2[p] in plan
        c2 = _with(p, conv2[p])
        trad = [c for c in geo.CASES if c.model == geo.T and not set(c.override) - {"n_feature_maps2"}]
        # conv2's pixel bounds: 16 MT < OH * OW <= 32 MT, each met from both sides at the reference's own filter
        px = {_conv2_px(c): conv2[p] in c.plan(p) for c in trad}
        assert px[geo.C2_LO] is False and px[geo.C2_LO + 13] is True, px
        assert px[geo.C2_HI] is True and px[geo.C2_HI + 13] is False, px
        assert all(geo.C2_LO < _conv2_px(c) <= geo.C2_HI for c in c2)
        # a ragged last 16-pixel m-tile, pitches other than 16, an odd tap count (conv2f), out-channel
        # counts that mask part of an n-tile and leave whole ones empty
        assert any(_conv2_px(c) % 16 for c in c2)
        assert {geo.geometry(c)[3] for c in c2} >= {15, 16, 18}
        assert {geo.config(c)["n_feature_maps2"] for c in c2} >= {64, 33, 12}
        taps = {int(np.prod(geo.config(c)["conv2_size"])) % 2 for c in c2}
        assert taps == ({0, 1} if p == "f32" else {0})
        assert all(geo.geometry(c)[2] * geo.geometry(c)[3] <= geo.C2_IMG_PIXELS for c in c2)
        # conv1's bounds: heights up to HMAX, widths from 39, odd oh1 / ow1; past either bound the
        # GEMM's NHWC epilogue feeds the conv2 kernel
        c1 = _with(p, conv1[p])
        assert {c.H for c in c1} >= {geo.C1_HMAX, geo.C1_HMAX - 1, 72} and max(c.H for c in c1) == geo.C1_HMAX
        assert {c.W for c in c1} == {geo.C1_WMIN, geo.C1_WMIN + 1}
        assert any(geo.geometry(c)[0] % 2 and geo.geometry(c)[1] % 2 for c in c1)
        nhwc = _with(p, geo.G(p, True, geo.NHWC[p]))
        assert {(c.H, c.W) for c in nhwc} >= {(geo.C1_HMAX + 1, 40), (geo.C1_HMAX, geo.C1_WMIN - 1), (61, 40)}
        assert all(conv2[p] in c.plan(p) for c in nhwc)
        assert any(geo.config(c)["conv1_size"] != (20, 8) for c in nhwc)
        # the generic GEMM's variants, each off 101 x 40 (the table has no 101 x 40 case)
        for k in (geo.G(p), geo.G(p, True), geo.G(p, True, geo.NHWC[p]), geo.MP, geo.L4, geo.L8, geo.L16, geo.LG[p]):
            assert _with(p, k), (p, k)
        assert any(c.plan(p).count(geo.G(p, True)) == 2 for c in geo.CASES)   # the fused pool on conv2 as well
        assert not any((c.H, c.W) == (101, 40) for c in geo.CASES)
    # K of a generic conv2 on both sides of KTAB = 4096, and an odd K past it
    ks = set()
    for c in geo.CASES:
        cfg = geo.config(c)
        if "conv2_size" in cfg and not c.fast("f32"):
            ks.add(cfg["n_feature_maps1"] * int(np.prod(cfg["conv2_size"])))
    assert 4096 in ks and any(k > 4096 and k % 4 == 0 for k in ks) and any(k > 4096 and k % 2 for k in ks), ks
    # a Linear past KTAB with K % 4 != 0; n_labels across the GEMV instances and the GEMM switch
    flats = {orc_flat(c) for c in geo.CASES if geo.config(c).get("tf_variant") is None}
    assert any(f > 4096 and f % 4 for f in flats), flats
    assert {geo.config(c)["n_labels"] for c in geo.CASES} >= {1, 4, 5, 8, 9, 16, 17}
    d1 = {geo.config(c).get("dnn1_size") for c in geo.CASES}
    assert d1 & {16} and d1 & {17} and any(d and d < 16 for d in d1), d1
    # N tails of the GEMM: out-channel counts off a multiple of 64
    assert {geo.config(c)["n_feature_maps1"] % 64 for c in geo.CASES} >= {0, 58, 48, 1, 3}


@pytest.mark.parametrize("case", geo.CASES, ids=repr)
def test_workspace_accepts_every_case(lib, case):
    for prec in geo.PRECS:
        d = geo.desc(case, prec)
        for B in geo.BATCHES:
            assert lib.honk_cnn_workspace_bytes(ctypes.byref(d), B) != 0, (prec, B, lib.honk_last_error())


def test_launch_plan_errors_raise_with_reason(lib):
    """A descriptor the forward refuses gets a negative status from the plan query too, with
    the library's reason; a short kinds buffer still gets the full count."""
    case = geo.BY_ID["trad-72x40"]
    d = geo.desc(case, "f32")
    d.precision = _native.PRECISIONS["bf16"]
    with pytest.raises(RuntimeError, match="precision"):
        _native.cnn_launch_plan(d)
    d = geo.desc(case, "f32")
    d.c1_kh = case.H + 1
    with pytest.raises(RuntimeError, match="status -"):
        _native.cnn_launch_plan(d)
    d = geo.desc(case, "f32")
    kinds = (ctypes.c_int32 * 2)(-1, -1)
    assert lib.honk_cnn_launch_plan(ctypes.byref(d), kinds, 1) == len(case.plan("f32"))
    assert kinds[0] == 7 and kinds[1] == -1      # HONK_CNN_KERNEL_PACK_CONV2F; nothing past max_kinds
    assert lib.honk_cnn_launch_plan(ctypes.byref(d), None, 0) == len(case.plan("f32"))


@pytest.mark.parametrize("case", geo.CASES, ids=repr)
def test_recorded_conditioning(case):
    """A 1e-4 failure on the device must not be blameable on the inputs: the float64 oracle
    accumulating in float32 instead stays within a quarter of the bar on the case's compared
    clips, on logits of O(1).  The table's values are what this derives (the float32 error
    within a factor of 3: it is rounding noise of a BLAS whose summation order may differ; the
    logits within 10 %), so neither can be edited by hand."""
    err, mx = geo.conditioning(case)
    print(f"{case}: float32-oracle error {err:.2e}, max|logit| {mx:.2f}")
    assert err <= geo.F32_ORACLE_MAX
    assert case.f32_err <= geo.F32_ORACLE_MAX
    assert case.f32_err / 3 <= err <= case.f32_err * 3, (case.f32_err, err)
    assert abs(case.max_logit - mx) <= 0.1 * mx + 0.005, (case.max_logit, mx)
    assert 0.05 <= mx <= 2.0   # far above the bar, no overflow headroom games
