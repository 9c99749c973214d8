"""The case table of the cnn training kernels (cnn_train_cases.py) against the library's host-only
plan query, and the host side of the cnn training entry points against their pinned refusals
(cnn_train_abi_refusal_cases.py).

test_gpu_cnn_train_geometry.py names the boundary each of its runs sits at; this is the guard that
the name is true: honk_conv2d_train_plan -- wgrad_plan_c and dgrad_plan_c, the functions
honk_conv2d_wgrad_f32 and honk_conv2d_dgrad_f32 launch from -- gives every row's pinned plan, and
what the table claims to cover is derived from the query's output.  A row that moves off its
boundary is a finding, not a row to re-pin.

The refusals run only where the process sees no GPU: every pointer of a refused call is null or a
host buffer (test_train_abi_refusals.py's rule)."""
import ctypes

import pytest
import torch

from honk_amd import _native
from oracle import ref_numpy as orc
import cnn_train_abi_refusal_cases as abi
import cnn_train_cases as tc


@pytest.fixture()
def lib():
    from honk_amd import build
    build.build()
    return _native.load()


@pytest.mark.parametrize("case", tc.CASES, ids=repr)
def test_plan_is_the_tables(lib, case):
    assert tc.signature(case) == case.sig
    assert case.why and (case.stride == (1, 1) or not case.xgrad)


def test_table_covers_what_it_claims(lib):
    """Every boundary of the module docstring of cnn_train_cases.py, from the plans alone."""
    assert len(tc.BY_ID) == len(tc.CASES)
    plans = {c.id: tc.plan(c) for c in tc.CASES}
    P = list(plans.values())
    M = {p["M"] for p in P}
    # the reduction: one partial stage, one full stage and one row more, one split and one row more
    assert 1 in M and any(m < tc.STAGE for m in M)
    assert {tc.STAGE, tc.STAGE + 1, tc.SPLIT_MIN, tc.SPLIT_MIN + 1} <= M
    for p in P:
        assert p["mper"] % tc.STAGE == 0 and (p["S"] - 1) * p["mper"] < p["M"] <= p["S"] * p["mper"]
        assert (p["S"] == 1) == (p["M"] <= tc.SPLIT_MIN or p["tn"] * p["tk"] >= tc.S_MAX), p
    # the split count: 1, in between, and the 1024 / (tn * tk) bound at its largest; S = 1 with a long M
    # because the tiles alone fill the device
    S = {p["S"] for p in P}
    assert 1 in S and tc.S_MAX in S and any(1 < s < tc.S_MAX for s in S) and max(S) == tc.S_MAX
    assert any(p["S"] == tc.S_MAX and p["tn"] * p["tk"] == 1 for p in P)
    assert any(p["S"] == 1 and p["M"] > tc.SPLIT_MIN and p["tn"] * p["tk"] >= tc.S_MAX for p in P)
    assert any(1 < p["S"] <= 2 and p["tn"] * p["tk"] >= 40 and p["M"] >= 400 for p in P)
    # the last split: a single row; shorter than one stage; ending in a one-row stage with the other
    # parity of stage count than the full splits; odd and even stage counts
    multi = [p for p in P if p["S"] > 1]
    assert any(tc.last_split(p) == 1 for p in multi)
    assert any(tc.last_split(p) < tc.STAGE for p in multi)
    assert any(tc.last_split(p) % tc.STAGE == 1 and tc.stages(tc.last_split(p)) % 2 != tc.stages(p["mper"]) % 2
               and tc.last_split(p) > tc.STAGE for p in multi)
    counts = {tc.stages(min(p["mper"], p["M"])) % 2 for p in P} | {tc.stages(tc.last_split(p)) % 2 for p in multi}
    assert counts == {0, 1}
    # out channels around a wave (16) and a tile (64), K around a tile (64), K % 8 != 0
    N = {c.shape[4] for c in tc.CASES}
    K = {c.shape[1] * c.shape[5] * c.shape[6] for c in tc.CASES}
    assert {1, 15, 16, 17, 64, 65} <= N and min(N) < 16
    assert {63, 64, 65} <= K and any(k % 8 for k in K)
    assert {(plans[i]["tn"], plans[i]["tk"]) for i in ("n16-k64", "n17-k65", "n64-k27", "n65")} == \
        {(1, 1), (1, 2), (2, 1)}
    for c in tc.CASES:
        assert plans[c.id]["tn"] == -(-c.shape[4] // tc.N_TILE) and plans[c.id]["tk"] == -(-(
            c.shape[1] * c.shape[5] * c.shape[6]) // tc.K_TILE)
    # a stage that straddles several clips of a conv; a Linear at batch 1; the widest Linear
    assert any(c.kind == "conv" and c.out_hw[0] * c.out_hw[1] < tc.STAGE / 2 and c.shape[0] > 2 for c in tc.CASES)
    assert any(c.kind != "conv" and c.shape[0] == 1 for c in tc.CASES)
    assert any(c.kind == "linear_relu" for c in tc.CASES)
    assert any(c.kind != "conv" and plans[c.id]["tk"] == 416 for c in tc.CASES)
    assert any(c.kind != "conv" and c.shape[1] > tc.KTAB and c.shape[1] % 4 and c.shape[4] == 65 for c in tc.CASES)
    # strides: a floor remainder on both axes, below and above the kernel; never-read inputs
    for i in tc.STRIDED:
        c = tc.BY_ID[i]
        B, Cin, H, W, N_, KH, KW = c.shape
        assert (H - KH) % c.stride[0] and (W - KW) % c.stride[1]
        nr = tc.never_read(c)
        assert nr.any() and not nr.all()
        assert plans[i]["dgrad_k"] == 0 and plans[i]["dgrad_m"] == 0
    big = tc.BY_ID["stride5x4"]
    assert big.stride[0] > big.shape[5] and big.stride[1] > big.shape[6]
    nr = tc.never_read(big)
    assert nr[:big.shape[2] - 2].all(axis=1).any() and nr[:, :big.shape[3] - 1].all(axis=0).any()   # inner rows / columns
    # the input gradient: K' on both sides of KTAB and odd past it; the table <-> computed offsets
    D = [plans[c.id] for c in tc.CASES if c.xgrad]
    Kp = {p["dgrad_k"] for p in D}
    assert tc.KTAB in Kp and any(tc.KTAB < k <= tc.KTAB + 4 for k in Kp) and any(k > tc.KTAB and k % 2 for k in Kp)
    assert all(p["dgrad_ktab"] == (p["dgrad_k"] <= tc.KTAB) for p in D)
    # aligned and misaligned flipped weights where K' % 4 == 0 (the vector loads' other condition)
    assert {p["dgrad_wf_aligned"] for p in D if p["dgrad_k"] % 4 == 0} == {True, False}
    assert any(not p["dgrad_wf_aligned"] and p["dgrad_k"] % 4 == 0 and p["dgrad_k"] > 4 for p in D)
    # the GEMM's rows: below one tile, one row into another; one and two passes of the pad loop
    assert any(p["dgrad_m"] < tc.GEMM_ROWS for p in D) and any(p["dgrad_m"] % tc.GEMM_ROWS == 1 for p in D)
    assert all(p["dgrad_grid_x"] == -(-p["dgrad_m"] // tc.GEMM_ROWS) for p in D)
    assert {p["dgrad_pad_passes"] for p in D} == {1, 2}
    assert all((p["dgrad_pad_passes"] == 2) == (p["dgrad_pad_blocks"] == 65536) for p in D)
    for i in tc.MASK_ROWS + tc.CONTRACT_ROWS:
        assert i in tc.BY_ID


@pytest.mark.parametrize("case", tc.CASES, ids=repr)
def test_workspace_bytes_follow_the_plan(lib, case):
    """honk_conv2d_wgrad_workspace_bytes == S * (cout * K + cout) floats; honk_conv2d_dgrad_workspace_bytes
    == the padded g' + the flipped weights, whose alignment and pad-loop plan are the query's."""
    _, Cin, H, W, N, KH, KW = case.shape
    K = Cin * KH * KW
    for B in (1, 64, 4096):
        p = _native.conv2d_train_plan(B, *case.shape[1:], *case.stride)
        got = int(lib.honk_conv2d_wgrad_workspace_bytes(B, *case.shape[1:], *case.stride))
        assert got == p["S"] * (N * K + N) * 4, B
        if case.stride != (1, 1):
            continue
        oh, ow = H - KH + 1, W - KW + 1
        npad = B * N * (oh + 2 * (KH - 1)) * (ow + 2 * (KW - 1))
        assert int(lib.honk_conv2d_dgrad_workspace_bytes(B, *case.shape[1:])) == (npad + N * K) * 4, B
        assert p["dgrad_wf_aligned"] == (npad % 4 == 0)
        assert p["dgrad_pad_blocks"] == min(-(-npad // 256), 65536)
        assert p["dgrad_pad_passes"] == -(-npad // (p["dgrad_pad_blocks"] * 256))
        assert p["dgrad_m"] == B * H * W and p["dgrad_k"] == N * KH * KW


def test_reference_configs_at_101x40(lib):
    """The workload the table stays off: conv1, conv2 and every Linear (as a 1x1 conv) of each
    reference cnn config plan without refusal at 101 x 40, at the batches of the table."""
    from golden_util import ref_configs
    names = [n for n in ref_configs() if n.startswith("cnn")]
    assert len(names) >= 6
    for name in names:
        cfg = dict(ref_configs()[name], height=101, width=40)
        g = orc.cnn_geometry(cfg)
        convs = [(1, 101, 40, g["conv1"][0], *cfg["conv1_size"], *cfg["conv1_stride"])]
        if "conv2" in g:
            convs.append((g["pool1"][0], *g["pool1"][1:], g["conv2"][0], *cfg["conv2_size"], *cfg["conv2_stride"]))
        linears = [s for k, s in orc.cnn_param_shapes(cfg).items() if k.endswith(".weight") and len(s) == 2]
        assert linears
        for B in (1, 64, 4096):
            for c in convs:
                p = _native.conv2d_train_plan(B, *c)
                assert p["M"] > 0 and p["S"] >= 1, (name, c)
                assert int(lib.honk_conv2d_wgrad_workspace_bytes(B, *c)) > 0
            for n_out, k_in in linears:
                p = _native.conv2d_train_plan(B, k_in, 1, 1, n_out, 1, 1)
                assert p["M"] == B and p["dgrad_k"] == n_out and p["dgrad_pad_passes"] == 1, (name, n_out, k_in)


@pytest.mark.parametrize("case", tc.CASES, ids=repr)
def test_float32_reference_meets_the_bar(case):
    """The bar of the device tests is the project's 1e-5 on every row because PyTorch's own float32
    CPU gradients meet it against float64 (no bar is derived from a kernel's error); and the seeded
    inputs mask what the device tests need masked."""
    err = tc.f32_errors(case)
    print(case, {k: f"{v:.2e}" for k, v in err.items()})
    assert max(err.values()) <= tc.BAR, err
    _, mask = tc.reference(case)
    if case.id == "m1":
        assert bool(mask.all())                       # its one output passes the gradient
    elif mask is not None:
        assert 0.2 <= float((~mask).float().mean()) <= 0.8
    if case.id in tc.MASK_ROWS:
        assert mask is not None


def test_maxpool_bwd_plan(lib):
    """honk_maxpool2d_bwd_f32's grid-stride loop: one pass up to 65536 x 256 elements, two past it
    (the device test's 65 x 64 x 64 x 64)."""
    assert _native.maxpool2d_bwd_plan(4, 6, 25, 17, 2, 3) == dict(blocks=40, passes=1)
    assert _native.maxpool2d_bwd_plan(64, 64, 64, 64, 2, 2) == dict(blocks=65536, passes=1)
    assert _native.maxpool2d_bwd_plan(65, 64, 64, 64, 2, 2) == dict(blocks=65536, passes=2)
    assert _native.maxpool2d_bwd_plan(0, 6, 25, 17, 2, 3) == dict(blocks=0, passes=0)
    with pytest.raises(RuntimeError, match="bad pool 26x3 on 25x17"):
        _native.maxpool2d_bwd_plan(4, 6, 25, 17, 26, 3)


def test_plan_query_buffer(lib):
    """A short buffer gets the first n_out values and the full count; none at all is allowed."""
    c = tc.BY_ID["c2-b1"]
    want = tc.plan(c)
    out = (ctypes.c_int64 * 4)(-1, -1, -1, -1)
    n = len(_native.CONV2D_TRAIN_PLAN_FIELDS)
    assert lib.honk_conv2d_train_plan(*c.shape, 1, 1, out, 3) == n
    assert list(out) == [want["M"], want["tn"], want["tk"], -1]
    assert lib.honk_conv2d_train_plan(*c.shape, 1, 1, None, 0) == n
    with pytest.raises(RuntimeError, match="bad conv geometry"):
        _native.conv2d_train_plan(1, 64, 9, 16, 64, 10, 4)


# ---- the refusals ------------------------------------------------------------------------------
_HOST = (ctypes.c_double * 8192)()   # 64 KiB: every size a row passes fits, were it ever read


def _call(lib, fn, change):
    base = abi.BASE[fn]
    assert set(change) <= set(base), (fn, change)
    args = [ctypes.addressof(_HOST) if v is abi.P else v for v in dict(base, **change).values()]
    if fn.endswith("_plan"):
        args[-2] = ctypes.cast(args[-2], ctypes.POINTER(ctypes.c_int64)) if args[-2] else None
    rc = getattr(lib, fn)(*args)
    return rc, lib.honk_last_error().decode()


def test_refusal_table_covers_the_cnn_training_entry_points():
    named = {r[0] for r in abi.REFUSALS}
    assert named == set(abi.BASE)
    ids = [abi.row_id(r) for r in abi.REFUSALS]
    assert len(set(ids)) == len(ids)
    byte_counts = {"honk_conv2d_wgrad_workspace_bytes", "honk_conv2d_dgrad_workspace_bytes"}
    training = {n for n in _native.EXPORTS
                if n.startswith(("honk_conv2d_wgrad", "honk_conv2d_dgrad", "honk_conv2d_train", "honk_maxpool2d_bwd"))}
    assert training - byte_counts == named
    for fn, base in abi.BASE.items():
        assert len(base) == len(_native._PROTOS[fn][1]), fn
        assert abi.OK in {r[2] for r in abi.REFUSALS if r[0] == fn} or fn.endswith(("_plan", "wgrad_f32"))


@pytest.mark.parametrize("row", abi.REFUSALS, ids=abi.row_id)
def test_refusal_is_the_pinned_one(lib, row):
    if torch.cuda.is_available():
        pytest.skip("the refusal table runs only in a process that sees no GPU (its pointers are host buffers)")
    fn, change, code, text = row
    assert code in (abi.OK, abi.ARG, abi.UNSUPPORTED, abi.WORKSPACE)
    rc, err = _call(lib, fn, change)
    if code == abi.OK:
        assert rc == abi.OK      # no clip at all: nothing launched, nothing read
    else:
        assert (rc, err) == (code, text)


def test_byte_counts_of_refused_shapes_are_zero(lib):
    """(host-only at any device count)"""
    base = tuple(abi._SHAPE.values())
    assert int(lib.honk_conv2d_wgrad_workspace_bytes(*base, 1, 1)) == abi.WGRAD_WS
    assert int(lib.honk_conv2d_dgrad_workspace_bytes(*base)) == abi.DGRAD_WS
    for bad in abi.WGRAD_BYTES_ZERO:
        assert int(lib.honk_conv2d_wgrad_workspace_bytes(*bad)) == 0, bad
    for bad in abi.DGRAD_BYTES_ZERO:
        assert int(lib.honk_conv2d_dgrad_workspace_bytes(*bad)) == 0, bad
