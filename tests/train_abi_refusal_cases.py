"""The refusals of the training ABI (honk_amd/csrc/train.hip), pinned: for every BN / tail /
conv / weight-gradient / stem entry point the calls it refuses BEFORE ANY LAUNCH, each with
its (return code, exact honk_last_error text), and the values of the byte-count queries that
do not depend on the device's CU count (test_train_abi_refusals.py).

A row is (entry point, the arguments that differ from BASE[entry point], code, text).  P
stands for a host buffer: a refused call never reads it.  Where one call trips two checks the
row pins which fires first (the "+" rows).  Calls that reach a launch or a hipMemsetAsync (a
weight gradient at batch 0, say) are not here: the device suites cover the accepted calls.
The rows were recorded from the library before its host side was rewritten in terms of one
chain of helpers; a row that changes is a changed ABI, not a row to re-pin."""

ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3     # HONK_ERR_* of include/honk_hip.h
P = "host buffer"
BIG = 1 << 31                                # one past 0x7fffffff

NULL = "null pointer argument"
BN_SHAPE = "bad batchnorm shape"
TAIL_SHAPE = "bad res tail shape"
NO_EPILOGUE = "res tail: no statistics epilogue for this shape"
NO_STATS = "conv3x3 statistics epilogue: shape outside conv3x3d_kernel"
NO_TAIL = "conv3x3 tail epilogue: shape outside conv3x3d_kernel"
NEEDS_STATS = "res tail: a folded BatchNorm needs the conv's statistics"
NEEDS_DMA = "conv3x3 wgrad: folded BatchNorm needs the DMA-staged kernels"


def short_ws(have, need):
    return f"workspace {have} B < required {need} B"


def short_stats(have, need):
    return f"statistics buffer {have} B < required {need} B"


# B = 2 of 19 maps: [19][2][2] doubles + 4 * 19 floats, for the BatchNorm workspace at any H x W
# and for the statistics buffer of 7 x 12 at d = 1 (one band per clip: a grid of 2)
BN_WS = STATS = 912
PARTIALS = 608            # honk_bn_partials_f32: the doubles alone
WGRAD_WS = 2 * 19 * 19 * 9 * 4   # 7 x 12, d = 1 and 17 x 5, d = 1: one band per clip in every family
STEM_WS = 2 * 19 * 9 * 4

_CONV = dict(batch=2, c=19, h=7, w_=12, dil=1)
_BN = dict(batch=2, c=19, hw=84)
_MAP = dict(batch=2, c=19, hh=7, ww=12, dil=1)
_STEM = dict(batch=2, c=19, h=10, w_=8, ph=2, pw=2)

# every argument of an accepted call, in the order of the C signature
BASE = {
    "honk_sgd_step_f32": dict(params=P, grads=P, momentum_buf=P, n=8, lr=0.1, momentum=0.9, weight_decay=0.0,
                              grad_scale=1.0, nesterov=0, stream=None),
    "honk_conv3x3_f32": dict(x=P, w=P, y=P, **_CONV, flip=0, stream=None),
    "honk_conv3x3_stats_f32": dict(x=P, w=P, y=P, **_CONV, flip=0, mode=1, aux=P, stats=P, stats_bytes=STATS,
                                   stream=None),
    "honk_conv3x3_stats_bn_f32": dict(x=P, w=P, y=P, **_CONV, flip=0, mode=1, aux=P, fold_mean=P, fold_invstd=P,
                                      stats=P, stats_bytes=STATS, stream=None),
    "honk_conv3x3_tail_f32": dict(x=P, w=P, s=P, mask=P, **_CONV, old=P, stats=P, stats_bytes=STATS, stream=None),
    "honk_conv3x3_tail_bn_f32": dict(x=P, w=P, s=P, mask=P, **_CONV, old=P, fold_mean=P, fold_invstd=P, stats=P,
                                     stats_bytes=STATS, stream=None),
    "honk_conv3x3_wgrad_f32": dict(x=P, dy=P, dw=P, **_CONV, workspace=P, ws_bytes=WGRAD_WS, stream=None),
    "honk_conv3x3_wgrad_bn_f32": dict(x=P, dy=P, dw=P, **_CONV, fold_mean=P, fold_invstd=P, workspace=P,
                                      ws_bytes=WGRAD_WS, stream=None),
    "honk_bn_count_scale": dict(k=1.0),
    "honk_bn_partials_f32": dict(a=P, b=P, part=P, part_bytes=PARTIALS, **_BN, stream=None),
    "honk_bn_train_fwd_f32": dict(x=P, y=P, mean=P, invstd=P, running_mean=P, running_var=P, **_BN, momentum=0.1,
                                  eps=1e-5, workspace=P, ws_bytes=BN_WS, stream=None),
    "honk_bn_train_bwd_f32": dict(dy=P, y=P, invstd=P, dx=P, **_BN, workspace=P, ws_bytes=BN_WS, stream=None),
    "honk_res_tail_fwd_f32": dict(h=P, old=P, s=P, y=P, mean=P, invstd=P, running_mean=P, running_var=P, **_BN,
                                  momentum=0.1, eps=1e-5, workspace=P, ws_bytes=BN_WS, stream=None),
    "honk_res_tail_bwd_f32": dict(gy=P, gs=P, y=P, invstd=P, h=P, gh=P, gold=P, **_BN, workspace=P, ws_bytes=BN_WS,
                                  stream=None),
    "honk_res_tail_fwd_s_f32": dict(s=P, y=P, mean=P, invstd=P, running_mean=P, running_var=P, stats=P, **_MAP,
                                    momentum=0.1, eps=1e-5, stream=None),
    "honk_res_tail_fwd_part_f32": dict(h=P, old=P, s=P, y=P, mean=P, invstd=P, running_mean=P, running_var=P,
                                       stats=P, **_MAP, momentum=0.1, eps=1e-5, stream=None),
    "honk_res_tail_bwd_part_f32": dict(gy=P, gs=P, y=P, invstd=P, h=P, gh=P, gold=P, stats=P, **_MAP, stream=None),
    "honk_res_tail_bwd_mask_f32": dict(gy=P, gs=P, y=P, invstd=P, mask=P, gh=P, gold=P, **_MAP, stats=P,
                                       stats_bytes=STATS, stream=None),
    "honk_res_tail_bwd_mask_bn_f32": dict(gy=P, gs=P, s=P, mean=P, invstd=P, mask=P, gh=P, gold=P, **_MAP, stats=P,
                                          stats_bytes=STATS, stream=None),
    "honk_res_stem_fwd_f32": dict(x=P, w0=P, y=P, **_STEM, stream=None),
    "honk_res_stem_wgrad_f32": dict(x=P, w0=P, gy=P, dw=P, **_STEM, workspace=P, ws_bytes=STEM_WS, stream=None),
}

# shapes of the geometry table (train_geometry_cases.py) without a statistics epilogue: 19 maps
# on the register-staged kernels, 45 maps
_M19 = dict(c=19, h=17, w_=5, dil=1)
_V45 = dict(c=45, h=5, w_=7, dil=1)
_M19_MAP = dict(c=19, hh=17, ww=5, dil=1)
_V45_MAP = dict(c=45, hh=5, ww=7, dil=1)


def _nulls(fn, names, text=NULL, code=ARG, **more):
    return [(fn, dict({n: None}, **more), code, text) for n in names]


def _conv_shape(fn):
    """The shape rule every block conv entry point shares (its three tensors first)."""
    return _nulls(fn, list(BASE[fn])[:3]) + [
        (fn, dict(batch=-1), ARG, "bad conv3x3 shape (B=-1 H=7 W=12)"),
        (fn, dict(h=0), ARG, "bad conv3x3 shape (B=2 H=0 W=12)"),
        (fn, dict(w_=0), ARG, "bad conv3x3 shape (B=2 H=7 W=0)"),
        (fn, dict(dil=0), ARG, "conv3x3: dilation 0 (1..64)"),
        (fn, dict(dil=65), ARG, "conv3x3: dilation 65 (1..64)"),
        (fn, dict(c=32), UNSUPPORTED, "conv3x3 training kernels: C=32 (19 or 45)"),
        (fn, dict(h=2, w_=286), UNSUPPORTED, "conv3x3: width 286 at dilation 1 too large"),
        (fn, dict(batch=BIG), ARG, "conv3x3: batch too large"),
        (fn, dict(batch=1 << 30, h=1), ARG, "conv3x3: batch too large"),
        (fn, dict(dil=0, c=32, h=2, w_=286), ARG, "conv3x3: dilation 0 (1..64)"),          # + the order of the rule
        (fn, dict(batch=-1, dil=65), ARG, "bad conv3x3 shape (B=-1 H=7 W=12)"),           # +
    ]


def _bn_shape(fn):
    return [(fn, ch, ARG, BN_SHAPE) for ch in (dict(batch=0), dict(batch=-1), dict(batch=BIG), dict(hw=0),
                                               dict(hw=BIG), dict(c=0))]


def _bn_chain(fn, required, running=False):
    rows = _nulls(fn, required) + _bn_shape(fn)
    if running:
        rows += _nulls(fn, ["running_mean", "running_var"])
    return rows + [
        (fn, dict(workspace=None), WORKSPACE, short_ws(BN_WS, BN_WS)),
        (fn, dict(ws_bytes=BN_WS - 1), WORKSPACE, short_ws(BN_WS - 1, BN_WS)),
        (fn, dict({required[0]: None}, batch=0), ARG, NULL),                               # +
        (fn, dict(batch=0, ws_bytes=0), ARG, BN_SHAPE),                                    # +
    ]


def _no_epilogue(fn, text, code=UNSUPPORTED, map_=False):
    """The statistics of a conv that has none: the two table shapes, other widths, dilations
    outside 1..64 and no clip at all."""
    m19, v45 = (_M19_MAP, _V45_MAP) if map_ else (_M19, _V45)
    return [(fn, ch, code, text) for ch in (m19, v45, dict(c=32), dict(dil=65), dict(batch=0))]


def _stats_conv(fn, fold):
    rows = _conv_shape(fn) + [
        (fn, dict(mode=3), ARG, "conv3x3 statistics mode 3 (1 or 2)"),
        (fn, dict(mode=0), ARG, "conv3x3 statistics mode 0 (1 or 2)"),
        (fn, dict(mode=2, aux=None), ARG, "conv3x3 statistics mode 2 needs the BN output"),
        (fn, _M19, UNSUPPORTED, NO_STATS), (fn, _V45, UNSUPPORTED, NO_STATS), (fn, dict(batch=0), UNSUPPORTED, NO_STATS),
        (fn, dict(stats=None), WORKSPACE, short_stats(STATS, STATS)),
        (fn, dict(stats_bytes=STATS - 1), WORKSPACE, short_stats(STATS - 1, STATS)),
        (fn, dict(mode=3, c=32), UNSUPPORTED, "conv3x3 training kernels: C=32 (19 or 45)"),   # +
        (fn, dict(_M19, mode=3), ARG, "conv3x3 statistics mode 3 (1 or 2)"),                # +
        (fn, dict(_M19, stats_bytes=0), UNSUPPORTED, NO_STATS),                             # +
    ]
    if fold:
        rows += _nulls(fn, ["fold_mean", "fold_invstd"]) + _nulls(fn, ["fold_mean"], dil=0)  # + before the shape
    return rows


def _tail_conv(fn, fold):
    rows = _conv_shape(fn) + _nulls(fn, ["mask"]) + [
        (fn, _M19, UNSUPPORTED, NO_TAIL), (fn, _V45, UNSUPPORTED, NO_TAIL), (fn, dict(batch=0), UNSUPPORTED, NO_TAIL),
        (fn, dict(stats=None), WORKSPACE, short_stats(STATS, STATS)),
        (fn, dict(stats_bytes=STATS - 1), WORKSPACE, short_stats(STATS - 1, STATS)),
        (fn, dict(mask=None, dil=0), ARG, "conv3x3: dilation 0 (1..64)"),                   # +
        (fn, dict(_M19, mask=None), ARG, NULL),                                             # +
        (fn, dict(_M19, stats_bytes=0), UNSUPPORTED, NO_TAIL),                              # +
    ]
    if fold:
        rows += _nulls(fn, ["fold_mean", "fold_invstd"]) + _nulls(fn, ["fold_mean"], dil=0)  # +
    return rows


def _wgrad(fn, fold):
    rows = _conv_shape(fn) + [
        (fn, dict(workspace=None), WORKSPACE, short_ws(WGRAD_WS, WGRAD_WS)),
        (fn, dict(ws_bytes=WGRAD_WS - 1), WORKSPACE, short_ws(WGRAD_WS - 1, WGRAD_WS)),
    ]
    if fold:
        rows += _nulls(fn, ["fold_mean", "fold_invstd"]) + _nulls(fn, ["fold_mean"], c=32) + [   # +
            (fn, _M19, UNSUPPORTED, NEEDS_DMA),   # the weight gradient of 17 x 5 is register-staged
            (fn, dict(_M19, ws_bytes=WGRAD_WS - 1), WORKSPACE, short_ws(WGRAD_WS - 1, WGRAD_WS)),   # + the size first
        ]
    return rows


def _part_tail(fn, required, running=False):
    rows = _nulls(fn, required) + _no_epilogue(fn, NO_EPILOGUE, map_=True) + [
        (fn, dict(dil=0), UNSUPPORTED, NO_EPILOGUE),
        (fn, dict(_M19_MAP, stats=None), ARG, NULL),                                        # +
    ]
    if running:
        rows += _nulls(fn, ["running_mean", "running_var"])
    return rows


def _mask_tail(fn, required, fold):
    rows = _nulls(fn, required) + [(fn, ch, ARG, TAIL_SHAPE) for ch in (
        dict(batch=0), dict(batch=-1), dict(batch=BIG), dict(c=0), dict(hh=0), dict(ww=0),
        dict(hh=65536, ww=32768), dict(batch=0, c=32))]                                     # (the last: +)
    rows += _no_epilogue(fn, NO_EPILOGUE, map_=True)[:4] + [
        (fn, dict(stats_bytes=STATS - 1), WORKSPACE, short_stats(STATS - 1, STATS)),
        (fn, dict(dil=-1, stats_bytes=BN_WS - 1), WORKSPACE, short_ws(BN_WS - 1, BN_WS)),
        (fn, dict(_M19_MAP, stats_bytes=0), UNSUPPORTED, NO_EPILOGUE),                      # +
        (fn, dict(stats=None, batch=0), ARG, NULL),                                         # +
    ]
    if fold:   # dil = 0 (the tail's own pass) is not open to a folded BatchNorm
        rows += [(fn, dict(dil=0), UNSUPPORTED, NEEDS_STATS), (fn, dict(dil=0, batch=0), UNSUPPORTED, NEEDS_STATS),
                 (fn, dict(dil=0, mask=None), ARG, NULL)]
    else:
        rows += [(fn, dict(dil=0, stats_bytes=BN_WS - 1), WORKSPACE, short_ws(BN_WS - 1, BN_WS))]
    return rows


def _stem(fn, required):
    return _nulls(fn, required) + [
        (fn, dict(batch=-1), ARG, "bad stem shape (B=-1 H=10 W=8 pool 2x2)"),
        (fn, dict(batch=BIG), ARG, f"bad stem shape (B={BIG} H=10 W=8 pool 2x2)"),
        (fn, dict(h=0), ARG, "bad stem shape (B=2 H=0 W=8 pool 2x2)"),
        (fn, dict(pw=0), ARG, "bad stem shape (B=2 H=10 W=8 pool 2x0)"),
        (fn, dict(ph=11), ARG, "bad stem shape (B=2 H=10 W=8 pool 11x2)"),
        (fn, dict(c=0), UNSUPPORTED, "stem: 0 feature maps (1..64)"),
        (fn, dict(c=65), UNSUPPORTED, "stem: 65 feature maps (1..64)"),
        (fn, dict(h=300, w_=300), UNSUPPORTED, "stem: 300x300 input too large ((H+2)(W+2) <= 38656)"),
        (fn, dict(c=65, h=0), ARG, "bad stem shape (B=2 H=0 W=8 pool 2x2)"),                 # +
    ]


REFUSALS = (
    _nulls("honk_sgd_step_f32", ["params", "grads", "momentum_buf"])
    + [("honk_sgd_step_f32", dict(n=-1), ARG, "negative size"),
       ("honk_sgd_step_f32", dict(n=-1, params=None), ARG, "negative size")]                  # +
    + _conv_shape("honk_conv3x3_f32")
    + _stats_conv("honk_conv3x3_stats_f32", fold=False) + _stats_conv("honk_conv3x3_stats_bn_f32", fold=True)
    + _tail_conv("honk_conv3x3_tail_f32", fold=False) + _tail_conv("honk_conv3x3_tail_bn_f32", fold=True)
    + _wgrad("honk_conv3x3_wgrad_f32", fold=False) + _wgrad("honk_conv3x3_wgrad_bn_f32", fold=True)
    + [("honk_bn_count_scale", dict(k=0.5), ARG, "BatchNorm count scale 0.5 outside [1, 65536]"),
       ("honk_bn_count_scale", dict(k=65537.0), ARG, "BatchNorm count scale 65537 outside [1, 65536]")]
    + _nulls("honk_bn_partials_f32", ["a", "part"]) + _bn_shape("honk_bn_partials_f32")
    + [("honk_bn_partials_f32", dict(part_bytes=PARTIALS - 1), WORKSPACE, "partials buffer too small")]
    + _bn_chain("honk_bn_train_fwd_f32", ["x", "y", "mean", "invstd"], running=True)
    + _bn_chain("honk_bn_train_bwd_f32", ["dy", "y", "invstd", "dx"])
    + _bn_chain("honk_res_tail_fwd_f32", ["h", "y", "mean", "invstd"], running=True)
    + _bn_chain("honk_res_tail_bwd_f32", ["gy", "y", "invstd", "h", "gh"])
    + _part_tail("honk_res_tail_fwd_s_f32", ["s", "mean", "invstd", "stats"], running=True)
    + _part_tail("honk_res_tail_fwd_part_f32", ["h", "y", "mean", "invstd", "stats"], running=True)
    + _part_tail("honk_res_tail_bwd_part_f32", ["gy", "y", "invstd", "h", "gh", "stats"])
    + _mask_tail("honk_res_tail_bwd_mask_f32", ["gy", "y", "invstd", "mask", "gh", "stats"], fold=False)
    + _mask_tail("honk_res_tail_bwd_mask_bn_f32", ["gy", "s", "mean", "invstd", "mask", "gh", "stats"], fold=True)
    + _stem("honk_res_stem_fwd_f32", ["x", "w0", "y"])
    + _stem("honk_res_stem_wgrad_f32", ["x", "w0", "gy", "dw"])
    + [("honk_res_stem_wgrad_f32", dict(workspace=None), WORKSPACE, short_ws(STEM_WS, STEM_WS)),
       ("honk_res_stem_wgrad_f32", dict(ws_bytes=STEM_WS - 1), WORKSPACE, short_ws(STEM_WS - 1, STEM_WS)),
       ("honk_res_stem_wgrad_f32", dict(gy=None, batch=0), ARG, NULL),                        # + before the memset
       ("honk_res_stem_wgrad_f32", dict(gy=None, c=65), UNSUPPORTED, "stem: 65 feature maps (1..64)")]   # +
)


def row_id(row):
    fn, change = row[:2]
    return fn[5:] + ":" + ",".join(f"{k}={'null' if v is None else v}" for k, v in change.items())


# ---- the byte-count queries ------------------------------------------------------------------
# honk_conv3x3_wgrad_workspace_bytes at B = 2: B * (the most bands per clip of any weight-
# gradient family that takes the shape) partial dW of C * C * 9 floats -- the bands by case id
# of train_geometry_cases.py (0: the same-conv path)
WGRAD_BANDS = {
    "19-1x4-d1": 1, "19-3x4-d4": 3, "19-4x8-d4": 4, "19-4x4-d4": 4, "19-5x256-d1": 5, "19-7x12-d3": 3,
    "19-3x220-d1": 3, "19-3x224-d1": 3, "19-26x20-d1": 2, "19-25x20-d1": 2, "19-49x20-d1": 3, "19-34x20-d1": 2,
    "19-50x20-d1": 3, "19-35x20-d1": 2, "19-7x12-d1": 1, "19-7x12-d2": 2, "19-7x12-d4": 4, "19-3x4-d1": 1,
    "19-3x4-d2": 2, "19-17x5-d1": 1, "19-5x8-d8": 5, "19-7x8-d16": 7, "19-7x12-d8": 7, "19-7x12-d16": 7,
    "19-3x4-d8": 3, "19-3x4-d16": 3, "19-1x1-d1": 1, "19-2x159-d1": 2, "19-2x161-d1": 1, "19-3x260-d1": 3,
    "19-2x285-d1": 2, "19-2x286-d1": 0, "45-25x13-d1": 2, "45-14x20-d1": 1, "45-5x7-d1": 1, "45-5x7-d2": 2,
    "45-5x7-d4": 4, "45-5x7-d8": 5, "45-5x7-d16": 5, "45-2x119-d1": 2, "45-2x120-d1": 0,
}

# honk_bn_train_workspace_bytes(B, C, HW): [C][S][2] doubles + 4 C floats, S = min(B, ceil(1024 / C))
BN_WORKSPACE = {
    (2, 19, 84): 912, (1, 19, 1): 608, (6, 19, 980): 2128, (64, 19, 980): 16720, (54, 19, 4): 16720,
    (53, 19, 4): 16416, (256, 45, 325): 17280, (23, 45, 35): 17280, (22, 45, 35): 16560, (3, 1, 7): 64,
    (2000, 1, 7): 16400, (5, 2000, 3): 64000,
}
