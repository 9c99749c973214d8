"""The refusals of the cnn training ABI (honk_amd/csrc/cnn.hip: honk_conv2d_wgrad_f32,
honk_conv2d_dgrad_f32, honk_maxpool2d_bwd_f32, their byte counts and the two host-only plan
queries), pinned like train_abi_refusal_cases.py pins train.hip's: the calls each entry point
refuses BEFORE ANY LAUNCH, with (return code, exact honk_last_error text).

A row is (entry point, the arguments that differ from BASE[entry point], code, text).  P stands
for a host buffer: a refused call never reads it, and the rows run only in a process that sees
no GPU (test_cnn_train_plan.py).  "+" rows pin which of two tripped checks fires first.  OK
rows are the calls that return HONK_OK without reaching a launch (no clip at all).  A weight
gradient at batch 0 reaches a hipMemsetAsync and is not here."""

OK, ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3     # HONK_* of include/honk_hip.h
P = "host buffer"
INT_MAX = 0x7fffffff
K_MAX = 65535 * 64          # conv_wgrad_kernel's gridDim.y (65535) x its 64 k columns

NULL = "null pointer argument"
PLAN_BUF = "bad plan buffer"

# 2 clips of 3 x 7 x 6 -> 5 maps by a 3 x 2 kernel: 5 x 5 outputs, M = 50, one split
_SHAPE = dict(batch=2, cin=3, h=7, w=6, cout=5, kh=3, kw=2)
WGRAD_WS = 1 * (5 * 18 + 5) * 4                      # S * (cout * K + cout) floats
DGRAD_WS = (2 * 5 * 9 * 7 + 5 * 3 * 3 * 2) * 4        # g' padded to 9 x 7, the flipped weights
_POOL = dict(batch=2, c=3, h=7, w=6, kh=3, kw=2)

BASE = {
    "honk_conv2d_wgrad_f32": dict(inp=P, gy=P, act=P, dw=P, db=P, **_SHAPE, sh=1, sw=1, workspace=P,
                                  ws_bytes=WGRAD_WS, stream=None),
    "honk_conv2d_dgrad_f32": dict(gy=P, act=P, wt=P, dx=P, **_SHAPE, workspace=P, ws_bytes=DGRAD_WS, stream=None),
    "honk_maxpool2d_bwd_f32": dict(inp=P, gout=P, gin=P, **_POOL, stream=None),
    "honk_conv2d_train_plan": dict(**_SHAPE, sh=1, sw=1, out=P, n_out=12),
    "honk_maxpool2d_bwd_plan": dict(**_POOL, out=P, n_out=2),
}


def geometry(**ch):
    g = dict(_SHAPE, sh=1, sw=1)
    g.update({k: v for k, v in ch.items() if k in g})
    return ("bad conv geometry (cin={cin} {h}x{w} k={kh}x{kw} s={sh}x{sw} cout={cout})").format(**g)


def too_large(which, chan, kh, kw, kmax):
    return f"conv training: {which}*kh*kw = {chan}*{kh}*{kw} too large (up to {kmax})"


def short_ws(have, need):
    return f"workspace {have} B < required {need} B"


def bad_pool(**ch):
    g = dict(_POOL, **ch)
    return "bad pool {kh}x{kw} on {h}x{w}".format(**g)


def _geometry_rows(fn, strided):
    """The shape rule of the two gradients and the plan query (conv_train_check)."""
    changes = [dict(batch=-1), dict(cin=0), dict(cout=0), dict(kh=0), dict(kw=0), dict(kh=8), dict(kw=7),
               dict(h=2), dict(w=1)]
    if strided:
        changes += [dict(sh=0), dict(sw=0), dict(sh=-1)]
    return [(fn, ch, ARG, geometry(**ch)) for ch in changes]


def _wgrad_k_rows(fn):
    """cin * kh * kw must fit gridDim.y of the weight gradient (and with it an int)."""
    return [
        (fn, dict(cin=K_MAX + 1, kh=1, kw=1), UNSUPPORTED, too_large("cin", K_MAX + 1, 1, 1, K_MAX)),
        (fn, dict(cin=K_MAX // 6 + 1), UNSUPPORTED, too_large("cin", K_MAX // 6 + 1, 3, 2, K_MAX)),
        (fn, dict(cin=INT_MAX), UNSUPPORTED, too_large("cin", INT_MAX, 3, 2, K_MAX)),          # past an int
        (fn, dict(cin=1, h=INT_MAX, w=INT_MAX, kh=INT_MAX, kw=INT_MAX), UNSUPPORTED,
         too_large("cin", 1, INT_MAX, INT_MAX, K_MAX)),                                       # kh * kw past an int
        (fn, dict(cin=K_MAX + 1, kh=1, kw=1, cout=0), ARG, geometry(cin=K_MAX + 1, kh=1, kw=1, cout=0)),   # +
    ]


REFUSALS = (
    # ---- honk_conv2d_wgrad_f32 -----------------------------------------------------------------
    _geometry_rows("honk_conv2d_wgrad_f32", True) + _wgrad_k_rows("honk_conv2d_wgrad_f32")
    + [("honk_conv2d_wgrad_f32", {n: None}, ARG, NULL) for n in ("inp", "gy", "dw")]
    + [("honk_conv2d_wgrad_f32", dict(workspace=None), WORKSPACE, short_ws(WGRAD_WS, WGRAD_WS)),
       ("honk_conv2d_wgrad_f32", dict(ws_bytes=WGRAD_WS - 1), WORKSPACE, short_ws(WGRAD_WS - 1, WGRAD_WS)),
       ("honk_conv2d_wgrad_f32", dict(ws_bytes=0, workspace=None), WORKSPACE, short_ws(0, WGRAD_WS)),
       ("honk_conv2d_wgrad_f32", dict(inp=None, kh=8), ARG, geometry(kh=8)),                   # + the shape first
       ("honk_conv2d_wgrad_f32", dict(inp=None, ws_bytes=0), ARG, NULL),                       # + then the pointers
       ("honk_conv2d_wgrad_f32", dict(gy=None, batch=0), ARG, NULL)]                           # + before the memset
    # ---- honk_conv2d_dgrad_f32 -----------------------------------------------------------------
    + _geometry_rows("honk_conv2d_dgrad_f32", False)
    + [("honk_conv2d_dgrad_f32", dict(cout=INT_MAX // 6 + 1), UNSUPPORTED,
        too_large("cout", INT_MAX // 6 + 1, 3, 2, INT_MAX)),
       ("honk_conv2d_dgrad_f32", dict(cout=INT_MAX), UNSUPPORTED, too_large("cout", INT_MAX, 3, 2, INT_MAX)),
       ("honk_conv2d_dgrad_f32", dict(cout=1, h=INT_MAX, w=INT_MAX, kh=INT_MAX, kw=INT_MAX), UNSUPPORTED,
        too_large("cout", 1, INT_MAX, INT_MAX, INT_MAX))]
    + [("honk_conv2d_dgrad_f32", {n: None}, ARG, NULL) for n in ("gy", "wt", "dx")]
    + [("honk_conv2d_dgrad_f32", dict(workspace=None), WORKSPACE, short_ws(DGRAD_WS, DGRAD_WS)),
       ("honk_conv2d_dgrad_f32", dict(ws_bytes=DGRAD_WS - 1), WORKSPACE, short_ws(DGRAD_WS - 1, DGRAD_WS)),
       ("honk_conv2d_dgrad_f32", dict(gy=None, kw=7), ARG, geometry(kw=7)),                    # +
       ("honk_conv2d_dgrad_f32", dict(gy=None, batch=0), ARG, NULL),                           # +
       ("honk_conv2d_dgrad_f32", dict(batch=0), OK, ""),
       ("honk_conv2d_dgrad_f32", dict(batch=0, workspace=None, ws_bytes=0), OK, "")]
    # ---- honk_maxpool2d_bwd_f32 ----------------------------------------------------------------
    + [("honk_maxpool2d_bwd_f32", {n: None}, ARG, NULL) for n in ("inp", "gout", "gin")]
    + [("honk_maxpool2d_bwd_f32", ch, ARG, bad_pool(**ch)) for ch in (
        dict(batch=-1), dict(c=0), dict(kh=0), dict(kw=0), dict(kh=8), dict(kw=7))]
    + [("honk_maxpool2d_bwd_f32", dict(inp=None, kh=8), ARG, NULL),                            # + the pointers first
       ("honk_maxpool2d_bwd_f32", dict(batch=0), OK, "")]
    # ---- the plan queries ------------------------------------------------------------------------
    + _geometry_rows("honk_conv2d_train_plan", True) + _wgrad_k_rows("honk_conv2d_train_plan")
    + [("honk_conv2d_train_plan", dict(cout=INT_MAX // 6 + 1), UNSUPPORTED,
        too_large("cout", INT_MAX // 6 + 1, 3, 2, INT_MAX)),
       ("honk_conv2d_train_plan", dict(batch=0), ARG, "conv training plan: batch 0"),
       ("honk_conv2d_train_plan", dict(out=None), ARG, PLAN_BUF),
       ("honk_conv2d_train_plan", dict(n_out=-1), ARG, PLAN_BUF),
       ("honk_conv2d_train_plan", dict(out=None, kh=8), ARG, PLAN_BUF)]                        # + the buffer first
    + [("honk_maxpool2d_bwd_plan", ch, ARG, bad_pool(**ch)) for ch in (
        dict(batch=-1), dict(c=0), dict(kh=0), dict(kh=8), dict(kw=7))]
    + [("honk_maxpool2d_bwd_plan", dict(out=None), ARG, PLAN_BUF),
       ("honk_maxpool2d_bwd_plan", dict(n_out=-1), ARG, PLAN_BUF)]
)


def row_id(row):
    fn, change = row[:2]
    return fn[5:] + ":" + ",".join(f"{k}={'null' if v is None else v}" for k, v in change.items())


# ---- the byte-count queries: 0 on every refused shape and with no clip ---------------------------
# (arguments in the order of the C signature; the accepted BASE shape gives WGRAD_WS / DGRAD_WS)
_S = tuple(_SHAPE.values())


def _shape(**ch):
    return tuple(dict(_SHAPE, **ch).values())


WGRAD_BYTES_ZERO = [_shape(batch=0) + (1, 1), _shape(batch=-1) + (1, 1), _shape(cin=0) + (1, 1),
                    _shape(cout=0) + (1, 1), _shape(kh=8) + (1, 1), _shape(kw=7) + (1, 1), _S + (0, 1), _S + (1, 0),
                    _shape(cin=K_MAX // 6 + 1) + (1, 1), _shape(cin=INT_MAX) + (1, 1)]
DGRAD_BYTES_ZERO = [_shape(batch=0), _shape(batch=-1), _shape(cin=0), _shape(cout=0), _shape(kh=8), _shape(kw=7),
                    _shape(kh=0), _shape(cout=INT_MAX // 6 + 1), _shape(cout=INT_MAX)]
