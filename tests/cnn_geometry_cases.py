"""The case table of the input-geometry tests of the SpeechModel (cnn-*) forward
(test_cnn_geometry_plan.py on the host, test_gpu_cnn_geometry.py on the device).

honk_cnn_forward picks its kernels from the descriptor: the four hand-scheduled kernels of
cnn-trad-pool2 (conv1x3 / conv1f, conv2x3 / conv2f) wherever their predicates in
honk_amd/csrc/cnn.hip hold -- not only at 101 x 40 -- and the generic implicit GEMM, in one of
its precision x fused-pool x epilogue variants, everywhere else.  Every case is one synthetic
config (a reference config with sizes overridden; a None override drops the key), random
weights from orc.make_params, PCG64 standard-normal clips of the case's own H x W, and carries

* ``plans``: per precision, the launch plan honk_cnn_launch_plan reports under the default
  environment and with the four fast paths switched off (ALL_OFF).  It is what makes a GPU
  test "of conv2f at an 18-pixel pitch" really run that kernel;
* ``f32_err`` / ``max_logit``: the conditioning of the case's own inputs -- max |logit| of
  the float64 oracle and the error of the same oracle accumulating in float32
  (orc.forward(acc=np.float32)) over the compared clips.  A 1e-4 miss on the device cannot be
  blamed on the inputs while the float32 oracle stays within a quarter of the bar
  (F32_ORACLE_MAX); test_cnn_geometry_plan re-derives both values, so neither can be edited
  by hand."""
import functools

import numpy as np

from honk_amd import _native
from oracle import ref_numpy as orc
from golden_util import ref_configs

PRECS = ("f32", "bf16x3")
ATOL = 1e-4                 # the project's bar in both modes (test_gpu_cnn_x3.ATOL, test_gpu_parity)
F32_ORACLE_MAX = ATOL / 4   # the float32-accumulating oracle's own error stays below this
SWITCHES = ("HONK_CNN_C1F", "HONK_CNN_C1X3", "HONK_CNN_C2F", "HONK_CNN_C2X3")
ALL_OFF = {v: "0" for v in SWITCHES}
# every variable that changes the cnn forward's dispatch: cleared before each run
ENV_VARS = SWITCHES + ("HONK_CNN_CHUNK",)
BATCHES = (1, 3, 300)       # 300: past a 256-CU persistent grid, some workgroups take a second clip
BMAX = max(BATCHES)

# constants of honk_amd/csrc/cnn.hip the table's bounds are about
C2_MT = 13                  # C2X3_MT == C2F_MT: 16 * MT < OH2 * OW2 <= 32 * MT
C2_LO, C2_HI = 16 * C2_MT, 32 * C2_MT
C2_IMG_PIXELS = 768         # C2X3_IMG / 128 B
C1_HMAX, C1_WMIN = 101, 39  # C1X3_HMAX; C1X3_COLS + C1X3_KW - 1 == C1F_COLS + 3

C1X, C1F, C2X, C2F = "conv1x3_kernel", "conv1f_kernel", "conv2x3_kernel", "conv2f_kernel"
PKX, PKF, MP = "pack_conv2x3_kernel", "pack_conv2f_kernel", "maxpool_kernel"
FAST = (C1X, C1F, C2X, C2F)
L4, L8, L16 = (f"linear_small_kernel<{n}>" for n in (4, 8, 16))
LG = {"f32": "linear_gemm<f32>", "bf16x3": "linear_gemm<x3>"}
P_ = {"f32": "f32", "bf16x3": "x3"}


def G(prec, pool=False, epi=""):
    """The generic conv GEMM's name (_native.cnn_kernel_name)."""
    return f"conv_gemm<{P_[prec]}{',pool2' if pool else ''}>{epi}"


NHWC = {"f32": ":nhwc-f32", "bf16x3": ":nhwc-bf16"}


def _trad(f32, x3, head=(L4,)):
    """Plans of a trad-pool2-class case: {prec: (default, all fast paths off)}; the off plan is
    conv1 on the GEMM with the fused pool, conv2 on the plain GEMM."""
    return {p: (list(d) + list(head), [G(p, True), G(p)] + list(head)) for p, d in (("f32", f32), ("bf16x3", x3))}


def _generic(*steps):
    """Plans of a case no fast path takes: the same under both environments.  A step is a
    kernel name, or a callable of the precision."""
    return {p: ([s(p) if callable(s) else s for s in steps],) * 2 for p in PRECS}


ALL_FAST = _trad([PKF, C1F, C2F], [PKX, C1X, C2X])
ALL_GEMM = _trad([G("f32", True), G("f32")], [G("bf16x3", True), G("bf16x3")])
# the generic conv1 with the NHWC epilogue feeding the dedicated conv2
C2_ONLY = _trad([PKF, G("f32", True, NHWC["f32"]), C2F], [PKX, G("bf16x3", True, NHWC["bf16x3"]), C2X])


class Case:
    def __init__(self, name, model, override, H, W, seed, plans, f32_err, max_logit):
        self.id, self.model, self.override, self.H, self.W, self.seed = name, model, override, H, W, seed
        self.plans = plans            # {precision: (default plan, plan with ALL_OFF)}
        self.f32_err = f32_err        # max |float32-accumulating oracle - float64 oracle| over sim_clips
        self.max_logit = max_logit    # max |float64 oracle logit| over sim_clips

    def plan(self, prec, off=False):
        return list(self.plans[prec][1 if off else 0])

    def fast(self, prec):
        """The hand-scheduled kernels of the case's default plan in `prec`."""
        return [k for k in self.plans[prec][0] if k in FAST]

    def __repr__(self):
        return self.id


T = "cnn-trad-pool2"        # conv1 20x8, 64 maps, pool 2x2, conv2 10x4 stride 1, no pool2, tf_variant
ONE = "cnn-one-fstride4"    # full-height conv1, stride (1, 4), 186 maps, lin + dnn1 + dnn2
K_BASE = dict(conv1_size=(6, 5), n_feature_maps2=20)  # 30 x 26 -> 25 x 22 -> pooled 12 x 11
LABELS = dict(conv1_size=(21, 8), n_feature_maps1=20)  # 21 x 16 -> 1 x 3: flat 60 -> lin 32 -> dnn1 -> ...

CASES = [
    # trad-pool2 class ----------------------------------------------------------------------
    # W = 39, the minimum width: ow1 = 32, pooled 41 x 16, conv2 416 px
    Case("trad-101x39", T, {}, 101, 39, 101, ALL_FAST, 2.38e-07, 0.30),
    # one column less: ow1 = 31, pooled 41 x 15 (615 pixels: no multiple of 4) refuses the conv1
    # kernels; conv2 32 x 12 = 384 px on its kernels at a 15-pixel pitch
    Case("trad-101x38", T, {}, 101, 38, 127, C2_ONLY, 1.95e-07, 0.46),
    # oh1 = 81 and ow1 = 33 both odd (the pool drops a row and a column): 40 x 16, conv2
    # 31 x 13 = 403 px, a ragged last m-tile
    Case("trad-100x40", T, {}, 100, 40, 102, ALL_FAST, 2.07e-07, 0.31),
    # 26 x 16, conv2 17 x 13 = 221 px: just inside the lower bound
    Case("trad-72x40", T, {}, 72, 40, 103, ALL_FAST, 2.45e-07, 0.51),
    # conv2 16 x 13 = 208 px, not above the bound: every layer on the GEMM, conv1's with the pool
    Case("trad-70x40", T, {}, 70, 40, 104, ALL_GEMM, 1.56e-07, 0.40),
    # height past C1X3_HMAX, conv2 still 416 px: generic conv1, NHWC epilogue
    Case("trad-102x40", T, {}, 102, 40, 105, C2_ONLY, 2.18e-07, 0.41),
    # conv2 33 x 13 = 429 px: everything generic
    Case("trad-103x40", T, {}, 103, 40, 106, ALL_GEMM, 1.74e-07, 0.29),
    # conv2 9 x 3: 27 taps, 18 x 14 = 252 px.  conv2f takes an odd tap count; conv2x3 refuses it,
    # and conv1x3 only runs ahead of conv2x3
    Case("trad-72x40-c2k9x3", T, dict(conv2_size=(9, 3)), 72, 40, 107,
         _trad([PKF, C1F, C2F], [G("bf16x3", True), G("bf16x3")]), 2.11e-07, 0.27),
    # out-channel counts off 64: a partly masked n-tile (33 = 2 tiles + 1), two empty ones (12)
    Case("trad-72x40-c2out33", T, dict(n_feature_maps2=33), 72, 40, 108, ALL_FAST, 2.01e-07, 0.41),
    Case("trad-72x40-c2out12", T, dict(n_feature_maps2=12), 72, 40, 109, ALL_FAST, 2.03e-07, 0.44),
    # conv1 10 x 4 (K = 40) -> 52 x 37 -> pooled 26 x 18: the conv2 kernels at an 18-pixel pitch,
    # 17 x 15 = 255 px
    Case("trad-61x40-c1k10x4", T, dict(conv1_size=(10, 4)), 61, 40, 110, C2_ONLY, 2.82e-07, 0.36),
    # 48 maps: no fast path; the GEMM with the fused pool, then K = 48 * 40
    Case("trad-72x40-maps48", T, dict(n_feature_maps1=48), 72, 40, 111, ALL_GEMM, 1.96e-07, 0.47),
    # generic class -------------------------------------------------------------------------
    # cnn-one-fstride off 101 x 40: full-height conv1 (K = 296), 9 columns at stride 4, 186 maps
    # (an N tail of 58), flat 1674 -> lin -> dnn1 -> dnn2 -> output
    Case("one-fstride4-37x43", ONE, dict(conv1_size=(37, 8)), 37, 43, 112,
         _generic(G, LG.get, LG.get, LG.get, L4), 3.34e-08, 0.18),
    # pool (3, 3) on 23 x 20 -> 7 x 6 (two rows and two columns dropped): the unfused maxpool_kernel
    Case("tpool3-37x27", "cnn-tpool3", {}, 37, 27, 113,
         _generic(G, MP, G, LG.get, LG.get, LG.get, L4), 4.90e-08, 0.08),
    # conv1 stride (4, 1) at a height that leaves a remainder: (45 - 16) / 4 + 1 = 8 rows, pool (1, 3)
    Case("tstride4-45x40", "cnn-tstride4", {}, 45, 40, 114,
         _generic(G, MP, G, LG.get, LG.get, LG.get, L4), 5.13e-08, 0.16),
    # conv2 with a stride of its own and a 2 x 2 pool2: 21 x 16 -> 9 x 14 -> 4 x 7, the fused pool
    # on conv2 (an odd oh2: a row dropped)
    Case("trad-61x40-c2s2-pool2", T, dict(conv2_size=(4, 3), conv2_stride=(2, 1), conv2_pool=(2, 2)), 61, 40, 115,
         _generic(lambda p: G(p, True), lambda p: G(p, True), L4), 2.64e-07, 0.45),
    # conv2's K = c1_out * kh * kw around KTAB = 4096 (pooled 12 x 11): the last K with the LDS
    # offset table, the first on the computed-offset path, and an odd one there (scalar W loads)
    Case("k4096", T, dict(K_BASE, conv2_size=(8, 8)), 30, 26, 116, ALL_GEMM, 1.69e-07, 0.42),
    Case("k4160", T, dict(K_BASE, conv2_size=(8, 8), n_feature_maps1=65), 30, 26, 117, ALL_GEMM, 2.37e-07, 0.41),
    Case("k4221", T, dict(K_BASE, conv2_size=(9, 7), n_feature_maps1=67), 30, 26, 118, ALL_GEMM, 1.63e-07, 0.33),
    # lin with flat = 186 * 35 = 6510: past KTAB and not a multiple of 4
    Case("one-lin6510-37x42", ONE, dict(conv1_size=(37, 8), conv1_stride=(1, 1)), 37, 42, 119,
         _generic(G, LG.get, LG.get, LG.get, L4), 4.08e-08, 0.14),
    # n_labels across the GEMV instances and the switch to the GEMM at 16 / 17, dnn1 on both
    # sides of 16 (a dnn1 of 17 also gives the next Linear a K of 17: scalar W loads)
    Case("labels1", ONE, dict(LABELS, n_labels=1, dnn1_size=16, dnn2_size=None), 21, 16, 120,
         _generic(G, LG.get, L16, L4), 1.02e-08, 0.19),
    Case("labels4", ONE, dict(LABELS, n_labels=4, dnn1_size=17), 21, 16, 121,
         _generic(G, LG.get, LG.get, LG.get, L4), 3.58e-08, 0.17),
    Case("labels5", ONE, dict(LABELS, n_labels=5, dnn1_size=12, dnn2_size=8), 21, 16, 122,
         _generic(G, LG.get, L16, L8, L8), 2.84e-08, 0.43),
    Case("labels8", ONE, dict(LABELS, n_labels=8, dnn1_size=16, dnn2_size=4), 21, 16, 123,
         _generic(G, LG.get, L16, L4, L8), 4.64e-08, 0.65),
    Case("labels9", ONE, dict(LABELS, n_labels=9, dnn1_size=17, dnn2_size=None), 21, 16, 124,
         _generic(G, LG.get, LG.get, L16), 2.72e-08, 0.29),
    Case("labels16", ONE, dict(LABELS, n_labels=16, dnn1_size=3, dnn2_size=None), 21, 16, 125,
         _generic(G, LG.get, L4, L16), 4.14e-08, 0.72),
    Case("labels17", ONE, dict(LABELS, n_labels=17, dnn1_size=16), 21, 16, 126,
         _generic(G, LG.get, L16, LG.get, LG.get), 2.06e-08, 0.23),
]
BY_ID = {c.id: c for c in CASES}

# 72 x 40 with one fast path off at a time: {switch: {precision: plan}} (a switch of the other
# precision changes nothing; conv1's dedicated kernel off leaves the GEMM's NHWC epilogue ahead
# of the dedicated conv2, conv2's off takes conv1's with it)
ONE_OFF_CASE = "trad-72x40"
ONE_OFF = {
    "HONK_CNN_C1F": {"f32": C2_ONLY["f32"][0], "bf16x3": ALL_FAST["bf16x3"][0]},
    "HONK_CNN_C1X3": {"f32": ALL_FAST["f32"][0], "bf16x3": C2_ONLY["bf16x3"][0]},
    "HONK_CNN_C2F": {"f32": ALL_GEMM["f32"][0], "bf16x3": ALL_FAST["bf16x3"][0]},
    "HONK_CNN_C2X3": {"f32": ALL_FAST["f32"][0], "bf16x3": ALL_GEMM["bf16x3"][0]},
}
SWITCH_OF = {C1F: "HONK_CNN_C1F", C1X: "HONK_CNN_C1X3", C2F: "HONK_CNN_C2F", C2X: "HONK_CNN_C2X3"}


def config(case):
    cfg = dict(ref_configs()[case.model])
    cfg.update(case.override)
    cfg = {k: v for k, v in cfg.items() if v is not None}
    cfg.update(height=case.H, width=case.W)
    return cfg


def geometry(case):
    """(oh1, ow1, ph1, pw1, oh2, ow2) of the case (conv2's: None without one)."""
    g = orc.cnn_geometry(config(case))
    c2 = g.get("conv2", (None, None, None))
    return g["conv1"][1:] + g["pool1"][1:] + c2[1:]


def desc(case, prec):
    """honk_cnn_desc of the case in `prec`, from its config alone (host-only): the fields
    SpeechModel.__init__ derives."""
    cfg = config(case)
    tf = bool(cfg.get("tf_variant"))
    d = dict(height=case.H, width=case.W, n_labels=int(cfg["n_labels"]), c1_out=int(cfg["n_feature_maps1"]),
             c1_kh=cfg["conv1_size"][0], c1_kw=cfg["conv1_size"][1], c1_sh=cfg["conv1_stride"][0],
             c1_sw=cfg["conv1_stride"][1], p1_h=cfg["conv1_pool"][0], p1_w=cfg["conv1_pool"][1],
             has_conv2=0, c2_out=0, c2_kh=0, c2_kw=0, c2_sh=1, c2_sw=1, p2_h=1, p2_w=1,
             has_lin=int(not tf), dnn1=int(cfg.get("dnn1_size", 0)), dnn2=int(cfg.get("dnn2_size", 0)),
             dnn1_relu=int(not tf))
    if "conv2_size" in cfg:
        d.update(has_conv2=1, c2_out=int(cfg["n_feature_maps2"]), c2_kh=cfg["conv2_size"][0],
                 c2_kw=cfg["conv2_size"][1], c2_sh=cfg["conv2_stride"][0], c2_sw=cfg["conv2_stride"][1],
                 p2_h=cfg["conv2_pool"][0], p2_w=cfg["conv2_pool"][1])
    return _native.CnnDesc(**{k: int(v) for k, v in d.items()}, precision=_native.PRECISIONS[prec])


@functools.lru_cache(maxsize=None)
def build(case):
    """(cfg, params, x): the model and the case's clips (read-only; a batch is the first B)."""
    cfg = config(case)
    params = orc.make_params(cfg, case.seed)
    rng = np.random.Generator(np.random.PCG64(case.seed))
    x = rng.standard_normal((BMAX, case.H, case.W)).astype(np.float32)
    x.setflags(write=False)
    return cfg, params, x


def compared(B):
    """The clips of a B-clip batch the oracle is computed for: all of a small batch; of a large
    one 8 spread clips plus the last three (second clips of the persistent workgroups)."""
    return sorted(set(list(range(0, B, max(1, B // 8)))[:8] + list(range(max(0, B - 3), B))))


def sim_clips():
    """Every clip some batch is compared on."""
    return sorted(set(i for B in BATCHES for i in compared(B)))


@functools.lru_cache(maxsize=None)
def reference(case):
    """{clip index: float64 oracle logits} over sim_clips (computed once, shared)."""
    cfg, params, x = build(case)
    idx = sim_clips()
    ref = orc.forward(params, cfg, x[idx])
    ref.setflags(write=False)
    return dict(zip(idx, ref))


def oracle(case, B):
    return np.stack([reference(case)[i] for i in compared(B)])


def conditioning(case):
    """(float32-oracle error, max |logit|) of the case over sim_clips."""
    cfg, params, x = build(case)
    idx = sim_clips()
    ref = np.stack([reference(case)[i] for i in idx])
    got = orc.forward(params, cfg, x[idx], acc=np.float32)
    return float(np.abs(got.astype(np.float64) - ref).max()), float(np.abs(ref).max())
