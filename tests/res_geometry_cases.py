"""The case table of the input-geometry tests of the packed SpeechResModel forward
(test_res_geometry_plan.py on the host, test_gpu_res_geometry.py on the device).

Map height and width are not constants: they are honk_res_desc.height / .width, and the host
planners of honk_amd/csrc/res.hip (plan_pair, pair_at, last_at, plan_w_th, plan_block16r,
band_geo, plan_block) are functions of them.  Every case is one calibrated random model with
inputs of its own shape -- built like test_gpu_res_kernels._case: orc.make_params,
orc.calibrate_bn on 2 clips of the case's shape, PCG64 seeds -- and carries

* ``plans``: per precision, the launch plan honk_res_launch_plan reports with 256 CUs under
  the default environment and under FORCED_P (one letter per launch, KERNEL_OF), the same for
  3 and 600 clips.  It is what makes a GPU test "of the pair kernel at 37-pixel rows" really
  run that kernel: the pair kernel is instantiated per DMA pieces-per-row, not per width
  (f16x2 / bf16: one instance for every W in 33..42, one for 11..21; bf16x3: 37..41, 19..22,
  10..13), the last-layer kernel takes 40-pixel rows only;
* ``sim``: the simulated max |logit - float64 oracle| of each reduced mode over the case's
  compared clips (sim_clips), from the float64 rounding simulation oracle/res_round_sim.py
  (operand roundings only).  The bars of f16x2 off its contract sizes and of bf16 derive from
  them (bar()); test_res_geometry_plan re-derives every value, so none can be edited by hand.

No maps of one or two pooled pixels per channel: calibrating BatchNorm on them is degenerate
(logits of 1e4, where the simulated bf16x3 error alone passes 1e-4)."""
import functools

import numpy as np

from honk_amd import _native
from oracle import ref_numpy as orc
from oracle import res_round_sim as sim
from golden_util import ref_configs

PRECS = ("bf16x3", "f16x2", "bf16")
KERNEL_OF = {"F": "block_kernel", "R": "block16r_kernel", "W": "block16w_kernel", "P": "block16p_kernel",
             "L": "block16l_kernel"}
# "forced-p": pairs wherever they plan, the last layer on the weight-stationary kernel --
# the environment of the pair-vs-w bitwise identity
FORCED_P = dict(HONK_RES_KERNEL="p", HONK_LAST_KERNEL="w")
# every variable that changes the res forward's dispatch: cleared before each run
ENV_VARS = ("HONK_RES_KERNEL", "HONK_LAST_KERNEL", "HONK_PAIR_STREAMS", "HONK_PAIR_IMM2",
            "HONK_PAIR_LIN", "HONK_F16X2_RERUN", "HONK_RES_CHUNK", "HONK_CONV0")
BMAX = 600
BF16_BOUND = 8e-3           # test_gpu_bf16.BF16_BOUND (relative past |logit| = 1)
SIM_SCHEME = {"bf16x3": "x3", "f16x2": "f16", "bf16": "bf16"}
SIM_MARGIN = 3.0            # simulated -> asserted, as the project's f16x2 bars (3.8e-5 -> 1e-4, 1.6e-4 -> 5e-4)


class Case:
    def __init__(self, model, override, H, W, seed, plans, sim, max_logit, contract=False):
        self.model, self.override, self.H, self.W, self.seed = model, override, H, W, seed
        self.plans = plans            # {precision: (default plan, forced-p plan)}, letters of KERNEL_OF
        self.sim = sim                # {precision: simulated max |logit - oracle| over sim_clips}
        self.max_logit = max_logit    # max |oracle logit| over sim_clips
        self.contract = contract      # an `auto` -> f16x2 contract size (>= 4040 unpooled pixels): B = 3 only
        self.id = f"{model}{''.join(f'-{k}{v}' for k, v in sorted(override.items()))}-{H}x{W}"

    @property
    def batches(self):
        return (3,) if self.contract else (3, BMAX)

    def plan(self, prec, forced=False):
        return [KERNEL_OF[c] for c in self.plans[prec][1 if forced else 0]]

    def __repr__(self):
        return self.id


P6L, P6W, W13, R13 = "PPPPPPL", "PPPPPPW", "W" * 13, "R" * 13
ALL_LAST = {p: (P6L, P6W) for p in PRECS}
POOLED = {"bf16x3": ("PPWW", "PPWW"), "f16x2": ("PPWW", "PPWW"), "bf16": ("PPP", "PPP")}
L6 = dict(n_layers=6)

CASES = [
    # res15 (45 maps, 13 layers, dilations 1 .. 16) ------------------------------------------
    # one row: a stream shorter than one 64-pixel step, H < every dilation > 1, dilation
    # classes with no rows at all (seed: the first past the table's whose 40-pixel calibration
    # keeps the oracle's own headroom -- simulated bf16x3 <= 2e-5, |logit| <= 2.2; 71 gave 3.2).
    # A pair whose A layer's dilation exceeds the map's height is refused (pair_at: its walk
    # takes every dilation class to hold a row; the first version of this table had P x 6 here
    # and at 7 x 40, and their 600-clip batches came out wrong by 0.1 .. 1.2): 2 pairs remain
    Case("res15", {}, 1, 40, 88, {p: ("PP" + "W" * 8 + "L", "PP" + "W" * 9) for p in PRECS},
         {"bf16x3": 1.72e-05, "f16x2": 6.43e-04, "bf16": 1.32e-02}, 1.57),
    # H < d for d = 8, 16: the (8, 8) pair refused, the (4, 8) one with its B layer's dilation
    # past the height kept
    Case("res15", {}, 7, 40, 72, {p: ("PPPPPWWL", "PPPPPWWW") for p in PRECS},
         {"bf16x3": 7.10e-06, "f16x2": 1.41e-04, "bf16": 4.96e-03}, 0.66),
    # H == 16: a multiple of every dilation (band_geo's rem == 0)
    Case("res15", {}, 16, 40, 73, ALL_LAST, {"bf16x3": 7.75e-06, "f16x2": 8.99e-05, "bf16": 3.31e-03}, 0.60),
    # an off-40 width: bf16x3's mixed plan, the other modes' 4-piece instance at a 37-pixel pitch
    Case("res15", {}, 33, 37, 74, {"bf16x3": ("PWWPPWWPW",) * 2, "f16x2": (P6W,) * 2, "bf16": (P6W,) * 2},
         {"bf16x3": 3.62e-06, "f16x2": 8.18e-05, "bf16": 3.02e-03}, 0.55),
    # both ends of the 4-piece row class (W * 96 B <= 4 KiB: 33 .. 42)
    Case("res15", {}, 9, 42, 75, {"bf16x3": (W13,) * 2, "f16x2": (P6W,) * 2, "bf16": (P6W,) * 2},
         {"bf16x3": 4.48e-06, "f16x2": 1.33e-04, "bf16": 4.09e-03}, 0.71),
    Case("res15", {}, 9, 33, 76, {"bf16x3": (W13,) * 2, "f16x2": (P6W,) * 2, "bf16": (P6W,) * 2},
         {"bf16x3": 4.51e-06, "f16x2": 1.38e-04, "bf16": 2.90e-03}, 0.71),
    # the upper end of bf16x3's 9-piece class
    Case("res15", {}, 48, 41, 77, {p: (P6W,) * 2 for p in PRECS},
         {"bf16x3": 3.46e-06, "f16x2": 6.17e-05, "bf16": 2.39e-03}, 0.47),
    # the 2-piece class off 13 / 20
    Case("res15", {}, 21, 17, 78, {"bf16x3": (W13,) * 2, "f16x2": (P6W,) * 2, "bf16": (R13, P6W)},
         {"bf16x3": 5.75e-06, "f16x2": 1.29e-04, "bf16": 3.95e-03}, 0.58),
    # the lower ends: 11-pixel rows
    Case("res15", {}, 19, 11, 79, {"bf16x3": (P6W,) * 2, "f16x2": (W13,) * 2, "bf16": (R13, "PP" + "W" * 9)},
         {"bf16x3": 5.31e-06, "f16x2": 1.10e-04, "bf16": 3.65e-03}, 0.78),
    # 25 pixels; W < d
    Case("res15", {}, 5, 5, 80, {"bf16x3": (W13,) * 2, "f16x2": (W13,) * 2, "bf16": (R13, W13)},
         {"bf16x3": 1.97e-05, "f16x2": 7.55e-04, "bf16": 1.07e-02}, 1.86),
    # the `auto` -> f16x2 contract sizes (>= 4040 unpooled pixels) off 101 x 40; 112 is the first
    # height that is a multiple of every dilation
    Case("res15", {}, 112, 40, 81, ALL_LAST, {"bf16x3": 3.80e-06, "f16x2": 3.84e-05, "bf16": 1.80e-03}, 0.34,
         contract=True),
    Case("res15", {}, 101, 41, 82, {p: (P6W,) * 2 for p in PRECS},
         {"bf16x3": 3.53e-06, "f16x2": 4.32e-05, "bf16": 3.20e-03}, 0.58, contract=True),
    # pooled: input -> map ------------------------------------------------------------------
    Case("res8", {}, 51, 39, 83, POOLED, {"bf16x3": 5.13e-06, "f16x2": 2.43e-04, "bf16": 5.17e-03}, 0.69),   # 12 x 13
    Case("res8", {}, 16, 33, 84, POOLED, {"bf16x3": 1.07e-05, "f16x2": 2.91e-04, "bf16": 5.97e-03}, 1.12),   # 4 x 11
    Case("res26", L6, 37, 41, 85, POOLED, {"bf16x3": 6.85e-06, "f16x2": 1.05e-04, "bf16": 5.33e-03}, 0.55),  # 18 x 20
    Case("res26", L6, 32, 34, 86, dict(POOLED, bf16x3=("WWWWWW",) * 2),
         {"bf16x3": 4.88e-06, "f16x2": 1.11e-04, "bf16": 2.20e-03}, 0.64),                                   # 16 x 17
    Case("res26", L6, 6, 44, 87, {"bf16x3": ("PPWW",) * 2, "f16x2": ("WWWWWW",) * 2, "bf16": ("RRRRRR", "WWWWWW")},
         {"bf16x3": 6.54e-06, "f16x2": 2.73e-04, "bf16": 3.69e-03}, 0.85),                                   # 3 x 22
]
BY_ID = {c.id: c for c in CASES}


def config(case):
    cfg = dict(ref_configs()[case.model])
    cfg.update(case.override)
    return cfg


def desc(case, prec):
    """honk_res_desc of the case in `prec`, from its config alone (host-only)."""
    cfg = config(case)
    pool = cfg.get("res_pool")
    return _native.ResDesc(n_labels=int(cfg["n_labels"]), n_maps=int(cfg["n_feature_maps"]),
                           n_layers=int(cfg["n_layers"]), use_dilation=int(bool(cfg["use_dilation"])),
                           pool_h=int(pool[0]) if pool else 0, pool_w=int(pool[1]) if pool else 0,
                           height=case.H, width=case.W, precision=_native.PRECISIONS[prec])


@functools.lru_cache(maxsize=None)
def build(case):
    """(cfg, params, x): the calibrated model and the case's clips (read-only; a batch is the
    first B of them)."""
    cfg = config(case)
    rng = np.random.Generator(np.random.PCG64(case.seed))
    params = orc.make_params(cfg, case.seed)
    params = orc.calibrate_bn(params, cfg, rng.standard_normal((2, case.H, case.W)).astype(np.float32), seed=case.seed)
    x = rng.standard_normal((max(case.batches), case.H, case.W)).astype(np.float32)
    x.setflags(write=False)
    return cfg, params, x


def compared(B):
    """The clips of a B-clip batch the oracle is computed for: all of a small batch, 8 spread
    over a large one (as test_gpu_res_kernels.test_pair_kernel_bitwise_vs_w).  (Of 600 clips on
    256 workgroups these are each a stream's first clip: the later clips of a stream are
    reached by the bitwise identities and by the batch-invariance test's last three.)"""
    return list(range(0, B, max(1, B // 8)))[:8]


def sim_clips(case):
    """Every clip some batch of the case is compared on: what the simulated errors cover."""
    return sorted(set(i for B in case.batches for i in compared(B)))


@functools.lru_cache(maxsize=None)
def reference(case):
    """{clip index: float64 oracle logits} over sim_clips (computed once, shared)."""
    cfg, params, x = build(case)
    idx = sim_clips(case)
    ref = orc.forward(params, cfg, x[idx])
    ref.setflags(write=False)
    return dict(zip(idx, ref))


def oracle(case, B):
    return np.stack([reference(case)[i] for i in compared(B)])


def simulate(case, prec):
    """max |simulated logit - oracle| of `prec`'s number formats over sim_clips."""
    cfg, params, x = build(case)
    idx = sim_clips(case)
    got = sim.fwd(params, cfg, x[idx], sim.all_layers(cfg, SIM_SCHEME[prec]))
    return float(np.abs(got - np.stack([reference(case)[i] for i in idx])).max())


def bar(case, prec):
    """The asserted bound on max |logit - float64 oracle|.  bf16x3 and f32: the project's 1e-4.
    f16x2 at its contract sizes: the header's 1e-4.  f16x2 elsewhere and bf16: the spatial mean
    averages the storage rounding over fewer pixels on a small map, so the bar follows the
    number formats' own error there -- SIM_MARGIN x the simulated error, never below the
    mode's floor (1e-4; BF16_BOUND, relative past |logit| = 1)."""
    if prec in ("bf16x3", "f32") or (prec == "f16x2" and case.contract):
        return 1e-4
    floor = 1e-4 if prec == "f16x2" else BF16_BOUND * max(1.0, case.max_logit)
    return max(floor, SIM_MARGIN * case.sim[prec])
