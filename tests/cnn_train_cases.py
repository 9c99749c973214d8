"""The case table of the SpeechModel (cnn) training kernels off the workload's own shapes
(test_cnn_train_plan.py on the host, test_gpu_cnn_train_geometry.py on the device).

honk_conv2d_wgrad_f32 and honk_conv2d_dgrad_f32 (honk_amd/csrc/cnn.hip) are the backward of both
cnn convs and, through honk_amd/head_train.py, of every nn.Linear of a training step (a 1x1 conv of
a [B, in, 1, 1] map).  How they run a shape is decided on the host: wgrad_plan_c picks the
(tn, tk, S) grid and the rows per split, dgrad_plan_c the pad geometry, the workspace layout and
the GEMM's paths.  Every row below sits at one boundary of those decisions, at the smallest shape
that reaches it, and carries a ``why`` and

``sig``: the plan honk_conv2d_train_plan reports for the row, as a string
``M<rows> g<tn>x<tk>x<S> mper<rows per split> | K<cout*kh*kw> tab|ofs al|mis gx<gridDim.x>
pad<blocks>x<passes> M'<rows>`` (``| -`` at a stride other than 1: no input gradient).
test_cnn_train_plan.py holds every row to it and derives what the table claims to cover from
the query's output alone; a row whose plan moves off its boundary is replaced, not re-pinned.

The bar of every row is the project's 1e-5 (decision_replay.rel_err against float64): PyTorch's
own float32 CPU gradients of each row's inputs meet it (f32_errors(); test_cnn_train_plan.py
asserts it for every row, the longest reduction included: s1024, M = 262 088, measured 3.7e-6
on dw), so no row needs a bar derived from that error.

``kind``: "conv" runs cnn_train.conv_relu, "linear" / "linear_relu" head_train's (H = W = kh = kw
= 1).  Inputs are seeded per row (inputs()); the float64 reference is computed once per process
and shared (reference())."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from honk_amd import _native
import decision_replay as dr

BAR = 1e-5            # the project's bar on a training kernel's gradient (test_gpu_cnn_train.py)
KTAB = 4096           # constants of honk_amd/csrc/cnn.hip the rows are about
STAGE, SPLIT_MIN, N_TILE, K_TILE, GEMM_ROWS = 32, 256, 64, 64, 128
S_MAX = 1024
PAD_PASS = 65536 * 256


class Case:
    def __init__(self, name, kind, shape, stride, xgrad, sig, why):
        self.id, self.kind, self.shape, self.stride, self.xgrad = name, kind, shape, stride, xgrad
        self.sig, self.why = sig, why
        if kind != "conv":
            assert shape[2:4] == (1, 1) and shape[5:] == (1, 1) and stride == (1, 1)

    @property
    def out_hw(self):
        B, C, H, W, N, KH, KW = self.shape
        return (H - KH) // self.stride[0] + 1, (W - KW) // self.stride[1] + 1

    def __repr__(self):
        return self.id


C, L, LR = "conv", "linear", "linear_relu"
S1 = (1, 1)

CASES = [
    # ---- the weight gradient's reduction: stages of 32 rows, splits of at least 256 -----------
    Case("m1", C, (1, 1, 3, 4, 1, 3, 4), S1, True, "M1 g1x1x1 mper32 | K12 tab mis gx1 pad1x1 M'12",
         "one output pixel, one channel: a single partial stage of one row; waves 1..3 wholly masked"),
    Case("m32", C, (2, 1, 5, 5, 1, 2, 2), S1, True, "M32 g1x1x1 mper32 | K4 tab al gx1 pad1x1 M'50",
         "exactly one full stage (two clips of 16 pixels)"),
    Case("m33", C, (1, 1, 4, 12, 1, 2, 2), S1, True, "M33 g1x1x1 mper64 | K4 tab mis gx1 pad1x1 M'48",
         "one row into the second stage"),
    Case("m256", C, (1, 1, 17, 17, 1, 2, 2), S1, True, "M256 g1x1x1 mper256 | K4 tab al gx3 pad2x1 M'289",
         "the last M with one split (8 stages)"),
    Case("m257", C, (1, 2, 258, 2, 5, 2, 2), S1, True, "M257 g1x1x2 mper160 | K20 tab mis gx5 pad16x1 M'516",
         "the first M with two splits: 160 rows, then 97 = 3 stages + 1 row"),
    Case("m321-parity", C, (1, 1, 322, 2, 3, 2, 2), S1, True, "M321 g1x1x2 mper192 | K12 tab mis gx6 pad12x1 M'644",
         "full split of 6 stages (even), last split of 4 stages + 1 row (odd): the double buffer ends on the "
         "other half"),
    Case("m1793-last1", C, (1, 1, 1794, 2, 1, 2, 2), S1, True,
         "M1793 g1x1x8 mper256 | K4 tab mis gx29 pad22x1 M'3588",
         "seven full splits and a last split holding a single row"),
    Case("s1024", C, (8, 1, 182, 182, 1, 2, 2), S1, True,
         "M262088 g1x1x1024 mper256 | K4 tab al gx2071 pad1047x1 M'264992",
         "S bound by 1024 / (tn * tk) at its largest (one tile): 1024 partials summed per weight"),
    Case("s1-tiles1024", C, (1, 512, 24, 24, 65, 8, 8), S1, False,
         "M289 g2x512x1 mper320 | K4160 ofs mis gx5 pad245x1 M'576",
         "tn * tk = 1024 tiles leave S = 1 although M is past 256: ten stages in one split"),
    Case("c2-b1", C, (1, 64, 41, 16, 64, 10, 4), S1, True, "M416 g1x40x2 mper224 | K2560 tab al gx6 pad238x1 M'656",
         "cnn-trad-pool2's conv2 at one clip: 40 k-tiles, two splits of 7 and 6 stages"),
    Case("straddle", C, (5, 2, 4, 5, 3, 2, 2), S1, True, "M60 g1x1x1 mper64 | K12 tab mis gx1 pad2x1 M'100",
         "12 output pixels per clip: a stage straddles three clips of a conv (not only of a Linear)"),
    # ---- tile tails: out channels against 16 (a wave) and 64 (tn), K against 64 (tk) ----------
    Case("n15-k63", C, (2, 7, 9, 7, 15, 3, 3), S1, True, "M70 g1x1x1 mper96 | K135 tab mis gx1 pad12x1 M'126",
         "15 out channels (wave 0 partly masked, waves 1..3 wholly), K = 63: odd, one short of a tile"),
    Case("n16-k64", C, (2, 4, 9, 7, 16, 4, 4), S1, True, "M48 g1x1x1 mper64 | K256 tab al gx1 pad15x1 M'126",
         "16 out channels (wave 0 exactly), K = 64 (one k-tile exactly)"),
    Case("n17-k65", C, (2, 13, 9, 7, 17, 5, 1), S1, True, "M70 g1x2x1 mper96 | K85 tab mis gx1 pad13x1 M'126",
         "17 out channels (one into wave 1), K = 65: a second k-tile of one column"),
    Case("n64-k27", C, (2, 3, 9, 7, 64, 3, 3), S1, True, "M70 g1x1x1 mper96 | K576 tab al gx1 pad50x1 M'126",
         "64 out channels (one n-tile exactly), K = 27: K % 8 != 0"),
    Case("n65", C, (2, 3, 9, 7, 65, 3, 3), S1, True, "M70 g2x1x1 mper96 | K585 tab mis gx1 pad51x1 M'126",
         "65 out channels: a second n-tile of one channel; dgrad's K' = 585 is odd"),
    # ---- strides -------------------------------------------------------------------------------
    Case("stride5x4", C, (2, 1, 25, 19, 5, 3, 2), (5, 4), False, "M50 g1x1x1 mper64 | -",
         "stride larger than the kernel with a floor remainder on both axes ((25-3) % 5 = 2, (19-2) % 4 = 1): "
         "input rows and columns no tap reads"),
    Case("stride2x3", C, (4, 3, 17, 13, 70, 4, 3), (2, 3), False, "M112 g2x1x1 mper128 | -",
         "stride below the kernel with a floor remainder on both axes (test_gpu_cnn_train's last shape)"),
    # ---- the input gradient's GEMM: K' = cout * kh * kw around KTAB, the flipped weights -------
    Case("dk4096", C, (1, 3, 10, 9, 64, 8, 8), S1, True, "M6 g1x3x1 mper32 | K4096 tab al gx1 pad68x1 M'90",
         "K' = 4096: the last reduction with the LDS offset table; M' = 90 below one GEMM tile"),
    Case("dk4100", C, (1, 3, 6, 46, 100, 1, 41), S1, True, "M36 g2x2x1 mper64 | K4100 ofs al gx3 pad202x1 M'276",
         "K' = 4100: the first on the computed-offset path, 16-byte weight loads"),
    Case("dk4165", C, (1, 2, 12, 12, 85, 7, 7), S1, True, "M36 g2x2x1 mper64 | K4165 ofs al gx2 pad108x1 M'144",
         "K' = 4165: odd past KTAB, scalar weight loads"),
    Case("wf-misaligned", C, (1, 2, 4, 4, 6, 2, 2), S1, True, "M9 g1x1x1 mper32 | K24 tab mis gx1 pad1x1 M'16",
         "K' = 24 is a multiple of 4 but the 150 padded floats put the flipped weights 8 bytes off 16: "
         "the GEMM must fall back to scalar weight loads"),
    Case("gm129", C, (1, 1, 3, 43, 2, 2, 2), S1, True, "M84 g1x1x1 mper96 | K8 tab al gx2 pad2x1 M'129",
         "M' = 129: a second GEMM tile of one row"),
    Case("pad2", C, (1170, 1, 8, 8, 64, 8, 8), S1, True,
         "M1170 g1x1x5 mper256 | K4096 tab al gx585 pad65536x2 M'74880",
         "16 848 000 padded floats: dgrad_pad_kernel's grid-stride loop goes round twice (a 15 x 15 pad around "
         "one pixel keeps g' and dx small)"),
    # ---- Linear layers (head_train.py) ----------------------------------------------------------
    Case("lin-b1", L, (1, 37, 1, 1, 5, 1, 1), S1, True, "M1 g1x1x1 mper32 | K5 tab mis gx1 pad1x1 M'1",
         "a Linear at batch 1"),
    Case("lin-out26624", L, (2, 26624, 1, 1, 12, 1, 1), S1, True, "M2 g1x416x1 mper32 | K12 tab al gx1 pad1x1 M'2",
         "cnn-trad-pool2's output layer at 12 labels: tk = 416"),
    Case("lin-k4099-n65", L, (3, 4099, 1, 1, 65, 1, 1), S1, True, "M3 g2x65x1 mper32 | K65 tab mis gx1 pad1x1 M'3",
         "in = 4099 (past KTAB, K % 4 != 0: the forward's computed offsets and scalar weight loads), 65 outputs"),
    Case("lin-relu-b33", LR, (33, 70, 1, 1, 17, 1, 1), S1, True, "M33 g1x2x1 mper64 | K17 tab mis gx1 pad3x1 M'33",
         "linear_relu (dnn1) at batch 33: the ReLU mask on a Linear, two stages"),
]
BY_ID = {c.id: c for c in CASES}

# the rows of the device tests that take a subset
STRIDED = ("stride5x4", "stride2x3")
MASK_ROWS = ("n17-k65", "stride2x3", "lin-relu-b33")     # a conv with xgrad, a strided conv, a linear_relu
CONTRACT_ROWS = ("s1024", "wf-misaligned", "pad2", "lin-b1")


def plan(case):
    return _native.conv2d_train_plan(*case.shape, *case.stride)


def signature(case):
    p = plan(case)
    s = f"M{p['M']} g{p['tn']}x{p['tk']}x{p['S']} mper{p['mper']} | "
    if case.stride != (1, 1):
        assert not any(v for k, v in p.items() if k.startswith("dgrad_"))
        return s + "-"
    return s + (f"K{p['dgrad_k']} {'tab' if p['dgrad_ktab'] else 'ofs'} {'al' if p['dgrad_wf_aligned'] else 'mis'} "
                f"gx{p['dgrad_grid_x']} pad{p['dgrad_pad_blocks']}x{p['dgrad_pad_passes']} M'{p['dgrad_m']}")


def last_split(p):
    """Rows of the last split of a weight-gradient plan."""
    return p["M"] - (p["S"] - 1) * p["mper"]


def stages(rows):
    return -(-rows // STAGE)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(x, w, b, gy) float32 CPU tensors of the row, seeded by its position in the table; the
    weights as nn.Conv2d initialises them, the bias N(0, 0.1) so that a ReLU masks about half."""
    B, Cin, H, W, N, KH, KW = case.shape
    g = torch.Generator().manual_seed(7001 + CASES.index(case))
    x = torch.randn(B, Cin, H, W, generator=g)
    bound = 1.0 / np.sqrt(Cin * KH * KW)
    w = (torch.rand(N, Cin, KH, KW, generator=g) * 2 - 1) * bound
    b = torch.randn(N, generator=g) * 0.1
    gy = torch.randn(B, N, *case.out_hw, generator=g)
    return x, w, b, gy


def pre_activation(case, dtype=torch.float64):
    x, w, b, _ = inputs(case)
    return F.conv2d(x.to(dtype), w.to(dtype), b.to(dtype), stride=case.stride)


def grads(case, mask, dtype=torch.float64, gy=None, x=None):
    """dict(dw, db, dx) of the row in `dtype` on the CPU under the ReLU mask `mask` (bool, the
    output's shape; None: no ReLU): the reference of test_conv_relu_grads_vs_float64."""
    x0, w, _, gy0 = inputs(case)
    x = (x0 if x is None else x).to(dtype)
    gp = (gy0 if gy is None else gy).to(dtype)
    if mask is not None:
        gp = torch.where(mask, gp, torch.zeros((), dtype=dtype))
    out = dict(dw=torch.nn.grad.conv2d_weight(x, w.shape, gp, stride=case.stride), db=gp.sum((0, 2, 3)))
    if case.stride == (1, 1):
        out["dx"] = torch.nn.grad.conv2d_input(x.shape, w.to(dtype), gp, stride=case.stride)
    return out


@functools.lru_cache(maxsize=None)
def reference(case):
    """(float64 pre-activation, its own ReLU mask) of the row, shared and read-only."""
    pre = pre_activation(case)
    return pre, (pre > 0) if case.kind != L else None


def f32_errors(case):
    """rel_err of PyTorch's float32 CPU gradients against float64, both under the float64 mask."""
    _, mask = reference(case)
    ref, got = grads(case, mask), grads(case, mask, torch.float32)
    return {k: dr.rel_err(got[k].numpy(), ref[k].numpy()) for k in ref}


def never_read(case):
    """Bool [H, W]: the input positions no tap of the row reads (the same in every clip and channel)."""
    B, Cin, H, W, N, KH, KW = case.shape
    oh, ow = case.out_hw
    rows, cols = np.zeros(H, bool), np.zeros(W, bool)
    for o in range(oh):
        rows[o * case.stride[0]:o * case.stride[0] + KH] = True
    for o in range(ow):
        cols[o * case.stride[1]:o * case.stride[1] + KW] = True
    return ~np.outer(rows, cols)
