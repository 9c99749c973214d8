"""ctypes binding of libhonk_hip.so (include/honk_hip.h).

The shared library is the product's compute path for GPU tensors.  It is loaded
lazily; if it is missing or fails to load, every native call raises
``RuntimeError`` -- there is no silent fallback for device tensors.
"""
from __future__ import annotations

import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libhonk_hip.so")

c_f32p = ctypes.c_void_p


class ResDesc(ctypes.Structure):
    """honk_res_desc -- mirrors the SpeechResModel config keys (utils/model.py:85-92)."""
    _fields_ = [(n, ctypes.c_int32) for n in (
        "n_labels", "n_maps", "n_layers", "use_dilation", "pool_h", "pool_w", "height", "width", "precision")]


PRECISIONS = {"f32": 0, "bf16": 1, "bf16x3": 2, "f16x2": 3}
PREC_AUTO = 4  # HONK_PREC_AUTO: honk_res_select_precision's "fastest mode holding 1e-4"
PRECISION_NAMES = {v: k for k, v in PRECISIONS.items()}
NUM_COUNT = 8  # HONK_NUM_COUNT
NUM_FIELDS = ("scale", "range", "w0sum", "rho", "f16_overflow", "rho_layer", "valid", "out_scale")  # HONK_NUM_*
NUM_KW = 64  # HONK_NUM_KW: the per-layer f16x2 weight exponents follow the header


class CnnDesc(ctypes.Structure):
    """honk_cnn_desc -- mirrors the SpeechModel config keys (utils/model.py:126-180)."""
    _fields_ = [(n, ctypes.c_int32) for n in (
        "height", "width", "n_labels",
        "c1_out", "c1_kh", "c1_kw", "c1_sh", "c1_sw", "p1_h", "p1_w",
        "has_conv2", "c2_out", "c2_kh", "c2_kw", "c2_sh", "c2_sw", "p2_h", "p2_w",
        "has_lin", "dnn1", "dnn2", "dnn1_relu", "precision")]


class MfccWindowsPlan(ctypes.Structure):
    """honk_mfcc_windows_plan_t."""
    _fields_ = [(n, ctypes.c_int64) for n in (
        "windows", "shared_frames", "edge_frames", "frames_computed", "workspace_bytes")] + [
        ("shared", ctypes.c_int32), ("frames", ctypes.c_int32)]


class MfccSegmentsPlan(ctypes.Structure):
    """honk_mfcc_segments_plan_t."""
    _fields_ = [(n, ctypes.c_int64) for n in (
        "windows", "shared_frames", "edge_frames", "frames_computed", "tiles", "workspace_bytes",
        "table_bytes")] + [("shared", ctypes.c_int32), ("frames", ctypes.c_int32)]


class BankSlot(ctypes.Structure):
    """honk_bank_slot_t: the host's bookkeeping of one stream-bank slot."""
    _fields_ = [(n, ctypes.c_int32) for n in ("tail", "cached", "skip", "parity")]


class StreamBankPlan(ctypes.Structure):
    """honk_stream_bank_plan_t."""
    _fields_ = [("slot_bytes", ctypes.c_int64)] + [(n, ctypes.c_int32) for n in (
        "tail_capacity", "cache_rows", "route", "frames", "row_floats", "flo", "fhi", "q")]


class BankTickPlan(ctypes.Structure):
    """honk_bank_tick_plan_t."""
    _fields_ = [(n, ctypes.c_int64) for n in (
        "windows", "frames_computed", "frames_reused", "edge_frames", "tiles", "workspace_bytes", "table_bytes",
        "samples_in")]


BANK_SLOT_DTYPE = [("tail", "<i4"), ("cached", "<i4"), ("skip", "<i4"), ("parity", "<i4")]  # numpy view of BankSlot
BANK_ROUTES = {0: "unshared", 1: "overlap", 2: "gapped"}


class FrontPlan(ctypes.Structure):
    """honk_front_plan_t."""
    _fields_ = [(n, ctypes.c_int32) for n in ("route", "frames", "n_bins", "launches")] + [
        ("lds_bytes", ctypes.c_int64)]


FRONT_ROUTES = {1: "mfma", 2: "valu"}  # HONK_FRONT_ROUTE_*


class PcenParams(ctypes.Structure):
    """honk_pcen_params_t (defaults: HONK_PCEN_* of include/honk_hip.h)."""
    _fields_ = [(n, ctypes.c_float) for n in ("eps", "s", "alpha", "delta", "r")] + [("power", ctypes.c_int32)]


# name -> (restype, argtypes)
_PROTOS = {
    "honk_res_packed_floats": (ctypes.c_size_t, [ctypes.POINTER(ResDesc)]),
    "honk_res_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(ResDesc), ctypes.c_int64]),
    "honk_res_launch_plan": (ctypes.c_int, [ctypes.POINTER(ResDesc), ctypes.c_int64, ctypes.c_int32,
                                            ctypes.POINTER(ctypes.c_int32), ctypes.c_int32]),
    "honk_res_pack": (ctypes.c_int, [ctypes.POINTER(ResDesc), ctypes.POINTER(ctypes.c_void_p), ctypes.c_int32,
                                     c_f32p, ctypes.c_void_p]),
    "honk_res_numerics": (ctypes.c_int, [ctypes.POINTER(ResDesc), c_f32p, ctypes.POINTER(ctypes.c_float),
                                         ctypes.c_int32, ctypes.c_void_p]),
    "honk_res_select_precision": (ctypes.c_int, [ctypes.POINTER(ResDesc), ctypes.POINTER(ctypes.c_float),
                                                 ctypes.c_int32, ctypes.c_char_p, ctypes.c_size_t]),
    "honk_res_forward": (ctypes.c_int, [ctypes.POINTER(ResDesc), c_f32p, c_f32p, c_f32p, ctypes.c_int64,
                                        ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "honk_res_rerun_count": (ctypes.c_int64, []),
    "honk_res_forward_ordered": (ctypes.c_int, [ctypes.POINTER(ResDesc), c_f32p, c_f32p, c_f32p, ctypes.c_int64,
                                                ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int64,
                                                ctypes.c_void_p]),
    "honk_res_rerun_clips": (ctypes.c_int64, [ctypes.POINTER(ResDesc), ctypes.c_int64]),
    "honk_res_forward_latency": (ctypes.c_int, [ctypes.POINTER(ResDesc), c_f32p, c_f32p, c_f32p, ctypes.c_int64,
                                                ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int64,
                                                ctypes.c_void_p]),
    "honk_res_latency_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(ResDesc), ctypes.c_int64]),
    "honk_res_latency_plan": (ctypes.c_int, [ctypes.POINTER(ResDesc), ctypes.c_int64, ctypes.c_int32,
                                             ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64),
                                             ctypes.c_int32]),
    "honk_cnn_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(CnnDesc), ctypes.c_int64]),
    "honk_cnn_launch_plan": (ctypes.c_int, [ctypes.POINTER(CnnDesc), ctypes.POINTER(ctypes.c_int32), ctypes.c_int32]),
    "honk_cnn_forward": (ctypes.c_int, [ctypes.POINTER(CnnDesc), ctypes.POINTER(ctypes.c_void_p), c_f32p, c_f32p,
                                        ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "honk_cnn_forward_latency": (ctypes.c_int, [ctypes.POINTER(CnnDesc), ctypes.POINTER(ctypes.c_void_p), c_f32p,
                                                c_f32p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t,
                                                ctypes.c_void_p]),
    "honk_cnn_latency_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(CnnDesc), ctypes.c_int64]),
    "honk_cnn_latency_plan": (ctypes.c_int, [ctypes.POINTER(CnnDesc), ctypes.c_int64, ctypes.c_int32,
                                             ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64),
                                             ctypes.c_int32]),
    "honk_cnn_latency_threshold": (ctypes.c_int64, [ctypes.POINTER(CnnDesc), ctypes.c_int32]),
    "honk_cnn_features_f32": (ctypes.c_int, [ctypes.POINTER(CnnDesc), ctypes.POINTER(ctypes.c_void_p), c_f32p, c_f32p,
                                             ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                             ctypes.c_int32]),
    "honk_linear_splitk_slices": (ctypes.c_int32, [ctypes.c_int32, ctypes.c_int32]),
    "honk_linear_splitk_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]),
    "honk_linear_splitk_f32": (ctypes.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_int64, ctypes.c_int32,
                                              ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_size_t,
                                              ctypes.c_void_p]),
    "honk_conv2d_f32": (ctypes.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_int64] + [ctypes.c_int32] * 9
                        + [ctypes.c_void_p]),
    "honk_maxpool2d_f32": (ctypes.c_int, [c_f32p, c_f32p, ctypes.c_int64] + [ctypes.c_int32] * 5
                           + [ctypes.c_void_p]),
    "honk_linear_f32": (ctypes.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_int64, ctypes.c_int32,
                                       ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]),
    "honk_maxpool2d_bwd_f32": (ctypes.c_int, [c_f32p, c_f32p, c_f32p, ctypes.c_int64] + [ctypes.c_int32] * 5
                               + [ctypes.c_void_p]),
    "honk_conv2d_wgrad_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64] + [ctypes.c_int32] * 8),
    "honk_conv2d_wgrad_f32": (ctypes.c_int, [c_f32p] * 5 + [ctypes.c_int64] + [ctypes.c_int32] * 8
                              + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "honk_conv2d_dgrad_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64] + [ctypes.c_int32] * 6),
    "honk_conv2d_dgrad_f32": (ctypes.c_int, [c_f32p] * 4 + [ctypes.c_int64] + [ctypes.c_int32] * 6
                              + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "honk_conv2d_train_plan": (ctypes.c_int, [ctypes.c_int64] + [ctypes.c_int32] * 8
                               + [ctypes.POINTER(ctypes.c_int64), ctypes.c_int32]),
    "honk_maxpool2d_bwd_plan": (ctypes.c_int, [ctypes.c_int64] + [ctypes.c_int32] * 5
                                + [ctypes.POINTER(ctypes.c_int64), ctypes.c_int32]),
    "honk_conv_same_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64] + [ctypes.c_int32] * 4),
    "honk_conv_same_f32": (ctypes.c_int, [c_f32p] * 3 + [ctypes.c_int64] + [ctypes.c_int32] * 5
                           + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "honk_conv_same_wgrad_f32": (ctypes.c_int, [c_f32p] * 3 + [ctypes.c_int64] + [ctypes.c_int32] * 4
                                 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "honk_sgd_step_f32": (ctypes.c_int, [c_f32p, c_f32p, c_f32p, ctypes.c_int64, ctypes.c_float, ctypes.c_float,
                                         ctypes.c_float, ctypes.c_float, ctypes.c_int32, ctypes.c_void_p]),
    "honk_conv3x3_f32": (ctypes.c_int, [c_f32p, c_f32p, c_f32p, ctypes.c_int64] + [ctypes.c_int32] * 5
                         + [ctypes.c_void_p]),
    "honk_conv3x3_check": (ctypes.c_int, [ctypes.c_int32] * 4),
    "honk_conv3x3_plan": (ctypes.c_int, [ctypes.c_int64] + [ctypes.c_int32] * 5 + [ctypes.POINTER(ctypes.c_int32)]),
    "honk_conv3x3_wgrad_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64] + [ctypes.c_int32] * 4),
    "honk_conv3x3_wgrad_f32": (ctypes.c_int, [c_f32p, c_f32p, c_f32p, ctypes.c_int64] + [ctypes.c_int32] * 4
                               + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "honk_bn_train_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int64]),
    "honk_bn_train_fwd_f32": (ctypes.c_int, [c_f32p] * 6 + [ctypes.c_int64, ctypes.c_int32, ctypes.c_int64,
                                             ctypes.c_float, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t,
                                             ctypes.c_void_p]),
    "honk_bn_train_bwd_f32": (ctypes.c_int, [c_f32p] * 4 + [ctypes.c_int64, ctypes.c_int32, ctypes.c_int64,
                                             ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "honk_res_tail_fwd_f32": (ctypes.c_int, [c_f32p] * 8 + [ctypes.c_int64, ctypes.c_int32, ctypes.c_int64,
                                             ctypes.c_float, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t,
                                             ctypes.c_void_p]),
    "honk_res_tail_bwd_f32": (ctypes.c_int, [c_f32p] * 7 + [ctypes.c_int64, ctypes.c_int32, ctypes.c_int64,
                                             ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "honk_bn_count_scale": (ctypes.c_int, [ctypes.c_double]),
    "honk_bn_partials_f32": (ctypes.c_int, [c_f32p, c_f32p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int64,
                                            ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p]),
    "honk_conv3x3_stats_bytes": (ctypes.c_size_t, [ctypes.c_int64] + [ctypes.c_int32] * 4),
    "honk_conv3x3_stats_f32": (ctypes.c_int, [c_f32p] * 3 + [ctypes.c_int64] + [ctypes.c_int32] * 6
                               + [c_f32p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "honk_conv3x3_tail_f32": (ctypes.c_int, [c_f32p] * 3 + [ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_int32] * 4
                              + [c_f32p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "honk_res_tail_fwd_s_f32": (ctypes.c_int, [c_f32p] * 6 + [ctypes.c_void_p, ctypes.c_int64]
                                + [ctypes.c_int32] * 4 + [ctypes.c_float, ctypes.c_float, ctypes.c_void_p]),
    "honk_res_tail_bwd_mask_f32": (ctypes.c_int, [c_f32p] * 4 + [ctypes.c_void_p] + [c_f32p] * 2
                                   + [ctypes.c_int64] + [ctypes.c_int32] * 4
                                   + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "honk_conv3x3_bn_fold_check": (ctypes.c_int, [ctypes.c_int64] + [ctypes.c_int32] * 4),
    "honk_conv3x3_tail_bn_f32": (ctypes.c_int, [c_f32p] * 3 + [ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_int32] * 4
                                 + [c_f32p] * 3 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "honk_conv3x3_stats_bn_f32": (ctypes.c_int, [c_f32p] * 3 + [ctypes.c_int64] + [ctypes.c_int32] * 6
                                  + [c_f32p] * 3 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "honk_conv3x3_wgrad_bn_f32": (ctypes.c_int, [c_f32p, c_f32p, c_f32p, ctypes.c_int64] + [ctypes.c_int32] * 4
                                  + [c_f32p] * 2 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "honk_res_tail_bwd_mask_bn_f32": (ctypes.c_int, [c_f32p] * 5 + [ctypes.c_void_p] + [c_f32p] * 2
                                      + [ctypes.c_int64] + [ctypes.c_int32] * 4
                                      + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "honk_res_tail_fwd_part_f32": (ctypes.c_int, [c_f32p] * 8 + [ctypes.c_void_p, ctypes.c_int64]
                                   + [ctypes.c_int32] * 4 + [ctypes.c_float, ctypes.c_float, ctypes.c_void_p]),
    "honk_res_tail_bwd_part_f32": (ctypes.c_int, [c_f32p] * 7 + [ctypes.c_void_p, ctypes.c_int64]
                                   + [ctypes.c_int32] * 4 + [ctypes.c_void_p]),
    "honk_res_stem_fwd_f32": (ctypes.c_int, [c_f32p] * 3 + [ctypes.c_int64] + [ctypes.c_int32] * 5
                              + [ctypes.c_void_p]),
    "honk_res_stem_wgrad_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int32]),
    "honk_res_stem_wgrad_f32": (ctypes.c_int, [c_f32p] * 4 + [ctypes.c_int64] + [ctypes.c_int32] * 5
                                + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "honk_mfcc_f32": (ctypes.c_int, [c_f32p, ctypes.c_int64, ctypes.c_int32, c_f32p, ctypes.c_int32, ctypes.c_int32,
                                     c_f32p, ctypes.c_int32, c_f32p, ctypes.c_int32, c_f32p, ctypes.c_void_p]),
    "honk_mfcc_plan": (ctypes.c_int, [ctypes.c_int32] * 5 + [ctypes.c_void_p]),
    "honk_pcen_plan": (ctypes.c_int, [ctypes.c_int32] * 4 + [ctypes.c_void_p]),
    "honk_mfcc_windows_plan": (ctypes.c_int, [ctypes.c_int64] + [ctypes.c_int32] * 4 + [ctypes.c_int64] * 2
                               + [ctypes.c_void_p]),
    "honk_mfcc_windows_i16": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                             ctypes.c_int64, ctypes.c_int64, c_f32p, ctypes.c_int32, ctypes.c_int32,
                                             c_f32p, ctypes.c_int32, c_f32p, ctypes.c_int32, c_f32p, ctypes.c_void_p,
                                             ctypes.c_size_t, ctypes.c_void_p]),
    "honk_pcen_f32": (ctypes.c_int, [c_f32p, ctypes.c_int64, ctypes.c_int32, c_f32p, ctypes.c_int32, ctypes.c_int32,
                                     c_f32p, ctypes.c_int32, ctypes.c_void_p, c_f32p, ctypes.c_void_p]),
    "honk_pcen_windows_plan": (ctypes.c_int, [ctypes.c_int64] + [ctypes.c_int32] * 5 + [ctypes.c_int64] * 2
                               + [ctypes.c_void_p]),
    "honk_pcen_windows_i16": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                             ctypes.c_int64, ctypes.c_int64, c_f32p, ctypes.c_int32, ctypes.c_int32,
                                             c_f32p, ctypes.c_int32, ctypes.c_void_p, c_f32p, ctypes.c_void_p,
                                             ctypes.c_size_t, ctypes.c_void_p]),
    "honk_mfcc_segments_plan": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_int32] * 4
                                + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "honk_mfcc_segments_i16": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                              ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int32, ctypes.c_int32,
                                              c_f32p, ctypes.c_int32, ctypes.c_int32, c_f32p, ctypes.c_int32,
                                              c_f32p, ctypes.c_int32, c_f32p, ctypes.c_void_p, ctypes.c_size_t,
                                              ctypes.c_void_p]),
    "honk_pcen_segments_plan": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_int32] * 5
                                + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "honk_pcen_segments_i16": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                              ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int32, ctypes.c_int32,
                                              c_f32p, ctypes.c_int32, ctypes.c_int32, c_f32p, ctypes.c_int32,
                                              ctypes.c_void_p, c_f32p, ctypes.c_void_p, ctypes.c_size_t,
                                              ctypes.c_void_p]),
    "honk_stream_bank_plan": (ctypes.c_int, [ctypes.c_int32] * 5 + [ctypes.c_void_p]),
    "honk_mfcc_bank_tick_plan": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_int64] + [ctypes.c_int32] * 5
                                 + [ctypes.c_void_p] * 3 + [ctypes.c_size_t, ctypes.c_void_p]),
    "honk_pcen_bank_tick_plan": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_int64] + [ctypes.c_int32] * 5
                                 + [ctypes.c_void_p] * 3 + [ctypes.c_size_t, ctypes.c_void_p]),
    "honk_mfcc_bank_tick_i16": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t,
                                               ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int32, ctypes.c_int32,
                                               c_f32p, ctypes.c_int32, ctypes.c_int32, c_f32p, ctypes.c_int32,
                                               c_f32p, ctypes.c_int32, c_f32p, ctypes.c_void_p, ctypes.c_size_t,
                                               ctypes.c_void_p]),
    "honk_pcen_bank_tick_i16": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t,
                                               ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int32, ctypes.c_int32,
                                               c_f32p, ctypes.c_int32, ctypes.c_int32, c_f32p, ctypes.c_int32,
                                               ctypes.c_void_p, c_f32p, ctypes.c_void_p, ctypes.c_size_t,
                                               ctypes.c_void_p]),
    "honk_listen_decide_f32": (ctypes.c_int, [c_f32p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64,
                                              ctypes.c_int32, ctypes.c_double] + [ctypes.c_void_p] * 6),
    "honk_spatial_mean_f32": (ctypes.c_int, [c_f32p, c_f32p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p]),
    "honk_spatial_mean_bwd_f32": (ctypes.c_int, [c_f32p, c_f32p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p]),
    "honk_cross_entropy_f32": (ctypes.c_int, [c_f32p, ctypes.c_void_p, c_f32p, ctypes.c_int64, ctypes.c_int32,
                                              ctypes.c_void_p]),
    "honk_cross_entropy_bwd_f32": (ctypes.c_int, [c_f32p, ctypes.c_void_p, c_f32p, c_f32p, ctypes.c_int64,
                                                  ctypes.c_int32, ctypes.c_void_p]),
    "honk_augment_f32": (ctypes.c_int, [c_f32p, c_f32p] + [ctypes.c_void_p] * 2 + [c_f32p, ctypes.c_void_p, c_f32p,
                                                                                    ctypes.c_int64, ctypes.c_int32,
                                                                                    ctypes.c_int64, ctypes.c_void_p]),
    "honk_last_error": (ctypes.c_char_p, []),
    "honk_version": (ctypes.c_char_p, []),
    "honk_timing_enable": (ctypes.c_int, [ctypes.c_int32]),
    "honk_timing_read": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64),
                                        ctypes.POINTER(ctypes.c_double)]),
}

EXPORTS = tuple(_PROTOS)

_lib = None
_lock = threading.Lock()


def load(path: str = None):
    """Load (once) and return the ctypes library; raise RuntimeError if unavailable.
    ``HONK_LIB`` names an alternative build of the library (experiment builds)."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("HONK_LIB") or LIB_PATH
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(path):
            raise RuntimeError(
                f"honk_amd: HIP extension not built ({path} missing); run `python -m honk_amd.build`")
        try:
            lib = ctypes.CDLL(path)
        except OSError as e:  # pragma: no cover - depends on ROCm install
            raise RuntimeError(f"honk_amd: cannot load {path}: {e}") from e
        for name, (res, args) in _PROTOS.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load().honk_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed (status {rc}): {msg}")


def version() -> str:
    return load().honk_version().decode()


def ptr(t) -> int:
    return t.data_ptr() if t is not None else 0


def ptr_array(tensors):
    arr = (ctypes.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = ptr(t) if t is not None else None
    return arr


def stream_handle(device) -> int:
    import torch
    return torch.cuda.current_stream(device).cuda_stream


def timing_enable(on: bool):
    check(load().honk_timing_enable(1 if on else 0), "honk_timing_enable")


def timing_read():
    ms = ctypes.c_double()
    n = ctypes.c_int64()
    fl = ctypes.c_double()
    check(load().honk_timing_read(ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl)), "honk_timing_read")
    return ms.value, n.value, fl.value


# HONK_KERNEL_* of include/honk_hip.h
KERNEL_NAMES = {1: "block_kernel", 2: "block16r_kernel", 3: "block16w_kernel", 4: "block16p_kernel",
                5: "block16l_kernel", 8: "block16s_kernel"}  # (6 and 7 are retired)


def res_launch_plan(desc, batch: int, n_cus: int = 0):
    """The block-layer launches honk_res_forward makes per batch chunk, as kernel
    names (HONK_KERNEL_* codes mapped through KERNEL_NAMES).  Host-only."""
    lib = load()
    kinds = (ctypes.c_int32 * 256)()
    n = lib.honk_res_launch_plan(ctypes.byref(desc), int(batch), int(n_cus), kinds, 256)
    if n < 0:
        check(n, "honk_res_launch_plan")
    return [KERNEL_NAMES[kinds[i]] for i in range(min(n, 256))]


def res_latency_plan(desc, batch: int, n_cus: int = 0):
    """The block-layer launches honk_res_forward_latency makes per batch chunk:
    [(kernel name, tiles)].  Host-only."""
    lib = load()
    kinds, tiles = (ctypes.c_int32 * 256)(), (ctypes.c_int64 * 256)()
    n = lib.honk_res_latency_plan(ctypes.byref(desc), int(batch), int(n_cus), kinds, tiles, 256)
    if n < 0:
        check(n, "honk_res_latency_plan")
    return [(KERNEL_NAMES[kinds[i]], int(tiles[i])) for i in range(min(n, 256))]


# HONK_CNN_KERNEL_* of include/honk_hip.h (the generic conv GEMM's flags: cnn_kernel_name)
CNN_KERNEL_NAMES = {1: "conv1x3_kernel", 2: "conv1f_kernel", 3: "conv2x3_kernel", 4: "conv2f_kernel",
                    5: "maxpool_kernel", 6: "pack_conv2x3_kernel", 7: "pack_conv2f_kernel",
                    8: "linear_small_kernel<4>", 9: "linear_small_kernel<8>", 10: "linear_small_kernel<16>",
                    11: "linear_gemm<f32>", 12: "linear_gemm<x3>",
                    # the latency schedule's (honk_cnn_latency_plan)
                    13: "conv1xs_kernel", 14: "conv1fs_kernel", 15: "conv2xs_kernel", 32: "conv2fs_kernel",
                    33: "linear_splitk_kernel", 34: "linear_splitk_sum_kernel"}
CNN_KERNEL_GEMM = 16
# a dedicated conv of the throughput plan -> its split form in the latency plan
CNN_SPLIT_OF = {"conv1x3_kernel": "conv1xs_kernel", "conv1f_kernel": "conv1fs_kernel",
                "conv2x3_kernel": "conv2xs_kernel", "conv2f_kernel": "conv2fs_kernel"}


def cnn_kernel_name(kind: int) -> str:
    """A HONK_CNN_KERNEL_* code as a name; the generic conv GEMM as
    ``conv_gemm<f32|x3[,pool2]>[:nhwc-bf16|:nhwc-f32]`` (no suffix: NCHW fp32)."""
    if kind & CNN_KERNEL_GEMM:
        flags = kind & ~CNN_KERNEL_GEMM
        if flags & ~15 or (flags & 12) == 12:
            raise RuntimeError(f"honk_cnn_launch_plan: unknown kernel kind {kind}")
        return (f"conv_gemm<{'x3' if flags & 1 else 'f32'}{',pool2' if flags & 2 else ''}>"
                + (":nhwc-bf16" if flags & 4 else ":nhwc-f32" if flags & 8 else ""))
    return CNN_KERNEL_NAMES[kind]


def cnn_launch_plan(desc):
    """The launches honk_cnn_forward makes -- the per-call conv2 weight pack (if any), then one
    chunk's kernels in order -- as names (cnn_kernel_name), under the current HONK_CNN_*
    environment.  Host-only."""
    kinds = (ctypes.c_int32 * 16)()
    n = load().honk_cnn_launch_plan(ctypes.byref(desc), kinds, 16)
    if n < 0:
        check(n, "honk_cnn_launch_plan")
    return [cnn_kernel_name(kinds[i]) for i in range(min(n, 16))]


def cnn_latency_plan(desc, batch: int, n_cus: int = 0):
    """The launches honk_cnn_forward_latency makes for one chunk of ``batch`` clips on a device
    of ``n_cus`` CUs (0: ask the device): [(kernel name, workgroups)], under the current
    HONK_CNN_* environment.  Host-only where n_cus > 0."""
    kinds, tiles = (ctypes.c_int32 * 16)(), (ctypes.c_int64 * 16)()
    n = load().honk_cnn_latency_plan(ctypes.byref(desc), int(batch), int(n_cus), kinds, tiles, 16)
    if n < 0:
        check(n, "honk_cnn_latency_plan")
    return [(cnn_kernel_name(kinds[i]), int(tiles[i])) for i in range(min(n, 16))]


def cnn_latency_threshold(desc, n_cus: int = 0) -> int:
    """Chunks of fewer clips than this run the latency schedule's split kernels in the descriptor's
    precision (n_cus 0: ask the device)."""
    n = load().honk_cnn_latency_threshold(ctypes.byref(desc), int(n_cus))
    if n < 0:
        check(int(n), "honk_cnn_latency_threshold")
    return int(n)


def front_plan(samples, n_fft, hop, n_mels, n_dct=None):
    """honk_mfcc_plan (n_dct given) or honk_pcen_plan (n_dct None) under the current HONK_MFCC_VALU
    environment -> (status, FrontPlan); the plan is filled where status is 0.  Host-only."""
    plan, lib = FrontPlan(), load()
    if n_dct is None:
        rc = lib.honk_pcen_plan(int(samples), int(n_fft), int(hop), int(n_mels), ctypes.addressof(plan))
    else:
        rc = lib.honk_mfcc_plan(int(samples), int(n_fft), int(hop), int(n_mels), int(n_dct), ctypes.addressof(plan))
    return rc, plan


LISTEN_MAX_LABELS = 64        # HONK_LISTEN_MAX_LABELS
LISTEN_MAX_WINDOWS = 1 << 23  # HONK_LISTEN_MAX_WINDOWS


def listen_window0(window0, n, who="listen_decide"):
    """A segment table as a contiguous int64 array: ``window0[0] == 0``, non-decreasing, last entry ``n``
    (ValueError otherwise)."""
    import numpy as np
    w0 = np.asarray(window0)
    if w0.ndim != 1 or w0.size < 1 or w0.dtype.kind not in "iu":
        raise ValueError(f"{who}: window0 must be a 1-D integer array of segments + 1 entries")
    w0 = np.ascontiguousarray(w0, dtype=np.int64)
    if w0[0] != 0 or (np.diff(w0) < 0).any() or w0[-1] != n:
        raise ValueError(f"{who}: window0 must start at 0, not decrease and end at {n}")
    return w0


def listen_decide(logits, window0=None, keyword=-1, min_prob=0.85):
    """honk_listen_decide_f32 on a ROCm float32 tensor ``logits`` [n, n_labels] -> device tensors
    ``(label int32 [n], prob float32 [n])``, and with ``window0`` (numpy int64 [segments + 1], checked here,
    then uploaded) also ``(sums float64, counts int32 [segments, n_labels], hit int64 [segments])``.
    Only enqueues on the current stream of the tensor's device."""
    import torch
    if not torch.is_tensor(logits) or not logits.is_cuda or logits.dtype != torch.float32 or logits.dim() != 2:
        raise ValueError("listen_decide: logits must be a 2-D float32 tensor on a ROCm device")
    n, n_labels = logits.shape
    w0 = None if window0 is None else listen_window0(window0, n)
    logits = logits.detach().contiguous()
    dev = logits.device
    label = torch.empty(n, dtype=torch.int32, device=dev)
    prob = torch.empty(n, dtype=torch.float32, device=dev)
    segments = 0 if w0 is None else w0.size - 1
    w0_dev = sums = counts = hit = None
    if w0 is not None:
        w0_dev = torch.from_numpy(w0).to(dev)
        sums = torch.empty(segments, n_labels, dtype=torch.float64, device=dev)
        counts = torch.empty(segments, n_labels, dtype=torch.int32, device=dev)
        hit = torch.empty(segments, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = load().honk_listen_decide_f32(ptr(logits), n, n_labels, ptr(w0_dev), segments, int(keyword),
                                           float(min_prob), ptr(label), ptr(prob), ptr(sums), ptr(counts), ptr(hit),
                                           stream_handle(dev))
    check(rc, "honk_listen_decide_f32")
    return (label, prob) if w0 is None else (label, prob, sums, counts, hit)


def res_numerics(desc, packed, device):
    """The pack-time numerics record of a packed res model (HONK_NUM_*) as a dict;
    synchronises the device's current stream (once per pack)."""
    n = NUM_KW + desc.n_layers
    rec = (ctypes.c_float * n)()
    check(load().honk_res_numerics(ctypes.byref(desc), packed.data_ptr(), rec, n, stream_handle(device)),
          "honk_res_numerics")
    out = {k: float(rec[i]) for i, k in enumerate(NUM_FIELDS)}
    out["kw"] = [int(rec[NUM_KW + i]) for i in range(desc.n_layers)]
    return out, rec


def res_select_precision(desc, rec, requested: str):
    """honk_res_select_precision: (precision name to run, note on why the request was
    not taken or "")."""
    note = ctypes.create_string_buffer(512)
    req = PREC_AUTO if requested == "auto" else PRECISIONS[requested]
    p = load().honk_res_select_precision(ctypes.byref(desc), rec, req, note, len(note))
    if p < 0:
        check(p, "honk_res_select_precision")
    return PRECISION_NAMES[p], note.value.decode(errors="replace")


# HONK_CONV3X3_FAMILY_* / HONK_CONV3X3_PLAN_* of include/honk_hip.h
CONV3X3_FAMILIES = {0: None, 1: "d", 2: "m", 3: "v"}
CONV3X3_PLAN_COUNT = 16


def conv3x3_plan(batch: int, c: int, h: int, w: int, dil: int, n_cus: int = 0):
    """honk_conv3x3_plan: the kernels the training block convs run (batch, C, H, W, dil) on
    under the current environment, or None where the dedicated kernels do not take the shape
    (the same-conv path).  Host-only.  {"conv": dict(family "d" | "m" | "v", np, fixed, th,
    nband, grid), "wgrad": dict(family, variant "q" | "h" | "d" | None, fixed, th, nband,
    grid), "stats": bool, "fold": bool}."""
    out = (ctypes.c_int32 * CONV3X3_PLAN_COUNT)()
    check(load().honk_conv3x3_plan(int(batch), int(c), int(h), int(w), int(dil), int(n_cus), out), "honk_conv3x3_plan")
    if not out[0]:
        return None
    return {"conv": dict(family=CONV3X3_FAMILIES[out[1]], np=out[2], fixed=bool(out[3]), th=out[4], nband=out[5],
                         grid=out[6]),
            "wgrad": dict(family=CONV3X3_FAMILIES[out[8]], variant=chr(out[9]) if out[9] else None,
                          fixed=bool(out[10]), th=out[11], nband=out[12], grid=out[13]),
            "stats": bool(out[7]), "fold": bool(out[14])}


# HONK_CONV2D_TRAIN_PLAN_* / HONK_MAXPOOL2D_BWD_PLAN_* of include/honk_hip.h, in order
CONV2D_TRAIN_PLAN_FIELDS = ("M", "tn", "tk", "S", "mper", "dgrad_k", "dgrad_ktab", "dgrad_wf_aligned",
                            "dgrad_grid_x", "dgrad_pad_blocks", "dgrad_pad_passes", "dgrad_m")
MAXPOOL2D_BWD_PLAN_FIELDS = ("blocks", "passes")


def conv2d_train_plan(batch: int, cin: int, h: int, w: int, cout: int, kh: int, kw: int, sh: int = 1, sw: int = 1):
    """honk_conv2d_train_plan: how honk_conv2d_wgrad_f32 and (at stride 1; zeros otherwise)
    honk_conv2d_dgrad_f32 run one conv shape, as a dict over CONV2D_TRAIN_PLAN_FIELDS (the
    two flags as bool).  Host-only; a Linear of a [B, K] input with N outputs is
    (B, K, 1, 1, N, 1, 1)."""
    n = len(CONV2D_TRAIN_PLAN_FIELDS)
    out = (ctypes.c_int64 * n)()
    rc = load().honk_conv2d_train_plan(int(batch), int(cin), int(h), int(w), int(cout), int(kh), int(kw), int(sh),
                                       int(sw), out, n)
    if rc != n:
        check(rc if rc < 0 else -1, "honk_conv2d_train_plan")
    p = dict(zip(CONV2D_TRAIN_PLAN_FIELDS, (int(v) for v in out)))
    p["dgrad_ktab"], p["dgrad_wf_aligned"] = bool(p["dgrad_ktab"]), bool(p["dgrad_wf_aligned"])
    return p


def maxpool2d_bwd_plan(batch: int, c: int, h: int, w: int, kh: int, kw: int):
    """honk_maxpool2d_bwd_plan: dict(blocks, passes) of honk_maxpool2d_bwd_f32's grid-stride
    loop.  Host-only."""
    n = len(MAXPOOL2D_BWD_PLAN_FIELDS)
    out = (ctypes.c_int64 * n)()
    rc = load().honk_maxpool2d_bwd_plan(int(batch), int(c), int(h), int(w), int(kh), int(kw), out, n)
    if rc != n:
        check(rc if rc < 0 else -1, "honk_maxpool2d_bwd_plan")
    return dict(zip(MAXPOOL2D_BWD_PLAN_FIELDS, (int(v) for v in out)))
