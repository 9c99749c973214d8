"""Drop-in model registry and modules: the call surface of /root/reference/utils/model.py.

Same names, same config dicts, same constructor RNG consumption, same
state_dict keys/shapes/dtypes as the reference, so ``utils/train.py`` and
``service.py``-style callers work unchanged:

* ``ConfigType``, ``find_model``, ``find_config``, ``_configs``   (model.py:33-62, 381-414)
* ``truncated_normal``                                             (model.py:64-70)
* ``SerializableModule.save/load``                                 (model.py:72-80)
* ``SpeechResModel``                                               (model.py:82-121)
* ``SpeechModel``                                                  (model.py:123-205)

Forward dispatch:

* eval mode on a ROCm (``cuda``) tensor -> the hand-written gfx950 kernels in
  ``libhonk_hip.so`` (``honk_res_forward`` / ``honk_cnn_forward``).  If the
  extension is missing this raises; there is no silent fallback.
* CPU tensors, or training mode (autograd) -> the same PyTorch module ops the
  reference runs (the reference is pure PyTorch; this keeps ``--no_cuda``
  evaluation and ``train()`` working); on ROCm tensors in training mode the
  stem (conv0 + relu + avg-pool), the block convs (every dilation) and each
  block's relu / residual / train-mode BatchNorm run on the native training
  kernels (``honk_amd/conv3x3.py``), and so do SpeechModel's relu(conv) layers
  and max-pools (``honk_amd/cnn_train.py``) and both families' head: the spatial
  mean and the Linear layers (``honk_amd/head_train.py``; the loss is
  ``head_train.CrossEntropyLoss``); dropout stays PyTorch's own op (its RNG).
"""
from __future__ import annotations

import os
import warnings
from enum import Enum

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _native
from . import cnn_train as _cnn_train
from . import head_train as _head
from . import conv3x3 as _conv3x3
from . import syncbn as _syncbn


class ConfigType(Enum):
    CNN_TRAD_POOL2 = "cnn-trad-pool2"  # default full model (TF variant)
    CNN_ONE_STRIDE1 = "cnn-one-stride1"  # default compact model (TF variant)
    CNN_ONE_FPOOL3 = "cnn-one-fpool3"
    CNN_ONE_FSTRIDE4 = "cnn-one-fstride4"
    CNN_ONE_FSTRIDE8 = "cnn-one-fstride8"
    CNN_TPOOL2 = "cnn-tpool2"
    CNN_TPOOL3 = "cnn-tpool3"
    CNN_TSTRIDE2 = "cnn-tstride2"
    CNN_TSTRIDE4 = "cnn-tstride4"
    CNN_TSTRIDE8 = "cnn-tstride8"
    RES15 = "res15"
    RES26 = "res26"
    RES8 = "res8"
    RES15_NARROW = "res15-narrow"
    RES8_NARROW = "res8-narrow"
    RES26_NARROW = "res26-narrow"


def find_model(conf):
    """model.py:51-57 -- ``res*`` -> SpeechResModel, everything else -> SpeechModel."""
    if isinstance(conf, ConfigType):
        conf = conf.value
    if conf.startswith("res"):
        return SpeechResModel
    return SpeechModel


def find_config(conf):
    """model.py:59-62 -- returns the SHARED dict (callers such as service.py:82 mutate it)."""
    if isinstance(conf, ConfigType):
        conf = conf.value
    return _configs[conf]


def truncated_normal(tensor, std_dev=0.01):
    """model.py:64-70 -- resample |x| > 2 std until none remain (same RNG call sequence)."""
    tensor.zero_()
    tensor.normal_(std=std_dev)
    while torch.sum(torch.abs(tensor) > 2 * std_dev) > 0:
        t = tensor[torch.abs(tensor) > 2 * std_dev]
        t.zero_()
        tensor[torch.abs(tensor) > 2 * std_dev] = torch.normal(t, std=std_dev)


class SerializableModule(nn.Module):
    """model.py:72-80."""

    def __init__(self):
        super().__init__()

    def save(self, filename):
        torch.save(self.state_dict(), filename)

    def load(self, filename):
        # weights_only load: a state_dict holds tensors only
        sd = torch.load(filename, map_location=lambda storage, loc: storage, weights_only=True)
        self.load_state_dict(upgrade_state_dict(self, sd))


def upgrade_state_dict(module, sd):
    """Accept honk-models checkpoints from torch < 0.4.1 (SURVEY §7 'Old checkpoints'):
    they lack ``bn*.num_batches_tracked``; those buffers only count eval-irrelevant
    training steps, so they are filled with 0 (what BatchNorm itself does for
    version-1 state_dicts).  Any other missing/unexpected key still fails strictly."""
    own = module.state_dict()
    missing = [k for k in own if k not in sd]
    if missing and all(k.endswith("num_batches_tracked") for k in missing):
        sd = dict(sd)
        for k in missing:
            sd[k] = torch.zeros_like(own[k])
    return sd


def _native_ready(x, module):
    return x.is_cuda and not module.training


def default_precision(config):
    """The eval-forward precision a module starts with, selectable without touching the
    reference's callers: ``config.get("honk_precision")`` (an optional key, not part of
    ``_configs``), else the ``HONK_PRECISION`` environment variable, else ``"auto"`` --
    the fastest mode that holds the north star's 1e-4 logit bar for the model (res:
    ``honk_res_select_precision``, f16x2 -> bf16x3 -> f32 on the pack-time numerics
    record; cnn: bf16x3).  ``module.honk_precision`` may be set afterwards as well."""
    p = None
    try:
        p = config.get("honk_precision")
    except AttributeError:
        pass
    return p or os.environ.get("HONK_PRECISION") or "auto"


def _warn_reroute(module, requested, chosen, why):
    seen = module.__dict__.setdefault("_honk_rerouted", set())
    key = (requested, chosen, why)
    if key in seen:
        return
    seen.add(key)
    warnings.warn(f"honk_amd: {type(module).__name__} honk_precision={requested!r} runs as {chosen!r}: {why} "
                  f"(set honk_reroute = False to force {requested!r})", RuntimeWarning, stacklevel=3)


def _state_key(tensors, device):
    return (str(device),) + tuple((t.data_ptr(), t._version) for t in tensors)


class CapturedForward:
    """A captured stream-ordered forward (``SpeechResModel.honk_capture``, ``SpeechModel.honk_capture``).

    ``replay(x)`` (also ``__call__``) copies ``x`` into the graph's input buffer, replays
    the graph on the current stream and returns ``logits``: the graph's STATIC output
    tensor, which the next replay overwrites (clone it to keep a result).  ``flagged`` is
    the static 0-dim int32 device tensor holding the last replay's flagged-clip count (cnn: None).
    Nothing here synchronises."""

    def __init__(self, graph, x, logits, flagged, packed):
        self.graph, self.x, self.logits, self.flagged = graph, x, logits, flagged
        self._packed = packed  # the weights the graph reads

    def replay(self, x):
        if tuple(x.shape) != tuple(self.x.shape) or x.dtype != self.x.dtype or x.device != self.x.device:
            raise RuntimeError(f"captured for {self.x.dtype} {tuple(self.x.shape)} on {self.x.device}, got "
                               f"{x.dtype} {tuple(x.shape)} on {x.device}")
        self.x.copy_(x)
        self.graph.replay()
        return self.logits

    __call__ = replay


class SpeechResModel(SerializableModule):
    """Deep residual KWS net (res8/15/26[-narrow]); model.py:82-121."""

    def __init__(self, config):
        super().__init__()
        n_labels = config["n_labels"]
        n_maps = config["n_feature_maps"]
        self.conv0 = nn.Conv2d(1, n_maps, (3, 3), padding=(1, 1), bias=False)
        if "res_pool" in config:
            self.pool = nn.AvgPool2d(config["res_pool"])

        self.n_layers = n_layers = config["n_layers"]
        dilation = config["use_dilation"]
        if dilation:
            self.convs = [nn.Conv2d(n_maps, n_maps, (3, 3), padding=int(2 ** (i // 3)), dilation=int(2 ** (i // 3)),
                                    bias=False) for i in range(n_layers)]
        else:
            self.convs = [nn.Conv2d(n_maps, n_maps, (3, 3), padding=1, dilation=1, bias=False)
                          for _ in range(n_layers)]
        for i, conv in enumerate(self.convs):
            self.add_module("bn{}".format(i + 1), nn.BatchNorm2d(n_maps, affine=False))
            self.add_module("conv{}".format(i + 1), conv)
        self.output = nn.Linear(n_maps, n_labels)

        pool = config.get("res_pool")
        self._honk_desc = dict(n_labels=int(n_labels), n_maps=int(n_maps), n_layers=int(n_layers),
                               use_dilation=int(bool(dilation)),
                               pool_h=int(pool[0]) if pool is not None else 0,
                               pool_w=int(pool[1]) if pool is not None else 0)
        self._honk_packed = None
        self._honk_key = None
        # the eval forward's precision (honk_amd/_native.PRECISIONS or "auto"): "f32" (fp32
        # MFMA), "bf16x3" / "f16x2" (1e-4 logit parity where the pack-time numerics record
        # admits them -- honk_res_select_precision -- else rerouted with a warning), "bf16"
        # (top-1 parity), "auto" (the fastest of f16x2 / bf16x3 / f32 that holds 1e-4);
        # default: default_precision(config)
        self.honk_precision = default_precision(config)
        # False: run honk_precision's kernels even where the policy would reroute them
        # (kernel tests of the f16x2 path on the pooled maps)
        self.honk_reroute = True
        # training on ROCm tensors: block convs on the gfx950 kernels (False: MIOpen)
        self.honk_native_train = True
        # True: the eval forward through honk_res_forward_ordered -- no host read of the
        # f16x2 admission's flagged-clip count, so the call only enqueues work (an
        # asynchronous forward, capturable: honk_capture).  The count stays on the device
        # (honk_last_rerun_dev, a 0-dim int32 tensor; honk_last_rerun is then None), and the
        # bf16x3 re-run takes up to honk_rerun_capacity flagged clips (None: the batch), the
        # ones past it keeping their f16x2 logits.
        self.honk_stream_ordered = False
        self.honk_rerun_capacity = None
        self.honk_last_rerun_dev = None
        # "throughput": the schedule planned for large batches (a workgroup owns whole clips or
        # tall row bands).  "latency": honk_res_forward_latency -- batches of fewer clips than the
        # device has CUs run every block layer split over all CUs (the same logits bit for bit;
        # larger batches run the throughput schedule); implies the stream-ordered contract above.
        self.honk_schedule = "throughput"

    # -- reference forward (CPU tensors / training mode): model.py:104-121 --
    # native_convs: training on a ROCm tensor runs the stem (conv0 + relu + pool) on
    # honk_res_stem_*, the block convs (conv1..convN) on honk_conv3x3_f32 /
    # honk_conv3x3_wgrad_f32 where they cover the shape (any dilation, 19 or 45 maps)
    # and each block's relu / residual / train-mode BatchNorm on honk_res_tail_*
    # (honk_amd/conv3x3.py), the mean and the Linear on honk_amd/head_train.py
    def _torch_forward(self, x, native_convs=False):
        phase = "training" if self.training else "the eval forward"
        x_in, x = x, x.unsqueeze(1)
        box_in = None
        for i in range(self.n_layers + 1):
            conv = getattr(self, "conv{}".format(i))
            pool = getattr(self, "pool", None)
            if native_convs and i == 0 and _conv3x3.stem_supported(x_in, conv, pool):
                # conv0, relu and the avg-pool as one native stem
                x = old_x = _conv3x3.stem(x_in, conv, pool)
                continue
            if native_convs and i == 0:
                _conv3x3.warn_fallback(self, "the stem (conv0 + relu + pool)", phase)
            if native_convs and i > 0 and not _conv3x3.supported(x, conv):
                _conv3x3.warn_fallback(self, f"the block convs ({conv.weight.shape[0]} maps, "
                                             f"{tuple(x.shape[2:])} map, dilation {conv.dilation[0]})", phase)
            if native_convs and i > 0 and _conv3x3.supported(x, conv) and \
                    _conv3x3.bn_supported(x, getattr(self, "bn{}".format(i))) and \
                    (not _syncbn.active() or _conv3x3.stats_supported(x, conv.dilation[0])):
                # conv, then relu / residual add / train BatchNorm as one fused tail
                # statistics boxes: the tail's BatchNorm sums come from this conv's epilogue
                # (forward) and from the next layer's input-gradient conv (backward)
                d = conv.dilation[0]
                box = {}
                old = old_x if i % 2 == 0 else None
                h = _conv3x3.conv3x3(x, conv.weight, d, old=old, box_out=box, box_in=box_in)
                if box_in is not None and "fold" in box_in:
                    # the tail below folded its BatchNorm for this conv, which did not take it:
                    # x is a placeholder, so stop rather than compute from it
                    raise RuntimeError("honk_amd: a folded BatchNorm was not consumed by the next conv")
                bn = getattr(self, "bn{}".format(i))
                # the BatchNorm goes into the next block's conv when that conv takes it
                # (the last block's output feeds the head: materialized)
                nxt = getattr(self, "conv{}".format(i + 1), None) if i < self.n_layers else None
                fold = nxt is not None and _conv3x3.supported(h, nxt) and \
                    _conv3x3.bn_supported(h, getattr(self, "bn{}".format(i + 1))) and \
                    _conv3x3.fold_supported(h, nxt.dilation[0])
                if i % 2 == 0:
                    keep = i + 2 <= self.n_layers  # old_x is read again by layer i + 2
                    out = _conv3x3.res_tail(h, old_x, bn, keep_s=keep, box=box, fold=fold)
                    x, old_x = out if keep else (out, None)
                else:
                    x = _conv3x3.res_tail(h, None, bn, box=box, fold=fold)
                box_in = box
                continue
            box_in = None
            if native_convs and i > 0 and _conv3x3.supported(x, conv):
                y = F.relu(_conv3x3.conv3x3(x, conv.weight, conv.dilation[0]))
            else:
                y = F.relu(conv(x))
            if i == 0:
                if hasattr(self, "pool"):
                    y = self.pool(y)
                old_x = y
            if i > 0 and i % 2 == 0:
                x = y + old_x
                old_x = x
            else:
                x = y
            if i > 0:
                bn = getattr(self, "bn{}".format(i))
                if native_convs and _conv3x3.bn_supported(x, bn):
                    x = _conv3x3.batch_norm_train(x, bn)
                else:
                    if native_convs and bn.training:
                        _conv3x3.warn_fallback(self, "train-mode BatchNorm", phase)
                    x = _syncbn.batch_norm(x, bn) if (_syncbn.active() and bn.training) else bn(x)
        if native_convs and _head.supported(x):
            return _head.linear(_head.spatial_mean(x), self.output)
        x = x.view(x.size(0), x.size(1), -1)  # shape: (batch, feats, o3)
        x = torch.mean(x, 2)
        return self.output(x)

    # -- native gfx950 path ------------------------------------------------------
    def _pack_tensors(self):
        L = self.n_layers
        ts = [self.conv0.weight]
        ts += [getattr(self, f"conv{i}").weight for i in range(1, L + 1)]
        for i in range(1, L + 1):
            bn = getattr(self, f"bn{i}")
            ts += [bn.running_mean, bn.running_var]
        ts += [self.output.weight, self.output.bias]
        return ts

    def _desc(self, height, width, precision=None):
        p = precision or self.honk_precision
        if p == "auto":
            p = "f32"
        if p not in _native.PRECISIONS:
            raise ValueError(f"honk_precision must be 'auto' or one of {sorted(_native.PRECISIONS)}")
        return _native.ResDesc(height=height, width=width, precision=_native.PRECISIONS[p], **self._honk_desc)

    def _packed(self, x):
        lib = _native.load()
        ts = self._pack_tensors()
        key = _state_key(ts, x.device)
        if self._honk_packed is not None and self._honk_key == key:
            return self._honk_packed
        for t in ts:
            if t.device != x.device or t.dtype != torch.float32:
                raise RuntimeError(f"honk_amd: parameters must be float32 on {x.device} (got {t.dtype} on {t.device})")
        ts = [t.detach().contiguous() for t in ts]
        desc = self._desc(x.shape[1], x.shape[2], "f32")  # one layout for every precision
        n = lib.honk_res_packed_floats(desc)
        if n == 0:
            _native.check(-1, "honk_res_packed_floats")
        packed = torch.empty(n, dtype=torch.float32, device=x.device)
        arr = _native.ptr_array(ts)
        _native.check(lib.honk_res_pack(desc, arr, len(ts), packed.data_ptr(), _native.stream_handle(x.device)),
                      "honk_res_pack")
        self._honk_packed, self._honk_key = packed, key
        self._honk_keep = ts  # keep contiguous copies alive until the pack kernels ran
        self._honk_select = {}
        return packed

    def honk_numerics(self, x):
        """The pack-time numerics record (HONK_NUM_*: the f16x2 scale, range, rho, ...)
        of this model for inputs shaped like ``x`` (a ROCm tensor)."""
        with torch.cuda.device(x.device):
            packed = self._packed(x)
            return _native.res_numerics(self._desc(x.shape[1], x.shape[2], "f32"), packed, x.device)[0]

    def _run_precision(self, x):
        """The precision the eval forward runs: honk_precision, or where that is auto /
        f16x2 / bf16x3 (and honk_reroute), the library's policy on the numerics record
        (once per pack; a rerouted explicit request warns once)."""
        req = self.honk_precision
        if req != "auto" and req not in _native.PRECISIONS:
            raise ValueError(f"honk_precision must be 'auto' or one of {sorted(_native.PRECISIONS)}")
        if req in ("f32", "bf16") or (req != "auto" and not self.honk_reroute) or x.dim() != 3:
            return "f32" if req == "auto" else req
        if self._native_fits(x, "f32") is not None:
            # beyond the packed kernels (e.g. more than 64 maps): forward() runs the
            # layer-level fp32 kernels; there is no packed buffer to read a record from
            return "f32"
        with torch.cuda.device(x.device):
            packed = self._packed(x)
            key = (req, x.shape[1], x.shape[2])
            sel = self._honk_select.get(key)
            if sel is None:
                desc = self._desc(x.shape[1], x.shape[2], "f32")
                _, rec = _native.res_numerics(desc, packed, x.device)
                prec, note = _native.res_select_precision(desc, rec, req)
                if prec in ("f16x2", "bf16x3"):
                    prec, note = self._probe(x, prec, note)
                sel = self._honk_select[key] = (prec, note)
        prec, note = sel
        if req != "auto" and prec != req:
            _warn_reroute(self, req, prec, note)
        return prec

    # the measured check behind the policy: the reduced modes' logits on PROBE_CLIPS clips
    # spread over the first batch against the fp32 kernels', within PROBE_TOL of the larger
    # of 1 and the logits' size -- half the 1e-4 bar, ABSOLUTE while |logit| <= 1 and
    # relative beyond (large logits carry the fp32 reference's own rounding: at |logit| ~
    # 1e3 fp32 itself differs from float64 by more than 1e-4); a mode that misses falls to
    # the next (f16x2 -> bf16x3 -> f32).  Once per pack and input shape; a synchronisation.
    # This is the model-level check (its conditioning); every batch is admitted clip by
    # clip on top of it (honk_res_forward: out-of-calibration clips re-run in bf16x3).
    PROBE_CLIPS = 8
    PROBE_TOL = 5e-5

    def _probe(self, x, prec, note):
        B = x.shape[0]
        idx = torch.linspace(0, B - 1, min(B, self.PROBE_CLIPS), device=x.device).round().long().unique()
        xs = x[idx]
        ref = self._native_forward(xs, "f32")
        scale = max(1.0, float(torch.nan_to_num(ref, nan=0.0, posinf=0.0, neginf=0.0).abs().max()))
        order = ["f16x2", "bf16x3"] if prec == "f16x2" else ["bf16x3"]
        for p in order:
            out = self._native_forward(xs, p)
            same_nonfinite = torch.isfinite(out) == torch.isfinite(ref)
            both = torch.isfinite(out) & torch.isfinite(ref)
            err = float((out - ref).abs()[both].max()) if bool(both.any()) else 0.0
            if bool(same_nonfinite.all()) and err <= self.PROBE_TOL * scale:
                return p, note
            note = (f"{note}; " if note else "") + (f"{p} measured {err:.2e} from the fp32 kernels on this "
                                                    f"model's first {xs.shape[0]} clips (bound "
                                                    f"{self.PROBE_TOL * scale:.2e})")
        return "f32", note

    def _native_forward(self, x, precision=None):
        if x.dim() != 3:
            raise RuntimeError(f"SpeechResModel expects [B, H, W] input, got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise RuntimeError(f"expected float32 input, got {x.dtype}")
        x = x.contiguous()
        lib = _native.load()
        with torch.cuda.device(x.device):
            packed = self._packed(x)
            desc = self._desc(x.shape[1], x.shape[2], precision)
            self.honk_last_precision = precision or self.honk_precision
            B = x.shape[0]
            out = torch.empty(B, self._honk_desc["n_labels"], dtype=torch.float32, device=x.device)
            if self.honk_schedule not in ("throughput", "latency"):
                raise ValueError("honk_schedule must be 'throughput' or 'latency'")
            latency = self.honk_schedule == "latency"
            ordered = self.honk_stream_ordered or latency
            if ordered:
                self.honk_last_rerun = None
                self.honk_last_rerun_dev = torch.zeros((), dtype=torch.int32, device=x.device)
            if B == 0:
                if not ordered:
                    self.honk_last_rerun = 0  # (not the previous batch's count)
                return out
            ws_query = "honk_res_latency_workspace_bytes" if latency else "honk_res_workspace_bytes"
            ws_bytes = getattr(lib, ws_query)(desc, B)
            if ws_bytes == 0:
                _native.check(-1, ws_query)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
            if ordered:
                cap = self.honk_rerun_capacity
                entry = "honk_res_forward_latency" if latency else "honk_res_forward_ordered"
                _native.check(getattr(lib, entry)(desc, packed.data_ptr(), x.data_ptr(), out.data_ptr(), B,
                                                  ws.data_ptr(), ws_bytes, _native.stream_handle(x.device),
                                                  0 if cap is None else int(cap),
                                                  self.honk_last_rerun_dev.data_ptr()),
                              entry)
                return out
            _native.check(lib.honk_res_forward(desc, packed.data_ptr(), x.data_ptr(), out.data_ptr(), B,
                                               ws.data_ptr(), ws_bytes, _native.stream_handle(x.device)),
                          "honk_res_forward")
            # f16x2: the clips the per-clip admission re-ran in bf16x3 (honk_res_rerun_count)
            self.honk_last_rerun = int(lib.honk_res_rerun_count())
        return out

    def honk_capture(self, x_example):
        """Capture the stream-ordered eval forward for inputs shaped like ``x_example`` (a
        float32 ROCm tensor [B, H, W]; eval mode) in a ``torch.cuda.CUDAGraph`` and return
        a ``CapturedForward``: ``replay(x) -> logits``.

        One eager forward runs first: the once-per-pack synchronisations (weight pack,
        numerics record, the precision policy's probe, the CU-count query) happen there,
        outside the capture.  The capture itself is the launches of
        ``honk_res_forward_ordered`` (``honk_schedule = "latency"``: ``honk_res_forward_latency``)
        on the capture stream, with ``honk_rerun_capacity`` as it is now; the flagged-clip count
        is read by the kernels at every replay, so one graph serves batches with any number of
        out-of-calibration clips.  A later change of the weights, ``honk_precision``,
        ``honk_schedule`` or ``honk_rerun_capacity`` needs a new capture."""
        if self.training:
            raise RuntimeError("honk_capture needs eval mode (module.eval())")
        if not (torch.is_tensor(x_example) and x_example.is_cuda and x_example.dim() == 3
                and x_example.dtype == torch.float32 and x_example.shape[0] > 0):
            raise RuntimeError("honk_capture expects a non-empty float32 [B, H, W] tensor on a ROCm device")
        prev = self.honk_stream_ordered
        self.honk_stream_ordered = True
        try:
            with torch.no_grad(), torch.cuda.device(x_example.device):
                static_x = x_example.detach().clone().contiguous()
                why = self._native_fits(static_x, self._run_precision(static_x))
                if why is not None:
                    raise RuntimeError(f"honk_capture: the packed forward does not take this model ({why})")
                self(static_x)
                torch.cuda.synchronize(static_x.device)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    static_out = self(static_x)
                    static_flagged = self.honk_last_rerun_dev
                packed = self._packed(static_x)
        finally:
            self.honk_stream_ordered = prev
        return CapturedForward(graph, static_x, static_out, static_flagged, packed)

    def _native_fits(self, x, precision):
        """None if the packed forward (honk_res_forward) takes this model and input shape,
        else the library's reason (host-only queries, cached per precision and map size)."""
        key = (precision, x.shape[1], x.shape[2])
        fits = self.__dict__.setdefault("_honk_fits", {})
        if key not in fits:
            lib = _native.load()
            desc = self._desc(x.shape[1], x.shape[2], precision)
            ok = lib.honk_res_packed_floats(desc) != 0 and lib.honk_res_workspace_bytes(desc, 1) != 0
            fits[key] = None if ok else lib.honk_last_error().decode(errors="replace")
        return fits[key]

    def forward(self, x):
        if _native_ready(x, self):
            prec = self._run_precision(x) if x.dim() == 3 else None
            why = self._native_fits(x, prec) if x.dim() == 3 else None
            if why is not None:
                # beyond the packed kernels' envelope (more than 64 maps in f32 / 48 in bf16,
                # maps wider than the bf16 staging plan): the same forward on the layer-level
                # kernels (native stem, block convs, mean, Linear; eval BatchNorm and the
                # residual adds as device elementwise ops), in fp32
                _conv3x3.warn_fallback(self, f"the eval forward of {tuple(x.shape[1:])} inputs in "
                                             f"{prec} ({why}): layer-level fp32 kernels instead")
                return self._torch_forward(x, native_convs=True)
            return self._native_forward(x, prec)
        return self._torch_forward(x, native_convs=x.is_cuda and self.honk_native_train)


class SpeechModel(SerializableModule):
    """TF-style KWS CNNs (cnn-trad-pool2, cnn-one-*, ...); model.py:123-205."""

    def __init__(self, config):
        super().__init__()
        n_labels = config["n_labels"]
        n_featmaps1 = config["n_feature_maps1"]

        conv1_size = config["conv1_size"]  # (time, frequency)
        conv1_pool = config["conv1_pool"]
        conv1_stride = tuple(config["conv1_stride"])
        dropout_prob = config["dropout_prob"]
        width = config["width"]
        height = config["height"]
        self.conv1 = nn.Conv2d(1, n_featmaps1, conv1_size, stride=conv1_stride)
        tf_variant = config.get("tf_variant")
        self.tf_variant = tf_variant
        if tf_variant:
            truncated_normal(self.conv1.weight.data)
            self.conv1.bias.data.zero_()
        self.pool1 = nn.MaxPool2d(conv1_pool)

        with torch.no_grad():  # shape probe, model.py:143-160 (consumes no RNG)
            x = torch.zeros(1, 1, height, width)
            x = self.pool1(self.conv1(x))
            conv_net_size = x.view(1, -1).size(1)
            last_size = conv_net_size

            desc = dict(height=int(height), width=int(width), n_labels=int(n_labels),
                        c1_out=int(n_featmaps1), c1_kh=int(conv1_size[0]), c1_kw=int(conv1_size[1]),
                        c1_sh=int(conv1_stride[0]), c1_sw=int(conv1_stride[1]),
                        p1_h=int(_pair(conv1_pool)[0]), p1_w=int(_pair(conv1_pool)[1]),
                        has_conv2=0, c2_out=0, c2_kh=0, c2_kw=0, c2_sh=1, c2_sw=1, p2_h=1, p2_w=1,
                        has_lin=0, dnn1=0, dnn2=0, dnn1_relu=int(not tf_variant))
            if "conv2_size" in config:
                conv2_size = config["conv2_size"]
                conv2_pool = config["conv2_pool"]
                conv2_stride = tuple(config["conv2_stride"])
                n_featmaps2 = config["n_feature_maps2"]
                self.conv2 = nn.Conv2d(n_featmaps1, n_featmaps2, conv2_size, stride=conv2_stride)
                if tf_variant:
                    truncated_normal(self.conv2.weight.data)
                    self.conv2.bias.data.zero_()
                self.pool2 = nn.MaxPool2d(conv2_pool)
                x = self.pool2(self.conv2(x))
                conv_net_size = x.view(1, -1).size(1)
                last_size = conv_net_size
                desc.update(has_conv2=1, c2_out=int(n_featmaps2), c2_kh=int(conv2_size[0]),
                            c2_kw=int(conv2_size[1]), c2_sh=int(conv2_stride[0]), c2_sw=int(conv2_stride[1]),
                            p2_h=int(_pair(conv2_pool)[0]), p2_w=int(_pair(conv2_pool)[1]))
        if not tf_variant:
            self.lin = nn.Linear(conv_net_size, 32)
            desc["has_lin"] = 1

        if "dnn1_size" in config:
            dnn1_size = config["dnn1_size"]
            last_size = dnn1_size
            if tf_variant:
                self.dnn1 = nn.Linear(conv_net_size, dnn1_size)
                truncated_normal(self.dnn1.weight.data)
                self.dnn1.bias.data.zero_()
            else:
                self.dnn1 = nn.Linear(32, dnn1_size)
            desc["dnn1"] = int(dnn1_size)
            if "dnn2_size" in config:
                dnn2_size = config["dnn2_size"]
                last_size = dnn2_size
                self.dnn2 = nn.Linear(dnn1_size, dnn2_size)
                if tf_variant:
                    truncated_normal(self.dnn2.weight.data)
                    self.dnn2.bias.data.zero_()
                desc["dnn2"] = int(dnn2_size)
        self.output = nn.Linear(last_size, n_labels)
        if tf_variant:
            truncated_normal(self.output.weight.data)
            self.output.bias.data.zero_()
        self.dropout = nn.Dropout(dropout_prob)
        self._honk_desc = desc
        # "f32": fp32 MFMA; "bf16x3": operands split into bf16 hi/lo pairs on the
        # bf16 MFMA pipe (same 1e-4 logit bar; tests/test_gpu_cnn_x3.py); "auto" =
        # bf16x3; default: default_precision(config)
        self.honk_precision = default_precision(config)
        self.honk_reroute = True
        # training on ROCm tensors: convs + ReLU and max-pools on the gfx950 kernels (False: MIOpen)
        self.honk_native_train = True
        # "throughput": honk_cnn_forward (a workgroup owns whole clips).  "latency":
        # honk_cnn_forward_latency -- batches of fewer clips than the device has CUs run the
        # dedicated convs split over all CUs (the conv stack bit for bit) and the long Linears
        # split over K (the same 1e-4 bar); larger batches run the throughput schedule.
        self.honk_schedule = "throughput"

    # -- reference forward (CPU tensors / training mode): model.py:186-205 --
    # native: training on a ROCm tensor runs relu(conv) and the max-pools on the
    # native training kernels (honk_amd/cnn_train.py) and the Linear layers (dnn1's
    # ReLU fused) on honk_amd/head_train.py; dropout stays PyTorch's op (its RNG stream)
    def _conv_relu(self, conv, x, native):
        if native and _cnn_train.conv_supported(x, conv):
            return _cnn_train.conv_relu(x, conv)
        if native:
            _conv3x3.warn_fallback(self, f"{tuple(conv.weight.shape)} conv")
        return F.relu(conv(x))

    def _pool(self, pool, x, native):
        if native and _cnn_train.pool_supported(x, pool):
            return _cnn_train.max_pool(x, pool)
        if native:
            _conv3x3.warn_fallback(self, f"MaxPool2d({pool.kernel_size})")
        return pool(x)

    def _torch_forward(self, x, native=False):
        x = self._conv_relu(self.conv1, x.unsqueeze(1), native)  # shape: (batch, channels, i1, o1)
        x = self.dropout(x)
        x = self._pool(self.pool1, x, native)
        if hasattr(self, "conv2"):
            x = self._conv_relu(self.conv2, x, native)  # shape: (batch, o1, i2, o2)
            x = self.dropout(x)
            x = self._pool(self.pool2, x, native)
        x = x.view(x.size(0), -1)  # shape: (batch, o3)
        lin = native and _head.supported(x)
        if hasattr(self, "lin"):
            x = _head.linear(x, self.lin) if lin else self.lin(x)
        if hasattr(self, "dnn1"):
            if lin and not self.tf_variant:
                x = _head.linear_relu(x, self.dnn1)
            else:
                x = _head.linear(x, self.dnn1) if lin else self.dnn1(x)
                if not self.tf_variant:
                    x = F.relu(x)
            x = self.dropout(x)
        if hasattr(self, "dnn2"):
            x = _head.linear(x, self.dnn2) if lin else self.dnn2(x)
            x = self.dropout(x)
        return _head.linear(x, self.output) if lin else self.output(x)

    def _native_tensors(self):
        def wb(name):
            m = getattr(self, name, None)
            return (m.weight, m.bias) if m is not None else (None, None)
        ts = []
        for name in ("conv1", "conv2", "lin", "dnn1", "dnn2", "output"):
            ts += list(wb(name))
        return ts

    def _native_forward(self, x):
        if x.dim() != 3:
            raise RuntimeError(f"SpeechModel expects [B, H, W] input, got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise RuntimeError(f"expected float32 input, got {x.dtype}")
        d = self._honk_desc
        if x.shape[1] != d["height"] or x.shape[2] != d["width"]:
            raise RuntimeError(f"input {tuple(x.shape[1:])} does not match config ({d['height']}, {d['width']})")
        x = x.contiguous()
        lib = _native.load()
        ts = self._native_tensors()
        for t in ts:
            if t is not None and (t.device != x.device or t.dtype != torch.float32):
                raise RuntimeError(f"honk_amd: parameters must be float32 on {x.device}")
        ts = [t.detach().contiguous() if t is not None else None for t in ts]
        prec = self.honk_precision
        if prec == "auto":
            prec = "bf16x3"
        elif prec == "f16x2" and self.honk_reroute:
            # the cnn path has no fp16 kernels; bf16x3 holds the same 1e-4 bar
            _warn_reroute(self, prec, "bf16x3", "SpeechModel has no f16x2 kernels")
            prec = "bf16x3"
        if prec not in ("f32", "bf16x3"):
            raise ValueError("SpeechModel.honk_precision must be 'auto', 'f32' or 'bf16x3'")
        if self.honk_schedule not in ("throughput", "latency"):
            raise ValueError("honk_schedule must be 'throughput' or 'latency'")
        latency = self.honk_schedule == "latency"
        self.honk_last_precision = prec
        desc = _native.CnnDesc(**d, precision=_native.PRECISIONS[prec])
        B = x.shape[0]
        with torch.cuda.device(x.device):
            out = torch.empty(B, d["n_labels"], dtype=torch.float32, device=x.device)
            if B == 0:
                return out
            ws_query = "honk_cnn_latency_workspace_bytes" if latency else "honk_cnn_workspace_bytes"
            entry = "honk_cnn_forward_latency" if latency else "honk_cnn_forward"
            ws_bytes = getattr(lib, ws_query)(desc, B)
            if ws_bytes == 0:
                _native.check(-1, ws_query)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
            _native.check(getattr(lib, entry)(desc, _native.ptr_array(ts), x.data_ptr(), out.data_ptr(), B,
                                              ws.data_ptr(), ws_bytes, _native.stream_handle(x.device)),
                          entry)
        return out

    def honk_capture(self, x_example):
        """Capture the eval forward for inputs shaped like ``x_example`` (a non-empty float32 ROCm
        tensor [B, H, W]; eval mode) in a ``torch.cuda.CUDAGraph`` and return a
        ``CapturedForward``: ``replay(x) -> logits`` (its ``flagged`` is None: the cnn forward has
        no admission count).

        One eager forward runs first -- the CU-count query of the schedule happens there, outside
        the capture -- then the capture records the launches of ``honk_cnn_forward``
        (``honk_schedule = "latency"``: ``honk_cnn_forward_latency``) on the capture stream.  The
        graph reads the parameter tensors in place and re-packs conv2's fragments inside every
        replay, so an in-place weight update (``load()``, an optimiser step) is seen by the next
        replay.  A NEW parameter tensor (a module moved or cast, a parameter replaced), another
        ``honk_precision`` or another ``honk_schedule`` needs a new capture."""
        if self.training:
            raise RuntimeError("honk_capture needs eval mode (module.eval())")
        if not (torch.is_tensor(x_example) and x_example.is_cuda and x_example.dim() == 3
                and x_example.dtype == torch.float32 and x_example.shape[0] > 0):
            raise RuntimeError("honk_capture expects a non-empty float32 [B, H, W] tensor on a ROCm device")
        with torch.no_grad(), torch.cuda.device(x_example.device):
            static_x = x_example.detach().clone().contiguous()
            self(static_x)
            torch.cuda.synchronize(static_x.device)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                static_out = self(static_x)
            keep = [t for t in self._native_tensors() if t is not None]  # the weights the graph reads
        return CapturedForward(graph, static_x, static_out, None, keep)

    def forward(self, x):
        if _native_ready(x, self):
            return self._native_forward(x)
        return self._torch_forward(x, native=x.is_cuda and self.honk_native_train)


def _pair(v):
    if isinstance(v, (tuple, list)):
        return (v[0], v[1])
    return (v, v)


_configs = {
    ConfigType.CNN_TRAD_POOL2.value: dict(dropout_prob=0.5, height=101, width=40, n_labels=4, n_feature_maps1=64,
        n_feature_maps2=64, conv1_size=(20, 8), conv2_size=(10, 4), conv1_pool=(2, 2), conv1_stride=(1, 1),
        conv2_stride=(1, 1), conv2_pool=(1, 1), tf_variant=True),
    ConfigType.CNN_ONE_STRIDE1.value: dict(dropout_prob=0.5, height=101, width=40, n_labels=4, n_feature_maps1=186,
        conv1_size=(101, 8), conv1_pool=(1, 1), conv1_stride=(1, 1), dnn1_size=128, dnn2_size=128, tf_variant=True),
    ConfigType.CNN_TSTRIDE2.value: dict(dropout_prob=0.5, height=101, width=40, n_labels=4, n_feature_maps1=78,
        n_feature_maps2=78, conv1_size=(16, 8), conv2_size=(9, 4), conv1_pool=(1, 3), conv1_stride=(2, 1),
        conv2_stride=(1, 1), conv2_pool=(1, 1), dnn1_size=128, dnn2_size=128),
    ConfigType.CNN_TSTRIDE4.value: dict(dropout_prob=0.5, height=101, width=40, n_labels=4, n_feature_maps1=100,
        n_feature_maps2=78, conv1_size=(16, 8), conv2_size=(5, 4), conv1_pool=(1, 3), conv1_stride=(4, 1),
        conv2_stride=(1, 1), conv2_pool=(1, 1), dnn1_size=128, dnn2_size=128),
    ConfigType.CNN_TSTRIDE8.value: dict(dropout_prob=0.5, height=101, width=40, n_labels=4, n_feature_maps1=126,
        n_feature_maps2=78, conv1_size=(16, 8), conv2_size=(5, 4), conv1_pool=(1, 3), conv1_stride=(8, 1),
        conv2_stride=(1, 1), conv2_pool=(1, 1), dnn1_size=128, dnn2_size=128),
    ConfigType.CNN_TPOOL2.value: dict(dropout_prob=0.5, height=101, width=40, n_labels=4, n_feature_maps1=94,
        n_feature_maps2=94, conv1_size=(21, 8), conv2_size=(6, 4), conv1_pool=(2, 3), conv1_stride=(1, 1),
        conv2_stride=(1, 1), conv2_pool=(1, 1), dnn1_size=128, dnn2_size=128),
    ConfigType.CNN_TPOOL3.value: dict(dropout_prob=0.5, height=101, width=40, n_labels=4, n_feature_maps1=94,
        n_feature_maps2=94, conv1_size=(15, 8), conv2_size=(6, 4), conv1_pool=(3, 3), conv1_stride=(1, 1),
        conv2_stride=(1, 1), conv2_pool=(1, 1), dnn1_size=128, dnn2_size=128),
    ConfigType.CNN_ONE_FPOOL3.value: dict(dropout_prob=0.5, height=101, width=40, n_labels=4, n_feature_maps1=54,
        conv1_size=(101, 8), conv1_pool=(1, 3), conv1_stride=(1, 1), dnn1_size=128, dnn2_size=128),
    ConfigType.CNN_ONE_FSTRIDE4.value: dict(dropout_prob=0.5, height=101, width=40, n_labels=4, n_feature_maps1=186,
        conv1_size=(101, 8), conv1_pool=(1, 1), conv1_stride=(1, 4), dnn1_size=128, dnn2_size=128),
    ConfigType.CNN_ONE_FSTRIDE8.value: dict(dropout_prob=0.5, height=101, width=40, n_labels=4, n_feature_maps1=336,
        conv1_size=(101, 8), conv1_pool=(1, 1), conv1_stride=(1, 8), dnn1_size=128, dnn2_size=128),
    ConfigType.RES15.value: dict(n_labels=12, use_dilation=True, n_layers=13, n_feature_maps=45),
    ConfigType.RES8.value: dict(n_labels=12, n_layers=6, n_feature_maps=45, res_pool=(4, 3), use_dilation=False),
    ConfigType.RES26.value: dict(n_labels=12, n_layers=24, n_feature_maps=45, res_pool=(2, 2), use_dilation=False),
    ConfigType.RES15_NARROW.value: dict(n_labels=12, use_dilation=True, n_layers=13, n_feature_maps=19),
    ConfigType.RES8_NARROW.value: dict(n_labels=12, n_layers=6, n_feature_maps=19, res_pool=(4, 3),
                                       use_dilation=False),
    ConfigType.RES26_NARROW.value: dict(n_labels=12, n_layers=24, n_feature_maps=19, res_pool=(2, 2),
                                        use_dilation=False),
}
