"""What the latency schedule of the cnn forward buys at small batches (one GPU,
cuda:0), on the protocol of exp/latency_schedule.py:

    python exp/cnn_latency.py [--batches 1 2 4 ...] [--reps 5] [--calls 300] [--slices 512 1024 ...]

Per model (cnn-trad-pool2 in f32 and bf16x3, cnn-one-fstride4 in bf16x3) and batch (default 1, 2,
4, ..., 128 and CU count - 1): wall time per call of --calls back-to-back forwards with the
stream drained once at the end, eager and as a graph replay, for
  throughput    honk_cnn_forward (a workgroup owns whole clips)
  latency       honk_schedule = "latency" (skipped on a tree without it: the parent commit, so
                the same script gives the baseline)
each warmed up, --reps windows each, the modes alternated inside every repetition.  --slices
adds, at batch 1, the latency schedule under each HONK_CNN_SPLITK_SLICE (the slice-length sweep).
Before anything is timed the latency schedule's conv features are checked equal to the
throughput schedule's and its logits within 1e-4 (relative to the largest logit past 1).  The
graph is captured here with torch.cuda.CUDAGraph, so that the baseline has one too.  Prints one
JSON line (median, min, max per figure, microseconds per call)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from honk_amd import _native  # noqa: E402

MODELS = (("cnn-trad-pool2", "f32"), ("cnn-trad-pool2", "bf16x3"), ("cnn-one-fstride4", "bf16x3"))
SLICE_ENV = "HONK_CNN_SPLITK_SLICE"


def stat(v):
    return dict(median=round(statistics.median(v) * 1e6, 1), min=round(min(v) * 1e6, 1), max=round(max(v) * 1e6, 1))


def timed(fn, n):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n


def capture(m, xb):
    """(replay function, static output) of the forward as it is scheduled now."""
    static_x = xb.clone()
    m(static_x)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m(static_x)
    return graph.replay, out


def features(m, prec, xb, latency):
    lib = _native.load()
    d = _native.CnnDesc(**m._honk_desc, precision=_native.PRECISIONS[prec])
    B = xb.shape[0]
    first = m.lin if hasattr(m, "lin") else m.dnn1 if m.tf_variant and hasattr(m, "dnn1") else m.output
    need = lib.honk_cnn_latency_workspace_bytes(ctypes.byref(d), B)
    ws = torch.empty(need, dtype=torch.uint8, device=xb.device)
    out = torch.empty(B, first.in_features, device=xb.device)
    ts = [t.detach().contiguous() if t is not None else None for t in m._native_tensors()]
    _native.check(lib.honk_cnn_features_f32(ctypes.byref(d), _native.ptr_array(ts), xb.data_ptr(), out.data_ptr(), B,
                                            ws.data_ptr(), need, _native.stream_handle(xb.device), int(latency)),
                  "honk_cnn_features_f32")
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--slices", type=int, nargs="*", default=[])
    ap.add_argument("--models", nargs="+", default=None, help="name:precision, default all three")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    batches = a.batches or [1, 2, 4, 8, 16, 32, 64, 128, cus - 1]
    models = [tuple(s.split(":")) for s in a.models] if a.models else MODELS
    os.environ.pop(SLICE_ENV, None)
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    out = {"device": torch.cuda.get_device_name(0), "cus": cus, "reps": a.reps, "calls": a.calls, "us_per_call": {}}
    with torch.no_grad():
        for name, prec in models:
            m = bench.bench_model(name, dev)
            m.honk_precision = prec
            has_latency = hasattr(m, "honk_schedule")
            out["has_latency"] = has_latency
            # mode -> (honk_schedule, slice length or None)
            modes = {"throughput": ("throughput", None)}
            if has_latency:
                modes["latency"] = ("latency", None)

            def enter(k, modes=modes):
                sched, sl = modes[k]
                os.environ.pop(SLICE_ENV, None)
                if sl:
                    os.environ[SLICE_ENV] = str(sl)
                if has_latency:
                    m.honk_schedule = sched

            for B in batches:
                mm = dict(modes)
                if has_latency and B == 1 and name == "cnn-trad-pool2":
                    mm.update({f"latency_slice_{sl}": ("latency", sl) for sl in a.slices})
                xb = bench.mfcc_like(B, dev, g)
                fns, ref = {}, None
                for k in mm:
                    enter(k, mm)
                    y = m(xb).clone()
                    if ref is None:
                        ref = y
                    bar = 1e-4 * max(1.0, float(ref.abs().max()))
                    assert float((y - ref).abs().max()) <= bar, (name, prec, B, k, float((y - ref).abs().max()))
                    if k != "throughput":
                        assert torch.equal(features(m, prec, xb, 1), features(m, prec, xb, 0)), (name, prec, B, k)
                    fns[k + "_eager"] = (k, lambda: m(xb))
                    replay, static_out = capture(m, xb)
                    replay()
                    torch.cuda.synchronize()
                    assert torch.equal(static_out, y), (name, prec, B, k)
                    fns[k + "_graph"] = (k, replay)
                t = {f: [] for f in fns}
                for f, (k, fn) in fns.items():
                    enter(k, mm)
                    timed(fn, 20)
                for _ in range(a.reps):
                    for f, (k, fn) in fns.items():
                        enter(k, mm)
                        t[f].append(timed(fn, a.calls))
                out["us_per_call"].setdefault(f"{name}:{prec}", {})[f"batch_{B}"] = {f: stat(v) for f, v in t.items()}
                enter("throughput", mm)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
