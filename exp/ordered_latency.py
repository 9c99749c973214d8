"""What the stream-ordered res15 forward costs and buys (one GPU, cuda:0).

    python exp/ordered_latency.py [--batch 131072] [--reps 5] [--calls 300]

1. The bench shape (res15, --batch MFCC-like clips, nothing flagged): step time of the
   synchronous forward, of the ordered one at the default capacity (every re-run round
   enqueued, all of them empty) and at a capacity of one round -- alternating, --reps timed
   steps each after a warm-up of every mode, host clock around a device synchronise.
2. Batch 1 and 8: per-call wall time of --calls back-to-back calls with the stream drained
   once at the end -- synchronous eager, ordered eager, graph replay -- --reps windows each,
   alternating; and the host's share of it (the time until the last call returned).
Prints one JSON line (median, min, max per figure)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from honk_amd import _native  # noqa: E402


def stat(v, scale=1.0):
    return dict(median=round(statistics.median(v) * scale, 3), min=round(min(v) * scale, 3),
                max=round(max(v) * scale, 3))


def timed(fn, n=1, host=None):
    """Seconds per call of n calls, the device drained once at the end; host (a list):
    gets the seconds per call the host spent before that drain (its enqueue time)."""
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    th = time.perf_counter()
    torch.cuda.synchronize()
    if host is not None:
        host.append((th - t) / n)
    return (time.perf_counter() - t) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=131072)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=300)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    m = bench.bench_model("res15", dev)
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    out = {"model": "res15", "device": torch.cuda.get_device_name(0), "reps": a.reps}

    def mode(ordered, cap=None):
        m.honk_stream_ordered, m.honk_rerun_capacity = ordered, cap

    with torch.no_grad():
        # 1. the bench shape
        x = bench.mfcc_like(a.batch, dev, g)
        rc = int(_native.load().honk_res_rerun_clips(m._desc(101, 40, "f16x2"), a.batch))
        modes = {"sync": (False, None), "ordered": (True, None), "ordered_cap_one_round": (True, rc)}
        ref = None
        for k, (o, c) in modes.items():  # warm-up of every mode; same logits, nothing flagged
            mode(o, c)
            y = m(x)
            assert m.honk_last_precision == "f16x2"
            flagged = int(m.honk_last_rerun_dev) if o else m.honk_last_rerun
            assert flagged == 0, (k, flagged)
            ref = y.clone() if ref is None else ref
            assert torch.equal(y, ref), k
        t = {k: [] for k in modes}
        for _ in range(a.reps):
            for k, (o, c) in modes.items():
                mode(o, c)
                t[k].append(timed(lambda: m(x)))
        out["bench_shape"] = {"batch": a.batch, "rerun_clips_per_round": rc, "rounds_default": -(-a.batch // rc),
                              "step_ms": {k: stat(v, 1e3) for k, v in t.items()},
                              "clips_per_s": {k: round(a.batch / statistics.median(v)) for k, v in t.items()}}
        del x, y, ref
        # 2. small batches
        out["small_batch_us_per_call"], out["small_batch_host_us_per_call"] = {}, {}
        for B in (1, 8):
            xb = bench.mfcc_like(B, dev, g)
            mode(False)
            m(xb)
            cap = m.honk_capture(xb)
            fns = {"sync_eager": (False, lambda: m(xb)), "ordered_eager": (True, lambda: m(xb)),
                   "graph_replay": (False, lambda: cap.replay(xb))}
            t, th = {k: [] for k in fns}, {k: [] for k in fns}
            for k, (o, f) in fns.items():
                mode(o)
                timed(f, 20)
            for _ in range(a.reps):
                for k, (o, f) in fns.items():
                    mode(o)
                    t[k].append(timed(f, a.calls, th[k]))
            out["small_batch_us_per_call"][f"batch_{B}"] = {k: stat(v, 1e6) for k, v in t.items()}
            out["small_batch_host_us_per_call"][f"batch_{B}"] = {k: stat(v, 1e6) for k, v in th.items()}
        mode(False)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
