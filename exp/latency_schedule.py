"""What the latency schedule of the res15 forward buys at small batches (one GPU,
cuda:0), on the protocol of exp/ordered_latency.py:

    python exp/latency_schedule.py [--batches 1 8 64 256] [--reps 5] [--calls 300]

Per batch: wall time per call of --calls back-to-back stream-ordered forwards with the stream
drained once at the end, eager and as a graph replay, for
  throughput    the default schedule (pairs + last-layer kernel: a workgroup owns whole clips)
  all_band      the same under HONK_RES_KERNEL=w (every layer on block16w_kernel's row bands)
  latency       honk_schedule = "latency" (skipped on a tree without it: the parent commit)
each warmed up, --reps windows each, the modes alternated inside every repetition; and
latency with the f16x2 admission off (what the empty re-run round costs).  Every mode's
logits are checked equal to the throughput schedule's first.  Prints one JSON line (median,
min, max per figure, microseconds per call)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def stat(v):
    return dict(median=round(statistics.median(v) * 1e6, 1), min=round(min(v) * 1e6, 1), max=round(max(v) * 1e6, 1))


def timed(fn, n):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 64, 256])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=300)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    m = bench.bench_model("res15", dev)
    has_latency = hasattr(m, "honk_schedule")
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    out = {"model": "res15", "device": torch.cuda.get_device_name(0), "reps": a.reps, "calls": a.calls,
           "has_latency": has_latency, "us_per_call": {}}
    # mode -> (environment, honk_schedule)
    modes = {"throughput": ({}, "throughput"), "all_band": ({"HONK_RES_KERNEL": "w"}, "throughput")}
    if has_latency:
        modes["latency"] = ({}, "latency")
        modes["latency_no_admission"] = ({"HONK_F16X2_RERUN": "0"}, "latency")

    def enter(k):
        env, sched = modes[k]
        for v in ("HONK_RES_KERNEL", "HONK_F16X2_RERUN"):
            os.environ.pop(v, None)
        os.environ.update(env)
        if has_latency:
            m.honk_schedule = sched
        m.honk_stream_ordered = True

    with torch.no_grad():
        m(bench.mfcc_like(8, dev, g))  # the policy's probe, once
        for B in a.batches:
            xb = bench.mfcc_like(B, dev, g)
            fns, ref = {}, None
            for k in modes:
                enter(k)
                y = m(xb).clone()
                assert m.honk_last_precision == "f16x2" and int(m.honk_last_rerun_dev) == 0, k
                ref = y if ref is None else ref
                assert torch.equal(y, ref) or k == "all_band", k  # (all_band's last layer sums in another order)
                fns[k + "_eager"] = (k, lambda: m(xb))
                cap = m.honk_capture(xb)
                assert torch.equal(cap.replay(xb), y), k
                fns[k + "_graph"] = (k, lambda cap=cap: cap.replay(xb))
            t = {f: [] for f in fns}
            for f, (k, fn) in fns.items():
                enter(k)
                timed(fn, 20)
            for _ in range(a.reps):
                for f, (k, fn) in fns.items():
                    enter(k)
                    t[f].append(timed(fn, a.calls))
            out["us_per_call"][f"batch_{B}"] = {f: stat(v) for f, v in t.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
