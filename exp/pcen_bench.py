"""The PCEN front end next to the MFCC front end on one GPU (cuda:0; DESIGN.md §3, "PCEN").

    python exp/pcen_bench.py [--batch 4096] [--reps 9] [--inner 5] [--seconds 60]

Device time (events around --inner back-to-back calls, divided by --inner) of compute_pcen_batch
and compute_mfccs_batch at [batch, 16000], on the fused / MFMA route and on the long / VALU route
(HONK_MFCC_VALU=1), and of the long PCEN route on one recording of --seconds.  Every route is warmed
up first; then --reps timed rounds, the routes alternating inside a round.  Prints one JSON line
(median, min, max per figure, in ms)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from honk_amd.audio import AudioPreprocessor  # noqa: E402


def device_timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def stat(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=4096)
    p.add_argument("--reps", type=int, default=9)
    p.add_argument("--inner", type=int, default=5)
    p.add_argument("--seconds", type=int, default=60)
    a = p.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    assert a.reps >= 5
    dev = torch.device("cuda:0")
    ap = AudioPreprocessor()
    g = torch.Generator(device="cpu").manual_seed(0)
    pcm = (torch.randn(a.batch, 16000, generator=g) * 0.1).to(dev)
    rec = (torch.randn(1, 16000 * a.seconds, generator=g) * 0.1).to(dev)

    def route(fn, valu):
        def run():
            if valu:
                os.environ["HONK_MFCC_VALU"] = "1"
            try:
                return fn()
            finally:
                os.environ.pop("HONK_MFCC_VALU", None)
        return run

    fns = {
        "mfcc_mfma": route(lambda: ap.compute_mfccs_batch(pcm), False),
        "pcen_fused": route(lambda: ap.compute_pcen_batch(pcm), False),
        "mfcc_valu": route(lambda: ap.compute_mfccs_batch(pcm), True),
        "pcen_long": route(lambda: ap.compute_pcen_batch(pcm), True),
        "pcen_long_recording": route(lambda: ap.compute_pcen_batch(rec), False),
    }
    for f in fns.values():  # warm-up: code objects, the tables, the allocator's blocks
        device_timed(f, 2)
    t = {k: [] for k in fns}
    for _ in range(a.reps):
        for k, f in fns.items():
            t[k].append(device_timed(f, a.inner))
    out = {"device": torch.cuda.get_device_name(0), "batch": a.batch, "reps": a.reps, "inner": a.inner,
           "recording_seconds": a.seconds, "recording_frames": 1 + 16000 * a.seconds // 160,
           "ms": {k: stat(v) for k, v in t.items()}}
    out["pcen_fused_over_mfcc_mfma"] = round(statistics.median(t["pcen_fused"]) / statistics.median(t["mfcc_mfma"]), 4)
    d = (fns["pcen_fused"]() - fns["pcen_long"]()).abs().max().item()
    out["max_abs_fused_minus_long"] = d
    print(json.dumps(out))


if __name__ == "__main__":
    main()
