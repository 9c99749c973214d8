"""The /listen front end on a long recording: today's per-window route against the
strided-window kernel (one GPU, cuda:0).

    python exp/listen_bench.py [--front mfcc|pcen] [--seconds 60] [--reps 7] [--strides 500 100 10] [--out FILE]

Per stride, back to back in one process, after a warm-up of every route, --reps timed runs
each, alternating, the device synchronised around every timed region:
  (a) the front end alone -- baseline: host slicing + np.stack + upload + compute_mfccs_batch
      (TorchLabelService._model_input on list(stride(...))); new: one int16 upload +
      compute_mfccs_windows.  End to end (host clock) and the device part alone (events around
      the MFCC call on inputs already on the device).
  (b) label_batch(list(stride(...))) against label_stream, end to end, with cnn-trad-pool2
      (auto precision) and res8 (bf16) as the service's model.
--front pcen: the same protocol with a PCEN service (audio_preprocess_type="PCEN"): compute_pcen_batch
on the unfolded float windows (the per-window route) against compute_pcen_windows.
Prints one JSON line (median, min, max per figure; the frames-computed counts of
honk_mfcc_windows_plan next to the device-time ratio); --out also writes it to a file."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from honk_amd import model as hm  # noqa: E402
from honk_amd import service as hs  # noqa: E402


def stat(v, scale=1e3):
    return dict(median=round(statistics.median(v) * scale, 4), min=round(min(v) * scale, 4),
                max=round(max(v) * scale, 4))


def host_timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def device_timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3


def recording(seconds, seed=0):
    n = 16000 * seconds
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    y = 0.05 * rng.standard_normal(n)
    for f in rng.uniform(100, 3500, 6):
        y += rng.uniform(0.02, 0.2) * np.sin(2 * np.pi * f * t + rng.uniform(0, 6.3))
    return (np.clip(y, -1, 1) * 32767).astype(np.int16)


def alternate(fns, reps, timer):
    for f in fns.values():
        timer(f)
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            t[k].append(timer(f))
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=60)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--strides", type=int, nargs="+", default=[500, 100, 10])
    ap.add_argument("--front", choices=["mfcc", "pcen"], default="mfcc")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    assert a.reps >= 5
    dev = torch.device("cuda:0")
    labels = ["_silence_", "_unknown_", "command", "random"]
    torch.manual_seed(0)
    with tempfile.TemporaryDirectory() as tmp:
        fn = os.path.join(tmp, "m.pt")
        hm.SpeechModel(dict(hm.find_config("cnn-trad-pool2"), n_labels=len(labels))).save(fn)
        svc = hs.TorchLabelService(fn, labels=labels,
                                   audio_preprocess_type="PCEN" if a.front == "pcen" else "MFCCs")
    cnn = svc.model
    res8 = hm.find_model("res8")(dict(hm.find_config("res8"), n_labels=len(labels))).eval().to(dev)
    res8.honk_precision = "bf16"
    pre = svc.audio_processor
    # the two routes of the front end under test: (plan query, per-window route, strided-window route)
    plan_of, per_window, windows = {
        "mfcc": (pre.windows_plan, pre.compute_mfccs_batch, pre.compute_mfccs_windows),
        "pcen": (pre.pcen_windows_plan, pre.compute_pcen_batch, pre.compute_pcen_windows)}[a.front]
    x = recording(a.seconds)
    wav = x.tobytes()
    out = {"front": a.front, "device": torch.cuda.get_device_name(0), "seconds": a.seconds, "reps": a.reps, "strides": {}}
    for ms in a.strides:
        sb = 32 * ms
        rc, plan = plan_of(len(x), sb // 2, 16000, 0, 0)
        W = plan.windows
        rc, plan = plan_of(len(x), sb // 2, 16000, 0, W)
        assert rc == 0
        r = {"windows": W, "frames_per_window_route": W * plan.frames, "frames_computed": plan.frames_computed,
             "frames_ratio": round(W * plan.frames / plan.frames_computed, 3)}
        # (a) the front end alone
        pcm_f = torch.from_numpy(np.stack([np.frombuffer(w, np.int16) for w in hs.stride(wav, sb, 32000)])
                                 .astype(np.float32) / 32768.).to(dev)
        pcm_i = torch.from_numpy(x).to(dev)
        new = windows(pcm_i, sb // 2)
        old = per_window(pcm_f)
        r["max_abs_diff_new_vs_baseline"] = float((new - old).abs().max())
        del new, old
        t = alternate({"baseline": lambda: per_window(pcm_f),
                       "new": lambda: windows(pcm_i, sb // 2)}, a.reps, device_timed)
        r["front_end_device_ms"] = {k: stat(v) for k, v in t.items()}
        r["front_end_device_ratio"] = round(statistics.median(t["baseline"]) / statistics.median(t["new"]), 3)
        del pcm_f, pcm_i
        t = alternate({"baseline": lambda: svc._model_input(list(hs.stride(wav, sb, 32000))),
                       "new": lambda: windows(
                           torch.from_numpy(np.frombuffer(wav, np.int16).copy()).to(dev), sb // 2)},
                      a.reps, host_timed)
        r["front_end_end_to_end_ms"] = {k: stat(v) for k, v in t.items()}
        # (b) the service
        r["service_end_to_end_ms"] = {}
        for name, m in (("cnn-trad-pool2", cnn), ("res8-bf16", res8)):
            svc.model = m
            got, want = svc.label_stream(wav, ms), svc.label_batch(list(hs.stride(wav, sb, 32000)))
            assert len(got) == len(want) == W
            t = alternate({"label_batch": lambda: svc.label_batch(list(hs.stride(wav, sb, 32000))),
                           "label_stream": lambda: svc.label_stream(wav, ms)}, a.reps, host_timed)
            r["service_end_to_end_ms"][name] = {k: stat(v) for k, v in t.items()}
            r["service_end_to_end_ms"][name]["labels_differ"] = sum(g[0] != w[0] for g, w in zip(got, want))
        out["strides"][str(ms)] = r
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
