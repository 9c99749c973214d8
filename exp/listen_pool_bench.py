"""Many live streams at once: a StreamPool tick (one label_streams call: one upload, one ragged-batch
front-end call, one forward, one download) against S StreamListener.feed calls (one label_stream
round trip per stream -- the code path the pool leaves unchanged), and against a
StreamPool(device_state=True) tick (tails and finished rows resident on the device: only the new bytes
uploaded, only the new frames computed) (one GPU, cuda:0).

    python exp/listen_pool_bench.py [--streams 1 64 1024] [--ticks 100 500] [--fronts mfcc pcen]
                                    [--reps 7] [--out profiles/listen_pool_bench.json]

Per front end, tick length (ms of audio per stream per tick, the stride being the tick) and number of
streams S, back to back in one process: every stream is primed with one second, so each further tick
completes exactly one window per stream.  After a warm-up tick of every route, --reps timed ticks each,
alternating tick by tick, the device synchronised around every timed region:
  (a) end to end (host clock): StreamPool.feed({k: chunk_k}) against [listener_k.feed(chunk_k)] and
      against StreamPool(device_state=True).feed({k: chunk_k}); all sides see the same chunks;
  (b) the front end's device time alone (events; the samples already on the device): one
      compute_*_segments on the S one-second recordings against S compute_*_windows calls, and against
      one StreamBank.tick on the S new chunks of a primed bank; with the bank tick's samples_in,
      frames_computed and frames_reused.
Next to them the frame-tile workgroups: the batch plan's `tiles` and the sum of the S single-recording
calls' (each rounds its edge tile up on its own).
Prints one JSON line (median, min, max per figure, ms); --out also writes it to a file."""
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

WIN = 16000


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


def recording(n, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    y = 0.05 * rng.standard_normal(n)
    for f in rng.uniform(100, 3500, 6):
        y += rng.uniform(0.02, 0.2) * np.sin(2 * np.pi * f * t + rng.uniform(0, 6.3))
    return (np.clip(y, -1, 1) * 32767).astype(np.int16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--ticks", type=int, nargs="+", default=[100, 500])
    ap.add_argument("--fronts", nargs="+", choices=["mfcc", "pcen"], default=["mfcc", "pcen"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    assert a.reps >= 5
    dev = torch.device("cuda:0")
    labels = ["_silence_", "_unknown_", "command", "random"]
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "model": "cnn-trad-pool2", "fronts": {}}
    for front in a.fronts:
        torch.manual_seed(0)
        with tempfile.TemporaryDirectory() as tmp:
            fn = os.path.join(tmp, "m.pt")
            hm.SpeechModel(dict(hm.find_config("cnn-trad-pool2"), n_labels=len(labels))).save(fn)
            svc = hs.TorchLabelService(fn, labels=labels, audio_preprocess_type="PCEN" if front == "pcen" else "MFCCs")
        pre = svc.audio_processor
        plan_of, windows, segments = {
            "mfcc": (pre.segments_plan, pre.compute_mfccs_windows, pre.compute_mfccs_segments),
            "pcen": (pre.pcen_segments_plan, pre.compute_pcen_windows, pre.compute_pcen_segments)}[front]
        res = out["fronts"][front] = {}
        for ms in a.ticks:
            step = 16 * ms                       # samples per tick = the stride
            n_ticks = 2 * (a.reps + 1)           # a warm-up and --reps timed ticks of each route
            for S in a.streams:
                # S different streams cut from one long recording, each one second plus its ticks
                need = WIN + n_ticks * step
                base = recording(need + 37 * S, seed=S + ms)
                wavs = [base[37 * k:37 * k + need].tobytes() for k in range(S)]
                r = {}
                # the frame-tile workgroups of one tick
                off = np.arange(S + 1, dtype=np.int64) * WIN
                rc, plan, _, _ = plan_of(off, step)
                rc1, one, _, _ = plan_of(off[:2], step)
                assert rc == 0 and rc1 == 0 and plan.windows == S
                r["tiles"] = {"pool": int(plan.tiles), "per_stream_sum": S * int(one.tiles)}
                # (a) end to end
                pool = hs.StreamPool(svc, ms)
                bank_pool = hs.StreamPool(svc, ms, device_state=True)
                assert bank_pool.bank is not None
                first = bank_pool.feed({k: w[:2 * WIN] for k, w in enumerate(wavs)})
                assert all(len(first[k]) == 1 for k in range(S))
                listeners = [hs.StreamListener(svc, ms) for _ in range(S)]
                first = pool.feed({k: w[:2 * WIN] for k, w in enumerate(wavs)})
                assert all(len(first[k]) == 1 for k in range(S))
                for k, sl in enumerate(listeners):
                    assert len(sl.feed(wavs[k][:2 * WIN])) == 1
                tick = [0]

                def chunks():
                    i = 2 * WIN + 2 * step * tick[0]
                    tick[0] += 1
                    return [w[i:i + 2 * step] for w in wavs]

                def run_pool(c):
                    got = pool.feed(dict(enumerate(c)))
                    assert all(len(got[k]) == 1 for k in range(S))

                def run_loop(c):
                    for sl, b in zip(listeners, c):
                        assert len(sl.feed(b)) == 1

                def run_bank(c):
                    got = bank_pool.feed(dict(enumerate(c)))
                    assert all(len(got[k]) == 1 for k in range(S))

                t = {"pool": [], "per_stream": [], "bank": []}
                fed = []
                for rep in range(a.reps + 1):
                    c = chunks()   # (every route's streams are at the same position: the same chunks)
                    fed.append(c)
                    for name, fn_ in (("pool", run_pool), ("per_stream", run_loop), ("bank", run_bank)):
                        dt = host_timed(lambda: fn_(c))
                        if rep:
                            t[name].append(dt)
                r["end_to_end_ms"] = {k: stat(v) for k, v in t.items()}
                r["end_to_end_ratio"] = round(statistics.median(t["per_stream"]) / statistics.median(t["pool"]), 3)
                r["end_to_end_pool_over_bank"] = round(statistics.median(t["pool"]) / statistics.median(t["bank"]), 3)
                r["ticks_per_second_pool"] = round(1.0 / statistics.median(t["pool"]), 1)
                r["ticks_per_second_bank"] = round(1.0 / statistics.median(t["bank"]), 1)
                # (b) the front end's device time alone, S one-second recordings on the device
                pcm = torch.from_numpy(np.concatenate([np.frombuffer(w, np.int16, WIN) for w in wavs])).to(dev)
                recs = [pcm[k * WIN:(k + 1) * WIN] for k in range(S)]
                x, w0 = segments(pcm, off, step)
                assert x.shape[0] == S and torch.equal(x[S - 1], windows(recs[S - 1], step)[0])
                # a bank primed with the same second of every stream; each timed tick feeds the next chunks
                bank = pre.stream_bank(step, WIN, "PCEN" if front == "pcen" else "MFCCs", dev, slots=S)
                ids = [bank.open() for _ in range(S)]
                xb, _ = bank.tick(ids, pcm, off)
                assert torch.equal(xb, x)
                new = [torch.from_numpy(np.concatenate([np.frombuffer(b, np.int16) for b in c])).to(dev) for c in fed]
                noff = np.arange(S + 1, dtype=np.int64) * step
                t = {"pool": [], "per_stream": [], "bank": []}
                fns = {"pool": lambda: segments(pcm, off, step),
                       "per_stream": lambda: [windows(rec, step) for rec in recs]}
                for rep in range(a.reps + 1):
                    for name, fn_ in fns.items():
                        dt = device_timed(fn_)
                        if rep:
                            t[name].append(dt)
                    before = dict(bank.stats)
                    dt = device_timed(lambda: bank.tick(ids, new[rep], noff))
                    if rep:
                        t["bank"].append(dt)
                r["bank_tick"] = {k: bank.stats[k] - before[k]
                                  for k in ("samples_in", "windows", "frames_computed", "frames_reused")}
                r["segments_tick"] = {"samples_in": S * WIN, "windows": S, "frames_computed": int(plan.frames_computed)}
                r["front_end_device_ms"] = {k: stat(v) for k, v in t.items()}
                r["front_end_device_pool_over_bank"] = round(
                    statistics.median(t["pool"]) / statistics.median(t["bank"]), 3)
                r["front_end_device_ratio"] = round(statistics.median(t["per_stream"]) / statistics.median(t["pool"]), 3)
                res.setdefault(str(ms), {})[str(S)] = r
                del pcm, recs, x, xb, new, bank
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
