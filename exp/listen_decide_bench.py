"""The stage after the forward on the device: a StreamPool(device_state=True) tick with the logits
downloaded and softmax / argmax / max run row by row on the host (the default service: the unchanged
route) against the same tick with (label, prob) from honk_listen_decide_f32 (``honk_decide=True``), and
against ``feed_arrays`` (the tick fed and read as arrays: no per-stream Python on either side of the device
work) (one GPU, cuda:0).

    python exp/listen_decide_bench.py [--streams 1 64 1024] [--ticks 100 500] [--fronts mfcc pcen]
                                      [--reps 7] [--out profiles/listen_decide_bench.json]

Per front end, tick length (ms of audio per stream per tick, the stride being the tick) and number of
streams S, back to back in one process: every stream is primed with one second, so each further tick
completes exactly one window per stream.  After a warm-up tick of every route, --reps timed ticks each,
alternating tick by tick on the same chunks, the device synchronised around every timed region (host clock):
  feed             StreamPool.feed({k: bytes_k}) on the default service;
  feed_decide      the same call on a honk_decide=True service;
  feed_arrays      pool.feed_arrays(keys, pcm, offsets), the int16 array and the offsets built beforehand
                   (a caller that receives its audio as one buffer);
  arrays_from_bytes  the same with the array built inside the timed region from the per-key byte strings
                   (one join), for a caller that holds what ``feed`` takes.
A difference between two routes counts only where it exceeds the larger of their min-to-max spreads
("beyond_spread").  Also: the bytes each route downloads per tick (from the shapes: the logits, or label +
prob), and the device time of honk_listen_decide_f32 alone on the tick's S x n_labels logits (events around
20 back-to-back calls on fixed buffers, per call), rows only and with S one-window segments.
Prints one JSON line (median, min, max per figure, ms); --out also writes it to a file."""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from honk_amd import _native  # noqa: E402
from honk_amd import model as hm  # noqa: E402
from honk_amd import service as hs  # noqa: E402
from listen_pool_bench import WIN, device_timed, host_timed, recording, stat  # noqa: E402

ROUTES = ("feed", "feed_decide", "feed_arrays", "arrays_from_bytes")
CALLS = 20


def compare(t, a, b):
    """a against b: the ratio of the medians, and whether the difference exceeds both spreads."""
    ma, mb = statistics.median(t[a]), statistics.median(t[b])
    spread = max(max(t[a]) - min(t[a]), max(t[b]) - min(t[b]))
    return {"ratio": round(ma / mb, 3), "difference_ms": round((ma - mb) * 1e3, 4), "spread_ms": round(spread * 1e3, 4),
            "beyond_spread": bool(abs(ma - mb) > spread)}


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
    lib = _native.load()
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "model": "cnn-trad-pool2", "fronts": {}}
    for front in a.fronts:
        torch.manual_seed(0)
        with tempfile.TemporaryDirectory() as tmp:
            fn = os.path.join(tmp, "m.pt")
            hm.SpeechModel(dict(hm.find_config("cnn-trad-pool2"), n_labels=len(labels))).save(fn)
            kind = "PCEN" if front == "pcen" else "MFCCs"
            plain = hs.TorchLabelService(fn, labels=labels, audio_preprocess_type=kind)
            dec = hs.TorchLabelService(fn, labels=labels, audio_preprocess_type=kind, honk_decide=True)
        res = out["fronts"][front] = {}
        for ms in a.ticks:
            step = 16 * ms                       # samples per tick = the stride
            for S in a.streams:
                need = WIN + (a.reps + 1) * step
                base = recording(need + 37 * S, seed=S + ms)
                wavs = [base[37 * k:37 * k + need].tobytes() for k in range(S)]
                keys = list(range(S))
                pools = {"feed": hs.StreamPool(plain, ms, device_state=True),
                         "feed_decide": hs.StreamPool(dec, ms, device_state=True),
                         "feed_arrays": hs.StreamPool(dec, ms, device_state=True),
                         "arrays_from_bytes": hs.StreamPool(dec, ms, device_state=True)}
                for pool in pools.values():
                    assert pool.bank is not None
                    first = pool.feed({k: w[:2 * WIN] for k, w in enumerate(wavs)})
                    assert all(len(first[k]) == 1 for k in keys)
                offsets = np.arange(S + 1, dtype=np.int64) * step
                got = {}

                def run(name, c, pcm):
                    if name in ("feed", "feed_decide"):
                        r = pools[name].feed(dict(enumerate(c)))
                        assert all(len(r[k]) == 1 for k in keys)
                        got[name] = ([labels.index(r[k][0][0]) for k in keys], [r[k][0][1] for k in keys])
                        return
                    if name == "arrays_from_bytes":
                        pcm = np.frombuffer(b"".join(c), np.int16)
                    label, prob, w0 = pools[name].feed_arrays(keys, pcm, offsets)
                    assert w0[-1] == S
                    got[name] = (label.tolist(), prob.tolist())

                t = {name: [] for name in ROUTES}
                for rep in range(a.reps + 1):
                    i = 2 * WIN + 2 * step * rep
                    c = [w[i:i + 2 * step] for w in wavs]   # (every route's streams are at the same position)
                    pcm = np.frombuffer(b"".join(c), np.int16).copy()
                    for name in ROUTES:
                        dt = host_timed(lambda: run(name, c, pcm))
                        if rep:
                            t[name].append(dt)
                    for name in ROUTES[1:]:                  # the routes agree on every tick
                        assert got[name][0] == got["feed"][0], (name, rep)
                        assert max(abs(x - y) for x, y in zip(got[name][1], got["feed"][1])) <= 1e-6, (name, rep)
                r = {"end_to_end_ms": {k: stat(v) for k, v in t.items()},
                     "against_feed": {k: compare(t, k, "feed") for k in ROUTES[1:]},
                     "downloaded_bytes_per_tick": {"feed": S * len(labels) * 4, "feed_decide": S * 8,
                                                   "feed_arrays": S * 8, "arrays_from_bytes": S * 8}}
                # honk_listen_decide_f32 alone on a tick's logits: fixed buffers, CALLS back-to-back calls
                logits = torch.randn(S, len(labels), device=dev)
                w0 = torch.arange(S + 1, dtype=torch.int64, device=dev)
                outs = (torch.empty(S, dtype=torch.int32, device=dev), torch.empty(S, device=dev),
                        torch.empty(S, len(labels), dtype=torch.float64, device=dev),
                        torch.empty(S, len(labels), dtype=torch.int32, device=dev),
                        torch.empty(S, dtype=torch.int64, device=dev))
                stream = _native.stream_handle(dev)

                def calls(segments):
                    for _ in range(CALLS):
                        _native.check(lib.honk_listen_decide_f32(
                            logits.data_ptr(), S, len(labels), w0.data_ptr(), segments, 2, 0.85,
                            *(o.data_ptr() for o in outs), stream), "honk_listen_decide_f32")

                d = {"rows": [], "rows_and_segments": []}
                for rep in range(a.reps + 1):
                    for name, segments in (("rows", 0), ("rows_and_segments", S)):
                        dt = device_timed(lambda: calls(segments)) / CALLS
                        if rep:
                            d[name].append(dt)
                r["decide_device_ms_per_call"] = {k: stat(v) for k, v in d.items()}
                res.setdefault(str(ms), {})[str(S)] = r
                del pools, logits, outs
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
