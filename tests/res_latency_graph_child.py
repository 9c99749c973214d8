"""Child process of tests/test_gpu_res_latency.py: everything that replays a captured graph runs
here, so the parent can bound it with a timeout (a replay that hung would otherwise hang the
suite).  Usage: python res_latency_graph_child.py OUT.npz TMPDIR -- captures the batch-1
latency forward of res15 (auto -> f16x2), replays it on three inputs (two calibrated clips and
an out-of-calibration one) and writes the replayed and the eager latency logits and flagged
counts; then the label service's label() with honk_latency, with and without honk_graph."""
import os
import pathlib
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from honk_amd import model as hm  # noqa: E402
from golden_util import load_fixture, load_range_fixture  # noqa: E402

DEV = "cuda:0"


def main(out_path, tmp):
    for v in ("HONK_PRECISION", "HONK_RES_KERNEL", "HONK_LAST_KERNEL", "HONK_CONV0", "HONK_F16X2_RERUN",
              "HONK_RES_CHUNK"):
        os.environ.pop(v, None)
    cfg, params, x, _, _ = load_fixture("res15-b3-mfcc")
    _, _, x_ood, _, _ = load_range_fixture("res15-ood")
    m = hm.find_model("res15")(cfg)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
    m = m.eval().to(DEV)
    clips = dict(a=x[0:1], ood=x_ood[0:1], b=x[1:2])
    dev = {k: torch.as_tensor(v).to(DEV) for k, v in clips.items()}
    res = {}
    with torch.no_grad():
        m(torch.as_tensor(x).to(DEV))  # the policy's probe sees the calibrated batch
        m.honk_schedule = "latency"
        for k, xb in dev.items():
            out = m(xb)
            res["eager_" + k], res["eager_count_" + k] = out.cpu().numpy(), int(m.honk_last_rerun_dev)
        res["precision"] = np.array(m.honk_last_precision)
        cap = m.honk_capture(dev["a"])
        res["schedule_kept"] = int(m.honk_schedule == "latency" and m.honk_stream_ordered is False)
        for k in ("a", "ood", "b"):
            out = cap.replay(dev[k])
            torch.cuda.synchronize()
            res["graph_" + k], res["graph_count_" + k] = out.cpu().numpy(), int(cap.flagged)

        # the label service with the res15 model in place of the reference caller's cnn
        import test_callers as tc
        z, svc = tc._service(pathlib.Path(tmp), no_cuda=False)
        m.honk_schedule = "throughput"
        svc.model, svc.labels = m, [str(i) for i in range(12)]
        svc.audio_processor = tc._FixedMfcc(x[0])
        wav = np.zeros(16000, np.int16).tobytes()
        off = svc.label(wav)
        svc.honk_latency = True
        on = svc.label(wav)
        res["svc_schedule"] = np.array(m.honk_schedule)
        svc.honk_graph = True
        g1 = svc.label(wav)
        captured = svc._honk_captured
        g2 = svc.label(wav)
        res["svc_labels"] = np.array([off[0], on[0], g1[0], g2[0]])
        res["svc_probs"] = np.array([float(off[1]), float(on[1]), float(g1[1]), float(g2[1])])
        res["svc_capture_kept"] = int(captured is not None and svc._honk_captured is captured)
    torch.cuda.synchronize()
    np.savez(out_path, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
