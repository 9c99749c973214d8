"""Child process of tests/test_gpu_ordered.py: everything that replays a captured graph runs
here, so the parent can bound it with a timeout (a replay that hung would otherwise hang the
suite).  Usage: python ordered_graph_child.py OUT.npz TMPDIR -- writes the eager stream-ordered
logits, the replayed ones and the flagged counts of three 6-clip batches, and the label
service's answers with and without honk_graph."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from honk_amd import model as hm  # noqa: E402
from golden_util import load_fixture, load_range_fixture  # noqa: E402

DEV = "cuda:0"


def batches():
    cfg, params, x, logits, meta = load_fixture("res15-b3-mfcc")
    _, _, x_ood, l_ood, _ = load_range_fixture("res15-ood")
    six = lambda a: np.concatenate([a] * (6 // len(a) + 1))[:6]  # noqa: E731
    return cfg, params, dict(mixed=np.stack([x[0], x_ood[0], x[1], x_ood[1], x[2], x_ood[2]]),
                             benign=six(x), flagged=six(x_ood))


def main(out_path, tmp):
    for v in ("HONK_PRECISION", "HONK_RES_KERNEL", "HONK_LAST_KERNEL", "HONK_CONV0", "HONK_F16X2_RERUN",
              "HONK_RES_CHUNK"):
        os.environ.pop(v, None)
    cfg, params, xs = batches()
    m = hm.find_model("res15")(cfg)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
    m = m.eval().to(DEV)
    res = {}
    dev = {k: torch.as_tensor(v).to(DEV) for k, v in xs.items()}
    with torch.no_grad():
        m.honk_stream_ordered = True
        for k, xb in dev.items():
            out = m(xb)
            res["eager_" + k], res["eager_count_" + k] = out.cpu().numpy(), int(m.honk_last_rerun_dev)
        m.honk_stream_ordered = False
        cap = m.honk_capture(dev["mixed"])
        res["ordered_restored"] = int(m.honk_stream_ordered is False)
        # one graph, three device-held counts
        for k in ("mixed", "benign", "flagged"):
            out = cap.replay(dev[k])
            res["static_output"] = int(out is cap.logits)
            torch.cuda.synchronize()
            res["graph_" + k], res["graph_count_" + k] = out.cpu().numpy(), int(cap.flagged)
        try:
            cap.replay(dev["mixed"][:3])
            res["mismatch_raises"] = 0
        except RuntimeError:
            res["mismatch_raises"] = 1

        # the label service: the reference caller's fixture (cnn-trad-pool2: honk_graph has
        # nothing to capture), then the same service with the res15 model in its place
        import pathlib
        import test_callers as tc
        z, svc = tc._service(pathlib.Path(tmp), no_cuda=False)
        wav = np.zeros(16000, np.int16).tobytes()
        off = svc.label(wav)
        svc.honk_graph = True
        on = svc.label(wav)
        res["cnn_same"] = int(off[0] == on[0] and float(off[1]) == float(on[1]) and svc._honk_captured is None)
        cnn_labels = svc.labels
        svc.model, svc.labels = m, [str(i) for i in range(12)]
        svc.audio_processor = tc._FixedMfcc(xs["benign"][0])
        svc.honk_graph = False
        off = svc.label(wav)
        svc.honk_graph = True
        on = svc.label(wav)
        captured = svc._honk_captured
        on2 = svc.label(wav)  # the second call replays the same capture
        res["res_labels"] = np.array([off[0], on[0], on2[0]])
        res["res_probs"] = np.array([float(off[1]), float(on[1]), float(on2[1])])
        res["capture_kept"] = int(captured is not None and svc._honk_captured is captured)
        svc.labels = cnn_labels  # (reload() builds the reference's cnn-trad-pool2 model for these)
        svc.reload()
        res["reload_drops"] = int(svc._honk_captured is None)
    torch.cuda.synchronize()
    np.savez(out_path, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
