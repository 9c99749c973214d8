"""Child process of tests/test_gpu_cnn_latency.py: everything that replays a captured graph runs
here, so the parent can bound it with a timeout.  Usage: python cnn_latency_graph_child.py OUT.npz
TMPDIR -- captures the batch-1 latency forward of cnn-trad-pool2 (SpeechModel.honk_capture) in
both precisions, replays it on three inputs and writes the replayed and the eager latency logits;
then the reference's label service on its saved cnn-trad-pool2 checkpoint: default arguments
against honk_graph=True, honk_latency=True on the same MFCC map."""
import os
import pathlib
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from honk_amd import model as hm  # noqa: E402
from honk_amd import service as hs  # noqa: E402
import cnn_geometry_cases as geo  # noqa: E402

DEV = "cuda:0"


def main(out_path, tmp):
    for v in geo.ENV_VARS + ("HONK_PRECISION", "HONK_CNN_SPLITK_SLICE"):
        os.environ.pop(v, None)
    case = geo.BY_ID["trad-100x40"]
    cfg, params, x = geo.build(case)
    m = hm.find_model(case.model)(cfg)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
    m = m.eval().to(DEV)
    res = {}
    with torch.no_grad():
        for prec in geo.PRECS:
            m.honk_precision, m.honk_schedule = prec, "latency"
            dev = [torch.tensor(x[i:i + 1]).to(DEV) for i in range(3)]
            eager = [m(d).cpu().numpy() for d in dev]
            cap = m.honk_capture(dev[0])
            res[f"{prec}_flagged_none"] = int(cap.flagged is None)
            res[f"{prec}_schedule_kept"] = int(m.honk_schedule == "latency")
            for i, d in enumerate(dev):
                out = cap.replay(d)
                torch.cuda.synchronize()
                res[f"{prec}_graph_{i}"], res[f"{prec}_eager_{i}"] = out.cpu().numpy(), eager[i]
            try:
                cap.replay(torch.tensor(x[:2]).to(DEV))
                res[f"{prec}_mismatch_raises"] = 0
            except RuntimeError:
                res[f"{prec}_mismatch_raises"] = 1

        # the label service as the reference constructs it, on its saved checkpoint
        import test_callers as tc
        z, plain = tc._service(pathlib.Path(tmp), no_cuda=False)
        wav = np.zeros(16000, np.int16).tobytes()
        off = plain.label(wav)
        svc = hs.TorchLabelService(plain.model_filename, labels=plain.labels, audio_processor=tc._FixedMfcc(z["x"]),
                                   honk_graph=True, honk_latency=True)
        res["svc_is_cnn"] = int(isinstance(svc.model, hm.SpeechModel))
        g1 = svc.label(wav)
        captured = svc._honk_cnn_captured
        g2 = svc.label(wav)
        res["svc_schedule"] = np.array(svc.model.honk_schedule)
        res["svc_labels"] = np.array([off[0], g1[0], g2[0]])
        res["svc_probs"] = np.array([float(off[1]), float(g1[1]), float(g2[1])])
        res["svc_capture_kept"] = int(captured is not None and svc._honk_cnn_captured is captured)
        res["svc_plain_untouched"] = int(plain.model.honk_schedule == "throughput" and plain._honk_cnn_captured is None)
        svc.reload()
        res["svc_reload_drops"] = int(svc._honk_cnn_captured is None)
    torch.cuda.synchronize()
    np.savez(out_path, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
