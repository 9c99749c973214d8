"""Child process of tests/test_cnn_nonfinite.py: the one captured replay.  Usage: python
cnn_nonfinite_graph_child.py OUT.npz -- captures the batch-3 latency forward of the cnn-trad-pool2
fixture (SpeechModel.honk_capture) in both precisions and replays it three times: on the clean
clips, with a NaN at a live entry of clip 1, and on the clean clips again.  Writes the three
replays' logits and the eager latency logits of the clean clips."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from honk_amd import model as hm  # noqa: E402
import cnn_geometry_cases as geo  # noqa: E402
import cnn_nonfinite_cases as nf  # noqa: E402
from golden_util import GOLDEN, load_fixture  # noqa: E402

DEV = "cuda:0"
NAME = "cnn-trad-pool2"


def main(out_path):
    for v in geo.ENV_VARS + ("HONK_PRECISION", "HONK_CNN_SPLITK_SLICE"):
        os.environ.pop(v, None)
    z = np.load(os.path.join(GOLDEN, f"nonfinite_{NAME}.npz"), allow_pickle=False)
    cfg, params, x0, _, meta = load_fixture(NAME)
    x = np.concatenate([x0] * 3)[:3].astype(np.float32)
    _, r, c, _ = nf.pokes(x.shape[1], x.shape[2], z["dead_rows"].tolist(), z["dead_cols"].tolist())[0]
    poked = x.copy()
    poked[1, r, c] = np.nan
    m = hm.find_model(meta["model"])(cfg)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
    m = m.eval().to(DEV)
    res = {}
    with torch.no_grad():
        for prec in geo.PRECS:
            m.honk_precision, m.honk_schedule = prec, "latency"
            clean_d, poked_d = torch.tensor(x).to(DEV), torch.tensor(poked).to(DEV)
            res[f"{prec}_eager"] = m(clean_d).cpu().numpy()
            cap = m.honk_capture(clean_d)
            for key, d in (("clean", clean_d), ("poked", poked_d), ("restored", clean_d)):
                out = cap.replay(d)
                torch.cuda.synchronize()
                res[f"{prec}_{key}"] = out.cpu().numpy()
    torch.cuda.synchronize()
    np.savez(out_path, **res)


if __name__ == "__main__":
    main(sys.argv[1])
