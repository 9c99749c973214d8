"""Child process of tests/test_gpu_listen_decide.py: honk_listen_decide_f32 captured in a torch.cuda.graph
on fixed buffers (logits, the uploaded segment table, the five outputs), logits refilled with other values,
ONE replay.  Runs here so the parent can bound it with a timeout (a replay that hung would otherwise hang
the suite).  Usage: python listen_decide_graph_child.py OUT.npz -- writes the replayed outputs and the
eager outputs on the second logits."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from honk_amd import _native  # noqa: E402

N, LABELS, KEYWORD, MIN_PROB = 257, 12, 3, 0.3
WINDOW0 = np.array([0, 0, 5, 5, 200, 257, 257], np.int64)
NAMES = ("label", "prob", "sums", "counts", "hit")


def main(out_path):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    first, second = (rng.standard_normal((N, LABELS)).astype(np.float32) for _ in range(2))
    eager = _native.listen_decide(torch.from_numpy(second).to(dev), WINDOW0, KEYWORD, MIN_PROB)

    # the host's part (the table's upload, the buffers) happens before the capture: the call itself only enqueues
    S = len(WINDOW0) - 1
    logits = torch.from_numpy(first).to(dev)
    w0 = torch.from_numpy(WINDOW0).to(dev)
    outs = (torch.zeros(N, dtype=torch.int32, device=dev), torch.zeros(N, dtype=torch.float32, device=dev),
            torch.zeros(S, LABELS, dtype=torch.float64, device=dev),
            torch.zeros(S, LABELS, dtype=torch.int32, device=dev), torch.zeros(S, dtype=torch.int64, device=dev))

    def call():
        _native.check(_native.load().honk_listen_decide_f32(
            logits.data_ptr(), N, LABELS, w0.data_ptr(), S, KEYWORD, MIN_PROB, *(t.data_ptr() for t in outs),
            _native.stream_handle(dev)), "honk_listen_decide_f32")

    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    logits.copy_(torch.from_numpy(second).to(dev))
    graph.replay()
    torch.cuda.synchronize()
    np.savez(out_path, **{f"replay_{k}": t.cpu().numpy() for k, t in zip(NAMES, outs)},
             **{f"eager_{k}": t.cpu().numpy() for k, t in zip(NAMES, eager)})


if __name__ == "__main__":
    main(sys.argv[1])
