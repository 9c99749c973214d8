"""Child process of tests/test_gpu_pcen_windows.py: compute_pcen_windows captured in a
torch.cuda.graph on a fixed input buffer, the buffer refilled with a second recording, one replay.
Runs here so the parent can bound it with a timeout (a replay that hung would otherwise hang the
suite).  Usage: python pcen_windows_graph_child.py OUT.npz -- writes the replayed output and the
eager output on the second recording."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from honk_amd.audio import AudioPreprocessor  # noqa: E402
from test_mfcc_windows_abi import _pcm  # noqa: E402

DEV = "cuda:0"


def main(out_path):
    n, stride = 16000 + 20 * 160, 160
    ap = AudioPreprocessor()
    first, second = (torch.from_numpy(_pcm(s, n)).to(DEV) for s in (11, 12))
    buf = first.clone()
    ap.compute_pcen_windows(buf, stride)  # the tables and the workspace exist before the capture
    eager = ap.compute_pcen_windows(second, stride)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ap.compute_pcen_windows(buf, stride)
    buf.copy_(second)
    graph.replay()
    torch.cuda.synchronize()
    np.savez(out_path, replay=out.cpu().numpy(), eager=eager.cpu().numpy())


if __name__ == "__main__":
    main(sys.argv[1])
