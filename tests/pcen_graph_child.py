"""Child process of tests/test_gpu_pcen.py: compute_pcen_batch (B = 4, S = 16000: the fused route)
captured in a torch.cuda.CUDAGraph on a fixed input buffer, the buffer refilled with other clips,
one replay.  Runs here so the parent can bound it with a timeout (a replay that hung would
otherwise hang the suite).  Usage: python pcen_graph_child.py OUT.npz -- writes the replayed
output and the eager output on the second set of clips."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import pcen_ref  # noqa: E402
from honk_amd.audio import AudioPreprocessor  # noqa: E402

DEV = "cuda:0"


def main(out_path):
    ap = AudioPreprocessor()
    ys = pcen_ref.clips()
    first, second = torch.from_numpy(ys[:4]).to(DEV), torch.from_numpy(ys[4:8]).to(DEV)
    buf = first.clone()
    ap.compute_pcen_batch(buf)  # the tables exist before the capture
    eager = ap.compute_pcen_batch(second)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ap.compute_pcen_batch(buf)
    buf.copy_(second)
    graph.replay()
    torch.cuda.synchronize()
    np.savez(out_path, replay=out.cpu().numpy(), eager=eager.cpu().numpy())


if __name__ == "__main__":
    main(sys.argv[1])
