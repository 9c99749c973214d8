"""Child process of tests/test_gpu_mfcc_segments.py and tests/test_gpu_pcen_segments.py:
honk_mfcc_segments_i16 / honk_pcen_segments_i16 captured in a torch.cuda.graph on fixed buffers (pcm,
the uploaded table, out, the workspace), pcm refilled with other recordings of the same lengths, ONE
replay.  Runs here so the parent can bound it with a timeout (a replay that hung would otherwise hang
the suite).  Usage: python mfcc_segments_graph_child.py mfccs|pcen OUT.npz -- writes the replayed
output and the eager output on the second batch."""
import ctypes
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import segments_cases as sc  # noqa: E402
from honk_amd import _native  # noqa: E402
from honk_amd.audio import AudioPreprocessor  # noqa: E402


def main(which, out_path):
    ap = AudioPreprocessor()
    first, off, stride, _ = sc.batch("ragged_q1", seed=100)
    second, off2, _, _ = sc.batch("ragged_q1", seed=200)
    assert np.array_equal(off, off2) and not np.array_equal(first, second)
    buf = torch.from_numpy(first).to(sc.DEV)
    eager = getattr(ap, f"compute_{which}_segments")(torch.from_numpy(second).to(sc.DEV), off, stride)[0]

    # the host's part (plan, table upload, buffers) happens before the capture: the call itself only enqueues
    rc, plan, _, table = (ap.segments_plan if which == "mfccs" else ap.pcen_segments_plan)(off, stride)
    assert rc == 0
    win, mel, dct = ap._device_tables(buf.device)
    cols = dct.shape[0] if which == "mfccs" else mel.shape[0]
    table_dev = torch.from_numpy(table).to(buf.device)
    out = torch.zeros(int(plan.windows), plan.frames, cols, dtype=torch.float32, device=buf.device)
    ws = torch.zeros(int(plan.workspace_bytes), dtype=torch.uint8, device=buf.device)
    p = ap.pcen_params
    params = _native.PcenParams(p["eps"], p["s"], p["alpha"], p["delta"], p["r"], int(p["power"]))
    head = (buf.data_ptr(), buf.shape[0], off.ctypes.data, len(off) - 1, table_dev.data_ptr(), table.nbytes, sc.WIN,
            stride, win.data_ptr(), ap.n_fft, ap.hop_length, mel.data_ptr(), mel.shape[0])
    mid = (dct.data_ptr(), cols) if which == "mfccs" else (ctypes.addressof(params),)
    fn = getattr(_native.load(), "honk_mfcc_segments_i16" if which == "mfccs" else "honk_pcen_segments_i16")

    def call():
        _native.check(fn(*head, *mid, out.data_ptr(), ws.data_ptr(), ws.numel(), _native.stream_handle(buf.device)),
                      f"honk_{which}_segments_i16")

    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    buf.copy_(torch.from_numpy(second).to(sc.DEV))
    graph.replay()
    torch.cuda.synchronize()
    np.savez(out_path, replay=out.cpu().numpy(), eager=eager.cpu().numpy())


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
