"""The ragged batches of tests/test_gpu_mfcc_segments.py and tests/test_gpu_pcen_segments.py
(honk_mfcc_segments_i16 / honk_pcen_segments_i16, csrc/mfcc_stream.hip) and what the two files share:
each batch is the smallest that reaches one way the per-recording lookup or the tiling can go wrong.

FT = 32 frame slots per workgroup; at n_fft 480 / hop 160 a window has 97 interior and 2 + 2 edge
frames, an edge group is one side of one window and an edge tile holds 16 groups."""
import ctypes

import numpy as np
import torch

from honk_amd import _native
from test_mfcc_windows_abi import _pcm

DEV = "cuda:0"
WIN = 16000
Q1 = [16000, 16000 + 32 * 160, 15999, 16000 + 160]

# name -> (recording lengths, stride, unowned samples before / between / after the recordings)
BATCHES = {
    # 1 / 33 / 0 / 2 windows: 129 shared frames (4 tiles + 1) in the second recording, a zero-window
    # recording in the middle, 72 edge groups (4.5 tiles), one edge tile holding three recordings
    "ragged_q1": (Q1, 160, 0),
    # the pool's tick: 18 edge groups (the second edge tile partly empty), 4 segment tiles per recording
    "ones_9": ([16000] * 9, 8000, 0),
    "gapped": ([56000, 16000, 40000], 24000, 0),     # per-window segment tiles across recordings
    "unshared": ([20000, 16399, 16400], 400, 0),     # stride % hop != 0
    "empty_ends": ([0, 24000, 0], 8000, 0),          # empty first and last recordings
    "holes": (Q1, 160, 1000),                        # offsets[0] > 0, samples that belong to no recording
}


# The helpers below take the shape by keyword (window; frames and cols of a row block; spec: a batch that
# is not in BATCHES, as (lengths, stride, hole)); the defaults are the reference shape the batches above
# are written for.  tests/stream_geometry_cases.py has the batches off that shape.
def n_windows(n, stride, window=WIN):
    return 0 if n < window else 1 + (n - window) // stride


def batch(name, reverse=False, seed=100, window=WIN, spec=None):
    """(pcm int16 [total], offsets int64, stride, rows) of a batch; rows: [(recording, index into offsets)]
    of the batch's recordings in order.  With unowned samples (``holes``) the buffer is hole, recording,
    hole, ..., recording, hole: offsets[0] skips the first, offsets[-1] stops before the last, and a hole
    between two recordings -- one offsets array locates contiguous ranges only -- is a range of its own,
    shorter than a window: it has no window, owns no row of out and must never be read."""
    lens, stride, hole = BATCHES[name] if spec is None else spec
    recs = [_pcm(seed + i, n) for i, n in enumerate(lens)]
    if reverse:
        recs = recs[::-1]
    gap = _pcm(seed + 50, hole)
    assert hole < window
    parts, off, rows, pos = [gap], [hole], [], hole
    for i, r in enumerate(recs):
        rows.append((r, len(off) - 1))
        parts.append(r)
        pos += len(r)
        off.append(pos)
        if hole and i + 1 < len(recs):
            parts.append(gap)
            pos += hole
            off.append(pos)
    parts.append(gap)
    return np.concatenate(parts), np.asarray(off, np.int64), stride, rows


def unowned(name, **kw):
    """Boolean mask over the buffer of batch(name): the samples of no recording."""
    pcm, off, _, rows = batch(name, **kw)
    mask = np.ones(len(pcm), bool)
    for r, i in rows:
        mask[off[i]:off[i + 1]] = False
    return mask


def native_segments(arena, which, ap, pcm, off, stride, frozen, window=WIN):
    """The C call itself on buffers of the test's own: out and the workspace from ``arena`` (poisoned,
    guard-banded), the table uploaded here; ``frozen(pcm, table)`` wraps the call.  -> out (device)."""
    plan_fn = ap.segments_plan if which == "mfccs" else ap.pcen_segments_plan
    rc, plan, w0, table = plan_fn(off, stride, window)
    assert rc == 0
    win, mel, dct = ap._device_tables(pcm.device)
    cols = dct.shape[0] if which == "mfccs" else mel.shape[0]
    table_dev = torch.from_numpy(table).to(pcm.device)
    out = arena.buffer((int(plan.windows), plan.frames, cols), torch.float32, pcm.device, "out")
    ws = arena.buffer((int(plan.workspace_bytes),), torch.uint8, pcm.device, "workspace")
    head = (pcm.data_ptr(), pcm.shape[0], off.ctypes.data, len(off) - 1, table_dev.data_ptr(), table.nbytes, window,
            stride, win.data_ptr(), ap.n_fft, ap.hop_length, mel.data_ptr(), mel.shape[0])
    tail = (out.data_ptr(), ws.data_ptr(), ws.numel(), _native.stream_handle(pcm.device))
    lib = _native.load()
    with frozen(pcm, table_dev):
        if which == "mfccs":
            rc = lib.honk_mfcc_segments_i16(*head, dct.data_ptr(), cols, *tail)
        else:
            p = ap.pcen_params
            params = _native.PcenParams(p["eps"], p["s"], p["alpha"], p["delta"], p["r"], int(p["power"]))
            rc = lib.honk_pcen_segments_i16(*head, ctypes.addressof(params), *tail)
        _native.check(rc, f"honk_{which}_segments_i16")
        torch.cuda.synchronize()
    return out


def segments(which, ap, pcm_np, off, stride, window=WIN):
    """compute_{which}_segments on the device -> (out numpy, window0)."""
    out, w0 = getattr(ap, f"compute_{which}_segments")(torch.from_numpy(pcm_np).to(DEV), off, stride, window)
    assert out.is_cuda and out.dtype == torch.float32
    return out.cpu().numpy(), w0


def alone(which, ap, rec, stride, window=WIN):
    """compute_{which}_windows of one recording in a buffer of its own: what its rows must equal."""
    return getattr(ap, f"compute_{which}_windows")(torch.from_numpy(np.ascontiguousarray(rec)).to(DEV),
                                                   stride, window).cpu().numpy()


def check_rows(which, ap, name, reverse=False, window=WIN, frames=101, cols=40, spec=None, seed=100):
    """Every recording's rows of the batch bit-equal to the single-recording call; the ranges that are no
    recording (holes) own no rows.  -> (out, [rows of each recording, in the batch's order])."""
    pcm, off, stride, rows = batch(name, reverse, seed, window=window, spec=spec)
    out, w0 = segments(which, ap, pcm, off, stride, window)
    W = [n_windows(int(off[i + 1] - off[i]), stride, window) for i in range(len(off) - 1)]
    assert w0.tolist() == np.concatenate([[0], np.cumsum(W)]).tolist()
    assert out.shape == (sum(W), frames, cols) and np.isfinite(out).all()
    blocks = []
    for rec, i in rows:
        want = alone(which, ap, rec, stride, window)
        got = out[w0[i]:w0[i + 1]]
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), (name, i)
        blocks.append(got)
    assert sum(len(b) for b in blocks) == len(out)
    return out, blocks
