"""compute_mfccs_windows on the device (honk_mfcc_windows_i16, csrc/mfcc_stream.hip) and the serving
surface over it (label_stream, listen_stream, StreamListener).

Reference of a window: oracle.mfcc_ref.mfcc(int16 slice / 32768.) at the front-end bound of
tests/frontend_geometry_cases.py (16 x the error of the float32 restatement oracle/frontend_f32_sim.py
on the recording's windows, never above 1e-4; relative to max|ref window|, rtol = 0), and today's
device path (compute_mfccs_batch on the sliced float windows) at the same bound, against the oracle
and against the new path.  Bitwise properties: shared frames, two runs, shifted
recordings, window ranges, a captured graph's replay.  The kernel works on tiles of FT = 32 frame
slots; an edge tile holds the 4 edge frames of 8 windows."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from honk_amd import model as hm
from honk_amd import service as hs
from honk_amd.audio import AudioPreprocessor
from oracle import frontend_f32_sim as sim
from oracle import mfcc_ref
from test_mfcc_windows_abi import _pcm, _same, _service

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"
WIN = 16000

# name -> (recording, stride); each the smallest recording that hits its case
CASES = {
    "stride160_21": lambda: (_pcm(20, WIN + 20 * 160), 160),    # q = 1: a frame fans out to up to 21 windows
    "stride8000_5": lambda: (_pcm(21, 48000), 8000),            # the reference's default stride
    "stride16000_3": lambda: (_pcm(22, 48000), 16000),          # no overlap
    "stride24000_2": lambda: (_pcm(23, 56000), 24000),          # gaps between the windows
    "stride400_11": lambda: (_pcm(24, 20000), 400),             # stride % hop != 0: the unshared route
    "single": lambda: (_pcm(25, WIN), 160),
    "one_short": lambda: (_pcm(26, WIN + 8000 - 1), 8000),      # 1 sample short of a second window
    "zeros": lambda: (np.zeros(24000, np.int16), 8000),
    # 33 windows at q = 1: 32 + 97 = 129 shared frames, one more than 4 tiles of 32; 132 edge frames, one
    # window's 4 (the step the count moves in) more than 4 tiles of 32; edge tiles cross workgroups
    "stride160_33": lambda: (_pcm(27, WIN + 32 * 160), 160),
    "stride320_9": lambda: (_pcm(28, WIN + 8 * 320), 320),      # 36 edge frames: one window more than a tile
}


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def _case(name):
    """(recording, stride, device result [W,101,40], per-window oracle) -- computed once, read-only."""
    x, stride = CASES[name]()
    out = AudioPreprocessor().compute_mfccs_windows(torch.from_numpy(x).to(DEV), stride).cpu().numpy()
    W = 0 if len(x) < WIN else 1 + (len(x) - WIN) // stride
    refs = [mfcc_ref.mfcc(x[w * stride:w * stride + WIN] / 32768.) for w in range(W)]
    out.setflags(write=False)
    return x, stride, out, refs


def _windows(x, stride, n):
    return np.stack([x[w * stride:w * stride + WIN] for w in range(n)]).astype(np.float32) / 32768.


@pytest.mark.parametrize("name", list(CASES))
def test_matches_oracle_and_per_window_kernel(name):
    _gpu()
    x, stride, out, refs = _case(name)
    assert out.shape == (len(refs), 101, 40) and len(refs) >= 1
    assert np.isfinite(out).all()
    old = AudioPreprocessor().compute_mfccs_batch(torch.from_numpy(_windows(x, stride, len(refs))).to(DEV)).cpu().numpy()
    e_ref = max(np.abs(out[w] - r).max() / max(np.abs(r).max(), 1e-30) for w, r in enumerate(refs))
    e_old = max(np.abs(out[w] - old[w]).max() / max(np.abs(r).max(), 1e-30) for w, r in enumerate(refs))
    print(f"{name}: max|new - oracle| / max|ref| = {e_ref:.3e}   max|new - per-window kernel| / max|ref| = {e_old:.3e}")
    b = sim.bound(sim.e32("mfcc", _windows(x, stride, len(refs)), refs)) if x.any() else sim.CAP
    for w, ref in enumerate(refs):
        np.testing.assert_allclose(out[w], ref, atol=b * np.abs(ref).max(), rtol=0)
        np.testing.assert_allclose(old[w], ref, atol=b * np.abs(ref).max(), rtol=0)
        np.testing.assert_allclose(out[w], old[w], atol=b * np.abs(ref).max(), rtol=0)


def test_zero_recording_passes_through():
    """log of the non-positive mel energies passes through (manage_audio.py:31-39): exact zeros."""
    _gpu()
    _, _, out, refs = _case("zeros")
    assert len(refs) == 2 and not out.any() and not np.any(refs[0])


def test_gapped_windows_ignore_the_samples_between_them():
    """Stride 24000: samples 16000..23999 belong to no window; changing them changes nothing."""
    _gpu()
    x, stride, out, _ = _case("stride24000_2")
    y = x.copy()
    y[16000:24000] = 12345
    got = AudioPreprocessor().compute_mfccs_windows(torch.from_numpy(y).to(DEV), stride).cpu().numpy()
    assert np.array_equal(got, out)


def test_sharing_is_real():
    _gpu()
    _, _, out, _ = _case("stride160_21")
    for w in range(20):
        assert np.array_equal(out[w, 3:99], out[w + 1, 2:98]), w


def test_two_runs_are_bitwise_equal():
    _gpu()
    x, stride, out, _ = _case("stride160_21")
    again = AudioPreprocessor().compute_mfccs_windows(torch.from_numpy(x).to(DEV), stride).cpu().numpy()
    assert np.array_equal(again, out)


@pytest.mark.parametrize("name,k", [("stride160_21", 1), ("stride160_21", 7), ("stride8000_5", 1)])
def test_position_independence(name, k):
    _gpu()
    x, stride, out, _ = _case(name)
    tail = AudioPreprocessor().compute_mfccs_windows(torch.from_numpy(x[k * stride:].copy()).to(DEV), stride)
    assert np.array_equal(tail.cpu().numpy(), out[k:])


def test_window_ranges_concatenate_to_the_whole():
    _gpu()
    x, stride, out, _ = _case("stride160_21")
    ap, pcm = AudioPreprocessor(), torch.from_numpy(x).to(DEV)
    parts = [ap.compute_mfccs_windows(pcm, stride, first=f, count=3) for f in range(0, 21, 3)]
    assert np.array_equal(torch.cat(parts).cpu().numpy(), out)
    assert ap.compute_mfccs_windows(pcm, stride, first=21, count=0).shape == (0, 101, 40)
    x4, s4, out4, _ = _case("stride400_11")
    part = ap.compute_mfccs_windows(torch.from_numpy(x4).to(DEV), s4, first=4, count=5)
    assert np.array_equal(part.cpu().numpy(), out4[4:9])


def test_capturable():
    """The call inside torch.cuda.graph on a fixed buffer; the buffer refilled, one replay: the eager
    result on the second recording, bit for bit.  In a child under a timeout."""
    _gpu()
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "child.npz")
        try:
            p = subprocess.run([sys.executable, os.path.join(HERE, "mfcc_windows_graph_child.py"), out],
                               capture_output=True, text=True, timeout=120)
        except subprocess.TimeoutExpired:
            pytest.exit("tests/mfcc_windows_graph_child.py (graph capture / replay) hung: stopping the GPU run", 1)
        if p.returncode < 0 or p.returncode in (134, 139):
            pytest.exit(f"tests/mfcc_windows_graph_child.py died with status {p.returncode}: stopping the GPU run\n"
                        f"{p.stderr[-3000:]}", 1)
        assert p.returncode == 0, p.stderr[-3000:]
        z = np.load(out)
        assert z["replay"].shape == (21, 101, 40) and np.array_equal(z["replay"], z["eager"])


# ---- the service ---------------------------------------------------------------------------------
SERVICE_SEEDS = {500: 31, 100: 31}  # 3 s recordings; no window of theirs is a near tie (checked below)


def _wav(seed):
    return _pcm(seed, 48000).tobytes()


def _no_ties(logits_fn, wav, stride_ms):
    """No window's top two probabilities (CPU, numpy MFCC) within 2e-4 of each other."""
    wins = list(hs.stride(wav, 32 * stride_ms, 32000))
    ap = AudioPreprocessor()
    x = torch.from_numpy(np.stack([ap.compute_mfccs(np.frombuffer(w, np.int16).astype(np.float32) / 32768.).squeeze(2)
                                   for w in wins]))
    with torch.no_grad():
        p = torch.softmax(logits_fn(x), 1).numpy()
    top = np.sort(p, 1)
    assert (top[:, -1] - top[:, -2] > 2e-4).all()
    return len(wins)


@pytest.mark.parametrize("stride_ms", [500, 100])
def test_label_stream_matches_label_batch(tmp_path, stride_ms):
    _gpu()
    wav = _wav(SERVICE_SEEDS[stride_ms])
    cpu = _service(tmp_path, no_cuda=True)
    n = _no_ties(cpu.model, wav, stride_ms)
    assert n == {500: 5, 100: 21}[stride_ms]
    svc = _service(tmp_path, no_cuda=False)
    got = svc.label_stream(wav, stride_ms)
    want = svc.label_batch(list(hs.stride(wav, 32 * stride_ms, 32000)))
    assert len(got) == n
    _same(got, want, 1e-4)
    _same(got, cpu.label_stream(wav, stride_ms), 1e-4)


def test_service_chunks_listen_and_listener(tmp_path):
    _gpu()
    wav = _wav(SERVICE_SEEDS[100])
    svc = _service(tmp_path, no_cuda=False)
    whole = svc.label_stream(wav, 100)
    _same(svc.label_stream(wav, 100, max_windows=3), whole, 1e-6)
    for ms in (500, 100):
        a, b = svc.listen_stream(wav, ms), svc.listen(wav, ms)
        assert a.keys() == b.keys() and all(abs(a[k] - b[k]) < 1e-4 for k in a)
        for kw in svc.labels:
            assert svc.listen_stream(wav, ms, method="command_tagging", keyword=kw, min_keyword_prob=0.2) == \
                svc.listen(wav, ms, method="command_tagging", keyword=kw, min_keyword_prob=0.2)
    sl, got = hs.StreamListener(svc, 100), []
    for i in range(0, len(wav), 2 * 1234):
        got += sl.feed(wav[i:i + 2 * 1234])
    _same(got, whole, 1e-6)


def test_label_stream_is_model_agnostic(tmp_path):
    """The same service with a res8 model on the device in place of cnn-trad-pool2."""
    _gpu()
    wav = _wav(SERVICE_SEEDS[500])
    svc = _service(tmp_path, no_cuda=False)
    torch.manual_seed(1)
    m = hm.find_model("res8")(dict(hm.find_config("res8"), n_labels=len(svc.labels))).eval()
    _no_ties(m, wav, 500)
    svc.model = m.to(DEV)
    got = svc.label_stream(wav, 500)
    want = svc.label_batch(list(hs.stride(wav, 16000, 32000)))
    assert len(got) == 5
    _same(got, want, 1e-4)
