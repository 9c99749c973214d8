"""compute_pcen_windows on the device (honk_pcen_windows_i16, csrc/mfcc_stream.hip: the mel energies
of each STFT frame once, then a scan per window) and the PCEN serving surface over it (label_stream,
listen_stream, StreamListener).

Reference of a window: the float64 tests/pcen_ref.pcen(int16 slice / 32768.).  Bound: the project's
front-end rule -- atol = sim.bound(sim.e32("pcen", windows, refs)) * max(max|ref window|, 1e-6), rtol = 0:
16 x the error of the float32 restatement oracle/frontend_f32_sim.py on the same windows, never above
sim.CAP = 1e-4 -- for the new route against the oracle, for the per-window route (compute_pcen_batch on
the sliced float windows) against the oracle, and for the two against each other.  Bitwise properties as
for the MFCC windows: two runs, shifted recordings, a window cut out, window ranges, a captured graph's
replay.  Every recording is at most 56,000 samples."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import frontend_geometry_cases as fg
import pcen_ref
import poison_util as pu
from honk_amd import model as hm
from honk_amd import service as hs
from honk_amd.audio import AudioPreprocessor
from oracle import frontend_f32_sim as sim
from test_gpu_memory_contract import four_fills
from test_gpu_mfcc_windows import CASES
from test_mfcc_windows_abi import _pcm, _same

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"
WIN = 16000
ALT = dict(s=0.1, alpha=0.8, delta=1.0, r=0.25)


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _new(x, stride, ap=None, **kw):
    out = (ap or AudioPreprocessor()).compute_pcen_windows(torch.from_numpy(np.ascontiguousarray(x)).to(DEV), stride,
                                                           **kw)
    assert out.is_cuda and out.dtype == torch.float32
    return out.cpu().numpy()


def _windows(x, stride, n, window=WIN):
    return np.stack([x[w * stride:w * stride + window] for w in range(n)]).astype(np.float32) / np.float32(32768.)


def _n(x, stride, window=WIN):
    return 0 if len(x) < window else 1 + (len(x) - window) // stride


@functools.lru_cache(maxsize=None)
def _case(name):
    """(recording, stride, device result [W,101,40], per-window oracle) -- computed once, read-only."""
    x, stride = CASES[name]()
    out = _new(x, stride)
    refs = [pcen_ref.pcen(x[w * stride:w * stride + WIN] / 32768.) for w in range(_n(x, stride))]
    out.setflags(write=False)
    return x, stride, out, refs


def _errs(got, want, refs):
    return max(np.abs(np.asarray(got[w], np.float64) - want[w]).max() / max(np.abs(r).max(), 1e-6)
               for w, r in enumerate(refs))


def _check(name, out, refs, ys, **kw):
    """out against the oracle at the bound of these windows (kw: pcen()'s keywords); prints both."""
    assert out.shape == (len(refs),) + refs[0].shape and np.isfinite(out).all()
    b = sim.bound(sim.e32("pcen", ys, refs, **kw)) if np.any(ys) else sim.CAP
    e = _errs(out, refs, refs)
    print(f"pcen windows {name}: max|new - oracle| / max|ref window| = {e:.3e} (bound {b:.1e})")
    for w, ref in enumerate(refs):
        np.testing.assert_allclose(out[w], ref, atol=b * max(np.abs(ref).max(), 1e-6), rtol=0)
    return b


# ---- parity ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_matches_oracle_and_per_window_kernel(name):
    _gpu()
    x, stride, out, refs = _case(name)
    assert out.shape == (len(refs), 101, 40) and len(refs) >= 1
    ys = _windows(x, stride, len(refs))
    b = _check(name, out, refs, ys)
    old = AudioPreprocessor().compute_pcen_batch(torch.from_numpy(ys).to(DEV)).cpu().numpy()
    print(f"pcen windows {name}: max|per-window kernel - oracle| = {_errs(old, refs, refs):.3e}   "
          f"max|new - per-window kernel| = {_errs(out, old, refs):.3e}   (/ max|ref window|)")
    for w, ref in enumerate(refs):
        atol = b * max(np.abs(ref).max(), 1e-6)
        np.testing.assert_allclose(old[w], ref, atol=atol, rtol=0)
        np.testing.assert_allclose(out[w], old[w], atol=atol, rtol=0)


def test_zero_recording_gives_exact_zeros():
    _gpu()
    _, _, out, refs = _case("zeros")
    assert len(refs) == 2 and not out.any() and not np.any(refs[0])


# ---- the smoother restarts, the edges are the window's own ---------------------------------------------
@functools.lru_cache(maxsize=None)
def _onset():
    x = _pcm(29, 56000).copy()
    x[16000:40000] = 0
    out = _new(x, 8000)
    out.setflags(write=False)
    return x, out


def test_silent_windows_between_loud_ones_are_exactly_zero():
    """Speech in [0, 16000) and from 40000 on, zeros between, stride 8000.  Window 2 = [16000, 32000) and
    window 3 = [24000, 40000) are all zeros: their shared neighbours are loud, the recording's frame at
    sample 16000 (window 2's left edge) holds speech, and a smoother carried over from window 0 or 1 would
    be far from 0 -- their own reflected edges and their own smoother give exact zeros."""
    _gpu()
    x, out = _onset()
    assert out.shape == (6, 101, 40)
    assert np.abs(x[15000:16000]).max() > 1000 and np.abs(x[40000:41000]).max() > 1000
    assert not out[2].any()
    assert not out[3].any()
    assert out[1].any() and out[4].any()


def test_onset_window_matches_the_oracle():
    """Window 4 = [32000, 48000): 8000 zeros, then speech -- the smoother starts at 0, so the gain at the
    onset is the largest of the set (the reference peaks near 4.6 against 1 to 2 on steady speech)."""
    _gpu()
    x, out = _onset()
    ys = _windows(x, 8000, 6)
    refs = [pcen_ref.pcen(y.astype(np.float64)) for y in ys]
    assert refs[4].max() > 3.0 and refs[4].max() > 1.5 * refs[0].max()
    _check("onset", out, refs, ys)


# ---- bitwise properties ------------------------------------------------------------------------------
def test_sharing_is_real_up_to_the_smoother():
    """q = 1: window w + 1 is window w one frame later.  Their outputs differ (each has its own smoother),
    so the shared thing is E -- visible where the smoother does not matter: s = 1 makes M = E."""
    _gpu()
    x, stride, _, _ = _case("stride160_21")
    out = _new(x, stride, AudioPreprocessor(pcen_params=dict(s=1.0)))
    for w in range(20):
        assert np.array_equal(out[w, 3:99], out[w + 1, 2:98]), w


def test_two_runs_are_bitwise_equal():
    _gpu()
    x, stride, out, _ = _case("stride160_21")
    assert np.array_equal(_new(x, stride), out)


@pytest.mark.parametrize("name,k", [("stride160_21", 1), ("stride160_21", 7), ("stride8000_5", 1)])
def test_position_independence(name, k):
    _gpu()
    x, stride, out, _ = _case(name)
    assert np.array_equal(_new(x[k * stride:].copy(), stride), out[k:])


def test_a_window_cut_out_of_the_middle():
    _gpu()
    for name, w in (("stride160_21", 10), ("stride8000_5", 2), ("stride400_11", 5)):
        x, stride, out, _ = _case(name)
        one = _new(x[w * stride:w * stride + WIN].copy(), stride)
        assert one.shape == (1, 101, 40) and np.array_equal(one[0], out[w]), (name, w)


def test_window_ranges_concatenate_to_the_whole():
    _gpu()
    x, stride, out, _ = _case("stride160_21")
    ap, pcm = AudioPreprocessor(), torch.from_numpy(x).to(DEV)
    parts = [ap.compute_pcen_windows(pcm, stride, first=f, count=3) for f in range(0, 21, 3)]
    assert np.array_equal(torch.cat(parts).cpu().numpy(), out)
    empty = ap.compute_pcen_windows(pcm, stride, first=21, count=0)
    assert empty.shape == (0, 101, 40) and empty.is_cuda
    x4, s4, out4, _ = _case("stride400_11")
    part = ap.compute_pcen_windows(torch.from_numpy(x4).to(DEV), s4, first=4, count=5)
    assert np.array_equal(part.cpu().numpy(), out4[4:9])
    x2, s2, out2, _ = _case("stride24000_2")
    part = ap.compute_pcen_windows(torch.from_numpy(x2).to(DEV), s2, first=1, count=1)
    assert np.array_equal(part.cpu().numpy(), out2[1:])


def test_gapped_windows_ignore_the_samples_between_them():
    """Stride 24000: samples 16000..23999 belong to no window; changing them changes nothing."""
    _gpu()
    x, stride, out, _ = _case("stride24000_2")
    y = x.copy()
    y[16000:24000] = 12345
    assert np.array_equal(_new(y, stride), out)


# ---- parameters ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", [dict(power=2), ALT], ids=["power2", "alt"])
def test_parameters(params):
    _gpu()
    x, stride, _, _ = _case("stride8000_5")
    ys = _windows(x, stride, 5)
    refs = [pcen_ref.pcen(y.astype(np.float64), **params) for y in ys]
    out = _new(x, stride, AudioPreprocessor(pcen_params=params))
    _check(f"stride8000_5 {params}", out, refs, ys, **params)


# ---- geometry -----------------------------------------------------------------------------------------
def _geo_ap(case, **kw):
    return AudioPreprocessor(n_fft=case.n_fft, hop_ms=case.hop // 16, n_mels=case.n_mels, n_dct_filters=case.n_dct,
                             **kw)


def _geo_kw(case):
    return dict(sr=fg.SR, n_fft=case.n_fft, hop=case.hop, n_mels=case.n_mels, fmin=fg.FMIN, fmax=fg.FMAX)


@pytest.mark.parametrize("which", ["shared", "unshared"])
@pytest.mark.parametrize("case", fg.WINDOWS, ids=repr)
def test_geometry(case, which):
    """129bands and 2048-16 are refused by the plan and take the per-window fallback; 128bands scans in
    256 / 128 = 2 segments; win300 has no interior frame (unshared at either stride)."""
    _gpu()
    stride = case.strides[which == "unshared"]
    x = fg.recording(case, stride)
    ap = _geo_ap(case)
    rc, plan = ap.pcen_windows_plan(len(x), stride, case.window, 0, case.n_windows)
    if rc == 0:
        assert plan.windows == case.n_windows and plan.frames == case.frames
        assert plan.shared == int(case.shared and which == "shared")
    else:  # (2048-16 at its unshared stride passes the plan; the call then refuses its LDS plan)
        assert rc == -2 and not case.kernel
    ys = _windows(x, stride, case.n_windows, case.window)
    refs = [pcen_ref.pcen(y.astype(np.float64), **_geo_kw(case)) for y in ys]
    out = _new(x, stride, ap, window=case.window)
    assert out.shape == (case.n_windows, case.frames, case.n_mels)
    _check(f"{case.id} {which}", out, refs, ys, **_geo_kw(case))
    if not case.kernel:
        # the fallback is the per-window kernel on the same float windows, here on its two-launch route
        # (129 bands, n_fft 2048: past the fused plan), which sums in a fixed order: the same bits
        old = ap.compute_pcen_batch(torch.from_numpy(ys).to(DEV)).cpu().numpy()
        assert np.array_equal(out, old)


# ---- memory contract ------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["shared", "unshared"])
@pytest.mark.parametrize("case_id", ["win16077", "320-80"])
def test_memory_contract(case_id, which):
    """The output and the (cached) workspace under the four fills, a fresh preprocessor per fill; then a
    long recording first and a shorter one on the same cached workspace, bit-equal to the shorter one on
    a fresh preprocessor; pcm is not modified."""
    _gpu()
    case = fg.WIN_BY_ID[case_id]
    stride = case.strides[which == "unshared"]
    x = fg.recording(case, stride)
    pcm = torch.from_numpy(x).to(DEV)
    short = pcm[:case.window + stride].contiguous()   # two windows
    rc, plan = _geo_ap(case).pcen_windows_plan(len(x), stride, case.window, 0, case.n_windows)
    assert rc == 0 and plan.shared == int(which == "shared") and plan.windows == case.n_windows

    def call():
        a = _geo_ap(case)
        whole = a.compute_pcen_windows(pcm, stride, window=case.window)
        again = a.compute_pcen_windows(short, stride, window=case.window)    # on the workspace `whole` left
        fresh = _geo_ap(case).compute_pcen_windows(short, stride, window=case.window)
        assert len(a._dev_ws) == 1 and a._dev_ws[str(pcm.device)].numel() >= plan.workspace_bytes
        return dict(whole=whole, again=again, fresh=fresh)

    r = four_fills(f"pcen windows {case_id} {which}", call, [pcm, short])
    assert pu.bits_equal(r["again"], r["fresh"])
    assert pu.bits_equal(r["again"], r["whole"][:2])
    ys = _windows(x, stride, case.n_windows, case.window)
    refs = [pcen_ref.pcen(y.astype(np.float64), **_geo_kw(case)) for y in ys]
    _check(f"{case_id} {which} (0xFF fill)", r["whole"], refs, ys, **_geo_kw(case))
    assert np.array_equal(pcm.cpu().numpy(), x)


# ---- capture ----------------------------------------------------------------------------------------------
def test_capturable():
    """The call inside torch.cuda.graph on a fixed buffer; the buffer refilled, one replay: the eager
    result on the second recording, bit for bit.  In a child under a timeout."""
    _gpu()
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "child.npz")
        try:
            p = subprocess.run([sys.executable, os.path.join(HERE, "pcen_windows_graph_child.py"), out],
                               capture_output=True, text=True, timeout=120)
        except subprocess.TimeoutExpired:
            pytest.exit("tests/pcen_windows_graph_child.py (graph capture / replay) hung: stopping the GPU run", 1)
        if p.returncode < 0 or p.returncode in (134, 139):
            pytest.exit(f"tests/pcen_windows_graph_child.py died with status {p.returncode}: stopping the GPU run\n"
                        f"{p.stderr[-3000:]}", 1)
        assert p.returncode == 0, p.stderr[-3000:]
        z = np.load(out)
        assert z["replay"].shape == (21, 101, 40) and np.array_equal(z["replay"], z["eager"])
        assert z["replay"].any()


# ---- the service --------------------------------------------------------------------------------------------
SERVICE_SEED = 35  # a 3 s recording; no window of it is a near tie at 500 or 100 ms (checked below)


def _service(tmp_path, no_cuda, labels=("_silence_", "_unknown_", "yes", "no")):
    torch.manual_seed(0)
    m = hm.SpeechModel(dict(hm.find_config("cnn-trad-pool2"), n_labels=len(labels)))
    fn = str(tmp_path / "m.pt")
    m.save(fn)
    return hs.TorchLabelService(fn, no_cuda=no_cuda, labels=list(labels), audio_preprocess_type="PCEN")


def _wav():
    return _pcm(SERVICE_SEED, 48000).tobytes()


def _no_ties(logits_fn, wav, stride_ms):
    """No window's top two probabilities (CPU, numpy PCEN) within 2e-4 of each other."""
    wins = list(hs.stride(wav, 32 * stride_ms, 32000))
    pcm = np.stack([np.frombuffer(w, np.int16) for w in wins]).astype(np.float32) / 32768.
    x = AudioPreprocessor().compute_pcen(pcm)
    with torch.no_grad():
        p = torch.softmax(logits_fn(x), 1).numpy()
    top = np.sort(p, 1)
    assert (top[:, -1] - top[:, -2] > 2e-4).all()
    return len(wins)


@pytest.mark.parametrize("stride_ms", [500, 100])
def test_label_stream_matches_label_batch(tmp_path, stride_ms):
    _gpu()
    wav = _wav()
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
    wav = _wav()
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


def test_label_stream_builds_no_float_windows(tmp_path, monkeypatch):
    """Peak device memory of label_stream up to the end of its front end, over what was allocated before
    the call: the int16 upload, the [21][101][40] output and nothing of the size of a [21][16000] float
    tensor (1,344,000 bytes; the parent's route also held a float copy of the recording).  Read when
    compute_pcen_windows returns, so the model's own buffers are not in the figure and need no slack; the
    slack is the allocator's rounding of each block (512 bytes) and the kernel-parameter struct: 64 KiB.
    The tables and the workspace are cached by a first call."""
    _gpu()
    wav = _wav()
    svc = _service(tmp_path, no_cuda=False)
    ap = svc.audio_processor
    svc.label_stream(wav, 100)
    rc, plan = ap.pcen_windows_plan(48000, 1600, 16000, 0, 21)
    assert rc == 0 and ap._dev_ws[str(torch.device(DEV))].numel() >= plan.workspace_bytes
    real, peaks, calls = ap.compute_pcen_windows, [], []

    def measured(pcm, *a, **kw):
        out = real(pcm, *a, **kw)
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated())
        calls.append((pcm.dtype, tuple(pcm.shape), tuple(out.shape)))
        return out

    monkeypatch.setattr(ap, "compute_pcen_windows", measured)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    got = svc.label_stream(wav, 100)
    assert len(got) == 21 and calls == [(torch.int16, (48000,), (21, 101, 40))]
    upload, out_bytes, slack = 2 * 48000, 21 * 101 * 40 * 4, 64 * 1024
    print(f"label_stream front end: peak {peaks[0] - base} bytes over the base; upload {upload} + output {out_bytes}")
    assert peaks[0] - base <= upload + out_bytes + slack
    assert 21 * 16000 * 4 > 2 * slack   # (the tensor that must not exist would not hide in the slack)
