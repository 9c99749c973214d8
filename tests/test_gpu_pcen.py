"""honk_pcen_f32 (csrc/pcen.hip) on the GPU: the fused route (one launch, the MFMA spectrum stage
shared with the MFCC kernel) and the long route (mel energies, then a segmented scan in place)
against the float64 restatement tests/pcen_ref.py, and the callers: compute_pcen_batch,
DeviceSpeechDataset, train(), TorchLabelService.

PARITY UNPINNED (the reference's ``pcen`` package is absent).  Bound: the front-end bound of
tests/frontend_geometry_cases.py -- 16 x the error of the float32 restatement oracle/frontend_f32_sim.py
against the same reference on the same clips, never above 1e-4; atol = bound * max(max|ref clip|, 1e-6),
rtol = 0, for a device result against the reference and for two device results against each other.
Inputs: pcen_ref.clips (speech-like, all-zero, an onset after 8000 zeros,
1e-3 x speech-like)."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import pcen_ref
from honk_amd import _native
from honk_amd import data as hdata
from honk_amd import model as hm
from honk_amd import service as hs
from honk_amd import train as htr
from honk_amd.audio import AudioPreprocessor, mel_filterbank
from oracle import frontend_f32_sim as sim
from test_mfcc_windows_abi import _pcm

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"
ALT = dict(s=0.1, alpha=0.8, delta=1.0, r=0.25)


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _run(ys, **kw):
    out = AudioPreprocessor(**kw).compute_pcen_batch(torch.from_numpy(np.ascontiguousarray(ys)).to(DEV))
    assert out.is_cuda and out.dtype == torch.float32
    return out.cpu().numpy()


def _rel(ys, ref, **kw):
    """The bound of these clips: kw are pcen()'s keywords (n_fft, n_mels, the PCEN parameters)."""
    return sim.bound(sim.e32("pcen", ys, ref, **kw))


def _report(name, got, ref, rel):
    worst = pcen_ref.check(got, ref, rel)
    print(f"pcen {name}: max |err| / max|ref clip| = {worst:.3e} (bound {rel:.1e})")


def test_fused_route_matches_reference():
    _gpu()
    ys, ref = pcen_ref.clips(), pcen_ref.ref_clips()
    got = _run(ys)
    assert got.shape == (8, 101, 40)
    _report("fused S=16000", got, ref, _rel(ys, ref))
    assert np.all(got[pcen_ref.ZERO_CLIP] == 0.0)


@pytest.mark.parametrize("S,frames", [(1600, 11), (16077, 101), (17920, 113)])
def test_edge_shapes(S, frames):
    """11 frames: one partly filled frame tile; S no multiple of hop; 113 frames: past the fused
    limit, so the first call of this shape takes the long route."""
    _gpu()
    ys, ref = pcen_ref.clips(S), pcen_ref.ref_clips(S)
    got = _run(ys)
    assert got.shape == (8, frames, 40)
    _report(f"S={S}", got, ref, _rel(ys, ref))
    assert np.all(got[pcen_ref.ZERO_CLIP] == 0.0)


def test_twenty_mel_bands():
    _gpu()
    ys, ref = pcen_ref.clips(), pcen_ref.ref_clips(n_mels=20)
    got = _run(ys, n_mels=20)
    assert got.shape == (8, 101, 20)
    _report("n_mels=20", got, ref, _rel(ys, ref, n_mels=20))


@pytest.mark.parametrize("S,frames", [(18080, 114), (48000, 301)])
def test_long_route_matches_reference(S, frames):
    """114 frames: the first shape past the fused kernel; 301 frames: 32 scan segments of 10 frames."""
    _gpu()
    ys, ref = pcen_ref.clips(S), pcen_ref.ref_clips(S)
    got = _run(ys)
    assert got.shape == (8, frames, 40)
    _report(f"long S={S}", got, ref, _rel(ys, ref))
    assert np.all(got[pcen_ref.ZERO_CLIP] == 0.0)


def test_long_route_matches_fused_route(monkeypatch):
    _gpu()
    ys, ref = pcen_ref.clips(), pcen_ref.ref_clips()
    fast = _run(ys)
    monkeypatch.setenv("HONK_MFCC_VALU", "1")
    slow = _run(ys)
    rel = _rel(ys, ref)
    _report("long S=16000", slow, ref, rel)
    for i in range(len(ys)):
        scale = max(np.abs(ref[i]).max(), 1e-6)
        np.testing.assert_allclose(slow[i], fast[i], atol=rel * scale, rtol=0)
    assert np.all(slow[pcen_ref.ZERO_CLIP] == 0.0)


def test_long_route_fewer_frames_than_segments(monkeypatch):
    """11 frames on the long route: segments of one frame, 21 of the 32 empty."""
    _gpu()
    monkeypatch.setenv("HONK_MFCC_VALU", "1")
    ys, ref = pcen_ref.clips(1600), pcen_ref.ref_clips(1600)
    got = _run(ys)
    _report("long S=1600", got, ref, _rel(ys, ref))
    assert np.all(got[pcen_ref.ZERO_CLIP] == 0.0)


def test_c_abi_n_fft_400():
    """n_fft = 400 through the C ABI, params NULL = the defaults."""
    _gpu()
    n_fft, hop, n_mels = 400, 160, 40
    ys, ref = pcen_ref.clips(), pcen_ref.ref_clips(n_fft=n_fft)
    pcm = torch.from_numpy(ys).to(DEV)
    win = torch.from_numpy(pcen_ref.window(n_fft).astype(np.float32)).to(DEV)
    mel = torch.from_numpy(mel_filterbank(16000, n_fft, n_mels, 20, 4000)).to(DEV)
    out = torch.full((8, 101, n_mels), float("nan"), device=DEV)
    rc = _native.load().honk_pcen_f32(pcm.data_ptr(), 8, 16000, win.data_ptr(), n_fft, hop, mel.data_ptr(), n_mels,
                                      None, out.data_ptr(), _native.stream_handle(pcm.device))
    _native.check(rc, "honk_pcen_f32")
    _report("n_fft=400", out.cpu().numpy(), ref, _rel(ys, ref, n_fft=n_fft))


@pytest.mark.parametrize("params", [dict(power=2), ALT], ids=["power2", "alt"])
@pytest.mark.parametrize("route", ["fused", "long"])
def test_parameters(monkeypatch, route, params):
    _gpu()
    if route == "long":
        monkeypatch.setenv("HONK_MFCC_VALU", "1")
    ys, ref = pcen_ref.clips(), pcen_ref.ref_clips(**params)
    got = _run(ys, pcen_params=params)
    _report(f"{route} {params}", got, ref, _rel(ys, ref, **params))
    assert np.all(got[pcen_ref.ZERO_CLIP] == 0.0)


def test_capturable():
    """compute_pcen_batch inside a torch.cuda.CUDAGraph on a fixed buffer; the buffer refilled, one
    replay: the eager output on the second set of clips, bit for bit.  In a child under a timeout."""
    _gpu()
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "child.npz")
        try:
            p = subprocess.run([sys.executable, os.path.join(HERE, "pcen_graph_child.py"), out],
                               capture_output=True, text=True, timeout=120)
        except subprocess.TimeoutExpired:
            pytest.exit("tests/pcen_graph_child.py (graph capture / replay) hung: stopping the GPU run", 1)
        if p.returncode < 0 or p.returncode in (134, 139):
            pytest.exit(f"tests/pcen_graph_child.py died with status {p.returncode}: stopping the GPU run\n"
                        f"{p.stderr[-3000:]}", 1)
        assert p.returncode == 0, p.stderr[-3000:]
        z = np.load(out)
        assert z["replay"].shape == (4, 101, 40) and np.array_equal(z["replay"], z["eager"])
        pcen_ref.check(z["replay"], pcen_ref.ref_clips()[4:8], _rel(pcen_ref.clips()[4:8], pcen_ref.ref_clips()[4:8]))


def test_clip_is_independent_of_its_batch():
    _gpu()
    ys, ref = pcen_ref.clips(), pcen_ref.ref_clips()
    pick = [6, 0, 7]  # the onset clip, a steady one, the quiet one
    small, big = _run(ys[pick]), _run(ys)
    rel = _rel(ys, ref)
    for j, i in enumerate(pick):
        scale = max(np.abs(ref[i]).max(), 1e-6)
        np.testing.assert_allclose(small[j], big[i], atol=rel * scale, rtol=0)


# ---- the data path and train() -------------------------------------------------------------------
def _dataset(clips, st, front_end, seed, **kw):
    cfg = dict(input_length=16000, timeshift_ms=100, noise_prob=0.8, silence_prob=0.1, cache_size=32,
               n_mels=40, n_dct_filters=40, audio_preprocess_type=front_end)
    return hdata.DeviceSpeechDataset(clips, st, cfg, device=DEV, rng=random.Random(seed), **kw)


def test_device_batch_is_augment_then_pcen():
    _gpu()
    g = np.random.default_rng(8)
    clips = {f"c{i}.wav": (pcen_ref.clips()[i % 8][:16000 - 13 * i], 2 + i % 3) for i in range(10)}
    bg = [(g.standard_normal(30000) * 0.1).astype(np.float32)]
    a, b = (_dataset(clips, hdata.DatasetType.TRAIN, "PCEN", 5, bg_noise_audio=bg) for _ in range(2))
    assert a.audio_preprocess_type == "PCEN"
    idx = torch.tensor([3, 0, 10, 7, 9, 3])  # (10: a silence item)
    x = hdata.batch_input(a, idx)
    want = b.audio_processor.compute_pcen_batch(b.augment_batch(idx))
    assert x.is_cuda and tuple(x.shape) == (6, 101, 40) and torch.isfinite(x).all()
    assert torch.equal(x, want)  # (the same draws, and the fused kernel sums in a fixed order)
    m = _dataset(clips, hdata.DatasetType.TRAIN, "MFCCs", 5, bg_noise_audio=bg)
    assert not torch.equal(m.device_batch(idx), x)
    with pytest.raises(ValueError):
        _dataset(clips, hdata.DatasetType.TRAIN, "bogus", 5)


def test_train_on_device_dataset_pcen(tmp_path, capsys):
    """tests/test_device_data.py::test_gpu_train_on_device_dataset with the PCEN front end."""
    _gpu()
    import warnings
    g = np.random.default_rng(4)
    clips = {f"c{i}.wav": ((g.standard_normal(16000 - 11 * i) * 0.2).astype(np.float32), 2 + i % 10)
             for i in range(48)}
    cfg_ds = dict(input_length=16000, timeshift_ms=100, noise_prob=0.8, silence_prob=0.1, cache_size=32,
                  n_mels=40, n_dct_filters=40, audio_preprocess_type="PCEN")
    bg = [(g.standard_normal(30000) * 0.5).astype(np.float32)]
    mk = lambda st: hdata.DeviceSpeechDataset(clips, st, cfg_ds, bg_noise_audio=bg, device="cuda:0",  # noqa: E731
                                              rng=random.Random(2))
    cfg = dict(hm.find_config("res8-narrow"))
    cfg.update(htr.default_run_config(str(tmp_path / "m.pt")))
    cfg.update(no_cuda=False, gpu_no=0, n_epochs=2, dev_every=1, batch_size=16, lr=[0.05], schedule=[])
    cfg.update(audio_preprocess_type="PCEN")
    cfg["model_class"] = hm.find_model("res8-narrow")
    torch.manual_seed(0)
    init = str(tmp_path / "init.pt")   # evaluate()'s model if no dev accuracy beats 0 (reference quirk)
    hm.find_model("res8-narrow")(cfg).save(init)
    cfg["input_file"] = init
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)   # every stage native
        htr.train(cfg, datasets=(mk(hdata.DatasetType.TRAIN), mk(hdata.DatasetType.DEV), mk(hdata.DatasetType.TEST)))
    out = capsys.readouterr().out
    assert "train step #" in out and "final test accuracy" in out
    losses = [float(v) for v in re.findall(r"loss: (\S+)", out)]
    assert losses and all(np.isfinite(losses))


# ---- serving ------------------------------------------------------------------------------------------
def _service(tmp_path, no_cuda):
    labels = ["_silence_", "_unknown_", "yes", "no"]
    torch.manual_seed(0)
    m = hm.SpeechModel(dict(hm.find_config("cnn-trad-pool2"), n_labels=len(labels)))
    fn = str(tmp_path / "m.pt")
    m.save(fn)
    return hs.TorchLabelService(fn, no_cuda=no_cuda, labels=labels, audio_preprocess_type="PCEN")


def _close(got, want, tol=1e-4):
    assert len(got) == len(want) > 0
    for (lg, pg), (lw, pw) in zip(got, want):
        assert lg == lw and abs(pg - pw) < tol


def test_service_matches_cpu_service(tmp_path):
    _gpu()
    gpu, cpu = _service(tmp_path, False), _service(tmp_path, True)
    wins = [_pcm(s, 16000).tobytes() for s in range(4)]
    _close(gpu.label_batch(wins), cpu.label_batch(wins))
    _close([gpu.label(wins[0])], [cpu.label(wins[0])])
    assert gpu._model_input(wins).is_cuda


def test_label_stream_matches_label_batch(tmp_path):
    _gpu()
    gpu = _service(tmp_path, False)
    wav = _pcm(5, 40000).tobytes()  # 2.5 s: 4 windows at 0.5 s
    wins = list(hs.stride(wav, 16000, 32000))
    assert len(wins) == 4
    _close(gpu.label_stream(wav), gpu.label_batch(wins))
    _close(gpu.label_stream(wav, max_windows=3), gpu.label_batch(wins))
    _close(gpu.label_stream(wav), _service(tmp_path, True).label_batch(wins))
