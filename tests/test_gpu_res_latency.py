"""The latency schedule of the res forward (honk_res_forward_latency, SpeechResModel.honk_schedule
= "latency", TorchLabelService.honk_latency): batches of fewer clips than CUs run every block
layer split over all CUs (block16s_kernel).  The contract is tolerance-free: per output the
split kernel issues the throughput kernels' MFMAs in their order and the last layer's channel
sums are added in their order, so the logits are those of the throughput schedule's
stream-ordered forward BIT FOR BIT -- in every 16-bit mode, at every geometry, with and
without the f16x2 admission.

Shapes: the small ones are where a band / tile / class-row index can go wrong, so the models
and maps are res_geometry_cases' (W below one m-tile, W % 16 != 0, H % d != 0, H < d, pooled
maps, more rows than the workload's) plus the 19-map res15-narrow fixture (NT = 2), at batches
1, 3 and 17 (one clip, a few, more clips than dilation classes), and res15 at 101 x 40 on both
sides of the crossover (CU count - 1: split; CU count: the throughput schedule)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from honk_amd import _native
from honk_amd import service as hs
import res_geometry_cases as geo
from golden_util import load_fixture, load_range_fixture
from test_gpu_range import DEV, module

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BATCHES = (1, 3, 17)
# mode -> (honk_precision, environment)
MODES = {"bf16": ("bf16", {}), "bf16x3": ("bf16x3", {}), "f16x2": ("f16x2", {}),
         "f16x2-raw": ("f16x2", {"HONK_F16X2_RERUN": "0"})}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _native.load()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for v in geo.ENV_VARS + ("HONK_PRECISION",):
        monkeypatch.delenv(v, raising=False)


def _forward(m, x, schedule, capacity=None):
    """(logits, flagged count) of the stream-ordered forward of `schedule`."""
    m.honk_schedule, m.honk_stream_ordered, m.honk_rerun_capacity = schedule, True, capacity
    try:
        with torch.no_grad():
            out = m(torch.tensor(np.asarray(x)).to(DEV))
        torch.cuda.synchronize()
        assert m.honk_last_rerun is None and m.honk_last_rerun_dev.dtype == torch.int32
        return out.cpu().numpy(), int(m.honk_last_rerun_dev)
    except RuntimeError as e:
        if "hip" in str(e).lower() or "illegal" in str(e).lower():
            pytest.exit(f"GPU error in {m.honk_precision} / {schedule} on {tuple(np.shape(x))}: {e}", returncode=3)
        raise
    finally:
        m.honk_schedule, m.honk_stream_ordered, m.honk_rerun_capacity = "throughput", False, None


def _both(m, x, capacity=None):
    return _forward(m, x, "throughput", capacity), _forward(m, x, "latency", capacity)


def _clips(seed, B, H, W):
    return np.random.Generator(np.random.PCG64(seed)).standard_normal((B, H, W)).astype(np.float32)


def _geo_module(case, prec):
    cfg, params, _ = geo.build(case)
    m = module(cfg, params, case.model, prec)
    m.honk_reroute = False  # the kernels of `prec` themselves, whatever the policy
    return m


@pytest.mark.parametrize("case", geo.CASES, ids=repr)
def test_bitwise_equal_to_the_throughput_schedule(monkeypatch, case):
    x = _clips(case.seed + 1000, max(BATCHES), case.H, case.W)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    split = 0
    for mode, (prec, env) in MODES.items():
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        m = _geo_module(case, prec)
        for B in BATCHES:
            plan = [k for k, _ in _native.res_latency_plan(m._desc(case.H, case.W), B, cus)]
            split += plan.count("block16s_kernel")
            (thr, n_thr), (lat, n_lat) = _both(m, x[:B])
            assert np.isfinite(thr).all()
            assert np.array_equal(lat, thr), (mode, B, plan, float(np.abs(lat - thr).max()))
            assert n_lat == n_thr
        for k in env:
            monkeypatch.delenv(k)
    assert split > 0  # the case ran the split kernel in some mode


def test_bitwise_on_the_narrow_model(monkeypatch):
    """19 maps (NT = 2): f16x2 runs the weight-stationary family, bf16 / bf16x3 the row-band
    kernel (whose arithmetic the split kernel then reproduces: bias table, residual by selection
    MFMA, one partial per m-tile); f16x2's re-run rounds are row-band bf16x3 too."""
    cfg, params, x, _, meta = load_fixture("res15-narrow-mfcc")
    xs = np.concatenate([x] * (17 // len(x) + 1))[:17] * np.linspace(0.5, 2.0, 17, dtype=np.float32)[:, None, None]
    xs[[1, 5]] *= 3000  # out of calibration: f16x2 re-runs them (test_gpu_ordered's row-band re-run)
    for mode, (prec, env) in MODES.items():
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        m = module(cfg, params, meta["model"], prec)
        m.honk_reroute = False
        assert _native.res_launch_plan(m._desc(101, 40), 3, 256) == [
            "block16w_kernel" if prec == "f16x2" else "block16r_kernel"] * 13
        assert {k for k, _ in _native.res_latency_plan(m._desc(101, 40), 3, 256)} == {"block16s_kernel"}
        for B in BATCHES:
            (thr, n_thr), (lat, n_lat) = _both(m, xs[:B])
            assert np.array_equal(lat, thr) and n_lat == n_thr, (mode, B)
            assert n_lat == (2 if mode == "f16x2" and B == 17 else 1 if mode == "f16x2" and B == 3 else 0), (mode, B)
        for k in env:
            monkeypatch.delenv(k)


@pytest.fixture(scope="module")
def res15():
    cfg, params, x, logits, meta = load_fixture("res15-b3-mfcc")
    return cfg, params, x, logits


@pytest.mark.parametrize("mode", list(MODES))
def test_both_sides_of_the_crossover(monkeypatch, res15, mode):
    """res15 at 101 x 40 with one clip fewer than the device has CUs (split) and with as many (the
    throughput schedule): both equal the throughput logits."""
    cfg, params, x, _ = res15
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    prec, env = MODES[mode]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = module(cfg, params, "res15", prec)
    m.honk_reroute = False
    d = m._desc(101, 40)
    assert {k for k, _ in _native.res_latency_plan(d, cus - 1, 0)} == {"block16s_kernel"}
    assert [k for k, _ in _native.res_latency_plan(d, cus, 0)] == _native.res_launch_plan(d, cus, 0)
    xs = np.concatenate([x] * (cus // len(x) + 1))[:cus] * np.linspace(0.5, 1.5, cus, dtype=np.float32)[:, None, None]
    (thr, n_thr), (lat, n_lat) = _both(m, xs)
    assert np.array_equal(lat, thr) and n_lat == n_thr
    (thr1, _), (lat1, _) = _both(m, xs[:cus - 1])
    assert np.array_equal(lat1, thr1)
    assert np.array_equal(thr1, thr[:cus - 1])  # (a clip's logits do not depend on the batch around it)


@pytest.mark.parametrize("name", ["res15", "res8"])
def test_parity_with_the_oracle_fixture(name):
    """auto through the latency schedule within the project's 1e-4 of the reference-written logits
    (follows from the equality above; kept so that a break of both schedules cannot hide)."""
    cfg, params, x, logits, meta = load_fixture(name)
    m = module(cfg, params, meta["model"], "auto")
    lat, _ = _forward(m, x, "latency")
    err = float(np.abs(lat - logits).max())
    print(f"{name}: auto -> {m.honk_last_precision}, latency schedule max|err| = {err:.2e}")
    np.testing.assert_allclose(lat, logits, atol=1e-4, rtol=0)


def test_admission(res15):
    """The benign + out-of-calibration batch of test_gpu_range / test_gpu_ordered at 6 clips: the
    flagged count and the logits of the throughput schedule's ordered forward, at the default
    capacity and at capacity 1 (the flagged clips past it keep their f16x2 logits)."""
    cfg, params, x, _ = res15
    _, _, x_ood, _, _ = load_range_fixture("res15-ood")
    mixed = np.stack([x[0], x_ood[0], x[1], x_ood[1], x[2], x_ood[2]])
    m = module(cfg, params, "res15")
    _forward(m, x, "throughput")  # the policy's probe sees the calibrated batch
    assert m.honk_last_precision == "f16x2"
    for cap in (None, 1):
        (thr, n_thr), (lat, n_lat) = _both(m, mixed, cap)
        assert n_thr == n_lat == 3
        assert np.array_equal(lat, thr), cap
    full, _ = _forward(m, mixed, "latency")
    one, _ = _forward(m, mixed, "latency", 1)
    assert np.array_equal(one[[0, 1, 2, 4]], full[[0, 1, 2, 4]]) and not np.array_equal(one[[3, 5]], full[[3, 5]])


def test_c_abi(res15):
    """honk_res_forward_latency itself: a workspace of exactly honk_res_latency_workspace_bytes
    with a sentinel tail behind it (untouched), logits pre-filled with NaN (all written), and
    batch 0 (0 written to flagged_count, nothing else)."""
    lib = _native.load()
    cfg, params, x, _ = res15
    m = module(cfg, params, "res15", "f16x2")
    m.honk_reroute = False
    want, n_want = _forward(m, x, "throughput")
    xd = torch.as_tensor(x).to(DEV)
    desc, packed = m._desc(101, 40, "f16x2"), m._packed(xd)
    B, TAIL = len(x), 4096
    ws_bytes = lib.honk_res_latency_workspace_bytes(ctypes.byref(desc), B)
    assert ws_bytes >= lib.honk_res_workspace_bytes(ctypes.byref(desc), B) > 0
    ws = torch.full((ws_bytes + TAIL,), 0xA5, dtype=torch.uint8, device=DEV)
    out = torch.full((B, 12), float("nan"), device=DEV)
    cnt = torch.full((), 7, dtype=torch.int32, device=DEV)
    st = _native.stream_handle(xd.device)
    _native.check(lib.honk_res_forward_latency(ctypes.byref(desc), packed.data_ptr(), xd.data_ptr(), out.data_ptr(), B,
                                               ws.data_ptr(), ws_bytes, st, 0, cnt.data_ptr()),
                  "honk_res_forward_latency")
    torch.cuda.synchronize()
    assert bool((ws[ws_bytes:] == 0xA5).all())
    got = out.cpu().numpy()
    assert np.isfinite(got).all() and np.array_equal(got, want) and int(cnt) == n_want == 0
    # one byte short: refused, nothing enqueued
    assert lib.honk_res_forward_latency(ctypes.byref(desc), packed.data_ptr(), xd.data_ptr(), out.data_ptr(), B,
                                        ws.data_ptr(), ws_bytes - 1, st, 0, None) != 0
    cnt.fill_(7)
    out.fill_(float("nan"))
    _native.check(lib.honk_res_forward_latency(ctypes.byref(desc), packed.data_ptr(), xd.data_ptr(), out.data_ptr(), 0,
                                               ws.data_ptr(), ws_bytes, st, 0, cnt.data_ptr()),
                  "honk_res_forward_latency")
    torch.cuda.synchronize()
    assert int(cnt) == 0 and bool(torch.isnan(out).all())


# ---- graph capture: in a child process under a timeout ---------------------------------
@pytest.fixture(scope="module")
def graph_child(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("latency_graph")
    out = str(tmp / "child.npz")
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "res_latency_graph_child.py"), out, str(tmp)],
                           capture_output=True, text=True, timeout=240)
    except subprocess.TimeoutExpired:
        pytest.exit("tests/res_latency_graph_child.py (graph capture / replay) hung: stopping the GPU run", 1)
    if p.returncode < 0 or p.returncode in (134, 139):
        pytest.exit(f"tests/res_latency_graph_child.py died with status {p.returncode}: stopping the GPU run\n"
                    f"{p.stderr[-3000:]}", 1)
    assert p.returncode == 0, p.stderr[-3000:]
    return np.load(out)


def test_graph_replays_equal_the_eager_latency_forward(graph_child):
    z = graph_child
    assert str(z["precision"]) == "f16x2" and int(z["schedule_kept"]) == 1
    for k, flagged in (("a", 0), ("ood", 1), ("b", 0)):
        assert int(z["graph_count_" + k]) == int(z["eager_count_" + k]) == flagged
        assert np.array_equal(z["graph_" + k], z["eager_" + k]), k
    assert not np.array_equal(z["graph_a"], z["graph_b"])


def test_label_service_graph_of_the_latency_schedule(graph_child):
    z = graph_child
    labels, probs = z["svc_labels"], z["svc_probs"]
    assert str(z["svc_schedule"]) == "latency" and int(z["svc_capture_kept"]) == 1
    assert len(set(labels.tolist())) == 1 and len(set(probs.tolist())) == 1


def test_label_service(res15, tmp_path):
    """TorchLabelService with a res model: label() and label_stream() on a 3 s seeded recording
    answer exactly as with honk_latency=False.  (label()'s batched MFCC call is not bit-for-bit
    repeatable from call to call -- measured with honk_latency False both times -- so the first
    window's MFCC is computed once and both services' label() are fed that map; label_stream's
    strided-window front end is repeatable and runs as it ships.)"""
    import test_callers as tc
    from honk_amd.audio import AudioPreprocessor
    from test_mfcc_windows_abi import _pcm
    cfg, params, x, _ = res15
    _, svc = tc._service(tmp_path, no_cuda=False)
    assert svc.honk_latency is False

    class Front(AudioPreprocessor):
        first = None

        def compute_mfccs_batch(self, pcm):
            if self.first is None:
                self.first = super().compute_mfccs_batch(pcm).clone()
            return self.first.clone()

    lat_svc = hs.TorchLabelService(svc.model_filename, labels=svc.labels, honk_latency=True, audio_processor=Front())
    assert lat_svc.honk_latency is True
    pcm = _pcm(21, 3 * 16000).tobytes()
    res = {}
    for latency in (False, True):
        m = module(cfg, params, "res15")
        lat_svc.model, lat_svc.labels, lat_svc.honk_latency = m, [str(i) for i in range(12)], latency
        res[latency] = (lat_svc.label(pcm[:2 * 16000]), lat_svc.label_stream(pcm),
                        hs.StreamListener(lat_svc).feed(pcm))
        assert m.honk_schedule == ("latency" if latency else "throughput")
    assert len(res[True][1]) == 5 and res[True][2] == res[True][1]
    assert res[True][0][0] == res[False][0][0] and float(res[True][0][1]) == float(res[False][0][1])
    assert res[True][1] == res[False][1] and res[True][2] == res[False][2]
