"""The latency schedule of the SpeechModel (cnn-*) forward (honk_cnn_forward_latency,
SpeechModel.honk_schedule = "latency", SpeechModel.honk_capture, TorchLabelService on the model
reload() builds): chunks of fewer clips than honk_cnn_latency_threshold run the dedicated convs as
their split forms and the long Linears split over K.

a. the conv stack (honk_cnn_features_f32) of the latency schedule is BIT FOR BIT the throughput
   schedule's, at every geometry of cnn_geometry_cases, both precisions, batches 1 / 3 / 17;
b. the logits are within the project's 1e-4 of the float64 oracle (the split-K sums are
   associated differently from the throughput Linears', so there is no bitwise claim here);
c. a clip's latency logits do not depend on the batch around it (bitwise at 1, 3, 17), and a
   repeated call repeats them;
d. trad-72x40 on both sides of the threshold: split below it, the throughput plan and
   honk_cnn_forward's very logits at it;
e. the split-K Linear alone (honk_linear_splitk_f32) against float64 numpy, at the bound
   test_gpu_parity.test_linear_small_n_abi holds the GEMV to;
f. the C ABI: exact workspace with a sentinel tail, NaN-filled logits, 0x00 / 0xFF workspace
   fills (bit-equal logits), one byte short, batch 0;
g. graph capture and the label service, in a child process under a timeout.

cgeo.oracle covers the clips compared at batches 1, 3 and 300; batch 17 compares
cgeo.compared(17), whose oracle logits come from the same orc.forward on the same clips."""
import contextlib
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from honk_amd import _native
from honk_amd import model as hm
from oracle import ref_numpy as orc
import cnn_geometry_cases as cgeo

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"
BATCHES = (1, 3, 17)
SPLIT_KINDS = tuple(_native.CNN_SPLIT_OF.values())
TAIL = 4096


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _native.load()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for v in cgeo.ENV_VARS + ("HONK_CNN_SPLITK_SLICE",):
        monkeypatch.delenv(v, raising=False)


_MODULES = {}


def _module(case, prec):
    key = (case.id, prec)
    if key not in _MODULES:
        cfg, params, _ = cgeo.build(case)
        m = hm.find_model(case.model)(cfg)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
        m = m.eval().to(DEV)
        m.honk_precision = prec
        _MODULES[key] = m
    return _MODULES[key]


def _desc(m, prec):
    return _native.CnnDesc(**m._honk_desc, precision=_native.PRECISIONS[prec])


@contextlib.contextmanager
def _device_errors_end_the_run(what):
    try:
        yield
    except RuntimeError as e:
        if "hip" in str(e).lower() or "illegal" in str(e).lower():
            pytest.exit(f"GPU error in {what}: {e}", returncode=3)
        raise


def _forward(m, x, schedule):
    m.honk_schedule = schedule
    try:
        with _device_errors_end_the_run(f"{m.honk_precision} / {schedule} on {tuple(np.shape(x))}"):
            with torch.no_grad():
                out = m(torch.tensor(np.asarray(x)).to(DEV))
            torch.cuda.synchronize()
            return out.cpu().numpy()
    finally:
        m.honk_schedule = "throughput"


def _tensors(m):
    return [t.detach().contiguous() if t is not None else None for t in m._native_tensors()]


def _features(m, prec, x, latency):
    lib, d = _native.load(), _desc(m, prec)
    B = len(x)
    flat = (m.lin if hasattr(m, "lin") else m.dnn1 if m.tf_variant and hasattr(m, "dnn1") else m.output).in_features
    need = lib.honk_cnn_latency_workspace_bytes(ctypes.byref(d), B)
    assert need >= lib.honk_cnn_workspace_bytes(ctypes.byref(d), B) > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.full((B, flat), float("nan"), device=DEV)
    xd, ts = torch.tensor(np.asarray(x)).to(DEV), _tensors(m)
    with _device_errors_end_the_run(f"features {prec} latency={latency} on {tuple(xd.shape)}"), torch.cuda.device(DEV):
        _native.check(lib.honk_cnn_features_f32(ctypes.byref(d), _native.ptr_array(ts), xd.data_ptr(), out.data_ptr(), B,
                                                ws.data_ptr(), need, _native.stream_handle(torch.device(DEV)),
                                                int(latency)), "honk_cnn_features_f32")
        torch.cuda.synchronize()
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _oracle17(case):
    """float64 oracle logits of cgeo.compared(17) (cgeo.reference holds the clips of its own batches)."""
    cfg, params, x = cgeo.build(case)
    return orc.forward(params, cfg, x[cgeo.compared(17)])


def _oracle(case, B):
    return _oracle17(case) if B == 17 else cgeo.oracle(case, B)


@pytest.mark.parametrize("prec", cgeo.PRECS)
@pytest.mark.parametrize("case", cgeo.CASES, ids=repr)
def test_conv_stack_bit_for_bit(case, prec):
    """(a)"""
    m = _module(case, prec)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    x = cgeo.build(case)[2]
    ran_split = 0
    for B in BATCHES:
        plan = [k for k, _ in _native.cnn_latency_plan(_desc(m, prec), B, cus)]
        ran_split += sum(plan.count(k) for k in SPLIT_KINDS)
        thr, lat = _features(m, prec, x[:B], 0), _features(m, prec, x[:B], 1)
        assert np.isfinite(thr).all()
        assert np.array_equal(lat, thr), (B, plan, float(np.abs(lat - thr).max()))
    if case.fast(prec):  # a trad-class case: its dedicated kernels ran as their split forms
        assert ran_split == len(BATCHES) * len(case.fast(prec)), ran_split
    else:
        assert ran_split == 0


@pytest.mark.parametrize("prec", cgeo.PRECS)
@pytest.mark.parametrize("case", cgeo.CASES, ids=repr)
def test_logits_vs_oracle_and_batch_invariance(case, prec):
    """(b), (c)"""
    m = _module(case, prec)
    x = cgeo.build(case)[2]
    outs = {}
    for B in BATCHES:
        out = outs[B] = _forward(m, x[:B], "latency")
        assert out.shape == (B, cgeo.config(case)["n_labels"]) and np.isfinite(out).all()
        ref = _oracle(case, B)
        err = float(np.abs(out[cgeo.compared(B)] - ref).max())
        print(f"{case} {prec} B={B} latency: max|logit - oracle| {err:.2e} (float32 oracle {case.f32_err:.1e})")
        assert err <= cgeo.ATOL
    assert np.array_equal(outs[1], outs[17][:1]) and np.array_equal(outs[3], outs[17][:3])
    assert np.array_equal(_forward(m, x[:17], "latency"), outs[17])


@pytest.mark.parametrize("prec", cgeo.PRECS)
def test_both_sides_of_the_threshold(prec):
    """(d)"""
    case = cgeo.BY_ID["trad-72x40"]
    m = _module(case, prec)
    d = _desc(m, prec)
    thr = _native.cnn_latency_threshold(d, 0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert 1 < thr <= min(cus, cgeo.BMAX)
    x = cgeo.build(case)[2]
    below = [k for k, _ in _native.cnn_latency_plan(d, thr - 1, 0)]
    assert [k for k in below if k in SPLIT_KINDS] == [_native.CNN_SPLIT_OF[k] for k in case.fast(prec)]
    assert "linear_splitk_kernel" in below
    assert [k for k, _ in _native.cnn_latency_plan(d, thr, 0)] == _native.cnn_launch_plan(d)
    at = _forward(m, x[:thr], "latency")
    assert np.array_equal(at, _forward(m, x[:thr], "throughput"))
    under = _forward(m, x[:thr - 1], "latency")
    assert np.array_equal(_features(m, prec, x[:thr - 1], 1), _features(m, prec, x[:thr - 1], 0))
    idx = cgeo.compared(cgeo.BMAX)[:7]  # the oracle's clips below the threshold
    idx = [i for i in idx if i < thr - 1]
    ref = np.stack([cgeo.reference(case)[i] for i in idx])
    assert float(np.abs(under[idx] - ref).max()) <= cgeo.ATOL
    assert float(np.abs(at[idx] - ref).max()) <= cgeo.ATOL


def _slice_len(n):
    """The split-K slice length of an n-output Linear: honk_linear_splitk_slices turns positive at
    K = two slices."""
    lib = _native.load()
    lo, hi = 1, 1 << 20
    assert lib.honk_linear_splitk_slices(hi, n) > 0 and lib.honk_linear_splitk_slices(lo, n) == 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if lib.honk_linear_splitk_slices(mid, n) > 0 else (mid, hi)
    assert hi % 2 == 0 and lib.honk_linear_splitk_slices(hi, n) == 2
    return hi // 2


@pytest.mark.parametrize("kname", ["slice-1", "slice", "slice+1", "6510", "26624"])
def test_split_k_linear_alone(kname):
    """(e) m in {1, 3, 17} x n in {1, 4, 5, 16, 17, 32, 128} x relu on / off at one K."""
    lib = _native.load()
    st = _native.stream_handle(torch.device(DEV))
    for n in (1, 4, 5, 16, 17, 32, 128):
        sl = _slice_len(n)
        k = {"slice-1": sl - 1, "slice": sl, "slice+1": sl + 1}.get(kname) or int(kname)
        g = torch.Generator().manual_seed(1000 * n + k)
        x = torch.randn(17, k, generator=g)
        w = torch.randn(n, k, generator=g) / k ** 0.5
        b = torch.randn(n, generator=g)
        ref = torch.nn.functional.linear(x.double(), w.double(), b.double())
        xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
        for m in (1, 3, 17):
            need = lib.honk_linear_splitk_workspace_bytes(m, k, n)
            assert need == -(-k // sl) * m * n * 4 and need >= lib.honk_linear_splitk_slices(k, n) * m * n * 4
            for relu in (0, 1):
                ws = torch.full((need + TAIL,), 0xA5, dtype=torch.uint8, device=DEV)
                y = torch.full((m, n), float("nan"), device=DEV)
                with _device_errors_end_the_run(f"split-K linear m={m} k={k} n={n}"):
                    _native.check(lib.honk_linear_splitk_f32(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), m,
                                                             k, n, relu, ws.data_ptr(), need, st), "honk_linear_splitk_f32")
                    torch.cuda.synchronize()
                assert bool((ws[need:] == 0xA5).all())
                want = (torch.relu(ref[:m]) if relu else ref[:m]).float()
                torch.testing.assert_close(y.cpu(), want, atol=1e-4, rtol=1e-5)
                if m < 17 and not relu:
                    first = y.cpu().numpy()
                if m == 17 and not relu:  # a row's sums do not depend on the rows around it
                    assert np.array_equal(y.cpu().numpy()[:3], first)


@pytest.mark.parametrize("prec", cgeo.PRECS)
@pytest.mark.parametrize("cid", ["trad-100x40", "one-lin6510-37x42"])
def test_c_abi(cid, prec):
    """(f)"""
    case, B = cgeo.BY_ID[cid], 3
    m = _module(case, prec)
    lib, d = _native.load(), _desc(m, prec)
    n_labels = cgeo.config(case)["n_labels"]
    need = lib.honk_cnn_latency_workspace_bytes(ctypes.byref(d), B)
    assert need >= lib.honk_cnn_workspace_bytes(ctypes.byref(d), B) > 0
    x = torch.tensor(cgeo.build(case)[2][:B]).to(DEV)
    ts = _tensors(m)
    st = _native.stream_handle(torch.device(DEV))
    outs = []
    for fill in (0xA5, 0x00, 0xFF):
        ws = torch.full((need + TAIL,), fill, dtype=torch.uint8, device=DEV)
        ws[need:] = 0xA5
        logits = torch.full((B * n_labels + TAIL // 4,), float("nan"), device=DEV)
        logits[B * n_labels:] = 12345.0
        with _device_errors_end_the_run(f"{cid} {prec} latency through the C ABI"), torch.cuda.device(DEV):
            _native.check(lib.honk_cnn_forward_latency(ctypes.byref(d), _native.ptr_array(ts), x.data_ptr(),
                                                       logits.data_ptr(), B, ws.data_ptr(), need, st),
                          "honk_cnn_forward_latency")
            torch.cuda.synchronize()
        assert bool((ws[need:] == 0xA5).all()), "workspace tail written"
        assert bool((logits[B * n_labels:] == 12345.0).all()), "logits tail written"
        out = logits[:B * n_labels].cpu().numpy().reshape(B, n_labels)
        assert not np.isnan(out).any(), "a logit was not written"
        outs.append(out)
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])  # nothing read before its write
    assert float(np.abs(outs[0] - cgeo.oracle(case, B)).max()) <= cgeo.ATOL
    assert np.array_equal(outs[0], _forward(m, cgeo.build(case)[2][:B], "latency"))
    # one byte short: refused, nothing enqueued
    logits.fill_(float("nan"))
    rc = lib.honk_cnn_forward_latency(ctypes.byref(d), _native.ptr_array(ts), x.data_ptr(), logits.data_ptr(), B,
                                      ws.data_ptr(), need - 1, st)
    assert rc != 0 and b"workspace" in lib.honk_last_error()
    # batch 0: nothing written
    _native.check(lib.honk_cnn_forward_latency(ctypes.byref(d), _native.ptr_array(ts), x.data_ptr(), logits.data_ptr(), 0,
                                               ws.data_ptr(), need, st), "honk_cnn_forward_latency")
    torch.cuda.synchronize()
    assert bool(torch.isnan(logits).all()) and bool((ws[need:] == 0xA5).all())


def test_schedule_attribute():
    m = _module(cgeo.BY_ID["trad-72x40"], "f32")
    assert m.honk_schedule == "throughput"
    m.honk_schedule = "fastest"
    try:
        with pytest.raises(ValueError):
            m(torch.zeros(1, 72, 40, device=DEV))
    finally:
        m.honk_schedule = "throughput"
    m.train()
    try:
        with pytest.raises(RuntimeError):
            m.honk_capture(torch.zeros(1, 72, 40, device=DEV))
    finally:
        m.eval()
    with pytest.raises(RuntimeError):
        m.honk_capture(torch.zeros(0, 72, 40, device=DEV))


# ---- graph capture and the label service: in a child process under a timeout -------------
@pytest.fixture(scope="module")
def graph_child(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cnn_latency_graph")
    out = str(tmp / "child.npz")
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "cnn_latency_graph_child.py"), out, str(tmp)],
                           capture_output=True, text=True, timeout=240)
    except subprocess.TimeoutExpired:
        pytest.exit("tests/cnn_latency_graph_child.py (graph capture / replay) hung: stopping the GPU run", 1)
    if p.returncode < 0 or p.returncode in (134, 139):
        pytest.exit(f"tests/cnn_latency_graph_child.py died with status {p.returncode}: stopping the GPU run\n"
                    f"{p.stderr[-3000:]}", 1)
    assert p.returncode == 0, p.stderr[-3000:]
    return np.load(out)


@pytest.mark.parametrize("prec", cgeo.PRECS)
def test_graph_replays_equal_the_eager_latency_forward(graph_child, prec):
    z = graph_child
    assert int(z[f"{prec}_flagged_none"]) == 1 and int(z[f"{prec}_schedule_kept"]) == 1
    assert int(z[f"{prec}_mismatch_raises"]) == 1
    for i in range(3):
        assert np.isfinite(z[f"{prec}_graph_{i}"]).all()
        assert np.array_equal(z[f"{prec}_graph_{i}"], z[f"{prec}_eager_{i}"]), i
    assert not np.array_equal(z[f"{prec}_graph_0"], z[f"{prec}_graph_1"])
    assert not np.array_equal(z[f"{prec}_graph_1"], z[f"{prec}_graph_2"])


def test_label_service_graph_of_the_latency_schedule(graph_child):
    z = graph_child
    labels, probs = z["svc_labels"], z["svc_probs"]
    assert int(z["svc_is_cnn"]) == 1 and str(z["svc_schedule"]) == "latency"
    assert int(z["svc_capture_kept"]) == 1 and int(z["svc_reload_drops"]) == 1 and int(z["svc_plain_untouched"]) == 1
    assert len(set(labels.tolist())) == 1
    assert abs(probs[1] - probs[0]) <= 1e-4 and probs[2] == probs[1]
