"""The stream-ordered res forward (honk_res_forward_ordered, SpeechResModel.honk_stream_ordered,
honk_capture, TorchLabelService.honk_graph): the f16x2 forward whose bf16x3 re-run is driven by
the flagged-clip count in DEVICE memory -- no host read, so the call only enqueues work and can
be captured in a graph.

Shapes: f16x2 is selected on full res15 maps only, so the batches are the 3 calibrated clips of
res15-b3-mfcc (nothing flagged), the same model's inputs x 3000 (range_res15-ood: every clip
flagged) and the interleaved 6-clip batch of test_gpu_range.py (clips 1, 3, 5 flagged).  The
bar of a re-run clip is the project's: |err| <= 5e-5 max(1, max|logit|) per clip against the
reference-written logits (test_gpu_range._rel_bound); clips that are not re-run must equal the
synchronous path bit for bit.  Measured: the re-run clips equal the synchronous path's bit for
bit too (one plan serves every clip count, a clip's arithmetic does not depend on its place in
the launch), so that is asserted as well."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from honk_amd import _native
from golden_util import load_fixture, load_range_fixture
from test_gpu_range import DEV, _rel_bound, module, run

pytestmark = pytest.mark.gpu
ENV = ("HONK_PRECISION", "HONK_RES_KERNEL", "HONK_LAST_KERNEL", "HONK_CONV0", "HONK_F16X2_RERUN", "HONK_RES_CHUNK")
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _native.load()


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)


class Data:
    pass


@pytest.fixture(scope="module")
def data(_need_gpu):
    """The three batches, the reference's logits, and -- computed once -- the synchronous
    path's logits and re-run counts and the raw f16x2 logits of the mixed batch."""
    d = Data()
    with pytest.MonkeyPatch.context() as mp:
        for v in ENV:
            mp.delenv(v, raising=False)
        cfg, params, x, logits, meta = load_fixture("res15-b3-mfcc")
        _, p_ood, x_ood, l_ood, _ = load_range_fixture("res15-ood")
        assert all(np.array_equal(params[k], p_ood[k]) for k in params)  # the same model
        d.cfg, d.params = cfg, params
        d.x = dict(benign=x, flagged=x_ood,
                   mixed=np.stack([x[0], x_ood[0], x[1], x_ood[1], x[2], x_ood[2]]))
        d.ref = dict(benign=logits, flagged=l_ood,
                     mixed=np.stack([logits[0], l_ood[0], logits[1], l_ood[1], logits[2], l_ood[2]]))
        d.flag = dict(benign=np.zeros(len(x), bool), flagged=np.ones(len(x_ood), bool),
                      mixed=np.array([False, True] * 3))
        d.m = module(cfg, params, "res15")
        d.sync, d.sync_rerun = {}, {}
        for k in ("benign", "flagged", "mixed"):  # benign first: the policy's probe sees the calibrated batch
            d.sync[k] = run(d.m, d.x[k])
            assert d.m.honk_last_precision == "f16x2"
            d.sync_rerun[k] = d.m.honk_last_rerun
        assert d.sync_rerun == dict(benign=0, flagged=len(x_ood), mixed=3)
        mp.setenv("HONK_F16X2_RERUN", "0")
        raw = module(cfg, params, "res15", "f16x2")
        raw.honk_reroute = False
        d.raw_mixed = run(raw, d.x["mixed"])
    return d


def ordered(m, x, capacity=None):
    """(logits, flagged count) of the stream-ordered forward on module m."""
    m.honk_stream_ordered, m.honk_rerun_capacity = True, capacity
    try:
        out = run(m, x)
        assert m.honk_last_rerun is None and m.honk_last_rerun_dev.dtype == torch.int32
        assert m.honk_last_rerun_dev.dim() == 0 and m.honk_last_rerun_dev.is_cuda
        return out, int(m.honk_last_rerun_dev)
    finally:
        m.honk_stream_ordered, m.honk_rerun_capacity = False, None


def check_against_sync(d, k, out, count, sync):
    flag, ref = d.flag[k], d.ref[k]
    assert count == d.sync_rerun[k]
    assert np.array_equal(out[~flag], sync[~flag])  # not re-run: the f16x2 logits, bit for bit
    err = np.abs(out - ref)
    if flag.any():
        print(f"{k}: re-run clips max err / bound = {float((err / _rel_bound(ref))[flag].max()):.3f}, "
              f"bitwise equal to the synchronous path: {np.array_equal(out[flag], sync[flag])}")
    assert (err <= _rel_bound(ref))[flag].all()
    assert np.array_equal(out[flag], sync[flag])  # (measured equal: see the module docstring)


@pytest.mark.parametrize("k", ["benign", "flagged", "mixed"])
def test_ordered_equals_synchronous(data, k):
    out, count = ordered(data.m, data.x[k])
    assert data.m.honk_last_precision == "f16x2"
    check_against_sync(data, k, out, count, data.sync[k])
    # and the default path is as it was
    assert np.array_equal(run(data.m, data.x[k]), data.sync[k]) and data.m.honk_last_rerun == data.sync_rerun[k]


def test_full_partial_and_empty_round(data, monkeypatch):
    """HONK_RES_CHUNK=4: two clips per re-run round, so the 3 flagged clips of the mixed batch
    take a full round, a partial round and -- the capacity being the batch -- an empty one."""
    monkeypatch.setenv("HONK_RES_CHUNK", "4")
    lib = _native.load()
    rc = lib.honk_res_rerun_clips(data.m._desc(101, 40, "f16x2"), 6)
    assert rc == 2 and math.ceil(6 / rc) == 3 and 3 % rc != 0
    sync = run(data.m, data.x["mixed"])
    assert data.m.honk_last_rerun == 3
    out, count = ordered(data.m, data.x["mixed"])
    check_against_sync(data, "mixed", out, count, sync)


def test_capacity_overflow_keeps_f16x2_logits(data):
    out, count = ordered(data.m, data.x["mixed"], capacity=2)
    assert count == 3  # the count is not clamped: count > capacity tells the caller
    ref = data.ref["mixed"]
    assert (np.abs(out - ref) <= _rel_bound(ref))[[1, 3]].all()  # the first two flagged clips: re-run
    assert np.array_equal(out[[1, 3]], data.sync["mixed"][[1, 3]])
    assert np.array_equal(out[5], data.raw_mixed[5])  # the third: its raw f16x2 logits
    assert not np.array_equal(out[5], data.sync["mixed"][5])
    assert np.array_equal(out[0::2], data.sync["mixed"][0::2])  # unflagged: unchanged


def test_row_band_rerun_on_narrow_maps(monkeypatch):
    """19 maps (res15-narrow, f16x2 forced): the bf16x3 re-run runs the row-band kernel, whose
    tiles follow the device's count too.  No reference logits for the scaled clips: the
    synchronous path is the reference, bit for bit (same kernels, same tiles per clip)."""
    monkeypatch.setenv("HONK_RES_CHUNK", "4")
    cfg, params, x, logits, meta = load_fixture("res15-narrow-mfcc")
    m = module(cfg, params, meta["model"], "f16x2")
    m.honk_reroute = False
    assert _native.res_launch_plan(m._desc(101, 40, "bf16x3"), 2) == ["block16r_kernel"] * 13
    xb = np.stack([x[0], x[0] * 3000, x[-1], x[-1] * 3000, x[0] * 3000])
    sync = run(m, xb)
    n = m.honk_last_rerun
    assert m.honk_last_precision == "f16x2" and n == 3, n  # clips 1, 3, 4: a full round of 2, a partial, an empty one
    out, count = ordered(m, xb)
    assert count == n and np.array_equal(out, sync)
    out, count = ordered(m, xb, capacity=1)
    assert count == n and np.array_equal(out[:2], sync[:2]) and not np.array_equal(out[3], sync[3])


def test_weight_stationary_rerun(data, monkeypatch):
    """HONK_RES_KERNEL=w: every layer of the re-run on the weight-stationary kernel (the
    kernel of shapes with no pair plan), two clips per round."""
    monkeypatch.setenv("HONK_RES_KERNEL", "w")
    monkeypatch.setenv("HONK_RES_CHUNK", "4")
    assert _native.res_launch_plan(data.m._desc(101, 40, "bf16x3"), 2) == ["block16w_kernel"] * 13
    sync = run(data.m, data.x["mixed"])
    assert data.m.honk_last_precision == "f16x2" and data.m.honk_last_rerun == 3
    out, count = ordered(data.m, data.x["mixed"])
    check_against_sync(data, "mixed", out, count, sync)


def test_pooled_maps_rerun_pairs_and_weight_stationary(monkeypatch):
    """res8 (25 x 13 pooled maps, f16x2 forced): the re-run is two 13-pixel-row pairs and two
    weight-stationary layers.  The synchronous path is the reference, bit for bit."""
    monkeypatch.setenv("HONK_RES_CHUNK", "4")
    cfg, params, x, logits, meta = load_fixture("res8")
    m = module(cfg, params, meta["model"], "f16x2")
    m.honk_reroute = False
    assert _native.res_launch_plan(m._desc(101, 40, "bf16x3"), 2) == ["block16p_kernel"] * 2 + ["block16w_kernel"] * 2
    xb = np.stack([x[0], x[0] * 3000, x[-1], x[-1] * 3000, x[0] * 3000])
    sync = run(m, xb)
    assert m.honk_last_precision == "f16x2" and m.honk_last_rerun == 3, m.honk_last_rerun
    out, count = ordered(m, xb)
    assert count == 3 and np.array_equal(out, sync)


@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
def test_other_precisions_are_the_default_path(data, prec):
    m = module(data.cfg, data.params, "res15", prec)
    want = run(m, data.x["benign"])
    out, count = ordered(m, data.x["benign"])
    assert m.honk_last_precision == prec and count == 0
    assert np.array_equal(out, want)


def test_c_abi_null_count_on_a_side_stream(data):
    """honk_res_forward_ordered itself: flagged_count = NULL, a non-default stream, nothing
    between the call and the stream's own synchronisation."""
    lib = _native.load()
    m = data.m
    x = torch.as_tensor(data.x["mixed"]).to(DEV)
    desc = m._desc(101, 40, "f16x2")
    packed = m._packed(x)
    ws_bytes = lib.honk_res_workspace_bytes(desc, 6)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    out = torch.full((6, 12), float("nan"), device=DEV)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        _native.check(lib.honk_res_forward_ordered(ctypes.byref(desc), packed.data_ptr(), x.data_ptr(), out.data_ptr(),
                                                   6, ws.data_ptr(), ws_bytes, s.cuda_stream, 0, None),
                      "honk_res_forward_ordered")
        assert lib.honk_res_rerun_count() == 0  # the host does not learn the count
        # batch 0: status ok, the count pointer set to 0
        cnt = torch.full((), 7, dtype=torch.int32, device=DEV)
        _native.check(lib.honk_res_forward_ordered(ctypes.byref(desc), packed.data_ptr(), x.data_ptr(), out.data_ptr(),
                                                   0, ws.data_ptr(), ws_bytes, s.cuda_stream, 0, cnt.data_ptr()),
                      "honk_res_forward_ordered")
    s.synchronize()
    assert int(cnt) == 0
    assert np.array_equal(out.cpu().numpy(), data.sync["mixed"])


# ---- graph capture: in a child process under a timeout ---------------------------------
@pytest.fixture(scope="module")
def graph_child(data, tmp_path_factory):
    """tests/ordered_graph_child.py, once: capture, three replays, the label service."""
    tmp = tmp_path_factory.mktemp("ordered_graph")
    out = str(tmp / "child.npz")
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "ordered_graph_child.py"), out, str(tmp)],
                           capture_output=True, text=True, timeout=240)
    except subprocess.TimeoutExpired:
        pytest.exit("tests/ordered_graph_child.py (graph capture / replay) hung: stopping the GPU run", 1)
    if p.returncode < 0 or p.returncode in (134, 139):
        pytest.exit(f"tests/ordered_graph_child.py died with status {p.returncode}: stopping the GPU run\n"
                    f"{p.stderr[-3000:]}", 1)
    assert p.returncode == 0, p.stderr[-3000:]
    return np.load(out)


@pytest.mark.parametrize("k,flagged", [("mixed", 3), ("benign", 0), ("flagged", 6)])
def test_one_graph_three_device_counts(data, graph_child, k, flagged):
    """One capture (on the mixed batch), replayed with 3, 0 and 6 flagged clips: the logits of
    the eager stream-ordered forward, bit for bit, and the count."""
    z = graph_child
    assert int(z["graph_count_" + k]) == int(z["eager_count_" + k]) == flagged
    assert np.array_equal(z["graph_" + k], z["eager_" + k])
    assert int(z["static_output"]) == 1 and int(z["mismatch_raises"]) == 1 and int(z["ordered_restored"]) == 1
    six = lambda a: np.concatenate([a] * (6 // len(a) + 1))[:6]  # noqa: E731  (the child's batches)
    if k == "flagged":
        ref = six(data.ref[k])
        assert (np.abs(z["graph_" + k] - ref) <= _rel_bound(ref)).all()
    else:  # (f16x2 logits do not depend on the clip's place in the batch)
        assert np.array_equal(z["eager_" + k], six(data.sync[k]))


def test_label_service_with_graph(graph_child):
    z = graph_child
    assert int(z["cnn_same"]) == 1  # the reference caller's cnn-trad-pool2 service: honk_graph changes nothing
    labels, probs = z["res_labels"], z["res_probs"]
    assert labels[0] == labels[1] == labels[2] and probs[0] == probs[1] == probs[2]
    assert int(z["capture_kept"]) == 1 and int(z["reload_drops"]) == 1
