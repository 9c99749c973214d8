"""honk_listen_decide_f32 on the device (csrc/listen.hip) and the serving surface over it
(TorchLabelService.decide / listen_streams / honk_decide, StreamPool.feed_arrays).

Rows: label is np.argmax of the logits exactly (first index of the largest); prob is held to the float64
softmax maximum within (n_labels + 8) * 2^-23 -- fp32 rounding of one expf (the largest term is exactly 1,
the others at most 1), n_labels adds and one divide on a value in [1/n_labels, 1], with a factor of two in
hand.  Segments: counts, sums and hit equal a Python loop over the returned label / prob BIT FOR BIT (a
finite prob is a multiple of 2^-29 and at most 2^23 of them are summed: exact in double, whatever the
order).  Service results are compared under _same(..., 1e-6), the tolerance the project already uses for
the same windows in another batch composition of the forward."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import poison_util as pu
import test_gpu_mfcc_windows as mfcc_w
import test_gpu_pcen_segments as pcen_s
import test_mfcc_windows_abi as mfcc_abi
from honk_amd import _native
from honk_amd import service as hs
from test_gpu_mfcc_segments import CHUNKS, _wavs
from test_mfcc_windows_abi import _pcm, _same

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"
INF, NAN = float("inf"), float("nan")
N_LABELS, NS, SCALES = (1, 2, 4, 12, 37, 64), (1, 3, 257), (1.0, 30.0)


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _run(z, *a):
    return tuple(t.cpu().numpy() for t in _native.listen_decide(torch.from_numpy(z).to(DEV), *a))


@functools.lru_cache(maxsize=None)
def _rows(n_labels, scale):
    """(logits [257, n_labels], label, prob of the native call on all 257, float64 softmax max); computed
    once, read-only.  Every 7th row has its last logit copied over its first: a tie."""
    rng = np.random.default_rng(1000 * n_labels + int(scale))
    z = (scale * rng.standard_normal((257, n_labels))).astype(np.float32)
    z[::7, 0] = z[::7, -1]
    label, prob = _run(z)
    z64 = z.astype(np.float64)
    ref = 1.0 / np.exp(z64 - z64.max(1, keepdims=True)).sum(1)
    for a in (z, label, prob, ref):
        a.setflags(write=False)
    return z, label, prob, ref


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("n_labels", N_LABELS)
def test_rows(n_labels, n, scale):
    _gpu()
    z, label257, prob257, ref = _rows(n_labels, scale)
    label, prob = _run(z[:n].copy())
    assert label.dtype == np.int32 and prob.dtype == np.float32 and label.shape == prob.shape == (n,)
    assert np.array_equal(label, np.argmax(z[:n], 1))
    tied = [r for r in range(0, n, 7) if z[r, 0] == z[r].max()]
    assert all(label[r] == 0 for r in tied)                   # where the tie is the maximum, index 0 wins
    assert tied or n_labels > 12 or n < 257                    # (in 3 to 37 rows of the 257 up to 12 labels)
    bound = (n_labels + 8) * 2.0 ** -23
    err = np.abs(prob.astype(np.float64) - ref[:n]).max()
    print(f"n_labels={n_labels} n={n} scale={scale}: max|prob - float64| = {err:.3e} ({err / bound:.3f} of the bound)")
    assert err <= bound
    if scale == 30.0 and n_labels >= 12 and n == 257:
        assert (np.exp(z - z.max(1, keepdims=True)) == 0).any()  # terms that underflow to 0 in fp32
    again = _run(z[:n].copy())
    assert again[0].tobytes() == label.tobytes() and again[1].tobytes() == prob.tobytes()
    # a row's result does not depend on n or on its neighbours
    assert label.tobytes() == label257[:n].tobytes() and prob.tobytes() == prob257[:n].tobytes()


def _nonfinite(n_labels):
    rng = np.random.default_rng(5)
    z = rng.standard_normal((9, n_labels)).astype(np.float32)
    z[1, n_labels // 2] = NAN
    z[2, -1] = INF
    z[3, :] = -INF
    z[4, 0] = -INF              # one -inf among finite values: an ordinary zero term
    z[5, 0], z[5, -1] = INF, NAN
    z[6, 0], z[6, -1] = -INF, INF
    z[7, :] = INF
    return z


@pytest.mark.parametrize("n_labels", [4, 12, 64])
def test_nonfinite_rows(n_labels):
    _gpu()
    z = _nonfinite(n_labels)
    p = torch.softmax(torch.from_numpy(z), 1).numpy()
    want_label, want_prob = np.argmax(p, 1).astype(np.int32), np.max(p, 1)
    assert np.isnan(want_prob[[1, 2, 3, 5, 6, 7]]).all() and not np.isnan(want_prob[[0, 4, 8]]).any()
    assert (want_label[[1, 2, 3, 5, 6, 7]] == 0).all()
    label, prob = _run(z)
    assert np.array_equal(label, want_label)
    assert np.array_equal(np.isnan(prob), np.isnan(want_prob))
    assert np.allclose(prob, want_prob, rtol=0, atol=(n_labels + 8) * 2.0 ** -23, equal_nan=True)
    alone = _run(z[[4]].copy())
    assert alone[0].tobytes() == label[4:5].tobytes() and alone[1].tobytes() == prob[4:5].tobytes()


# ---- segments ------------------------------------------------------------------------------------
TABLES = {"one": [0, 257], "singletons": list(range(258)), "empties": [0, 0, 5, 5, 200, 257, 257]}


def _loop(label, prob, w0, n_labels, kw, min_prob):
    S = len(w0) - 1
    sums, counts, hit = np.zeros((S, n_labels)), np.zeros((S, n_labels), np.int32), np.full(S, -1, np.int64)
    for s in range(S):
        for i in range(w0[s], w0[s + 1]):
            sums[s, label[i]] += float(prob[i])
            counts[s, label[i]] += 1
            if hit[s] < 0 and label[i] == kw and float(prob[i]) >= min_prob:
                hit[s] = i - w0[s]
    return sums, counts, hit


def _threshold(probs, tol):
    """The midpoint of the widest gap among the sorted probs; no prob is within ``tol`` of it."""
    p = np.sort(np.asarray(probs, np.float64))
    assert len(p) >= 2
    i = int(np.argmax(np.diff(p)))
    t = (p[i] + p[i + 1]) / 2
    assert np.abs(p - t).min() > tol
    return t


@pytest.mark.parametrize("table", list(TABLES))
def test_segments_equal_the_host_loop_bit_for_bit(table):
    _gpu()
    z, label257, prob257, ref = _rows(12, 1.0)
    w0 = np.array(TABLES[table], np.int64)
    kw = int(np.bincount(label257).argmax())                    # a label that occurs
    min_prob = _threshold(ref[label257 == kw], (12 + 8) * 2.0 ** -23)
    for keyword, mp in ((kw, min_prob), (-1, 0.0), (kw, 0.0), (kw, 2.0)):
        label, prob, sums, counts, hit = _run(z.copy(), w0, keyword, mp)
        assert label.tobytes() == label257.tobytes() and prob.tobytes() == prob257.tobytes()
        assert sums.dtype == np.float64 and counts.dtype == np.int32 and hit.dtype == np.int64
        assert sums.shape == counts.shape == (len(w0) - 1, 12) and hit.shape == (len(w0) - 1,)
        ws, wc, wh = _loop(label, prob, w0, 12, keyword, mp)
        assert counts.tobytes() == wc.tobytes()
        assert sums.tobytes() == ws.tobytes()
        assert hit.tobytes() == wh.tobytes()
        if keyword < 0 or mp > 1:
            assert (hit == -1).all()
    label, prob, sums, counts, hit = _run(z.copy(), w0, kw, min_prob)
    assert (hit >= 0).any() and int(counts.sum()) == 257
    if table == "singletons":
        assert (hit == -1).any()                                 # the threshold separates the label's windows
    if table == "empties":
        assert not sums[[0, 2, 5]].any() and not counts[[0, 2, 5]].any() and (hit[[0, 2, 5]] == -1).all()


def test_a_nan_row_inside_a_segment():
    _gpu()
    z = _rows(12, 1.0)[0][:40].copy()
    z[17, 3] = NAN
    w0 = np.array([0, 10, 30, 40], np.int64)
    label, prob, sums, counts, hit = _run(z, w0, 0, 0.0)
    assert label[17] == 0 and np.isnan(prob[17]) and np.isnan(prob).sum() == 1
    ws, wc, wh = _loop(label, prob, w0, 12, 0, 0.0)
    assert np.isnan(sums[1, 0]) and np.isnan(sums).sum() == 1 and np.array_equal(np.isnan(sums), np.isnan(ws))
    assert sums[~np.isnan(sums)].tobytes() == ws[~np.isnan(ws)].tobytes()
    assert counts.tobytes() == wc.tobytes() and hit.tobytes() == wh.tobytes()
    # the NaN row is labelled 0 and is no hit: the segment's hit is its first finite row labelled 0, if any
    finite0 = [i - 10 for i in range(10, 30) if label[i] == 0 and i != 17]
    assert hit[1] == (finite0[0] if finite0 else -1)
    only = _run(z[17:18].copy(), np.array([0, 1], np.int64), 0, 0.0)
    assert np.isnan(only[2][0, 0]) and only[3][0, 0] == 1 and only[4][0] == -1


# ---- memory contract -----------------------------------------------------------------------------
def test_memory_contract():
    """The five outputs poisoned and guard-banded, for every fill: the unpoisoned result, every guard intact,
    every element written; logits and the table unchanged."""
    _gpu()
    z, label257, prob257, _ = _rows(12, 1.0)
    w0 = np.array(TABLES["empties"], np.int64)
    want = _run(z.copy(), w0, 3, 0.3)
    logits = torch.from_numpy(z.copy()).to(DEV)
    for fill in pu.FILLS:
        with pu.arena(fill) as a, pu.frozen(logits):
            got = _native.listen_decide(logits, w0, 3, 0.3)
            torch.cuda.synchronize()
        a.check()
        assert len(a.typed()) == 5, a.sites()
        for g, w in zip(got, want):
            assert g.cpu().numpy().tobytes() == w.tobytes(), hex(fill)
        if fill == 0x3C:   # (no label, count, hit, prob >= 2^-6 or sum is 0x3C3C...: 0xFF is a NaN and a -1)
            for g in got:
                assert not a.untouched(g)


def test_n_zero_and_no_segments_write_nothing():
    _gpu()
    lib, z = _native.load(), torch.from_numpy(_rows(12, 1.0)[0].copy()).to(DEV)
    w0 = torch.zeros(5, dtype=torch.int64, device=DEV)
    for fill in pu.FILLS:
        a = pu.arena(fill)
        label, prob = a.buffer(64, torch.int32, DEV), a.buffer(64, torch.float32, DEV)
        sums, counts = a.buffer((4, 12), torch.float64, DEV), a.buffer((4, 12), torch.int32, DEV)
        hit = a.buffer(4, torch.int64, DEV)
        outs = (label, prob, sums, counts, hit)

        def call(n, segments):
            _native.check(lib.honk_listen_decide_f32(z.data_ptr(), n, 12, w0.data_ptr(), segments, 3, 0.3,
                                                     *(t.data_ptr() for t in outs), _native.stream_handle(z.device)),
                          "honk_listen_decide_f32")
            torch.cuda.synchronize()
            a.check()

        call(0, 0)
        for t in outs:
            assert len(a.untouched(t)) == t.numel()
        call(64, 0)     # rows only: the segment outputs stay as they were
        assert label.cpu().numpy().tobytes() == _rows(12, 1.0)[1][:64].tobytes()
        for t in outs[2:]:
            assert len(a.untouched(t)) == t.numel()
        label.view(torch.uint8).fill_(fill)
        prob.view(torch.uint8).fill_(fill)
        call(0, 4)      # segments only (all empty): nothing per window is written
        for t in outs[:2]:
            assert len(a.untouched(t)) == t.numel()
        assert not sums.any() and not counts.any() and (hit == -1).all()


# ---- graph ---------------------------------------------------------------------------------------
def test_capturable():
    """The call inside torch.cuda.graph on fixed buffers; logits refilled, one replay: the eager result on
    the second logits, bit for bit.  In a child under a timeout."""
    _gpu()
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "child.npz")
        try:
            p = subprocess.run([sys.executable, os.path.join(HERE, "listen_decide_graph_child.py"), out],
                               capture_output=True, text=True, timeout=120)
        except subprocess.TimeoutExpired:
            pytest.exit("tests/listen_decide_graph_child.py (graph capture / replay) hung: stopping the GPU run", 1)
        if p.returncode < 0 or p.returncode in (134, 139):
            pytest.exit(f"tests/listen_decide_graph_child.py died with status {p.returncode}: stopping the GPU run\n"
                        f"{p.stderr[-3000:]}", 1)
        assert p.returncode == 0, p.stderr[-3000:]
        z = np.load(out)
        for k in ("label", "prob", "sums", "counts", "hit"):
            assert z[f"replay_{k}"].shape == z[f"eager_{k}"].shape
            assert z[f"replay_{k}"].tobytes() == z[f"eager_{k}"].tobytes(), k
        assert z["replay_prob"].shape == (257,) and z["replay_prob"].all() and (z["replay_hit"] >= 0).any()


# ---- the service ---------------------------------------------------------------------------------
FRONTS = {"MFCCs": (mfcc_abi._service, mfcc_w._no_ties, (31, 36, 37)),
          "PCEN": (pcen_s._service, pcen_s._no_ties, pcen_s.SEEDS)}


def _services(tmp_path, front):
    make, no_ties, seeds = FRONTS[front]
    cpu, plain, dec = make(tmp_path, no_cuda=True), make(tmp_path, no_cuda=False), make(tmp_path, no_cuda=False)
    dec.honk_decide = True
    assert dec.audio_preprocess_type == front and not plain.honk_decide
    return cpu, plain, dec, no_ties, _wavs(seeds)


@pytest.mark.parametrize("stride_ms", [500, 100])
@pytest.mark.parametrize("front", list(FRONTS))
def test_service_with_honk_decide(tmp_path, front, stride_ms):
    _gpu()
    cpu, plain, dec, no_ties, wavs = _services(tmp_path, front)
    for w in wavs:
        assert no_ties(cpu.model, w, stride_ms) == {500: 5, 100: 21}[stride_ms]
    recs = wavs + [b"", wavs[0][:31998]]                          # (and two that complete no window)
    want = plain.label_streams(recs, stride_ms)
    for got in (dec.label_streams(recs, stride_ms), dec.label_streams(recs, stride_ms, max_windows=12)):
        assert [len(g) for g in got] == [len(w) for w in want] and got[3:] == [[], []]
        for g, w in zip(got, want):
            _same(g, w, 1e-6)
    _same(dec.label_stream(wavs[0], stride_ms), want[0], 1e-6)
    wins = list(hs.stride(wavs[0], 32 * stride_ms, 32000))
    _same(dec.label_batch(wins), plain.label_batch(wins), 1e-6)

    # listen_streams against listen_stream per recording
    per_rec = [plain.listen_stream(r, stride_ms) for r in recs]
    for got in (dec.listen_streams(recs, stride_ms), plain.listen_streams(recs, stride_ms, max_windows=12)):
        assert len(got) == len(recs)
        for g, w, labelled in zip(got, per_rec, want):
            assert set(g) == set(w)
            assert all(abs(g[k] - w[k]) <= len(labelled) * 1e-6 for k in w)
    # the keyword: a label that occurs; the threshold: between two of its windows' probabilities on the CPU
    # service, none of which is within 1e-4 (the bar the device service is held to against the CPU's) of it
    on_cpu = [lp for r in wavs for lp in cpu.label_stream(r, stride_ms)]
    names = [l for l, _ in on_cpu]
    kw = max(set(names), key=names.count)
    t = _threshold([p for l, p in on_cpu if l == kw], 1e-4)
    for keyword, mp in ((kw, t), (kw, 0.0), (kw, 1.1), ("command", 0.0)):
        tagged = [plain.listen_stream(r, stride_ms, "command_tagging", keyword, mp) for r in recs]
        assert dec.listen_streams(recs, stride_ms, "command_tagging", keyword, mp) == tagged
    assert any(x["contains_command"] for x in
               dec.listen_streams(recs, stride_ms, "command_tagging", kw, 0.0))


@pytest.mark.parametrize("stride_ms", [500, 100])
@pytest.mark.parametrize("front", list(FRONTS))
def test_feed_arrays_equals_feed_on_a_twin_pool(tmp_path, front, stride_ms):
    """The CHUNKS schedules of the pool tests: three streams, the third opened two ticks late and fed whole."""
    _gpu()
    _, plain, dec, _, wavs = _services(tmp_path, front)
    arrays, twin = hs.StreamPool(dec, stride_ms, device_state=True), hs.StreamPool(plain, stride_ms, device_state=True)
    assert arrays.bank is not None and twin.bank is not None
    start = (0, 0, 2)
    size = [c or len(w) for c, w in zip(CHUNKS, wavs)]
    ticks = max(s + -(-len(w) // c) for s, w, c in zip(start, wavs, size))
    completed = []
    for t in range(ticks):
        fed = {}
        for k, w in enumerate(wavs):
            i = (t - start[k]) * size[k]
            if t >= start[k] and i < len(w):
                fed[k] = w[i:i + size[k]]
        want = twin.feed(fed)
        parts = [np.frombuffer(fed[k], np.int16) for k in fed]
        off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
        pcm = np.concatenate(parts)
        if t % 2:                                                 # a tensor or an array
            pcm = torch.from_numpy(pcm)
        label, prob, w0 = arrays.feed_arrays(list(fed), pcm, off)
        assert label.dtype == np.int32 and prob.dtype == np.float32 and w0.dtype == np.int64
        assert w0.tolist() == np.concatenate([[0], np.cumsum([len(want[k]) for k in fed])]).tolist()
        assert label.shape == prob.shape == (w0[-1],)
        for j, k in enumerate(fed):
            got = [(dec.labels[l], float(p)) for l, p in zip(label[w0[j]:w0[j + 1]], prob[w0[j]:w0[j + 1]])]
            _same(got, want[k], 1e-6)
        completed.append((len(fed), np.diff(w0).tolist()))
    # a tick that completes no window, one where a stream completes several, a key that appears mid-way
    assert completed[0] == (2, [0, 0]) and completed[2][0] == 3 and completed[2][1][2] > 1
    assert sorted(arrays.keys()) == sorted(twin.keys()) == [0, 1, 2]
    assert arrays.bank.stats == twin.bank.stats
    # the same streams through feed on the next tick
    more = {k: _pcm(80 + k, 16000).tobytes() for k in range(3)}
    a, b = arrays.feed(more), twin.feed(more)
    for k in more:
        assert len(a[k]) == len(b[k]) > 0
        _same(a[k], b[k], 1e-6)
