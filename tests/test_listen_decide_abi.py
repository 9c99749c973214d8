"""honk_listen_decide_f32 (csrc/listen.hip), host-only: the symbol, the refusals the call makes before it
would touch the GPU (every device pointer here is NULL or a stand-in that is never dereferenced), and the
CPU side of the Python surface: TorchLabelService.decide on the definition, listen_streams, honk_decide,
StreamPool.feed_arrays without a bank."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from honk_amd import _native
from honk_amd import service as hs
from test_mfcc_windows_abi import _pcm, _service

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED = -1, -2
P = 0x1000  # a non-null stand-in for a device pointer
INF, NAN = float("inf"), float("nan")


@pytest.fixture()
def lib():
    from honk_amd import build
    build.build()
    return _native.load()


def _call(lib, n=4, n_labels=4, segments=0, ptrs=(None,) * 7, keyword=-1, min_prob=0.85):
    logits, window0, label, prob, sums, counts, hit = ptrs
    return lib.honk_listen_decide_f32(logits, n, n_labels, window0, segments, keyword, min_prob, label, prob, sums,
                                      counts, hit, None)


def test_symbol_exists_and_header_agrees(lib):
    src = open(os.path.join(REPO, "include", "honk_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert hasattr(lib, "honk_listen_decide_f32") and "honk_listen_decide_f32" in _native.EXPORTS
    assert re.search(r"\bhonk_listen_decide_f32\s*\(", src)
    assert re.search(r"#define\s+HONK_LISTEN_MAX_LABELS\s+64\b", src)
    assert _native.LISTEN_MAX_LABELS == 64 and _native.LISTEN_MAX_WINDOWS == 1 << 23
    from honk_amd import build
    assert "listen.hip" in build.SOURCES


@pytest.mark.parametrize("kw, status, text", [
    (dict(n=-1), ERR_ARG, "n=-1"),
    (dict(n_labels=-1), ERR_ARG, "n_labels=-1"),
    (dict(n_labels=0), ERR_UNSUPPORTED, "n_labels=0"),
    (dict(n_labels=65), ERR_UNSUPPORTED, "n_labels=65"),
    (dict(n=(1 << 23) + 1), ERR_UNSUPPORTED, "8388609"),
    (dict(segments=-1), ERR_ARG, "segments=-1"),
    (dict(n=4, ptrs=(P, None, None, P, None, None, None)), ERR_ARG, "null"),        # NULL label, n > 0
    (dict(n=4, ptrs=(None, None, P, P, None, None, None)), ERR_ARG, "null"),        # NULL logits, n > 0
    (dict(n=4, segments=2, ptrs=(P, P, P, P, None, P, P)), ERR_ARG, "null"),        # NULL sums, segments > 0
    (dict(n=0, segments=2, ptrs=(None, None, None, None, P, P, P)), ERR_ARG, "null"),  # NULL window0
])
def test_refusals_are_made_on_the_host_and_leave_a_text(lib, kw, status, text):
    lib.honk_spatial_mean_f32(None, None, 0, 0, None)   # (another call's text first: the refusal must replace it)
    before = lib.honk_last_error()
    assert _call(lib, **kw) == status
    err = lib.honk_last_error().decode()
    assert err != before.decode() and "listen decide" in err and text in err, err


def test_nothing_to_do_is_ok_with_every_pointer_null(lib):
    assert _call(lib, n=0, segments=0) == 0


# ---- the definition, on the CPU ------------------------------------------------------------------
def _loop(label, prob, w0, n_labels, kw, min_prob):
    """The host loop of ListenEndpoint.POST per segment, on (label, prob)."""
    S = len(w0) - 1
    sums, counts, hit = np.zeros((S, n_labels)), np.zeros((S, n_labels), np.int32), np.full(S, -1, np.int64)
    for s in range(S):
        for i in range(w0[s], w0[s + 1]):
            sums[s, label[i]] += float(prob[i])
            counts[s, label[i]] += 1
            if hit[s] < 0 and label[i] == kw and float(prob[i]) >= min_prob:
                hit[s] = i - w0[s]
    return sums, counts, hit


LOGITS = np.array([[0.5, 2.0, 2.0, -1.0],       # a tie: the first index wins
                   [3.0, -INF, 0.0, 1.0],       # a -inf among finite values: a zero term
                   [0.0, NAN, 1.0, 2.0],        # NaN row
                   [0.0, INF, 1.0, 2.0],        # +inf row
                   [-INF, -INF, -INF, -INF],    # nothing above -inf
                   [-2.0, -1.0, 4.0, 0.0],
                   [1.0, 1.0, 1.0, 1.0],
                   [0.0, 9.0, 0.0, 0.0]], np.float32)


def test_cpu_decide_follows_the_definition(tmp_path):
    svc = _service(tmp_path, no_cuda=True)
    label, prob = svc.decide(torch.from_numpy(LOGITS))
    assert label.dtype == np.int32 and prob.dtype == np.float32 and label.shape == prob.shape == (8,)
    assert label.tolist() == [1, 0, 0, 0, 0, 2, 0, 1]
    assert np.isnan(prob[2:5]).all() and not np.isnan(np.delete(prob, [2, 3, 4])).any()
    z = LOGITS[[0, 1, 5, 6, 7]].astype(np.float64)
    want = 1.0 / np.exp(z - z.max(1, keepdims=True)).sum(1)
    assert np.abs(prob[[0, 1, 5, 6, 7]] - want).max() <= 12 * 2.0 ** -23
    assert prob[6] == 0.25
    # exactly softmax -> argmax / max
    p = F.softmax(torch.from_numpy(LOGITS), dim=1).numpy()
    assert np.array_equal(label, np.argmax(p, 1)) and np.array_equal(prob, np.max(p, 1), equal_nan=True)

    # segments: empty ones first, in the middle and last; single-window ones; a NaN row inside one
    w0 = np.array([0, 0, 1, 2, 2, 5, 8, 8], np.int64)
    for kw, min_prob in ((1, 0.5), (1, 0.9999), (0, 0.0), ("yes", 0.5), (None, 0.0), (-1, 0.0), (3, 0.0)):
        l2, p2, sums, counts, hit = svc.decide(torch.from_numpy(LOGITS), w0, kw, min_prob)
        assert np.array_equal(l2, label) and np.array_equal(p2, prob, equal_nan=True)
        assert sums.dtype == np.float64 and counts.dtype == np.int32 and hit.dtype == np.int64
        k = {"yes": 2, None: -1}.get(kw, kw)
        ws, wc, wh = _loop(label, prob, w0, 4, k, min_prob)
        assert np.array_equal(counts, wc) and np.array_equal(hit, wh)
        assert np.array_equal(np.isnan(sums), np.isnan(ws))
        assert sums[~np.isnan(ws)].tobytes() == ws[~np.isnan(ws)].tobytes()
    _, _, sums, counts, hit = svc.decide(torch.from_numpy(LOGITS), w0, 1, 0.4)
    assert hit.tolist() == [-1, 0, -1, -1, -1, 2, -1]       # row 0 (0.44); row 7 is the third of rows 5..7
    assert svc.decide(torch.from_numpy(LOGITS), w0, 1, 0.5)[4].tolist() == [-1, -1, -1, -1, -1, 2, -1]
    assert counts[4].tolist() == [3, 0, 0, 0] and np.isnan(sums[4, 0]) and not sums[4, 1:].any()
    assert not sums[[0, 3, 6]].any() and not counts[[0, 3, 6]].any()
    _, _, _, _, hit = svc.decide(torch.from_numpy(LOGITS), w0, 0, 0.0)
    assert hit[4] == -1 and hit[2] == 0                      # NaN compares false; row 1's 0.84 passes 0.0

    # no rows at all
    label, prob, sums, counts, hit = svc.decide(torch.zeros(0, 4), np.array([0, 0, 0]), 1, 0.5)
    assert label.shape == prob.shape == (0,) and not sums.any() and not counts.any() and hit.tolist() == [-1, -1]
    for bad in ([1, 8], [0, 5, 4, 8], [0, 7], [[0, 8]], [0.0, 8.0]):
        with pytest.raises(ValueError):
            svc.decide(torch.from_numpy(LOGITS), np.array(bad))


def test_native_wrapper_refuses_what_is_not_a_device_tensor():
    with pytest.raises(ValueError):
        _native.listen_decide(torch.from_numpy(LOGITS))
    with pytest.raises(ValueError):
        _native.listen_window0(np.array([0, 3, 2, 8]), 8)


RECS = ((11, 40000), (12, 15999), (13, 16000), (14, 52017), (15, 0))   # (seed, samples): one shorter than a window


@pytest.mark.parametrize("stride_ms", [500, 100])
def test_cpu_listen_streams_equals_listen_stream_per_recording(tmp_path, stride_ms):
    svc = _service(tmp_path, no_cuda=True)
    recs = [_pcm(seed, n).tobytes() for seed, n in RECS]
    want = [svc.listen_stream(r, stride_ms) for r in recs]
    assert want[1] == {} == want[4] and sum(len(w) for w in want) > 0
    assert svc.listen_streams(recs, stride_ms) == want
    probs = sorted(p for r in recs for _, p in svc.label_stream(r, stride_ms))
    for kw in svc.labels + ["command"]:
        for min_prob in (0.0, probs[0], probs[len(probs) // 2], probs[-1], 1.1):
            assert svc.listen_streams(recs, stride_ms, "command_tagging", kw, min_prob) == \
                [svc.listen_stream(r, stride_ms, "command_tagging", kw, min_prob) for r in recs]
    assert svc.listen_streams([]) == []


def test_cpu_honk_decide_service_returns_what_the_default_does(tmp_path):
    plain, dec = _service(tmp_path, no_cuda=True), _service(tmp_path, no_cuda=True)
    dec.honk_decide = True
    assert hs.TorchLabelService(dec.model_filename, no_cuda=True, labels=dec.labels, honk_decide=True).honk_decide
    assert not plain.honk_decide
    recs = [_pcm(seed, n).tobytes() for seed, n in RECS]
    wins = list(hs.stride(recs[0], 16000, 32000))
    assert dec.label_batch(wins) == plain.label_batch(wins) and len(wins) == 4
    assert dec.label_batch([]) == []
    for r in recs:
        assert dec.label_stream(r, 100) == plain.label_stream(r, 100)
        assert dec.listen_stream(r) == plain.listen_stream(r)
    assert dec.label_streams(recs, 500) == plain.label_streams(recs, 500)
    got = dec.label_streams(recs, 500)
    assert all(type(l) is str and type(p) is float for g in got for l, p in g)
    a, b = hs.StreamPool(dec, 500), hs.StreamPool(plain, 500)
    for t in range(0, len(recs[3]), 9000):
        fed = {"x": recs[3][t:t + 9000], 7: recs[0][t:t + 9000]}
        assert a.feed(fed) == b.feed(fed)


def test_feed_arrays_needs_a_bank(tmp_path):
    svc = _service(tmp_path, no_cuda=True)
    with pytest.raises(ValueError):
        hs.StreamPool(svc).feed_arrays(["a"], np.zeros(100, np.int16), np.array([0, 100]))
    with pytest.warns(UserWarning):
        pool = hs.StreamPool(svc, device_state=True)   # (no bank on a CPU service)
    with pytest.raises(ValueError):
        pool.feed_arrays(["a"], np.zeros(100, np.int16), np.array([0, 100]))
