"""The res forward past one DEFAULT chunk (chunk_clips, honk_amd/csrc/res.hip: 4096 clips of
res15, 8192 of the pooled maps res8 / res26).  Every other test of the chunk loop sets
HONK_RES_CHUNK to 3, 4 or 300, and the full-size grid is otherwise run at exactly one chunk;
here a second full-size chunk reuses the first one's workspace, a ragged remainder runs
behind full chunks, and the f16x2 flags, clip scales and re-run list are indexed past the
first chunk.

Shapes (the smallest that cross): res8 at 2 x 8192 + 77 clips (bf16, C3's mode, and auto =
bf16x3), res26 at 8192 + 77 (bf16x3), res15 at 4096 + 77 (f32, bf16x3, auto = f16x2 with
flagged clips in both chunks and on both sides of the boundary).  The models and inputs are
the bench's (bench.bench_model, bench.mfcc_like).  Checks: bit-equal to the same batch under a
smaller HONK_RES_CHUNK and to the same clips in a small batch (a clip's arithmetic depends on
neither its chunk nor its place in it), and a sample of clips from every chunk against the
float64 oracle at the mode's own bar."""
import numpy as np
import pytest
import torch

from honk_amd import _native
from oracle import ref_numpy as orc
from golden_util import ref_configs
from test_gpu_bf16 import margin_check
from test_gpu_ordered import ordered
from test_gpu_range import ATOL, DEV, _rel_bound, run

pytestmark = pytest.mark.gpu
ENV = ("HONK_PRECISION", "HONK_RES_KERNEL", "HONK_LAST_KERNEL", "HONK_CONV0", "HONK_F16X2_RERUN", "HONK_RES_CHUNK")
TAIL = 77   # the ragged remainder (odd, fewer clips than CUs)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _native.load()


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)


def spread(lo, hi, n):
    """n clips of [lo, hi), both ends included."""
    return np.unique(np.linspace(lo, hi - 1, n).round().astype(np.int64))


class Case:
    """One bench model, its MFCC-like batch (on the device) and the float64 oracle's logits of
    a sample of clips, computed once."""

    def __init__(self, name, full_chunks, n_oracle, seed, flag=False):
        import bench
        self.name, self.cfg = name, dict(ref_configs()[name])
        self.chunk = 4096 if name == "res15" else 8192
        self.B = full_chunks * self.chunk + TAIL
        self.m = bench.bench_model(name, torch.device(DEV))
        g = torch.Generator(device=DEV)
        g.manual_seed(seed)
        self.x = bench.mfcc_like(self.B, DEV, g)
        self.flag = np.zeros(self.B, bool)
        if flag:  # the admission test's out-of-calibration input: every 64th clip and the boundary's far side
            self.flag[::64] = True
            self.flag[self.chunk:] = True
            self.x[torch.from_numpy(self.flag).to(DEV)] *= 64
        # clips of every chunk, each chunk's first and last among them
        edges = list(range(0, self.B, self.chunk)) + [self.B]
        k = n_oracle * 3 // 8
        per = [k] * full_chunks + [n_oracle - full_chunks * k]
        self.sample = np.concatenate([spread(lo, hi, k) for lo, hi, k in zip(edges[:-1], edges[1:], per)])
        self.small = np.concatenate([spread(lo, hi, k) for lo, hi, k in
                                     zip(edges[:-1], edges[1:], [26] * full_chunks + [TAIL - 26 * full_chunks])])
        assert len(self.small) == TAIL
        if flag:  # more flagged clips of the first chunk, and the boundary's second clip
            self.sample = np.unique(np.concatenate([self.sample, [64, 2048, self.chunk - 64, self.chunk + 1]]))
        params = {k: v.detach().cpu().numpy() for k, v in self.m.state_dict().items() if "num_batches" not in k}
        self.ref = orc.forward(params, self.cfg, self.x[torch.from_numpy(self.sample).to(DEV)].cpu().numpy())

    def loud_frames(self):
        """(x', mask): the calibrated batch with four whole frames at +-100 in every clip = 32
        (mod 64) and every odd clip past the first chunk.  No entry is louder than the
        calibrated c0, so the clip scale stays within HONK_F16X2_DROP_MAX of s_model, while
        the last-layer means leave calibration (float64 oracle on such clips: max|z| = 20.6):
        clips that only tail_sum_kernel flags, in both chunks."""
        mask = np.zeros(self.B, bool)
        mask[32:self.chunk:64] = True
        mask[self.chunk + 1::2] = True
        x = self.x.clone()
        x[torch.from_numpy(self.flag).to(DEV)] /= 64
        sign = torch.tensor([1.0 if (k * 7) % 5 < 2 else -1.0 for k in range(40)], device=DEV)
        frames = torch.tensor([20, 40, 60, 80], device=DEV)
        idx = torch.from_numpy(np.nonzero(mask)[0]).to(DEV)
        x[idx[:, None], frames[None, :]] = 100 * sign
        return x, mask

    def desc(self, prec):
        return self.m._desc(101, 40, prec)

    def set(self, prec):
        self.m.honk_precision = prec
        self.m.honk_reroute = prec == "auto"

    def assert_default_chunk(self, prec):
        """The workspace query follows chunk_clips: the batch's workspace is one default
        chunk's, and a chunk of one clip fewer takes less."""
        lib = _native.load()
        ws = lambda n: lib.honk_res_workspace_bytes(self.desc(prec), n)  # noqa: E731
        assert ws(self.B) == ws(self.chunk) == ws(self.chunk + 1) > ws(self.chunk - 1) > 0, (self.name, prec)

    def small_batch(self, idx=None):
        idx = self.small if idx is None else idx
        return idx, run(self.m, self.x[torch.from_numpy(idx).to(DEV)])


@pytest.fixture(scope="module")
def res8(_need_gpu):
    return Case("res8", 2, 64, seed=31)


@pytest.fixture(scope="module")
def res26(_need_gpu):
    return Case("res26", 1, 16, seed=32)


@pytest.fixture(scope="module")
def res15(_need_gpu):
    return Case("res15", 1, 12, seed=33, flag=True)


def clip_bar(ref, tol=ATOL):
    """The project's bar per clip: absolute to |logit| = 1, relative beyond."""
    return tol * np.maximum(1.0, np.abs(ref).max(axis=1, keepdims=True))


def crossing(c, prec, monkeypatch, other_chunk):
    """The batch under the default chunking and under other_chunk clips per chunk, and the 77
    clips of every chunk as a batch of their own: bit for bit the same logits."""
    c.set(prec)
    full = run(c.m, c.x)
    assert np.isfinite(full).all()
    monkeypatch.setenv("HONK_RES_CHUNK", str(other_chunk))
    assert np.array_equal(run(c.m, c.x), full), f"{c.name} {prec}: default chunks != HONK_RES_CHUNK={other_chunk}"
    monkeypatch.delenv("HONK_RES_CHUNK")
    idx, small = c.small_batch()
    same = (small == full[idx]).all(axis=1)
    assert same.all(), f"{c.name} {prec}: clips {idx[~same]} differ from the same clips in a {TAIL}-clip batch"
    return full


def test_res8_bf16_two_full_chunks_and_a_remainder(res8, monkeypatch):
    """C3's mode and batch shape: 8192-clip chunks of res8 in bf16."""
    c = res8
    c.assert_default_chunk("bf16")
    full = crossing(c, "bf16", monkeypatch, 4096)
    margin_check(full[c.sample], c.ref, f"res8 bf16, {len(c.sample)} of {c.B} clips")


def test_res8_auto_two_full_chunks_and_a_remainder(res8, monkeypatch):
    c = res8
    c.assert_default_chunk("bf16x3")
    full = crossing(c, "auto", monkeypatch, 4096)
    assert c.m.honk_last_precision == "bf16x3"
    err = np.abs(full[c.sample] - c.ref)
    print(f"res8 auto (bf16x3), {len(c.sample)} of {c.B} clips: max|err| {err.max():.2e}")
    assert (err <= ATOL).all()


def test_res26_bf16x3_full_chunk_and_a_remainder(res26, monkeypatch):
    c = res26
    c.assert_default_chunk("bf16x3")
    full = crossing(c, "bf16x3", monkeypatch, 4096)
    err = np.abs(full[c.sample] - c.ref)
    print(f"res26 bf16x3, {len(c.sample)} of {c.B} clips: max|err| {err.max():.2e}")
    assert (err <= ATOL).all()


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_res15_full_chunk_and_a_remainder(res15, prec, monkeypatch):
    """4096 + 77 clips of res15, every 64th clip and the whole remainder x 64."""
    c = res15
    c.assert_default_chunk(prec)
    full = crossing(c, prec, monkeypatch, 1024)
    err = np.abs(full[c.sample] - c.ref)
    print(f"res15 {prec}, {len(c.sample)} of {c.B} clips: max err / bar {(err / clip_bar(c.ref)).max():.3f}")
    assert (err <= clip_bar(c.ref)).all()


def test_res15_auto_flags_across_the_chunk_boundary(res15, monkeypatch):
    """auto = f16x2 with the per-clip admission: the flagged clips (x 64: every 64th clip and
    clips 4096 .. 4172) sit in both chunks and on both sides of the boundary, so the flags,
    the clip scales and the re-run list are indexed past the first chunk."""
    c = res15
    c.assert_default_chunk("bf16x3")   # (f16x2's workspace adds per-batch admission buffers)
    c.set("auto")
    clean = np.nonzero(~c.flag)[0][:8]
    c.small_batch(clean)               # latch auto on calibrated clips
    assert c.m.honk_last_precision == "f16x2" and c.m.honk_last_rerun == 0
    n_flag = int(c.flag.sum())
    assert n_flag == len(range(0, c.B, 64)) + TAIL - 2
    full = run(c.m, c.x)
    assert c.m.honk_last_precision == "f16x2" and c.m.honk_last_rerun == n_flag
    assert np.isfinite(full).all()
    monkeypatch.setenv("HONK_RES_CHUNK", "1024")
    assert np.array_equal(run(c.m, c.x), full) and c.m.honk_last_rerun == n_flag
    monkeypatch.delenv("HONK_RES_CHUNK")
    # unflagged clips: their f16x2 logits, bit for bit, in a small batch
    idx = c.small[~c.flag[c.small]]
    _, small = c.small_batch(idx)
    assert c.m.honk_last_rerun == 0 and np.array_equal(small, full[idx])
    # flagged clips, in a small batch with unflagged ones between them: the same re-run logits
    idx = np.sort(np.concatenate([c.small[c.flag[c.small]], idx[:8]]))
    _, small = c.small_batch(idx)
    assert c.m.honk_last_rerun == int(c.flag[idx].sum()) and np.array_equal(small, full[idx])
    # the sample against the oracle: 1e-4 on the f16x2 clips, the probe's bar on the re-run ones
    err, fl = np.abs(full[c.sample] - c.ref), c.flag[c.sample]
    assert fl.any() and (~fl).any() and (c.sample >= c.chunk).any()
    print(f"res15 auto, {len(c.sample)} of {c.B} clips ({int(fl.sum())} re-run): f16x2 max|err| {err[~fl].max():.2e}, "
          f"re-run max err / bound {(err / _rel_bound(c.ref))[fl].max():.3f}")
    assert (err[~fl] <= clip_bar(c.ref)[~fl]).all()
    assert (err <= _rel_bound(c.ref))[fl].all()
    # the stream-ordered entry: the same logits, the count on the device
    out, count = ordered(c.m, c.x)
    assert count == n_flag and np.array_equal(out, full)
    # x 64 lowers the clip scale past HONK_F16X2_DROP_MAX too, so clip_scale_kernel flags those
    # clips by itself; clips that only the last-layer means flag (loud frames at the calibrated
    # amplitude), again in both chunks: tail_sum_kernel's flags past the first chunk
    x2, loud = c.loud_frames()
    full2 = run(c.m, x2)
    assert c.m.honk_last_rerun == int(loud.sum()) == 64 + TAIL // 2
    assert np.array_equal(full2[~loud & ~c.flag], full[~loud & ~c.flag])
    monkeypatch.setenv("HONK_RES_CHUNK", "1024")
    assert np.array_equal(run(c.m, x2), full2) and c.m.honk_last_rerun == int(loud.sum())
    monkeypatch.delenv("HONK_RES_CHUNK")
    out, count = ordered(c.m, x2)
    assert count == int(loud.sum()) and np.array_equal(out, full2)
    m3_idx = np.nonzero(loud)[0][[0, 1, -2, -1]]   # the re-run clips: a bf16x3 forward of themselves
    c.set("bf16x3")
    np.testing.assert_allclose(full2[m3_idx], run(c.m, x2[torch.from_numpy(m3_idx).to(DEV)]), rtol=0, atol=1e-3)
