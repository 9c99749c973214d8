"""The fused pair / last-layer kernels (block16p_kernel, block16l_kernel) at the edges of a
workgroup's stream, where the A waves' software-pipelined DMA descriptors can go wrong:

* the prologue (step 0's descriptors are derived before the step loop) and the last steps
  (the frontier clamps at the stream's last row and the count of new rows falls to 0);
* workgroups with no clip, one clip, an uneven split and several clips (table refills,
  prologue and clamp in one stream), streams of different length in one workgroup;
* 13- and 20-pixel rows (up to three row wraps per m-tile, more rows per step);
* last-layer mode, which restarts the walk -- and the descriptors -- at every clip;
* the linear DMA of the bf16 two-stream pairs, which keeps its own piece counters.

Every check is bitwise: the pair computes what two single-layer launches compute, a clip's
logits do not depend on its place in the batch, and the DMA variants move the same bytes."""
import warnings

import numpy as np
import pytest
import torch

from honk_amd import _native
from honk_amd import model as hm
from oracle import ref_numpy as orc
from golden_util import ref_configs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _native.load()


def _module(cfg, params, name, prec):
    m = hm.find_model(name)(cfg)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
    m = m.eval().to(DEV)
    m.honk_precision = prec
    m.honk_reroute = False   # the kernels of `prec` themselves, pooled maps included
    return m


def _run(m, x):
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)   # no silent fallback to the fp32 layer path
        with torch.no_grad():
            out = m(torch.tensor(x).to(DEV))   # (a copy: the shared clips are read-only)
    torch.cuda.synchronize()
    return out.cpu().numpy()


_CASES = {}


def _case(name, override, prec, nmax, seed):
    """One calibrated random model and nmax clips per (config, precision), shared by the
    batch sizes of a test (a batch is the first B clips)."""
    key = (name, tuple(sorted(override.items())), prec)
    if key not in _CASES:
        cfg = dict(ref_configs()[name])
        cfg.update(override)
        rng = np.random.Generator(np.random.PCG64(seed))
        params = orc.make_params(cfg, seed)
        params = orc.calibrate_bn(params, cfg, rng.standard_normal((2, 101, 40)).astype(np.float32), seed=seed)
        x = rng.standard_normal((nmax, 101, 40)).astype(np.float32)
        x.setflags(write=False)
        _CASES[key] = (_module(cfg, params, name, prec), x)
    return _CASES[key]


def _pair_vs_w(monkeypatch, m, x):
    B = len(x)
    monkeypatch.setenv("HONK_RES_KERNEL", "p")
    monkeypatch.setenv("HONK_LAST_KERNEL", "w")
    plan = _native.res_launch_plan(m._desc(101, 40), B)
    assert "block16p_kernel" in plan and "block16l_kernel" not in plan, plan
    outp = _run(m, x)
    monkeypatch.setenv("HONK_RES_KERNEL", "w")
    assert "block16p_kernel" not in _native.res_launch_plan(m._desc(101, 40), B)
    outw = _run(m, x)
    assert np.isfinite(outw).all()
    assert np.array_equal(outp, outw), float(np.abs(outp - outw).max())


# one clip on one workgroup (the others return at once), two, a clip per workgroup minus
# one / exactly / plus one (a single two-clip stream), an uneven split (513), four clips per
# workgroup (several table refills, prologue and clamp in one stream)
@pytest.mark.parametrize("B", [1, 2, 255, 256, 257, 513, 1024])
def test_f16x2_res15_pair_bitwise_vs_w_at_workgroup_edges(monkeypatch, B):
    m, x = _case("res15", {}, "f16x2", 1024, seed=61)
    _pair_vs_w(monkeypatch, m, x[:B])


# 20- and 13-pixel rows (res26, res8: up to three row wraps per m-tile, up to five new rows
# per step), 33 maps, undilated five layers -- at the small end
OTHER_GEOMETRIES = [("res26", {}), ("res8", {}), ("res15", dict(n_feature_maps=33)),
                    ("res15", dict(use_dilation=False, n_layers=5))]


@pytest.mark.parametrize("B", [1, 2, 257])
@pytest.mark.parametrize("name,override", OTHER_GEOMETRIES)
def test_f16x2_other_geometries_pair_bitwise_vs_w_small(monkeypatch, name, override, B):
    m, x = _case(name, override, "f16x2", 257, seed=62)
    _pair_vs_w(monkeypatch, m, x[:B])


def test_f16x2_last_layer_restarts_per_clip():
    """block16l_kernel runs a stream's clips one at a time and restarts the walk -- with it the
    pipelined DMA descriptors -- at each: three clips computed alone, first in a 515-clip batch
    and last in it (the third pass of a workgroup's stream) give the same logits bit for bit."""
    m, x = _case("res15", {}, "f16x2", 1024, seed=61)
    assert _native.res_launch_plan(m._desc(101, 40), 3)[-1] == "block16l_kernel"
    assert _native.res_launch_plan(m._desc(101, 40), 515)[-1] == "block16l_kernel"
    alone = _run(m, x[:3])
    assert np.isfinite(alone).all()
    xb = np.concatenate([x[:3], x[3:512], x[:3]])
    assert len(xb) == 515
    big = _run(m, xb)
    assert np.array_equal(big[:3], alone), float(np.abs(big[:3] - alone).max())
    assert np.array_equal(big[-3:], alone), float(np.abs(big[-3:] - alone).max())


@pytest.mark.parametrize("B", [1, 2, 257])
def test_bf16_res8_linear_dma_and_streams_bitwise(monkeypatch, B):
    """res8 in bf16: the default plan (two streams per workgroup, the A-in rows copied linearly
    in 1-KiB pieces with their own piece counters) against the row pieces (HONK_PAIR_LIN=0) and
    against one stream per workgroup (HONK_PAIR_STREAMS=1), bit for bit."""
    m, x = _case("res8", {}, "bf16", 257, seed=63)
    x = x[:B]
    for v in ("HONK_PAIR_LIN", "HONK_PAIR_STREAMS", "HONK_RES_KERNEL", "HONK_LAST_KERNEL"):
        monkeypatch.delenv(v, raising=False)
    assert "block16p_kernel" in _native.res_launch_plan(m._desc(101, 40), B)
    out = _run(m, x)
    assert np.isfinite(out).all()
    monkeypatch.setenv("HONK_PAIR_LIN", "0")
    assert "block16p_kernel" in _native.res_launch_plan(m._desc(101, 40), B)
    outr = _run(m, x)
    assert np.array_equal(out, outr), float(np.abs(out - outr).max())
    monkeypatch.delenv("HONK_PAIR_LIN")
    monkeypatch.setenv("HONK_PAIR_STREAMS", "1")
    if "block16p_kernel" in _native.res_launch_plan(m._desc(101, 40), B):   # where the plan allows it
        out1 = _run(m, x)
        assert np.array_equal(out, out1), float(np.abs(out - out1).max())
