"""Non-finite and never-read input entries on the SpeechModel (cnn-*) eval forward
(cnn_nonfinite_cases.py; tests/golden/nonfinite_cnn-*.npz, written by the reference itself:
make_cnn_nonfinite_golden.py).

torch.relu and nn.MaxPool2d propagate a NaN, so the reference's logits for a clip with one NaN /
-NaN / +Inf / -Inf entry it reads are NaN in every logit, and the other clips are untouched.  The
VALID strided convs and floor-mode pools never read some rows and columns ("dead"): NaN or +-Inf
there leaves the reference's logits bit-identical.

On the host: the fixtures' own consistency, the oracle and the CPU module path against the
reference's pattern, the oracle's dead-entry probe against the reference's lists and against
the pinned table of every cnn_geometry_cases geometry, and the admissibility of the range inputs.

On the device (marked gpu), always the module path with honk_precision set:
a. the 12 fixtures, b. every geometry case -- precision x schedule x {default, fast paths off}:
   the reference's (b: the oracle's) per-clip pattern, every finite clip BIT-EQUAL to the same
   batch with the non-finite entries replaced by 0, and within 1e-4 of the reference;
c. 300 clips (past a 256-CU persistent grid) and 17 clips in chunks of 7 on the all-dedicated
   plans: every unpoked clip bit-equal to the clean run;
d. one captured latency graph replayed with a NaN copied in and taken out again (child process);
e. MFCC-like inputs at scale 1 and 2000 against the float64 oracle."""
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
from golden_util import GOLDEN, load_fixture
import cnn_geometry_cases as cgeo
import cnn_nonfinite_cases as nf
from test_gpu_cnn_latency import _device_errors_end_the_run

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"
SCHEDULES = ("throughput", "latency")
UNSPLIT = {v: k for k, v in _native.CNN_SPLIT_OF.items()}


# ---- shared, computed once ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture(name):
    """(cfg, params, model name, x0, x, poke list, dead rows, dead columns, reference logits)"""
    z = np.load(os.path.join(GOLDEN, f"nonfinite_{name}.npz"), allow_pickle=False)
    cfg, params, x0, _, meta = load_fixture(str(z["fixture"]))
    dead_rows, dead_cols = z["dead_rows"].tolist(), z["dead_cols"].tolist()
    x, pk = nf.batch(x0, dead_rows, dead_cols)
    assert nf.crc(x) == int(z["crc"]), "not the batch the reference saw"
    assert pk == [tuple(p) for p in z["pokes"].tolist()]
    for a in (x, z["logits"]):
        a.setflags(write=False)
    return cfg, params, meta["model"], x0, x, pk, dead_rows, dead_cols, z["logits"]


@functools.lru_cache(maxsize=None)
def _geo(case):
    """(x, float64 oracle logits of x, of x without the dead fills): the ten-clip batch on the
    case's own clips with the pinned dead lists.  The two oracle runs have the same shape: the
    oracle's rounding may depend on the batch's shape, never compare across shapes."""
    cfg, params, x0 = cgeo.build(case)
    dead = nf.geo_dead(case.id)
    x, _ = nf.batch(x0[:nf.B], *dead)
    with np.errstate(invalid="ignore", over="ignore"):
        out = orc.forward(params, cfg, x)
        nofill = orc.forward(params, cfg, nf.batch(x0[:nf.B], *dead, fills=False)[0])
    for a in (x, out, nofill):
        a.setflags(write=False)
    return x, out, nofill


def _cpu_module(cfg, params, model_name):
    m = hm.find_model(model_name)(cfg)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
    return m.eval()


# ---- host -----------------------------------------------------------------------------------
def test_the_twelve_cnn_fixtures():
    from golden_util import fixture_names
    assert sorted(nf.NAMES) == [n for n in fixture_names() if n.startswith("cnn")]


@pytest.mark.parametrize("name", nf.NAMES)
def test_fixture_self_consistency(name):
    """The CRC (in _fixture) and the reference's pattern: NaN in every logit of the live pokes,
    finite elsewhere -- the dead-filled clips too."""
    cfg, _, _, x0, x, pk, dead_rows, dead_cols, ref = _fixture(name)
    assert x.shape == (nf.B,) + x0.shape[1:] and ref.shape == (nf.B, cfg["n_labels"])
    assert nf.pattern(ref) == nf.PATTERN
    live = np.ones(x.shape[1:], bool)
    live[dead_rows, :] = False
    live[:, dead_cols] = False
    bad = ~np.isfinite(x)
    for i in range(nf.B):
        assert bool((bad[i] & live).any()) == (i in nf.LIVE_CLIPS), i
        if i in nf.FILLS and (dead_rows or dead_cols):
            assert bad[i][~live].all(), i
    for c, r, w, code in pk:
        assert live[r, w] and x[c, r, w].tobytes() == nf.VALUES[code].tobytes()


@pytest.mark.parametrize("name", nf.NAMES)
def test_oracle_and_cpu_module_pattern(name):
    """orc.forward and the CPU module path show the reference's pattern, and their dead-filled
    clips are bit-equal to their own run of the same batch without the fills."""
    cfg, params, model_name, x0, x, _, dead_rows, dead_cols, ref = _fixture(name)
    nofill = nf.batch(x0, dead_rows, dead_cols, fills=False)[0]
    fills, fin = list(nf.FILL_CLIPS), np.isfinite(ref).all(1)
    with np.errstate(invalid="ignore", over="ignore"):
        out, out0 = orc.forward(params, cfg, x), orc.forward(params, cfg, nofill)
    assert nf.pattern(out) == nf.pattern(ref)
    assert np.array_equal(out[fills], out0[fills])
    np.testing.assert_allclose(out[fin], ref[fin], atol=1e-5, rtol=0)
    m = _cpu_module(cfg, params, model_name)
    with torch.no_grad():
        cpu, cpu0 = m(torch.tensor(x)).numpy(), m(torch.tensor(nofill)).numpy()
    assert nf.pattern(cpu) == nf.pattern(ref)
    assert np.array_equal(cpu[fills], cpu0[fills])
    np.testing.assert_allclose(cpu[fin], ref[fin], atol=1e-5, rtol=0)


@pytest.mark.parametrize("name", nf.NAMES)
def test_oracle_probe_finds_the_reference_dead_entries(name):
    cfg, params, _, x0, _, _, dead_rows, dead_cols, _ = _fixture(name)
    assert nf.probe(params, cfg, x0[0]) == (dead_rows, dead_cols)


def test_geometry_dead_table_names_cases():
    assert set(nf.GEO_DEAD) <= set(cgeo.BY_ID)


@pytest.mark.parametrize("case", cgeo.CASES, ids=repr)
def test_geometry_dead_table(case):
    """The pinned dead lists are what the oracle's probe gives (whole rows and whole columns: a
    ten-clip batch filled on exactly those has the clean pattern, bit-equal in clips 6-8 to the
    equally shaped batch without the fills)."""
    cfg, params, x0 = cgeo.build(case)
    assert nf.probe(params, cfg, x0[0]) == tuple(list(d) for d in nf.geo_dead(case.id))
    _, out, nofill = _geo(case)
    assert nf.pattern(out) == nf.PATTERN
    fills = list(nf.FILL_CLIPS)
    assert np.array_equal(out[fills], nofill[fills])


def _range_case(name, scale):
    cfg, params, *_ = load_fixture(name)
    x = nf.range_batch(name, scale)
    ref = orc.forward(params, cfg, x)
    return cfg, params, x, ref, cgeo.ATOL * max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize("name,scale", nf.RANGE_CASES)
def test_range_inputs_admissible(name, scale):
    """A miss on the device cannot be blamed on the inputs: the float32-accumulating oracle
    stays within a quarter of the bar (cgeo.F32_ORACLE_MAX's rule, scaled like the bar)."""
    cfg, params, x, ref, bar = _range_case(name, scale)
    err = float(np.abs(orc.forward(params, cfg, x, acc=np.float32).astype(np.float64) - ref).max())
    print(f"{name} x{scale:g}: max|logit| {np.abs(ref).max():.4g}, float32 oracle error {err:.3g}, bar {bar:.3g}")
    assert np.isfinite(ref).all() and err <= bar / 4


# ---- device ---------------------------------------------------------------------------------
@pytest.fixture
def gpu(monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _native.load()
    for v in cgeo.ENV_VARS + ("HONK_CNN_SPLITK_SLICE",):
        monkeypatch.delenv(v, raising=False)
    return monkeypatch


def _off(monkeypatch, off):
    for k, v in (cgeo.ALL_OFF if off else {}).items():
        monkeypatch.setenv(k, v)


_MODULES = {}


def _module(key, prec, cfg, params, model_name):
    if (key, prec) not in _MODULES:
        m = _cpu_module(cfg, params, model_name).to(DEV)
        m.honk_precision = prec
        m.honk_reroute = False
        _MODULES[key, prec] = m
    return _MODULES[key, prec]


def _forward(m, x, schedule, prec):
    m.honk_schedule = schedule
    try:
        with _device_errors_end_the_run(f"{prec} / {schedule} on {tuple(np.shape(x))}"):
            with torch.no_grad():
                out = m(torch.tensor(np.asarray(x)).to(DEV))
            torch.cuda.synchronize()
            out = out.cpu().numpy()
    finally:
        m.honk_schedule = "throughput"
    assert m.honk_last_precision == prec
    return out


def _convs(plan):
    """The conv-stack launches of a plan, a split form under its throughput kernel's name."""
    return [UNSPLIT.get(k, k) for k in plan if not k.startswith("linear")]


def _assert_plan(m, prec, schedule, B, want):
    """The launches of this call: the throughput plan `want` itself; under the latency schedule
    its conv stack, every dedicated kernel as its split form."""
    d = _native.CnnDesc(**m._honk_desc, precision=_native.PRECISIONS[prec])
    if schedule == "throughput":
        assert _native.cnn_launch_plan(d) == want
        return
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert B < _native.cnn_latency_threshold(d, cus)
    plan = [k for k, _ in _native.cnn_latency_plan(d, B, cus)]
    assert _convs(plan) == _convs(want), (plan, want)
    assert not [k for k in plan if k in cgeo.FAST]
    assert sum(k in UNSPLIT for k in plan) == sum(k in cgeo.FAST for k in want)


def _check(out, cleaned, ref, what):
    """The three assertions of a ten-clip run."""
    assert nf.pattern(out) == nf.pattern(ref), (what, nf.pattern(out))
    fin = np.isfinite(ref).all(1)
    assert np.array_equal(out[fin], cleaned[fin]), (what, [i for i in np.flatnonzero(fin)
                                                            if not np.array_equal(out[i], cleaned[i])])
    err = float(np.abs(out[fin] - ref[fin]).max())
    print(f"{what}: max|logit - reference| over the finite clips {err:.2e}")
    assert err <= cgeo.ATOL


TRAD_FIXTURES = ("cnn-trad-pool2", "cnn-trad-pool2-12")


@pytest.mark.gpu
@pytest.mark.parametrize("off", (False, True), ids=("default", "alloff"))
@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("prec", cgeo.PRECS)
@pytest.mark.parametrize("name", nf.NAMES)
def test_gpu_fixtures(gpu, name, prec, schedule, off):
    """(a)"""
    cfg, params, model_name, _, x, _, _, _, ref = _fixture(name)
    _off(gpu, off)
    m = _module(name, prec, cfg, params, model_name)
    plan = _native.cnn_launch_plan(_native.CnnDesc(**m._honk_desc, precision=_native.PRECISIONS[prec]))
    if name in TRAD_FIXTURES:  # the service's config: the four dedicated kernels, or none of them
        assert plan[:-1] == cgeo.ALL_FAST[prec][1 if off else 0][:-1]
    else:
        assert not [k for k in plan if k in cgeo.FAST]
    _assert_plan(m, prec, schedule, nf.B, plan)
    out, cleaned = _forward(m, x, schedule, prec), _forward(m, nf.clean(x), schedule, prec)
    _check(out, cleaned, ref, f"{name} {prec} {schedule} {'all off' if off else 'default'}")


@pytest.mark.gpu
@pytest.mark.parametrize("off", (False, True), ids=("default", "alloff"))
@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("prec", cgeo.PRECS)
@pytest.mark.parametrize("case", cgeo.CASES, ids=repr)
def test_gpu_geometries(gpu, case, prec, schedule, off):
    """(b)"""
    cfg, params, _ = cgeo.build(case)
    x, ref, _ = _geo(case)
    _off(gpu, off)
    m = _module(case.id, prec, cfg, params, case.model)
    _assert_plan(m, prec, schedule, nf.B, case.plan(prec, off))
    out, cleaned = _forward(m, x, schedule, prec), _forward(m, nf.clean(x), schedule, prec)
    _check(out, cleaned, ref, f"{case} {prec} {schedule} {'all off' if off else 'default'}")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", cgeo.PRECS)
@pytest.mark.parametrize("cid,off", [("trad-101x39", False), ("trad-100x40", False), ("trad-72x40", True)])
def test_gpu_persistent_workgroups_and_chunks(gpu, cid, off, prec):
    """(c) 300 clips with clips 0-3 and 296-299 poked (clips 256-259 run on the workgroups that
    have just processed 0-3), and 17 clips in chunks of 7 with a NaN in the last clip of a
    chunk, the first of the next and the last of the batch."""
    case = cgeo.BY_ID[cid]
    cfg, params, x0 = cgeo.build(case)
    dead = nf.geo_dead(cid)
    _off(gpu, off)
    m = _module(cid, prec, cfg, params, case.model)
    _assert_plan(m, prec, "throughput", nf.BIG, case.plan(prec, off))
    if not off:
        assert case.fast(prec) == [k for k in cgeo.ALL_FAST[prec][0] if k in cgeo.FAST]
    x = nf.big_batch(x0, *dead)
    base, out = _forward(m, x0[:nf.BIG], "throughput", prec), _forward(m, x, "throughput", prec)
    assert np.isfinite(base).all()
    poked = sorted(nf.BIG_POKES)
    rest = [i for i in range(nf.BIG) if i not in nf.BIG_POKES]
    assert np.array_equal(out[rest], base[rest]), [i for i in rest if not np.array_equal(out[i], base[i])]
    assert dict(zip(poked, nf.pattern(out[poked]))) == nf.BIG_PATTERN
    deadfill = [i for i in poked if nf.BIG_POKES[i][0] == "dead"]
    assert np.array_equal(out[deadfill], base[deadfill])
    # the same clips at batch 10: the same pattern
    small = _forward(m, x[poked + [4, 5]], "throughput", prec)
    assert nf.pattern(small[:len(poked)]) == nf.pattern(out[poked])
    # chunks
    _, r, c, _ = nf.pokes(case.H, case.W, *dead)[0]
    xc = np.array(x0[:nf.CHUNK_B])
    xc[list(nf.CHUNK_CLIPS), r, c] = np.nan
    gpu.setenv("HONK_CNN_CHUNK", str(nf.CHUNK))
    for schedule in SCHEDULES:
        got = _forward(m, xc, schedule, prec)
        assert nf.pattern(got) == ["nan" if i in nf.CHUNK_CLIPS else "finite" for i in range(nf.CHUNK_B)], schedule
        keep = [i for i in range(nf.CHUNK_B) if i not in nf.CHUNK_CLIPS]
        if schedule == "throughput":
            assert np.array_equal(got[keep], base[keep])
        else:
            assert np.array_equal(got[keep], _forward(m, x0[:nf.CHUNK_B], schedule, prec)[keep])


@pytest.fixture(scope="module")
def graph_child(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = str(tmp_path_factory.mktemp("cnn_nonfinite_graph") / "child.npz")
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "cnn_nonfinite_graph_child.py"), out],
                           capture_output=True, text=True, timeout=180)
    except subprocess.TimeoutExpired:
        pytest.exit("tests/cnn_nonfinite_graph_child.py (graph capture / replay) hung: stopping the GPU run", 1)
    if p.returncode < 0 or p.returncode in (134, 139):
        pytest.exit(f"tests/cnn_nonfinite_graph_child.py died with status {p.returncode}: stopping the GPU run\n"
                    f"{p.stderr[-3000:]}", 1)
    assert p.returncode == 0, p.stderr[-3000:]
    return np.load(out)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", cgeo.PRECS)
def test_gpu_captured_replay(graph_child, prec):
    """(d) replay clean, with a live NaN copied into clip 1 of the static input, and with it
    taken out again."""
    clean0, poked, clean1 = (graph_child[f"{prec}_{k}"] for k in ("clean", "poked", "restored"))
    assert clean0.shape == (3, 4)
    assert nf.pattern(clean0) == ["finite"] * 3 and nf.pattern(clean1) == ["finite"] * 3
    assert nf.pattern(poked) == ["finite", "nan", "finite"]
    for other in (poked, clean1):
        assert np.array_equal(other[[0, 2]], clean0[[0, 2]])
    assert np.array_equal(clean1, clean0)
    assert np.array_equal(clean0, graph_child[f"{prec}_eager"])
    ref = _fixture("cnn-trad-pool2")[8]
    assert float(np.abs(clean0 - ref[[0, 5, 0]]).max()) <= cgeo.ATOL  # clips 0, 1, 2 of the tiled fixture


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("prec", cgeo.PRECS)
@pytest.mark.parametrize("name,scale", nf.RANGE_CASES)
def test_gpu_range(gpu, name, scale, prec, schedule):
    """(e)"""
    cfg, params, x, ref, bar = _range_case(name, scale)
    m = _module(name, prec, cfg, params, load_fixture(name)[4]["model"])
    out = _forward(m, x, schedule, prec)
    err = float(np.abs(out - ref).max())
    print(f"{name} x{scale:g} {prec} {schedule}: max|logit - oracle| {err:.3g} (bar {bar:.3g}, max|logit| "
          f"{np.abs(ref).max():.4g})")
    assert err <= bar
