"""GPU: the res TRAINING kernels off 101 x 40 and past one tile per workgroup.

Every case of train_geometry_cases.py (whose plan test_train_geometry_plan.py pins: the kernel
a run here is about is the one the table names) at 2 clips and, for the many-tile cases, at
batches sized from the device's CU count so that a workgroup of the LDS-DMA kernels walks two
and three tiles (both buffers reused; the statistics epilogue's per-lane sums and its
deferred epilogue carry across tiles of different clips):

* kernel level: forward / input gradient / weight gradient vs float64 on the CPU (1e-5 of each
  result's max |value|); the bitwise contracts d == m == VALU, q == h == d, fixed == runtime
  geometry; the fused epilogue (s, ReLU mask words) bit-equal to composed fp32 ops on the plain
  conv's h, zero-weight channel, -0.0 and NaN included; the statistics that reach the tails vs
  the float64 statistics of that s; MODE 2 and the masked tail backward vs the float64
  BatchNorm backward; the folded forms bit-equal to the unfolded ones; the large-mean input;
* step level: one native step of res15-narrow, res26-narrow (6 layers), res8-narrow and res15
  on inputs that put the block maps on the table, vs the decision-matched float64 step
  (tests/decision_replay.py; the bounds of test_train_golden.py), with STATS_USED / FOLD_USED
  as honk_conv3x3_plan predicts, and the FUSE_TAIL / FOLD_BN bit-identities.
"""
import functools
import warnings

import pytest
import torch
import torch.nn.functional as F

import decision_replay as dr
import train_geometry_cases as geo
from honk_amd import _native
from honk_amd import conv3x3 as hc
from honk_amd import model as hm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ZERO_CH = 5      # the output channel with all-zero weights


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _native.load()


@pytest.fixture(autouse=True)
def _default_env(monkeypatch):
    for v in geo.ENV_VARS:
        monkeypatch.delenv(v, raising=False)


@functools.lru_cache(maxsize=None)
def n_cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _batches(case):
    """2 clips; a many-tile case also at two and three tiles per workgroup of each of its DMA
    kernels (the conv's and the weight gradient's bands may differ)."""
    if not case.many:
        return [2]
    return [2] + [b for nb in sorted(set(case.nband())) for b in geo.many_tile_batches(nb, n_cus())]


def _params(pred=lambda c: True):
    return [pytest.param(c, i, id=f"{c.id}-b{i}") for c in geo.CASES if pred(c)
            for i in range(1 + 2 * len(set(c.nband())) if c.many else 1)]


def _batch(case, i):
    return _batches(case)[i]


def _tiles_per_wg(case, B):
    p = _native.conv3x3_plan(B, *case.shape, 0)
    return tuple(-(-B * p[k]["nband"] // p[k]["grid"]) for k in ("conv", "wgrad"))


def _data(case, B):
    C, H, W, d = case.shape
    g = torch.Generator(device=DEV).manual_seed(1000 * C + 37 * H + 5 * W + d + B)
    t = dict(x=torch.randn(B, C, H, W, device=DEV, generator=g), dy=torch.randn(B, C, H, W, device=DEV, generator=g),
             old=torch.randn(B, C, H, W, device=DEV, generator=g), gs=torch.randn(B, C, H, W, device=DEV, generator=g),
             w=torch.randn(C, C, 3, 3, device=DEV, generator=g) * 0.1,
             w2=torch.randn(C, C, 3, 3, device=DEV, generator=g) * 0.1)
    t["w"][ZERO_CH] = 0.0
    t["w2"][ZERO_CH] = 0.0
    t["old"][0, ZERO_CH, 0, 0] = -0.0
    return t


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _biteq(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _clips(B):
    """The clips a large batch's conv outputs are compared with float64 on: 8 spread over the
    batch and the last (every clip enters the bitwise comparisons and the weight gradient)."""
    return list(range(B)) if B <= 16 else sorted(set(range(0, B, B // 8)) | {B - 1})


def _ref_conv(x, w, d, flip, idx):
    x64, w64 = x[idx].double().cpu(), w.double().cpu()
    if flip:
        return torch.nn.grad.conv2d_input(x64.shape, w64, x64, padding=d, dilation=d)
    return F.conv2d(x64, w64, padding=d, dilation=d)


def _ref_wgrad(x, dy, d):
    return torch.nn.grad.conv2d_weight(x.double().cpu(), (x.shape[1],) * 2 + (3, 3), dy.double().cpu(), padding=d,
                                       dilation=d)


@pytest.mark.parametrize("case,bi", _params())
def test_kernels_match_float64(monkeypatch, case, bi):
    """Forward, input gradient and weight gradient vs float64 conv2d / conv2d_input /
    conv2d_weight on the CPU: 1e-5 of each result's max |value| (the bar of
    test_conv3x3_kernels_match_float64).  45 maps: the default route (same-conv forward,
    VALU weight gradient) and conv3x3_kernel<45, NP> (HONK_TRAIN_CONV=v), bit-equal; a shape
    the dedicated kernels refuse runs on the same-conv path with no error."""
    B = _batch(case, bi)
    C, H, W, d = case.shape
    t = _data(case, B)
    assert hc._dedicated(C, H, W, d) == (case.family() is not None)
    if case.family() is not None:
        assert geo.signature(B, C, H, W, d, n_cus())[0] == case.sigs["default"]
        print(case, "B", B, "tiles per workgroup (conv, wgrad):", _tiles_per_wg(case, B))
    idx = _clips(B)
    y, dx, dw = hc._conv(t["x"], t["w"], flip=False, d=d), hc._conv(t["dy"], t["w"], flip=True, d=d), \
        hc._wgrad(t["x"], t["dy"], d=d)
    errs = (_rel(y[idx], _ref_conv(t["x"], t["w"], d, False, idx)), _rel(dx[idx], _ref_conv(t["dy"], t["w"], d, True, idx)),
            _rel(dw, _ref_wgrad(t["x"], t["dy"], d)))
    print(case, "B", B, "fwd / dgrad / wgrad vs float64: %.2e %.2e %.2e" % errs)
    assert max(errs) < 1e-5, errs
    assert float(y[:, ZERO_CH].abs().max()) == 0.0
    if C == 45 and case.family() is not None:
        monkeypatch.setenv("HONK_TRAIN_CONV", "v")
        assert hc._dedicated_conv(C, H, W, d)
        assert torch.equal(hc._conv(t["x"], t["w"], flip=False, d=d), y)
        assert torch.equal(hc._conv(t["dy"], t["w"], flip=True, d=d), dx)


@pytest.mark.parametrize("case,bi", _params(lambda c: c.C == 19 and c.family() in (("d", "d"), ("d", "v"), ("m", "m"), ("m", "v"))))
def test_bitwise_contracts(case, bi):
    """Wherever the plan says two kernels apply: d == m == VALU for forward and input
    gradient, q == h == d for the weight gradient, the compile-time instances == the runtime
    geometry."""
    B = _batch(case, bi)
    C, H, W, d = case.shape
    t = _data(case, B)

    def run(env):
        with geo.environment(env):
            assert geo.signature(B, C, H, W, d, n_cus())[0] == case.sigs[env], env
            return (hc._conv(t["x"], t["w"], flip=False, d=d), hc._conv(t["dy"], t["w"], flip=True, d=d),
                    hc._wgrad(t["x"], t["dy"], d=d))

    base = run("default")
    for env in ("m", "v"):
        if case.family(env)[0] != case.family()[0]:
            o = run(env)
            assert torch.equal(o[0], base[0]) and torch.equal(o[1], base[1]), env
    if case.family()[1] == "d":
        for env in ("wh", "wd"):
            assert torch.equal(run(env)[2], base[2]), env
    if "F" in case.sigs["default"]:
        o = run("nofix")
        assert all(torch.equal(u, v) for u, v in zip(o, base))
        if case.family()[1] == "d":   # the d and h weight-gradient kernels' instances too
            for env in ("wd", "wh"):
                with geo.environment(env, HONK_TD_FIXED="0"):
                    assert torch.equal(hc._wgrad(t["x"], t["dy"], d=d), base[2]), env


def _mask_bits(h):
    """The packed ReLU decision !(h <= 0) of [B, C, H, W]: one int32 word per pixel, bit o."""
    C = h.shape[1]
    on = ~(h <= 0)
    sh = torch.arange(C, device=h.device, dtype=torch.int32).view(1, C, 1, 1)
    return (on.to(torch.int32) << sh).sum(1, dtype=torch.int32)


def _bn64(s):
    """float64 train BatchNorm of s (affine=False, eps 1e-5): y, mean, biased var, n."""
    s64 = s.detach().double().cpu()
    n = s64.numel() // s64.shape[1]
    mean = s64.mean(dim=(0, 2, 3), keepdim=True)
    var = s64.var(dim=(0, 2, 3), unbiased=False, keepdim=True)
    return (s64 - mean) / torch.sqrt(var + 1e-5), mean, var, n


def _check_tail_forward(what, s, y, bn):
    """honk_res_tail_fwd_s_f32 on the conv epilogue's statistics vs the float64 statistics of
    that s: y within 1e-6 of its max, running stats rtol 1e-5 / atol 1e-6 (the bars of
    test_batchnorm_train_matches_torch)."""
    y64, mean, var, n = _bn64(s)
    if y is not None:
        e = _rel(y, y64)
        print(what, "y vs float64: %.2e" % e)
        assert e < 1e-6, (what, e)
    rm = 0.1 * mean.flatten()
    rv = 0.9 + 0.1 * var.flatten() * n / (n - 1)
    print(what, "running mean / var max abs err: %.2e %.2e" % (
        float((bn.running_mean.double().cpu() - rm).abs().max()), float((bn.running_var.double().cpu() - rv).abs().max())))
    torch.testing.assert_close(bn.running_mean.double().cpu(), rm, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(bn.running_var.double().cpu(), rv, rtol=1e-5, atol=1e-6)
    return y64, mean, var


def _bn_bwd64(gy, y64, var, mask=None, gs=None):
    """float64 BatchNorm backward (+ the residual's gs, x the ReLU mask)."""
    gy64 = gy.detach().double().cpu()
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    g = invstd * (gy64 - gy64.mean(dim=(0, 2, 3), keepdim=True) - y64 * (gy64 * y64).mean(dim=(0, 2, 3), keepdim=True))
    if gs is not None:
        g = g + gs.detach().double().cpu()
    return g, (g * mask.double().cpu() if mask is not None else None)


def _chain(case, t, fold):
    """Two blocks as SpeechResModel._torch_forward chains them: conv (MODE 1 epilogue: s, mask,
    statistics) -> tail (residual, keeps s) -> conv (MODE 1, no residual; its input gradient
    is the MODE 2 conv that sums the first tail's backward statistics) -> tail.  fold: the
    first tail writes no y, the second conv / its input gradient / its weight gradient / the
    first tail's backward read (s - mean) * invstd."""
    C, H, W, d = case.shape
    leaf = {k: t[k].clone().requires_grad_(True) for k in ("x", "old", "w", "w2")}
    bn1, bn2 = (torch.nn.BatchNorm2d(C, affine=False).to(DEV).train() for _ in range(2))
    used0, fold0 = dict(hc.STATS_USED), hc.FOLD_USED["n"]
    box1, box2 = {}, {}
    h1 = hc.conv3x3(leaf["x"], leaf["w"], d, old=leaf["old"], box_out=box1)
    out = dict(m1=box1["mask"].clone(), s1=h1.detach().clone())
    h1.retain_grad()
    y1, s1 = hc.res_tail(h1, leaf["old"], bn1, keep_s=True, box=box1, fold=fold)
    h2 = hc.conv3x3(y1, leaf["w2"], d, old=None, box_out=box2, box_in=box1)
    out.update(m2=box2["mask"].clone(), s2=h2.detach().clone())
    h2.retain_grad()
    y2 = hc.res_tail(h2, None, bn2, box=box2)
    # the MODE 2 conv's output (the gradient of y1) as the first tail's backward receives it:
    # observed at the call, not through a tensor hook (the tail takes the conv's statistics
    # only for the very tensor the conv returned)
    mode2, orig = [], hc._conv_stats

    def spy(x, w, flip, dil, mode, aux, buf, fold=None):
        y = orig(x, w, flip, dil, mode, aux, buf, fold)
        mode2.append((mode, flip, y))
        return y

    hc._conv_stats = spy
    try:
        torch.autograd.backward([y2, s1], [t["dy"], t["gs"]])
    finally:
        hc._conv_stats = orig
    assert [(m, f) for m, f, _ in mode2] == [(2, True)]
    assert {k: hc.STATS_USED[k] - used0[k] for k in used0} == {"fwd": 2, "bwd": 1}
    assert hc.FOLD_USED["n"] - fold0 == int(fold)
    out.update(y1=None if fold else y1.detach(), y2=y2.detach(), gh1=h1.grad, gh2=h2.grad, gy1=mode2[0][2].detach(),
               gx=leaf["x"].grad, gold=leaf["old"].grad, gw=leaf["w"].grad, gw2=leaf["w2"].grad,
               rm1=bn1.running_mean.clone(), rv1=bn1.running_var.clone(), rm2=bn2.running_mean.clone(),
               rv2=bn2.running_var.clone())
    return out, bn1, bn2


@pytest.mark.parametrize("case,bi", _params(lambda c: "s" in c.flags()))
def test_fused_epilogue_chain(case, bi):
    """The statistics-epilogue kernels of a DMA case, each against a reference of its own
    inputs (the GPU's upstream tensors), so every bar is one kernel's."""
    B = _batch(case, bi)
    C, H, W, d = case.shape
    t = _data(case, B)
    can_fold = "f" in case.flags()
    assert hc.FUSE_TAIL and hc.FOLD_BN
    assert bool(_native.load().honk_conv3x3_bn_fold_check(B, C, H, W, d) == 0) == can_fold
    print(case, "B", B, "tiles per workgroup (conv, wgrad):", _tiles_per_wg(case, B))
    r, bn1, bn2 = _chain(case, t, fold=False)
    # -- MODE 1: s and the mask words are composed fp32 ops on the plain conv's h
    h1 = hc._conv(t["x"], t["w"], flip=False, d=d)
    assert _biteq(r["s1"], torch.relu(h1) + t["old"])
    assert torch.equal(r["m1"], _mask_bits(h1)) and int((r["m1"] >> C).abs().max()) == 0
    assert float(h1[:, ZERO_CH].abs().max()) == 0.0 and int(((r["m1"] >> ZERO_CH) & 1).max()) == 0
    h2 = hc._conv(r["y1"], t["w2"], flip=False, d=d)
    assert _biteq(r["s2"], torch.relu(h2))
    assert torch.equal(r["m2"], _mask_bits(h2)) and int((r["m2"] >> C).abs().max()) == 0
    # -- the statistics that reach honk_res_tail_fwd_s_f32
    y1_64, _, var1 = _check_tail_forward(f"{case} B {B} tail 1", r["s1"], r["y1"], bn1)
    y2_64, _, var2 = _check_tail_forward(f"{case} B {B} tail 2", r["s2"], r["y2"], bn2)
    # -- the last tail's backward (its own statistics), MODE 2, the first tail's backward
    on1 = ((r["m1"].unsqueeze(1) >> torch.arange(C, device=DEV, dtype=torch.int32).view(1, C, 1, 1)) & 1).bool()
    on2 = ((r["m2"].unsqueeze(1) >> torch.arange(C, device=DEV, dtype=torch.int32).view(1, C, 1, 1)) & 1).bool()
    _, gh2_64 = _bn_bwd64(t["dy"], y2_64, var2, mask=on2)
    idx = _clips(B)
    assert torch.equal(r["gy1"], hc._conv(r["gh2"], t["w2"], flip=True, d=d))    # MODE 2 == MODE 0
    g1_64, gh1_64 = _bn_bwd64(r["gy1"], y1_64, var1, mask=on1, gs=t["gs"])
    errs = dict(gh2=_rel(r["gh2"], gh2_64), gy1=_rel(r["gy1"][idx], _ref_conv(r["gh2"], t["w2"], d, True, idx)),
                gh1=_rel(r["gh1"], gh1_64), gold=_rel(r["gold"], g1_64),
                gw2=_rel(r["gw2"], _ref_wgrad(r["y1"], r["gh2"], d)), gw=_rel(r["gw"], _ref_wgrad(t["x"], r["gh1"], d)),
                gx=_rel(r["gx"][idx], _ref_conv(r["gh1"], t["w"], d, True, idx)))
    print(case, "B", B, "backward vs float64:", {k: "%.2e" % v for k, v in errs.items()})
    assert max(errs.values()) < 1e-5, errs
    # -- the folded forms: bit-equal to the unfolded ones fed the materialized y
    if can_fold:
        f, _, _ = _chain(case, t, fold=True)
        for k in r:
            if k != "y1":
                assert _biteq(r[k], f[k]), k


@pytest.mark.parametrize("case", [c for c in geo.CASES if "s" in c.flags()], ids=repr)
@pytest.mark.parametrize("res", [False, True])
def test_fused_epilogue_nan_pixel(case, res):
    """A NaN input pixel: s and the mask words still equal torch's relu [+ old] and
    threshold_backward on the plain conv's h (a NaN passes the ReLU and keeps its gradient)."""
    C, H, W, d = case.shape
    t = _data(case, 2)
    x = t["x"].clone()
    x[0, 3, H // 2, W // 2] = float("nan")
    old = t["old"] if res else None
    box = {}
    with torch.no_grad():
        s = hc.conv3x3(x, t["w"], d, old=old, box_out=box)
        h = hc._conv(x, t["w"], flip=False, d=d)
        ref = torch.relu(h) + old if res else torch.relu(h)
        keep = torch.ops.aten.threshold_backward(torch.ones_like(h), h, 0.0) != 0
    nan = torch.isnan(h)
    assert int(nan.sum()) >= C - 1 and torch.equal(torch.isnan(s), nan) and torch.equal(torch.isnan(ref), nan)
    assert _biteq(torch.where(nan, torch.zeros_like(s), s), torch.where(nan, torch.zeros_like(ref), ref))
    assert torch.equal(keep, ~(h <= 0)) and bool(keep[nan].all())
    assert torch.equal(box["mask"], _mask_bits(h))


@pytest.mark.parametrize("case", [c for c in geo.CASES if c.many], ids=repr)
def test_fused_tail_statistics_large_mean_many_tiles(case):
    """test_fused_tail_statistics_large_mean's input (s ~ 300 + 0.01 N(0, 1)) with three tiles
    on a workgroup: the per-lane pivoted sums carry across tiles of different clips; mean
    within 1e-6, variance within 1e-3 of the float64 statistics of s (that test's bars)."""
    C, H, W, d = case.shape
    B = geo.many_tile_batches(case.nband()[0], n_cus())[1]
    assert _tiles_per_wg(case, B)[0] == 3
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(B, C, H, W, device=DEV, generator=g) * 0.01
    w = torch.randn(C, C, 3, 3, device=DEV, generator=g) * 0.1
    old = 300.0 + torch.randn(B, C, H, W, device=DEV, generator=g) * 0.01
    bn = torch.nn.BatchNorm2d(C, affine=False, momentum=1.0).to(DEV).train()   # running = batch stats
    box = {}
    with torch.no_grad():
        h = hc.conv3x3(x, w, d, old=old, box_out=box)
        assert "mask" in box
        hc.res_tail(h, old, bn, keep_s=True, box=box)
        s64 = (torch.relu(hc._conv(x, w, flip=False, d=d)) + old).double()
    mean, var = s64.mean(dim=(0, 2, 3)), s64.var(dim=(0, 2, 3), unbiased=True)
    rv = float(((bn.running_var.double() - var).abs() / var).max())
    print(case, "B", B, "running_mean rel err %.2e running_var rel err %.2e" % (_rel(bn.running_mean, mean), rv))
    assert _rel(bn.running_mean, mean) < 1e-6
    assert rv < 1e-3


# ---- step level ------------------------------------------------------------------------------
def _cfg(step):
    cfg = dict(hm.find_config(step.model))
    cfg.update(step.override)
    return cfg


def _step_batches(step):
    """The step's small batch; a many-tile step also at a batch past one tile per workgroup
    of its DMA case of the most bands (three tiles on maps of <= 64 pixels, else two: the
    float64 replay of the step stays at a few seconds)."""
    if not step.many:
        return [step.B]
    nb = max(c.nband()[0] for c in geo.step_cases(step, _cfg(step)) if c.family() == ("d", "d"))
    b2, b3 = geo.many_tile_batches(nb, n_cus())
    return [step.B, b3 if step.maps[0] * step.maps[1] <= 64 else b2]


def _step_params():
    return [pytest.param(s, i, id=f"{s.id}-b{i}") for s in geo.STEPS for i in range(2 if s.many else 1)]


def _predict(step, cfg, B):
    """(STATS_USED fwd, bwd, FOLD_USED) of one step, from honk_conv3x3_plan at the device's CU
    count: a tail takes its conv's epilogue statistics (fwd) and the next conv's MODE 2 ones
    (bwd); it folds its BatchNorm when the next conv has all the folded kernels."""
    plans = [_native.conv3x3_plan(B, cfg["n_feature_maps"], *step.maps, d, 0) for d in geo.dilations(cfg)]
    st = [bool(p and p["stats"]) for p in plans]
    fo = [bool(p and p["fold"]) for p in plans]
    return sum(st), sum(st[1:]), sum(a and b for a, b in zip(st[:-1], fo[1:]))


def _run_step(step, cfg, B, record=False):
    torch.manual_seed(11)
    m = hm.find_model(step.model)(cfg)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    m = m.to(DEV).train()
    g = torch.Generator().manual_seed(12 + B)
    x = torch.randn(B, step.H, step.W, generator=g)
    y = torch.randint(0, cfg["n_labels"], (B,), generator=g)
    dec = dr.Decisions()
    used0, fold0 = dict(hc.STATS_USED), hc.FOLD_USED["n"]
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)   # no fallback to PyTorch / MIOpen
        if record:
            with dr.record(dec):
                loss = F.cross_entropy(m(x.to(DEV)), y.to(DEV))
        else:
            loss = F.cross_entropy(m(x.to(DEV)), y.to(DEV))
        loss.backward()
    used = (hc.STATS_USED["fwd"] - used0["fwd"], hc.STATS_USED["bwd"] - used0["bwd"], hc.FOLD_USED["n"] - fold0)
    return dict(loss=loss.detach(), g={k: p.grad.detach().clone() for k, p in m.named_parameters()},
                b={k: v.detach().clone() for k, v in m.state_dict().items() if "running_" in k}, used=used, dec=dec,
                state=state, x=x, y=y)


@pytest.mark.parametrize("step,bi", _step_params())
def test_train_step_vs_decision_matched_float64(step, bi):
    """One native step vs the float64 step with the GPU's own decisions: gradients 1e-4
    relative, loss 1e-5, running stats 1e-5, no ambiguous decision (test_train_golden.py's
    bounds), no fallback warning, and the fused paths taken exactly where the plan says."""
    cfg = _cfg(step)
    B = _step_batches(step)[bi]
    r = _run_step(step, cfg, B, record=True)
    assert r["used"] == _predict(step, cfg, B), (r["used"], _predict(step, cfg, B))
    if any(c.family() == ("d", "d") for c in geo.step_cases(step, cfg)):
        assert r["used"][0] > 0 and r["used"][2] > 0
    ref = dr.replay_step(cfg, step.model, r["state"], r["x"].numpy(), r["y"].numpy(), r["dec"], dict(lr=0.1, momentum=0.9))
    got = (max(dr.rel_err(r["g"][k].cpu().numpy(), ref["g"][k]) for k in ref["g"]),
           abs(float(r["loss"].item()) - ref["loss"]),
           max(dr.rel_err(r["b"][k].cpu().numpy(), ref["b"][k]) for k in ref["b"]))
    print(step, "B", B, "used (fwd, bwd, fold)", r["used"], "grad rel %.2e loss abs %.2e running-stat rel %.2e" % got)
    assert ref["ambiguous"] == 0 and r["dec"].count() > 0
    for v, bound, what in zip(got, (1e-4, 1e-5, 1e-5), ("grad", "loss", "running stats")):
        assert v <= bound, f"{what}: {v:.3e} > {bound:.0e} vs the decision-matched float64 step"


@pytest.mark.parametrize("step,bi", [p for p in _step_params() if p.values[0].model != "res15"])
def test_train_step_fuse_and_fold_bitwise(monkeypatch, step, bi):
    """At each DMA geometry: FUSE_TAIL off (the tails read h and old) and FOLD_BN off (every
    y materialized) give the bit-identical step -- loss, gradients, running statistics."""
    cfg = _cfg(step)
    B = _step_batches(step)[bi]
    base = _run_step(step, cfg, B)
    fwd, bwd, fold = _predict(step, cfg, B)
    assert base["used"] == (fwd, bwd, fold) and fwd > 0 and fold > 0
    for attr, want in (("FOLD_BN", (fwd, bwd, 0)), ("FUSE_TAIL", (fwd, bwd, 0))):
        monkeypatch.setattr(hc, attr, False)
        o = _run_step(step, cfg, B)
        monkeypatch.undo()
        assert o["used"] == want, (attr, o["used"])
        assert torch.equal(o["loss"], base["loss"]), attr
        for k in base["g"]:
            assert torch.equal(o["g"][k], base["g"][k]), (attr, k)
        for k in base["b"]:
            assert torch.equal(o["b"][k], base["b"][k]), (attr, k)
