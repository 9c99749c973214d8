"""The SpeechModel (cnn) training kernels off the workload's own shapes (cnn_train_cases.py; the
plans behind the rows are held by test_cnn_train_plan.py on the host): honk_conv2d_wgrad_f32 and
honk_conv2d_dgrad_f32 -- the backward of both cnn convs and, through head_train.py, of every
nn.Linear of a training step -- and honk_maxpool2d_bwd_f32.

a. every row through cnn_train.conv_relu / head_train.linear / linear_relu against float64 on the
   CPU under the kernel's own ReLU mask (test_conv_relu_grads_vs_float64's reference): dw, db, dx
   within 1e-5 (decision_replay.rel_err, a max-norm), no entry whose float64 value is exactly 0
   comes back non-zero, and two calls give the same bits (the fixed-order split sum);
b. input entries no tap reads (a stride past the kernel, floor remainders) may hold NaN: y, dw, db
   keep their bits;
c. the ReLU mask selects: +inf, -inf and NaN in gy at masked positions leave dw, db, dx bit-equal
   to the run with zeros there; through the C ABI with a hand-made act, -0.0 and +0.0 mask, a
   denormal and NaN pass gy;
d. max-pool backward bit-equal to torch on integer-valued inputs (ties everywhere): the second
   pass of its grid-stride loop (17 039 360 elements), a one-row window, a 4 x 3 pool with both
   remainders, the 1 x 1 identity;
e. the memory contract (poison_util's four fills, as test_gpu_memory_contract.py) on the 1024-split,
   misaligned-weights, two-pass-pad and batch-1 Linear rows;
f. one native train step at input geometries of cnn_geometry_cases.py, batches 1, 3 and 33, against
   the float64 step with the GPU's decisions (decision_replay.py): loss within 1e-5, every
   parameter gradient within 1e-4, no fallback, every ReLU site both masking and passing."""
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cnn_geometry_cases as cgeo
import cnn_train_cases as tc
import decision_replay as dr
import poison_util as pu
import test_gpu_memory_contract as mc    # (four_fills and its device-error rule)
from honk_amd import _native
from honk_amd import cnn_train as ct
from honk_amd import head_train as ht
from honk_amd import model as hm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _native.load()


def _layer(case):
    """The row's nn.Conv2d / nn.Linear on the device, with the row's weights."""
    _, w, b, _ = tc.inputs(case)
    B, Cin, H, W, N, KH, KW = case.shape
    if case.kind == "conv":
        m = torch.nn.Conv2d(Cin, N, (KH, KW), stride=case.stride)
        w_ = w
    else:
        m = torch.nn.Linear(Cin, N)
        w_ = w.view(N, Cin)
    with torch.no_grad():
        m.weight.copy_(w_)
        m.bias.copy_(b)
    return m.to(DEV)


def _forward(case, layer, xd):
    if case.kind == "conv":
        assert ct.conv_supported(xd, layer)
        return ct.conv_relu(xd, layer)
    x2 = xd.view(xd.shape[0], -1)
    assert ht.supported(x2)
    return (ht.linear_relu if case.kind == "linear_relu" else ht.linear)(x2, layer)


def _run(case, layer, x=None, gy=None):
    """One forward + backward of the row on the device: dict(y, dw, db[, dx]) of CPU tensors."""
    x0, _, _, gy0 = tc.inputs(case)
    xd = (x0 if x is None else x).to(DEV).requires_grad_(case.xgrad)
    gyd = (gy0 if gy is None else gy).to(DEV)
    with mc._device_errors_end_the_run(f"cnn training row {case}"):
        y = _forward(case, layer, xd)
        gr = torch.autograd.grad(y, [layer.weight, layer.bias] + ([xd] if case.xgrad else []), gyd.view(y.shape))
        torch.cuda.synchronize()
    out = dict(y=y.detach().cpu().view(gy0.shape), dw=gr[0].cpu().view(tc.inputs(case)[1].shape), db=gr[1].cpu())
    if case.xgrad:
        out["dx"] = gr[2].cpu()
    return out


def _mask_of(case, y):
    """The kernel's own ReLU mask (None for a Linear without one)."""
    return None if case.kind == "linear" else (y > 0)


def _check_vs_float64(case, r):
    pre, _ = tc.reference(case)
    np.testing.assert_allclose(r["y"].double().numpy(), (pre if case.kind == "linear" else pre.clamp_min(0)).numpy(),
                               atol=2e-5, rtol=1e-5)
    ref = tc.grads(case, _mask_of(case, r["y"]))
    for k in ("dw", "db") + (("dx",) if case.xgrad else ()):
        err = dr.rel_err(r[k].numpy(), ref[k].numpy())
        print(f"{case} {k}: rel_err {err:.2e}")
        assert err <= tc.BAR, (k, err)
        # rel_err is a max-norm: what float64 says is exactly 0 (a tap or pixel no term reaches, a
        # channel masked everywhere) must be 0, not merely small
        zero = ref[k] == 0
        assert not bool((r[k][zero] != 0).any()), (k, int(zero.sum()))


@pytest.mark.parametrize("case", tc.CASES, ids=repr)
def test_grads_vs_float64(case):
    """(a)"""
    assert tc.signature(case) == case.sig
    layer = _layer(case)
    r = _run(case, layer)
    _check_vs_float64(case, r)
    again = _run(case, layer)
    for k in r:
        assert pu.bits_equal(r[k], again[k]), f"{k}: two calls differ"


@pytest.mark.parametrize("name", tc.STRIDED)
def test_never_read_inputs_may_hold_nan(name):
    """(b)"""
    case = tc.BY_ID[name]
    nr = torch.from_numpy(tc.never_read(case))
    assert bool(nr.any())
    layer = _layer(case)
    x = tc.inputs(case)[0].clone()
    x[:, :, nr] = 0.0
    zeroed = _run(case, layer, x=x)
    x[:, :, nr] = float("nan")
    poisoned = _run(case, layer, x=x)
    for k in ("y", "dw", "db"):
        assert pu.bits_equal(zeroed[k], poisoned[k]), k
    assert bool(torch.isfinite(poisoned["dw"]).all())


@pytest.mark.parametrize("name", tc.MASK_ROWS)
def test_masked_positions_keep_nonfinite_gy_out(name):
    """(c) through the autograd functions: the mask selects, it does not multiply."""
    case = tc.BY_ID[name]
    _, ref_mask = tc.reference(case)
    assert 0.2 <= float((~ref_mask).float().mean()) <= 0.8
    layer = _layer(case)
    gy = tc.inputs(case)[3]
    y = _run(case, layer)["y"]
    masked = (y <= 0)
    assert 0.2 <= float(masked.float().mean()) <= 0.8
    bad = torch.tensor([float("inf"), float("-inf"), float("nan")]).repeat(int(masked.sum()) // 3 + 1)
    gy_bad, gy_zero = gy.clone(), gy.clone()
    gy_bad[masked] = bad[:int(masked.sum())]
    gy_zero[masked] = 0.0
    a, b = _run(case, layer, gy=gy_bad), _run(case, layer, gy=gy_zero)
    for k in ("dw", "db") + (("dx",) if case.xgrad else ()):
        assert pu.bits_equal(a[k], b[k]), k
        assert bool(torch.isfinite(a[k]).all()), k
    _check_vs_float64(case, b)     # (gy is masked there anyway: the reference is the row's own)


def test_mask_rule_through_the_abi():
    """(c) act <= 0 ? 0 : gy -- torch's threshold_backward: -0.0 and +0.0 mask; a denormal and NaN
    pass the gradient.  A hand-made act handed to the two gradients directly."""
    B, Cin, H, W, N, KH, KW = 2, 3, 6, 5, 4, 3, 2
    OH, OW = H - KH + 1, W - KW + 1
    g = torch.Generator().manual_seed(41)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(N, Cin, KH, KW, generator=g)
    gy = torch.randn(B, N, OH, OW, generator=g)
    vals = torch.tensor([-0.0, 0.0, 1e-45, float("nan"), 1.0, -1.0])     # 1e-45: the smallest denormal
    passes = torch.tensor([False, False, True, True, True, False])
    n = gy.numel()
    idx = torch.arange(n) % 6
    act, keep = vals[idx].view(gy.shape), passes[idx].view(gy.shape)
    assert float(act.view(-1)[2]) > 0 and bool(torch.signbit(act.view(-1)[0]))
    gp = torch.where(keep, gy.double(), torch.zeros((), dtype=torch.float64))
    ref = dict(dw=torch.nn.grad.conv2d_weight(x.double(), w.shape, gp), db=gp.sum((0, 2, 3)),
               dx=torch.nn.grad.conv2d_input(x.shape, w.double(), gp))
    lib = _native.load()
    xd, wd, gyd, actd = (t.to(DEV) for t in (x, w, gy, act))
    dw, db, dx = torch.empty_like(wd), torch.empty(N, device=DEV), torch.empty_like(xd)
    st = _native.stream_handle(xd.device)
    nb = int(lib.honk_conv2d_wgrad_workspace_bytes(B, Cin, H, W, N, KH, KW, 1, 1))
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    with mc._device_errors_end_the_run("the mask rule through the ABI"):
        _native.check(lib.honk_conv2d_wgrad_f32(xd.data_ptr(), gyd.data_ptr(), actd.data_ptr(), dw.data_ptr(),
                                                db.data_ptr(), B, Cin, H, W, N, KH, KW, 1, 1, ws.data_ptr(), nb, st),
                      "honk_conv2d_wgrad_f32")
        nb = int(lib.honk_conv2d_dgrad_workspace_bytes(B, Cin, H, W, N, KH, KW))
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        _native.check(lib.honk_conv2d_dgrad_f32(gyd.data_ptr(), actd.data_ptr(), wd.data_ptr(), dx.data_ptr(), B, Cin,
                                                H, W, N, KH, KW, ws.data_ptr(), nb, st), "honk_conv2d_dgrad_f32")
        torch.cuda.synchronize()
    for k, got in (("dw", dw), ("db", db), ("dx", dx)):
        assert dr.rel_err(got.cpu().numpy(), ref[k].numpy()) <= tc.BAR, k


# ---- (d) max-pool backward ---------------------------------------------------------------------
@pytest.mark.parametrize("shape,k", [((65, 64, 64, 64), (2, 2)), ((2, 3, 5, 7), (5, 2)), ((2, 3, 14, 11), (4, 3)),
                                     ((2, 3, 5, 7), (1, 1))], ids=["two-passes", "one-window-row", "4x3", "1x1"])
def test_maxpool_bwd_bitwise_vs_torch(shape, k):
    plan = _native.maxpool2d_bwd_plan(*shape, *k)
    assert plan["passes"] == (2 if shape[0] == 65 else 1)
    g = torch.Generator().manual_seed(sum(shape) + k[0])
    x = torch.randint(-3, 4, shape, generator=g).float()
    gy = torch.randn(shape[0], shape[1], shape[2] // k[0], shape[3] // k[1], generator=g)
    xr = x.clone().requires_grad_(True)
    ref = F.max_pool2d(xr, k)
    ref.backward(gy)
    xd = x.to(DEV).requires_grad_(True)
    assert ct.pool_supported(xd, torch.nn.MaxPool2d(k))
    with mc._device_errors_end_the_run(f"max-pool {shape} {k}"):
        out = ct._MaxPool.apply(xd, *k)         # (max_pool() returns a 1 x 1 pool's input as it is)
        out.backward(gy.to(DEV))
        torch.cuda.synchronize()
    assert torch.equal(out.detach().cpu(), ref.detach())
    assert torch.equal(xd.grad.cpu(), xr.grad)


# ---- (e) the memory contract ---------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.CONTRACT_ROWS)
def test_memory_contract(name):
    case = tc.BY_ID[name]
    layer = _layer(case)
    x, _, _, gy = tc.inputs(case)
    xd, gyd = x.to(DEV), gy.to(DEV)
    plain = _run(case, layer)

    def call():
        xx = xd.clone().requires_grad_(case.xgrad)
        y = _forward(case, layer, xx)
        gr = torch.autograd.grad(y, [layer.weight, layer.bias] + ([xx] if case.xgrad else []), gyd.view(y.shape))
        return dict(y=y.detach(), dw=gr[0], db=gr[1], dx=gr[2] if case.xgrad else None)

    r = mc.four_fills(f"cnn training row {case}", call, [xd, gyd, layer.weight, layer.bias])
    for k, v in r.items():
        assert pu.bits_equal(v.reshape(plain[k].shape), plain[k].numpy()), f"{k}: differs from the unpoisoned run"
    _check_vs_float64(case, plain)


# ---- (f) train steps off 101 x 40 ------------------------------------------------------------------
# (cnn_geometry_cases id, what the row brings)
STEP_ROWS = [
    ("trad-101x38", "conv2 on a 41 x 15 map (odd pooled height and width)"),
    ("tstride4-45x40", "a time-strided conv1 with a floor remainder, pool (1, 3)"),
    ("one-fstride4-37x43", "cnn-one-fstride4 at height 37: lin, dnn1 (linear_relu), dnn2"),
    ("tpool3-37x27", "a (3, 3) pool dropping two rows and two columns"),
    ("one-lin6510-37x42", "lin with flat = 6510: past 4096 and not a multiple of 4"),
    ("trad-72x40-c2out33", "conv2 with 33 out channels"),
]
STEPS = [(i, B) for i, _ in STEP_ROWS for B in (1, 3)] + [("tstride4-45x40", 33)]


def test_step_rows_are_what_they_claim():
    from oracle import ref_numpy as orc
    geos = {i: orc.cnn_geometry(cgeo.config(cgeo.BY_ID[i])) for i, _ in STEP_ROWS}
    assert geos["trad-101x38"]["pool1"][1] % 2 and geos["trad-101x38"]["pool1"][2] % 2
    c = cgeo.config(cgeo.BY_ID["tstride4-45x40"])
    assert c["conv1_stride"][0] > 1 and (45 - c["conv1_size"][0]) % c["conv1_stride"][0]
    c = cgeo.config(cgeo.BY_ID["tpool3-37x27"])
    assert geos["tpool3-37x27"]["conv1"][1] % c["conv1_pool"][0] and geos["tpool3-37x27"]["conv1"][2] % c["conv1_pool"][1]
    assert geos["one-lin6510-37x42"]["flat"] == 6510
    assert cgeo.config(cgeo.BY_ID["one-fstride4-37x43"]).get("dnn1_size") and cgeo.BY_ID["one-fstride4-37x43"].H != 101
    assert not any((cgeo.BY_ID[i].H, cgeo.BY_ID[i].W) == (101, 40) for i, _ in STEP_ROWS)


@pytest.mark.parametrize("cid,B", STEPS, ids=[f"{i}-b{B}" for i, B in STEPS])
def test_train_step_off_101x40(cid, B):
    case = cgeo.BY_ID[cid]
    cfg = dict(cgeo.config(case))
    cfg.update(dropout_prob=0.0, n_labels=12)
    torch.manual_seed(11)
    m = hm.find_model(case.model)(cfg)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    m = m.to(DEV).train()
    g = torch.Generator().manual_seed(12 + B)
    x = torch.randn(B, case.H, case.W, generator=g)
    y = torch.randint(0, 12, (B,), generator=g)
    dec = dr.Decisions()
    with mc._device_errors_end_the_run(f"train step {cid} B={B}"):
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)    # no fallback to PyTorch / MIOpen
            with dr.record(dec):
                loss = F.cross_entropy(m(x.to(DEV)), y.to(DEV))
            loss.backward()
        torch.cuda.synchronize()
    sites = 1 + int(hasattr(m, "conv2")) + int(hasattr(m, "dnn1") and not m.tf_variant)
    assert len(dec.relu) == sites
    for mask in dec.relu:
        assert bool(mask.any()) and not bool(mask.all())
    r = dr.replay_step(cfg, case.model, state, x.numpy(), y.numpy(), dec, dict(lr=0.01))
    assert abs(float(loss.item()) - r["loss"]) <= 1e-5
    for k, p in m.named_parameters():
        err = dr.rel_err(p.grad.cpu().numpy(), r["g"][k])
        print(f"{cid} B={B} {k}: {err:.2e}")
        assert err <= 1e-4, k
