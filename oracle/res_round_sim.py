"""Rounding simulation of the packed res forward's reduced-precision modes.

The inference kernels' arithmetic in float64 except for the operand roundings, per layer
(the one copy: exp/f16_mix_sim.py and the geometry tests import it):
  * "x3":   input tensor stored as bf16 (hi, lo); weights (input BN folded, W * invstd)
            as bf16 (hi, lo); products hw*hx + hw*lx + lw*hx         (3 per MAC: bf16x3)
  * "f16":  input tensor stored as one fp16; weights as fp16 (hi, lo); products
            hw*x + lw*x                                              (2 per MAC: f16x2)
  * "bf16": input tensor stored as one bf16; weights as ONE bf16; one product hw*x
            (the bf16 mode)
  * "f16c": input stored as fp16 (hi, lo); the conv reads hi only (2 products, as
            f16) while the residual add uses hi + lo (the stream keeps ~22 bits)
  * "f16s": as f16c, but the stored value is x - mean_BN (the conv input after the
            BN shift, so zero padding needs no border bias)
  * "f16w1": input stored as one fp16; weights as ONE fp16 (RNE); one product hw*x
An "f16" tensor may carry a per-clip power-of-two scale s (clip_scale_kernel's: s_model
lowered by the binades the clip's conv0 bound exceeds the model's range): it is stored as
f16(t * s) / s, so a loud clip's small values meet fp16's subnormals as on the device.
The border-class bias (folded BN) is exact.  The conv0 output (layer 0) and every
layer output are stored in the format of the layer that reads them as input.
Accumulation, the spatial mean and the head are exact, so a simulated error is the share
of a mode's logit error that its number formats alone explain, at any input geometry.
"""
import numpy as np

from oracle import ref_numpy as orc


def bf16(x):
    x = np.asarray(x, np.float32)
    b = x.view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return r.view(np.float32).astype(np.float64)


def f16(x):
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def split(x, rnd):
    h = rnd(x)
    return h, rnd(np.asarray(x, np.float64) - h)


def conv(x, w, d):
    return orc.conv2d(x, w, padding=(d, d), dilation=(d, d))


def f16_scaled(x, scale):
    """One fp16 at the clips' scales: f16(x * s) / s, s [B] (None: s = 1)."""
    if scale is None:
        return f16(x)
    s = np.asarray(scale, np.float64).reshape(-1, 1, 1, 1)
    return f16(np.asarray(x, np.float64) * s) / s


def layer_conv(x, W, mean, var, d, scheme, scale=None):
    """conv(bn(x)) with zero padding of the post-BN tensor, x the stored pre-BN tensor
    (already rounded to its storage), in the scheme's products.  scale: "f16" only."""
    s = 1.0 / np.sqrt(var.astype(np.float64) + 1e-5)
    Ws = W.astype(np.float64) * s[None, :, None, None]
    valid = np.ones_like(x[:1, :1])
    bias = conv(valid * (mean.astype(np.float64) * s)[None, :, None, None] * np.ones_like(x[:1]), W.astype(np.float64), d)
    if scheme == "exact":
        return conv(x, Ws, d) - bias
    if scheme == "x3":
        hx, lx = split(x, bf16)
        hw, lw = split(Ws, bf16)
        return conv(hx + lx, hw, d) + conv(hx, lw, d) - bias
    if scheme in ("f16", "f16c"):
        hw, lw = split(Ws, f16)
        xc = f16_scaled(x, scale if scheme == "f16" else None)  # the conv reads one fp16 (f16c: the hi half)
        return conv(xc, hw + lw, d) - bias
    if scheme == "f16w1":
        return conv(f16(x), f16(Ws), d) - bias
    if scheme == "bf16":
        return conv(bf16(x), bf16(Ws), d) - bias
    if scheme == "f16s":
        hw, lw = split(Ws, f16)
        u = f16(x - mean.astype(np.float64)[None, :, None, None])
        return conv(u, hw + lw, d)
    raise ValueError(scheme)


def store(x, scheme, scale=None):
    """The stored tensor's value as the residual add sees it.  scale: the clips' scales
    ([B], "f16" only)."""
    if scheme == "exact":
        return x
    if scheme == "x3":
        h, l = split(x, bf16)
        return h + l
    if scheme == "f16":
        return f16_scaled(x, scale)
    if scheme == "f16w1":
        return f16(x)
    if scheme == "bf16":
        return bf16(x)
    if scheme in ("f16c", "f16s"):
        h, l = split(x, f16)
        return h + l
    raise ValueError(scheme)


def clip_scales(x, s_model, M, w0sum):
    """clip_scale_kernel (honk_amd/csrc/res.hip) restated: per clip (scale, binades below
    s_model).  bound = max|x| * w0sum; where it exceeds M the scale drops by the exponent
    ex of bound / M (bound / M < 2^ex), and is clamped to [2^-24, 2^14]."""
    mx = np.abs(np.asarray(x, np.float32)).reshape(len(x), -1).max(axis=1)
    bound = mx * np.float32(w0sum)
    r = (bound / np.float32(M)).astype(np.float32)
    ex = np.where(bound > np.float32(M), np.frexp(r)[1], 0).astype(np.int64)
    s = np.clip(np.ldexp(np.float64(s_model), -ex), 2.0 ** -24, 2.0 ** 14)
    return s, ex


def fwd(params, cfg, x, schemes, scale=None):
    """schemes[i] = format of the tensor layer i (1..L) reads (i.e. layer i-1's output).
    x: [B, H, W], any H and W the model takes.  scale: [B] the clips' scales of "f16" stores."""
    x = np.asarray(x, np.float64)[:, None]
    L = int(cfg["n_layers"])
    y = orc.relu(orc.conv2d(x, params["conv0.weight"], padding=(1, 1)))
    if "res_pool" in cfg:
        y = orc.avg_pool2d(y, tuple(cfg["res_pool"]))
    cur = y            # pre-BN tensor, exact value
    old = y
    for i in range(1, L + 1):
        sc = schemes[i]
        xin = store(cur, sc, scale)
        if i % 2 == 1:
            # cur is a residual-stream tensor (conv0 output or an even layer's sum):
            # the residual of layer i+1 reads the stored value
            old = xin
        d = orc.res_dilation(cfg, i)
        mean = params[f"bn{i - 1}.running_mean"] if i > 1 else np.zeros(xin.shape[1], np.float32)
        var = params[f"bn{i - 1}.running_var"] if i > 1 else np.full(xin.shape[1], 1.0 - 1e-5, np.float32)
        h = orc.relu(layer_conv(xin, params[f"conv{i}.weight"], mean, var, d, sc, scale))
        cur = h + old if i % 2 == 0 else h
    z = orc.batch_norm_eval(cur, params[f"bn{L}.running_mean"], params[f"bn{L}.running_var"])
    z = z.reshape(z.shape[0], z.shape[1], -1).mean(axis=2)
    return orc.linear(z, params["output.weight"], params["output.bias"])


def all_layers(cfg, scheme):
    """The schemes argument of fwd for one scheme on every layer."""
    return {i: scheme for i in range(1, int(cfg["n_layers"]) + 1)}
