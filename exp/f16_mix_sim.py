"""Numerics of mixed fp16 / bf16x3 res layers.

Simulates the inference kernels' arithmetic in float64 except for the operand
roundings, per layer (the simulation itself lives in oracle/res_round_sim.py, which the
geometry tests share):
  * "x3":  input tensor stored as bf16 (hi, lo); weights (input BN folded, W * scale)
           as bf16 (hi, lo); products hw*hx + hw*lx + lw*hx          (3 per MAC)
  * "f16": input tensor stored as one fp16; weights as fp16 (hi, lo); products
           hw*x + lw*x                                              (2 per MAC)
  * "f16c": input stored as fp16 (hi, lo); the conv reads hi only (2 products, as
           f16) while the residual add uses hi + lo (the stream keeps ~22 bits)
  * "f16s": as f16c, but the stored value is x - mean_BN (the conv input after the
           BN shift, so zero padding needs no border bias)
  * "f16w1": input stored as one fp16; weights as ONE fp16 (RNE); one product hw*x
The border-class bias (folded BN) is exact.  The conv0 output (layer 0) and every
layer output are stored in the format of the layer that reads them as input.
Reports the worst |logit - float64 reference| over the res golden fixtures and
calibrated random cases, per scheme.
"""
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_numpy as orc  # noqa: E402
from oracle.res_round_sim import fwd  # noqa: E402  (the one copy of the simulation)
from golden_util import fixture_names, load_fixture, ref_configs  # noqa: E402


def cases(n_random=3):
    out = []
    for name in fixture_names():
        if not name.startswith("res"):
            continue
        cfg, params, x, logits, meta = load_fixture(name)
        out.append((name, cfg, params, x))
    for seed in range(n_random):
        for name in ("res15", "res8", "res26"):
            cfg = dict(ref_configs()[name])
            rng = np.random.Generator(np.random.PCG64(1000 + seed))
            params = orc.make_params(cfg, 1000 + seed)
            params = orc.calibrate_bn(params, cfg, rng.standard_normal((2, 101, 40)).astype(np.float32), seed=seed)
            out.append((f"rand{seed}-{name}", cfg, params, rng.standard_normal((3, 101, 40)).astype(np.float32)))
    return out


def evaluate(all_cases, scheme_fn):
    worst, rows = 0.0, []
    for name, cfg, params, x in all_cases:
        L = int(cfg["n_layers"])
        ref = orc.forward(params, cfg, x)
        got = fwd(params, cfg, x, scheme_fn(L))
        e = float(np.abs(got - ref).max())
        rows.append((name, e))
        worst = max(worst, e)
    return worst, rows


if __name__ == "__main__":
    cs = cases(int(os.environ.get("NRAND", "2")))
    only = os.environ.get("ONLY")
    for sch in ("x3", "f16", "f16c", "f16s", "f16w1"):
        if only and sch not in only.split(","):
            continue
        w, rows = evaluate(cs, lambda L, s=sch: {i: s for i in range(1, L + 1)})
        print(f"all-{sch:5s} worst {w:.2e}   " + "  ".join(f"{n}:{e:.1e}" for n, e in rows))
