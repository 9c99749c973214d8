"""The case table of the geometry tests of the res TRAINING convs (test_train_geometry_plan.py
on the host, test_gpu_train_geometry.py on the device).

The block convs of a training step (honk_amd/csrc/train.hip) are planned per (C, H, W, d):
td_rows / tm_rows / tc_rows pick the forward / input-gradient kernel and its class-band
geometry, twd_rows / tw_rows / tc_rows the weight gradient's, and the compile-time instances
are taken at W == 20, d == 1 and 25 (conv) / 17 (wgrad) rows per band.  honk_conv3x3_plan
reports what the launches read; every case pins it as a signature

    "<conv> <wgrad>[ <flags>]"      conv / wgrad = <family>[<kind>]:<TH>x<nband>[F]

family d (LDS-DMA staged MFMA), m (register-staged MFMA), v (VALU); kind = the VALU conv's
pixels per thread (NP) or the DMA weight gradient's variant (q, h, d: HONK_WGRAD); F = the
compile-time instance; flags s = the statistics epilogue, f = the folded BatchNorm; "same" =
the dedicated kernels refuse the shape (honk_conv_same_f32 runs it).  ``sigs`` holds the
default environment's signature and the ones of ENVS that differ from it.  A case whose
signature changes is a finding, not a row to re-pin.

STEPS are the model-level inputs that put the block maps of a whole training step on the
table's cases (map = input, pooled by res_pool)."""
import contextlib
import os

from honk_amd import _native

N_CUS = 256   # the CU count the table's signatures are taken at
ENV_VARS = ("HONK_TRAIN_CONV", "HONK_WGRAD", "HONK_TD_FIXED")
ENVS = {"default": {}, "m": {"HONK_TRAIN_CONV": "m"}, "v": {"HONK_TRAIN_CONV": "v"}, "wd": {"HONK_WGRAD": "d"},
        "wh": {"HONK_WGRAD": "h"}, "nofix": {"HONK_TD_FIXED": "0"}}


class Case:
    def __init__(self, C, H, W, d, default, why, many=False, **other):
        self.C, self.H, self.W, self.d = C, H, W, d
        self.sigs = dict({k: default for k in ENVS}, **other)
        self.why = why
        self.many = many     # also run with more tiles than workgroups (many_tile_batches)
        self.id = f"{C}-{H}x{W}-d{d}"

    @property
    def shape(self):
        return self.C, self.H, self.W, self.d

    def family(self, env="default"):
        """(conv family, wgrad family) letters, or None for the same-conv path."""
        s = self.sigs[env]
        return None if s == "same" else (s.split()[0][0], s.split()[1][0])

    def flags(self, env="default"):
        p = self.sigs[env].split()
        return p[2] if len(p) > 2 else ""

    def nband(self, env="default"):
        """(conv, wgrad) bands per clip."""
        p = self.sigs[env].split()
        return tuple(int(q.rstrip("F").split("x")[1]) for q in p[:2])

    def __repr__(self):
        return self.id


def _dma(conv, wgrad, fixed=""):
    """The signatures of a 19-map case on the LDS-DMA kernels: conv / wgrad = "<TH>x<nband>"
    of the d kernels (the register-staged kernels get the same bands unless `m` is given
    with the case), fixed = which of them take the compile-time instance ("c", "w")."""
    cf, wf = ("F" if "c" in fixed else ""), ("F" if "w" in fixed else "")
    out = dict(default=f"d:{conv}{cf} dq:{wgrad}{wf} sf", wd=f"d:{conv}{cf} dd:{wgrad}{wf} sf",
               wh=f"d:{conv}{cf} dh:{wgrad}{wf} sf")
    if fixed:
        out["nofix"] = f"d:{conv} dq:{wgrad} sf"
    return out


def _c19(H, W, d, conv, wgrad, np, why, fixed="", m=None, vth=None, many=False):
    sig = _dma(conv, wgrad, fixed)
    return Case(19, H, W, d, sig.pop("default"), why, many=many, m=m or f"m:{conv} m:{wgrad}",
                v=f"v{np}:{vth or conv} v:{vth or conv}", **sig)


def _m19(H, W, d, band, why):
    return Case(19, H, W, d, f"m:{band} m:{band}", why, v=f"v1:{band} v:{band}")


CASES = [
    # ---- 19 maps on the LDS-DMA kernels (W % 4 == 0, d <= 4) ---------------------------------
    _c19(1, 4, 1, "1x1", "1x1", 1, "one row, 4 live lanes of a super tile", many=True),
    _c19(3, 4, 4, "1x3", "1x3", 1, "H < d: class 3 is empty (nb0 == 0)"),
    _c19(4, 8, 4, "1x4", "1x4", 1, "H == d: every class one row"),
    _c19(4, 4, 4, "1x4", "1x4", 1, "H == d at 4 pixels a row: the many-tile case of d = 4", many=True),
    Case(19, 5, 256, 1, "d:1x5 v:1x5 s", "the widest DMA row: TH == 1, nband == H, the conv's waves 4..7 idle; the "
         "weight gradient leaves the DMA kernels (no fold)", m="m:1x5 v:1x5", v="v1:1x5 v:1x5"),
    _c19(7, 12, 3, "3x3", "3x3", 1, "Wr = 20: not a multiple of 8; classes of 3, 2, 2 rows"),
    _c19(3, 220, 1, "1x3", "1x3", 1, "the widest row of the DMA weight gradient", m="m:1x3 v:1x3"),
    Case(19, 3, 224, 1, "d:1x3 v:1x3 s", "one 4-pixel step past it: the conv stays, the weight gradient goes to VALU",
         m="m:1x3 v:1x3", v="v1:1x3 v:1x3"),
    _c19(26, 20, 1, "26x1", "13x2", 3, "npx = 520: 9 super tiles, 520 % 64 != 0; one past the fixed conv instance",
         m="m:26x1 m:13x2"),
    _c19(25, 20, 1, "25x1", "13x2", 2, "the fixed conv instance's lower end: one full band", fixed="c",
         m="m:25x1 m:13x2"),
    _c19(49, 20, 1, "25x2", "17x3", 2, "the fixed conv instance with a 24-row last band; fixed wgrad, 15-row last band",
         fixed="cw", m="m:25x2 m:17x3", many=True),
    _c19(34, 20, 1, "17x2", "17x2", 3, "the fixed wgrad instance, two full bands", fixed="w", m="m:34x1 m:17x2",
         vth="34x1"),
    _c19(50, 20, 1, "25x2", "17x3", 2, "both fixed instances at res26-narrow's own map", fixed="cw", m="m:25x2 m:17x3"),
    _c19(35, 20, 1, "18x2", "18x2", 3, "the neighbour of 34 x 20: TH == 18, no fixed wgrad instance",
         m="m:35x1 m:18x2", vth="35x1"),
    # res15-narrow's dilations on one tiny map (STEPS): d = 1, 2, 4 here, 8 and 16 below
    _c19(7, 12, 1, "7x1", "7x1", 1, "res15-narrow on 7 x 12: d = 1"),
    _c19(7, 12, 2, "4x2", "4x2", 1, "res15-narrow on 7 x 12: d = 2, classes of 4 and 3 rows"),
    _c19(7, 12, 4, "2x4", "2x4", 1, "res15-narrow on 7 x 12: d = 4, classes of 2, 2, 2, 1 rows"),
    _c19(3, 4, 1, "3x1", "3x1", 1, "res15-narrow on 3 x 4: d = 1"),
    _c19(3, 4, 2, "2x2", "2x2", 1, "res15-narrow on 3 x 4: d = 2"),
    # ---- 19 maps off the DMA kernels ----------------------------------------------------------
    _m19(17, 5, 1, "17x1", "W % 4 != 0: the register-staged kernels' scalar row staging"),
    _m19(5, 8, 8, "1x5", "d = 8, H < d"),
    _m19(7, 8, 16, "1x7", "d = 16, H < d"),
    _m19(7, 12, 8, "1x7", "res15-narrow on 7 x 12: d = 8, H < d"),
    _m19(7, 12, 16, "1x7", "res15-narrow on 7 x 12: d = 16"),
    _m19(3, 4, 8, "1x3", "res15-narrow on 3 x 4: d = 8"),
    _m19(3, 4, 16, "1x3", "res15-narrow on 3 x 4: d = 16"),
    _m19(1, 1, 1, "1x1", "one pixel"),
    Case(19, 2, 159, 1, "m:2x1 m:1x2", "the widest row of the register-staged weight gradient", v="v2:2x1 v:2x1"),
    Case(19, 2, 161, 1, "m:2x1 v:2x1", "past it (and W % 4 != 0): conv3x3m_kernel with the VALU weight gradient",
         v="v2:2x1 v:2x1"),
    Case(19, 3, 260, 1, "v2:1x3 v:1x3", "W > 256: the m kernels decline, the VALU kernels take it"),
    Case(19, 2, 285, 1, "v2:1x2 v:1x2", "the widest accepted 19-map row at d = 1"),
    Case(19, 2, 286, 1, "same", "one past it: the same-conv path, no error"),
    # ---- 45 maps (VALU; the forward / input gradient default to the same-conv path in
    # conv3x3.py, HONK_TRAIN_CONV=v keeps conv3x3_kernel<45, NP>) -------------------------------
    Case(45, 25, 13, 1, "v1:13x2 v:13x2", "res8's map: NP = 1, 13- and 12-row bands"),
    Case(45, 14, 20, 1, "v2:14x1 v:14x1", "NP = 2: 280 pixels a tile"),
    Case(45, 5, 7, 1, "v1:5x1 v:5x1", "res15 on 5 x 7: d = 1"),
    Case(45, 5, 7, 2, "v1:3x2 v:3x2", "res15 on 5 x 7: d = 2"),
    Case(45, 5, 7, 4, "v1:2x4 v:2x4", "res15 on 5 x 7: d = 4"),
    Case(45, 5, 7, 8, "v1:1x5 v:1x5", "res15 on 5 x 7: d = 8, H < d"),
    Case(45, 5, 7, 16, "v1:1x5 v:1x5", "res15 on 5 x 7: d = 16, H < d, W < d"),
    Case(45, 2, 119, 1, "v1:1x2 v:1x2", "the widest accepted 45-map row at d = 1"),
    Case(45, 2, 120, 1, "same", "one past it: the same-conv path, no error"),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


class Step:
    """One native training step: `model` (with `override`) on B clips of H x W inputs; maps =
    the block convs' (Hm, Wm); `many`: also at a batch past one tile per workgroup."""

    def __init__(self, model, override, B, H, W, maps, many=False):
        self.model, self.override, self.B, self.H, self.W, self.maps, self.many = model, override, B, H, W, maps, many
        self.id = f"{model}-{H}x{W}"

    def __repr__(self):
        return self.id


L6 = dict(n_layers=6)
STEPS = [
    Step("res15-narrow", {}, 6, 7, 12, (7, 12)),              # d = 1, 2, 4 on the DMA kernels, 8 and 16 on m
    Step("res15-narrow", {}, 6, 3, 4, (3, 4), many=True),     # H < d from d = 4 on
    Step("res26-narrow", L6, 8, 98, 40, (49, 20), many=True),  # both fixed instances, short last bands
    Step("res26-narrow", L6, 8, 52, 40, (26, 20)),            # 9 super tiles a band
    Step("res8-narrow", {}, 6, 4, 12, (1, 4), many=True),     # one 4-pixel row
    Step("res15", {}, 4, 5, 7, (5, 7)),                       # 45 maps, 13 layers, H < d for d = 8, 16
]


def dilations(cfg):
    """The block convs' dilations, conv1 .. convN (model.py: 2 ** (i // 3) with use_dilation)."""
    return [int(2 ** (i // 3)) if cfg["use_dilation"] else 1 for i in range(cfg["n_layers"])]


def step_cases(step, cfg):
    """The table's case of every block conv of the step."""
    return [BY_ID[f"{cfg['n_feature_maps']}-{step.maps[0]}x{step.maps[1]}-d{d}"] for d in dilations(cfg)]


@contextlib.contextmanager
def environment(env, **more):
    """ENVS[env] (and `more`) set, every other dispatch variable cleared, restored on exit."""
    saved = {k: os.environ.pop(k, None) for k in ENV_VARS}
    os.environ.update(ENVS[env], **more)
    try:
        yield
    finally:
        for k in ENV_VARS:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in saved.items() if v is not None})


def signature(B, C, H, W, d, n_cus=N_CUS):
    """honk_conv3x3_plan as a signature string (module docstring) and its two grids."""
    p = _native.conv3x3_plan(B, C, H, W, d, n_cus)
    if p is None:
        return "same", None
    cv, wg = p["conv"], p["wgrad"]
    s = f"{cv['family']}{cv['np'] or ''}:{cv['th']}x{cv['nband']}{'F' if cv['fixed'] else ''} " \
        f"{wg['family']}{wg['variant'] or ''}:{wg['th']}x{wg['nband']}{'F' if wg['fixed'] else ''}"
    fl = ("s" if p["stats"] else "") + ("f" if p["fold"] else "")
    return s + (" " + fl if fl else ""), (cv["grid"], wg["grid"])


def many_tile_batches(nband, n_cus):
    """Batches whose B * nband lies in (n_cus, 2 n_cus] and past 2 n_cus: two and three tiles
    on a workgroup of a grid of n_cus (both LDS buffers reused)."""
    b2, b3 = n_cus // nband + 1, 2 * n_cus // nband + 1
    assert n_cus < b2 * nband <= 2 * n_cus < b3 * nband
    return b2, b3
