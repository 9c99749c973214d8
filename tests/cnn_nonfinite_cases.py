"""Non-finite and never-read input entries on the SpeechModel (cnn-*) eval forward: what
tests/golden/make_cnn_nonfinite_golden.py (the reference's side) and tests/test_cnn_nonfinite.py
share.  Imports nothing from the reference.

The cnn convolutions are VALID and strided and their pools floor, so some rows and columns of
the input are never read ("dead"): the entries only conv outputs the pool drops would read.  A
window is a rectangle and the kept outputs are a product set, so the dead set is whole rows plus
whole columns.  The reference's logits do not change, bit for bit, when those entries are NaN or
+-Inf; a kernel that stages the whole clip, multiplies a padded zero weight against them or
max-reduces past a pool window turns them into NaN logits.

One batch of B = 10 clips per model (``batch``), built from the model's own clips:

  0, 5     clean (the leak check)
  1        NaN at the live entry nearest the centre
  2        -NaN at (0, 0)
  3        +Inf at the live corner (largest live row, largest live column)
  4        -Inf at a live interior entry
  6, 7, 8  every dead entry NaN / +Inf / -Inf (no dead entries: clean copies)
  9        the dead NaN fill plus the live NaN of clip 1"""
import zlib

import numpy as np

from oracle import ref_numpy as orc

NAMES = ("cnn-one-fpool3", "cnn-one-fstride4", "cnn-one-fstride4-12", "cnn-one-fstride8", "cnn-one-stride1",
         "cnn-tpool2", "cnn-tpool3", "cnn-trad-pool2", "cnn-trad-pool2-12", "cnn-tstride2", "cnn-tstride4",
         "cnn-tstride8")
B = 10
NEG_NAN = np.copysign(np.float32(np.nan), np.float32(-1.0))
VALUES = (np.float32(np.nan), NEG_NAN, np.float32(np.inf), np.float32(-np.inf))  # a poke's code indexes this
NAN, NNAN, PINF, NINF = range(4)
CLEAN_CLIPS, LIVE_CLIPS, FILL_CLIPS = (0, 5), (1, 2, 3, 4, 9), (6, 7, 8)
FILLS = {6: NAN, 7: PINF, 8: NINF, 9: NAN}   # clip: the value its dead entries take
PATTERN = ["nan" if i in LIVE_CLIPS else "finite" for i in range(B)]

# cnn_geometry_cases.CASES: (dead rows, dead columns), as probe() finds them (re-derived by
# test_cnn_nonfinite.test_geometry_dead_table); a case that is not here has none
GEO_DEAD = {
    "trad-101x38": ([], [37]),
    "trad-100x40": ([99], [39]),
    "trad-72x40": ([71], [39]),
    "trad-72x40-c2k9x3": ([71], [39]),
    "trad-72x40-c2out33": ([71], [39]),
    "trad-72x40-c2out12": ([71], [39]),
    "trad-72x40-maps48": ([71], [39]),
    "trad-70x40": ([69], [39]),
    "trad-102x40": ([101], [39]),
    "trad-103x40": ([], [39]),
    "trad-61x40-c1k10x4": ([], [39]),
    "one-fstride4-37x43": ([], [40, 41, 42]),
    "tpool3-37x27": ([35, 36], [25, 26]),
    "tstride4-45x40": ([44], []),
    "trad-61x40-c2s2-pool2": ([55, 56, 57, 58, 59, 60], [39]),
    "k4096": ([29], []),
    "k4160": ([29], []),
    "k4221": ([29], []),
}


def geo_dead(case_id):
    return GEO_DEAD.get(case_id, ([], []))


def pattern(out):
    """Per clip "nan" (every logit NaN), "inf" (some logit not finite) or "finite"."""
    return [("nan" if np.isnan(r).all() else "inf" if not np.isfinite(r).all() else "finite") for r in out]


def clean(x):
    """The batch with every non-finite entry replaced by 0 (same composition)."""
    return np.where(np.isfinite(x), x, np.float32(0)).astype(np.float32)


def crc(x):
    return zlib.crc32(np.ascontiguousarray(x, dtype=np.float32).tobytes())


def probe_batches(clip, chunk=32):
    """The probe clips of one [H, W] clip, in chunks: clip r < H has row r NaN, clip H + c has
    column c NaN."""
    H, W = clip.shape
    for a in range(0, H + W, chunk):
        idx = range(a, min(a + chunk, H + W))
        xb = np.repeat(np.asarray(clip, np.float32)[None], len(idx), 0)
        for j, i in enumerate(idx):
            if i < H:
                xb[j, i, :] = np.nan
            else:
                xb[j, :, i - H] = np.nan
        yield xb


def dead_from_logits(out, H, W):
    """(dead rows, dead columns) from the [H + W, n_labels] logits of the probe clips: a row or
    column is dead if its clip's logits hold no NaN."""
    hit = np.isnan(np.asarray(out)).any(1)
    assert hit.shape == (H + W,)
    return [r for r in range(H) if not hit[r]], [c for c in range(W) if not hit[H + c]]


def probe(params, cfg, clip):
    """The dead rows and columns of the model by the numpy oracle.  Only NaN-ness is read, so the
    oracle accumulates in float32 and runs in chunks."""
    H, W = clip.shape
    with np.errstate(invalid="ignore", over="ignore"):
        out = np.concatenate([orc.forward(params, cfg, xb, acc=np.float32) for xb in probe_batches(clip)])
    return dead_from_logits(out, H, W)


def _nearest(live, target):
    return min(live, key=lambda i: (abs(i - target), i))


def pokes(H, W, dead_rows, dead_cols):
    """[(clip, row, column, value code)] of the single live pokes (module docstring)."""
    lr = [r for r in range(H) if r not in set(dead_rows)]
    lc = [c for c in range(W) if c not in set(dead_cols)]
    assert lr[0] == 0 and lc[0] == 0
    centre = (_nearest(lr, H // 2), _nearest(lc, W // 2))
    interior = (_nearest(lr, (3 * H) // 8), _nearest(lc, W // 8))
    return [(1, centre[0], centre[1], NAN), (2, 0, 0, NNAN), (3, lr[-1], lc[-1], PINF),
            (4, interior[0], interior[1], NINF), (9, centre[0], centre[1], NAN)]


def fill_dead(clip, dead_rows, dead_cols, value):
    clip[list(dead_rows), :] = value
    clip[:, list(dead_cols)] = value


def batch(x0, dead_rows, dead_cols, fills=True):
    """(x [B, H, W], poke list): the clips x0 tiled to B, the dead fills of clips 6-9 (left out
    with fills=False: what clips 6-8 must stay bit-equal to), then the live pokes."""
    x0 = np.asarray(x0, np.float32)
    x = np.concatenate([x0] * -(-B // len(x0)))[:B].copy()
    if fills:
        for i, code in FILLS.items():
            fill_dead(x[i], dead_rows, dead_cols, VALUES[code])
    pk = pokes(x.shape[1], x.shape[2], dead_rows, dead_cols)
    for c, r, w, code in pk:
        x[c, r, w] = VALUES[code]
    return x, pk


# ---- persistent workgroups and chunks -------------------------------------------------------
BIG = 300
# clip: (what, value code) -- on a 256-CU persistent grid the workgroups of clips 256 .. 259 have
# just processed clips 0 .. 3
BIG_POKES = {0: ("live", NAN), 1: ("live", PINF), 2: ("dead", NAN), 3: ("dead", PINF),
             296: ("live", NAN), 297: ("live", PINF), 298: ("dead", NAN), 299: ("dead", PINF)}
BIG_PATTERN = {i: "nan" if what == "live" else "finite" for i, (what, _) in BIG_POKES.items()}


def big_batch(x, dead_rows, dead_cols):
    """x[:BIG] with BIG_POKES: a live poke sits at the centre entry of ``pokes``."""
    x = np.array(x[:BIG], np.float32)
    _, r, c, _ = pokes(x.shape[1], x.shape[2], dead_rows, dead_cols)[0]
    for i, (what, code) in BIG_POKES.items():
        if what == "live":
            x[i, r, c] = VALUES[code]
        else:
            fill_dead(x[i], dead_rows, dead_cols, VALUES[code])
    return x


CHUNK, CHUNK_B, CHUNK_CLIPS = 7, 17, (6, 7, 16)  # last of a chunk, first of the next, last of the batch


# ---- range ----------------------------------------------------------------------------------
def mfcc_like(rng, b, H=101, W=40):
    """MFCC-shaped clips, the distribution of the golden generator's "mfcc" inputs:
    c0 ~ N(-30, 20^2), c_k ~ N(0, (8 / (1 + k))^2)."""
    x = rng.standard_normal((b, H, W)).astype(np.float32)
    scale = np.array([20.0] + [8.0 / (1 + k) for k in range(1, W)], dtype=np.float32)
    x = x * scale
    x[:, :, 0] += -30.0
    return x.astype(np.float32)


RANGE_B = 4
# (fixture, scale).  The bar is ATOL * max(1, max |float64 logit|); the inputs are admissible while
# the float32-accumulating oracle stays within a quarter of it
# (test_cnn_nonfinite.test_range_inputs_admissible, which measured the figures on the right)
RANGE_CASES = [("cnn-trad-pool2", 1.0),        # max|logit| 0.302: float32 oracle 2.5e-07, bar 1e-4
               ("cnn-trad-pool2", 2000.0),     # max|logit| 571.3: float32 oracle 5.1e-04, bar 5.7e-2
               ("cnn-one-fstride4", 1.0),      # max|logit| 0.274: float32 oracle 1.1e-07, bar 1e-4
               ("cnn-one-fstride4", 2000.0)]   # max|logit| 483.8: float32 oracle 2.0e-04, bar 4.8e-2
RANGE_SEED = 4711


def range_batch(name, scale):
    rng = np.random.Generator(np.random.PCG64(RANGE_SEED + NAMES.index(name)))
    return (mfcc_like(rng, RANGE_B) * np.float32(scale)).astype(np.float32)
