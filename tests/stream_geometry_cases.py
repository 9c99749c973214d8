"""The batched and the resident front ends off 16000 / 480 / 160 / 40: the shapes, strides, ragged batches
and tick schedules of tests/test_gpu_stream_geometry.py (compute_{mfccs,pcen}_segments, StreamBank on the
device) and tests/test_stream_geometry_plan.py (the host side of the same table).

A shape is every windows case of frontend_geometry_cases.WINDOWS the kernel takes, and win800.  Its interior
frames and frame count are derived HERE from the definitions in the header comment of csrc/mfcc_stream.hip
-- a frame is window-specific when its n_fft span crosses a window edge -- and not from a plan query:

    frames = 1 + window // hop
    flo    = ceil((n_fft / 2) / hop)                            the first frame that starts inside the window
    fhi    = (window - n_fft / 2) // hop, at most frames - 1    the last one that ends inside it
    nint   = fhi - flo + 1 (<= 0: none)

so head = flo and tail = frames - 1 - fhi edge frames per window, gs = max(head, tail) slots per edge group,
FT // gs groups per edge tile (FT = 32), q = stride / hop, the cache nint - q rows of n_dct (PCEN: n_mels)
floats where stride % hop == 0 and q <= nint, and the tail capacity window - 1 samples.  At the reference
shape these are 101, 2, 98, 97, gs 2, 16 groups, 40-float rows and 32 000-byte tails: a formula that only
agrees with those constants passes every other segments / bank test.
"""
import functools

import numpy as np

import frontend_geometry_cases as fg
from honk_amd.audio import AudioPreprocessor

FT = 32
FRONTS = ("MFCCs", "PCEN")
WHICH = {"MFCCs": "mfccs", "PCEN": "pcen"}

# what each shape adds to the windows table's own reason (fg.WinCase.why)
WHY = {
    "win8000": "51 frames: 47 interior, the cache and the tiles of a window half the reference one",
    "win16077": "an odd 16 076-sample tail capacity: tail_bytes rounds 32 152 up to 32 160",
    "512-160": "pad 256 is no multiple of hop: flo = ceil(1.6), fhi = floor(98.4)",
    "320-80": "hop 80: LDS slots every 88 floats, 101 frames of a window of 8000 samples",
    "640-320": "gs = 1: 32 edge groups per tile, one edge row per side in the PCEN workspace",
    "256-64": "20-float rows, 63 frames; 9 windows per recording in the windows table",
    "128-160": "n_fft < hop: flo = 1 with a pad of 64, no sample shared between frames",
    "dct13": "13-float MFCC rows: half_floats * 4 is no multiple of 16, the second cache half 4-byte aligned",
    "80bands": "PCEN scans 3 segments per band over 80-float E rows; 13-float MFCC rows at hop 64",
    "128bands": "PCEN scans 2 segments per band over the widest E rows",
    "win300": "no interior frame: tails only, no cache, every frame a window's own",
    "800-160": "gs = 3: 10 groups per edge tile, two slots idle; gspan rounds 1 184 up to 1 200",
    "1024-128": "gs = 4: 8 groups per edge tile; 65 frames; gspan rounds 1 504 up to 1 520",
    "win16240": "2 head and 1 tail edge frame: head != tail in the PCEN edge rows, gs = 2 with an idle tail slot",
    "win800": "6 frames, 2 interior: the cache is 1 row or none, a segment tile holds 2 frames",
}
# the shapes that also run q = 1, q = nint, q = nint + 1 and stride > window
MORE_STRIDES = ("win16240", "800-160", "1024-128", "256-64", "dct13", "640-320")


class Geo:
    """One shape with the strides it runs at: [(stride, why)]."""

    def __init__(self, id, window, n_fft, hop, n_mels, n_dct, strides, why):
        self.id, self.window, self.n_fft, self.hop, self.n_mels, self.n_dct = id, window, n_fft, hop, n_mels, n_dct
        self.why = why
        pad = n_fft // 2
        self.frames = 1 + window // hop
        self.flo = -(-pad // hop)
        self.fhi = min((window - pad) // hop, self.frames - 1)
        self.nint = self.fhi - self.flo + 1
        self.head, self.tail = self.flo, self.frames - 1 - self.fhi
        self.gs = max(self.head, self.tail)
        self.strides = strides(self) if callable(strides) else list(strides)
        assert len({s for s, _ in self.strides}) == len(self.strides)

    def __repr__(self):
        return self.id

    def cols(self, front):
        return self.n_mels if front == "PCEN" else self.n_dct

    def ap(self, **kw):
        assert self.hop % 16 == 0
        return AudioPreprocessor(n_fft=self.n_fft, hop_ms=self.hop // 16, n_mels=self.n_mels,
                                 n_dct_filters=self.n_dct, **kw)

    def shared(self, stride):
        return stride % self.hop == 0 and self.nint > 0

    def route(self, stride):
        if not self.shared(stride):
            return "unshared"
        return "overlap" if stride // self.hop <= self.nint else "gapped"

    def cache_rows(self, stride):
        return self.nint - stride // self.hop if self.route(stride) == "overlap" else 0

    def slot_bytes(self, stride, front):
        """(tail_capacity, cache_rows, slot_bytes): the tail as int16, rounded up to 16 bytes, then two cache
        halves, the whole rounded up to 16 bytes."""
        tail_bytes = -(-2 * (self.window - 1) // 16) * 16
        half_floats = self.cache_rows(stride) * self.cols(front)
        return self.window - 1, self.cache_rows(stride), -(-(tail_bytes + 2 * 4 * half_floats) // 16) * 16

    def shape(self, front):
        """The shape keywords of the segments_cases / stream_bank_cases helpers."""
        return dict(window=self.window, frames=self.frames, cols=self.cols(front))

    def model(self, stride):
        import stream_bank_cases as bc
        return bc.Model(stride, self.window, self.hop, self.flo, self.fhi, self.frames)


def _table_strides(case):
    return lambda g: [(case.strides[0], "the windows table's shared stride" if g.nint > 0 else
                       "a multiple of hop, unshared all the same: no interior frame"),
                      (case.strides[1], "the windows table's unshared stride: stride % hop = 7")] + (
        [(g.hop, "q = 1: the largest cache, nint - 1 rows; one new shared frame per window"),
         (g.nint * g.hop, "q = nint: the overlapping route with an empty cache, windows abut"),
         ((g.nint + 1) * g.hop, "q = nint + 1: gapped, per-window segment tiles"),
         ((g.frames + 2) * g.hop, "stride > window: gapped, the host's skip")] if g.id in MORE_STRIDES else [])


GEOS = [Geo(c.id, c.window, c.n_fft, c.hop, c.n_mels, c.n_dct, _table_strides(c), WHY[c.id])
        for c in fg.WINDOWS if c.kernel]
GEOS.append(Geo("win800", 800, 480, 160, 40, 40,
                [(160, "q = 1: a cache of 1 row"), (320, "q = 2 = nint: overlapping, no cache"),
                 (480, "q = 3: gapped, 2 segment frames per window"), (167, "unshared: 6 frames per window")],
                WHY["win800"]))
BY_ID = {g.id: g for g in GEOS}
assert len(BY_ID) == len(GEOS) == 15 and set(WHY) == set(BY_ID)
COMBOS = [(g.id, s) for g in GEOS for s, _ in g.strides]

# ---- seeds --------------------------------------------------------------------------------------------
# The recordings of a (shape, stride) come in four groups -- the ragged batch (with and without holes), the
# ones batch, the long batch, the bank's streams -- each from a base seed of its own: 1000 x the shape's
# place + 10 x the group's + 100 x RESEED.  RESEED exists for the oracle pin: frame 0 and the last frame of a
# window are even extensions of the signal, their spectra are real, and a narrow mel band of one can hold
# next to no energy, where log / PCEN's gain turn the float32 restatement's rounding into an e32 of 1e-5 and
# more -- past the point where 16 x e32 meets the rule's 1e-4 cap.  Such a group takes the first k for which
# every recording of it stays under E32_MAX for both front ends (found on the CPU with the oracle and
# oracle/frontend_f32_sim.py alone; the pin asserts it).  The rule is not touched.
#
# 128 bands is the exception no seed mends: between 20 and 4000 Hz at n_fft 480 most of its bands hold one
# or two bins, and under PCEN about one window in three has an e32 above E32_MAX (4.9e-6 for MFCC already
# in the windows table).  Of 300 seeds none brings the three groups of AT_CAP -- 42 and 29 windows each --
# under it; they take the seed with the smallest e32 (1.1e-5, 7.2e-6, 8.9e-6, all PCEN's) and are pinned at
# the rule's cap itself, 1e-4: a bound 9 to 14 x e32, tighter than 16 x e32.
E32_MAX = 6e-6          # 16 x e32 <= 0.96e-4
E32_AT_CAP = 1.2e-5     # the groups of AT_CAP: the bound is the cap
GROUPS = ("ragged", "ones", "long", "bank")
RESEED = {
    ("512-160", 4000, "bank"): 1,
    ("320-80", 2000, "long"): 1,
    ("320-80", 2000, "bank"): 1,
    ("128-160", 1927, "ragged"): 1,
    ("dct13", 7680, "bank"): 1,
    ("80bands", 960, "ragged"): 2,
    ("80bands", 960, "long"): 100,
    ("80bands", 960, "bank"): 6,
    ("80bands", 967, "ragged"): 2,
    ("80bands", 967, "long"): 20,
    ("80bands", 967, "bank"): 152,
    ("128bands", 1920, "ragged"): 7,
    ("128bands", 1920, "ones"): 37,
    ("128bands", 1920, "long"): 23,
    ("128bands", 1920, "bank"): 54,
    ("128bands", 1927, "ragged"): 15,
    ("128bands", 1927, "ones"): 37,
    ("128bands", 1927, "long"): 40,
    ("128bands", 1927, "bank"): 221,
    ("win800", 480, "long"): 1,
}
AT_CAP = {("128bands", 1920, "long"), ("128bands", 1920, "bank"), ("128bands", 1927, "long")}


def e32_max(geo, stride, recording):
    """The largest e32 a pinned recording (a key of pinned_recordings) may have."""
    group = "bank" if recording.startswith("bank") else recording.split("[")[0]
    return E32_AT_CAP if (geo.id, stride, group) in AT_CAP else E32_MAX


def group_seed(geo, stride, group):
    group = "ragged" if group == "holes" else group
    return 1000 * (1 + GEOS.index(geo)) + 10 * GROUPS.index(group) + 100 * RESEED.get((geo.id, stride, group), 0)


# ---- ragged batches (compute_*_segments) ------------------------------------------------------------
def batches(geo, stride):
    """name -> (recording lengths, stride, unowned samples before / between / after the recordings), the
    spec of segments_cases.batch."""
    W, s = geo.window, stride
    # 1 / 5 / 0 / 0 / 2 windows: 16 edge groups straddle an edge-tile boundary at 10 and at 8 groups per
    # tile, one tile holds three recordings, a one-sample-short and an empty recording in the middle
    ragged = [W, W + 4 * s + 1, W - 1, 0, W + s]
    return {
        "ragged": (ragged, s, 0),
        "holes": (ragged, s, min(100, W // 3)),     # offsets[0] > 0, samples that belong to no recording
        "ones": ([W] * 9, s, 0),                    # the pool's tick: 18 edge groups
        # 41 windows: on the q = 1 stride the first recording's shared frames span several segment tiles
        # from an off-tile start; on the per-window routes 41 x tps tiles before the second recording's
        "long": ([W + 40 * s, W], s, 0),
    }


def batch_seed(geo, stride, name):
    return group_seed(geo, stride, name)


# ---- the tick schedule (StreamBank) -----------------------------------------------------------------
def schedule(geo, stride):
    """(stride, ticks) as stream_bank_cases.CASES holds them, on a bank grown from 2 slots:
      a  chunks W, s, s - 1, 1, 3 s + 5, then the rest     (a chunk without a window, one sample that
                                                            completes one, three windows in a tick)
      b  uniform chunks of 3 W // 8 + 1
      c  opened at tick 2 with W + 2 s (three windows at once), then s per tick
      d  fed W + s // 2 in tick 0 and closed after tick 1  (a tail and a cache left behind)
      e  opens at tick 2, before c, and takes d's slot; chunks of W // 2 + 1
    every surviving stream ends at W + 6 s samples (7 windows); odd ticks feed in descending slot order."""
    W, s = geo.window, stride
    total = W + 6 * s
    a_chunks = [W, s, s - 1, 1, 3 * s + 5]
    a_chunks.append(total - sum(a_chunks))
    assert min(a_chunks) > 0
    plan = [("a", 0), ("b", 0), ("d", 0), ("e", 2), ("c", 2)]
    pos = {k: 0 for k, _ in plan}
    ticks, t = [], 0
    while any(pos[k] < total for k, _ in plan if k != "d"):
        feed = []
        for k, start in plan:
            if t < start or (k == "d" and t > 0) or pos[k] >= total:
                continue
            if k == "a":
                n = a_chunks[t]
            elif k == "b":
                n = 3 * W // 8 + 1
            elif k == "c":
                n = W + 2 * s if t == 2 else s
            elif k == "d":
                n = W + s // 2
            else:
                n = W // 2 + 1
            n = min(n, total - pos[k])
            feed.append((k, n))
            pos[k] += n
        ticks.append((feed, ["d"] if t == 1 else [], t % 2 == 1))
        t += 1
    return s, ticks


def coverage(geo, stride):
    """What the schedule must reach at this shape, from the definitions alone (no library call): played on
    the bookkeeping of a bank grown from 2 slots.  -> dict of the facts, each asserted."""
    s, ticks = schedule(geo, stride)
    models, slot, open_, n_slots = {}, {}, [False, False], 2
    seen = dict(many=False, none=False, one_sample=False, reused=False, grew=False)
    freed = set()
    for feed, close, _ in ticks:
        for k, n in feed:
            if k not in models:
                if all(open_):
                    open_ += [False] * len(open_)
                    seen["grew"] = True
                slot[k] = open_.index(False)
                open_[slot[k]] = True
                seen["reused"] |= slot[k] in freed
                models[k] = geo.model(s)
            w, _, _ = models[k].feed(n)
            seen["many"] |= w >= 2
            seen["none"] |= w == 0 and n > 0
            seen["one_sample"] |= w >= 1 and n == 1
        for k in close:
            open_[slot[k]] = False
            freed.add(slot[k])
    assert all(seen.values()), (geo.id, stride, seen)
    assert slot["e"] == slot["d"] and len(open_) > 2
    for k, m in models.items():
        assert m.N == (geo.window + s // 2 if k == "d" else geo.window + 6 * s), k
        assert m.E == (1 if k == "d" else 7), k
    return seen


def bank_seed(geo, stride):
    return group_seed(geo, stride, "bank")


def expected_stats(geo, stride):
    """The bank's cumulative counters from the generalised Model's arithmetic: samples_in counts what is
    uploaded, after the host dropped a gap's samples (stride > window)."""
    s, ticks = schedule(geo, stride)
    models = {}
    st = dict(ticks=0, samples_in=0, windows=0, frames_computed=0, frames_reused=0)
    for feed, _, _ in ticks:
        st["ticks"] += 1
        for k, n in feed:
            m = models.setdefault(k, geo.model(s))
            st["samples_in"] += n - min(m.state()[2], n)
            w, computed, reused = m.feed(n)
            st["windows"] += w
            st["frames_computed"] += computed
            st["frames_reused"] += reused
    return st


# ---- the float64 oracle of a recording's windows ----------------------------------------------------
def windows_of(geo, rec, stride):
    n = 0 if len(rec) < geo.window else 1 + (len(rec) - geo.window) // stride
    return [rec[w * stride:w * stride + geo.window] for w in range(n)]


def oracle(geo, front, win_i16):
    """The float64 oracle of one int16 window: oracle.mfcc_ref.mfcc / tests.pcen_ref.pcen of window / 32768."""
    import pcen_ref
    from oracle import mfcc_ref
    y = win_i16 / 32768.
    if front == "PCEN":
        return pcen_ref.pcen(y, fg.SR, geo.n_fft, geo.hop, geo.n_mels, fg.FMIN, fg.FMAX)
    return mfcc_ref.mfcc(y, fg.SR, geo.n_fft, geo.hop, geo.n_mels, geo.n_dct, fg.FMIN, fg.FMAX)


def sim_kw(geo, front):
    kw = dict(sr=fg.SR, n_fft=geo.n_fft, hop=geo.hop, n_mels=geo.n_mels, fmin=fg.FMIN, fmax=fg.FMAX)
    if front != "PCEN":
        kw["n_dct"] = geo.n_dct
    return kw


@functools.lru_cache(maxsize=None)
def pinned_recordings(geo_id, stride):
    """Every recording the segments and the bank tests of (shape, stride) take for a reference, by name; the
    holes batch's are the ragged batch's."""
    import segments_cases as sc
    import stream_bank_cases as bc
    geo = BY_ID[geo_id]
    recs = {}
    for name, spec in batches(geo, stride).items():
        if name == "holes":
            continue
        _, _, _, rows = sc.batch(name, seed=batch_seed(geo, stride, name), window=geo.window, spec=spec)
        recs.update({f"{name}[{i}]": r for i, (r, _) in enumerate(rows)})
    recs.update({f"bank {k}": r
                 for k, r in bc.recordings(None, schedule(geo, stride), bank_seed(geo, stride)).items()})
    for r in recs.values():
        r.setflags(write=False)
    return recs
