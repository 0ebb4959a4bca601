"""Case table of tests/test_worklist_reference.py (CPU) and tests/test_gpu_work_list.py: batches made from a PER-GROUP HISTOGRAM.

The host's cut sees nothing of a batch but its group starts, so every case is a histogram -- events per source tile, or per (tile, time
bin) -- and `batch` draws pixels and times inside it.  All batches are handed to set_events with the extremes (0, 1), so an event's
normalised time is its own t, exactly; binned cases draw t strictly inside the bin.  `active` limits the distinct pixels of a tile (long
runs: >= 8 events per active pixel give big segments their compact copy).

A case: id, size, T (time bins at set_events), hist (callable -> int array [ntiles] or [ntiles, T]), active, steps -- ("bins", k) |
("slabs", k) | ("events", case id: that case's batch on the same handle) --, expect: what `cut_with_reasons` must say of step 0 (the
regime the id names), evals: list of "2dof" | "dense" | "voxel" (binned cases: a motion per time bin), extreme: put the extreme times of the compact cases into the batch."""
import numpy as np

_batches = {}


def tiles(size):
    return (size[0] + 15) // 16, (size[1] + 15) // 16


def batch_from_histogram(size, hist, T=0, active=256, seed=0, extreme=False):
    """[n, 4] float64 events (row, col, t, p), shuffled, with exactly hist[tile] (or hist[tile, bin]) events per group."""
    rng = np.random.default_rng(seed)
    ntr, ntc = tiles(size)
    hist = np.asarray(hist, np.int64).reshape(ntr * ntc, max(T, 1))
    per_tile = hist.sum(axis=1)
    n = int(per_tile.sum())
    tile = np.repeat(np.arange(ntr * ntc), per_tile)
    r0, c0 = 16 * (tile // ntc), 16 * (tile % ntc)
    hgt, wid = np.minimum(16, size[0] - r0), np.minimum(16, size[1] - c0)
    k = rng.integers(0, active, n)                       # the k-th of the tile's first `active` pixels (row-major inside the tile)
    k = k % (hgt * wid)
    ev = np.empty((n, 4))
    ev[:, 0], ev[:, 1] = r0 + k // wid, c0 + k % wid
    if T == 0:
        ev[:, 2] = rng.uniform(0.0, 1.0, n)
        if n >= 2:                                       # the batch's own extremes are (0, 1) too: what a reference normalises by
            ev[:2, 2] = [0.0, 1.0]
        if extreme and n >= 8:                           # tau = 0 and 1, a negative residual byte, times below 2^-24 and below 2^-95
            ev[:8, 2] = [0.0, 1.0, np.float64(np.float32(0.3)) - 2.0 ** -30, 0.75 * 2.0 ** -24, 2.0 ** -26 * 1.5, 2.0 ** -100, 1.0 - 2.0 ** -26, 0.5 + 2.0 ** -26]
    else:
        bins = np.repeat(np.tile(np.arange(T), ntr * ntc), hist.reshape(-1))
        ev[:, 2] = (bins + rng.uniform(0.05, 0.95, n)) / T
        first, last = np.flatnonzero(bins == 0), np.flatnonzero(bins == T - 1)
        if first.size and last.size:                     # ... and t = 1 belongs to the last bin
            ev[first[0], 2], ev[last[-1], 2] = 0.0, 1.0
    ev[:, 3] = rng.integers(0, 2, n)
    return ev[rng.permutation(n)]


def _fill(size, T, value):
    ntr, ntc = tiles(size)
    return np.full((ntr * ntc, max(T, 1)), value, np.int64)


def _vary(size, T, lo, hi, seed, empty=0):
    """Counts uniform in [lo, hi], `empty` groups set to zero."""
    rng = np.random.default_rng(seed)
    h = rng.integers(lo, hi + 1, _fill(size, T, 0).shape)
    if empty:
        h.reshape(-1)[rng.choice(h.size, empty, replace=False)] = 0
    return h


def _rows_mix(size, rows_a, a_first, a_second, small_first=False):
    """Rows of 24 tiles: `a` tiles of 1100 events then 24 - a of 680 (small_first: the other way round); the first `rows_a` rows with
    a = a_first, the others a_second."""
    ntr, ntc = tiles(size)
    h = np.empty((ntr, ntc), np.int64)
    for r in range(ntr):
        a = a_first if r < rows_a else a_second
        h[r, :a], h[r, a:] = 1100, 680
    if small_first:
        h = h[:, ::-1]
    return h.reshape(-1, 1)


def _set(h, pairs):
    h = h.copy()
    for idx, v in pairs:
        h.reshape(-1)[idx] = v
    return h


def case(id, size, hist, T=0, active=256, steps=(), expect=None, evals=(), extreme=False, seed=None, batch_of=None):
    """batch_of: the id of the case whose batch this one takes (the same events under another environment)."""
    return {"batch_of": batch_of, "id": id, "size": size, "T": T, "hist": hist, "active": active, "steps": list(steps), "expect": expect or {}, "evals": list(evals),
            "extreme": extreme, "seed": seed if seed is not None else sum(map(ord, id))}


SMALL = dict(big=False, mid=False, owned=False, big_rule="small")

CASES = [
    # ---- below 522 240 events: merged groups under the cap n / 512 (at least 256), never owned -------------------------------------------
    case("small-empty-tiles-between-full", (64, 80), lambda: np.array([300, 0, 0, 250, 0, 0, 0, 0, 0, 0, 256, 0, 257, 0, 1, 0, 0, 0, 0, 255]),
         expect=dict(SMALL, seg_cap=256, split_groups=2), evals=["2dof"]),
    case("small-tile-row-change-inside-a-segment", (48, 64), lambda: np.array([90, 80, 70, 100, 100, 40, 0, 0, 0, 0, 0, 60]),
         expect=dict(SMALL, seg_cap=256, split_groups=0)),
    case("small-group-above-cap-odd-parts", (32, 48), lambda: np.array([10, 771, 5, 0, 1285, 3]),  # 4 parts of 193, 6 parts of 215
         expect=dict(SMALL, seg_cap=256, split_groups=2), evals=["2dof"]),
    case("small-cap-n-over-512", (64, 64), lambda: _vary((64, 64), 0, 9000, 14000, 3),           # cap = ceil(n / 512) above 256
         expect=dict(SMALL, split_groups=16)),
    case("small-binned-T4", (64, 80), lambda: _vary((64, 80), 4, 0, 400, 4, empty=9), T=4, expect=dict(SMALL, max_groups=12), evals=["voxel"]),
    case("small-binned-T10-30k-span-3T", (240, 320), lambda: np.random.default_rng(10).multinomial(30000, np.full(3000, 1 / 3000)).reshape(300, 10), T=10,
         expect=dict(SMALL, seg_cap=256, max_groups=30)),
    case("small-binned-T40-coarse-key", (48, 64), lambda: _vary((48, 64), 40, 0, 90, 40, empty=50), T=40, expect=dict(SMALL, max_groups=120)),
    case("small-rebinned-and-slabbed", (64, 80), lambda: _vary((64, 80), 0, 100, 1500, 5, empty=3),
         steps=[("bins", 4), ("slabs", 2), ("slabs", 4), ("bins", 0)], expect=dict(SMALL)),
    case("small-second-smaller-batch", (64, 80), lambda: _vary((64, 80), 0, 2000, 5000, 6),
         steps=[("events", "small-tile-row-change-inside-a-segment-64x80")], expect=dict(SMALL)),
    case("small-tile-row-change-inside-a-segment-64x80", (64, 80), lambda: np.array([0, 0, 0, 100, 100, 90, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 60]),
         expect=dict(SMALL, seg_cap=256)),
    case("small-n-1", (32, 48), lambda: np.array([0, 0, 0, 0, 1, 0]), expect=dict(SMALL)),
    case("small-n-2", (32, 48), lambda: np.array([0, 1, 0, 0, 0, 1]), expect=dict(SMALL)),
    case("small-n-255", (32, 48), lambda: np.array([100, 100, 55, 0, 0, 0]), expect=dict(SMALL)),
    case("small-empty-batch", (32, 48), lambda: np.zeros(6, np.int64), expect=dict(SMALL)),
    # ---- from 522 240 events on, small sensors ---------------------------------------------------------------------------------------------
    case("owned-standard-every-tile-at-most-2040", (272, 272), lambda: _set(_vary((272, 272), 0, 1830, 2040, 7, empty=4), [(0, 2040), (5, 0), (288, 0)]), active=64,
         expect=dict(big=False, mid=False, owned=True, big_rule="ratio"), evals=["2dof", "dense"]),
    case("one-tile-of-2041-not-owned-standard-equal-parts", (272, 272),
         lambda: _set(_vary((272, 272), 0, 1830, 2040, 7, empty=4), [(0, 2040), (5, 0), (288, 0), (100, 2041), (101, 2846)]),
         expect=dict(big=False, mid=False, owned=False, big_rule="unaligned", seg_cap=2040, free_cut=False, split_groups=2), evals=["2dof"]),
    case("ratio-4-std-equals-11-big-takes-big-owned", (336, 384), lambda: _rows_mix((336, 384), 21, 21, 21), active=64,
         expect=dict(big=True, mid=False, owned=True, big_rule="ratio", std_n=462, big_n=168, compact=True), evals=["2dof", "dense"], extreme=True),
    case("ratio-above-big-owned-3-and-6-tiles-wide", (368, 384), lambda: _rows_mix((368, 384), 23, 18, 18, small_first=True), active=64,
         expect=dict(big=True, mid=False, owned=True, big_rule="ratio", std_n=460, big_n=161, compact=True), extreme=True),
    case("ratio-4-std-below-11-big-stays-standard", (336, 384), lambda: _rows_mix((336, 384), 19, 21, 15), active=64,
         expect=dict(big=False, mid=False, owned=True, big_rule="ratio", std_n=454, big_n=166)),
    case("mid-one-round-rule-528x512", (528, 512), lambda: _vary((528, 512), 0, 1480, 1520, 8),
         expect=dict(big=False, mid=True, owned=True, big_rule="ratio", std_n=1056, mid_n=528), evals=["2dof", "dense"]),
    case("binned-T4-small-accumulators-at-481-per-group", (304, 240), lambda: _fill((304, 240), 4, 481), T=4,
         expect=dict(big=False, mid=False, owned=True, small_accumulators=True), evals=["voxel"]),
    case("binned-T4-479-per-group-just-below-small-accumulators", (304, 240), lambda: _fill((304, 240), 4, 479), T=4,
         expect=dict(big=False, mid=False, owned=True, small_accumulators=False), evals=["voxel"]),
    case("free-cut-above-2088960", (64, 64), lambda: _vary((64, 64), 0, 125001, 140001, 9),
         expect=dict(big=False, mid=False, owned=False, big_rule="unaligned", free_cut=True, split_groups=0), evals=["2dof"]),
]

# ---- forced layouts: one child process per environment (the switches are read once per process) ------------------------------------------
CHILD_IDS = ["big", "big-nocompact", "mid", "no-owned", "small-acc-0"]
CHILD_ENV = [{"CMAX_BIG_SEG": "1"}, {"CMAX_BIG_SEG": "1", "CMAX_COMPACT": "0"}, {"CMAX_MID_SEG": "1"}, {"CMAX_NO_OWNED": "1"}, {"CMAX_SMALL_ACC": "0"}]
SWITCHES = ("CMAX_BIG_SEG", "CMAX_MID_SEG", "CMAX_NO_OWNED", "CMAX_SMALL_ACC", "CMAX_COMPACT", "CMAX_FREE_CUT", "CMAX_SEG_CAP", "CMAX_DEBUG_COMPACT")

_BIG_FORCED = [
    # (below 522 240 events the small-batch cap holds for big segments too, and no list is owned: spans of at most 3 tiles)
    case("forced-big-32x48-long-runs", (32, 48), lambda: np.array([6001, 4999, 0, 7000, 3, 9000]), extreme=True,
         expect=dict(big=True, owned=False, big_rule="forced", seg_cap=256, compact=True), evals=["2dof"]),
    case("forced-big-48x160-long-runs-3-wide", (48, 160), lambda: _set(_vary((48, 160), 0, 40, 90, 11, empty=5), [(3, 9001), (17, 7777)]), active=4,
         expect=dict(big=True, owned=False, big_rule="forced", seg_cap=256, compact=True), extreme=True),
    case("forced-big-odd-starts-and-full-4088-segments", (32, 48), lambda: np.array([8176, 88001, 4088, 250001, 4087, 180003]), extreme=True,
         expect=dict(big=True, owned=False, big_rule="forced", seg_cap=4088, free_cut=False, compact=True), evals=["2dof"]),
    case("forced-big-48x160-short-runs-no-compact", (48, 160), lambda: _vary((48, 160), 0, 500, 900, 12),
         expect=dict(big=True, owned=False, big_rule="forced", compact=False)),
    case("forced-big-owned-standard-batch", (272, 272), lambda: BY_ID["owned-standard-every-tile-at-most-2040"]["hist"](), batch_of="owned-standard-every-tile-at-most-2040",
         expect=dict(big=True, owned=True, big_rule="forced", compact=True), evals=["2dof", "dense"]),
]
FORCED = [
    _BIG_FORCED,
    [dict(c, expect=dict(c["expect"], compact=False)) for c in _BIG_FORCED],
    [case("forced-mid-4-tiles-wide", (432, 432), lambda: _fill((432, 432), 0, 750), expect=dict(big=False, mid=True, owned=True, mid_n=189), evals=["2dof", "dense"]),
     case("forced-mid-binned-T4-small-accumulators-5-wide", (304, 240), lambda: _fill((304, 240), 4, 481), T=4, batch_of="binned-T4-small-accumulators-at-481-per-group",
          expect=dict(big=False, mid=True, owned=True, small_accumulators=True), evals=["voxel"])],
    [case("no-owned-standard-batch", (272, 272), lambda: BY_ID["owned-standard-every-tile-at-most-2040"]["hist"](), batch_of="owned-standard-every-tile-at-most-2040",
          expect=dict(big=False, mid=False, owned=False, seg_cap=2040, free_cut=False), evals=["2dof", "dense"]),
     case("no-owned-mid-rule-skipped", (528, 512), lambda: BY_ID["mid-one-round-rule-528x512"]["hist"](), batch_of="mid-one-round-rule-528x512",
          expect=dict(big=False, mid=False, owned=False, mid_n=None))],
    [case("binned-T4-481-per-group-small-accumulators-off-span-12", (304, 240), lambda: _fill((304, 240), 4, 481), T=4, batch_of="binned-T4-small-accumulators-at-481-per-group",
          expect=dict(big=False, mid=False, owned=True, small_accumulators=False), evals=["voxel"])],
]

BY_ID = {c["id"]: c for c in CASES}
for _k, _table in enumerate(FORCED):
    for _c in _table:
        BY_ID[f"{CHILD_IDS[_k]}/{_c['id']}"] = _c


def batch(c):
    if c["batch_of"]:
        return batch(BY_ID[c["batch_of"]])
    key = (c["id"], c["size"], c["T"], c["active"], c["extreme"])
    if key not in _batches:
        _batches[key] = batch_from_histogram(c["size"], c["hist"](), c["T"], c["active"], c["seed"], c["extreme"])
        _batches[key].setflags(write=False)
    return _batches[key]


def theta(c):
    return np.array([3.25, -2.5])


def motion(c, model):
    """The motion of one evaluation: theta (2dof), a dense flow, or that flow scaled per time bin (voxel)."""
    if model == "2dof":
        return theta(c)
    f = flow(c)
    return f if model == "dense" else np.stack([f * (1.0 + 0.125 * k) for k in range(c["T"])])


def flow(c):
    """A smooth dense flow of a few pixels (fp32-exact values)."""
    H, W = c["size"]
    y, x = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing="ij")
    f = np.stack([3.0 * np.sin(2.0 * y + x) + 1.0, 2.5 * np.cos(y - 3.0 * x) - 0.5])
    return f.astype(np.float32).astype(np.float64)
