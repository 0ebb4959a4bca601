"""The case table of tests/test_gpu_counting_sort.py, shared by the parent and its child program (tests/_radix_worker.py run with this
module as its table): both build the SAME arrays from the seeds below.  Numpy only.

The rows are the smallest batches at which each branch of the two-level counting sort (csrc/cmax_sort_kernels.h) runs: the 4096-event
chunk edges of the bucket passes, dropped / kept events, the pixel-run layouts of k_run_time_sort around its 1024-event chunks, its
192-event limit and its 200-event halo, tied times, the three key forms of k_tile_sort, sensors above 4096 tiles, and re-sort chains.
Rows of the radix table (tests/_sort_cases.py) are taken as they are; the builders and the retry for distinct fp32 times inside every
pixel are that module's.  Times are in drawn order, not sorted."""
import numpy as np

import _sort_cases as S
import _sort_ref as R

SIZE_A, SIZE_B, SIZE_R, SIZE_TILE, SIZE_BIG = S.SIZE_A, S.SIZE_B, (50, 70), (16, 16), (1040, 1040)
N_EDGES = (1, 2, 4095, 4096, 4097, 8191, 8192, 8193, 12289)
N_MAX = 60_000
TWO_DOF_VAR = S.TWO_DOF_VAR

CHILDREN = ({}, {"CMAX_NO_RUN_SORT": "1"})
CHILD_IDS = ("default", "norun")
CHILD_RUN_SORTED = (True, False)
ENV_NAMES = ("CMAX_SORT", "CMAX_RS_BITS", "CMAX_NO_RUN_SORT")   # removed from the inherited environment, then CHILDREN[k] set

EDGE_CHAIN_STEPS = [("bins", 49), ("bins", 33), ("bins", 0), ("slabs", 4), ("bins", 0)]

_sz = S._sz


def _case(cid, kind, size, n, **kw):
    c = S._case(cid, kind, size, n, long=[], distinct=True)
    c.update(kw)
    return c


def fill(total, run=150):
    """Per-pixel counts that add up to `total`: runs of `run` events and the rest."""
    return [run] * (total // run) + ([total % run] if total % run else [])


# ---- run layouts: per-pixel event counts in KEY order (pixel k of the tile holds counts[k] events), so packed run k starts at
# sum(counts[:k]).  `long` declares the runs above 192 events, in packed order.
RUN_LAYOUTS = {
    # a 192-run at 1023 .. 1214 (1 event in chunk 0, 191 in chunk 1), one at 1857 .. 2048 (191 in chunk 1, 1 in chunk 2), runs of 1,
    # and a run of 2 at 3071 .. 3072
    "straddle": (fill(900) + [123, 192] + fill(642) + [192, 1, 1, 1, 7] + fill(1012) + [2], []),
    # 192 events that end at 1023, 192 that start at 1024; then 191, 192, 193 side by side, and runs of 1
    "limit": (fill(832) + [192, 192, 191, 192, 193, 1, 1, 1, 1, 1], [193]),
    # 2900 events at 100 .. 2999: chunk 1 (staged 824 .. 2247) sees neither end; then 150 events at 3000 .. 3149 across 3072
    "long": ([100, 2900, 150, 40], [2900]),
}
# one run is the whole batch; its pixel (8, 8) lies inside the tile (the variance leaves the image's border out)
ONE_RUN_PIXEL = 8 * 16 + 8
for _last in (1, 2, 192):
    for _n in (1024, 1025, 2047):   # n = 0, 1, 1023 (mod 1024)
        RUN_LAYOUTS[f"last/{_last}/{_n}"] = (fill(_n - _last) + [_last], [])
# (16, 32): the last pixel of tile 0 and the first pixel of tile 1 are neighbours in the packed order; the second run lies across 1024
TWO_TILE_RUNS = [(0, 256 - len(fill(900)) - 1 + k, c) for k, c in enumerate(fill(900) + [100])] + [(1, 0, 100), (1, 1, 30)]


def _table():
    t = []
    for size in (SIZE_A, SIZE_R):
        for n in N_EDGES:
            ev = {0: [TWO_DOF_VAR]} if n in (4097, 8193) else {}
            t.append(_case(f"chunk-edges/{_sz(size)}/{n}", "uniform", size, n, seed=300 + n, evals=ev))
        for n in (4097, 8193):
            t.append(_case(f"chunk-edges/{_sz(size)}/{n}/f32", "uniform", size, n, dtype="f32", seed=400 + n, evals={0: [TWO_DOF_VAR]}))
    for cid in ("dropped/front", "dropped/back", "dropped/inf-time", "all-dropped", "kept-outside", "fractional/f32", "fractional/f64"):
        t.append(dict(S.BY_ID[cid], long=[], distinct=True))   # (fractional/*: the dense flow on a fractional row)
    for name, (counts, long) in RUN_LAYOUTS.items():
        runs = [(0, k, c) for k, c in enumerate(counts)]
        t.append(_case(f"runs/{name}", "runs", SIZE_TILE, sum(counts), runs=runs, long=long, seed=500, evals={0: [TWO_DOF_VAR]}))
    for n in (150, 300):
        t.append(_case(f"runs/one-run/{n}", "runs", SIZE_TILE, n, runs=[(0, ONE_RUN_PIXEL, n)], long=[n] if n > R.RUN_SORT_MAX else [], seed=500,
                       evals={0: [TWO_DOF_VAR]}))
    t.append(_case("runs/two-tiles", "runs", (16, 32), sum(r[2] for r in TWO_TILE_RUNS), runs=TWO_TILE_RUNS, seed=501, evals={0: [TWO_DOF_VAR]}))
    t.append(_case("tied/one-time", "tied", SIZE_B, 5000, values=1, distinct=False, seed=502))
    t.append(_case("tied/64-times", "tied", SIZE_B, 20_000, values=64, distinct=False, seed=503))
    # T = 1 has no inner bin edge and the builder's formula needs T >= 2: its batch is the one built for the edges of T = 4
    t.append(_case("bins/1", "edges", SIZE_A, 40_000, T=1, edge_T=4, seed=510))
    t.append(_case("bins/4", "edges", SIZE_A, 40_000, T=4, seed=511, evals={0: [S._ev("dense-flow-voxel", "image_variance", T=4)]}))
    t.append(_case("bins/32", "edges", SIZE_A, 40_000, T=32, seed=512))
    t.append(_case("bins/33", "edges", SIZE_A, 40_000, T=33, seed=513))
    t.append(_case("bins/40", "edges", SIZE_A, 40_000, T=40, seed=514))
    t.append(_case("bins/49", "edges", SIZE_A, 40_000, T=49, seed=515))
    t.append(_case(f"bins/4/{_sz(SIZE_R)}", "edges", SIZE_R, 30_000, T=4, seed=516))
    t.append(_case("bins/255-sparse", "edges", SIZE_B, 3000, T=255, seed=517))
    t.append(dict(S.BY_ID["bins-coarse-given-extremes"], long=[], distinct=True))
    t.append(dict(S.BY_ID["bins-coarse-given-extremes"], id="unbinned-given-extremes", T=0, long=[], distinct=True))
    t.append(_case("many-tiles/0", "uniform", SIZE_BIG, 20_000, seed=520))
    t.append(_case("many-tiles/4", "uniform", SIZE_BIG, 4000, T=4, seed=521))
    t.append(_case("many-tiles/last-tile", "last-tile", SIZE_BIG, 60, seed=522))
    t.append(dict(S.BY_ID["sparse-720p/0"], long=[], distinct=True))
    t.append(dict(S.BY_ID["sparse-720p/4"], long=[], distinct=True))
    for size in (SIZE_A, SIZE_B):
        t.append(dict(S.BY_ID[f"rebin-chain/{_sz(size)}"], long=[], distinct=True))
    t.append(_case("rebin-chain/edges", "edges", SIZE_A, 40_000, edge_T=49, seed=530, steps=EDGE_CHAIN_STEPS,
                   evals={s: [TWO_DOF_VAR] for s in range(len(EDGE_CHAIN_STEPS) + 1)}))
    t.append(_case("weight-grad/uniform", "uniform", SIZE_A, 30_000, weights="uniform", seed=531,
                   evals={0: [S._ev("dense-flow", "gradient_magnitude", sigma=1, weight_grad=True)]}))
    return t


CASES = _table()
BY_ID = {c["id"]: c for c in CASES}


def _build_own(c, seed):
    rng = np.random.default_rng(seed)
    H, W = c["size"]
    n = c["n"]
    ev = S._uniform(rng, c)
    if c["kind"] == "runs":
        ntc = (W + 15) // 16
        tile = np.concatenate([np.full(cnt, tl) for tl, _, cnt in c["runs"]])
        pix = np.concatenate([np.full(cnt, px) for _, px, cnt in c["runs"]])
        at = rng.permutation(n)   # input positions shuffled: the scatter does not hand the runs over in order
        ev[at, 0] = (tile // ntc) * 16 + (pix >> 4)
        ev[at, 1] = (tile % ntc) * 16 + (pix & 15)
    elif c["kind"] == "tied":
        v = np.sort(rng.uniform(0.0, S.T_MAX, c["values"]))
        ev[:, 2] = v[rng.integers(0, c["values"], n)]
    elif c["kind"] == "last-tile":
        ev[:, 0] = rng.integers(H - 16, H, n)
        ev[:, 1] = rng.integers(W - 16, W, n)
    else:
        raise KeyError(c["kind"])
    return ev


_built = {}


def batch(c):
    """The events of a case ([n, 4], fp64 or fp32), built once per process.  Kinds of the radix table go through ITS `batch` (builders,
    retry for distinct fp32 times inside every pixel); the kinds of this module's own retry the same way unless the case is about ties."""
    if c["id"] in _built:
        return _built[c["id"]]
    if c["kind"] in ("runs", "tied", "last-tile"):
        for attempt in range(64):
            ev = _build_own(c, c["seed"] + 1000 * attempt)
            if not c["distinct"] or S._distinct(c, ev):
                break
        else:
            raise AssertionError(f"{c['id']}: no seed gives distinct fp32 times inside every pixel")
        ev.setflags(write=False)
    else:
        ev = S.batch(dict(c, T=c["edge_T"]) if "edge_T" in c else c)
    _built[c["id"]] = ev
    return ev


def weights(c):
    from _weighted_ref import weight_set
    return None if c["weights"] is None else weight_set(c["weights"], np.asarray(batch(c), np.float64), seed=c["seed"] + 7)


motion = S.motion


def step_bins(c):
    """[(T, slabs)] of step 0 and every later step of a case."""
    out = [(c["T"], False)]
    for what, k in c["steps"]:
        T = k if k > 1 or what == "bins" else 0
        out.append((T, what == "slabs" and T > 0))
    return out


# ---- what the run layouts must exhibit, read off the EXPECTED packed positions (tests/test_counting_reference.py) ---------------------
SITUATIONS = ("straddle-1-far", "straddle-191-far", "192-ends-at-edge-then-192", "191-192-193", "run-of-1", "chunk-inside-long-run-then-straddle",
              "one-run-150", "one-run-300", "two-tiles-adjacent") + tuple(f"last-{k}-mod-{m}" for k in (1, 2, 192) for m in (0, 1, 1023))


def situations(x, size):
    """The tags of SITUATIONS that the expected un-binned sequence x (R.counting_expected) shows."""
    start, length = x["run_start"], x["run_len"]
    n, CH, MAXR, HALO = int(x["idx"].size), R.RUN_SORT_CHUNK, R.RUN_SORT_MAX, R.RUN_SORT_HALO
    end = start + length
    tags = set()
    short = (length >= 2) & (length <= MAXR)
    edge = (end - 1) // CH * CH   # the chunk edge in front of a run's last event: the run lies across it where it starts before it
    across = short & (start < edge)
    for far in (1, 191):          # events of the run behind the edge
        if (across & (end - edge == far)).any():
            tags.add(f"straddle-{far}-far")
    for k in range(start.size - 1):
        if length[k] == MAXR and length[k + 1] == MAXR and end[k] % CH == 0:
            tags.add("192-ends-at-edge-then-192")
        if k + 2 < start.size and tuple(length[k:k + 3]) == (191, 192, 193):
            tags.add("191-192-193")
        # a chunk c whose staged positions c * 1024 - 200 .. (c + 1) * 1024 + 199 hold neither the head of run k nor the head behind it,
        # and run k + 1 short and across the chunk edge that follows
        blind = any(start[k] < c * CH - HALO and end[k] >= (c + 1) * CH + HALO for c in range(n // CH + 1))
        if blind and length[k] > CH + 2 * HALO and across[k + 1] and edge[k + 1] == -(-end[k] // CH) * CH:
            tags.add("chunk-inside-long-run-then-straddle")
    if (length == 1).any():
        tags.add("run-of-1")
    if start.size == 1 and n in (150, 300):
        tags.add(f"one-run-{n}")
    if start.size and int(length[-1]) in (1, 2, MAXR) and n % CH in (0, 1, 1023) and start.size > 1:
        tags.add(f"last-{int(length[-1])}-mod-{n % CH}")
    ntc = (size[1] + 15) // 16
    tile = (x["row"] >> 4) * ntc + (x["col"] >> 4)
    pix = ((x["row"] & 15) << 4) | (x["col"] & 15)
    nxt = np.flatnonzero(tile[1:] != tile[:-1])
    if any(pix[i] == 255 and pix[i + 1] == 0 and tile[i + 1] == tile[i] + 1 for i in nxt):
        tags.add("two-tiles-adjacent")
    return tags
