"""The case table of tests/test_gpu_radix_sort.py, shared by the parent and its child program (tests/_radix_worker.py): both build
the SAME arrays from the seeds below.  Numpy only.

Times are uniform draws left in the order they were drawn (NOT sorted): only such an input tells a stable sort from one that orders a
pixel's events by time.  Inside every pixel the fp32 normalised times of the surviving events are distinct -- `batch` asserts it and
moves on to the next seed otherwise -- so that a packed event is identified by (pixel, word 1)."""
import numpy as np

import _sort_ref as R

SIZE_A, SIZE_B = (64, 96), (48, 64)   # 24 tiles: 13-bit key, P = 3 (6-bit digits) / 7 (2-bit); 12 tiles: 12-bit key, P = 2 / 6
N_EDGES = (1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 6145, 8193)
THETA = np.array([7.3, -4.1])
T_MAX = 0.05

CHILDREN = ({"CMAX_SORT": "radix"}, {"CMAX_SORT": "radix", "CMAX_RS_BITS": "2"})
CHILD_IDS = ("bits6", "bits2")
CHILD_DIGIT_BITS = (6, 2)


def _sz(size):
    return f"{size[0]}x{size[1]}"


def _case(cid, kind, size, n, **kw):
    c = {"id": cid, "kind": kind, "size": size, "n": n, "dtype": "f64", "T": 0, "pad": 0, "keep_outside": True, "extremes": None,
         "weights": None, "steps": [], "evals": {}, "seed": 1}
    c.update(kw)
    return c


def _ev(model, cost, sigma=0, T=0, weight_grad=False):
    return {"tag": f"{model}/{cost}/s{sigma}", "model": model, "cost": cost, "sigma": sigma, "T": T, "weight_grad": weight_grad}


TWO_DOF_VAR = _ev("2d-translation", "image_variance")
CHAIN_STEPS = [("bins", 4), ("bins", 40), ("bins", 0), ("slabs", 2), ("slabs", 4), ("bins", 0)]


def _table():
    t = []
    for size in (SIZE_A, SIZE_B):
        for n in N_EDGES:
            t.append(_case(f"n-edges/{_sz(size)}/{n}", "uniform", size, n, seed=100 + n))
    for size in (SIZE_A, SIZE_B):
        for dtype in ("f32", "f64"):
            t.append(_case(f"plain/{_sz(size)}/{dtype}", "uniform", size, 50_000, dtype=dtype, seed=2, evals={0: [TWO_DOF_VAR]}))
    t.append(_case("hot-pixel", "hot-pixel", SIZE_B, 20_000, seed=3))
    t.append(_case("one-pixel/16x16", "one-pixel", (16, 16), 5000, seed=4))
    t.append(_case("one-pixel/8x8", "uniform", (8, 8), 300, seed=5))
    t.append(_case("dropped/front", "dropped", SIZE_A, 30_000, keep_outside=False, seed=6, survivors="front"))
    t.append(_case("dropped/back", "dropped", SIZE_A, 30_000, keep_outside=False, seed=7, survivors="back"))
    # (not in the issue's list: +-inf times are dropped like NaN ones and, unlike them, would otherwise reach the batch's extremes)
    t.append(_case("dropped/inf-time", "dropped", SIZE_A, 30_000, keep_outside=False, seed=21, survivors="front", inf_times=True))
    t.append(_case("all-dropped", "all-dropped", SIZE_A, 3000, keep_outside=False, seed=8, evals={0: [_ev("dense-flow", "image_variance")]}))
    t.append(_case("kept-outside", "kept-outside", SIZE_A, 20_000, pad=10, seed=9, evals={0: [TWO_DOF_VAR]}))
    for dtype in ("f32", "f64"):
        t.append(_case(f"fractional/{dtype}", "fractional", SIZE_A, 30_000, dtype=dtype, seed=10,
                       evals={0: [_ev("dense-flow", "image_variance"), _ev("2d-translation", "gradient_magnitude", sigma=1)]}))
    t.append(_case("bins-fine/4", "uniform", SIZE_A, 40_000, T=4, seed=11, evals={0: [_ev("dense-flow-voxel", "image_variance", T=4)]}))
    t.append(_case("bins-fine/32", "uniform", SIZE_A, 40_000, T=32, seed=12))
    t.append(_case("bins-coarse/33", "edges", SIZE_A, 40_000, T=33, seed=13))
    t.append(_case("bins-coarse/40", "edges", SIZE_A, 40_000, T=40, seed=14))
    # T = 49 is not in the issue's list: at T = 33 and 40 trunc(tau * T) is already the bin for every tau (fl(fl(k / T) * T) == k for all
    # k), so the loop of sort_voxel_bin that walks UP never runs there; at T = 49 it has to for the events on edges 1, 2, 4, 8, 16, 27
    t.append(_case("bins-coarse/49", "edges", SIZE_A, 40_000, T=49, seed=20))
    t.append(_case("bins-coarse-given-extremes", "uniform", SIZE_A, 40_000, T=40, seed=15, t_range=(0.01, 0.04), extremes=(0.0, 0.0625)))
    t.append(_case("sparse-720p/0", "uniform", (720, 1280), 20_000, seed=16))
    t.append(_case("sparse-720p/4", "uniform", (720, 1280), 4000, T=4, seed=17))
    for size in (SIZE_A, SIZE_B):
        evals = {s: [TWO_DOF_VAR] for s in range(len(CHAIN_STEPS) + 1)}
        evals[1] = [TWO_DOF_VAR, _ev("dense-flow-voxel", "image_variance", T=4)]
        t.append(_case(f"rebin-chain/{_sz(size)}", "fractional", size, 40_000, weights="polarity", seed=18, steps=CHAIN_STEPS, evals=evals))
    t.append(_case("weight-grad", "uniform", SIZE_A, 30_000, weights="zeros", seed=19,
                   evals={0: [_ev("dense-flow", "gradient_magnitude", sigma=1, weight_grad=True)]}))
    return t


CASES = _table()
BY_ID = {c["id"]: c for c in CASES}


def _uniform(rng, c):
    H, W = c["size"]
    n = c["n"]
    lo, hi = c.get("t_range", (0.0, T_MAX))
    ev = np.empty((n, 4))
    ev[:, 0] = rng.integers(0, H, n)
    ev[:, 1] = rng.integers(0, W, n)
    ev[:, 2] = rng.uniform(lo, hi, n)   # in the order drawn: shuffled in time
    ev[:, 3] = rng.integers(0, 2, n)
    return ev


def _build(c, seed):
    rng = np.random.default_rng(seed)
    H, W = c["size"]
    n = c["n"]
    ev = _uniform(rng, c)
    kind = c["kind"]
    if kind == "fractional":
        ev[:, 0] = np.minimum(ev[:, 0] + rng.uniform(0, 0.999, n), H - 1e-3)
        ev[:, 1] = np.minimum(ev[:, 1] + rng.uniform(0, 0.999, n), W - 1e-3)
    elif kind == "one-pixel":
        ev[:, 0], ev[:, 1] = 3, 7
    elif kind == "hot-pixel":
        # 6000 events in one pixel, 3000 in its right neighbour; input positions 4196 .. 5219 (1024 in a row: the whole 512-lane step
        # 4608 .. 5119 of workgroup 2 among them) all lie in the first pixel: a step whose 512 lanes hold one digit, in every pass
        pos = rng.permutation(np.concatenate([np.arange(0, 4196), np.arange(5220, n)]))
        first = np.concatenate([np.arange(4196, 5220), pos[:6000 - 1024]])
        ev[first, 0], ev[first, 1] = 21, 37
        ev[pos[6000 - 1024:6000 - 1024 + 3000], 0], ev[pos[6000 - 1024:6000 - 1024 + 3000], 1] = 21, 38
    elif kind in ("dropped", "all-dropped"):
        off = np.ones(n, bool)
        if kind == "dropped":
            k = int(0.4 * n)
            off[:k] = False  # survivors at the front: the later passes see n = *total << n_in, whole trailing workgroups are empty
            if c["survivors"] == "back":
                off = off[::-1].copy()
        m = int(off.sum())
        side = rng.integers(0, 4, m)
        d = rng.integers(1, 30, m).astype(np.float64)
        x, y = ev[off, 0], ev[off, 1]
        x = np.where(side == 0, -d, np.where(side == 1, H - 1 + d, x))
        y = np.where(side == 2, -d, np.where(side == 3, W - 1 + d, y))
        ev[off, 0], ev[off, 1] = x, y
        if kind == "dropped":
            on = np.flatnonzero(~off)
            bad = rng.choice(on[1:-1], 7, replace=False)
            ev[bad[:3], 0] = np.nan
            ev[bad[3:5], 1] = np.nan
            ev[bad[5:], 2] = np.nan
            if c.get("inf_times"):
                more = np.setdiff1d(on[1:-1], bad)[[11, 1234]]
                ev[more, 2] = [np.inf, -np.inf]
            ev[on[0], 2], ev[on[-1], 2] = 0.0, T_MAX  # the batch's time extremes lie on survivors
    elif kind == "kept-outside":
        out = rng.choice(n, 300, replace=False)
        side = rng.integers(0, 4, 300)
        d = rng.uniform(0.01, 9.0, 300)
        x, y = ev[out, 0] + rng.uniform(0, 0.9, 300), ev[out, 1] + rng.uniform(0, 0.9, 300)
        ev[out, 0] = np.where(side == 0, -d, np.where(side == 1, H + d - 0.01, x))
        ev[out, 1] = np.where(side == 2, -d, np.where(side == 3, W + d - 0.01, y))
    elif kind == "edges":
        # t_min = 0 and t_max = 2^-4 make the normalisation exact; 200 events sit on the bin edges k / T and one fp64 ulp either side
        T, tmax = c["T"], 0.0625
        ev[:, 2] = rng.uniform(0.0, tmax, n)
        ev[0, 2], ev[n - 1, 2] = tmax, 0.0
        pix = rng.choice(H * W, 200, replace=False)  # (one edge event per pixel: its neighbours by one ulp share their fp32 time)
        at = rng.choice(np.arange(1, n - 1), 200, replace=False)
        k = (1 + (np.arange(200) // 3) % (T - 1)).astype(np.float64)  # every edge, each in all three variants
        e = (k / T) * tmax
        which = np.arange(200) % 3
        ev[at, 2] = np.where(which == 0, e, np.where(which == 1, np.nextafter(e, -1.0), np.nextafter(e, 1.0)))
        ev[at, 0], ev[at, 1] = pix // W, pix % W
    elif kind != "uniform":
        raise KeyError(kind)
    if c["dtype"] == "f32":
        ev = ev.astype(np.float32)
    return ev


def _distinct(c, ev):
    tmin, tmax = c["extremes"] if c["extremes"] else (None, None)
    ok, row, col, _ = R.classify(ev, c["size"], c["keep_outside"])
    t32 = R.normalised_time(ev, tmin, tmax)[1].view(np.uint32).astype(np.int64)
    k = ((row[ok] * 4096 + col[ok]) << 32) | t32[ok]
    return np.unique(k).size == k.size


_built = {}


def batch(c):
    """The events of a case ([n, 4], fp64 or fp32): built once per process."""
    if c["id"] not in _built:
        for attempt in range(64):
            ev = _build(c, c["seed"] + 1000 * attempt)
            if _distinct(c, ev):
                break
        else:
            raise AssertionError(f"{c['id']}: no seed gives distinct fp32 times inside every pixel")
        ev.setflags(write=False)
        _built[c["id"]] = ev
    return _built[c["id"]]


def weights(c):
    """`_weighted_ref.weight_set(c["weights"], ...)` (imported by the callers: this module stays numpy-only)."""
    from _weighted_ref import weight_set
    return None if c["weights"] is None else weight_set(c["weights"], np.asarray(batch(c), np.float64), seed=c["seed"] + 7)


def motion(c, e):
    """fp32-representable motion of an evaluation: theta [2], flow [2, H, W] or voxel [T, 2, H, W]."""
    if e["model"] == "2d-translation":
        return THETA
    H, W = c["size"]
    r, q = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing="ij")

    def flow(k):
        f = np.stack([6.0 * np.sin(2 * np.pi * r + 0.3 * k) * np.cos(2 * np.pi * q), -5.0 * np.cos(2 * np.pi * r) * np.sin(2 * np.pi * q + 0.2 * k) + 1.5])
        return f.astype(np.float32).astype(np.float64)

    return flow(0) if e["model"] == "dense-flow" else np.stack([flow(k + 1) for k in range(e["T"])])
