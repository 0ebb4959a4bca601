"""The case table of the solver-side parity tests (tests/test_patch_reference.py on the CPU, tests/test_gpu_patch_side.py on the GPU):
the smallest shapes that reach each branch of csrc/cmax_patch_kernels.h, k_patch_tail (csrc/cmax_solver.hip) and
csrc/cmax_search_kernels.h.  References are computed once per process and shared (built_*), and never modified."""
import numpy as np

import event_based_optical_flow_amd as E

import _hvp_ref
import _patch_ref
import _search_ref

PERIOD = 0.05
DROP_CAP = 0.005
TAIL_LDS = 4096        # kTailLds of csrc/cmax_solver.hip: 2 ph pw values staged in LDS at or below it
SEARCH_LDS = 65280     # 64 KB - 256: the patch image and its scratch copy, 2 h w floats (cmax_patch_search)
YAML_HYBRID = (("multi_focal_normalized_gradient_magnitude", 1.0),)
YAML_TV = 0.01


def f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


# ---- 1. patch grid geometries ------------------------------------------------------------------------------------------------------
def geometry(gid, patch_image_size, pad, sw, sizes):
    return dict(id=gid, patch_image_size=tuple(patch_image_size), pad=tuple(pad), sw=tuple(sw), sizes=[tuple(s) for s in sizes])


GEOMETRIES = [
    geometry("1x1-pad0", (1, 1), (0, 0), (20, 28), [(20, 28)]),                         # one cell, no padding: sw = sensor
    geometry("1x5", (1, 5), (1, 1), (9, 4), [(27, 28), (25, 27)]),                      # one-row grid
    geometry("5x1", (5, 1), (1, 1), (9, 4), [(63, 12), (61, 11)]),                      # one-column grid
    geometry("2x2-fixture", (2, 2), _patch_ref.patch_pad((32, 40), (32, 40), (2, 5)), (32, 40), [(68, 90)]),
    geometry("3x4-exact", (3, 4), (0, 0), (8, 10), [(24, 40)]),                         # pad 0, sensor == up-sampled grid
    geometry("3x4-odd", (3, 4), (3, 2), (3, 5), [(27, 40), (26, 39), (21, 33), (20, 32)]),  # odd sw, odd extent 27, odd and even H
    geometry("16x16", (16, 16), (1, 1), (4, 5), [(66, 90)]),                            # 260 x 346 / (16, 21) scaled down by four
    geometry("16x16-sw16x21", (16, 16), (1, 1), (16, 21), [(66, 90)]),                  # grid far beyond the sensor: cells without a pixel
    geometry("overlap", (7, 7), _patch_ref.patch_pad((16, 20), (8, 10), (2, 5)), (8, 10), [(68, 90)]),  # sw != patch_size -> pad (2, 2)
    geometry("shift", (8, 8), _patch_ref.patch_pad((8, 10), (8, 10), (9, 12)), (8, 10), [(68, 90)]),    # patch_shift >= sw -> pad (2, 2)
    geometry("45x45", (45, 45), (1, 1), (2, 2), [(92, 90)]),                            # 2 ph pw = 4050: the tail's LDS path
    geometry("46x45", (46, 45), (1, 1), (2, 2), [(92, 90)]),                            # 2 ph pw = 4140: its global-memory path
    geometry("64x64-sw1", (64, 64), (1, 1), (1, 1), [(64, 64)]),                        # one pixel per cell
]
GEOMETRY = {g["id"]: g for g in GEOMETRIES}
LEAF_CASES = [(g["id"], s) for g in GEOMETRIES for s in g["sizes"]]
assert GEOMETRY["overlap"]["pad"] == (2, 2) and GEOMETRY["shift"]["pad"] == (2, 2) and GEOMETRY["2x2-fixture"]["pad"] == (1, 1)


def leaf_inputs(gid, size):
    """-> (motion [2,ph,pw], random cotangent [2,H,W]) fp64, values exact in fp32 so both precisions see the same numbers."""
    g = GEOMETRY[gid]
    rng = np.random.default_rng(1000 + 17 * size[0] + size[1] + len(gid))
    return f32(rng.normal(0, 30.0, (2,) + g["patch_image_size"])), f32(rng.normal(size=(2,) + tuple(size)))


def band_pixels(gid, size):
    """Pixels for one-hot cotangents: the sensor's corners and, per axis, the output lines on either side of every place where the
    first tap changes its padded cell (the lines that bound a cell's band in k_patch_to_dense_adj), crossed with three columns."""
    g = GEOMETRY[gid]
    out = set()
    lines = []
    for k in (0, 1):
        n, sw, G = size[k], g["sw"][k], (g["patch_image_size"][k] + 2 * g["pad"][k]) * g["sw"][k]
        off = G // 2 - n // 2
        src = np.maximum((np.arange(n) + off + 0.5) / sw - 0.5, 0.0)
        cell = np.floor(src).astype(int)
        edge = np.nonzero(np.diff(cell))[0]
        pick = {0, n - 1} | set(edge.tolist()) | set((edge + 1).tolist())
        lines.append(sorted(pick))
    rows, cols = lines
    some_cols = sorted({cols[0], cols[len(cols) // 2], cols[-1]})
    some_rows = sorted({rows[0], rows[len(rows) // 2], rows[-1]})
    for i in rows:
        for j in some_cols:
            out.add((i, j))
    for j in cols:
        for i in some_rows:
            out.add((i, j))
    return sorted(out)


# ---- 2. batches and motions --------------------------------------------------------------------------------------------------------
def batch(size, n=3000, seed=7):
    """Uniform events plus moving point features, so the contrast is not flat; sorted by time."""
    H, W = size
    a = E.utils.generate_events(n - n // 3, H, W, 0.0, PERIOD, seed=seed)
    b = E.utils.generate_structured_events(n // 3, H, W, (4.0, -3.0), n_dots=max(4, H * W // 200), tmin=0.0, tmax=PERIOD, seed=seed + 1)
    ev = np.concatenate([a, b])
    ev[:, 0], ev[:, 1] = np.clip(ev[:, 0], 0, H - 1), np.clip(ev[:, 1], 0, W - 1)
    return np.ascontiguousarray(ev[np.argsort(ev[:, 2], kind="stable")])


def patch_motion(kind, pis, seed, px=4.0):
    """[2 ph pw] patch motion in pixel per second whose displacement over the batch is a few pixels.  Values are multiples of 2^-10: the
    total variation takes the SIGN of Sobel responses, and on a constant, a plateau or a symmetric smooth field some responses are zero
    in exact arithmetic.  With such values every sum of the nine weighted taps is exact in fp64 in any order, so a response is exactly
    zero or at least 2^-13 in every implementation -- device, torch's convolution and the C oracle -- instead of a rounding residue
    whose sign depends on the order of summation (torch gives -8.9e-16 where x = -48.00000000000001 is constant)."""
    ph, pw = pis
    rng = np.random.default_rng(seed)
    if kind == "random":
        m = rng.normal(0, px, (2, ph, pw))
    elif kind == "smooth":
        i, j = np.meshgrid(np.linspace(0, 1, ph), np.linspace(0, 1, pw), indexing="ij")
        m = px * np.stack([np.sin(2.0 * i + j) + 0.3, np.cos(i - 1.5 * j) - 0.2])
    elif kind == "zero":
        m = np.zeros((2, ph, pw))
    elif kind == "constant":
        m = np.stack([np.full((ph, pw), px), np.full((ph, pw), -0.6 * px)])
    elif kind == "plateau":  # random, with a flat block (exactly-zero Sobel responses inside it) when the grid has room for one
        m = rng.normal(0, px, (2, ph, pw))
        m[:, : max(1, (2 * ph) // 3), : max(1, (2 * pw) // 3)] = 0.75 * px
    else:
        raise KeyError(kind)
    return (np.round(m / PERIOD * 1024.0) / 1024.0).reshape(-1)


def spec_of(gid, size, *, terms=YAML_HYBRID, tv_weight=YAML_TV, sigma=1.0, time_aware=False, T=10, scheme="burgers", t0="middle",
            scale_later=False, t_scale=None):
    g = GEOMETRY[gid]
    return dict(size=tuple(size), patch_image_size=g["patch_image_size"], sw=g["sw"], pad=g["pad"], t_scale=t_scale, terms=tuple(terms),
                sigma=sigma, tv_weight=tv_weight, tv_omit=True, omit=True, time_aware=time_aware, T=T, scheme=scheme, t0=t0,
                scale_later=scale_later and time_aware)


def plan_case(cid, gid, size, motion, **kw):
    return dict(id=cid, gid=gid, size=tuple(size), motion=motion, kw=kw)


_TWO_TERMS = (("multi_focal_normalized_gradient_magnitude", 1.0), ("image_variance", 0.5))
_BURGERS = dict(time_aware=True, T=10, scheme="burgers", t0="middle")
PLAN_CASES = [
    plan_case("1x1-dense", "1x1-pad0", (20, 28), "random"),
    plan_case("1x5-dense", "1x5", (25, 27), "smooth"),
    plan_case("5x1-burgers-mid", "5x1", (63, 12), "random", **_BURGERS),
    plan_case("exact-single-term", "3x4-exact", (24, 40), "random", terms=(("image_variance", 1.0),), tv_weight=0.0),  # fp32 adjoint branch
    plan_case("odd-dense", "3x4-odd", (27, 40), "random"),
    plan_case("odd-zero", "3x4-odd", (26, 39), "zero"),
    plan_case("odd-upwind-first-T5", "3x4-odd", (21, 33), "smooth", time_aware=True, T=5, scheme="upwind", t0="first"),
    plan_case("odd-scale-later", "3x4-odd", (20, 32), "random", scale_later=True, **_BURGERS),
    plan_case("16x16-dense", "16x16", (66, 90), "smooth"),
    plan_case("overlap-two-terms", "overlap", (68, 90), "random", terms=_TWO_TERMS, tv_weight=0.0),
    plan_case("overlap-burgers-first-T5", "overlap", (68, 90), "plateau", time_aware=True, T=5, scheme="burgers", t0="first"),
    plan_case("overlap-scale-later-upwind", "overlap", (68, 90), "smooth", time_aware=True, T=10, scheme="upwind", t0="middle", scale_later=True),
    plan_case("shift-constant", "shift", (68, 90), "constant"),
    plan_case("45x45-dense", "45x45", (92, 90), "random"),
    plan_case("46x45-dense", "46x45", (92, 90), "random"),
    plan_case("46x45-upwind-mid", "46x45", (92, 90), "smooth", time_aware=True, T=10, scheme="upwind", t0="middle"),
    plan_case("64x64-dense", "64x64-sw1", (64, 64), "plateau"),
]
PLAN = {c["id"]: c for c in PLAN_CASES}

HVP_CASES = [
    plan_case(f"hvp-{g}-{name}", gid, size, "smooth" if name == "scale-later" else "random", **kw)
    for g, gid, size in (("odd", "3x4-odd", (27, 40)), ("overlap", "overlap", (68, 90)), ("46x45", "46x45", (92, 90)))
    for name, kw in (("dense", {}), ("burgers", _BURGERS), ("scale-later", dict(scale_later=True, **_BURGERS)))
]
HVP = {c["id"]: c for c in HVP_CASES}

_BUILT = {}


def _motion_and_spec(c):
    pis = GEOMETRY[c["gid"]]["patch_image_size"]
    seed = 300 + sum(ord(ch) for ch in c["id"])
    x = patch_motion(c["motion"], pis, seed)
    return x, spec_of(c["gid"], c["size"], t_scale=PERIOD, **c["kw"])


def built_plan(c):
    """-> dict(ev, x, spec, loss, grad, loss_smooth, grad_smooth): the reference with and without the TV term."""
    if c["id"] not in _BUILT:
        x, spec = _motion_and_spec(c)
        ev = batch(c["size"])
        spec["t_scale"] = float(ev[:, 2].max() - ev[:, 2].min())
        loss, grad, _ = _patch_ref.plan(x, ev, spec)
        loss_s, grad_s, _ = _patch_ref.plan(x, ev, spec, with_tv=False)
        _BUILT[c["id"]] = dict(ev=ev, x=x, spec=spec, loss=loss, grad=grad, loss_smooth=loss_s, grad_smooth=grad_s)
    return _BUILT[c["id"]]


def _model(spec):
    return "dense-flow-voxel" if spec["time_aware"] else "dense-flow"


def hvp_inputs(c):
    """-> (ev, x, spec, dropped): the batch without the events within the scaled _border.MARGIN of a cell border at the motion the device
    holds (tests/_hvp_ref.drop_ambiguous; the product is not defined there).  t_scale stays the whole batch's duration (it is a
    parameter of the objective), so the flow does not move while the filter settles."""
    x, spec = _motion_and_spec(c)
    ev = batch(c["size"])
    spec["t_scale"] = float(ev[:, 2].max() - ev[:, 2].min())
    m = _patch_ref.device_motion(x, spec)
    directions = sorted({d for cost, _ in spec["terms"] for d in _hvp_ref.cost_directions(cost)})
    margin = _hvp_ref.border_margin(ev, m, _model(spec), spec["size"], directions)
    kept, dropped = _hvp_ref.drop_ambiguous(ev, m, _model(spec), spec["size"], directions, margin)
    return kept, x, spec, dropped


def hvp_tangents(c, x):
    rng = np.random.default_rng(900 + len(c["id"]))
    one = np.zeros_like(x)
    one[(3 * x.size) // 5] = 1.0
    return {"random": f32(rng.normal(size=x.shape)), "one-hot": one, "zero": np.zeros_like(x)}


def built_hvp(c):
    key = "hvp/" + c["id"]
    if key not in _BUILT:
        ev, x, spec, dropped = hvp_inputs(c)
        out = dict(ev=ev, x=x, spec=spec, dropped=dropped, v=hvp_tangents(c, x), hv={})
        for name, v in out["v"].items():
            out["loss"], out["grad"], out["hv"][name] = _patch_ref.plan(x, ev, spec, v=v)
        _BUILT[key] = out
    return _BUILT[key]


# ---- 3. the tail's total variation ------------------------------------------------------------------------------------------------
TV_GRIDS = [(1, 1), (1, 5), (2, 2), (2, 7), (3, 2), (3, 3), (8, 8), (45, 45), (46, 45), (64, 64)]
TV_MOTIONS = ("random", "zero", "constant", "plateau")


def tv_geometry(pis):
    """A sensor and sliding window for a patch grid whose only purpose is the TV term: pad (1, 1), sw >= 2, sensor = ph sw x pw sw."""
    sw = tuple(max(2, -(-24 // n)) for n in pis)
    return dict(patch_image_size=tuple(pis), pad=(1, 1), sw=sw, size=(pis[0] * sw[0], pis[1] * sw[1]))


# ---- 4. per-patch search -----------------------------------------------------------------------------------------------------------
SEARCH_SENSOR = (80, 102)
SEARCH_IMAGES = [(1, 1), (1, 7), (7, 1), (2, 2), (8, 10), (16, 21), (64, 84), (80, 102)]  # 80 x 102: the largest the LDS check admits
SEARCH_SIGMAS = [0.0, 0.5, 1.0, 3.0]  # sigma 3: radius 12 > 8, 10 and the one- and two-pixel axes (the reflection wraps more than once)
SEARCH_T = (0.2, 0.26)
SEARCH_BOXES = np.array([
    [0, 16, 16, 48],       # tile aligned
    [3, 24, 5, 33],        # straddles the 16-pixel tiles
    [70, 95, 95, 120],     # partly off the sensor
    [-10, 5, -4, 12],      # partly off, on the negative side
    [90, 100, 0, 10],      # wholly off
    [0, 80, 0, 102],       # the whole sensor: larger than every patch image but the last
    [20, 21, 10, 11],      # one pixel: smaller than most patch images
    [30, 37, 40, 49],      # empty
    [40, 45, 60, 66],      # one event
    [60, 64, 90, 96],      # all events on one timestamp
])
SWEEP = 1e9        # px per unit time: with every event >= SWEEP_GAP from its box's middle time, every vote lands >= 1000 px away
SWEEP_GAP = 1e-6
SEARCH_CANDIDATES = np.array([[0.0, 0.0], [300.0, -300.0], [-300.0, 300.0], [SWEEP, SWEEP]])
SEARCH_HANDLES = [dict(id=f"{name}-{'frac' if frac else 'int'}", frac=frac, **kw)
                  for name, kw in (("unbinned", dict(T=0, slabs=0)), ("T10-fine", dict(T=10, slabs=0)), ("T40-coarse", dict(T=40, slabs=0)),
                                   ("slabs4", dict(T=0, slabs=4)))
                  for frac in (False, True)]


def _in_box(ev, box):
    return (ev[:, 0] >= box[0]) & (ev[:, 0] < box[1]) & (ev[:, 1] >= box[2]) & (ev[:, 1] < box[3])


def search_events(frac):
    key = ("search-ev", frac)
    if key not in _BUILT:
        H, W = SEARCH_SENSOR
        rng = np.random.default_rng(21)
        ev = batch(SEARCH_SENSOR, n=5000, seed=11)
        ev[:, 2] = np.sort(rng.uniform(*SEARCH_T, len(ev)))
        ev = ev[~_in_box(ev, SEARCH_BOXES[7]) & ~_in_box(ev, SEARCH_BOXES[8])]
        one = np.array([[42.0, 63.0, 0.5 * (SEARCH_T[0] + SEARCH_T[1]) + 1e-3, 1.0]])
        pixel = np.array([[20.0, 10.0, t, 1.0] for t in (0.205, 0.221, 0.252)])  # the one-pixel box is not empty
        ev = np.concatenate([ev, one, pixel])
        ev = ev[np.argsort(ev[:, 2], kind="stable")]
        ev[_in_box(ev, SEARCH_BOXES[9]), 2] = 0.2411  # (not the middle of any other box)
        ev = ev[np.argsort(ev[:, 2], kind="stable")]
        # the sweeping candidate needs every event away from its box's middle time; removing an event can move a span, so repeat
        for _ in range(16):
            bad = np.zeros(len(ev), dtype=bool)
            for box in SEARCH_BOXES:
                inside = _in_box(ev, box)
                t = ev[inside, 2]
                if len(t) and t.max() > t.min():
                    near = np.abs(ev[:, 2] - (t.min() + 0.5 * (t.max() - t.min()))) < SWEEP_GAP
                    bad |= inside & near
            if not bad.any():
                break
            ev = ev[~bad]
        else:
            raise AssertionError("search_events: the middle-time filter does not settle")
        if frac:
            ev = ev.copy()
            ev[:, 0] = np.minimum(ev[:, 0] + rng.uniform(0, 0.999, len(ev)), H - 1e-3)
            ev[:, 1] = np.minimum(ev[:, 1] + rng.uniform(0, 0.999, len(ev)), W - 1e-3)
        _BUILT[key] = np.ascontiguousarray(ev)
    return _BUILT[key]


def search_candidates():
    return np.tile(SEARCH_CANDIDATES[None], (len(SEARCH_BOXES), 1, 1))


def built_search(frac, image, sigma):
    """-> (loss, gm, count) of tests/_search_ref.py on the whole box table."""
    key = ("search", frac, tuple(image), float(sigma))
    if key not in _BUILT:
        _BUILT[key] = _search_ref.patch_search(search_events(frac), SEARCH_BOXES, image, search_candidates(), sigma)
    return _BUILT[key]


def capacity_events():
    """8191 events on one pixel: the stated capacity of the 2^18 fixed point (8191 * 2^18 < 2^31)."""
    ev = np.zeros((8191, 4))
    ev[:, 0], ev[:, 1] = 5.0, 9.0
    ev[:, 2] = np.linspace(0.0, PERIOD, len(ev))
    ev[:, 3] = 1.0
    return ev
