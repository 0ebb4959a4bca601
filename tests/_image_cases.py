"""TEST INFRASTRUCTURE ONLY: the case table of the image-side kernels (csrc/cmax_fused.hip, csrc/cmax_image_kernels.h: vote image ->
loss and G = dL/dIWE), shared by tests/test_image_reference.py (CPU: the references against each other, the coverage condition),
tests/test_gpu_image_side.py and its child program tests/_image_worker.py (the kernels against the references).

What matters is the PADDED shape Hp x Wp, stated in every id.  The fused kernels work on 8 x 32 tiles (kGmTileH x kGmTileW) with
i0 = 1 under omit_boundary and 0 otherwise; the constants below restate them and `k1_sums_ok` of eval_plan (Hp, Wp >= 4): a change
there has to be repeated here.  A case is a dict of plain values; `built(case)` makes its batch and motion (flows rounded to fp32, a
2-DoF theta handed over as fp64), removes the events whose warped coordinate lies on a cell border (_hvp_ref.drop_ambiguous: across
it the gradient has a kink and an fp32 evaluation may take the other cell) and is computed once per process."""
import numpy as np

import _hvp_ref as R

TILE_H, TILE_W = 8, 32  # kGmTileH, kGmTileW
FUSED_MIN = 4           # k1_sums_ok: Hp >= 4 && Wp >= 4
PERIOD = 0.05
DROP_CAP = 0.005
MAX_EVENTS = 100_000
AMPLITUDE = 1.5         # px: the largest displacement along one axis

# label -> (cost, sigma); "normalized_image_variance@0" exists for the tangent-image path only (it has no blurred form)
# the normalised variance without a blur: rows of the tangent-image path only (it is none of the issue's eight objectives)
EXTRA_OBJECTIVES = {"normalized_image_variance@0": ("normalized_image_variance", 0)}
OBJECTIVES = {
    "image_variance@0": ("image_variance", 0),
    "image_variance@1": ("image_variance", 1),
    "gradient_magnitude@0": ("gradient_magnitude", 0),
    "gradient_magnitude@1": ("gradient_magnitude", 1),
    "normalized_image_variance@1": ("normalized_image_variance", 1),
    "normalized_gradient_magnitude@0": ("normalized_gradient_magnitude", 0),
    "multi_focal_normalized_gradient_magnitude@1": ("multi_focal_normalized_gradient_magnitude", 1),
    "multi_focal_normalized_image_variance@0": ("multi_focal_normalized_image_variance", 0),
}
LABELS = list(OBJECTIVES)
TAN2_NORMALISED = "normalized_image_variance@0"
_SHORT = {"image_variance": "iv", "gradient_magnitude": "gm", "normalized_image_variance": "niv", "normalized_gradient_magnitude": "ngm",
          "multi_focal_normalized_image_variance": "mfiv", "multi_focal_normalized_gradient_magnitude": "mfgm"}

# padded shape -> (sensor, pad) of its plain form.  Below and at the fused limit; one tile and one pixel over; both sides of the
# interior-tile predicate of k_stats_gimage_gm (tile row 8..15 is interior from H >= 17 + i0, tile column 32..63 from W >= 65 + i0);
# thin; one unaligned shape with more than two interior tiles each way whose pixel count (2727) is no multiple of 4.  17 x 65 sits on
# the predicate's edge under omit_boundary only; 16 x 65 and 17 x 64 do WITHOUT it (i0 = 0: tile row 8..15 ends on row H - 1, tile
# column 32..63 on column W - 1), so a predicate loosened by one is seen for both values of i0, on rows and on columns.
SHAPES = [(1, 9), (2, 7), (3, 5), (4, 4), (4, 37), (5, 5), (5, 33), (8, 32), (9, 33), (8, 64), (16, 33), (17, 65), (18, 66), (7, 130), (130, 5),
          (27, 101), (16, 65), (17, 64)]
NO_OMIT = {(1, 9), (2, 7)}  # omit_boundary needs Hp, Wp > 2
PADDED = {(17, 65): 1, (9, 33): 1, (5, 33): 1, (27, 101): 2}  # the same padded shape reached as a smaller sensor with outer_padding
LARGEST = [(27, 101), (18, 66)]
MEAN_SHAPES = [(4, 4), (5, 5), (5, 33), (17, 65), (27, 101)]
# eval_plan runs the statistics inside K3 (kFoldStatsInside) on a work list that is not group-aligned only where K1 can clear the flow
# gradient with 16-byte stores: 2 H W a multiple of 4.  Of MEAN_SHAPES that is 4 x 4 alone, so the border rows also run on these:
EVEN_SHAPES = [(4, 37), (8, 64), (18, 66), (7, 130)]
assert (27 * 101) % 4 != 0


_REGISTRY = {}  # id -> case: every row any path uses is made by case() and lands here


def objective_of(label):
    return OBJECTIVES[label] if label in OBJECTIVES else EXTRA_OBJECTIVES[label]


def label_id(label):
    cost, sigma = objective_of(label)
    return f"{_SHORT[cost]}{sigma}"


# Rows whose batch is drawn with another seed, and why.  3 x 5 with omit_boundary leaves Omega = 1 x 3 pixels; with seed 0 the 2-DoF border
# batch puts 29 / 34 / 30 votes on them: a variance of 0.4 % of the mean square.  The deferred 2-DoF variance takes sum I^2 from K3's
# gather in fp32 terms ("Image sums from the gather"), so the contrast is off by about mean^2 / variance x 2^-24 and
# the gradient of a normalised cost by twice that per reference time: _image_ref.fp32_statistics_error, 7.1e-5 for that batch, 1.7e-5 for
# seed 2; tests/test_image_reference.py holds every such row to STATISTICS_BUDGET.
RESEED = {((3, 5), "2d-translation", "border"): 2}


def case(shape, label, omit, model="dense-flow", events="cover", direction="minimize", pad=0, T=0):
    Hp, Wp = shape
    cost, sigma = objective_of(label)
    seed = RESEED.get((shape, model, events), 0) if pad == 0 else 0
    c = dict(shape=shape, size=(Hp - 2 * pad, Wp - 2 * pad), pad=pad, label=label, cost=cost, sigma=sigma, omit=bool(omit), model=model,
             events=events, direction=direction, T=T, seed=seed)
    assert c["size"][0] >= 1 and c["size"][1] >= 1 and (not omit or shape not in NO_OMIT)
    c["id"] = "-".join([f"{Hp}x{Wp}" + (f"p{pad}" if pad else ""), label_id(label), "omit" if omit else "full",
                        {"dense-flow": "dense", "2d-translation": "2dof", "dense-flow-voxel": f"voxel{T}"}[model], events] +
                       ([direction] if direction != "minimize" else []))
    return _REGISTRY.setdefault(c["id"], c)


def omits(shape):
    return (False,) if shape in NO_OMIT else (True, False)


def _grid():
    """every shape x every objective x both omit values: dense flow, `cover`, minimize -- the rows of the whole-call default path"""
    return [case(s, lab, o) for s in SHAPES for lab in LABELS for o in omits(s)]


def _axes():
    out = []
    for i, s in enumerate(SHAPES):
        om = omits(s)
        # 2-DoF throughout; sparse images (exact zeros) with `maximize`; the border set through both models
        out.append(case(s, LABELS[i % 8], om[i % len(om)], model="2d-translation"))
        out.append(case(s, LABELS[(i + 1) % 8], om[(i + 1) % len(om)], model="2d-translation", direction="maximize", events="sparse"))
        out.append(case(s, LABELS[(i + 3) % 8], om[(i + 1) % len(om)], events="sparse", direction="maximize"))
        out.append(case(s, LABELS[(i + 5) % 8], om[i % len(om)], model="2d-translation", events="border"))
        out.append(case(s, LABELS[(i + 6) % 8], om[(i + 1) % len(om)], events="border"))
    for s in MEAN_SHAPES + EVEN_SHAPES:  # the mean from K1's vote sums: fused blurred variance and the statistics inside K3, events along the border
        for o in (True, False):
            for lab in ("image_variance@1", "image_variance@0"):
                out.append(case(s, lab, o, events="border"))
    for s, pad in PADDED.items():
        # (a multi-focal cost also warps to the LAST event, where the ring that leaves the sensor at the first moves into it: no dense
        # flow covers a padding at both reference times, so on padded shapes those two costs run on the sparse set)
        for j, lab in enumerate(LABELS):
            out.append(case(s, lab, (j + pad) % 2 == 0, pad=pad, events="sparse" if lab.startswith("multi_focal") else "cover"))
        out.append(case(s, "image_variance@1", True, pad=pad, events="border"))
        out.append(case(s, "image_variance@0", False, pad=pad, events="border"))
        out.append(case(s, "gradient_magnitude@0", True, pad=pad, events="border", model="2d-translation"))
        # ... and on the 2-DoF border set, whose off-sensor sources sit in the padding itself and cover it at every reference time
        out.append(case(s, "multi_focal_normalized_gradient_magnitude@1", pad % 2 == 0, pad=pad, events="border", model="2d-translation"))
        out.append(case(s, "multi_focal_normalized_image_variance@0", pad % 2 == 1, pad=pad, events="border", model="2d-translation"))
    for s in LARGEST:  # voxel: T = 3 on two shapes
        out += [case(s, "image_variance@0", True, model="dense-flow-voxel", T=3), case(s, "gradient_magnitude@1", False, model="dense-flow-voxel", T=3),
                case(s, "multi_focal_normalized_image_variance@0", True, model="dense-flow-voxel", T=3)]
    return out


def _tan2():
    """the tangent-image path: 2-DoF plain variance (and the normalised variance on a second evaluation) on the border set"""
    out = []
    for i, s in enumerate(SHAPES):
        om = omits(s)
        for lab in ("image_variance@0", TAN2_NORMALISED):
            out.append(case(s, lab, om[i % len(om)], model="2d-translation", events="border"))
    out += [case((17, 65), "image_variance@0", True, model="2d-translation", events="border", pad=1),
            case((27, 101), "image_variance@0", False, model="2d-translation", events="border", pad=2)]
    return out


def _unique(cases):
    return list({c["id"]: c for c in cases}.values())


GRID = _grid()
AXES = [c for c in _unique(_axes()) if c["id"] not in {g["id"] for g in GRID}]
TAN2 = _unique(_tan2())


def rotation(shift, model="dense-flow"):
    """16 rows of the table, one per shape, that between them hold every objective twice and both omit values: a path that is run on
    `rotation(k)` meets every shape and every objective.  Dense rows come from GRID (their references are shared)."""
    out = []
    for i, s in enumerate(SHAPES):
        om = omits(s)
        out.append(case(s, LABELS[(i + shift) % 8], om[(i + shift) % len(om)], model=model))
    return out


def select(labels, shapes=SHAPES, omit=None):
    """the GRID rows of the given objectives (and shapes)"""
    return [c for c in GRID if c["label"] in labels and c["shape"] in shapes and (omit is None or c["omit"] == omit)]


# ---- what each path of tests/test_gpu_image_side.py runs, and the kernels the rows are meant to reach ---------------------------
PATHS = {
    # k_blur_stats_adj_var (iv1), k_stats_gimage_gm (gm0, ngm0), k_blur_stats_gimage_gm (gm1, mfgm1), kFoldStatsInside (dense iv0), deferred
    # statistics (2-DoF iv0), k_stats + kFoldScale (normalised); below Hp, Wp = 4 the two-kernel forms and k_stats -> kFoldStats
    "default": GRID + AXES,
    # k_blur_stats_var, k_stats, k_finalize
    "value_only": GRID,
    # k_blur_stats_var + k_gimage_blur_adj_var; the fused gradient-magnitude kernels with K3 deriving its own windows; k_stats -> kFoldStats
    "finish": GRID + [c for c in AXES if c["events"] == "border"],
    # k_blur3, k_stats<., 1024>, k_gimage, k_blur3_adj
    "deterministic": rotation(0) + rotation(3) + rotation(2, "2d-translation") + select(["image_variance@1", "gradient_magnitude@1"], [(17, 65), (18, 66), (4, 4)]),
    # k_gimage, k_blur3_adj, k_gimage_orig: G read at every sensor pixel
    "weight_grad": rotation(1) + rotation(4) + [case(s, lab, True, pad=p) for s, p in PADDED.items() for lab in ("image_variance@1", "normalized_gradient_magnitude@0")],
    # double-buffered vote images and musum buffers, the cached un-warped statistics
    "repeated": rotation(5) + rotation(2) + rotation(7, "2d-translation"),
}
OFFSET_PATTERNS = ("corners", "inner", "checker", "ramp", "constant")
# (pattern, row): every pattern on every shape, the objectives rotating
OFFSETS = [(p, c) for k, p in enumerate(OFFSET_PATTERNS) for c in rotation(k + 1)] + \
          [(p, c) for p in ("corners", "checker") for c in select(["image_variance@1", "gradient_magnitude@0", "gradient_magnitude@1"], [(17, 65), (18, 66)])]

_STATS_LABELS = ["image_variance@0", "image_variance@1", "gradient_magnitude@0", "gradient_magnitude@1", "normalized_image_variance@1",
                 "multi_focal_normalized_image_variance@0"]
_NSUB_ROWS = select(_STATS_LABELS, [(4, 4), (9, 33), (17, 65), (27, 101)]) + \
    [case(s, LABELS[i % 8], omits(s)[i % len(omits(s))], model="2d-translation") for i, s in enumerate(SHAPES)]
# child -> (environment, rows, mode).  mode: "grad" one evaluation with a gradient; "both" that and a value-only one (k_stats, k_blur_stats_var);
# "tan2": a gradient evaluation, the normalised rows evaluated twice (the first builds the un-warped statistics on the standard path)
CHILDREN = {
    "no_fused_blurvar": ({"CMAX_NO_FUSED_BLURVAR": "1"}, select(["image_variance@1", "normalized_image_variance@1"]) +
                         [c for c in AXES if c["label"] == "image_variance@1" and c["events"] == "border" and c["model"] == "dense-flow"], "grad"),
    "no_stats_inside": ({"CMAX_NO_STATS_INSIDE": "1"}, select(["image_variance@0"]) +
                        [c for c in AXES if c["label"] == "image_variance@0" and c["events"] == "border" and c["model"] == "dense-flow"], "grad"),
    "tan2": ({"CMAX_TAN2": "1"}, TAN2, "tan2"),
    "nsub1": ({"CMAX_NSUB": "1"}, _NSUB_ROWS, "both"),
    "nsub32": ({"CMAX_NSUB": "32"}, _NSUB_ROWS, "both"),
    "sweeps1": ({"CMAX_STAT_SWEEPS": "1"}, select(["image_variance@0"], LARGEST + [(7, 130), (4, 4)]), "grad"),
    "sweeps8": ({"CMAX_STAT_SWEEPS": "8"}, select(["image_variance@0"], LARGEST + [(7, 130), (4, 4)]), "grad"),
}
SWITCHES = ("CMAX_NO_FUSED_BLURVAR", "CMAX_NO_STATS_INSIDE", "CMAX_TAN2", "CMAX_NSUB", "CMAX_STAT_SWEEPS")
for _name in PATHS:
    PATHS[_name] = _unique(PATHS[_name])
ALL = dict(_REGISTRY)  # every row of every path


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def _ring(H, W):
    """distance of every sensor pixel to the sensor's edge (0 on the outermost ring)"""
    r, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return np.minimum(np.minimum(r, H - 1 - r), np.minimum(c, W - 1 - c)), r, c


def _outward(H, W):
    """(row, column) unit steps that leave the sensor by the nearest side(s); corners leave diagonally.  A one-pixel-wide sensor has
    no single outward side along that axis: its pixels alternate."""
    d, r, c = _ring(H, W)
    orow = np.where(r == d, -1.0, 0.0) + np.where(H - 1 - r == d, 1.0, 0.0)
    ocol = np.where(c == d, -1.0, 0.0) + np.where(W - 1 - c == d, 1.0, 0.0)
    alt = np.where((r + c) % 2 == 0, 1.0, -1.0)
    orow = np.where((orow == 0) & (H - 1 - r == r), alt, orow) if H == 1 else orow
    ocol = np.where((ocol == 0) & (W - 1 - c == c), alt, ocol) if W == 1 else ocol
    return orow, ocol


def dense_flow(c, rng, scale=1.0):
    """[2, H, W]: uniform in +-AMPLITUDE with a fractional part; the outermost ring of the sensor moves OUT of it by 0.97 AMPLITUDE along
    its normal (votes leave the image on all four sides, and reach a padded border), the ring behind it -- on the border set -- INTO the
    image.  A dense warp is x' = x - dt * flow."""
    H, W = c["size"]
    flow = rng.uniform(-AMPLITUDE, AMPLITUDE, (2, H, W))
    d, r, col = _ring(H, W)
    orow, ocol = _outward(H, W)
    push = 0.97 * AMPLITUDE
    out = d == 0
    # (along the ring it leans towards the nearer corner by less than a pixel: every pixel of a padding then has an event of the ring
    # pixel next to it above it, the padding's corners included)
    lean = rng.uniform(0.05, 0.6, (2, H, W))
    flow[0] = np.where(out & (orow == 0), np.where(r < H / 2.0, 1.0, -1.0) * lean[0], flow[0])
    flow[1] = np.where(out & (ocol == 0), np.where(col < W / 2.0, 1.0, -1.0) * lean[1], flow[1])
    flow[0] = np.where(out & (orow != 0), -orow * push, flow[0])
    flow[1] = np.where(out & (ocol != 0), -ocol * push, flow[1])
    if c["events"] == "border":
        inward = d == 1
        flow[0] = np.where(inward & (orow != 0), orow * push, flow[0])
        flow[1] = np.where(inward & (ocol != 0), ocol * push, flow[1])
    return f32(flow * scale)


THETAS = [(1.31, -0.83), (-1.17, 1.42), (0.77, 1.29), (-1.44, -0.91)]


def motion(c, rng, scale=1.0):
    if c["model"] == "2d-translation":
        k = LABELS.index(c["label"]) if c["label"] in LABELS else 0
        return np.asarray(THETAS[(c["shape"][0] + c["shape"][1] + k) % 4]) * scale
    flow = dense_flow(c, rng, scale)
    if c["model"] == "dense-flow":
        return flow
    return f32(np.stack([flow * (1.0 - 0.3 * k) for k in range(c["T"])]))


def _sources(c, rng):
    """integer source pixels [n, 2] of the case's event set"""
    H, W = c["size"]
    d, r, col = _ring(H, W)
    if c["events"] == "border":
        sel = d < 2
        k = rng.integers(20, 41, int(sel.sum()))  # (uneven: a constant un-warped image has no contrast to normalise by)
        rows, cols = np.repeat(r[sel], k), np.repeat(col[sel], k)
        if c["model"] == "2d-translation":  # finite off-sensor sources, up to 3 px outside on every side
            rr, cc = np.meshgrid(np.arange(-3, H + 3), np.arange(-3, W + 3), indexing="ij")
            off = (rr < 0) | (rr >= H) | (cc < 0) | (cc >= W)
            k = rng.integers(6, 19, int(off.sum()))
            rows, cols = np.concatenate([rows, np.repeat(rr[off], k)]), np.concatenate([cols, np.repeat(cc[off], k)])
        return np.stack([rows, cols], axis=1)
    per = 30 if c["events"] == "cover" else 1
    n = min(per * H * W, MAX_EVENTS)
    if c["events"] == "cover":  # 30 per pixel on average, every pixel at least 20
        base = np.stack([np.repeat(r.ravel(), 20), np.repeat(col.ravel(), 20)], axis=1)
        extra = np.stack([rng.integers(0, H, n - len(base)), rng.integers(0, W, n - len(base))], axis=1)
        return np.concatenate([base, extra])
    return np.stack([rng.integers(0, H, n), rng.integers(0, W, n)], axis=1)


def directions(c):
    return R.cost_directions(c["cost"], "first")


def ref_kwargs(c):
    return dict(cost=c["cost"], sigma=c["sigma"], outer_padding=c["pad"], omit_boundary=c["omit"], direction=c["direction"])


def batch(c, motions):
    """[n, 4] events of the case: seeded, times sorted, filtered for every motion in `motions`.  -> (events, share dropped)"""
    rng = np.random.default_rng([c["shape"][0], c["shape"][1], c["pad"], c["seed"], {"cover": 1, "sparse": 2, "border": 3}[c["events"]],
                                 {"dense-flow": 1, "2d-translation": 2, "dense-flow-voxel": 3}[c["model"]]])
    src = _sources(c, rng)
    src = src[rng.permutation(len(src))]
    n = len(src)
    ev = np.stack([src[:, 0].astype(np.float64), src[:, 1].astype(np.float64), np.sort(rng.uniform(0.0, PERIOD, n)), rng.integers(0, 2, n).astype(np.float64)],
                  axis=1)
    for _ in range(4):
        before = len(ev)
        for m in motions:
            margin = R.border_margin(ev, m, c["model"], c["size"], directions(c))
            ev, _ = R.drop_ambiguous(ev, m, c["model"], c["size"], directions(c), margin)
        if len(ev) == before:
            break
    return ev, (n - len(ev)) / max(n, 1)


def _motion_rng(c):
    return np.random.default_rng([c["shape"][0], c["shape"][1], c["pad"], c["seed"], 77])


REPEAT_SCALES = (1.0, -0.8, 0.55, 0.9)  # the four motions of the `repeated` path
_BUILT = {}


def built(c, repeated=False):
    """-> dict(ev, motion, motions, dropped).  `motions`: the four motions of the repeated path (the batch is filtered for all four)."""
    key = (c["id"], repeated)
    if key not in _BUILT:
        motions = [motion(c, _motion_rng(c), s) for s in (REPEAT_SCALES if repeated else (1.0,))]
        ev, dropped = batch(c, motions)
        assert len(ev) <= MAX_EVENTS
        _BUILT[key] = dict(ev=ev, motion=motions[0], motions=motions, dropped=dropped)
    return _BUILT[key]


def weight_grad_batch(c):
    """-> (events, motion) of the weight-gradient path: 1 to 4 events on EVERY sensor pixel (a constant image has no contrast), integral
    sources, evaluated at zero motion: dL/dw_e is then the sum over the reference times of G_k at the event's own pixel."""
    H, W = c["size"]
    rng = np.random.default_rng([c["shape"][0], c["shape"][1], c["pad"], 5])
    count = rng.integers(1, 5, (H, W))
    r, col = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    rows, cols = np.repeat(r.ravel(), count.ravel()), np.repeat(col.ravel(), count.ravel())
    order = rng.permutation(len(rows))
    n = len(rows)
    ev = np.stack([rows[order].astype(np.float64), cols[order].astype(np.float64), np.sort(rng.uniform(0.0, PERIOD, n)), np.ones(n)], axis=1)
    if "normalized" in c["cost"] and not (c["cost"].endswith("image_variance") and c["omit"]):
        # (at zero motion a normalised cost is the ratio of two equal images' contrasts: where both are cropped alike its derivative is
        # identically zero.  Those rows take the row's own motion: dL/dw_e is then G interpolated at the warped event, still per event.
        # The normalised variance under omit_boundary crops only the warped image, so it keeps zero motion and reads k_gimage_orig pointwise)
        return ev, motion(c, _motion_rng(c))
    return ev, (np.zeros(2) if c["model"] == "2d-translation" else np.zeros((2,) + c["size"]))


# ---- offsets of caller-supplied images ------------------------------------------------------------------------------------------
def n_slots(c):
    return len(directions(c)) + (1 if "normalized" in c["cost"] else 0)


def offsets(pattern, c, vote_max):
    """One fp64 [Hp, Wp] array per image slot (reference times, then the un-warped image of a normalised cost), exact in fp32, amplitudes
    between 0.25 x and 1 x `vote_max` (the largest entry of the case's own vote images)."""
    Hp, Wp = c["shape"]
    r, col = np.meshgrid(np.arange(Hp), np.arange(Wp), indexing="ij")
    out = []
    for k in range(n_slots(c)):
        amp = vote_max * (1.0, 0.5, 0.5, 0.75)[k]  # (the patterns scale it by 0.5 at the least: 0.25 x vote_max and up)
        o = np.zeros((Hp, Wp))
        if pattern == "corners":  # a spike at each of the four corner pixels, signs and sizes differing
            for (i, j), f in zip(((0, 0), (0, Wp - 1), (Hp - 1, 0), (Hp - 1, Wp - 1)), (1.0, -0.5, 0.75, -1.0)):
                o[i, j] += f * amp
        elif pattern == "inner":  # (1, 1) and (Hp - 2, Wp - 2): the first pixels inside the omitted boundary
            o[min(1, Hp - 1), min(1, Wp - 1)] += amp
            o[max(Hp - 2, 0), max(Wp - 2, 0)] -= 0.5 * amp
        elif pattern == "checker":  # +-1 across every tile seam (and everywhere else)
            o = np.where((r + col) % 2 == 0, amp, -amp)
        elif pattern == "ramp":  # smooth, with negative values
            o = amp * (np.sin(0.9 * r / max(Hp - 1, 1) * np.pi + 0.3) * np.cos(1.7 * col / max(Wp - 1, 1) * np.pi) - 0.2 + 0.5 * (col - r) / (Hp + Wp))
        else:
            assert pattern == "constant"
            o = np.full((Hp, Wp), 0.5 * amp)
        out.append(f32(o))
    return out
