"""The cases of the exact-product parity tests: built once per process, shared by tests/test_hvp_reference.py (which anchors the fp64
reference on them without a GPU and checks the share of dropped events) and tests/test_gpu_hvp_parity.py / tests/_layout_worker.py
(which hold the kernels to it).  A case is a dict of plain values; `built(case)` makes its batch, motion and tangent -- motion and
tangent rounded to fp32, so that both sides see the same numbers --, removes the events the product is not defined for
(_hvp_ref.drop_ambiguous) and evaluates the reference ONCE."""
import numpy as np

import event_based_optical_flow_amd as E
import _hvp_ref as R

BASE = (40, 56)  # 3 x 4 tiles of 16 x 16, ragged on both axes
VEL = (7.0, -5.0)  # pixel per batch period
PERIOD = 0.05
DROP_CAP = 0.005
COSTS = ["image_variance", "gradient_magnitude", "normalized_image_variance", "normalized_gradient_magnitude",
         "multi_focal_normalized_image_variance", "multi_focal_normalized_gradient_magnitude"]
MODELS = ["2d-translation", "dense-flow", "dense-flow-voxel"]
_SHORT = {"2d-translation": "2dof", "dense-flow": "dense", "dense-flow-voxel": "voxel", "image_variance": "iv", "gradient_magnitude": "gm",
          "normalized_image_variance": "niv", "normalized_gradient_magnitude": "ngm", "multi_focal_normalized_image_variance": "mfiv",
          "multi_focal_normalized_gradient_magnitude": "mfgm"}


def f32(x):
    """the values the device holds (fp32) in the container the references take (fp64)"""
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def case(group, model, cost, sigma, n=30_000, **kw):
    c = dict(group=group, model=model, cost=cost, sigma=int(sigma), n=int(n), size=BASE, pad=0, omit=True, direction="minimize",
             warp_direction="first", normalize_t=True, frac=False, outside=False, T=0, events="structured", mag=None, tangent="normal",
             zero_motion=False, deterministic=False, slabs=0, seed=0, t_slice=None)
    c.update(kw)
    if model == "dense-flow-voxel" and not c["T"]:
        c["T"] = 5
    c["id"] = "-".join(str(p) for p in (
        group, _SHORT[model] + (str(c["T"]) if c["T"] else ""), _SHORT[cost], f"s{c['sigma']}", f"n{c['n']}",
        *(k + str(c[k]) for k in ("pad",) if c[k]), *(k for k in ("frac", "outside", "zero_motion", "deterministic") if c[k]),
        *(f"{k}{c[k]}" for k in ("slabs",) if c[k]), *(str(c[k]) for k in ("direction", "warp_direction") if c[k] not in ("minimize", "first")),
        *(("raw_t",) if not c["normalize_t"] else ()), *(("border",) if not c["omit"] else ()),
        *((c["tangent"],) if c["tangent"] != "normal" else ()), *((f"slice{c['t_slice']}",) if c["t_slice"] is not None else ())))
    return c


def _matrix():
    out = []
    sizes = (60, 2000, 30_000)  # one partly filled wave; a few segments; the n / 512 segment cap (~120 segments)
    for mi, model in enumerate(MODELS):
        for ci, cost in enumerate(COSTS):
            for sigma in (0, 1):
                i = 2 * ci + sigma
                out.append(case("matrix", model, cost, sigma, n=sizes[(i + mi) % 3], T=(2 if i % 2 == 0 else 5) if model == "dense-flow-voxel" else 0,
                                seed=10 * i + mi))
    return out


def _edges():
    out = []
    two, dense, voxel = MODELS
    iv, gm, niv, ngm, mfiv, mfgm = COSTS
    # fractional sources (reference time 1/3) and padding, pairwise; 2-DoF on both costs: its plain variance has a tangent kernel of its own
    for model in (two, dense):
        for frac, pad in ((True, 0), (True, 3), (False, 3)):
            for cost, sigma in ((iv, 0), (gm, 1)):
                out.append(case("fracpad", model, cost, sigma, frac=frac, pad=pad, warp_direction=(1.0 / 3.0) if frac else "first", seed=21))
    out += [case("border", two, iv, 1, n=2000, omit=False, seed=22), case("border", dense, gm, 0, n=2000, omit=False, seed=22),
            case("border", voxel, niv, 1, n=2000, omit=False, seed=22), case("border", two, ngm, 0, n=2000, omit=False, seed=22)]
    out += [case("maximize", two, mfgm, 1, n=2000, direction="maximize", seed=23), case("maximize", dense, iv, 0, n=2000, direction="maximize", seed=23),
            case("maximize", voxel, ngm, 1, n=2000, direction="maximize", seed=23), case("maximize", two, niv, 0, n=2000, direction="maximize", seed=23)]
    for wd in ("middle", "last", 0.3):
        out += [case("reftime", two, gm, 0, warp_direction=wd, seed=24), case("reftime", dense, iv, 1, warp_direction=wd, seed=24)]
    out += [case("rawtime", two, mfiv, 0, normalize_t=False, seed=25), case("rawtime", two, iv, 1, normalize_t=False, seed=25),
            case("rawtime", dense, gm, 1, normalize_t=False, seed=25), case("rawtime", dense, mfgm, 0, normalize_t=False, n=2000, seed=25),
            case("rawtime", voxel, iv, 0, normalize_t=False, seed=25), case("rawtime", voxel, mfgm, 1, normalize_t=False, T=2, seed=25)]
    for pad in (0, 3):
        out += [case("outside", two, iv, 0, outside=True, pad=pad, seed=26), case("outside", two, gm, 1, outside=True, pad=pad, seed=26),
                case("outside", two, mfiv, 1, outside=True, pad=pad, n=2000, seed=26)]
    # the clipped LDS window: the batch of test_large_displacements_clip_the_lds_window; the same batch in four time slabs
    for slabs in (0, 4):
        for model, cost, sigma in ((two, iv, 0), (two, gm, 1), (dense, iv, 0), (dense, gm, 1)):
            out.append(case("clipped", model, cost, sigma, n=120_000, size=(130, 173), events="uniform", mag=150.0, slabs=slabs, seed=61))
    out += [case("tangent", dense, iv, 0, tangent="onehot", seed=27), case("tangent", dense, gm, 1, tangent="onehot", seed=27),
            case("tangent", voxel, iv, 1, tangent="onehot", T=2, seed=27)]
    out += [case("zero", two, iv, 0, n=2000, zero_motion=True, seed=28), case("zero", two, gm, 1, n=2000, zero_motion=True, seed=28),
            case("zero", dense, iv, 1, n=2000, zero_motion=True, seed=28), case("zero", dense, gm, 0, n=2000, zero_motion=True, seed=28)]
    for model in MODELS:
        out += [case("det", model, iv, 1, deterministic=True, seed=29), case("det", model, gm, 0, deterministic=True, seed=29)]
    out += [case("slices", two, iv, 0, normalize_t=False, t_slice=0, seed=30), case("slices", two, iv, 0, normalize_t=False, t_slice=1, seed=30),
            case("slices", dense, iv, 1, normalize_t=False, t_slice=0, seed=30), case("slices", dense, iv, 1, normalize_t=False, t_slice=1, seed=30)]
    return out


CASES = _matrix() + _edges()

# Non-default segment layouts, each forced by its environment switch in a fresh child process (tests/_layout_worker.py).
# mid: 256 x 256 tiles of ~2340 +- 50 uniform events: a group-aligned list of >= 256 x 2040 events whose groups hold <= 3064 events.
_B = dict(n=150_000, size=(96, 128), events="uniform", mag=10.0, seed=41)
_M = dict(n=600_000, size=(256, 256), events="uniform", mag=10.0, seed=42)
LAYOUT_CASES = {
    "big": [case("big", "2d-translation", COSTS[0], 0, **_B), case("big", "2d-translation", COSTS[1], 1, **_B),
            case("big", "dense-flow", COSTS[0], 1, **_B), case("big", "dense-flow", COSTS[1], 0, **_B),
            case("big", "dense-flow-voxel", COSTS[0], 0, T=5, **_B), case("big", "dense-flow-voxel", COSTS[1], 1, T=5, **_B),
            case("big", "dense-flow", COSTS[0], 0, frac=True, warp_direction=1.0 / 3.0, **_B),
            case("big", "2d-translation", COSTS[5], 1, **_B), case("big", "dense-flow", COSTS[4], 0, **_B)],
    "mid": [case("mid", "dense-flow", COSTS[0], 0, **_M), case("mid", "2d-translation", COSTS[0], 1, **_M)],
}
LAYOUT_ENV = {"big": [{"CMAX_BIG_SEG": "1"}, {"CMAX_BIG_SEG": "1", "CMAX_COMPACT": "0"}], "mid": [{"CMAX_MID_SEG": "1"}]}
LAYOUT_SEGMENT_EVENTS = {"big": 4088, "mid": 3064}
ALL = {c["id"]: c for c in CASES + LAYOUT_CASES["big"] + LAYOUT_CASES["mid"]}
assert len(ALL) == len(CASES) + len(LAYOUT_CASES["big"]) + len(LAYOUT_CASES["mid"]), "case ids must be unique"


def ref_kwargs(c, t_range=None):
    return dict(cost=c["cost"], sigma=c["sigma"], outer_padding=c["pad"], omit_boundary=c["omit"], direction=c["direction"],
                warp_direction=c["warp_direction"], normalize_t=c["normalize_t"], t_range=t_range)


def _batch(c):
    rng = np.random.default_rng(7000 + c["seed"])
    (H, W), n = c["size"], c["n"]
    if c["events"] == "uniform":
        ev = E.utils.generate_events(n, H, W, 0.0, PERIOD, seed=c["seed"])
    else:
        ev = E.utils.generate_structured_events(n, H, W, VEL, n_dots=max(3, n // 60), seed=c["seed"], tmin=0.0, tmax=PERIOD)
    if c["frac"]:  # rectified events
        ev[:, 0] = np.minimum(ev[:, 0] + rng.uniform(0, 0.99, n), H - 1e-3)
        ev[:, 1] = np.minimum(ev[:, 1] + rng.uniform(0, 0.99, n), W - 1e-3)
    if c["outside"]:  # a quarter of the sources up to 30 px off the sensor
        sel = rng.random(n) < 0.25
        ev[sel, 0] = rng.uniform(-30.0, H + 30.0, int(sel.sum()))
        ev[sel, 1] = rng.uniform(-30.0, W + 30.0, int(sel.sum()))
    t_range = None
    if c["t_slice"] is not None:  # one half of the batch, with the whole batch's extremes
        t_range = (float(ev[:, 2].min()), float(ev[:, 2].max()))
        ev = ev[: n // 2] if c["t_slice"] == 0 else ev[n // 2:]
    return ev, t_range, rng


def _motion(c, rng):
    (H, W), model, T = c["size"], c["model"], c["T"]
    if c["mag"] is not None:  # uniform batches: a motion of the given magnitude
        mag = c["mag"]
        theta = np.array([0.9871 * mag, -0.9317 * mag])  # (no whole number of pixels: the last event would end on a cell border)
        flow = E.utils.generate_smooth_flow((H, W), mag, grid=3, seed=c["seed"] + 1)
    else:  # about 0.9 x the generating velocity plus a smooth flow (dense models warp with minus the flow)
        theta = 0.9 * np.asarray(VEL)
        flow = -(E.utils.generate_smooth_flow((H, W), 4.0, grid=3, seed=c["seed"] + 7) * 0.3 + theta[:, None, None])
    if model == "2d-translation":
        m = theta
    elif model == "dense-flow":
        m = flow
    else:
        m = np.stack([flow * (1.0 + 0.05 * k) for k in range(T)])
    if c["zero_motion"]:
        m = np.zeros_like(m)
    if not c["normalize_t"]:
        m = m / PERIOD  # pixel per second
    return f32(m)


def _tangent(c, motion, ev, rng):
    v = rng.normal(0.0, 1.0, motion.shape)
    if c["tangent"] == "onehot":  # one column of the Hessian: the source pixel that holds the most events
        cnt = np.zeros(c["size"], dtype=np.int64)
        np.add.at(cnt, (ev[:, 0].astype(np.int64), ev[:, 1].astype(np.int64)), 1)
        r, col = np.unravel_index(int(cnt.argmax()), cnt.shape)
        v = np.zeros(motion.shape)
        v[(0, 1, r, col) if motion.ndim == 4 else (1, r, col)] = 1.0
    return f32(v)


_BUILT = {}


def inputs(c):
    """-> dict(ev, t_range, motion, v, dropped, margin): the case's batch after the filter, its motion and its tangent."""
    ev, t_range, rng = _batch(c)
    motion = _motion(c, rng)
    v = _tangent(c, motion, ev, rng)
    dirs = R.cost_directions(c["cost"], c["warp_direction"])
    margin = R.border_margin(ev, motion, c["model"], c["size"], dirs, c["normalize_t"], t_range)
    kept, dropped = R.drop_ambiguous(ev, motion, c["model"], c["size"], dirs, margin, c["normalize_t"], t_range)
    return dict(ev=kept, t_range=t_range, motion=motion, v=v, dropped=dropped, margin=margin)


def built(c):
    """inputs(c) plus the reference's answers loss, grad, hv -- computed once per process and shared."""
    if c["id"] not in _BUILT:
        b = inputs(c)
        b["loss"], b["grad"], b["hv"] = R.value_grad_hvp(b["ev"], b["motion"], c["model"], c["size"], b["v"], **ref_kwargs(c, b["t_range"]))
        _BUILT[c["id"]] = b
    return _BUILT[c["id"]]
