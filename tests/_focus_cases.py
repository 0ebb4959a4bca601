"""TEST INFRASTRUCTURE ONLY: the cases of the focus-loss tests, shared by tests/test_focus_reference.py (CPU: the share of dropped events),
tests/test_gpu_focus_costs.py and its child program tests/_focus_worker.py.

The fused image kernel works on 8 x 32 tiles: 8 x 32 is one tile, 9 x 33 lies one pixel past a seam both ways, 17 x 40 and 37 x 53 are
several ragged tiles, 3 x 34 with omit_boundary leaves an Omega one row high; padding 2 turns 17 x 40 into 21 x 44.  The product
costs x forms x omit x sigma x padding x models x directions is pruned to the list below so that every value of every axis occurs with
every cost.  About 4 000 uniform events each; motions of at most 10 px over the batch.  Events whose warped coordinate lies within
fp32 rounding of a cell border are removed first (_hvp_ref.drop_ambiguous; at most DROP_CAP of them)."""
import numpy as np

import event_based_optical_flow_amd as E
import _focus_ref as R

N_EVENTS = 4000
PERIOD = 0.05
DROP_CAP = 0.05
TWO, DENSE, VOXEL = "2d-translation", "dense-flow", "dense-flow-voxel"
MS, LAP, HES = "mean_square", "laplacian_magnitude", "hessian_magnitude"
_SHORT = {TWO: "2dof", DENSE: "dense", VOXEL: "voxel3", MS: "ms", LAP: "lap", HES: "hes"}


def f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def case(kind, form, model, shape, sigma=0, omit=True, pad=0, direction="minimize", seed=0):
    cost = {"plain": "", "norm": "normalized_", "multi": "multi_focal_normalized_"}[form] + kind
    c = dict(kind=kind, form=form, cost=cost, model=model, size=shape, sigma=sigma, omit=omit, pad=pad, direction=direction,
             T=3 if model == VOXEL else 0, seed=seed)
    c["id"] = "-".join([_SHORT[kind], form, _SHORT[model], f"{shape[0]}x{shape[1]}", f"s{sigma}"] + (["border"] if not omit else []) +
                       ([f"pad{pad}"] if pad else []) + ([direction] if direction != "minimize" else []))
    return c


CASES = [
    case(MS, "plain", TWO, (8, 32), seed=1),
    case(LAP, "plain", TWO, (9, 33), seed=2),
    case(HES, "plain", DENSE, (17, 40), seed=3),
    case(MS, "norm", DENSE, (37, 53), sigma=1, seed=4),
    case(LAP, "multi", VOXEL, (37, 53), sigma=1, seed=5),
    case(HES, "norm", TWO, (17, 40), sigma=1, omit=False, seed=6),
    case(LAP, "plain", TWO, (3, 34), seed=7),
    case(HES, "multi", DENSE, (9, 33), direction="maximize", seed=8),
    case(MS, "multi", VOXEL, (17, 40), omit=False, direction="maximize", seed=9),
    case(LAP, "norm", DENSE, (17, 40), sigma=1, pad=2, seed=10),
    case(HES, "plain", VOXEL, (37, 53), sigma=1, direction="maximize", seed=11),
    case(HES, "plain", TWO, (3, 34), sigma=1, seed=12),
    case(LAP, "plain", DENSE, (8, 32), omit=False, pad=2, direction="maximize", seed=13),
    case(MS, "plain", TWO, (37, 53), omit=False, direction="maximize", seed=14),
    case(MS, "norm", TWO, (9, 33), sigma=1, pad=2, direction="maximize", seed=15),
]
ALL = {c["id"]: c for c in CASES}
assert len(ALL) == len(CASES), "case ids must be unique"


def ref_kwargs(c):
    return dict(cost=c["cost"], sigma=c["sigma"], outer_padding=c["pad"], omit_boundary=c["omit"], direction=c["direction"])


def descriptor(c):
    return E.make_descriptor(c["cost"], c["model"], direction=c["direction"], sigma=float(c["sigma"]), omit_boundary=c["omit"], time_bin=c["T"])


def handle(c, ev, deterministic=False):
    h = E.CMaxHandle(c["size"], c["pad"])
    if deterministic:
        h.set_deterministic(True)
    h.set_events(ev, time_bin=c["T"], on_dropped="ignore")
    assert h.n_events == len(ev), (c["id"], h.n_events, len(ev))
    return h


def _motion(c, rng):
    (H, W), model = c["size"], c["model"]
    # (no whole number of pixels: the last event would end on a cell border); at most 10 px, less on the small shapes
    theta = np.array([0.9871 * min(5.0, H / 4.0), -0.9317 * min(7.0, W / 4.0)])
    if model == TWO:
        return f32(theta)
    flow = -(E.utils.generate_smooth_flow((H, W), 2.0, grid=3, seed=c["seed"] + 7) * 0.5 + theta[:, None, None])
    return f32(flow if model == DENSE else np.stack([flow * (1.0 + 0.05 * k) for k in range(c["T"])]))


def inputs(c):
    """-> dict(ev, motion, v, dropped): the batch after the filter, motion and tangent (fp32 values in fp64 containers)."""
    rng = np.random.default_rng(9000 + c["seed"])
    H, W = c["size"]
    ev = E.utils.generate_events(N_EVENTS, H, W, 0.0, PERIOD, seed=c["seed"])
    motion = _motion(c, rng)
    v = f32(rng.normal(0.0, 1.0, motion.shape))
    dirs = R.cost_directions(c["cost"], "first")
    margin = R.border_margin(ev, motion, c["model"], c["size"], dirs)
    kept, dropped = R.drop_ambiguous(ev, motion, c["model"], c["size"], dirs, margin)
    return dict(ev=kept, motion=motion, v=v, dropped=dropped)


_BUILT = {}


def built(c):
    """inputs(c) plus the reference's loss, grad, hv -- computed once per process, shared and left unchanged."""
    if c["id"] not in _BUILT:
        b = inputs(c)
        b["loss"], b["grad"], b["hv"] = R.value_grad_hvp(b["ev"], b["motion"], c["model"], c["size"], b["v"], **ref_kwargs(c))
        _BUILT[c["id"]] = b
    return _BUILT[c["id"]]
