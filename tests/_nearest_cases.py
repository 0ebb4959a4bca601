"""The case table of tests/test_gpu_nearest_filter.py (and of its child process, tests/_nearest_plan_worker.py): the geometries of
tests/_patch_cases.py plus the ones only the nearest filter asks for, and the plan cases with their references (tests/_mixed_ref.py),
computed once per process and never modified."""
import numpy as np

import event_based_optical_flow_amd as E
from event_based_optical_flow_amd.solver import PatchFlowObjective

import _hvp_ref
import _mixed_ref
import _patch_cases as C

EXTRA = [
    C.geometry("sw25", (2, 3), (1, 1), (25, 25), [(51, 75), (50, 74)]),   # the largest factor of the fixture's table; odd and even H
    C.geometry("1x1-pad1", (1, 1), (1, 1), (9, 7), [(20, 15), (27, 21)]),  # one cell: every pixel is its, padding included
]
GEOMETRY = dict(C.GEOMETRY, **{g["id"]: g for g in EXTRA})
LEAF_CASES = list(C.LEAF_CASES) + [(g["id"], s) for g in EXTRA for s in g["sizes"]]


def crop_offset(g, size, k):
    return ((g["patch_image_size"][k] + 2 * g["pad"][k]) * g["sw"][k]) // 2 - size[k] // 2


def border_pixels(gid, size):
    """Pixels for one-hot cotangents: per axis the sensor's first and last line and the lines on either side of EVERY border between
    two cells of the up-sampled array ((line + crop offset) % sw in {0, sw - 1}), crossed with three lines of the other axis."""
    g = GEOMETRY[gid]
    lines = []
    for k in (0, 1):
        n, sw, off = size[k], g["sw"][k], crop_offset(g, size, k)
        at = (np.arange(n) + off) % sw
        lines.append(sorted({0, n - 1} | set(np.nonzero((at == 0) | (at == sw - 1))[0].tolist())))
    rows, cols = lines
    some_cols = sorted({cols[0], cols[len(cols) // 2], cols[-1]})
    some_rows = sorted({rows[0], rows[len(rows) // 2], rows[-1]})
    return sorted({(i, j) for i in rows for j in some_cols} | {(i, j) for j in cols for i in some_rows})


# ---- the native plan -------------------------------------------------------------------------------------------------------------------
_BURGERS = dict(time_aware=True, T=10, scheme="burgers", t0="middle")
PLAN_CASES = {
    "plain": dict(gid="overlap", size=(68, 90), motion="random", kw={}),
    "burgers": dict(gid="overlap", size=(68, 90), motion="random", kw=_BURGERS),
    "odd-plain": dict(gid="3x4-odd", size=(27, 40), motion="random", kw={}),
    "plain-exact": dict(gid="overlap", size=(68, 90), motion="random", kw={}, exact_flow=True),
    "burgers-exact": dict(gid="overlap", size=(68, 90), motion="random", kw=_BURGERS, exact_flow=True),
    "burgers-scale-later": dict(gid="overlap", size=(68, 90), motion="random", kw=dict(scale_later=True, **_BURGERS)),
}
_BUILT = {}


def built(cid, filter_type="nearest"):
    """-> dict(ev, x, v, spec, exact_flow, dropped, loss, grad, hv): the batch without the events within the scaled margin of a cell
    border at the motion the device holds (as tests/_patch_cases.hvp_inputs: the product is not defined there)."""
    key = (cid, filter_type)
    if key not in _BUILT:
        c = PLAN_CASES[cid]
        exact = bool(c.get("exact_flow"))
        pis = GEOMETRY[c["gid"]]["patch_image_size"]
        x = C.patch_motion(c["motion"], pis, 500 + sum(ord(ch) for ch in cid))
        ev = C.batch(c["size"])
        spec = C.spec_of(c["gid"], c["size"], t_scale=float(ev[:, 2].max() - ev[:, 2].min()), **c["kw"])
        spec.update(filter=filter_type, round32=not exact)  # exact_flow: the fused terms see the fp64 field itself
        model = "dense-flow-voxel" if spec["time_aware"] else "dense-flow"
        m = _mixed_ref.device_motion(x, dict(spec, round32=True))
        directions = sorted({d for cost, _ in spec["terms"] for d in _hvp_ref.cost_directions(cost)})
        margin = _hvp_ref.border_margin(ev, m, model, spec["size"], directions)
        ev, dropped = _hvp_ref.drop_ambiguous(ev, m, model, spec["size"], directions, margin)
        v = C.f32(np.random.default_rng(77 + len(cid)).normal(size=x.shape))
        loss, grad, hv = _mixed_ref.plan(x, ev, spec, v=v)
        _BUILT[key] = dict(ev=ev, x=x, v=v, spec=spec, exact_flow=exact, dropped=dropped, loss=loss, grad=grad, hv=hv)
    return _BUILT[key]


def make_objective(ev, spec, exact_flow=False, filter_type=None):
    """filter_type None: the argument is not passed at all (a caller written before it existed)."""
    h = E.CMaxHandle(spec["size"])
    h.set_events(ev, time_bin=spec["T"] if spec["time_aware"] else 0)
    assert h.n_events == len(ev)
    names = {name: w for name, w in spec["terms"]}
    if spec["tv_weight"]:
        names["total_variation"] = spec["tv_weight"]
    hybrid = len(names) > 1
    # patch_size == sliding_window and a shift of (pad - 1) windows give the table's pad through patch_pad
    shift = tuple(max(spec["pad"][k] - 1, 0) * spec["sw"][k] for k in (0, 1))
    kw = {} if filter_type is None else {"filter_type": filter_type}
    obj = PatchFlowObjective(h, spec["t_scale"], spec["patch_image_size"], spec["sw"], spec["sw"], shift,
                             cost="hybrid" if hybrid else next(iter(names)), cost_with_weight=names if hybrid else None, blur_sigma=spec["sigma"],
                             time_aware=spec["time_aware"], time_bin=spec["T"], flow_interpolation=spec["scheme"], t0_flow_location=spec["t0"],
                             scale_later=spec["scale_later"], omit_boundary=spec["omit"], exact_flow=exact_flow, **kw)
    assert obj.has_native_plan and obj.pad == tuple(spec["pad"])
    return h, obj
