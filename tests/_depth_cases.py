"""The case table of the depth-plan tests (tests/test_depth_reference.py on the CPU, tests/test_gpu_depth_plan.py on the GPU): the smallest
shapes that reach each branch of csrc/cmax_depth_kernels.h and of the depth plan (csrc/cmax_solver.hip).  References are computed once per
process and shared (built_*), and never modified."""
import numpy as np

import event_based_optical_flow_amd as E

import _basis_cases as B
import _depth_ref
import _hvp_ref
import _patch_cases as C

PERIOD = C.PERIOD
DROP_CAP = C.DROP_CAP  # 0.005 of the batch: a condition on every product case, asserted in tests/test_depth_reference.py
ADJ_CHUNK = 1024       # CMAX_DEPTH_ADJ_CHUNK: PIXELS per workgroup of k_depth_adj
ONE_TERM, TWO_TERMS, BURGERS, UPWIND = B.ONE_TERM, B.TWO_TERMS, B.BURGERS, B.UPWIND
# (geometry of tests/_patch_cases.py, sensor): 560 pixels (below one chunk), 1080 (one seam), 1014 (below, odd extent), 5940 (cells without a
# pixel), 6120 (five seams)
LEAF_CASES = [("1x1-pad0", (20, 28)), ("3x4-odd", (27, 40)), ("3x4-odd", (26, 39)), ("16x16-sw16x21", (66, 90)), ("overlap", (68, 90))]
LEAF_K = [(1, 0), (3, 3), (3, 5), (2, 62)]  # no B at all; one tile / across the tile of four fields; the largest Ka + Kb
_BUILT = {}


def geometry_spec(gid, size):
    g = C.GEOMETRY[gid]
    return dict(size=tuple(size), patch_image_size=g["patch_image_size"], sw=g["sw"], pad=g["pad"])


def geometry_six(spec):
    return tuple(spec["patch_image_size"]) + tuple(spec["pad"]) + tuple(spec["sw"])


def leaf_inputs(gid, size, Ka, Kb):
    """-> (spec with A, B; x, u [nx]; g, dg [2,H,W]): every value exact in fp32, so both precisions see the same numbers."""
    spec = geometry_spec(gid, size)
    ph, pw = spec["patch_image_size"]
    rng = np.random.default_rng(7000 + 31 * size[0] + size[1] + 100 * Ka + Kb)
    spec["A"] = B.smooth_basis(Ka, size, 40 + Ka)
    spec["B"] = B.smooth_basis(Kb, size, 50 + Kb) if Kb else np.zeros((0, 2) + tuple(size))
    nx = Ka + Kb + ph * pw
    x, u = C.f32(rng.normal(0.0, 2.0, nx)), C.f32(rng.normal(0.0, 1.0, nx))
    g, dg = C.f32(rng.normal(size=(2,) + tuple(size))), C.f32(rng.normal(size=(2,) + tuple(size)))
    return spec, x, u, g, dg


def seam_pixels(size):
    """(row, column) of the first and last pixel and of both sides of every chunk seam of the adjoint."""
    H, W = size
    out = {0, H * W - 1}
    for s in range(ADJ_CHUNK, H * W, ADJ_CHUNK):
        out |= {s - 1, s}
    return [(e // W, e % W) for e in sorted(out)]


# ---- plan cases: camera bases ------------------------------------------------------------------------------------------------------
def calib_of(size):
    """A camera whose principal point is the sensor's centre; the focal length makes the field of view about 37 degrees wide."""
    H, W = size
    f = 1.5 * W
    return (f, f, (W - 1) / 2.0, (H - 1) / 2.0)


# a PERIOD f / 60 and b PERIOD: with rho around 1, some 3 px of translation over the batch and well under 1 px of rotation -- neither
# component of the flow changes sign on the sensor (the upwind selectors of the voxel chain take that sign)
A_DISP = (0.05, -0.04, 0.02)
B_DISP = (0.004, -0.006, 0.01)


def case(cid, gid, size, terms=ONE_TERM, exact=False, basis_dtype="float64", sigma=1.0, **kw):
    return dict(id=cid, gid=gid, size=tuple(size), terms=tuple(terms), exact=exact, basis_dtype=basis_dtype, sigma=sigma, kw=kw)


PLAN_CASES = [
    case(f"cam-{size[0]}x{size[1]}-{tname}", gid, size, terms=terms)
    for gid, size in (("3x4-odd", (27, 40)), ("overlap", (68, 90))) for tname, terms in (("one", ONE_TERM), ("two", TWO_TERMS))
] + [
    case("cam-27x40-zero", "3x4-odd", (27, 40), terms=TWO_TERMS),
    case("cam-68x90-exact", "overlap", (68, 90), terms=TWO_TERMS, exact=True),
    case("cam-27x40-exact-one", "3x4-odd", (27, 40), terms=ONE_TERM, exact=True),
    case("cam-27x40-f32basis", "3x4-odd", (27, 40), terms=ONE_TERM, basis_dtype="float32"),
    case("cam-27x40-burgers", "3x4-odd", (27, 40), terms=TWO_TERMS, **BURGERS),
    case("cam-27x40-upwind-first-T5", "3x4-odd", (27, 40), terms=ONE_TERM, **UPWIND),
    case("cam-27x40-exact-burgers", "3x4-odd", (27, 40), terms=TWO_TERMS, exact=True, **BURGERS),  # both planes from the fp64 voxel
]
PLAN = {c["id"]: c for c in PLAN_CASES}
GRAPH_CASE = "cam-27x40-two"
REG_CASES = ["cam-27x40-two", "cam-27x40-burgers"]
FLOW_REG = {"kind": "divergence", "weight": 0.05, "eps": 1e-3, "s": 1.0}

# Products on sensors with both sides even, for the reason given in tests/_basis_cases.HVP_CASES (the principal point then lies between pixels)
HVP_CASES = [
    case("hvp-cam-68x90-two", "overlap", (68, 90), terms=TWO_TERMS),
    case("hvp-cam-20x32-burgers", "3x4-odd", (20, 32), terms=TWO_TERMS, **BURGERS),
    # an exact plan (the fused terms take both planes of the fp64 motion) on an fp32 basis, without and with the voxel chain
    case("hvp-cam-20x32-exact-f32basis", "3x4-odd", (20, 32), terms=TWO_TERMS, exact=True, basis_dtype="float32"),
    case("hvp-cam-20x32-exact-burgers-f32basis", "3x4-odd", (20, 32), terms=TWO_TERMS, exact=True, basis_dtype="float32", **BURGERS),
]
HVP = {c["id"]: c for c in HVP_CASES}


def batch(size):
    return B.batch(size)


def inputs(c):
    """-> (ev, x, spec): spec in the form of tests/_depth_ref.py.  s is random within [0.6, 1.4] (multiples of 2^-10), a and b give the
    displacements above; the '-zero' case has x = 0."""
    ev = batch(c["size"])
    t_scale = float(ev[:, 2].max() - ev[:, 2].min())
    spec = geometry_spec(c["gid"], c["size"])
    calib = calib_of(c["size"])
    A, Bm = E.utils.motion_field_basis(c["size"], calib)
    if c["basis_dtype"] == "float32":  # the plan keeps what it is given: the reference takes the same numbers
        A, Bm = C.f32(A), C.f32(Bm)
    ph, pw = spec["patch_image_size"]
    rng = np.random.default_rng(600 + sum(ord(ch) for ch in c["id"]))
    s = np.round(rng.uniform(0.6, 1.4, ph * pw) * 1024.0) / 1024.0
    a = np.asarray(A_DISP) * 60.0 / calib[0] / t_scale
    b = np.asarray(B_DISP) / t_scale
    x = np.concatenate([a, b, s])
    if c["id"].endswith("-zero"):
        x = np.zeros_like(x)
    spec.update(A=A, B=Bm, calib=calib, t_scale=t_scale, terms=c["terms"], sigma=c["sigma"], omit=True, time_aware=False, T=0, scheme="burgers", t0="middle",
                round32=not c["exact"])
    spec.update(c["kw"])
    return ev, x, spec


def built_plan(c):
    key = "plan/" + c["id"]
    if key not in _BUILT:
        ev, x, spec = inputs(c)
        loss, grad, _ = _depth_ref.plan(x, ev, spec)
        _BUILT[key] = dict(ev=ev, x=x, spec=spec, loss=loss, grad=grad)
    return _BUILT[key]


def _model(spec):
    return "dense-flow-voxel" if spec["time_aware"] else "dense-flow"


def hvp_inputs(c):
    """-> (ev, x, spec, dropped): the batch without the events a cell border makes ambiguous at the motion the device holds
    (tests/_basis_cases.hvp_inputs)."""
    ev, x, spec = inputs(c)
    m = _depth_ref.device_motion(x, spec)
    directions = sorted({d for cost, _ in spec["terms"] for d in _hvp_ref.cost_directions(cost)})
    margin = _hvp_ref.border_margin(ev, m, _model(spec), spec["size"], directions)
    kept, dropped = _hvp_ref.drop_ambiguous(ev, m, _model(spec), spec["size"], directions, margin)
    return kept, x, spec, dropped


def hvp_tangents(c, x, spec):
    Ka, Kb = spec["A"].shape[0], spec["B"].shape[0]
    rng = np.random.default_rng(900 + len(c["id"]))

    def one(i):
        v = np.zeros_like(x)
        v[i] = 1.0
        return v

    ns = x.size - Ka - Kb
    return {"random": C.f32(rng.normal(size=x.shape)), "one-hot-a": one(Ka - 1), "one-hot-b": one(Ka + 1), "one-hot-s": one(Ka + Kb + (3 * ns) // 5),
            "zero": np.zeros_like(x)}


def built_hvp(c):
    key = "hvp/" + c["id"]
    if key not in _BUILT:
        ev, x, spec, dropped = hvp_inputs(c)
        out = dict(ev=ev, x=x, spec=spec, dropped=dropped, v=hvp_tangents(c, x, spec), hv={})
        for name, v in out["v"].items():
            out["loss"], out["grad"], out["hv"][name] = _depth_ref.plan(x, ev, spec, v=v)
        _BUILT[key] = out
    return _BUILT[key]


# ---- the recovery scene ------------------------------------------------------------------------------------------------------------
SCENE_SIZE = (68, 90)
SCENE_GID = "overlap"
# px over the batch at rho = 1, (columns, rows): a lateral translation, no motion along the optical axis.  Not along one image axis alone: events
# sit on integer pixels, and a flow with an exactly zero component leaves every one of them ON a cell border of that axis, where the loss has a kink
SCENE_SHIFT = (4.0, 1.5)
SCENE_LEVELS = (0.5, 1.5)  # inverse depth of the left and of the right half of the grid


def scene():
    """-> dict(ev, spec, x_true, x_start): events of point features in a scene of two depths seen by a camera that translates sideways.
    The model warps an event at x, time tau to x + tau u(x) with u = -D: a feature that rests at p when warped to the first timestamp fires
    at the x with x + tau u(x) = p, found by fixed-point iteration on the reference map (u sampled bilinearly between pixels; the map
    contracts: tau |du/dx| < 0.2).  Pixels are rounded, events off the sensor dropped, a fifth of the batch is uniform noise.  The start
    knows the camera's motion and takes the mean depth everywhere."""
    if "scene" in _BUILT:
        return _BUILT["scene"]
    import torch
    H, W = SCENE_SIZE
    spec = geometry_spec(SCENE_GID, SCENE_SIZE)
    calib = calib_of(SCENE_SIZE)
    A, Bm = E.utils.motion_field_basis(SCENE_SIZE, calib)
    ph, pw = spec["patch_image_size"]
    s = np.full((ph, pw), SCENE_LEVELS[0])
    s[:, pw // 2:] = SCENE_LEVELS[1]
    a = np.array([SCENE_SHIFT[0] / calib[0] / PERIOD, SCENE_SHIFT[1] / calib[1] / PERIOD, 0.0])
    x_true = np.concatenate([a, np.zeros(3), s.reshape(-1)])
    x_start = np.concatenate([a, np.zeros(3), np.full(ph * pw, float(np.mean(SCENE_LEVELS)))])
    spec.update(A=A, B=Bm, calib=calib, t_scale=PERIOD, terms=ONE_TERM, sigma=1.0, omit=True, time_aware=False, T=0, scheme="burgers", t0="middle", round32=True)
    with torch.no_grad():
        u = -_depth_ref.dense(torch.as_tensor(x_true), spec).numpy()  # px per second

    def sample(field, r, c):
        r, c = np.clip(r, 0.0, H - 1.0), np.clip(c, 0.0, W - 1.0)
        r0, c0 = np.minimum(np.floor(r).astype(int), H - 2), np.minimum(np.floor(c).astype(int), W - 2)
        fr, fc = r - r0, c - c0
        return ((1 - fr) * (1 - fc) * field[r0, c0] + fr * (1 - fc) * field[r0 + 1, c0] + (1 - fr) * fc * field[r0, c0 + 1] + fr * fc * field[r0 + 1, c0 + 1])

    n, n_dots, seed = 3000, 60, 5
    rng = np.random.default_rng(seed)
    n_feat = n - n // 5
    p = rng.uniform([4.0, 4.0], [H - 5.0, W - 5.0], (n_dots, 2))[rng.integers(0, n_dots, n_feat)]
    tau = rng.uniform(0.0, PERIOD, n_feat)
    xr, xc = p[:, 0].copy(), p[:, 1].copy()
    for _ in range(30):
        xr, xc = p[:, 0] - tau * sample(u[0], xr, xc), p[:, 1] - tau * sample(u[1], xr, xc)
    feat = np.stack([np.round(xr), np.round(xc), tau, np.ones(n_feat)], axis=1)
    noise = E.utils.generate_events(n // 5, H, W, 0.0, PERIOD, seed=seed + 1)
    ev = np.concatenate([feat, noise])
    ev = ev[(ev[:, 0] >= 0) & (ev[:, 0] <= H - 1) & (ev[:, 1] >= 0) & (ev[:, 1] <= W - 1)]
    ev = np.ascontiguousarray(ev[np.argsort(ev[:, 2], kind="stable")])
    spec["t_scale"] = float(ev[:, 2].max() - ev[:, 2].min())
    _BUILT["scene"] = dict(ev=ev, spec=spec, x_true=x_true, x_start=x_start)
    return _BUILT["scene"]


def scene_error(x, sc):
    """Mean end-point error of the displacement field over the batch, in px, over the pixels that hold events."""
    import torch
    with torch.no_grad():
        D = _depth_ref.dense(torch.as_tensor(np.asarray(x, dtype=np.float64)), sc["spec"]).numpy()
        Dt = _depth_ref.dense(torch.as_tensor(sc["x_true"]), sc["spec"]).numpy()
    mask = np.zeros(SCENE_SIZE, dtype=bool)
    mask[sc["ev"][:, 0].astype(int), sc["ev"][:, 1].astype(int)] = True
    return float(np.sqrt(((D - Dt) ** 2).sum(axis=0))[mask].mean() * sc["spec"]["t_scale"])
