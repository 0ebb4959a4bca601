"""The case table of the flow-basis tests (tests/test_basis_reference.py on the CPU, tests/test_gpu_basis_plan.py on the GPU): the
smallest shapes that reach each branch of csrc/cmax_basis_kernels.h and of the basis plan (csrc/cmax_solver.hip).  References are
computed once per process and shared (built_*), and never modified."""
import numpy as np

import event_based_optical_flow_amd as E

import _basis_ref
import _hvp_ref
import _patch_cases as C

PERIOD = C.PERIOD
DROP_CAP = C.DROP_CAP
ADJ_CHUNK = 2048  # CMAX_BASIS_ADJ_CHUNK: elements of [2,H,W] per workgroup of k_basis_adj
# displacement over the batch, theta * t_scale, in flow_basis order: a few pixels anywhere on a 68 x 90 sensor
DISPLACEMENT = {"affine": (2.0, -1.5, 0.10, -0.06, 0.05, 0.12), "similarity": (2.0, -1.5, 0.10, 0.08)}
ONE_TERM = (("image_variance", 1.0),)                               # the fp32 adjoint branch of backward_motion
TWO_TERMS = C.YAML_HYBRID + (("image_variance", 0.5),)              # the YAML hybrid plus a second term: its fp64 branch
BURGERS = dict(time_aware=True, T=10, scheme="burgers", t0="middle")
UPWIND = dict(time_aware=True, T=5, scheme="upwind", t0="first")
LEAF_SIZES = [(20, 28), (27, 40), (68, 90)]  # 2 H W = 1120 (below a chunk), 2160 (one seam), 12240 (five seams); none a multiple of 256
LEAF_K = [1, 6, 7, 9, 64]                    # below, across and beyond the tile of four fields; the largest K
_BUILT = {}


def smooth_basis(K, size, seed):
    """[K,2,H,W] random smooth fields within [-1, 1], values exact in fp32 (a float32 and a float64 basis hold the same numbers)."""
    H, W = size
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.linspace(0.0, 1.0, H), np.linspace(0.0, 1.0, W), indexing="ij")
    a = rng.uniform(0.5, 3.0, (K, 2, 2))
    ph = rng.uniform(0.0, 2.0 * np.pi, (K, 2, 2))
    B = np.sin(a[:, :, 0, None, None] * i + ph[:, :, 0, None, None]) * np.cos(a[:, :, 1, None, None] * j + ph[:, :, 1, None, None])
    return C.f32(B)


def model_basis(model, size):
    return E.utils.flow_basis(model, size)


def seam_elements(n):
    """Flat indices of [2,H,W] for one-hot cotangents: the four corners of the first plane's image are added by the caller; here the
    first and last element and both sides of every chunk seam of the adjoint."""
    out = {0, n - 1}
    for s in range(ADJ_CHUNK, n, ADJ_CHUNK):
        out |= {s - 1, s}
    return sorted(out)


def case(cid, size, basis, disp=None, terms=ONE_TERM, exact=False, basis_dtype="float64", sigma=1.0, **kw):
    return dict(id=cid, size=tuple(size), basis=basis, disp=disp, terms=tuple(terms), exact=exact, basis_dtype=basis_dtype, sigma=sigma, kw=kw)


def _model_case(cid, model, size, **kw):
    return case(cid, size, model, DISPLACEMENT[model], **kw)


PLAN_CASES = [
    _model_case(f"{model}-{size[0]}x{size[1]}-{tname}", model, size, terms=terms)
    for model in ("affine", "similarity") for size in ((27, 40), (68, 90)) for tname, terms in (("one", ONE_TERM), ("two", TWO_TERMS))
] + [
    case("K1-27x40", (27, 40), ("smooth", 1, 11), terms=TWO_TERMS),
    case("K64-27x40-f32basis", (27, 40), ("smooth", 64, 12), terms=ONE_TERM, basis_dtype="float32"),
    case("K64-68x90", (68, 90), ("smooth", 64, 13), terms=TWO_TERMS),
    _model_case("affine-27x40-zero", "affine", (27, 40), terms=TWO_TERMS),
    _model_case("affine-68x90-exact", "affine", (68, 90), terms=TWO_TERMS, exact=True),
    _model_case("similarity-27x40-exact-one", "similarity", (27, 40), terms=ONE_TERM, exact=True),
    _model_case("similarity-27x40-burgers", "similarity", (27, 40), terms=TWO_TERMS, **BURGERS),
    _model_case("affine-27x40-upwind-first-T5", "affine", (27, 40), terms=ONE_TERM, **UPWIND),
    _model_case("similarity-27x40-exact-burgers", "similarity", (27, 40), terms=TWO_TERMS, exact=True, **BURGERS),  # both planes from the fp64 voxel
]
PLAN = {c["id"]: c for c in PLAN_CASES}
GRAPH_CASE = "affine-27x40-two"

HVP_CASES = [
    _model_case("hvp-affine-27x40-two", "affine", (27, 40), terms=TWO_TERMS),
    _model_case("hvp-similarity-68x90-one", "similarity", (68, 90), terms=ONE_TERM),
    # On a sensor with an odd side the centred coordinates are integers and both tabulated fields have a flow component that is zero at a
    # pixel in exact arithmetic (similarity, 27 x 40: 2 + 0.10 r - 0.08 c at r = -10, c = 12.5); what the fp64 sum leaves there is a
    # residue of 1e-17 whose SIGN the upwind selectors of the voxel chain take, and the second derivative jumps with it (the reference's
    # own product moves by 5e-3 when theta moves by 1e-13).  The value and the gradient are continuous there; the product is not defined.
    # With both sides even the coordinates are half-integers and neither component of the similarity field vanishes at a pixel
    # (tests/test_basis_reference.py checks that no time-aware product case sits on such a zero).
    _model_case("hvp-similarity-68x90-burgers", "similarity", (68, 90), terms=TWO_TERMS, **BURGERS),
    # an exact plan (the fused terms take both planes of the fp64 motion), without and with the voxel chain; both sides even, as above
    _model_case("hvp-similarity-20x32-exact-f32basis", "similarity", (20, 32), terms=TWO_TERMS, exact=True, basis_dtype="float32"),
    _model_case("hvp-similarity-20x32-exact-burgers", "similarity", (20, 32), terms=TWO_TERMS, exact=True, **BURGERS),
]
HVP = {c["id"]: c for c in HVP_CASES}


def batch(size):
    key = ("batch", tuple(size))
    if key not in _BUILT:
        _BUILT[key] = C.batch(tuple(size))
    return _BUILT[key]


def basis_of(c):
    b = c["basis"]
    if isinstance(b, str):
        return model_basis(b, c["size"])
    kind, K, seed = b
    assert kind == "smooth"
    return smooth_basis(K, c["size"], seed)


def inputs(c):
    """-> (ev, theta, spec): spec in the form of tests/_basis_ref.py; theta = displacement / t_scale (zero for the '-zero' case; random
    with a few pixels of displacement for the random bases)."""
    ev = batch(c["size"])
    t_scale = float(ev[:, 2].max() - ev[:, 2].min())
    B = basis_of(c)
    K = B.shape[0]
    if c["id"].endswith("-zero"):
        disp = np.zeros(K)
    elif c["disp"] is not None:
        disp = np.asarray(c["disp"], dtype=np.float64)
    else:
        disp = np.random.default_rng(500 + K).normal(0.0, 3.0 / np.sqrt(K), K)
    spec = dict(size=c["size"], basis=B, t_scale=t_scale, terms=c["terms"], sigma=c["sigma"], omit=True, time_aware=False, T=0, scheme="burgers",
                t0="middle", round32=not c["exact"])  # exact_flow: the fused terms see the fp64 field itself
    spec.update(c["kw"])
    return ev, disp / t_scale, spec


def built_plan(c):
    """-> dict(ev, theta, spec, loss, grad)."""
    key = "plan/" + c["id"]
    if key not in _BUILT:
        ev, theta, spec = inputs(c)
        loss, grad, _ = _basis_ref.plan(theta, ev, spec)
        _BUILT[key] = dict(ev=ev, theta=theta, spec=spec, loss=loss, grad=grad)
    return _BUILT[key]


def _model(spec):
    return "dense-flow-voxel" if spec["time_aware"] else "dense-flow"


def hvp_inputs(c):
    """-> (ev, theta, spec, dropped): the batch without the events within the scaled margin of a cell border at the motion the device
    holds (tests/_hvp_ref.drop_ambiguous at _hvp_ref.border_margin, as tests/_patch_cases.hvp_inputs); t_scale stays the whole batch's."""
    ev, theta, spec = inputs(c)
    m = _basis_ref.device_motion(theta, spec)
    directions = sorted({d for cost, _ in spec["terms"] for d in _hvp_ref.cost_directions(cost)})
    margin = _hvp_ref.border_margin(ev, m, _model(spec), spec["size"], directions)
    kept, dropped = _hvp_ref.drop_ambiguous(ev, m, _model(spec), spec["size"], directions, margin)
    return kept, theta, spec, dropped


def hvp_tangents(c, theta):
    rng = np.random.default_rng(900 + len(c["id"]))
    one = np.zeros_like(theta)
    one[(3 * theta.size) // 5] = 1.0
    return {"random": C.f32(rng.normal(size=theta.shape)), "one-hot": one, "zero": np.zeros_like(theta)}


def built_hvp(c):
    key = "hvp/" + c["id"]
    if key not in _BUILT:
        ev, theta, spec, dropped = hvp_inputs(c)
        out = dict(ev=ev, theta=theta, spec=spec, dropped=dropped, v=hvp_tangents(c, theta), hv={})
        for name, v in out["v"].items():
            out["loss"], out["grad"], out["hv"][name] = _basis_ref.plan(theta, ev, spec, v=v)
        _BUILT[key] = out
    return _BUILT[key]


# ---- events of a known similarity field ----------------------------------------------------------------------------------------------
SIM_SIZE = (68, 90)
SIM_TRUE = DISPLACEMENT["similarity"]  # displacement over the batch: theta_true * PERIOD


def similarity_events(size=SIM_SIZE, n=3000, disp=SIM_TRUE, n_dots=60, seed=5):
    """Events of point features that move with the similarity field u(x) = b + z (r, c) + w (-c, r) of utils.flow_basis("similarity"):
    the model warps an event at x, time t to x + (t - t_min) u(x), so a feature that rests at p when warped to the first timestamp
    fires at the x with x + tau u(x) = p, tau = t - t_min -- a 2 x 2 linear system per event.  Pixels are integers (rounded), events off
    the sensor are dropped, a fifth of the batch is uniform noise; sorted by time.  -> [n', 4] (row, column, time, polarity)."""
    H, W = size
    rng = np.random.default_rng(seed)
    b0, b1, z, w = (v / PERIOD for v in disp)
    centre = np.array([(H - 1) / 2.0, (W - 1) / 2.0])
    n_feat = n - n // 5
    p = rng.uniform([4.0, 4.0], [H - 5.0, W - 5.0], (n_dots, 2))[rng.integers(0, n_dots, n_feat)] - centre
    tau = rng.uniform(0.0, PERIOD, n_feat)
    # (I + tau A) x = p - tau b,  A = [[z, -w], [w, z]]
    a, c = 1.0 + tau * z, tau * w
    det = a * a + c * c
    q0, q1 = p[:, 0] - tau * b0, p[:, 1] - tau * b1
    x0, x1 = (a * q0 + c * q1) / det, (-c * q0 + a * q1) / det
    feat = np.stack([np.round(x0 + centre[0]), np.round(x1 + centre[1]), tau, np.ones(n_feat)], axis=1)
    noise = E.utils.generate_events(n // 5, H, W, 0.0, PERIOD, seed=seed + 1)
    ev = np.concatenate([feat, noise])
    ev = ev[(ev[:, 0] >= 0) & (ev[:, 0] <= H - 1) & (ev[:, 1] >= 0) & (ev[:, 1] <= W - 1)]
    return np.ascontiguousarray(ev[np.argsort(ev[:, 2], kind="stable")])
