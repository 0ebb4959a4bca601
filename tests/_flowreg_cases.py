"""The case table of the flow-regulariser tests (tests/test_flowreg_reference.py on the CPU, tests/test_gpu_flow_regularizer.py on the
GPU): the smallest shapes that reach each seam of the 8 x 32 tiles of csrc/cmax_flowreg_kernels.h, and the plans the term rides on.
References are computed once per process and shared (built_*), and never modified."""
import numpy as np
import torch

from event_based_optical_flow_amd import solver

import _basis_cases as B
import _flowreg_ref as R
import _hvp_ref
import _mixed_ref
import _nearest_cases as N
import _patch_cases as C

TILE = (8, 32)
# a single pixel of Omega; one row / one column of Omega; exactly one tile; one past each seam; 3 x 3 tiles; no multiple of anything
SHAPES = [(3, 3), (3, 40), (10, 3), (8, 32), (9, 33), (17, 65), (37, 53)]
EPS = [0.0, 1e-3, 1.0]
S = [1.0, 0.5]
FIELDS = ("random", "linear", "zero")
AMPLITUDE = 3.0
SEEDS = (0, 1, 2)
# With a single pixel of Omega nothing averages out: where eps << |u| and the two signs of sigma give arguments of opposite sign, the
# area product is a sum psi'(u+) + psi'(u-) of +-1 that cancels seven digits, and the fp64 reference itself is 1e-10 of the largest entry
# away from the same formulas in extended precision (seeds 2, 3 and 5; tests/_flowreg_ref.own_error).  A reference cannot gate below its
# own error: the seeds of a shape are the first three at which that error is below REFERENCE_ERROR_CAP, a tenth of the fp64 gate.
SEEDS_OF = {(3, 3): (0, 1, 4)}
REFERENCE_ERROR_CAP = 1e-11
LINEAR_M = np.array([[0.25, -0.125], [0.0625, -0.5]])  # tr = -0.25; det(I - sM) - 1 = 0.132... (s = 1), 0.0957... (s = 1/2): exact in fp32
LINEAR_X0 = (1.5, 2.25)


def field(name, size, seed=0):
    """[2,H,W] fp64 with values exact in fp32, so a float32 and a float64 tensor hold the same numbers."""
    if name == "random":
        return C.f32(np.random.default_rng(40 + 1000 * seed + 17 * size[0] + size[1]).normal(0.0, AMPLITUDE, (2,) + tuple(size)))
    if name == "linear":
        return R.linear_field(LINEAR_M, LINEAR_X0, size)
    assert name == "zero", name
    return np.zeros((2,) + tuple(size))


def tangent(size, seed=0):
    return C.f32(np.random.default_rng(90 + 1000 * seed + 17 * size[0] + size[1]).normal(size=(2,) + tuple(size)))


def leaf_cases(size):
    """Every (field name, seed, kind, eps, s) of one shape: the divergence does not depend on s, so it takes s = 1 only."""
    out = []
    for name in FIELDS:
        for seed in (SEEDS_OF.get(tuple(size), SEEDS) if name == "random" else (0,)):
            for kind in R.KINDS:
                for eps in EPS:
                    for s in (S if kind == "area" else S[:1]):
                        out.append((name, seed, kind, eps, s))
    return out


def seam_pixels(size):
    """Pixels on either side of every tile seam, the corners and the ring next to the border (where Omega ends)."""
    H, W = size
    rows = sorted({0, 1, H - 2, H - 1} | {r for k in range(TILE[0], H, TILE[0]) for r in (k - 1, k)})
    cols = sorted({0, 1, W - 2, W - 1} | {c for k in range(TILE[1], W, TILE[1]) for c in (k - 1, k)})
    return [(r, c) for r in rows for c in cols]


# ---- plans ---------------------------------------------------------------------------------------------------------------------------------
# eps >= 1e-3 on every plan: patch-interpolated flows have border strips where the derivatives are zero in exact arithmetic
REGS = {
    "divergence": dict(kind="divergence", weight=0.5, eps=1e-3, s=1.0),
    "area": dict(kind="area", weight=0.25, eps=1e-2, s=1.0),
    "area-half": dict(kind="area", weight=-0.5, eps=1e-3, s=0.5),
}
# a time-aware upwind plan on the 68 x 90 sensor, in the form of a row of tests/_nearest_cases.PLAN_CASES (which has Burgers only)
UPWIND_ROW = dict(gid="overlap", size=(68, 90), motion="random", kw=dict(time_aware=True, T=5, scheme="upwind", t0="first"))
# (id, row of N.PLAN_CASES or "upwind", filter, regulariser)
PATCH_PLANS = [
    ("bilinear-div", "odd-plain", "bilinear", "divergence"),
    ("bilinear-area", "odd-plain", "bilinear", "area"),
    ("nearest-area", "odd-plain", "nearest", "area-half"),
    ("burgers-area", "burgers", "bilinear", "area"),           # the 68 x 90 sensor
    ("upwind-div", "upwind", "bilinear", "divergence"),
    ("exact-area", "plain-exact", "bilinear", "area"),         # exact_flow
    # exact_flow behind the voxel chain, and the nearest filter with the chain, with exact_flow, with both
    ("burgers-exact-area", "burgers-exact", "bilinear", "area"),
    ("nearest-burgers-area", "burgers", "nearest", "area-half"),
    ("nearest-exact-area", "plain-exact", "nearest", "area-half"),
    ("nearest-burgers-exact-area", "burgers-exact", "nearest", "area-half"),
]
# (id, B.HVP row, regulariser)
BASIS_PLANS = [
    ("affine-area", "hvp-affine-27x40-two", "area"),                   # K = 6
    ("similarity-div", "hvp-similarity-68x90-one", "divergence"),      # K = 4, one term: the accumulate path only because of the term
    ("similarity-burgers-area", "hvp-similarity-68x90-burgers", "area-half"),
    ("similarity-exact-div", "hvp-similarity-20x32-exact-f32basis", "divergence"),            # exact_flow, an fp32 basis
    ("similarity-exact-burgers-area", "hvp-similarity-20x32-exact-burgers", "area-half"),     # exact_flow behind the voxel chain
]
GRAPH_PLAN = "affine-area"
_BUILT = {}


def patch_map(spec):
    ph, pw = spec["patch_image_size"]
    return lambda x: _mixed_ref.patch_to_dense(x.reshape(2, ph, pw), spec["size"], spec["sw"], spec["pad"], spec.get("filter", "bilinear"))


def basis_map(spec):
    basis = torch.as_tensor(np.ascontiguousarray(spec["basis"], dtype=np.float64))
    return lambda theta: torch.einsum("k,kchw->chw", theta.reshape(-1), basis)


def _with_term(b, x, dense_of, reg, vs):
    """The plan's reference plus weight * R(t_scale * map x): loss, gradient and one product per tangent."""
    out = dict(b, reg=reg, x=x, hv={})
    for name, v in vs.items():
        r_loss, r_grad, r_hv = R.plan_term(x, dense_of, reg, b["spec"]["t_scale"], v=v)
        out["hv"][name] = b_hv(b, name) + r_hv
    out["reg_loss"], out["reg_grad"] = r_loss, r_grad
    out["loss"], out["grad"] = b["loss"] + r_loss, b["grad"] + r_grad
    return out


def b_hv(b, name):
    return b["hv"][name] if isinstance(b["hv"], dict) else b["hv"]


def _built_row(c, cid, filter_type):
    """tests/_nearest_cases.built for a row that is not in its table: the batch without the events a cell border makes ambiguous at the
    motion the device holds, the reference plan and one product."""
    pis = N.GEOMETRY[c["gid"]]["patch_image_size"]
    x = C.patch_motion(c["motion"], pis, 500 + sum(ord(ch) for ch in cid))
    ev = C.batch(c["size"])
    spec = C.spec_of(c["gid"], c["size"], t_scale=float(ev[:, 2].max() - ev[:, 2].min()), **c["kw"])
    spec.update(filter=filter_type, round32=True)
    model = "dense-flow-voxel" if spec["time_aware"] else "dense-flow"
    m = _mixed_ref.device_motion(x, spec)
    directions = sorted({d for cost, _ in spec["terms"] for d in _hvp_ref.cost_directions(cost)})
    margin = _hvp_ref.border_margin(ev, m, model, spec["size"], directions)
    ev, dropped = _hvp_ref.drop_ambiguous(ev, m, model, spec["size"], directions, margin)
    v = C.f32(np.random.default_rng(77 + len(cid)).normal(size=x.shape))
    loss, grad, hv = _mixed_ref.plan(x, ev, spec, v=v)
    return dict(ev=ev, x=x, v=v, spec=spec, exact_flow=False, dropped=dropped, loss=loss, grad=grad, hv=hv)


def built_patch(pid):
    if pid not in _BUILT:
        _, row, filt, reg = next(p for p in PATCH_PLANS if p[0] == pid)
        b = _built_row(UPWIND_ROW, "flowreg-upwind", filt) if row == "upwind" else N.built(row, filt)
        _BUILT[pid] = _with_term(b, b["x"], patch_map(b["spec"]), REGS[reg], {"random": b["v"]})
    return _BUILT[pid]


def built_basis(pid):
    if pid not in _BUILT:
        _, row, reg = next(p for p in BASIS_PLANS if p[0] == pid)
        b = B.built_hvp(B.HVP[row])
        vs = {k: v for k, v in b["v"].items() if k != "zero"}
        _BUILT[pid] = dict(_with_term(b, b["theta"], basis_map(b["spec"]), REGS[reg], vs), case=B.HVP[row], v=vs)
    return _BUILT[pid]


# ---- the solver classes with the key solver.flow_regularizer ---------------------------------------------------------------------------
PARAMS = {"trans_x": {"min": -150, "max": 150}, "trans_y": {"min": -150, "max": 150}}
SOLVER_COMMON = {"motion_model": "2d-translation", "warp_direction": "first", "parameters": ["trans_x", "trans_y"], "cost": "image_variance", "outer_padding": 0,
          "iwe": {"method": "bilinear_vote", "blur_sigma": 0}}
SOLVER_OPT = {"n_iter": 5, "method": "Adam", "max_iter": 25, "parameters": PARAMS}
REG = {"kind": "area", "weight": 0.1, "eps": 1e-3}


def make_solver(kind, reg, **more):
    """A solver class with (or without) the key solver.flow_regularizer; nothing here touches a device."""
    extra = dict(more)
    if reg is not None:
        extra["flow_regularizer"] = dict(reg)
    if kind == "pyramid":
        cfg = dict(SOLVER_COMMON, method="pyramidal_patch_contrast_maximization", time_aware=False,
                   patch=dict(initialize="zero", scale=3, crop_height=64, crop_width=80, filter_type="bilinear"), **extra)
        return solver.collections["pyramidal_patch_contrast_maximization"]((66, 90), {}, cfg, dict(SOLVER_OPT), {}, None)
    time_aware = kind == "time-aware"
    cfg = dict(SOLVER_COMMON, time_aware=time_aware, patch=dict(initialize="random", size=16, sliding_window=16, filter_type="bilinear"), **extra)
    if time_aware:
        cfg.update(time_bin=10, flow_interpolation="burgers", t0_flow_location="middle")
        return solver.collections["time_aware_mixed_patch_contrast_maximization"]((68, 90), {}, cfg, dict(SOLVER_OPT), {}, None)
    return solver.MixedPatchContrastMaximization((68, 90), {}, cfg, dict(SOLVER_OPT), {}, None)
