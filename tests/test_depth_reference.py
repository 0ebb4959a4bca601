"""The fp64 reference of the depth plan (tests/_depth_ref.py) anchored to the references the project already trusts, and the host-side
properties of the feature: utils.motion_field_basis, the gauge, the header and its ctypes mirror, the case table's conditions.  No GPU.

Anchors, at the 1e-10 the project anchors its references with:
  * s = 1 and no B: the map is a flow basis -- tests/_basis_ref.plan on A, loss, gradient (the a block) and product
  * one field A = -1 on component 0, a = 1: D[0] = -Q s, which IS tests/_patch_ref.patch_to_dense of the grid (s, 0)
  * gradient and H v against central differences of the reference loss (round32 False: a smooth chain)"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import event_based_optical_flow_amd as E
from event_based_optical_flow_amd import _lib

import _basis_cases as B
import _basis_ref
import _depth_cases as D
import _depth_ref
import _patch_cases as C
import _patch_ref

ANCHOR = 1e-10
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cmax_hip.h")
ENTRIES = ("cmax_depth_to_dense", "cmax_depth_to_dense_tan", "cmax_depth_to_dense_adj", "cmax_depth_to_dense_adj2", "cmax_sizeof_depth_objective",
           "cmax_depth_plan_create")


def rel_max(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


# ---- anchors -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["dense", "burgers"])
def test_unit_depth_without_rotation_is_the_basis_plan(variant):
    gid, size = "3x4-odd", (27, 40)
    kw = dict(B.BURGERS) if variant == "burgers" else {}
    ev = C.batch(size)
    t_scale = float(ev[:, 2].max() - ev[:, 2].min())
    A = E.utils.flow_basis("affine", size)
    theta = np.array(B.DISPLACEMENT["affine"]) / t_scale
    common = dict(size=size, t_scale=t_scale, terms=B.TWO_TERMS, sigma=1.0, omit=True, round32=False, time_aware=bool(kw), T=kw.get("T", 0),
                  scheme=kw.get("scheme", "burgers"), t0=kw.get("t0", "middle"))
    spec = dict(D.geometry_spec(gid, size), A=A, B=np.zeros((0, 2) + size), **common)
    ns = int(np.prod(spec["patch_image_size"]))
    x = np.concatenate([theta, np.ones(ns)])
    v = np.concatenate([C.f32(np.random.default_rng(3).normal(size=6)), np.zeros(ns)])
    want = _basis_ref.plan(theta, ev, dict(basis=A, **common), v=v[:6])
    got = _depth_ref.plan(x, ev, spec, v=v)
    e = (abs(got[0] - want[0]) / abs(want[0]), rel_max(got[1][:6], want[1]), rel_max(got[2][:6], want[2]))
    print(f"[depth-ref] s = 1, Kb = 0 ({variant}): rel diff to the basis reference loss {e[0]:.1e} grad {e[1]:.1e} Hv {e[2]:.1e}")
    assert np.abs(want[2]).max() > 0.0 and max(e) <= ANCHOR


@pytest.mark.parametrize("gid,size", D.LEAF_CASES, ids=[f"{g}-{s[0]}x{s[1]}" for g, s in D.LEAF_CASES])
def test_one_negative_field_is_the_patch_interpolation(gid, size):
    spec = D.geometry_spec(gid, size)
    A = np.zeros((1, 2) + tuple(size))
    A[0, 0] = -1.0
    spec.update(A=A, B=np.zeros((0, 2) + tuple(size)))
    ph, pw = spec["patch_image_size"]
    s = np.random.default_rng(5).normal(size=(ph, pw))
    got = _depth_ref.leaf(np.concatenate([[1.0], s.reshape(-1)]), spec)["D"]
    want = _patch_ref.patch_to_dense_numpy(np.stack([s, np.zeros_like(s)]), size, spec["sw"], spec["pad"])
    assert np.array_equal(got[0], want[0]) and not np.any(got[1]) and not np.any(want[1])


def _central(f, x, v, h):
    return (f(x + h * v) - f(x - h * v)) / (2.0 * h)


def test_gradient_and_product_against_central_differences():
    """On the batches of the product cases (no event within 2e-5 px of a cell border, where the gradient has a kink), with steps that move
    no pixel's displacement by more than 5e-6 px: the loss is smooth between x - h v and x + h v, the truncation error is O(h^2) and what
    remains is the rounding of a difference of gradients, eps |g| / h ~ 1e-8 of the product."""
    burgers = D.HVP["hvp-cam-20x32-burgers"]
    rng = np.random.default_rng(11)
    for name, c in (("dense", dict(burgers, id="hvp-cam-20x32-dense", kw={})), ("burgers", burgers)):
        ev, x, spec, _ = D.hvp_inputs(c)
        sp = dict(spec, round32=False)
        # in units where every unknown is O(1): a and b are ~1 / t_scale, s ~ 1
        scale = np.concatenate([np.full(6, 1.0 / sp["t_scale"]), np.ones(x.size - 6)])
        loss, grad, _ = _depth_ref.plan(x, ev, sp)
        for trial in range(2):
            v = rng.normal(size=x.size) * scale
            _, _, hv = _depth_ref.plan(x, ev, sp, v=v)
            moved = np.abs(_depth_ref.leaf(x, sp, u=v)["tan"]).max() * sp["t_scale"]  # px of displacement per unit step
            h = 5e-6 / moved
            fd_g = _central(lambda y: _depth_ref.plan(y, ev, sp)[0], x, v, h)
            fd_h = _central(lambda y: _depth_ref.plan(y, ev, sp)[1], x, v, h)
            e_g = abs(fd_g - grad @ v) / abs(grad @ v)
            e_h = rel_max(fd_h / scale, hv / scale)
            print(f"[depth-ref] central differences {name} #{trial}: step {h:.1e}, directional derivative {e_g:.1e}, H v {e_h:.1e}")
            assert e_g <= 1e-5 and e_h <= 1e-5


def test_gauge_and_canonical():
    c = D.PLAN["cam-27x40-one"]
    ev, x, spec = D.inputs(c)
    lam = 3.5
    y = np.concatenate([x[:3] * lam, x[3:6], x[6:] / lam])
    Dx, Dy = _depth_ref.leaf(x, spec)["D"], _depth_ref.leaf(y, spec)["D"]
    assert rel_max(Dy, Dx) <= 1e-14
    # the Hessian is singular along the gauge line: the tangent (a, 0, -s) at x
    t = np.concatenate([x[:3], np.zeros(3), -x[6:]])
    loss, grad, hv = _depth_ref.plan(x, ev, dict(spec, round32=False), v=t)
    _, _, hv_other = _depth_ref.plan(x, ev, dict(spec, round32=False), v=np.concatenate([x[:3], np.zeros(3), x[6:]]))
    print(f"[depth-ref] gauge: <grad, t> {grad @ t:.2e} (|grad| |t| {np.linalg.norm(grad) * np.linalg.norm(t):.2e}); t^T H t {t @ hv:.2e}")
    assert abs(grad @ t) <= 1e-10 * np.linalg.norm(grad) * np.linalg.norm(t)

    from event_based_optical_flow_amd.solver import DepthEgoMotionObjective
    obj = object.__new__(DepthEgoMotionObjective)  # `canonical` and `split` read only the shape: no handle, no GPU
    obj.Ka, obj.Kb, obj.patch_image_size, obj._nx = 3, 3, spec["patch_image_size"], x.size
    z = obj.canonical(x)
    a, b, s = obj.split(z)
    assert abs(np.linalg.norm(a) - 1.0) <= 1e-15 and np.array_equal(b, x[3:6]) and s.shape == spec["patch_image_size"]
    assert rel_max(_depth_ref.leaf(z, spec)["D"], Dx) <= 1e-14
    zt = obj.canonical(torch.as_tensor(x))
    assert np.allclose(zt.numpy(), z, rtol=1e-15, atol=0.0)


# ---- motion_field_basis ------------------------------------------------------------------------------------------------------------
def test_motion_field_basis_shapes_and_signs():
    size = (6, 9)
    H, W = size
    calib = (40.0, 50.0, 3.5, 2.0)
    A, Bm = E.utils.motion_field_basis(size, calib)
    assert A.shape == Bm.shape == (3, 2, H, W) and A.dtype == np.float64 and A.flags["C_CONTIGUOUS"]
    assert np.array_equal(Bm, E.utils.flow_basis("rotation", size, calib))
    fx, fy, cx, cy = calib
    x = (np.arange(W)[None, :] - cx) / fx + np.zeros(size)
    y = (np.arange(H)[:, None] - cy) / fy + np.zeros(size)
    # stored as -u, rows first: u_col = fx (-v_x + x v_z), u_row = fy (-v_y + y v_z)
    assert np.array_equal(A[0], np.stack([np.zeros(size), np.full(size, fx)]))
    assert np.array_equal(A[1], np.stack([np.full(size, fy), np.zeros(size)]))
    np.testing.assert_allclose(A[2], np.stack([-fy * y, -fx * x]), atol=1e-15)
    assert not np.any(np.signbit(A[A == 0.0]))
    # a camera that moves towards the scene: the field leaves the principal point (u = -A points outwards)
    assert -A[2, 1, 0, W - 1] > 0 and -A[2, 1, 0, 0] < 0 and -A[2, 0, H - 1, 0] > 0
    with pytest.raises(ValueError, match="calib"):
        E.utils.motion_field_basis(size, None)


# ---- header and binding ------------------------------------------------------------------------------------------------------------
def test_header_declares_the_new_entries():
    text = open(HEADER).read()
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _lib.SIGNATURES
        args = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text).group(1)
        n_args = 0 if args.strip() == "void" else len(args.split(","))
        assert n_args == len(_lib.SIGNATURES[name][1]), name
    assert re.search(r"#define\s+CMAX_ABI_VERSION\s+4\b", text) and _lib.ABI_VERSION == 4
    assert int(re.search(r"#define\s+CMAX_DEPTH_ADJ_CHUNK\s+(\d+)", text).group(1)) == _lib.DEPTH_ADJ_CHUNK == D.ADJ_CHUNK == 1024


def test_descriptor_mirror_matches_the_header():
    text = open(HEADER).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*cmax_depth_objective_t;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names, size = [], 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, rest = decl.split(None, 1)
        for field in rest.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", field)
            names.append(m.group(1))
            count = int(m.group(2)) if m.group(2) else 1
            width = {"int32_t": 4, "double": 8, "cmax_objective_t": ctypes.sizeof(_lib.CmaxObjective)}[ctype]
            size = (size + min(width, 8) - 1) // min(width, 8) * min(width, 8) + width * count
    assert names == [n for n, _ in _lib.CmaxDepthObjective._fields_]
    assert size == ctypes.sizeof(_lib.CmaxDepthObjective) and size % 8 == 0
    assert _lib.CmaxDepthObjective.t_scale.offset == 72 and _lib.CmaxDepthObjective.Ka.offset == 28


# ---- the case table ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(D.HVP))
def test_the_border_filter_stays_under_the_cap(cid):
    ev, x, spec, dropped = D.hvp_inputs(D.HVP[cid])
    print(f"[depth-ref] {cid}: {len(ev)} events kept, dropped share {dropped:.5f} (cap {D.DROP_CAP})")
    assert 0.0 <= dropped <= D.DROP_CAP
    assert spec["size"][0] % 2 == 0 and spec["size"][1] % 2 == 0
    if spec["time_aware"]:
        # the upwind selectors of the voxel chain take the sign of each flow component: no pixel may carry a rounding residue there
        F = _depth_ref.device_motion(x, dict(spec, time_aware=False, round32=False))
        print(f"[depth-ref] {cid}: smallest |flow component| at a pixel {np.abs(F).min():.3e} px")
        assert np.abs(F).min() > 1e-6


def test_the_table_reaches_what_it_claims():
    n = [h * w for _, (h, w) in D.LEAF_CASES]
    assert n[0] < D.ADJ_CHUNK < n[1] < 2 * D.ADJ_CHUNK and n[2] < D.ADJ_CHUNK and n[4] > 5 * D.ADJ_CHUNK and all(v % 256 for v in n)
    assert D.seam_pixels((27, 40)) == [(0, 0), (25, 23), (25, 24), (26, 39)]
    assert len(D.seam_pixels((68, 90))) == 12
    assert max(ka + kb for ka, kb in D.LEAF_K) == _lib.BASIS_MAX_K and min(kb for _, kb in D.LEAF_K) == 0
    for c in D.PLAN_CASES:
        ev, x, spec = D.inputs(c)
        assert x.size == 6 + int(np.prod(spec["patch_image_size"]))
        if not c["id"].endswith("-zero"):
            F = np.abs(_depth_ref.device_motion(x, dict(spec, time_aware=False)))
            assert 1.0 < F.max() < 40.0, (c["id"], F.max())  # a few pixels of displacement
    # cells of the 16x16-sw16x21 grid that no pixel touches exist: their column of Q is zero
    spec = D.geometry_spec("16x16-sw16x21", (66, 90))
    s = torch.zeros(spec["patch_image_size"], dtype=torch.float64, requires_grad=True)
    (col,) = torch.autograd.grad(_depth_ref.Q(s, spec).sum(), s)
    assert int((col == 0).sum()) > 0 and abs(float(col.sum()) - 66 * 90) < 1e-9  # (and Q is a convex combination: its rows sum to 1)


# ---- the recovery scene ------------------------------------------------------------------------------------------------------------
def test_recovery_scene_meets_its_criterion_on_the_reference():
    """The premise of the GPU test that runs minimize_lbfgs on these events: from the start that knows the camera's motion and takes the mean
    depth everywhere, a quasi-Newton descent on the REFERENCE loss ends lower than it started and halves the end-point error of D."""
    from scipy.optimize import minimize
    sc = D.scene()
    assert len(sc["ev"]) > 2500 and np.all(np.diff(sc["ev"][:, 2]) >= 0)
    f = lambda x: _depth_ref.plan(x, sc["ev"], sc["spec"])[:2]  # noqa: E731
    loss_true, loss_start = f(sc["x_true"])[0], f(sc["x_start"])[0]
    e_start = D.scene_error(sc["x_start"], sc)
    res = minimize(f, sc["x_start"], jac=True, method="L-BFGS-B", options={"maxiter": 60, "maxfun": 80})
    e_end = D.scene_error(res.x, sc)
    print(f"[depth-ref] recovery scene: loss {loss_start:.6g} at the start, {res.fun:.6g} at the end ({res.nit} iterations, {res.nfev} evaluations), "
          f"{loss_true:.6g} at the scene; mean end-point error {e_start:.3f} px -> {e_end:.3f} px")
    assert loss_true < loss_start
    assert res.fun < loss_start and e_end < 0.5 * e_start
