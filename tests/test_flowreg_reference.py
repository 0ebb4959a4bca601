"""The flow regularisers without a GPU: tests/_flowreg_ref.py (the fp64 restatement the device is held to) anchored on the closed form of
tabulated linear fields and on central finite differences; the host side of the new entries -- header, ctypes signatures, struct size,
ABI version -- and the argument validation of the Python entries, which runs before anything needs a device; and the condition under
which the eps = 0 rows of the case table are well posed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from event_based_optical_flow_amd import _lib
from event_based_optical_flow_amd import functional as F
from event_based_optical_flow_amd import solver
from event_based_optical_flow_amd.solver import common

import _flowreg_cases as K
import _flowreg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the closed form --------------------------------------------------------------------------------------------------------------------
MATRICES = {
    "table": K.LINEAR_M,
    "zoom": np.array([[-0.3, 0.0], [0.0, -0.3]]),            # a sink: the collapse the term is there for
    "rotation": np.array([[0.0, -0.4], [0.4, 0.0]]),          # divergence-free, but the area grows: A = 1 + s^2 w^2
    "shear": np.array([[0.0, 0.7], [0.0, 0.0]]),              # divergence-free and area-preserving: R = 0 for both kinds
    "singular": np.array([[1.0, 0.0], [0.0, 0.5]]),           # I - M is singular at s = 1: the warp flattens a cell, A(+1) = 0
}


@pytest.mark.parametrize("name", list(MATRICES))
def test_linear_fields_reach_the_closed_form(name):
    M = MATRICES[name]
    worst = 0.0
    for size in ((3, 3), (9, 33), (37, 53)):
        Fl = torch.as_tensor(R.linear_field(M, K.LINEAR_X0, size))
        a, b, c, d = R.derivatives(Fl)
        e_tr = float((a + d - np.trace(M)).abs().max())
        e_det = max(float((1.0 - sg * (a + d) + sg * sg * (a * d - b * c) - np.linalg.det(np.eye(2) - sg * M)).abs().max()) for sg in (1.0, -0.5))
        assert e_tr <= 1e-13 and e_det <= 1e-13, (name, size, e_tr, e_det)  # (the differences of a tabulated field: rounding only)
        for kind in R.KINDS:
            for eps in K.EPS:
                for s in K.S:
                    got, want = float(R.value(Fl, kind, eps, s)), R.closed_form(M, kind, eps, s)
                    worst = max(worst, abs(got - want))
                    assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (name, size, kind, eps, s, got, want)
    print(f"[flowreg] closed form {name}: worst |R - closed form| {worst:.1e}")
    if name == "shear":
        assert R.closed_form(M, "divergence") == 0.0 and R.closed_form(M, "area") == 0.0
    if name == "singular":
        assert abs(np.linalg.det(np.eye(2) - M)) == 0.0 and R.closed_form(M, "area", 0.0, 1.0) == pytest.approx(0.5 * (1.0 + 2.0))
    if name == "rotation":
        assert R.closed_form(M, "divergence") == 0.0 and R.closed_form(M, "area", 0.0, 1.0) == pytest.approx(0.16)


# ---- 2. finite differences -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("eps", [1e-3, 1.0])
def test_gradient_and_product_against_central_differences(kind, eps):
    """Directional derivatives of the value and of the gradient along a random tangent, central differences with steps that balance
    truncation (h^2) against rounding (1e-16 / h): agreement to 1e-6 of the larger side."""
    size, s = (9, 33), 0.5
    F0, dF = K.field("random", size), K.tangent(size)
    _, g = R.value_grad(F0, kind, eps, s)
    hv = R.product(F0, dF, kind, eps, s)
    h = 1e-5 * min(1.0, eps * 100.0)  # psi bends on the scale of eps
    vp, gp = R.value_grad(F0 + h * dF, kind, eps, s)
    vm, gm = R.value_grad(F0 - h * dF, kind, eps, s)
    d_val, d_grad = (vp - vm) / (2.0 * h), (gp - gm) / (2.0 * h)
    e_g = abs(d_val - float((g * dF).sum())) / abs(d_val)
    e_h = float(np.abs(d_grad - hv).max() / np.abs(hv).max())
    print(f"[flowreg] finite differences {kind} eps {eps}: <g, dF> {e_g:.1e}, H dF {e_h:.1e}")
    assert e_g <= 1e-6 and e_h <= 1e-6
    # the Hessian is symmetric: <w, H v> = <v, H w>
    w = K.tangent(size, seed=1)
    lhs, rhs = float((w * hv).sum()), float((dF * R.product(F0, w, kind, eps, s)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1e-300)


def test_second_order_term_at_eps_zero():
    """psi'' = 0: the divergence product is exactly zero, the area product is not (psi' acts on the constant Hessian of A) and equals
    the difference quotient of the gradient wherever no sign flips."""
    size = (9, 33)
    F0, dF = K.field("random", size), K.tangent(size)
    assert not np.any(R.product(F0, dF, "divergence", 0.0))
    hv = R.product(F0, dF, "area", 0.0, 1.0)
    assert np.any(hv)
    h = 1e-7  # far below min |u| / |du|: no argument changes its sign
    assert R.min_abs_argument(F0, "area", 1.0) > 1e-4
    gp, gm = R.value_grad(F0 + h * dF, "area", 0.0, 1.0)[1], R.value_grad(F0 - h * dF, "area", 0.0, 1.0)[1]
    assert np.abs((gp - gm) / (2.0 * h) - hv).max() <= 1e-6 * np.abs(hv).max()
    # psi'(0) = 0: the zero field has a zero gradient for both kinds
    for kind in R.KINDS:
        val, g = R.value_grad(np.zeros((2,) + size), kind, 0.0)
        assert val == 0.0 and not np.any(g)


def test_gradient_lives_on_the_whole_image():
    """dR/d(a,b,c,d) are zero outside Omega, their transposed differences are not: border pixels receive a gradient."""
    size = (9, 33)
    _, g = R.value_grad(K.field("random", size), "area", 1e-3)
    assert np.any(g[:, 0, 1:-1]) and np.any(g[:, -1, 1:-1]) and np.any(g[:, 1:-1, 0]) and np.any(g[:, 1:-1, -1])
    assert not np.any(g[:, 0, 0]) and not np.any(g[:, -1, -1])  # (a corner is no neighbour of Omega along an axis)


# ---- 3. the condition of the eps = 0 rows ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", K.SHAPES, ids=[f"{h}x{w}" for h, w in K.SHAPES])
def test_eps_zero_rows_are_away_from_the_kink(size):
    """A condition, not a measurement: below 1e-6 the sign of an argument may legitimately differ between two correct summation orders
    (and between the fp64 arithmetic of the device and of the reference).  The fields are exact in fp32, so the condition covers the
    float32 rows too.  The zero field sits ON the kink by construction: psi'(0) = 0 there in both implementations, exactly."""
    worst = np.inf
    for name, seed, kind, eps, s in K.leaf_cases(size):
        if eps != 0.0 or name == "zero":
            continue
        m = R.min_abs_argument(K.field(name, size, seed), kind, s)
        worst = min(worst, m)
        assert m >= 1e-6, (size, name, seed, kind, s, m)
    print(f"[flowreg] eps = 0 rows at {size}: min over Omega of |u| >= {worst:.1e}")


@pytest.mark.parametrize("size", K.SHAPES, ids=[f"{h}x{w}" for h, w in K.SHAPES])
def test_reference_is_ten_times_closer_to_the_formulas_than_the_gate(size):
    """Also a condition: the autograd reference against the same formulas in extended precision (tests/_flowreg_ref.extended, derivatives
    written out by hand -- a second, independent statement), on every row of the table.  The fp64 gate of the device is 1e-10."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        print("[flowreg] long double is double here: the reference's own error is not measured")
        return
    dF = K.tangent(size)
    worst = [0.0, 0.0, 0.0]
    for name, seed, kind, eps, s in K.leaf_cases(size):
        e = R.own_error(K.field(name, size, seed), dF, kind, eps, s)
        worst = [max(a, b) for a, b in zip(worst, e)]
        assert max(e) <= K.REFERENCE_ERROR_CAP, (size, name, seed, kind, eps, s, e)
    print(f"[flowreg] reference vs extended precision at {size}: value {worst[0]:.0e} gradient {worst[1]:.0e} product {worst[2]:.0e}")
    if tuple(size) == (3, 3):  # why this shape has seeds of its own
        assert R.own_error(K.field("random", size, 2), dF, "area", 1e-3, 0.5)[2] > K.REFERENCE_ERROR_CAP


def test_the_table_reaches_what_it_claims():
    th, tw = K.TILE
    assert (3, 3) in K.SHAPES and (th, tw) in K.SHAPES and (th + 1, tw + 1) in K.SHAPES
    assert any(h > 2 * th and w > 2 * tw for h, w in K.SHAPES)  # an inner tile, with neighbours on every side
    assert {0.0, 1e-3, 1.0} == set(K.EPS) and {1.0, 0.5} == set(K.S)
    pix = K.seam_pixels((17, 65))
    assert (7, 31) in pix and (8, 32) in pix and (16, 64) in pix and (0, 0) in pix
    assert all(r["eps"] >= 1e-3 for r in K.REGS.values())  # plans: border strips of a patch flow have zero derivatives
    kinds = {K.REGS[p[-1]]["kind"] for p in K.PATCH_PLANS} | {K.REGS[p[-1]]["kind"] for p in K.BASIS_PLANS}
    assert kinds == set(R.KINDS)


# ---- 4. header, binding, ABI ---------------------------------------------------------------------------------------------------------------
def _header():
    with open(os.path.join(ROOT, "include", "cmax_hip.h")) as f:
        return f.read()


def test_header_binding_and_abi_agree():
    text = _header()
    assert re.search(r"#define CMAX_ABI_VERSION 4\b", text) and _lib.ABI_VERSION == 4
    for name, code in (("NONE", 0), ("DIVERGENCE", 1), ("AREA", 2)):
        assert re.search(rf"#define CMAX_FLOWREG_{name} {code}\b", text)
    assert (_lib.FLOWREG_NONE, _lib.FLOWREG_DIVERGENCE, _lib.FLOWREG_AREA) == (0, 1, 2)
    assert _lib.FLOWREG_CODES == {"divergence": 1, "area": 2}
    for name in ("cmax_sizeof_flow_regularizer", "cmax_flow_regularizer", "cmax_flow_regularizer_tan", "cmax_patch_plan_set_flow_regularizer"):
        m = re.search(rf"\bint {name}\(([^;]*)\);", text)
        assert m, name
        args = [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]
        res, argtypes = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(argtypes) == len(args), (name, args)
    # the struct: int32 kind, int32 reserved, double weight, eps, s
    m = re.search(r"typedef struct \{([^}]*)\} cmax_flow_regularizer_t;", text)
    fields = re.findall(r"(int32_t|double)\s+(\w+);", m.group(1))
    assert fields == [("int32_t", "kind"), ("int32_t", "reserved"), ("double", "weight"), ("double", "eps"), ("double", "s")]
    assert [n for n, _ in _lib.CmaxFlowRegularizer._fields_] == [n for _, n in fields]
    assert ctypes.sizeof(_lib.CmaxFlowRegularizer) == 32
    lib = _lib.load()  # (loading needs no device; a layout mismatch raises here)
    assert lib.cmax_sizeof_flow_regularizer() == 32 and lib.cmax_abi_version() == 4


def test_the_library_refuses_bad_parameters_before_any_launch():
    """The checks of the leaf entries come before the first HIP call: they answer CMAX_EINVAL on a machine without a device."""
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    ptr = ctypes.addressof(buf)

    def call(H=5, W=5, dtype=_lib.F64, **kw):
        d = _lib.CmaxFlowRegularizer()
        d.kind, d.weight, d.eps, d.s = kw.get("kind", 2), 1.0, kw.get("eps", 0.0), kw.get("s", 1.0)
        rc = lib.cmax_flow_regularizer(ptr, dtype, H, W, ctypes.byref(d), ptr, ptr, None)
        rc_tan = lib.cmax_flow_regularizer_tan(ptr, ptr, dtype, H, W, ctypes.byref(d), ptr, None)
        return rc, rc_tan

    for bad in (dict(H=2), dict(W=2), dict(eps=-1e-9), dict(s=0.0), dict(s=-1.0), dict(kind=0), dict(kind=3), dict(eps=float("nan")),
                dict(s=float("inf")), dict(eps=float("inf")), dict(dtype=2)):
        assert call(**bad) == (_lib.EINVAL, _lib.EINVAL), bad
    assert lib.cmax_patch_plan_set_flow_regularizer(None, None) == _lib.EINVAL


# ---- 5. the Python entries -----------------------------------------------------------------------------------------------------------------
def test_python_entries_validate_without_a_device():
    flow = torch.zeros(2, 5, 6, dtype=torch.float64)
    with pytest.raises(ValueError, match="kind"):
        F.flow_regularizer(flow, "curl")
    with pytest.raises(ValueError, match="kind"):
        F.flow_regularizer(flow, 0)
    with pytest.raises(ValueError, match="eps"):
        F.flow_regularizer(flow, "area", eps=-1.0)
    with pytest.raises(ValueError, match="s must be > 0"):
        F.flow_regularizer(flow, "area", s=0.0)
    with pytest.raises(ValueError, match="finite"):
        F.flow_regularizer(flow, "divergence", eps=float("nan"))
    with pytest.raises(ValueError, match=r"\[2, H, W\]"):
        F.flow_regularizer(torch.zeros(3, 5, 6), "area")
    with pytest.raises(ValueError, match="at least 3"):
        F.flow_regularizer(torch.zeros(2, 2, 6), "area")
    with pytest.raises(TypeError, match="float32/float64"):
        F.flow_regularizer(torch.zeros(2, 5, 6, dtype=torch.float16), "area")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="needs an AMD GPU"):  # everything else was in order: the device is asked for last
            F.flow_regularizer(flow, "area", eps=1e-3, s=0.5)
    d = _lib.flow_regularizer_from_config({"kind": "area", "weight": 0.25, "eps": 1e-3, "s": 0.5})
    assert (d.kind, d.reserved, d.weight, d.eps, d.s) == (2, 0, 0.25, 1e-3, 0.5)
    d = _lib.flow_regularizer_from_config({"kind": "divergence"})
    assert (d.kind, d.weight, d.eps, d.s) == (1, 1.0, 0.0, 1.0)
    with pytest.raises(ValueError, match="'kind'"):
        _lib.flow_regularizer_from_config({"weight": 1.0})
    with pytest.raises(ValueError, match="'kind'"):
        _lib.flow_regularizer_from_config({"kind": "area", "epsilon": 1.0})
    with pytest.raises(ValueError, match="finite"):
        _lib.flow_regularizer_from_config({"kind": "area", "weight": float("inf")})


make_solver, REG, COMMON, OPT_CFG = K.make_solver, K.REG, K.SOLVER_COMMON, K.SOLVER_OPT


@pytest.mark.parametrize("kind", ["pyramid", "mixed", "time-aware"])
def test_solver_classes_read_the_key(kind):
    assert make_solver(kind, None).flow_regularizer is None  # absent: what the objective's constructor takes as "no such term"
    assert make_solver(kind, REG).flow_regularizer == REG
    with pytest.raises(ValueError, match="kind"):
        make_solver(kind, {"kind": "curl"})
    with pytest.raises(ValueError, match="eps"):
        make_solver(kind, dict(REG, eps=-1.0))
    with pytest.raises(ValueError, match="'kind'"):
        make_solver(kind, {"weight": 1.0})


def test_scale_later_and_the_key_exclude_each_other():
    assert common.flow_regularizer_config({}) is None and common.flow_regularizer_config({}, scale_later=True) is None
    assert common.flow_regularizer_config({"flow_regularizer": REG}) == REG
    with pytest.raises(NotImplementedError, match="scale_later"):
        common.flow_regularizer_config({"flow_regularizer": REG}, scale_later=True)
    cfg = dict(COMMON, method="pyramidal_patch_contrast_maximization", time_aware=True, time_bin=10, flow_interpolation="burgers", t0_flow_location="middle",
               scale_later=True, flow_regularizer=dict(REG), patch=dict(initialize="zero", scale=3, crop_height=64, crop_width=80, filter_type="bilinear"))
    with pytest.raises(NotImplementedError, match="divided by its maximum"):
        solver.collections["pyramidal_patch_contrast_maximization"]((66, 90), {}, cfg, dict(OPT_CFG), {}, None)
