"""Device-resident L-BFGS, what can be checked without a GPU: the numpy restatement of the rules (tests/_lbfgs_ref.py, the yardstick of
tests/test_gpu_lbfgs.py) against anchors that do not depend on it -- the dense BFGS inverse-Hessian update built from the same pairs,
the ring order, the minimisers SciPy's L-BFGS-B finds -- and every branch of the rule taken at least once; the ABI (struct size, symbols
declared / bound / exported, version 4); the descriptor checks, which return CMAX_EINVAL naming the field before any GPU call; the
solver classes' `optimizer.method: "device-L-BFGS"`."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.optimize

from event_based_optical_flow_amd import _lib, build, solver
from event_based_optical_flow_amd.solver import common

import _lbfgs_cases as K
import _lbfgs_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cmax_hip.h")
SYMBOLS = ("cmax_sizeof_lbfgs", "cmax_patch_plan_lbfgs", "cmax_objective_lbfgs")

# the 7-parameter quadratic of tests/test_descent_reference.py: f(x) = 1/2 x^T A x - b^T x, A symmetric positive definite
_RNG = np.random.default_rng(11)
_Q = np.linalg.qr(_RNG.normal(size=(7, 7)))[0]
A = _Q @ np.diag([0.3, 0.7, 1.1, 2.0, 3.5, 6.0, 9.0]) @ _Q.T
A = 0.5 * (A + A.T)
B = _RNG.normal(size=7)
X0 = _RNG.normal(size=7)
XSTAR = np.linalg.solve(A, B)


def quadratic(x):
    return 0.5 * x @ A @ x - B @ x, A @ x - B


def rosenbrock(x):
    return scipy.optimize.rosen(x), scipy.optimize.rosen_der(x)


def accepted_points(out):
    keep = (out["code"] == R.START) | (out["code"] == R.ACCEPTED)
    return out["trace"][:-1][keep], out["loss_history"][keep]


# ---- anchors ---------------------------------------------------------------------------------------------------------------------------
def test_direction_is_the_dense_bfgs_product_of_the_same_pairs():
    """m >= the number of accepted steps: nothing was dropped, so -H g with H the dense BFGS inverse Hessian grown from
    H0 = (s^T y / y^T y) I of the newest pair through every pair in order is the direction."""
    out = R.minimize(quadratic, X0, R.descriptor(12, history=16, gtol=0.0, max_move=50.0))
    pairs = out["state"]["pairs"]
    assert len(pairs) == out["nit"] >= 5
    s, y = pairs[-1]
    H = (s @ y) / (y @ y) * np.eye(7)
    for s, y in pairs:
        rho, eye = 1.0 / (s @ y), np.eye(7)
        H = (eye - rho * np.outer(s, y)) @ H @ (eye - rho * np.outer(y, s)) + rho * np.outer(s, s)
    g = out["state"]["ga"]
    d, want = R.two_loop(pairs, g), -H @ g
    err = np.abs(d - want).max() / np.abs(want).max()
    print(f"[lbfgs] two-loop vs dense BFGS over {len(pairs)} pairs: {err:.2e} of the largest entry")
    assert err <= 1e-12
    np.testing.assert_array_equal(out["state"]["d"], d)  # ... and it is the direction the state machine holds


@pytest.mark.parametrize("m", [1, 3])
def test_ring_order(m):
    """More than m accepts: the held pairs are the LAST m differences of the accepted points, oldest first."""
    out = R.minimize(quadratic, X0, R.descriptor(12, history=m, gtol=0.0, max_move=50.0))
    xs, _ = accepted_points(out)
    assert len(xs) - 1 == out["nit"] > m + 2 and "drop_oldest" in out["branches"]
    pairs = out["state"]["pairs"]
    assert len(pairs) == m
    for i, (s, y) in enumerate(pairs):
        j = len(xs) - 1 - m + i
        np.testing.assert_array_equal(s, xs[j + 1] - xs[j])
        np.testing.assert_array_equal(y, quadratic(xs[j + 1])[1] - quadratic(xs[j])[1])


@pytest.mark.parametrize("name", ["quadratic", "rosenbrock"])
def test_ends_where_scipys_lbfgsb_ends(name):
    """Both stop on a gradient tolerance, so neither is AT the minimiser: SciPy's own distance to the known minimiser is the
    tolerance the restatement is held to (with a floor of 1e-6, the scale of gtol 1e-6 on Hessians of order one and more)."""
    fun, x0, xstar = (quadratic, X0, XSTAR) if name == "quadratic" else (rosenbrock, np.array([-1.2, 1.0]), np.ones(2))
    want = scipy.optimize.minimize(lambda x: fun(x)[0], x0, jac=lambda x: fun(x)[1], method="L-BFGS-B")
    out = R.minimize(fun, x0, R.descriptor(200, history=8, gtol=1e-6, max_move=50.0))
    e_scipy, e_ours = np.abs(want.x - xstar).max(), np.abs(out["x"] - xstar).max()
    print(f"[lbfgs] {name}: status {R.STATUS_WORDS[out['status']]}, {out['nit']} steps / {out['nfev']} evaluations (SciPy: {want.nit} / {want.nfev}), "
          f"distance to the minimiser {e_ours:.2e} (SciPy {e_scipy:.2e}), between the two {np.abs(out['x'] - want.x).max():.2e}")
    assert want.success and out["status"] == R.CONVERGED
    assert e_ours <= max(e_scipy, 1e-6)
    _, losses = accepted_points(out)
    assert (np.diff(losses) <= 0.0).all()  # the property users rely on
    assert np.isnan(out["loss_history"][out["nfev"]:]).all() and (out["code"][out["nfev"]:] == R.IDLE).all()


# ---- every branch ------------------------------------------------------------------------------------------------------------------------
def test_reject_then_accept():
    out = R.minimize(quadratic, X0, R.descriptor(8, step0=1e3, gtol=0.0, max_move=1e4))
    assert out["code"][0] == R.START and out["code"][1] == R.REJECTED and R.ACCEPTED in out["code"]
    assert "reject" in out["branches"]
    k = int(np.argmax(out["code"] == R.ACCEPTED))
    np.testing.assert_allclose(out["alpha"][1:k + 1], out["alpha"][1] * 0.5 ** np.arange(k), rtol=1e-15)


def test_linesearch_failure_with_an_empty_history():
    out = R.minimize(quadratic, X0, R.descriptor(8, step0=1e3, max_ls=1, gtol=0.0, max_move=1e4))
    assert out["status"] == R.LINESEARCH and "linesearch" in out["branches"] and out["nit"] == 0 and out["nfev"] == 3
    np.testing.assert_array_equal(out["x"], X0)
    assert list(out["code"][:4]) == [R.START, R.REJECTED, R.REJECTED, R.IDLE]


def _scripted(desc, x0, script):
    """Feeds (L, g) pairs to the state machine whatever the points are: the rule reads nothing else."""
    st = R.start(x0, desc)
    codes = []
    for L, g in script:
        st, _ = R.transition(st, L, np.asarray(g, dtype=np.float64))
        codes.append(st["code"])
    return st, codes


def test_reset_after_max_ls_with_a_history():
    desc = R.descriptor(8, max_ls=1, gtol=0.0, max_move=10.0)
    st, codes = _scripted(desc, [1.0, 1.0], [(10.0, [1.0, 2.0]), (9.0, [0.5, 1.0]), (99.0, [0.0, 0.0]), (99.0, [0.0, 0.0]), (8.5, [0.4, 0.9])])
    assert codes == [R.START, R.ACCEPTED, R.REJECTED, R.RESET, R.ACCEPTED] and "reset" in st["branches"]
    assert st["n_iter"] == 2 and len(st["pairs"]) == 1  # the history went at the reset; the accept behind it pushed a new pair


def test_skipped_pair():
    desc = R.descriptor(4, gtol=0.0, max_move=10.0)
    st, codes = _scripted(desc, [1.0, 1.0], [(10.0, [1.0, 2.0]), (9.0, [1.0, 2.0])])  # y = 0
    assert codes == [R.START, R.ACCEPTED] and "skipped_pair" in st["branches"] and not st["pairs"] and st["n_iter"] == 1
    st, codes = _scripted(desc, [1.0, 1.0], [(10.0, [1.0, 2.0]), (9.0, [2.0, 4.0])])  # s = -alpha g, y = g: s^T y < 0
    assert "skipped_pair" in st["branches"] and not st["pairs"]


def test_nondescent_direction_clears_the_history():
    """s^T y > 0 makes H positive definite, so only rounding gets here: with H0 = 1e-300 I the product H g underflows to zero."""
    desc = R.descriptor(4, curv_eps=0.0, gtol=0.0, step0=1e-200, max_move=10.0)
    st = R.start([0.0, 0.0], desc)  # (at the origin, where a step of 1e-200 is representable)
    st, _ = R.transition(st, 10.0, np.array([-1e100, 1e-100]))  # alpha = 1e-300: s = (1e-200, 0)
    st, _ = R.transition(st, 9.0, np.array([0.0, 1e-100]))  # y = (1e100, 0): s^T y = 1e-100 > 0, y^T y = 1e200
    assert st["code"] == R.ACCEPTED and "push" in st["branches"] and "nondescent_reset" in st["branches"]
    assert not st["pairs"] and np.array_equal(st["d"], -st["ga"]) and st["gd"] < 0.0


def test_box():
    """The minimiser is far outside: the first step is clipped to the wall, the next direction points through it."""
    out = R.minimize(lambda x: (0.5 * (x - 100.0) @ (x - 100.0), x - 100.0), np.zeros(3), R.descriptor(8, step0=1e3, gtol=0.0, max_move=0.5))
    assert out["status"] == R.BOX and {"box", "clipped_alpha"} <= out["branches"] and out["nit"] == 1
    assert np.abs(out["trace"] - 0.0).max() <= 0.5
    np.testing.assert_array_equal(out["x"], np.full(3, 0.5))


def test_converged_at_the_start():
    out = R.minimize(quadratic, X0, R.descriptor(4, gtol=1e9))
    assert out["status"] == R.CONVERGED and out["nit"] == 0 and out["nfev"] == 1 and "converged_at_start" in out["branches"]
    assert list(out["code"]) == [R.START, R.IDLE, R.IDLE, R.IDLE] and np.isnan(out["loss_history"][1:]).all()
    np.testing.assert_array_equal(out["x"], X0)


def test_nonfinite_trial_is_a_reject():
    def barrier(x):  # defined for x < 1 only
        if (x >= 1.0).any():
            return np.nan, np.full_like(x, np.nan)
        return float(-np.log(1.0 - x).sum() - 3.0 * x.sum()), 1.0 / (1.0 - x) - 3.0

    out = R.minimize(barrier, np.zeros(2), R.descriptor(16, step0=8.0, gtol=1e-8, max_move=10.0))
    assert "nonfinite_trial" in out["branches"] and out["code"][1] == R.REJECTED and np.isnan(out["loss_history"][1])
    assert out["status"] == R.CONVERGED and np.abs(out["x"] - 2.0 / 3.0).max() < 1e-6
    st, codes = _scripted(R.descriptor(4, max_move=10.0), [0.0, 0.0], [(1.0, [1.0, 1.0]), (0.5, [np.inf, 1.0])])  # a finite, lower loss; one bad entry
    assert codes == [R.START, R.REJECTED] and "nonfinite_trial" in st["branches"]


def test_nonfinite_start():
    out = R.minimize(lambda x: (np.nan, np.zeros_like(x)), X0, R.descriptor(3))
    assert out["status"] == R.NONFINITE_START and out["nit"] == 0 and out["nfev"] == 1 and "nonfinite_start" in out["branches"]
    np.testing.assert_array_equal(out["x"], X0)
    assert np.isnan(out["loss_history"]).all() and list(out["code"]) == [R.START, R.IDLE, R.IDLE]
    out = R.minimize(lambda x: (1.0, np.array([0.0, np.inf])), np.zeros(2), R.descriptor(2))
    assert out["status"] == R.NONFINITE_START


def test_budget():
    out = R.minimize(rosenbrock, np.array([-1.2, 1.0]), R.descriptor(5, gtol=0.0, max_move=50.0))
    assert out["status"] == R.BUDGET and out["nfev"] == 5 and (out["code"] != R.IDLE).all()
    xs, losses = accepted_points(out)
    np.testing.assert_array_equal(out["x"], xs[-1])  # a trial that was never accepted is never returned
    assert out["fun"] == losses[-1] == losses.min()


# ---- the cases of tests/test_gpu_lbfgs.py, on the CPU -------------------------------------------------------------------------------------
EXPECT = {  # branches each case must take in fp64 over tests/_patch_ref.plan, and its status
    "1x1-m1-plain": ({"push", "drop_oldest", "reject", "skipped_pair"}, R.BUDGET),
    "3x4-m3-tv": ({"push", "drop_oldest", "reject", "skipped_pair"}, R.BUDGET),
    "3x4-m8-burgers": ({"push", "reject", "clipped_alpha", "box"}, R.BOX),
    "46x45-m3-plain": ({"push", "drop_oldest", "reject"}, R.BUDGET),
    "46x45-m8-tv": ({"push", "drop_oldest", "reject"}, R.BUDGET),
    "overshoot": ({"reject", "push", "drop_oldest"}, R.BUDGET),
    "max-ls-1": ({"reject", "linesearch"}, R.LINESEARCH),
    "small-box": ({"clipped_alpha", "box"}, R.BOX),
    "reset-3x4-m8": ({"push", "reject", "reset"}, R.BUDGET),
    "reset-46x45-m3": ({"push", "reject", "reset"}, R.BUDGET),
}


@pytest.mark.parametrize("cid", list(EXPECT))
def test_gpu_cases_take_their_branches_with_margin(cid):
    """No Armijo decision of a chosen case is closer than 1e-9 max(1, |L_a|): a thousand times the 1e-12 below which the GPU test
    calls a decision undecided."""
    c = {**K.RULE, **K.FORCED}[cid]
    _, _, x0, _ = K.inputs(c)
    out = R.minimize(K.reference_fun(c), x0, R.descriptor(**K.descriptor_kwargs(c)))
    print(f"[lbfgs] case {cid}: codes {''.join(map(str, out['code']))} status {R.STATUS_WORDS[out['status']]} nit {out['nit']} "
          f"branches {sorted(out['branches'])} smallest margin {out['margins'].min():.2e}")
    want, status = EXPECT[cid]
    assert want <= out["branches"] and out["status"] == status
    assert out["margins"].min() >= 1e-9
    assert np.abs(out["trace"] - x0).max() <= c["max_move"]
    if cid.startswith("reset"):
        first = int(np.argmax(out["code"] == R.RESET))
        assert out["code"][first - 1] == R.REJECTED and (out["code"][:first] == R.ACCEPTED).any()  # two rejects in a row behind an accept
        assert out["code"][first + 1] == R.ACCEPTED  # ... and the steepest step behind the reset is taken
    if cid == "overshoot":
        first = int(np.argmax(out["code"] == R.ACCEPTED))
        assert first >= 2 and (out["code"][1:first] == R.REJECTED).all()


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------
FIELDS = ("n_eval", "history", "max_ls", "c1", "shrink", "curv_eps", "gtol", "step0", "max_move")


def test_header_binding_and_library_agree():
    text = open(HEADER).read()
    assert re.search(r"#define CMAX_ABI_VERSION 4\b", text) and _lib.ABI_VERSION == 4  # new structs, no layout changed
    for word, code in (("BUDGET", 0), ("CONVERGED", 1), ("LINESEARCH", 2), ("BOX", 3), ("NONFINITE_START", 4)):
        assert re.search(r"#define CMAX_LBFGS_%s %d\b" % (word, code), text) and _lib.LBFGS_STATUS[code] == word and getattr(R, word) == code
    for word, code in (("START", 0), ("ACCEPTED", 1), ("REJECTED", 2), ("RESET", 3), ("IDLE", 4)):
        assert re.search(r"#define CMAX_LBFGS_CODE_%s %d\b" % (word, code), text) and _lib.LBFGS_CODES[code] == word.lower() and getattr(R, word) == code
    assert re.search(r"#define CMAX_LBFGS_MAX_HISTORY 16\b", text) and _lib.LBFGS_MAX_HISTORY == 16
    assert re.search(r"int cmax_sizeof_lbfgs\(void\);", text)
    assert re.search(r"int cmax_patch_plan_lbfgs\(cmax_patch_plan_t plan, const double \*x0_host, int with_tv, const cmax_lbfgs_t \*lbfgs,", text)
    assert re.search(r"int cmax_objective_lbfgs\(cmax_handle_t h, const cmax_objective_t \*desc_host, const double \*theta0_host, const cmax_lbfgs_t \*lbfgs,", text)
    assert [f[0] for f in _lib.CmaxLbfgs._fields_] == list(FIELDS)
    for field in FIELDS:
        assert re.search(r"\b(int32_t|double) %s;" % field, text), field
    assert [f[0] for f in _lib.CmaxLbfgsResult._fields_] == ["final_loss", "gnorm_inf", "last_alpha", "n_iter", "n_eval_used", "status"]
    assert re.search(r"8 \* \(%d \+ \(4 \+ 2 m\) nx" % _lib.LBFGS_FIXED_DOUBLES, text)  # the documented state size
    lib = _lib.load()
    assert lib.cmax_abi_version() == 4
    assert lib.cmax_sizeof_lbfgs() == ctypes.sizeof(_lib.CmaxLbfgs) == 64
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    exported = subprocess.run(["nm", "-D", "--defined-only", build.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in SYMBOLS:
        assert re.search(r" T %s$" % name, exported, re.M), name


def _good():
    return _lib.lbfgs_descriptor(n_eval=6, history=3, max_move=2.0)


def _call(lib, entry, d, res, p):
    if entry == "cmax_patch_plan_lbfgs":
        return lib.cmax_patch_plan_lbfgs(None, p, 1, d, ctypes.byref(res), p, p, p, p, None, None)
    return lib.cmax_objective_lbfgs(None, None, p, d, ctypes.byref(res), p, p, p, p, None, None)


NAN, INF = float("nan"), float("inf")
BAD = [
    ("n_eval", 0), ("n_eval", 4097), ("history", 0), ("history", 17), ("max_ls", 0), ("c1", 0.0), ("c1", 0.5), ("c1", NAN), ("shrink", 0.0),
    ("shrink", 1.0), ("shrink", NAN), ("curv_eps", -1e-3), ("curv_eps", INF), ("curv_eps", NAN), ("gtol", -1.0), ("gtol", INF), ("gtol", NAN),
    ("step0", 0.0), ("step0", INF), ("step0", NAN), ("max_move", 0.0), ("max_move", -1.0), ("max_move", INF), ("max_move", NAN),
]


@pytest.mark.parametrize("entry", ["cmax_patch_plan_lbfgs", "cmax_objective_lbfgs"])
@pytest.mark.parametrize("field,value", BAD, ids=[f"{f}={v}" for f, v in BAD])
def test_bad_descriptors_are_refused_before_any_gpu_call(entry, field, value):
    """No plan, no handle, no device: the descriptor is checked first and the message names the field."""
    lib = _lib.load()
    d = _good()
    setattr(d, field, value)
    res, buf = _lib.CmaxLbfgsResult(), np.zeros(64)
    rc = _call(lib, entry, ctypes.byref(d), res, buf.ctypes.data)
    assert rc == _lib.EINVAL == -1
    msg = lib.cmax_last_error().decode()
    assert "bad lbfgs descriptor" in msg and (field + " must") in msg, msg
    with pytest.raises(_lib.CmaxError, match="bad lbfgs descriptor"):
        _lib.check(rc)


@pytest.mark.parametrize("entry", ["cmax_patch_plan_lbfgs", "cmax_objective_lbfgs"])
def test_null_pointers_are_refused(entry):
    lib = _lib.load()
    d, res, buf = _good(), _lib.CmaxLbfgsResult(), np.zeros(64)
    assert _call(lib, entry, None, res, buf.ctypes.data) == _lib.EINVAL
    assert "null descriptor" in lib.cmax_last_error().decode()
    assert _call(lib, entry, ctypes.byref(d), res, buf.ctypes.data) == _lib.EINVAL  # (a good descriptor: the null plan / handle is next)
    assert "null pointer" in lib.cmax_last_error().decode()


def test_descriptor_defaults_and_state_size():
    d = _lib.lbfgs_descriptor()
    assert (d.n_eval, d.history, d.max_ls, d.c1, d.shrink, d.curv_eps, d.gtol, d.step0, d.max_move) == (32, 8, 10, 1e-4, 0.5, 1e-10, 1e-5, 1.0, 10.0)
    assert _lib.lbfgs_state_bytes(2, 8, 6, True) == 8 * (1112 + 20 * 2 + 12 + 3 + 14)


# ---- the solver classes ----------------------------------------------------------------------------------------------------------------
PARAMS = {"trans_x": {"min": -150, "max": 150}, "trans_y": {"min": -150, "max": 150}}
COMMON = {"motion_model": "2d-translation", "warp_direction": "first", "parameters": ["trans_x", "trans_y"], "cost": "hybrid", "outer_padding": 0,
          "cost_with_weight": {"multi_focal_normalized_gradient_magnitude": 1.0, "total_variation": 0.01},
          "iwe": {"method": "bilinear_vote", "blur_sigma": 1}}


def make(kind, method, **opt):
    opt_cfg = dict({"n_iter": 5, "method": method, "max_iter": 25, "parameters": PARAMS}, **opt)
    if kind == "pyramid":
        cfg = dict(COMMON, method="pyramidal_patch_contrast_maximization", time_aware=False,
                   patch={"initialize": "random", "scale": 3, "crop_height": 64, "crop_width": 80, "filter_type": "bilinear"})
        return solver.collections["pyramidal_patch_contrast_maximization"]((66, 90), {}, cfg, opt_cfg, {}, None)
    time_aware = kind == "time-aware"
    cfg = dict(COMMON, time_aware=time_aware, patch={"initialize": "random", "size": 16, "sliding_window": 16, "filter_type": "bilinear"})
    if time_aware:
        cfg.update(time_bin=10, flow_interpolation="burgers", t0_flow_location="middle")
        return solver.collections["time_aware_mixed_patch_contrast_maximization"]((68, 90), {}, cfg, opt_cfg, {}, None)
    return solver.MixedPatchContrastMaximization((68, 90), {}, cfg, opt_cfg, {}, None)


def test_check_opt_method():
    common.check_opt_method("device-L-BFGS")
    assert common.DEVICE_QUASI_NEWTON == ["device-L-BFGS"] and common.DESCENT_OPTIMIZERS == ["SGD", "Adam"]
    with pytest.raises(NotImplementedError) as e:
        common.check_opt_method("LBFGS")  # torch.optim's name stays refused
    assert str(common.DESCENT_OPTIMIZERS) in str(e.value) and "device-L-BFGS" in str(e.value)


@pytest.mark.parametrize("kind", ["pyramid", "mixed", "time-aware"])
def test_solver_classes_take_the_method(kind):
    assert make(kind, "device-L-BFGS").opt_method == "device-L-BFGS"
    assert make(kind, "device-L-BFGS", lbfgs={"history": 4, "max_move": 3.0}).opt_config["lbfgs"] == {"history": 4, "max_move": 3.0}
    with pytest.raises(KeyError, match="lr"):
        make(kind, "device-L-BFGS", lbfgs={"lr": 0.1})
