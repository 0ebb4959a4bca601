"""Device-resident SGD / Adam, what can be checked without a GPU: the numpy restatement of the update rule (tests/_descent_ref.py, the
yardstick of tests/test_gpu_descent.py) IS torch.optim.SGD / torch.optim.Adam under StepLR -- the optimisers SolverBase.run_torch
calls (src/solver/base.py:840-881); the ABI (struct size, symbols declared / bound / exported, version 4); the descriptor checks, which
return CMAX_EINVAL with the reason before any GPU call; the solver classes' `optimizer.method`."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from event_based_optical_flow_amd import _lib, build, solver

import _descent_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cmax_hip.h")
SYMBOLS = ("cmax_sizeof_descent", "cmax_patch_plan_descend", "cmax_objective_descend")

# a fixed 7-parameter quadratic: f(x) = 1/2 x^T A x - b^T x, A symmetric positive definite with a spread spectrum
_RNG = np.random.default_rng(11)
_Q = np.linalg.qr(_RNG.normal(size=(7, 7)))[0]
A = _Q @ np.diag([0.3, 0.7, 1.1, 2.0, 3.5, 6.0, 9.0]) @ _Q.T
A = 0.5 * (A + A.T)
B = _RNG.normal(size=7)
X0 = _RNG.normal(size=7)
N_STEPS = 8


def torch_trajectory(make_optimizer):
    x = torch.tensor(X0, dtype=torch.float64, requires_grad=True)
    At, bt = torch.tensor(A), torch.tensor(B)
    opt = make_optimizer([x])
    sched = torch.optim.lr_scheduler.StepLR(opt, 2, 0.5)
    xs = [x.detach().numpy().copy()]
    for _ in range(N_STEPS):
        opt.zero_grad()
        loss = 0.5 * x @ At @ x - bt @ x
        loss.backward()
        opt.step()
        sched.step()
        xs.append(x.detach().numpy().copy())
    return np.stack(xs)


def ref_trajectory(opt):
    state, x, xs = {}, X0.copy(), [X0.copy()]
    for it in range(N_STEPS):
        x = _descent_ref.step(state, x, A @ x - B, it, opt)
        xs.append(x.copy())
    return np.stack(xs)


@pytest.mark.parametrize("name", ["sgd", "sgd-momentum", "adam"])
def test_the_rule_is_torch_optim_under_steplr(name):
    if name == "adam":
        got = ref_trajectory(_descent_ref.options("Adam", lr=0.05, lr_step=2, lr_decay=0.5))
        want = torch_trajectory(lambda p: torch.optim.Adam(p, lr=0.05))
    else:
        mom = 0.9 if name == "sgd-momentum" else 0.0
        got = ref_trajectory(_descent_ref.options("SGD", lr=0.05, lr_step=2, lr_decay=0.5, momentum=mom))
        want = torch_trajectory(lambda p: torch.optim.SGD(p, lr=0.05, momentum=mom))
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"[descent] {name}: {N_STEPS} steps on the 7-parameter quadratic, worst difference to torch {err:.2e} of the largest entry")
    assert np.abs(want[-1] - X0).max() > 1e-2  # the run moves
    assert err <= 1e-13


def test_steplr_and_best_tracking():
    opt = _descent_ref.options("SGD", lr=0.05, lr_step=2, lr_decay=0.5)
    assert [_descent_ref.learning_rate(it, opt) for it in range(6)] == [0.05, 0.05, 0.025, 0.025, 0.0125, 0.0125]
    assert _descent_ref.best_of([3.0, 1.0, 1.0, float("nan"), 2.0]) == (1.0, 1)  # strict: the first occurrence; a NaN never wins
    assert _descent_ref.best_of([float("nan")] * 3) == (np.inf, -1)


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    text = open(HEADER).read()
    assert re.search(r"#define CMAX_ABI_VERSION 4\b", text) and _lib.ABI_VERSION == 4  # a new struct, no layout changed
    assert re.search(r"#define CMAX_OPT_SGD 0\b", text) and re.search(r"#define CMAX_OPT_ADAM 1\b", text)
    assert (_lib.OPT_SGD, _lib.OPT_ADAM) == (0, 1) and _lib.OPT_CODES == {"SGD": 0, "Adam": 1}
    assert re.search(r"int cmax_sizeof_descent\(void\);", text)
    assert re.search(r"int cmax_patch_plan_descend\(cmax_patch_plan_t plan, const double \*x0_host, int with_tv, const cmax_descent_t \*descent,", text)
    assert re.search(r"int cmax_objective_descend\(cmax_handle_t h, const cmax_objective_t \*desc_host, const double \*theta0_host,", text)
    assert text.count("src/solver/base.py:840-881") >= 3  # the block and each entry cite the function they replace
    for field in ("method", "n_iter", "lr", "lr_step", "lr_decay", "momentum", "beta1", "beta2", "eps"):
        assert re.search(r"\b(int32_t|double) %s;" % field, text), field
        assert field in [f[0] for f in _lib.CmaxDescent._fields_]
    assert [f[0] for f in _lib.CmaxDescentResult._fields_] == ["best_loss", "best_iter", "n_done", "last_lr"]
    lib = _lib.load()
    assert lib.cmax_abi_version() == 4
    assert lib.cmax_sizeof_descent() == ctypes.sizeof(_lib.CmaxDescent)
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    exported = subprocess.run(["nm", "-D", "--defined-only", build.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in SYMBOLS:
        assert re.search(r" T %s$" % name, exported, re.M), name


def _good():
    return _lib.descent_descriptor("Adam", n_iter=6, lr=0.05, lr_step=2, lr_decay=0.5)


BAD = [
    ("method", 7, "method"), ("n_iter", 0, "n_iter"), ("n_iter", 4097, "n_iter"), ("lr", 0.0, "lr "), ("lr", float("nan"), "lr "),
    ("lr", float("inf"), "lr "), ("lr_decay", -0.5, "lr_decay"), ("lr_decay", float("inf"), "lr_decay"), ("eps", 0.0, "eps"),
    ("eps", float("nan"), "eps"), ("lr_step", 0, "lr_step"), ("momentum", 1.0, "momentum"), ("momentum", -0.1, "momentum"),
    ("beta1", 1.0, "beta1"), ("beta1", float("nan"), "beta1"), ("beta2", 1.5, "beta2"), ("beta2", -1e-3, "beta2"),
]


@pytest.mark.parametrize("entry", ["cmax_patch_plan_descend", "cmax_objective_descend"])
@pytest.mark.parametrize("field,value,word", BAD, ids=[f"{f}={v}" for f, v, _ in BAD])
def test_bad_descriptors_are_refused_before_any_gpu_call(entry, field, value, word):
    """No plan, no handle, no device: the descriptor is checked first and the message names the field."""
    lib = _lib.load()
    d = _good()
    setattr(d, field, value)
    res, buf = _lib.CmaxDescentResult(), np.zeros(64)
    p = buf.ctypes.data
    if entry == "cmax_patch_plan_descend":
        rc = lib.cmax_patch_plan_descend(None, p, 1, ctypes.byref(d), ctypes.byref(res), p, p, p, None, None)
    else:
        rc = lib.cmax_objective_descend(None, None, p, ctypes.byref(d), ctypes.byref(res), p, p, p, None, None)
    assert rc == _lib.EINVAL == -1
    msg = lib.cmax_last_error().decode()
    assert "bad descent descriptor" in msg and word in msg, msg
    with pytest.raises(_lib.CmaxError, match="bad descent descriptor"):
        _lib.check(rc)


def test_null_pointers_are_refused():
    lib = _lib.load()
    d, res, buf = _good(), _lib.CmaxDescentResult(), np.zeros(64)
    p = buf.ctypes.data
    assert lib.cmax_patch_plan_descend(None, p, 1, None, ctypes.byref(res), p, p, p, None, None) == _lib.EINVAL
    assert "null descriptor" in lib.cmax_last_error().decode()
    assert lib.cmax_patch_plan_descend(None, p, 1, ctypes.byref(d), ctypes.byref(res), p, p, p, None, None) == _lib.EINVAL
    assert "null pointer" in lib.cmax_last_error().decode()
    assert lib.cmax_objective_descend(None, None, p, ctypes.byref(d), ctypes.byref(res), p, p, p, None, None) == _lib.EINVAL
    assert "null pointer" in lib.cmax_last_error().decode()


def test_descriptor_defaults_are_the_references():
    d = _lib.descent_descriptor("Adam", n_iter=40)  # src/solver/base.py:857-862 and torch.optim.Adam's defaults
    assert (d.method, d.n_iter, d.lr, d.lr_step, d.lr_decay) == (_lib.OPT_ADAM, 40, 0.05, 40, 0.1)
    assert (d.beta1, d.beta2, d.eps) == (0.9, 0.999, 1e-8)
    s = _lib.descent_descriptor("SGD", n_iter=5, momentum=0.9, lr_step=2)
    assert (s.method, s.momentum, s.lr_step) == (_lib.OPT_SGD, 0.9, 2)
    with pytest.raises(NotImplementedError, match="RMSprop"):
        _lib.descent_descriptor("RMSprop")


# ---- the solver classes ----------------------------------------------------------------------------------------------------------------
PARAMS = {"trans_x": {"min": -150, "max": 150}, "trans_y": {"min": -150, "max": 150}}
COMMON = {"motion_model": "2d-translation", "warp_direction": "first", "parameters": ["trans_x", "trans_y"], "cost": "hybrid", "outer_padding": 0,
          "cost_with_weight": {"multi_focal_normalized_gradient_magnitude": 1.0, "total_variation": 0.01},
          "iwe": {"method": "bilinear_vote", "blur_sigma": 1}}


def make(kind, method):
    opt_cfg = {"n_iter": 5, "method": method, "max_iter": 25, "parameters": PARAMS}
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


@pytest.mark.parametrize("kind", ["pyramid", "mixed", "time-aware"])
def test_solver_classes_take_the_first_order_methods(kind):
    for method in ("Adam", "SGD", "Newton-CG"):
        assert make(kind, method).opt_method == method
    for method in ("LBFGS", "optuna", "RMSprop", "AdamW"):  # the rest of the reference's TORCH_OPTIMIZERS, and Optuna
        with pytest.raises(NotImplementedError, match="SGD"):  # the message says what IS built
            make(kind, method)
