"""Device-resident L-BFGS (cmax_patch_plan_lbfgs, cmax_objective_lbfgs; k_lbfgs_step of csrc/cmax_solver.hip): a budget of evaluations
per library call, every accept / backtrack / reset decision on the device.

What is held to what:
  1. the RULE, on a bit-repeatable (deterministic) handle: every traced point is re-evaluated on the same handle (the bits the loop saw)
     and fed to tests/_lbfgs_ref.py TEACHER-FORCED -- its history is rebuilt from the traced accepted points.  Every code is the
     decision the inequality gives (a margin below 1e-12 max(1, |L_a|) is counted; at most one per case), every trial point agrees to
     1e-9 max(1, |x|inf), the loss history to 1e-12, the bookkeeping exactly, and a second call returns the same bytes;
  2. forced branches (parameters from tests/_lbfgs_cases.py, picked on the CPU), each asserting that the branch was taken: overshoot,
     LINESEARCH, the reset of a non-empty history (nx 24 and 4140), the box, convergence at the start, a budget of one, the NaN start;
  3. the 2-DoF entry end to end, at the gates tests/test_gpu_solver.py sets SciPy's BFGS;
  4. a basis plan and a plan with a flow regulariser, teacher-forced as in 1;
  5. state hygiene;  6. the solver classes, and with "Newton-CG" the calls the parent commit made;  7. the refusals, a handle with a
     (one-rank) communicator included.
Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import event_based_optical_flow_amd as E  # noqa: E402
from event_based_optical_flow_amd import _lib, solver  # noqa: E402
from event_based_optical_flow_amd.solver import PatchFlowObjective  # noqa: E402

import _basis_cases as B  # noqa: E402
import _basis_gpu as G  # noqa: E402
import _flowreg_cases as FK  # noqa: E402
import _lbfgs_cases as K  # noqa: E402
import _lbfgs_ref as R  # noqa: E402
import _patch_cases as C  # noqa: E402


def make_objective(ev, spec, deterministic=True):
    """tests/test_gpu_descent.py's construction of a PatchFlowObjective from a row of the case table."""
    h = E.CMaxHandle(spec["size"])
    if deterministic:
        h.set_deterministic(True)
    h.set_events(ev, time_bin=spec["T"] if spec["time_aware"] else 0)
    names = {name: w for name, w in spec["terms"]}
    if spec["tv_weight"]:
        names["total_variation"] = spec["tv_weight"]
    hybrid = len(names) > 1
    shift = tuple(max(spec["pad"][k] - 1, 0) * spec["sw"][k] for k in (0, 1))
    obj = PatchFlowObjective(h, spec["t_scale"], spec["patch_image_size"], spec["sw"], spec["sw"], shift,
                             cost="hybrid" if hybrid else next(iter(names)), cost_with_weight=names if hybrid else None, blur_sigma=spec["sigma"],
                             time_aware=spec["time_aware"], time_bin=spec["T"], flow_interpolation=spec["scheme"], t0_flow_location=spec["t0"],
                             scale_later=spec["scale_later"], omit_boundary=spec["omit"])
    if obj.pad != tuple(spec["pad"]):  # pad 0: below what patch_pad ever returns, but a geometry the library takes
        assert min(spec["pad"]) == 0
        obj.pad = tuple(spec["pad"])
        obj.__del__()
        obj._build_native_plan()
    assert obj.has_native_plan and obj.pad == tuple(spec["pad"])
    return h, obj


def case_setup(c):
    ev, spec, x0, tv = K.inputs(c)
    h, obj = make_objective(ev, spec)
    return h, obj, x0, tv


def _bytes(res):
    return (res.x.tobytes(), res.loss_history.tobytes(), res.alpha.tobytes(), res.code.tobytes(), None if res.trace is None else res.trace.tobytes(),
            res.fun, res.gnorm_inf, res.last_alpha, res.nit, res.nfev, res.status_code)


def check_identities(res, n):
    """The bookkeeping that needs no restatement: the result is the last accepted point of the trace, the accepted losses never increase,
    the evaluations behind the terminating one are idle."""
    accepted = np.flatnonzero((res.code == R.START) | (res.code == R.ACCEPTED))
    assert res.nit == len(accepted) - 1 and res.fun == res.loss_history[accepted[-1]]
    np.testing.assert_array_equal(res.x, res.trace[accepted[-1]])
    np.testing.assert_array_equal(res.x, res.trace[n])
    assert res.last_alpha == (res.alpha[accepted[-1]] if res.nit else 0.0)
    assert np.isnan(res.loss_history[res.nfev:]).all() and (res.code[res.nfev:] == R.IDLE).all() and np.isfinite(res.loss_history[:res.nfev]).all()
    assert (res.alpha[res.nfev:] == 0.0).all()
    assert (np.diff(res.accepted_losses) <= 0.0).all()


def teacher_forced(tag, res, x0, kw, evaluate):
    """The gates of 1 on one result.  evaluate(x) -> (L, g): the bits the loop saw."""
    desc, n = R.descriptor(**kw), kw["n_eval"]
    assert res.trace.shape == (n + 1, x0.size) and res.loss_history.shape == res.alpha.shape == res.code.shape == (n,)
    np.testing.assert_array_equal(res.trace[0], x0)
    st = R.start(x0, desc)
    e_x = e_loss = e_alpha = 0.0
    undecided, smallest, g_acc = 0, np.inf, None
    for e in range(n):
        st["x"] = res.trace[e].copy()  # teacher-forced: the point the device evaluated
        L, g = evaluate(res.trace[e])
        was_done, La = st["done"], st["La"]
        st, _ = R.transition(st, L, g)
        if st["margin"] is not None:
            rel = abs(st["margin"]) / max(1.0, abs(La))
            smallest = min(smallest, rel)
            if rel < 1e-12:
                undecided += 1
                if res.code[e] != st["code"]:
                    print(f"[lbfgs] {tag}: evaluation {e} undecided (margin {rel:.2e}) and taken the other way; the comparison ends here")
                    assert undecided <= 1
                    check_identities(res, n)
                    return
        assert res.code[e] == st["code"], (tag, e, _lib.LBFGS_CODES[int(res.code[e])], _lib.LBFGS_CODES[st["code"]], st["margin"])
        if was_done:
            assert np.isnan(res.loss_history[e]) and res.alpha[e] == 0.0
        else:
            e_loss = max(e_loss, abs(res.loss_history[e] - L) / abs(L))
            e_alpha = max(e_alpha, abs(res.alpha[e] - st["alpha_e"]) / max(st["alpha_e"], 1e-300) if st["alpha_e"] else abs(res.alpha[e]))
        if st["code"] in (R.START, R.ACCEPTED):
            g_acc = g
        expected = st["x"] if e < n - 1 else st["xa"]  # row e + 1: the next point evaluated; the last row: the final x_a
        e_x = max(e_x, np.abs(res.trace[e + 1] - expected).max() / max(1.0, np.abs(expected).max()))
    print(f"[lbfgs] {tag}: nx {x0.size}, codes {''.join(map(str, res.code))}, status {res.status}, nit {res.nit}, nfev {res.nfev}, loss "
          f"{res.loss_history[0]:.6g} -> {res.fun:.6g}; worst trial-point error {e_x:.2e} of max(1, |x|inf), loss history {e_loss:.2e}, alpha {e_alpha:.2e}, "
          f"smallest Armijo margin {smallest:.2e}, undecided {undecided}")
    assert undecided <= 1
    assert e_x <= 1e-9 and e_loss <= 1e-12 and e_alpha <= 1e-9
    # the bookkeeping, exactly
    assert (res.nit, res.status_code, res.status) == (st["n_iter"], st["status"], R.STATUS_WORDS[st["status"]])
    assert res.nfev == (st["used"] if st["done"] else n)
    assert res.gnorm_inf == np.abs(g_acc).max()
    check_identities(res, n)


# ---- 1. the rule, on a bit-repeatable handle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(K.RULE))
def test_rule_on_a_bit_repeatable_handle(cid):
    c = K.RULE[cid]
    h, obj, x0, tv = case_setup(c)
    kw = K.descriptor_kwargs(c)
    res = obj.minimize_lbfgs(x0, with_tv=tv, trace=True, **kw)
    teacher_forced(cid, res, x0, kw, lambda x: obj.value_and_grad_numpy(x, with_tv=tv))
    assert res.nit > min(c["history"], 3)  # the ring wrapped (m = 1, 3) or is partly filled (m = 8)
    again = obj.minimize_lbfgs(x0, with_tv=tv, trace=True, **kw)
    assert _bytes(again) == _bytes(res)
    del obj
    h.close()


# ---- 2. forced branches ----------------------------------------------------------------------------------------------------------------------
def test_overshoot_rejects_then_accepts():
    c = K.FORCED["overshoot"]
    h, obj, x0, tv = case_setup(c)
    kw = K.descriptor_kwargs(c)
    res = obj.minimize_lbfgs(x0, with_tv=tv, trace=True, **kw)
    teacher_forced("overshoot", res, x0, kw, lambda x: obj.value_and_grad_numpy(x, with_tv=tv))
    first = int(np.argmax(res.code == R.ACCEPTED))
    assert first >= 2 and (res.code[1:first] == R.REJECTED).all() and res.code[first] == R.ACCEPTED
    np.testing.assert_allclose(res.alpha[1:first + 1], res.alpha[1] * 0.5 ** np.arange(first), rtol=1e-15)
    assert (res.loss_history[1:first] > res.loss_history[0]).all() and res.loss_history[first] < res.loss_history[0]
    del obj
    h.close()


def test_max_ls_one_ends_the_line_search():
    c = K.FORCED["max-ls-1"]
    h, obj, x0, tv = case_setup(c)
    kw = K.descriptor_kwargs(c)
    res = obj.minimize_lbfgs(x0, with_tv=tv, trace=True, **kw)
    teacher_forced("max-ls-1", res, x0, kw, lambda x: obj.value_and_grad_numpy(x, with_tv=tv))
    assert res.status == "LINESEARCH" or (res.code == R.RESET).any()
    assert res.status == "LINESEARCH" and res.nit == 0 and res.nfev == 3 and list(res.code[:4]) == [R.START, R.REJECTED, R.REJECTED, R.IDLE]
    np.testing.assert_array_equal(res.x, x0)
    np.testing.assert_array_equal(res.trace[3:], np.tile(x0, (kw["n_eval"] - 2, 1)))  # the idle evaluations run at x_a
    del obj
    h.close()


@pytest.mark.parametrize("cid", ["reset-3x4-m8", "reset-46x45-m3"])
def test_reset_with_a_history(cid):
    """max_ls = 1 behind accepted steps: the second reject in a row meets a non-empty history, which goes; the direction is chosen
    again from g_a (steepest) and the solve continues."""
    c = K.FORCED[cid]
    h, obj, x0, tv = case_setup(c)
    kw = K.descriptor_kwargs(c)
    res = obj.minimize_lbfgs(x0, with_tv=tv, trace=True, **kw)
    teacher_forced(cid, res, x0, kw, lambda x: obj.value_and_grad_numpy(x, with_tv=tv))
    first = int(np.argmax(res.code == R.RESET))
    assert res.code[first] == R.RESET and res.code[first - 1] == R.REJECTED and (res.code[:first] == R.ACCEPTED).sum() >= 2
    np.testing.assert_allclose(res.alpha[first], 0.9 * res.alpha[first - 1], rtol=1e-15)  # the trial that failed was the shrunk one
    assert res.status == "BUDGET" and res.code[first + 1] == R.ACCEPTED and res.alpha[first + 1] <= 1.0
    assert _bytes(obj.minimize_lbfgs(x0, with_tv=tv, trace=True, **kw)) == _bytes(res)
    del obj
    h.close()


def test_small_box():
    c = K.FORCED["small-box"]
    h, obj, x0, tv = case_setup(c)
    kw = K.descriptor_kwargs(c)
    res = obj.minimize_lbfgs(x0, with_tv=tv, trace=True, **kw)
    teacher_forced("small-box", res, x0, kw, lambda x: obj.value_and_grad_numpy(x, with_tv=tv))
    lo, hi = x0 - c["max_move"], x0 + c["max_move"]
    assert ((res.trace >= lo) & (res.trace <= hi)).all()  # every row, trial points included
    reached = np.abs(res.trace - x0).max()
    print(f"[lbfgs] small box: status {res.status}, reached {reached:.6g} of {c['max_move']}, alphas {res.alpha[:res.nfev]}")
    assert res.status == "BOX" or (res.alpha[1:res.nfev] < 1.0).any()
    assert reached == c["max_move"]  # a clipped alpha puts an entry ON the wall
    del obj
    h.close()


def test_converged_at_the_start_and_a_budget_of_one():
    c = K.RULE["3x4-m3-tv"]
    h, obj, x0, tv = case_setup(c)
    loss, grad = obj.value_and_grad_numpy(x0, with_tv=tv)
    res = obj.minimize_lbfgs(x0, n_eval=4, gtol=1e9, max_move=1.0, with_tv=tv, trace=True)
    assert (res.status, res.nit, res.nfev, res.success) == ("CONVERGED", 0, 1, True) and list(res.code) == [R.START, R.IDLE, R.IDLE, R.IDLE]
    assert res.fun == res.loss_history[0] and abs(res.fun - loss) <= 1e-12 * abs(loss) and np.isnan(res.loss_history[1:]).all()
    assert res.gnorm_inf == np.abs(grad).max()
    np.testing.assert_array_equal(res.trace, np.tile(x0, (5, 1)))
    one = obj.minimize_lbfgs(x0, n_eval=1, max_move=1.0, with_tv=tv, trace=True)
    assert (one.status, one.nit, one.nfev) == ("BUDGET", 0, 1) and list(one.code) == [R.START] and one.fun == res.fun
    np.testing.assert_array_equal(one.x, x0)
    np.testing.assert_array_equal(one.trace, np.tile(x0, (2, 1)))
    del obj
    h.close()


def test_nonfinite_start_on_the_documented_nan():
    """A scale_later plan at x = 0: max D = 0, loss and gradient are the reference's 0/0 (the input of tests/test_gpu_descent.py::
    test_stop_rule_on_the_documented_nan).  No step is taken; the plan is usable afterwards."""
    ev = C.batch((20, 32))
    spec = C.spec_of("3x4-odd", (20, 32), t_scale=float(ev[:, 2].max() - ev[:, 2].min()), scale_later=True, **K.BURGERS)
    h, obj = make_objective(ev, spec, deterministic=False)
    x0 = np.zeros(obj._nx)
    res = obj.minimize_lbfgs(x0, n_eval=5, max_move=1.0, trace=True)
    print(f"[lbfgs] NaN start: status {res.status}, nit {res.nit}, nfev {res.nfev}, fun {res.fun}, history {res.loss_history}")
    assert (res.status, res.nit, res.nfev, res.last_alpha) == ("NONFINITE_START", 0, 1, 0.0) and np.isnan(res.gnorm_inf) and np.isnan(res.fun)
    assert np.isnan(res.loss_history).all() and list(res.code) == [R.START] + [R.IDLE] * 4 and (res.alpha == 0.0).all()
    np.testing.assert_array_equal(res.x, x0)
    np.testing.assert_array_equal(res.trace, np.zeros((6, obj._nx)))
    x1 = C.patch_motion("random", spec["patch_image_size"], 5)
    again = obj.minimize_lbfgs(x1, n_eval=5, max_move=50.0)
    assert again.status in ("BUDGET", "BOX") and again.nit >= 1 and np.isfinite(again.loss_history[:again.nfev]).all()
    assert (np.diff(again.accepted_losses) <= 0.0).all()
    del obj
    h.close()


# ---- 3. the 2-DoF entry, end to end ----------------------------------------------------------------------------------------------------------
def test_two_dof_recovers_the_generating_velocity():
    """The setting and the gates of tests/test_gpu_solver.py::test_minimize_recovers_the_generating_velocity (SciPy's BFGS there)."""
    size, vel = (96, 128), np.array([9.0, -6.0])
    ev = E.utils.generate_structured_events(60000, size[0], size[1], tuple(vel), n_dots=120, jitter=0.3, seed=5)
    h = E.CMaxHandle(size).set_events(ev)
    obj = E.ContrastObjective(h, "2d-translation", cost="image_variance", sigma=1)
    res = obj.minimize_lbfgs(vel * 0.7, n_eval=32, history=4, gtol=1e-7, max_move=5.0, trace=True)
    desc = obj.terms[0][2]
    _, grad = h.evaluate(desc, torch.tensor(res.x, dtype=torch.float64, device="cuda"))
    gnorm = float(np.linalg.norm(grad.cpu().numpy()))
    print(f"[lbfgs] 2-DoF: {res}, x {res.x}, |x - vel|inf {np.abs(res.x - vel).max():.3f}, |g|2 at x {gnorm:.3e} (reported |g|inf {res.gnorm_inf:.3e}), "
          f"codes {''.join(map(str, res.code))}")
    assert np.abs(res.x - vel).max() < 0.35, res
    assert gnorm < 0.05
    acc = res.accepted_losses
    assert len(acc) == res.nit + 1 >= 3 and (np.diff(acc) <= 0.0).all() and res.fun == acc[-1]
    assert ((res.trace >= vel * 0.7 - 5.0) & (res.trace <= vel * 0.7 + 5.0)).all()
    h.close()


TWO_DOF_SIZE = (40, 56)


def two_dof_events():
    H, W = TWO_DOF_SIZE
    a = E.utils.generate_events(1500, H, W, 0.0, 0.05, seed=7)
    b = E.utils.generate_structured_events(2500, H, W, (4.0, -3.0), n_dots=12, tmin=0.0, tmax=0.05, seed=8)
    ev = np.concatenate([a, b])
    ev[:, 0], ev[:, 1] = np.clip(ev[:, 0], 0, H - 1), np.clip(ev[:, 1], 0, W - 1)
    return np.ascontiguousarray(ev[np.argsort(ev[:, 2], kind="stable")])


def test_two_dof_rule_and_state_on_a_deterministic_handle():
    """nx = 2 through cmax_objective_lbfgs, teacher-forced as in 1; the state is handle-owned and counted in cmax_handle_info."""
    h = E.CMaxHandle(TWO_DOF_SIZE).set_deterministic(True).set_events(two_dof_events())
    obj = E.ContrastObjective(h, "2d-translation", cost="image_variance", sigma=1)
    desc, theta0 = obj.terms[0][2], np.array([3.0, -2.0])
    h.evaluate(desc, torch.tensor(theta0, device="cuda"))  # (the evaluation's own lazy workspaces first)
    before = h.workspace_bytes
    kw = dict(n_eval=12, history=3, gtol=1e-9, max_move=4.0, step0=1.0, max_ls=10)
    res = obj.minimize_lbfgs(theta0, trace=True, **kw)
    assert h.workspace_bytes - before == 8 * 16 + _lib.lbfgs_state_bytes(2, 3, 12, True)  # theta | grad | result in front of the documented state

    def evaluate(x):
        result, grad = h.evaluate(desc, torch.tensor(x, dtype=torch.float64, device="cuda"))
        return float(result[0].item()), grad.cpu().numpy().astype(np.float64)

    teacher_forced("2-DoF deterministic", res, theta0, kw, evaluate)
    assert _bytes(obj.minimize_lbfgs(theta0, trace=True, **kw)) == _bytes(res)
    assert h.workspace_bytes - before == 8 * 16 + _lib.lbfgs_state_bytes(2, 3, 12, True)  # kept while it is large enough
    h.close()


# ---- 4. a basis plan, a plan with a flow regulariser -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reg", [None, "area"], ids=["affine", "affine+area"])
def test_basis_plan_and_regulariser(reg):
    c = B.PLAN["affine-27x40-two"]
    ev, theta0, spec = B.inputs(c)
    h, obj = G.make_objective(c, ev, spec, deterministic=True)
    assert theta0.size == 6
    if reg:
        obj.set_flow_regularizer(FK.REGS[reg])
    kw = dict(n_eval=12, history=3, gtol=1e-9, max_move=20.0, step0=1.0, max_ls=10)
    res = obj.minimize_lbfgs(theta0, trace=True, **kw)
    teacher_forced(f"basis {reg}", res, np.asarray(theta0, dtype=np.float64).reshape(-1), kw, obj.value_and_grad_numpy)
    assert res.nit > kw["history"]  # the ring wrapped
    del obj
    h.close()


# ---- 5. state hygiene --------------------------------------------------------------------------------------------------------------------------
def test_state_hygiene():
    c = K.RULE["3x4-m8-burgers"]
    h, obj, x0, tv = case_setup(c)
    h2, fresh, _, _ = case_setup(c)
    big = dict(K.descriptor_kwargs(c), n_eval=20, history=8)
    small = dict(K.descriptor_kwargs(c), n_eval=7, history=2)
    first = obj.minimize_lbfgs(x0, with_tv=tv, trace=True, **big)
    # evaluations after a solve are what a fresh plan returns
    loss, grad = obj.value_and_grad_numpy(x0)
    loss_f, grad_f = fresh.value_and_grad_numpy(x0)
    assert loss == loss_f and grad.tobytes() == grad_f.tobytes()
    # a smaller budget, a shorter history, no trace behind the larger call: what a plan that never ran the larger call gives
    a, b = obj.minimize_lbfgs(x0, with_tv=tv, trace=True, **small), fresh.minimize_lbfgs(x0, with_tv=tv, trace=True, **small)
    assert _bytes(a) == _bytes(b)
    quiet = obj.minimize_lbfgs(x0, with_tv=tv, **small)
    assert quiet.trace is None and quiet.x.tobytes() == a.x.tobytes() and quiet.loss_history.tobytes() == a.loss_history.tobytes()
    assert quiet.code.tobytes() == a.code.tobytes()
    # ... and the larger call again: the same bytes; its first evaluations do not depend on the budget
    assert _bytes(obj.minimize_lbfgs(x0, with_tv=tv, trace=True, **big)) == _bytes(first)
    assert _bytes(fresh.minimize_lbfgs(x0, with_tv=tv, trace=True, **big)) == _bytes(first)
    # a descent in between shares the tail's output buffer and the result block
    obj.descend(x0, n_iter=3)
    assert _bytes(obj.minimize_lbfgs(x0, with_tv=tv, trace=True, **big)) == _bytes(first)
    del obj, fresh
    h.close()
    h2.close()


# ---- 6. the solver classes ---------------------------------------------------------------------------------------------------------------------
PARAMS = {"trans_x": {"min": -150, "max": 150}, "trans_y": {"min": -150, "max": 150}}
COMMON = {"motion_model": "2d-translation", "warp_direction": "first", "parameters": ["trans_x", "trans_y"], "cost": "hybrid", "outer_padding": 0,
          "cost_with_weight": {"multi_focal_normalized_gradient_magnitude": 1.0, "total_variation": 0.01},
          "iwe": {"method": "bilinear_vote", "blur_sigma": 1}}
SOLVER_SIZE = (66, 90)


def opt_cfg(method):
    return {"n_iter": 5, "method": method, "max_iter": 3, "parameters": PARAMS, "lbfgs": {"history": 3, "max_move": 30.0}}


def make_solver(kind, method):
    if kind == "pyramid":
        cfg = dict(COMMON, method="pyramidal_patch_contrast_maximization", time_aware=False,
                   patch={"initialize": "random", "scale": 3, "crop_height": 64, "crop_width": 80, "filter_type": "bilinear"})
        return solver.collections["pyramidal_patch_contrast_maximization"](SOLVER_SIZE, {}, cfg, opt_cfg(method), {}, None), SOLVER_SIZE
    time_aware = kind == "time-aware"
    cfg = dict(COMMON, time_aware=time_aware, patch={"initialize": "random", "size": 16, "sliding_window": 16, "filter_type": "bilinear"})
    if time_aware:
        cfg.update(time_bin=10, flow_interpolation="burgers", t0_flow_location="middle")
    cls = solver.collections["time_aware_mixed_patch_contrast_maximization"] if time_aware else solver.MixedPatchContrastMaximization
    return cls((68, 90), {}, cfg, opt_cfg(method), {}, None), (68, 90)


@pytest.mark.parametrize("kind", ["pyramid", "mixed", "time-aware"])
def test_solver_classes_with_device_lbfgs(kind):
    slv, size = make_solver(kind, "device-L-BFGS")
    np.random.seed(3)
    motion = slv.optimize(C.batch(size))
    results = [r for _, r in slv.history] if kind == "pyramid" else [slv.history[-1]]
    assert len(results) == (2 if kind == "pyramid" else 1)
    for res in results:
        assert isinstance(res, _lib.LbfgsResult) and res.loss_history.shape == (5,) and res.nfev <= 5
        print(f"[lbfgs] {kind}: loss {res.loss_history[0]:.6g} -> {res.fun:.6g}, status {res.status}, nit {res.nit}")
        assert res.fun <= res.loss_history[0] and (np.diff(res.accepted_losses) <= 0.0).all()
    last = motion[max(motion)] if kind == "pyramid" else motion
    np.testing.assert_array_equal(np.asarray(last).reshape(-1), results[-1].x)


# What the objectives of the three classes were asked with "Newton-CG" BEFORE this change: counted on the parent commit with the wrapper
# below, the same configuration and seed, on a deterministic handle (bit-repeatable, so the optimiser's path and with it the counts are
# the same in every run).
PARENT_CALLS = {
    "pyramid": {"value_and_grad_numpy": 11, "hvp_numpy": 6, "ensure_time_slabs": 17},
    "mixed": {"value_and_grad_numpy": 5, "hvp_numpy": 3, "ensure_time_slabs": 8},
    "time-aware": {"value_and_grad_numpy": 5, "hvp_numpy": 3, "ensure_time_slabs": 8},
}
COUNTED = ("value_and_grad_numpy", "hvp_numpy", "descend", "minimize_lbfgs", "ensure_time_slabs", "set_t_scale")


@pytest.mark.parametrize("kind", ["pyramid", "mixed", "time-aware"])
def test_newton_cg_makes_the_calls_it_made(kind, monkeypatch):
    """Without the new method name not one call changes: the objectives' entries are counted through a wrapper and held to the counts
    of the parent commit; none of the new ones is reached."""
    counts = {}

    def counted(name):
        orig = getattr(PatchFlowObjective, name)

        def wrapper(self, *a, **k):
            counts[name] = counts.get(name, 0) + 1
            return orig(self, *a, **k)

        monkeypatch.setattr(PatchFlowObjective, name, wrapper)

    for name in COUNTED:
        counted(name)
    slv, size = make_solver(kind, "Newton-CG")
    slv._handle = E.CMaxHandle(size).set_keep_outside(False).set_deterministic(True)
    np.random.seed(3)
    slv.optimize(C.batch(size))
    print(f"[lbfgs] {kind} + Newton-CG: calls {counts} (parent: {PARENT_CALLS[kind]})")
    assert counts == PARENT_CALLS[kind]
    assert "minimize_lbfgs" not in counts and "descend" not in counts and counts["value_and_grad_numpy"] > 0 and counts["hvp_numpy"] > 0


# ---- 7. the refusals -----------------------------------------------------------------------------------------------------------------------------
def test_plan_refusals():
    c = K.RULE["3x4-m3-tv"]
    ev, spec, x0, tv = K.inputs(c)
    h, obj = make_objective(ev, spec, deterministic=False)
    with pytest.raises(ValueError, match="elements"):
        obj.minimize_lbfgs(x0[:-1])
    with pytest.raises(_lib.CmaxError, match="history"):
        obj.minimize_lbfgs(x0, history=17)
    with pytest.raises(_lib.CmaxError, match="max_move"):
        obj.minimize_lbfgs(x0, max_move=0.0)
    h.set_event_weights(np.full(len(ev), 0.5))  # a plan made before the handle received weights: refused like cmax_patch_plan_descend
    with pytest.raises(NotImplementedError, match="per-event weights"):
        obj.minimize_lbfgs(x0, n_eval=2)
    h.set_event_weights(None)
    assert obj.minimize_lbfgs(x0, n_eval=2).nfev == 2
    del obj
    h.close()


def test_handles_with_a_communicator_are_refused():
    """Rule 3 of the entries: CMAX_EUNSUPPORTED behind the descriptor and null-pointer checks, before anything is reserved or enqueued
    -- n_eval evaluations of a time-sliced batch would be n_eval collectives with no host in between.  A one-rank RCCL communicator
    (tests/test_gpu_basis_plan.py makes one the same way) on a plan built before it arrived, and on the 2-DoF entry.  A handle cannot
    hold weights and a communicator at once (each refuses the other), so the weighted refusal is reached only without one."""
    import ctypes

    lib = _lib.load()
    c = K.RULE["3x4-m3-tv"]
    ev, spec, x0, tv = K.inputs(c)
    h, obj = make_objective(ev, spec, deterministic=False)
    h.comm_init(force_rccl=True)
    before = h.workspace_bytes
    with pytest.raises(NotImplementedError, match="communicator"):
        obj.minimize_lbfgs(x0, n_eval=3)
    d, res = _lib.lbfgs_descriptor(n_eval=3), _lib.CmaxLbfgsResult()
    out = np.full(4 * x0.size + 16, -7.0)
    code = np.full(4, -7, dtype=np.int32)
    rc = lib.cmax_patch_plan_lbfgs(obj._plan, x0.ctypes.data, 1, ctypes.byref(d), ctypes.byref(res), out.ctypes.data, out[x0.size:].ctypes.data,
                                   out[x0.size + 4:].ctypes.data, code.ctypes.data, None, None)
    assert rc == _lib.EUNSUPPORTED and b"communicator" in lib.cmax_last_error()
    d.history = 0  # the descriptor is checked first, the null pointers second
    assert lib.cmax_patch_plan_lbfgs(obj._plan, x0.ctypes.data, 1, ctypes.byref(d), ctypes.byref(res), out.ctypes.data, out.ctypes.data, out.ctypes.data,
                                     code.ctypes.data, None, None) == _lib.EINVAL and b"history" in lib.cmax_last_error()
    d.history = 3
    assert lib.cmax_patch_plan_lbfgs(obj._plan, x0.ctypes.data, 1, ctypes.byref(d), ctypes.byref(res), None, out.ctypes.data, out.ctypes.data,
                                     code.ctypes.data, None, None) == _lib.EINVAL and b"null pointer" in lib.cmax_last_error()
    two = E.ContrastObjective(h, "2d-translation", cost="image_variance", sigma=1)
    with pytest.raises(NotImplementedError, match="communicator"):
        two.minimize_lbfgs(np.array([1.0, -1.0]), n_eval=3, max_move=2.0)
    desc = _lib.CmaxObjective.from_buffer_copy(two.terms[0][2])
    desc.motion_dtype = _lib.F64
    theta0 = np.array([1.0, -1.0])
    rc = lib.cmax_objective_lbfgs(h._h, ctypes.byref(desc), theta0.ctypes.data, ctypes.byref(d), ctypes.byref(res), out.ctypes.data, out[2:].ctypes.data,
                                  out[6:].ctypes.data, code.ctypes.data, None, None)
    assert rc == _lib.EUNSUPPORTED and b"communicator" in lib.cmax_last_error()
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (code == -7).all() and res.n_eval_used == 0  # nothing was written
    assert h.workspace_bytes == before  # ... and no state was reserved
    h.comm_destroy()
    h.set_event_weights(np.full(len(ev), 0.5))  # without the communicator the weighted refusal is next
    with pytest.raises(NotImplementedError, match="per-event weights"):
        obj.minimize_lbfgs(x0, n_eval=2)
    h.set_event_weights(None)
    assert obj.minimize_lbfgs(x0, n_eval=3).nfev == 3 and two.minimize_lbfgs(theta0, n_eval=3, max_move=2.0).nfev == 3
    del obj
    h.close()


def test_two_dof_refusals():
    h = E.CMaxHandle(TWO_DOF_SIZE).set_events(two_dof_events())
    obj = E.ContrastObjective(h, "2d-translation", cost="image_variance", sigma=0)
    desc, d = obj.terms[0][2], _lib.lbfgs_descriptor(n_eval=3)
    dense = E.ContrastObjective(h, "dense-flow", cost="image_variance")
    with pytest.raises(NotImplementedError, match="2-DoF"):
        dense.minimize_lbfgs(np.zeros(2))
    bad = _lib.CmaxObjective.from_buffer_copy(dense.terms[0][2])
    with pytest.raises(_lib.CmaxError, match="2-DoF descriptors only"):
        h.minimize_lbfgs(bad, np.zeros(2), d)
    f32 = _lib.CmaxObjective.from_buffer_copy(desc)
    f32.motion_dtype = _lib.F32
    res, buf = _lib.CmaxLbfgsResult(), np.zeros(64)
    import ctypes
    p = buf.ctypes.data
    rc = _lib.load().cmax_objective_lbfgs(h._h, ctypes.byref(f32), p, ctypes.byref(d), ctypes.byref(res), p, p, p, p, None, None)
    assert rc == _lib.EINVAL and b"motion_dtype must be CMAX_F64" in _lib.load().cmax_last_error()
    hybrid = E.ContrastObjective(h, "2d-translation", cost="hybrid", cost_with_weight={"image_variance": 1.0, "gradient_magnitude": 0.5})
    with pytest.raises(NotImplementedError, match="ONE fused term"):
        hybrid.minimize_lbfgs(np.zeros(2))
    d.n_eval = 0
    with pytest.raises(_lib.CmaxError, match="n_eval"):
        h.minimize_lbfgs(desc, np.array([1.0, -1.0]), d)
    with pytest.raises(ValueError, match="needs 2"):
        h.minimize_lbfgs(desc, np.zeros(3), _lib.lbfgs_descriptor(n_eval=3))
    assert obj.minimize_lbfgs(np.array([1.0, -1.0]), n_eval=3, max_move=2.0).nfev == 3  # (the deferred-path objective takes the general sequence)
    h.close()
