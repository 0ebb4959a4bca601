"""Device-resident SGD / Adam (cmax_patch_plan_descend, cmax_objective_descend; k_descent_step of csrc/cmax_solver.hip and
k_finish_raw_step of csrc/cmax_fused.hip): n iterations per library call, iterate and optimiser state in device memory.

What is held to what:
  1. the RULE, on a bit-repeatable (deterministic) handle: every traced iterate is re-evaluated on the same handle (the same bits the loop
     saw), the optimiser's state is rebuilt from those gradients with tests/_descent_ref.py (== torch.optim, tests/test_descent_reference.py)
     and every step must agree to 1e-10 max(1, |x|inf) -- fp64 rounding and FMA contraction are all that separates the two;
  2. the steps against INDEPENDENT gradients (tests/_patch_ref.py, fp64) on a default handle, SGD: linear in g, so the project's 1e-4
     gradient gate carried through the momentum sum, lr_it 1e-4 |g_ref|inf / (1 - momentum);
  3. the 2-DoF entry on the deferred path (the fused finishing kernel), on the general path and on a weighted handle, SGD as in 2 and
     Adam at 2e-3 of the step once the reference gradients' entries are within a factor 4 of each other;
  4. the stop rule on the documented NaN of a scale_later plan at x = 0 (no non-finite motion ever reaches an event kernel);
  5. state hygiene: evaluations after a descent, repeated descents, another method / n_iter behind the first;
  6. the solver classes with optimizer.method "Adam".
Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import event_based_optical_flow_amd as E  # noqa: E402
from event_based_optical_flow_amd import _lib, solver  # noqa: E402
from event_based_optical_flow_amd.solver import PatchFlowObjective  # noqa: E402

import _descent_ref  # noqa: E402
import _hvp_ref  # noqa: E402
import _patch_cases as C  # noqa: E402
import _patch_ref  # noqa: E402
from _weighted_ref import weighted_objective  # noqa: E402

N_ITER, LR, LR_STEP, LR_DECAY, MOMENTUM = 6, 0.05, 2, 0.5, 0.9  # three learning rates occur
GRAD_TOL = 1e-4  # the project's gradient gate (tests/test_gpu_patch_side.py, tests/test_gpu_fused.py)
METHODS = {"sgd": dict(method="SGD", momentum=MOMENTUM), "adam": dict(method="Adam")}
SCHEDULE = dict(n_iter=N_ITER, lr=LR, lr_step=LR_STEP, lr_decay=LR_DECAY)
_BURGERS = dict(time_aware=True, T=10, scheme="burgers", t0="middle")
_BATCH = {}


def ref_options(mid):
    kw = METHODS[mid]
    return _descent_ref.options(kw["method"], lr=LR, lr_step=LR_STEP, lr_decay=LR_DECAY, momentum=kw.get("momentum", 0.0))


def batch(size):
    if size not in _BATCH:
        _BATCH[size] = C.batch(size)
    return _BATCH[size]


def make_objective(ev, spec, deterministic=False):
    """tests/test_gpu_patch_side.py's construction of a PatchFlowObjective from a row of the case table."""
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


def plan_setup(gid, size, deterministic, **kw):
    ev = batch(size)
    spec = C.spec_of(gid, size, t_scale=float(ev[:, 2].max() - ev[:, 2].min()), **kw)
    h, obj = make_objective(ev, spec, deterministic)
    x0 = C.patch_motion("random", C.GEOMETRY[gid]["patch_image_size"], 77 + len(gid))
    return ev, spec, h, obj, x0


def check_bookkeeping(res, x0, n_iter=N_ITER):
    """What does not depend on the gradients: shapes, the argmin (first occurrence) of the history, x_best, x_last, the trace's ends."""
    assert res.trace.shape == (n_iter + 1, x0.size) and res.loss_history.shape == (n_iter,)
    assert res.n_done == n_iter and np.isfinite(res.loss_history).all()
    np.testing.assert_array_equal(res.trace[0], x0)
    np.testing.assert_array_equal(res.x_last, res.trace[n_iter])
    best, best_it = _descent_ref.best_of(res.loss_history)
    assert res.best_iter == best_it == int(np.argmin(res.loss_history)) and res.best_loss == best
    np.testing.assert_array_equal(res.x_best, res.trace[best_it])
    assert res.last_lr == _descent_ref.learning_rate(n_iter - 1, dict(lr=LR, lr_step=LR_STEP, lr_decay=LR_DECAY))


# ---- 1. the rule, on a bit-repeatable handle ----------------------------------------------------------------------------------------------
RULE_GEOMETRIES = [("1x1-pad0", (20, 28)), ("3x4-odd", (27, 40)), ("46x45", (92, 90))]  # nx 2 (below a wave), 24, 4140 (a grid-stride remainder)


@pytest.mark.parametrize("mid", list(METHODS))
@pytest.mark.parametrize("variant", ["plain", "burgers"])
@pytest.mark.parametrize("gid,size", RULE_GEOMETRIES, ids=[g for g, _ in RULE_GEOMETRIES])
def test_rule_on_a_bit_repeatable_handle(gid, size, variant, mid):
    ev, spec, h, obj, x0 = plan_setup(gid, size, True, **(_BURGERS if variant == "burgers" else {}))
    res = obj.descend(x0, trace=True, **SCHEDULE, **METHODS[mid])
    check_bookkeeping(res, x0)
    opt, state = ref_options(mid), {}
    e_x = e_loss = 0.0
    for it in range(N_ITER):
        loss, grad = obj.value_and_grad_numpy(res.trace[it])  # the same bits the loop saw: the handle is bit-repeatable
        expected = _descent_ref.step(state, res.trace[it], grad, it, opt)
        e_x = max(e_x, np.abs(res.trace[it + 1] - expected).max() / max(1.0, np.abs(expected).max()))
        e_loss = max(e_loss, abs(res.loss_history[it] - loss) / abs(loss))
    moved = np.abs(res.x_last - x0).max()
    print(f"[descent] rule {gid} {variant} {mid}: nx {x0.size}, moved {moved:.3e}, worst step error {e_x:.2e} of max(1, |x|inf), "
          f"loss history {e_loss:.2e}, best {res.best_loss:.6g} at {res.best_iter}")
    assert moved > 0.0
    assert e_x <= 1e-10 and e_loss <= 1e-12
    del obj
    h.close()


# ---- 2. independent gradients, default handle, SGD ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_tv", [True, False], ids=["tv", "smooth"])
@pytest.mark.parametrize("gid,size", [("3x4-odd", (27, 40)), ("16x16", (66, 90))], ids=["3x4-odd", "16x16"])
def test_sgd_steps_against_the_fp64_reference_gradients(gid, size, with_tv):
    ev, spec, h, obj, x0 = plan_setup(gid, size, False)
    res = obj.descend(x0, trace=True, with_tv=with_tv, **SCHEDULE, **METHODS["sgd"])
    check_bookkeeping(res, x0)
    opt, state, worst = ref_options("sgd"), {}, 0.0
    for it in range(N_ITER):
        loss_ref, g_ref, _ = _patch_ref.plan(res.trace[it], ev, spec, with_tv=with_tv)
        expected = _descent_ref.step(state, res.trace[it], g_ref, it, opt)
        tol = _descent_ref.learning_rate(it, opt) * GRAD_TOL * np.abs(g_ref).max() / (1.0 - MOMENTUM)
        err = np.abs(res.trace[it + 1] - expected).max()
        e_loss = abs(res.loss_history[it] - loss_ref) / abs(loss_ref)
        worst = max(worst, err / tol)
        print(f"[descent] sgd {gid} tv={with_tv} it {it}: |g_ref|inf {np.abs(g_ref).max():.3e}, step error {err:.3e} (bound {tol:.3e}), loss rel err {e_loss:.2e}")
        assert err <= tol, (gid, with_tv, it, err, tol)
        assert e_loss <= GRAD_TOL
    print(f"[descent] sgd {gid} tv={with_tv}: worst step error {worst:.3f} of its bound")
    del obj
    h.close()


# ---- 3. the 2-DoF entry --------------------------------------------------------------------------------------------------------------------
TWO_DOF_SIZE = (40, 56)
TWO_DOF = {
    "deferred": dict(cost="image_variance", sigma=0, theta0=(1.0, -1.0), weighted=False),  # K1 -> K3 -> k_finish_raw_step
    "general": dict(cost="gradient_magnitude", sigma=1, theta0=(2.5, -1.5), weighted=False),  # the normal sequence, then k_descent_step with nx 2
    "weighted": dict(cost="image_variance", sigma=0, theta0=(1.0, -1.0), weighted=True),
}
_TWO_DOF_EVENTS = []


def two_dof_events():
    if not _TWO_DOF_EVENTS:
        H, W = TWO_DOF_SIZE
        a = E.utils.generate_events(1500, H, W, 0.0, 0.05, seed=7)
        b = E.utils.generate_structured_events(2500, H, W, (4.0, -3.0), n_dots=12, tmin=0.0, tmax=0.05, seed=8)
        ev = np.concatenate([a, b])
        ev[:, 0], ev[:, 1] = np.clip(ev[:, 0], 0, H - 1), np.clip(ev[:, 1], 0, W - 1)
        _TWO_DOF_EVENTS.append(np.ascontiguousarray(ev[np.argsort(ev[:, 2], kind="stable")]))
    return _TWO_DOF_EVENTS[0]


def two_dof_weights(n):
    return np.random.default_rng(5).uniform(0.5, 1.0, n)


def two_dof_reference(case, theta):
    """fp64 (loss, gradient) at theta: tests/_hvp_ref.objective + autograd, tests/_weighted_ref.py on the weighted handle."""
    c, ev = TWO_DOF[case], two_dof_events()
    if c["weighted"]:
        out = weighted_objective(ev, np.asarray(theta), "2d-translation", TWO_DOF_SIZE, two_dof_weights(len(ev)), cost=c["cost"], sigma=c["sigma"])
        return float(out["loss"]), np.asarray(out["grad"], dtype=np.float64).reshape(-1)
    m = torch.tensor(np.asarray(theta, dtype=np.float64), requires_grad=True)
    loss = _hvp_ref.objective(torch.as_tensor(ev), m, "2d-translation", TWO_DOF_SIZE, cost=c["cost"], sigma=c["sigma"])
    (g,) = torch.autograd.grad(loss, m)
    return float(loss.detach()), g.numpy().copy()


def two_dof_setup(case):
    c, ev = TWO_DOF[case], two_dof_events()
    h = E.CMaxHandle(TWO_DOF_SIZE).set_events(ev)
    if c["weighted"]:
        h.set_event_weights(torch.as_tensor(two_dof_weights(len(ev)), device="cuda"))
    obj = E.ContrastObjective(h, "2d-translation", cost=c["cost"], sigma=c["sigma"])
    desc = obj.terms[0][2]
    # the deferred path is what cmax_objective takes for the plain variance without a blur on an unweighted default handle: the raw form
    # exists, and nothing that deferred_applies refuses holds (weights, deterministic mode, a blur, another cost)
    deferred = h.has_raw(desc) and not h.weighted and not h.deterministic and c["cost"] == "image_variance" and not c["sigma"]
    assert deferred == (case == "deferred")
    return h, obj


@pytest.mark.parametrize("mid", list(METHODS))
@pytest.mark.parametrize("case", list(TWO_DOF))
def test_two_dof_descent(case, mid):
    h, obj = two_dof_setup(case)
    theta0 = np.array(TWO_DOF[case]["theta0"])
    res = obj.descend(theta0, trace=True, **SCHEDULE, **METHODS[mid])
    check_bookkeeping(res, theta0)
    opt, state = ref_options(mid), {}
    for it in range(N_ITER):
        loss_ref, g_ref = two_dof_reference(case, res.trace[it])
        expected = _descent_ref.step(state, res.trace[it], g_ref, it, opt)
        e_loss = abs(res.loss_history[it] - loss_ref) / abs(loss_ref)
        if mid == "sgd":
            tol = _descent_ref.learning_rate(it, opt) * GRAD_TOL * np.abs(g_ref).max() / (1.0 - MOMENTUM)
            err = np.abs(res.trace[it + 1] - expected).max()
            print(f"[descent] 2-DoF {case} sgd it {it}: theta {res.trace[it]}, g_ref {g_ref}, step error {err:.3e} (bound {tol:.3e}), loss rel err {e_loss:.2e}")
            assert err <= tol, (case, it, err, tol)
        else:
            # every entry of the gradient is within 4e-4 relative by the 1e-4 gate once the entries are within a factor 4 of each other; the
            # step then carries the relative error of m plus half that of v: 2e-3 (a wrong bias correction moves step 2 by several per cent)
            ratio = np.abs(g_ref).max() / np.abs(g_ref).min()
            step, want = res.trace[it + 1] - res.trace[it], expected - res.trace[it]
            err = np.abs(step - want)
            print(f"[descent] 2-DoF {case} adam it {it}: theta {res.trace[it]}, g_ref {g_ref} (ratio {ratio:.2f}), step {step}, expected {want}, "
                  f"rel err {(err / np.abs(want)).max():.2e}, loss rel err {e_loss:.2e}")
            assert ratio <= 4.0, (case, it, ratio)
            assert (err <= 2e-3 * np.abs(want) + 1e-12).all(), (case, it, step, want)
        assert e_loss <= GRAD_TOL
    h.close()


@pytest.mark.parametrize("mid", list(METHODS))
@pytest.mark.parametrize("cost,sigma", [("image_variance", 0), ("normalized_gradient_magnitude", 1)], ids=["variance", "normalized-gm"])
def test_two_dof_rule_on_a_deterministic_handle(cost, sigma, mid):
    """Deterministic handles are allowed: the integer-accumulating sequence, then k_descent_step with nx = 2.  Bit-repeatable, so the
    traced iterates re-evaluated through cmax_objective give the bits the loop saw and the rule is held to fp64 rounding, as in 1."""
    h = E.CMaxHandle(TWO_DOF_SIZE).set_deterministic(True).set_events(two_dof_events())
    obj = E.ContrastObjective(h, "2d-translation", cost=cost, sigma=sigma)
    desc, theta0 = obj.terms[0][2], np.array([1.0, -1.0])
    h.evaluate(desc, torch.tensor(theta0, device="cuda"))  # (the evaluation's own lazy workspaces first)
    before = h.workspace_bytes
    res = obj.descend(theta0, trace=True, **SCHEDULE, **METHODS[mid])
    check_bookkeeping(res, theta0)
    state_bytes = 8 * (16 + 8 + 4 * 2 + N_ITER + (N_ITER + 1) * 2)  # theta | grad | result, control block, x_best | x_last | m | v, history, trace
    assert h.workspace_bytes - before == state_bytes  # handle-owned, counted in cmax_handle_info
    opt, state, e_x, e_loss = ref_options(mid), {}, 0.0, 0.0
    for it in range(N_ITER):
        result, grad = h.evaluate(desc, torch.tensor(res.trace[it], dtype=torch.float64, device="cuda"))
        loss, grad = float(result[0].item()), grad.cpu().numpy()
        expected = _descent_ref.step(state, res.trace[it], grad, it, opt)
        e_x = max(e_x, np.abs(res.trace[it + 1] - expected).max() / max(1.0, np.abs(expected).max()))
        e_loss = max(e_loss, abs(res.loss_history[it] - loss) / abs(loss))
    print(f"[descent] 2-DoF deterministic {cost} {mid}: moved {np.abs(res.x_last - theta0).max():.3e}, worst step error {e_x:.2e}, loss history {e_loss:.2e}")
    assert e_x <= 1e-10 and e_loss <= 1e-12
    again = obj.descend(theta0, trace=True, **SCHEDULE, **METHODS[mid])
    assert _bytes(again) == _bytes(res)
    h.close()


def test_plan_refusals():
    ev, spec, h, obj, x0 = plan_setup("3x4-odd", (27, 40), False)
    with pytest.raises(ValueError, match="elements"):
        obj.descend(x0[:-1])
    with pytest.raises(NotImplementedError, match="RMSprop"):
        obj.descend(x0, method="RMSprop")
    with pytest.raises(_lib.CmaxError, match="momentum"):
        obj.descend(x0, method="SGD", momentum=1.0)
    h.set_event_weights(np.full(len(ev), 0.5))  # a plan made before the handle received weights: refused like cmax_patch_plan_evaluate
    with pytest.raises(NotImplementedError, match="per-event weights"):
        obj.descend(x0, n_iter=2)
    h.set_event_weights(None)
    assert obj.descend(x0, n_iter=2).n_done == 2
    del obj
    h.close()


def test_two_dof_refusals():
    h, obj = two_dof_setup("deferred")
    desc = obj.terms[0][2]
    d = _lib.descent_descriptor("Adam", n_iter=3)
    dense = E.ContrastObjective(h, "dense-flow", cost="image_variance")
    with pytest.raises(NotImplementedError, match="2-DoF"):
        dense.descend(np.zeros(2))
    bad = _lib.CmaxObjective.from_buffer_copy(dense.terms[0][2])
    with pytest.raises(_lib.CmaxError, match="2-DoF descriptors only"):
        h.descend(bad, np.zeros(2), d)
    hybrid = E.ContrastObjective(h, "2d-translation", cost="hybrid", cost_with_weight={"image_variance": 1.0, "gradient_magnitude": 0.5})
    with pytest.raises(NotImplementedError, match="ONE fused term"):
        hybrid.descend(np.zeros(2))
    d.n_iter = 0
    with pytest.raises(_lib.CmaxError, match="n_iter"):
        h.descend(desc, np.array([1.0, -1.0]), d)
    h.close()


# ---- 4. the stop rule -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mid", list(METHODS))
def test_stop_rule_on_the_documented_nan(mid):
    """A scale_later plan at x = 0: max D = 0, loss and gradient are the reference's 0/0 (tests/test_gpu_scale_later.py::
    test_zero_motion_returns_nan).  No step is taken, the later evaluations run at the unchanged x, the call returns 0."""
    ev = batch((20, 32))
    spec = C.spec_of("3x4-odd", (20, 32), t_scale=float(ev[:, 2].max() - ev[:, 2].min()), scale_later=True, **_BURGERS)
    h, obj = make_objective(ev, spec)
    x0 = np.zeros(obj._nx)
    res = obj.descend(x0, trace=True, **SCHEDULE, **METHODS[mid])
    print(f"[descent] stop rule {mid}: n_done {res.n_done}, best_iter {res.best_iter}, best_loss {res.best_loss}, history {res.loss_history}")
    assert res.n_done == 0 and res.best_iter == -1 and res.best_loss == np.inf and res.last_lr == 0.0
    assert np.isnan(res.loss_history).all() and res.loss_history.shape == (N_ITER,)
    np.testing.assert_array_equal(res.x_last, x0)
    np.testing.assert_array_equal(res.x_best, x0)
    np.testing.assert_array_equal(res.trace, np.zeros((N_ITER + 1, obj._nx)))
    x1 = C.patch_motion("random", spec["patch_image_size"], 5)  # the plan is usable afterwards
    again = obj.descend(x1, trace=True, **SCHEDULE, **METHODS[mid])
    assert again.n_done == N_ITER and np.isfinite(again.loss_history).all()
    del obj
    h.close()


# ---- 5. state hygiene ----------------------------------------------------------------------------------------------------------------------
def _bytes(res):
    return (res.x_best.tobytes(), res.x_last.tobytes(), res.loss_history.tobytes(), res.trace.tobytes(), res.best_iter, res.n_done)


@pytest.mark.parametrize("variant", ["plain", "burgers"])
def test_state_hygiene(variant):
    kw = _BURGERS if variant == "burgers" else {}
    ev, spec, h, obj, x0 = plan_setup("3x4-odd", (27, 40), True, **kw)
    _, _, h2, fresh, _ = plan_setup("3x4-odd", (27, 40), True, **kw)
    v = np.random.default_rng(3).normal(size=x0.size)
    adam = obj.descend(x0, trace=True, **SCHEDULE, **METHODS["adam"])
    # evaluations and products after a descent are what a fresh plan returns
    loss, grad = obj.value_and_grad_numpy(x0)
    loss_f, grad_f = fresh.value_and_grad_numpy(x0)
    hv, hv_f = obj.hvp_numpy(x0, v), fresh.hvp_numpy(x0, v)
    e = (abs(loss - loss_f) / abs(loss_f), np.abs(grad - grad_f).max() / np.abs(grad_f).max(), np.abs(hv - hv_f).max() / np.abs(hv_f).max())
    print(f"[descent] hygiene {variant}: after a descent vs a fresh plan: loss {e[0]:.2e} grad {e[1]:.2e} Hv {e[2]:.2e}")
    assert max(e) <= 1e-12
    # the same call again: the same bytes
    assert _bytes(obj.descend(x0, trace=True, **SCHEDULE, **METHODS["adam"])) == _bytes(adam)
    # another method and n_iter behind it: no stale m / v, no stale history -- what a plan that never ran Adam gives
    short = dict(SCHEDULE, n_iter=3)
    assert _bytes(obj.descend(x0, trace=True, **short, **METHODS["sgd"])) == _bytes(fresh.descend(x0, trace=True, **short, **METHODS["sgd"]))
    longer = dict(SCHEDULE, n_iter=8)
    a, b = obj.descend(x0, trace=True, **longer, **METHODS["adam"]), fresh.descend(x0, trace=True, **longer, **METHODS["adam"])
    assert _bytes(a) == _bytes(b)
    np.testing.assert_array_equal(a.trace[: N_ITER + 1], adam.trace)  # (the schedule's first six iterations are the same)
    # without a trace: the same results
    quiet = obj.descend(x0, **SCHEDULE, **METHODS["adam"])
    assert quiet.trace is None and quiet.x_last.tobytes() == adam.x_last.tobytes() and quiet.loss_history.tobytes() == adam.loss_history.tobytes()
    del obj, fresh
    h.close()
    h2.close()


# ---- 6. the solver classes -----------------------------------------------------------------------------------------------------------------
PARAMS = {"trans_x": {"min": -150, "max": 150}, "trans_y": {"min": -150, "max": 150}}
COMMON = {"motion_model": "2d-translation", "warp_direction": "first", "parameters": ["trans_x", "trans_y"], "cost": "hybrid", "outer_padding": 0,
          "cost_with_weight": {"multi_focal_normalized_gradient_magnitude": 1.0, "total_variation": 0.01},
          "iwe": {"method": "bilinear_vote", "blur_sigma": 1}}
OPT_CFG = {"n_iter": 5, "method": "Adam", "max_iter": 25, "parameters": PARAMS}
SOLVER_SIZE = (66, 90)


def test_pyramid_solver_with_adam():
    ev = batch(SOLVER_SIZE)
    cfg = dict(COMMON, method="pyramidal_patch_contrast_maximization", time_aware=False,
               patch={"initialize": "random", "scale": 3, "crop_height": 64, "crop_width": 80, "filter_type": "bilinear"})
    slv = solver.collections["pyramidal_patch_contrast_maximization"](SOLVER_SIZE, {}, cfg, OPT_CFG, {}, None)
    slv._handle = E.CMaxHandle(SOLVER_SIZE).set_keep_outside(False).set_deterministic(True)  # bit-repeatable: the comparison below is exact
    np.random.seed(3)
    x0 = slv.initialize_random(slv.scaled_n_patch[1]).reshape(-1)  # what optimize() draws first
    np.random.seed(3)
    motion = slv.optimize(ev)
    assert sorted(motion) == [0, 1, 2] and motion[2].shape == (2, 4, 4) and motion[1].shape == (2, 2, 2)
    assert [s for s, _ in slv.history] == [1, 2]
    for s, res in slv.history:
        assert isinstance(res, _lib.DescentResult) and res.n_done == 5 and res.loss_history.shape == (5,)
        assert res.best_loss <= res.loss_history[0] and res.best_loss == res.loss_history.min()
    first = slv.history[0][1]
    direct = slv._objectives[1].descend(x0, method="Adam", n_iter=5)  # the reference's constants are descend's defaults
    print(f"[descent] pyramid + Adam: scale 1 loss {first.loss_history[0]:.6g} -> {first.best_loss:.6g} (iteration {first.best_iter}); "
          f"scale 2 {slv.history[1][1].loss_history[0]:.6g} -> {slv.history[1][1].best_loss:.6g}")
    assert first.x_best.tobytes() == direct.x_best.tobytes() and first.loss_history.tobytes() == direct.loss_history.tobytes()
    assert (direct.last_lr, first.last_lr) == (0.05, 0.05)  # StepLR(n_iter, 0.1): no decay inside the run


@pytest.mark.parametrize("time_aware", [False, True], ids=["mixed", "time-aware"])
def test_single_scale_solvers_with_adam(time_aware):
    ev = batch((68, 90))
    cfg = dict(COMMON, time_aware=time_aware, patch={"initialize": "random", "size": 16, "sliding_window": 16, "filter_type": "bilinear"})
    if time_aware:
        cfg.update(time_bin=10, flow_interpolation="burgers", t0_flow_location="middle")
    cls = solver.collections["time_aware_mixed_patch_contrast_maximization"] if time_aware else solver.MixedPatchContrastMaximization
    slv = cls((68, 90), {}, cfg, OPT_CFG, {}, None)
    np.random.seed(4)
    motion = slv.optimize(ev)
    res = slv.history[-1]
    assert motion.shape == (2,) + slv.patch_image_size and isinstance(res, _lib.DescentResult)
    np.testing.assert_array_equal(motion.reshape(-1), res.x_best)
    print(f"[descent] single-scale + Adam (time_aware={time_aware}): loss {res.loss_history[0]:.6g} -> {res.best_loss:.6g} at {res.best_iter}")
    assert res.n_done == 5 and res.best_loss <= res.loss_history[0]
