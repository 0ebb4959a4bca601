"""GPU tests of `solver.scale_later` (src/solver/base.py:219-224, src/solver/patch_contrast_pyramid.py:489-515): the flow is divided
by its signed maximum before the Burgers / upwind propagation and the voxel multiplied by it afterwards.  Loss, gradient and
Hessian-vector product of the native plan and of the autograd-chained path against tests/golden/solver_scale_later.npz = the
reference's objective_scipy with `scale_later: True` (gen_golden_scale_later.py), at the tolerances tests/test_gpu_solver.py uses
for the same quantities.  Every test prints the worst error it measured before it asserts.

No reference TRAJECTORY exists for the end-to-end run (the reference's optimiser depends on Optuna / skimage, absent where the
fixtures are made): test_pyramid_solver_runs_with_scale_later only asks for a finite loss that does not rise."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import event_based_optical_flow_amd as E  # noqa: E402
from event_based_optical_flow_amd.solver import PatchFlowObjective  # noqa: E402
from event_based_optical_flow_amd.solver import pyramid as P  # noqa: E402
from event_based_optical_flow_amd.solver.scipy_autograd import TorchWrapper  # noqa: E402

TOL = HVP_TOL = 1e-4  # tests/test_gpu_solver.py:16-17
YAML_HYBRID = {"multi_focal_normalized_gradient_magnitude": 1.0, "total_variation": 0.01}
CASES = ["burgers_s1", "burgers_s3", "interior_s3", "upwind_s1", "burgers_first_s1", "plateau_s3", "negative_s3"]
OPT_CFG = {"n_iter": 40, "method": "Newton-CG", "max_iter": 25,
           "parameters": {"trans_x": {"min": -150, "max": 150}, "trans_y": {"min": -150, "max": 150}}}


def rel_max(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max()


def solver_config(scale=4, **extra):
    cfg = {"method": "pyramidal_patch_contrast_maximization", "time_aware": True, "scale_later": True, "time_bin": 10,
           "flow_interpolation": "burgers", "t0_flow_location": "middle",
           "patch": {"initialize": "random", "scale": scale, "crop_height": 64, "crop_width": 80, "filter_type": "bilinear"},
           "motion_model": "2d-translation", "warp_direction": "first", "parameters": ["trans_x", "trans_y"], "cost": "hybrid",
           "outer_padding": 0, "cost_with_weight": YAML_HYBRID, "iwe": {"method": "bilinear_vote", "blur_sigma": 1}}
    cfg.update(extra)
    return cfg


def _scene(golden):
    g = golden("solver_objective")
    ev = g["events"]
    return tuple(int(v) for v in g["image_size"]), ev, float(ev[:, 2].max() - ev[:, 2].min())


def _objective(golden, case, handle=None, deterministic=False, **kw):
    gs = golden("solver_scale_later")
    size, ev, t_scale = _scene(golden)
    if handle is None:
        handle = E.CMaxHandle(size)
        if deterministic:
            handle.set_deterministic(True)
        handle.set_events(ev, time_bin=10)
    kw.setdefault("scale_later", True)
    return PatchFlowObjective(handle, t_scale, gs[case + "__patch_image_size"], gs[case + "__patch_size"], gs[case + "__sliding_window"],
                              gs[case + "__patch_shift"], cost="hybrid", cost_with_weight=YAML_HYBRID, blur_sigma=1, time_aware=True,
                              time_bin=10, flow_interpolation=str(gs[case + "__flow_interpolation"]),
                              t0_flow_location=str(gs[case + "__t0_flow_location"]), **kw)


def _ref(golden, case):
    gs = golden("solver_scale_later")
    return tuple(np.asarray(gs[f"{case}__{k}"], dtype=np.float64).reshape(-1) for k in ("x", "grad", "v", "vhp")) + (float(gs[case + "__loss"]),)


@pytest.mark.parametrize("case", CASES)
def test_native_plan_against_the_reference(golden, case):
    """cmax_patch_plan_evaluate / _hvp with scale_later: loss, gradient, exact Hessian-vector product."""
    obj = _objective(golden, case)
    assert obj.has_native_plan and obj.scale_later and obj.has_exact_hvp
    x, grad_ref, v, vhp_ref, loss_ref = _ref(golden, case)
    loss, grad = obj.value_and_grad_numpy(x)
    hv = obj.hvp_numpy(x, v)
    print(f"[scale_later] native {case}: loss rel err {abs(loss - loss_ref) / abs(loss_ref):.2e}, gradient {rel_max(grad, grad_ref):.2e}, "
          f"hvp {rel_max(hv, vhp_ref):.2e}")
    assert abs(loss - loss_ref) <= TOL * abs(loss_ref)
    assert rel_max(grad, grad_ref) <= TOL
    assert rel_max(hv, vhp_ref) <= HVP_TOL
    for _ in range(3):  # value only; repeated calls flip the handle's vote buffers
        loss_v, none = obj.value_and_grad_numpy(x, want_grad=False)
        assert none is None and abs(loss_v - loss) <= 1e-9 * abs(loss)
    assert rel_max(obj.hvp_numpy(x, 3.0 * v), 3.0 * vhp_ref) <= HVP_TOL  # linear in v
    assert np.array_equal(obj.hvp_numpy(x, np.zeros_like(v)), np.zeros_like(v))


@pytest.mark.parametrize("case", CASES)
def test_autograd_path_against_the_reference_and_the_native_plan(golden, case):
    """objective(x) + torch.autograd.grad: cmax_field_max and its adjoint chained with the interpolation and the voxel operator."""
    obj = _objective(golden, case)
    x, grad_ref, _, _, loss_ref = _ref(golden, case)
    xt = torch.tensor(x, dtype=torch.float64, device="cuda", requires_grad=True)
    loss_t = obj(xt)
    (grad_t,) = torch.autograd.grad(loss_t, xt)
    loss_a, grad_a = loss_t.item(), grad_t.cpu().numpy()
    loss_n, grad_n = obj.value_and_grad_numpy(x)
    print(f"[scale_later] autograd {case}: loss rel err {abs(loss_a - loss_ref) / abs(loss_ref):.2e}, gradient {rel_max(grad_a, grad_ref):.2e}; "
          f"native vs autograd: loss {abs(loss_n - loss_a) / abs(loss_a):.2e}, gradient {rel_max(grad_n, grad_a):.2e}")
    assert abs(loss_a - loss_ref) <= TOL * abs(loss_ref)
    assert rel_max(grad_a, grad_ref) <= TOL
    assert abs(loss_n - loss_a) <= 1e-6 * abs(loss_a)
    assert rel_max(grad_n, grad_a) <= 1e-5
    w = TorchWrapper(obj, precision="float64", device="cuda")
    w.get_input(x)
    loss_w, grad_w = w.get_value_and_grad(x)  # what scipy calls: the native plan
    assert abs(float(loss_w) - loss_n) <= 1e-6 * abs(loss_n) and rel_max(grad_w, grad_n) <= 1e-5


def test_field_max_leaf_operator():
    """cmax_field_max / _adj: signed maximum, ties share the gradient evenly (torch.Tensor.max), fp32 and fp64."""
    rng = np.random.default_rng(7)
    for dtype in (torch.float64, torch.float32):
        for sign in (1.0, -1.0):  # all-negative fields: the maximum is not the largest magnitude
            a = torch.tensor(sign * rng.uniform(0.5, 9.0, (2, 37, 53)), dtype=dtype, device="cuda")
            a[1, 5, 7:11] = a.max() + 0.25  # a plateau of four (still negative when sign < 0)
            a.requires_grad_()
            m = E.functional.field_max(a)
            (ga,) = torch.autograd.grad(m * 3.0, a)
            b = a.detach().clone().requires_grad_()
            (gb,) = torch.autograd.grad(b.max() * 3.0, b)
            assert m.item() == b.max().item() and m.dtype == dtype
            assert torch.equal(ga, gb) and ga.sum().item() == pytest.approx(3.0)


def test_graph_replay_reads_the_scale_from_device_memory(golden, monkeypatch):
    """CMAX_PLAN_GRAPHS=1: replayed evaluations at two x whose maxima sit on different pixels (and differ) equal the eager ones."""
    names = ["interior_s3", "burgers_s3", "negative_s3"]
    xs = [_ref(golden, c)[0] for c in names]
    v = _ref(golden, "interior_s3")[2]
    monkeypatch.delenv("CMAX_PLAN_GRAPHS", raising=False)
    eager_obj = _objective(golden, "interior_s3")
    assert eager_obj.native_plan_info() == (0, False)
    eager = [eager_obj.value_and_grad_numpy(x) + (eager_obj.hvp_numpy(x, v),) for x in xs]
    monkeypatch.setenv("CMAX_PLAN_GRAPHS", "1")
    obj = _objective(golden, "interior_s3")
    worst = [0.0, 0.0, 0.0]
    for rep in range(4):  # eager warm-up calls, then capture, then replay
        for x, (l_ref, g_ref, hv_ref) in zip(xs, eager):
            l, gr = obj.value_and_grad_numpy(x)
            hv = obj.hvp_numpy(x, v)
            lv, _ = obj.value_and_grad_numpy(x, want_grad=False)
            worst = [max(worst[0], abs(l - l_ref) / abs(l_ref)), max(worst[1], rel_max(gr, g_ref)), max(worst[2], rel_max(hv, hv_ref))]
            assert abs(lv - l) <= 1e-9 * abs(l)
    n_graphs, enabled = obj.native_plan_info()
    print(f"[scale_later] graph replay ({n_graphs} graphs) vs eager: loss {worst[0]:.2e}, gradient {worst[1]:.2e}, hvp {worst[2]:.2e}")
    assert enabled and n_graphs >= 2, (n_graphs, enabled)
    assert worst[0] <= 1e-6 and worst[1] <= 1e-5 and worst[2] <= 1e-5
    assert abs(eager[0][0] - eager[1][0]) > 1e-4 * abs(eager[0][0])  # the two x really differ


@pytest.mark.parametrize("case", CASES)
def test_motion_to_dense_flow_against_the_numpy_branch(golden, case):
    """The voxel the metrics and pictures use (numpy branch of patch_contrast_pyramid.py:489-504), on the fixture's pixel lattice.
    fp64 leaf operators: a relative 1e-11 of the largest entry, the class of test_patch_to_dense_golden -- ~1e5 ulp of headroom
    over an interpolation, one division, <= 9 propagation steps and two multiplications in fp64."""
    gs = golden("solver_scale_later")
    size, ev, t_scale = _scene(golden)
    s = int(gs[case + "__patch_scale"])
    slv = P.PyramidalPatchContrastMaximization(size, {}, solver_config(flow_interpolation=str(gs[case + "__flow_interpolation"]),
                                                                       t0_flow_location=str(gs[case + "__t0_flow_location"])), OPT_CFG, {}, None)
    motion = np.asarray(gs[case + "__x"]).reshape((2,) + tuple(int(v) for v in gs[case + "__patch_image_size"]))
    voxel = slv.motion_to_dense_flow({s: motion}, t_scale)
    assert voxel.shape == (10, 2) + size
    sh, sw = (int(v) for v in gs["vox_stride"])
    err = rel_max(voxel[..., ::sh, ::sw], gs[case + "__voxel_numpy"])
    print(f"[scale_later] motion_to_dense_flow {case}: rel err vs the numpy branch {err:.2e} "
          f"(tensor branch: {rel_max(voxel[..., ::sh, ::sw], gs[case + '__voxel_tensor']):.2e})")
    assert err <= 1e-11
    off = P.PyramidalPatchContrastMaximization(size, {}, solver_config(scale_later=False), OPT_CFG, {}, None).motion_to_dense_flow({s: motion}, t_scale)
    assert rel_max(off[..., ::sh, ::sw], gs[case + "__voxel_numpy"]) > 1e-3  # the flag changes the voxel


def test_flow_error_of_the_solver_class(golden):
    gs, g = golden("solver_scale_later"), golden("flow_error")
    H, W = (int(v) for v in g["image_size"])
    period = float(g["timescale"])
    s = int(g["burgers__scale"])
    best = {s: g["burgers__motion"]}
    slv = P.PyramidalPatchContrastMaximization((H, W), {}, solver_config(scale=3), OPT_CFG, {}, None)
    sh, sw = (int(v) for v in gs["vox_stride"])
    assert rel_max(slv.motion_to_dense_flow(best, period)[..., ::sh, ::sw], gs["flow_error__dense"]) <= TOL
    err = slv.calculate_flow_error(best, g["gt_flow"], period, g["events"])
    keys = [k[len("flow_error__mask__"):] for k in gs if k.startswith("flow_error__mask__")]
    assert {"EPE", "AE", "GT_FWL", "PRED_FWL"} <= set(keys)
    worst = max(abs(err[k] - float(gs["flow_error__mask__" + k])) / max(abs(float(gs["flow_error__mask__" + k])), 1e-3) for k in keys)
    print(f"[scale_later] calculate_flow_error: worst relative deviation {worst:.2e}")
    for k in keys:
        assert err[k] == pytest.approx(float(gs["flow_error__mask__" + k]), rel=TOL, abs=1e-3 * TOL), k
    nomask = slv.calculate_flow_error(best, g["gt_flow"], period)
    for k in (k[len("flow_error__nomask__"):] for k in gs if k.startswith("flow_error__nomask__")):
        assert nomask[k] == pytest.approx(float(gs["flow_error__nomask__" + k]), rel=TOL, abs=1e-3 * TOL), k
    assert slv.calculate_fwl_pred(best, g["events"], period)["PRED_FWL"] == pytest.approx(float(gs["flow_error__fwl_pred_only"]), rel=TOL)


def test_zero_motion_returns_nan(golden):
    """x = 0: max D = 0, the reference divides 0 by 0.  The call returns; the loss is NaN."""
    obj = _objective(golden, "burgers_s3")
    loss, _ = obj.value_and_grad_numpy(np.zeros(obj._nx))
    assert np.isnan(loss)


def test_deterministic_handle_is_bit_repeatable(golden):
    obj = _objective(golden, "plateau_s3", deterministic=True)
    x, _, v, _, _ = _ref(golden, "plateau_s3")
    outs = []
    for _ in range(2):
        loss, grad = obj.value_and_grad_numpy(x)
        outs.append((np.float64(loss).tobytes(), grad.tobytes(), obj.hvp_numpy(x, v).tobytes()))
    assert outs[0] == outs[1]


def test_scale_later_off_is_the_untouched_path(golden):
    """scale_later=False, and scale_later=True without time_aware, give bit for bit what a plan made without the field gives."""
    g = golden("solver_objective")
    size, ev, t_scale = _scene(golden)
    h = E.CMaxHandle(size)
    h.set_deterministic(True)
    h.set_events(ev, time_bin=10)
    x = np.asarray(g["burgers_s3__x"], dtype=np.float64).reshape(-1)
    v = np.random.default_rng(3).normal(size=x.shape)
    outs = []
    for kw in ({}, {"scale_later": False}):
        gs = golden("solver_scale_later")
        obj = PatchFlowObjective(h, t_scale, gs["burgers_s3__patch_image_size"], gs["burgers_s3__patch_size"], gs["burgers_s3__sliding_window"],
                                 gs["burgers_s3__patch_shift"], cost="hybrid", cost_with_weight=YAML_HYBRID, blur_sigma=1, time_aware=True,
                                 time_bin=10, flow_interpolation="burgers", t0_flow_location="middle", **kw)
        assert not obj.scale_later
        loss, grad = obj.value_and_grad_numpy(x)
        outs.append((np.float64(loss).tobytes(), grad.tobytes(), obj.hvp_numpy(x, v).tobytes()))
        assert abs(loss - float(g["burgers_s3__loss"])) <= TOL * abs(float(g["burgers_s3__loss"]))
        assert rel_max(grad, np.asarray(g["burgers_s3__grad"]).reshape(-1)) <= TOL
    assert outs[0] == outs[1]
    h2 = E.CMaxHandle(size).set_events(ev)
    k = "plain_s3"
    plain = PatchFlowObjective(h2, t_scale, g[k + "__patch_image_size"], g[k + "__patch_size"], g[k + "__sliding_window"], g["plain__patch_shift"],
                               cost="hybrid", cost_with_weight=YAML_HYBRID, blur_sigma=1, scale_later=True)
    assert not plain.scale_later  # ignored without time_aware, as in the reference
    loss, _ = plain.value_and_grad_numpy(np.asarray(g[k + "__x"]).reshape(-1))
    assert abs(loss - float(g[k + "__loss"])) <= TOL * abs(float(g[k + "__loss"]))


def test_time_sliced_batches_are_refused(golden):
    size, ev, _ = _scene(golden)
    h = E.CMaxHandle(size).set_events(ev, time_bin=10)
    with pytest.raises(NotImplementedError):
        _objective(golden, "burgers_s3", handle=h, sliced=object())


def test_pyramid_solver_runs_with_scale_later(monkeypatch):
    """optimize() on test_pyramid_solver_end_to_end's scene with scale_later: True: at every scale a finite loss, not above the loss
    of that scale's starting point."""
    H, W = 68, 90
    rng = np.random.default_rng(11)
    V = E.utils.generate_smooth_flow((H, W), 7.0, grid=3, seed=12)
    n, n_dots = 80_000, 500
    cx, cy = rng.uniform(4, H - 4, n_dots), rng.uniform(4, W - 4, n_dots)
    dot = rng.integers(0, n_dots, n)
    tau = np.sort(rng.uniform(0, 1, n))
    vx = V[0, cx.astype(int), cy.astype(int)][dot]
    vy = V[1, cx.astype(int), cy.astype(int)][dot]
    x = np.clip(np.round(cx[dot] + tau * vx + rng.normal(0, 0.4, n)), 0, H - 1)
    y = np.clip(np.round(cy[dot] + tau * vy + rng.normal(0, 0.4, n)), 0, W - 1)
    ev = np.stack([x, y, tau * 0.05, rng.integers(0, 2, n).astype(float)], 1)
    opt_cfg = {"n_iter": 40, "method": "Newton-CG", "max_iter": 25,
               "parameters": {"trans_x": {"min": -30, "max": 30}, "trans_y": {"min": -30, "max": 30}}}
    starts = []
    minimize = P.scipy_autograd.minimize

    def recording_minimize(objective, x0, **kw):
        starts.append(objective.value_and_grad_numpy(np.asarray(x0, dtype=np.float64))[0])
        return minimize(objective, x0, **kw)

    monkeypatch.setattr(P.scipy_autograd, "minimize", recording_minimize)
    np.random.seed(46)
    slv = E.solver.collections["pyramidal_patch_contrast_maximization"]((H, W), {}, solver_config(), opt_cfg, {}, None)
    best = slv.optimize(ev)
    assert sorted(best) == [0, 1, 2, 3] and all(o.scale_later for o in slv._objectives.values())
    assert len(starts) == len(slv.history) == 3
    for f0, (s, res) in zip(starts, slv.history):
        print(f"[scale_later] optimize, scale {s}: loss {f0:.6f} -> {float(res.fun):.6f}")
        assert np.isfinite(f0) and np.isfinite(res.fun) and float(res.fun) <= f0
    flow = slv.motion_to_dense_flow(best) * 0.05
    assert flow.shape == (10, 2, H, W) and np.isfinite(flow).all()
