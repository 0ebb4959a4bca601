"""The event-collapse regularisers on the device, from the kernels up: the leaf operators cmax_flow_regularizer[_tan]
(csrc/cmax_flowreg_kernels.h), the term of a patch plan and of a basis plan (cmax_patch_plan_set_flow_regularizer: value, gradient,
exact product, descent, graph replay), functional.flow_regularizer, the objectives' keyword and the solver key.

What is held to what:
  1. leaf value, gradient and product against tests/_flowreg_ref.py (anchored by tests/test_flowreg_reference.py) on the same numbers:
     fp64 fields 1e-10, fp32 fields 1e-4 (the gates of tests/test_gpu_flow_chain.py), of the largest entry; the zero field and the
     divergence product at eps = 0 exactly; a one-hot bump next to every tile seam; two runs bit-equal;
  2. a plan with the term against the plan's own reference (tests/_mixed_ref.plan, tests/_basis_ref.plan) plus weight * R(t map x) in
     fp64, at the project's 1e-4 of the largest entry on loss, gradient and product;
  3. the descent against tests/_descent_ref.py stepping on the plan WITHOUT the term (the same deterministic handle: the bits the loop
     saw) plus the reference's term, at the tolerances of tests/test_gpu_basis_plan.py's descent case;
  4. set-then-removed and never-set plans bit-equal; the refusals; the Python layer; the solver classes.
Every figure is printed before it is asserted; tools/probe_flow_regularizer.py collects them in profiles/flow_regularizer_parity.txt."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import event_based_optical_flow_amd as E  # noqa: E402
from event_based_optical_flow_amd import _lib  # noqa: E402
from event_based_optical_flow_amd import functional as F  # noqa: E402
from event_based_optical_flow_amd.solver import FlowBasisObjective, PatchFlowObjective  # noqa: E402

import _basis_cases as B  # noqa: E402
import _basis_gpu as G  # noqa: E402
import _descent_ref  # noqa: E402
import _flowreg_cases as K  # noqa: E402
import _flowreg_ref as R  # noqa: E402
import _nearest_cases as N  # noqa: E402

TOL = 1e-4                                                 # the project's plain gate on a plan
LEAF_TOL = {torch.float64: 1e-10, torch.float32: 1e-4}     # tests/test_gpu_flow_chain.py
HERE = os.path.dirname(os.path.abspath(__file__))


def rel_max(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def dev(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


# ---- 1. the leaf operators -----------------------------------------------------------------------------------------------------------------
def leaf(Fd, kind, eps, s, dFd=None, want_grad=True):
    """-> (value, grad or None, hv or None) as numpy, from the C entries themselves (outputs pre-filled: every element must be written)."""
    lib, desc = _lib.load(), _lib.flow_regularizer_descriptor(kind, 123.0, eps, s)  # (the weight is ignored at the leaf)
    _, H, W = Fd.shape
    value = torch.full((1,), 5.0, dtype=torch.float64, device="cuda")
    grad = torch.full_like(Fd, 5.0) if want_grad else None
    _lib.check(lib.cmax_flow_regularizer(Fd.data_ptr(), F._code(Fd), H, W, ctypes.byref(desc), value.data_ptr(), F._ptr(grad), F._stream()))
    hv = None
    if dFd is not None:
        hv = torch.full_like(Fd, 5.0)
        _lib.check(lib.cmax_flow_regularizer_tan(Fd.data_ptr(), dFd.data_ptr(), F._code(Fd), H, W, ctypes.byref(desc), hv.data_ptr(), F._stream()))
    torch.cuda.synchronize()
    return value.item(), None if grad is None else grad.cpu().numpy(), None if hv is None else hv.cpu().numpy()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("size", K.SHAPES, ids=[f"{h}x{w}" for h, w in K.SHAPES])
def test_leaf_against_the_reference(size, dtype):
    tol = LEAF_TOL[dtype]
    worst = {"value": 0.0, "grad": 0.0, "hv": 0.0, "closed": 0.0}
    dF = K.tangent(size)
    dFd = dev(dF, dtype)
    for name, seed, kind, eps, s in K.leaf_cases(size):
        Fn = K.field(name, size, seed)  # exact in fp32: both dtypes (and the reference) hold these numbers
        Fd = dev(Fn, dtype)
        v_ref, g_ref = R.value_grad(Fn, kind, eps, s)
        hv_ref = R.product(Fn, dF, kind, eps, s)
        v, g, hv = leaf(Fd, kind, eps, s, dFd)
        v_only = leaf(Fd, kind, eps, s, want_grad=False)[0]
        assert v_only == v, "the value does not depend on whether a gradient is asked for"
        tag = (size, name, seed, kind, eps, s)
        if name == "zero":  # psi(0) = 0, psi'(0) = 0; the product of a zero field: psi''(0) du ua only
            assert v == 0.0 and not np.any(g), tag
        else:
            e_v, e_g = abs(v - v_ref) / abs(v_ref), rel_max(g, g_ref)
            worst["value"], worst["grad"] = max(worst["value"], e_v), max(worst["grad"], e_g)
            assert e_v <= tol and e_g <= tol, (tag, e_v, e_g)
        if name == "linear":
            e_c = abs(v - R.closed_form(K.LINEAR_M, kind, eps, s)) / R.closed_form(K.LINEAR_M, kind, eps, s)
            worst["closed"] = max(worst["closed"], e_c)
            assert e_c <= 1e-10, (tag, e_c)  # (the field is exact in fp32 and the arithmetic fp64 in both dtypes)
        if not np.any(hv_ref):
            assert not np.any(hv), tag  # the divergence at eps = 0: exactly zero
        else:
            e_h = rel_max(hv, hv_ref)
            worst["hv"] = max(worst["hv"], e_h)
            assert e_h <= tol, (tag, e_h)
    print(f"[flowreg] leaf {size} {str(dtype)[6:]}: {len(K.leaf_cases(size))} cases, worst rel err value {worst['value']:.1e} grad {worst['grad']:.1e} "
          f"product {worst['hv']:.1e}; linear field vs closed form {worst['closed']:.1e}")


def test_one_hot_bumps_at_every_tile_seam():
    """A smooth field plus a unit bump at one pixel: the gradient changes on the bump's 5 x 5 neighbourhood, across whatever seam lies
    there.  Every pixel on either side of a seam of the 3 x 3 tiles of a 17 x 65 field, the corners and the ring where Omega ends."""
    size = (17, 65)
    i, j = np.meshgrid(np.linspace(0.0, 1.0, size[0]), np.linspace(0.0, 1.0, size[1]), indexing="ij")
    base = np.stack([2.0 * np.sin(2.0 * i + j) + 0.3, 1.5 * np.cos(i - 1.5 * j) - 0.2])
    dF = K.tangent(size)
    dFd = dev(dF)
    worst = [0.0, 0.0]
    pixels = K.seam_pixels(size)
    for n, (r, c) in enumerate(pixels):
        Fn = base.copy()
        Fn[n % 2, r, c] += 1.0
        kind, eps, s = ("area", 1e-3, 0.5) if n % 3 else ("divergence", 1e-3, 1.0)
        _, g, hv = leaf(dev(Fn), kind, eps, s, dFd)
        e_g, e_h = rel_max(g, R.value_grad(Fn, kind, eps, s)[1]), rel_max(hv, R.product(Fn, dF, kind, eps, s))
        worst = [max(worst[0], e_g), max(worst[1], e_h)]
        assert e_g <= 1e-10 and e_h <= 1e-10, ((r, c), kind, e_g, e_h)
    print(f"[flowreg] one-hot bumps at {len(pixels)} pixels of {size}: worst rel err grad {worst[0]:.1e} product {worst[1]:.1e}")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_two_runs_are_bit_equal(dtype):
    size = (37, 53)
    Fd, dFd = dev(K.field("random", size), dtype), dev(K.tangent(size), dtype)
    for kind in R.KINDS:
        a, b = leaf(Fd, kind, 1e-3, 0.5, dFd), leaf(Fd, kind, 1e-3, 0.5, dFd)
        assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


# ---- 2. plans ------------------------------------------------------------------------------------------------------------------------------
def patch_objective(b):
    return N.make_objective(b["ev"], b["spec"], exact_flow=b["exact_flow"], filter_type=b["spec"]["filter"])


@pytest.mark.parametrize("pid", [p[0] for p in K.PATCH_PLANS])
def test_patch_plan_with_the_term(pid):
    b = K.built_patch(pid)
    h, obj = patch_objective(b)
    plain = obj.value_and_grad_numpy(b["x"])[0]
    obj.set_flow_regularizer(b["reg"])
    loss, grad = obj.value_and_grad_numpy(b["x"])
    hv = obj.hvp_numpy(b["x"], b["v"])
    loss_v = obj.value_and_grad_numpy(b["x"], want_grad=False)[0]
    e = (abs(loss - b["loss"]) / abs(b["loss"]), rel_max(grad, b["grad"]), rel_max(hv, b["hv"]["random"]))
    share = (abs(b["reg_loss"] / b["loss"]), np.abs(b["reg_grad"]).max() / np.abs(b["grad"]).max())
    print(f"[flowreg] patch plan {pid}: rel err loss {e[0]:.2e} grad {e[1]:.2e} Hv {e[2]:.2e} (the term is {share[0]:.1e} of the loss, "
          f"{share[1]:.1e} of the largest gradient entry; its value on the device {loss - plain:.9g}, reference {b['reg_loss']:.9g})")
    assert max(e) <= TOL, (pid, e)
    assert abs(loss_v - b["loss"]) <= TOL * abs(b["loss"])
    assert min(share) > 10.0 * TOL  # the gate sees the term
    del obj
    h.close()


@pytest.mark.parametrize("pid", [p[0] for p in K.BASIS_PLANS])
def test_basis_plan_with_the_term(pid):
    b = K.built_basis(pid)
    h, obj = G.make_objective(b["case"], b["ev"], b["spec"])
    obj.set_flow_regularizer(b["reg"])
    loss, grad = obj.value_and_grad_numpy(b["theta"])
    bmax = np.abs(b["spec"]["basis"]).reshape(len(grad), -1).max(axis=1)
    e = [abs(loss - b["loss"]) / abs(b["loss"]), rel_max(grad, b["grad"]), rel_max(grad / bmax, b["grad"] / bmax)]
    for name, v in b["v"].items():
        hv = obj.hvp_numpy(b["theta"], v)
        e += [rel_max(hv, b["hv"][name]), rel_max(hv / bmax, b["hv"][name] / bmax)]
    print(f"[flowreg] basis plan {pid}: K {len(grad)}, rel err loss {e[0]:.2e} grad {e[1]:.2e} (per max|B_k| {e[2]:.2e}) Hv {max(e[3:]):.2e}; "
          f"the term is {abs(b['reg_loss'] / b['loss']):.1e} of the loss")
    assert max(e) <= TOL, (pid, e)
    assert not np.any(obj.hvp_numpy(b["theta"], np.zeros_like(b["theta"])))
    del obj
    h.close()


def test_graph_replay_in_a_child_process():
    """CMAX_PLAN_GRAPHS=1 is read when a plan is created: a fresh process with it set; the term is set before the first call, six
    evaluations and products (replayed from the fourth on), then the term is removed (captured sequences are dropped) and the plain
    plan evaluated six times more."""
    b = K.built_basis(K.GRAPH_PLAN)
    env = dict(os.environ, CMAX_PLAN_GRAPHS="1")
    run = subprocess.run([sys.executable, os.path.join(HERE, "_flowreg_plan_worker.py"), K.GRAPH_PLAN], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    out = json.loads(run.stdout.strip().splitlines()[-1])
    assert out["enabled"] and out["n_graphs"] >= 2 and out["n_graphs_after_removal"] == 0 and out["n_graphs_plain"] >= 2, out
    worst = [0.0, 0.0, 0.0]
    for call in out["calls"]:
        worst = [max(worst[0], abs(call["loss"] - b["loss"]) / abs(b["loss"])), max(worst[1], rel_max(call["grad"], b["grad"])),
                 max(worst[2], rel_max(call["hv"], b["hv"]["random"]))]
    plain = B.built_hvp(b["case"])
    worst_plain = max(max(abs(c["loss"] - plain["loss"]) / abs(plain["loss"]), rel_max(c["grad"], plain["grad"])) for c in out["plain"])
    print(f"[flowreg] graph replay {K.GRAPH_PLAN} ({out['n_graphs']} graphs): worst rel err loss {worst[0]:.2e} grad {worst[1]:.2e} Hv {worst[2]:.2e}; "
          f"after removal {worst_plain:.2e}")
    assert max(worst) <= TOL and worst_plain <= TOL


# ---- 3. the descent ------------------------------------------------------------------------------------------------------------------------
N_ITER, LR, LR_STEP, LR_DECAY, MOMENTUM = 6, 0.05, 2, 0.5, 0.9
METHODS = {"sgd": dict(method="SGD", momentum=MOMENTUM), "adam": dict(method="Adam")}


@pytest.mark.parametrize("mid", list(METHODS))
@pytest.mark.parametrize("cid,reg", [("affine-27x40-two", "area"), ("similarity-27x40-burgers", "divergence")])
def test_descent_carries_the_term(cid, reg, mid):
    """`descend` with the term, traced; then the term is removed and every traced iterate re-evaluated on the same deterministic handle
    (the bits the loop saw of the fused terms), the reference's weight * R and its gradient added in fp64 on the host, and the optimiser
    stepped by tests/_descent_ref.py.  Both plans take the fp64 accumulate path with and without the term, so fp64 rounding is all that
    separates the two: the tolerances of tests/test_gpu_basis_plan.py's descent case."""
    c, reg = B.PLAN[cid], K.REGS[reg]
    ev, theta0, spec = B.inputs(c)
    dense_of = K.basis_map(spec)
    h, obj = G.make_objective(c, ev, spec, deterministic=True)
    obj.set_flow_regularizer(reg)
    kw = METHODS[mid]
    res = obj.descend(theta0, trace=True, n_iter=N_ITER, lr=LR, lr_step=LR_STEP, lr_decay=LR_DECAY, **kw)
    assert res.trace.shape == (N_ITER + 1, theta0.size) and res.n_done == N_ITER and np.isfinite(res.loss_history).all()
    obj.set_flow_regularizer(None)
    plain = obj.descend(theta0, trace=True, n_iter=N_ITER, lr=LR, lr_step=LR_STEP, lr_decay=LR_DECAY, **kw)
    assert np.abs(plain.trace[-1] - res.trace[-1]).max() > 1e-6  # the term moved the trajectory
    opt, state = _descent_ref.options(kw["method"], lr=LR, lr_step=LR_STEP, lr_decay=LR_DECAY, momentum=kw.get("momentum", 0.0)), {}
    e_x = e_loss = 0.0
    for it in range(N_ITER):
        loss, grad = obj.value_and_grad_numpy(res.trace[it])
        r_loss, r_grad, _ = R.plan_term(res.trace[it], dense_of, reg, spec["t_scale"])
        expected = _descent_ref.step(state, res.trace[it], grad + r_grad, it, opt)
        e_x = max(e_x, np.abs(res.trace[it + 1] - expected).max() / max(1.0, np.abs(expected).max()))
        e_loss = max(e_loss, abs(res.loss_history[it] - (loss + r_loss)) / abs(loss + r_loss))
    best, best_it = _descent_ref.best_of(res.loss_history)
    print(f"[flowreg] descent {cid} {mid}: worst step error {e_x:.2e} of max(1, |x|inf), loss history {e_loss:.2e}; the term moved the end point by "
          f"{np.abs(plain.trace[-1] - res.trace[-1]).max():.2e}")
    assert res.best_iter == best_it and res.best_loss == best
    assert e_x <= 1e-10 and e_loss <= 1e-12
    del obj
    h.close()


# ---- 4. no term = the plan as it was ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["affine-27x40-two", "similarity-27x40-exact-one", "similarity-27x40-burgers"])
def test_removed_and_never_set_are_bit_equal(cid):
    c = B.PLAN[cid]
    ev, theta, spec = B.inputs(c)
    v = B.hvp_tangents(c, theta)["random"]
    h, never = G.make_objective(c, ev, spec, deterministic=True)
    l0, g0 = never.value_and_grad_numpy(theta)
    hv0 = never.hvp_numpy(theta, v)
    obj = never  # the same plan from here on: set, compare, remove
    obj.set_flow_regularizer(K.REGS["area"])
    l1, g1 = obj.value_and_grad_numpy(theta)
    assert l1 != l0 and not np.array_equal(g1, g0)
    for removal in (None, {"kind": 0}):
        obj.set_flow_regularizer(K.REGS["divergence"])
        if removal is None:
            obj.set_flow_regularizer(None)
        else:  # kind 0 through the C entry
            d = _lib.CmaxFlowRegularizer()
            _lib.check(_lib.load().cmax_patch_plan_set_flow_regularizer(obj._plan, ctypes.byref(d)))
            obj.flow_reg = None
        l2, g2 = obj.value_and_grad_numpy(theta)
        hv2 = obj.hvp_numpy(theta, v)
        assert l2 == l0 and np.array_equal(g2, g0) and np.array_equal(hv2, hv0), (cid, removal)
    del obj, never
    h.close()


def test_with_the_term_a_deterministic_handle_is_bit_repeatable():
    c = B.PLAN["similarity-27x40-burgers"]
    ev, theta, spec = B.inputs(c)
    v = B.hvp_tangents(c, theta)["random"]
    h, obj = G.make_objective(c, ev, spec, deterministic=True)
    obj.set_flow_regularizer(K.REGS["area"])
    a = obj.value_and_grad_numpy(theta) + (obj.hvp_numpy(theta, v),)
    b = obj.value_and_grad_numpy(theta) + (obj.hvp_numpy(theta, v),)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    del obj
    h.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    lib = _lib.load()
    size = (20, 28)
    ev = B.batch(size)
    t_scale = float(ev[:, 2].max() - ev[:, 2].min())
    h = E.CMaxHandle(size).set_events(ev)
    obj = FlowBasisObjective(h, t_scale, "affine", cost="image_variance")
    theta = np.array(B.DISPLACEMENT["affine"]) / t_scale

    def rc_of(**kw):
        d = _lib.CmaxFlowRegularizer()
        d.kind, d.weight, d.eps, d.s = kw.get("kind", 2), kw.get("weight", 1.0), kw.get("eps", 0.0), kw.get("s", 1.0)
        return lib.cmax_patch_plan_set_flow_regularizer(obj._plan, ctypes.byref(d))

    for bad in (dict(kind=3), dict(kind=-1), dict(eps=-1.0), dict(s=0.0), dict(eps=float("nan")), dict(s=float("inf")), dict(weight=float("nan"))):
        assert rc_of(**bad) == _lib.EINVAL, bad
    plain = obj.value_and_grad_numpy(theta)[0]  # (a refused descriptor left the plan as it was)
    assert rc_of(kind=2, eps=1e-3) == 0 and obj.value_and_grad_numpy(theta)[0] != plain
    # the leaf entries launch nothing when they refuse
    out = torch.zeros((2, 5, 5), dtype=torch.float64, device="cuda")
    d = _lib.flow_regularizer_descriptor("area")
    d.eps = -1.0
    assert lib.cmax_flow_regularizer(out.data_ptr(), _lib.F64, 5, 5, ctypes.byref(d), out.data_ptr(), out.data_ptr(), F._stream()) == _lib.EINVAL
    assert lib.cmax_flow_regularizer(out.data_ptr(), _lib.F64, 2, 5, ctypes.byref(_lib.flow_regularizer_descriptor("area")), out.data_ptr(), out.data_ptr(),
                                     F._stream()) == _lib.EINVAL
    torch.cuda.synchronize()
    assert not bool(out.any())
    # a communicator that arrives later: evaluate, hvp and descend refuse; and the setter refuses on such a handle
    h.comm_init(force_rccl=True)
    for call in (lambda: obj.value_and_grad_numpy(theta), lambda: obj.hvp_numpy(theta, np.ones(6)), lambda: obj.descend(theta, n_iter=2)):
        with pytest.raises(NotImplementedError, match="communicator"):
            call()
    assert rc_of(kind=0) == 0  # removing is always allowed
    assert rc_of(kind=1) == _lib.EUNSUPPORTED and b"communicator" in lib.cmax_last_error()
    h.comm_destroy()
    assert obj.value_and_grad_numpy(theta)[0] == pytest.approx(plain, rel=1e-6)
    del obj
    h.close()
    # scale_later: the library and the Python layer both say why
    b = N.built("burgers-scale-later", "bilinear")
    h, sl = N.make_objective(b["ev"], b["spec"], filter_type="bilinear")
    d = _lib.flow_regularizer_descriptor("area")
    assert lib.cmax_patch_plan_set_flow_regularizer(sl._plan, ctypes.byref(d)) == _lib.EINVAL and b"scale_later" in lib.cmax_last_error()
    with pytest.raises(ValueError, match="scale_later"):
        sl.set_flow_regularizer({"kind": "area"})
    del sl
    h.close()


# ---- 6. the Python layer -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("kind,eps,s", [("divergence", 1e-3, 1.0), ("area", 1e-2, 0.5), ("area", 0.0, 1.0)])
def test_functional_is_differentiable_twice(kind, eps, s, dtype):
    size = (9, 33)
    tol = LEAF_TOL[dtype]
    Fn, vn = K.field("random", size), K.tangent(size)
    x = dev(Fn, dtype).requires_grad_()
    val = F.flow_regularizer(x, kind, eps, s)
    assert val.dim() == 0 and val.dtype == dtype
    (g,) = torch.autograd.grad(val, x)
    v_ref, g_ref = R.value_grad(Fn, kind, eps, s)
    hv_ref = R.product(Fn, vn, kind, eps, s)
    _, hv = torch.autograd.functional.vhp(lambda t: F.flow_regularizer(t, kind, eps, s), dev(Fn, dtype), dev(vn, dtype))
    # ... and through a chain: the gradient of 3 R(2 x)^2 with create_graph, differentiated again along v
    y = dev(Fn, dtype).requires_grad_()
    r = F.flow_regularizer(2.0 * y, kind, eps, s)
    (gy,) = torch.autograd.grad(3.0 * r * r, y, create_graph=True)
    (hy,) = torch.autograd.grad((gy * dev(vn, dtype)).sum(), y)
    r2, g2 = R.value_grad(2.0 * Fn, kind, eps, s)
    h2 = R.product(2.0 * Fn, vn, kind, eps, s)
    hy_ref = 6.0 * (4.0 * float((g2 * vn).sum()) * g2 + r2 * 4.0 * h2)  # d/dx [6 r 2 g2] along v, r = R(2x): dr = 2 <g2, v>, dg2 = 2 h2
    e = (abs(val.item() - v_ref) / abs(v_ref), rel_max(g.cpu().numpy(), g_ref), rel_max(hv.cpu().numpy(), hv_ref), rel_max(hy.cpu().numpy(), hy_ref))
    print(f"[flowreg] functional {kind} eps {eps} s {s} {str(dtype)[6:]}: value {e[0]:.1e} grad {e[1]:.1e} vhp {e[2]:.1e} chained second order {e[3]:.1e}")
    assert max(e) <= tol
    if dtype == torch.float64 and eps > 0.0:  # gradcheck-style: the analytic gradient against central differences of the device's own value
        rng = np.random.default_rng(3)
        for _ in range(8):
            w = K.C.f32(rng.normal(size=Fn.shape))
            hstep = 1e-6
            vp = F.flow_regularizer(dev(Fn + hstep * w), kind, eps, s).item()
            vm = F.flow_regularizer(dev(Fn - hstep * w), kind, eps, s).item()
            want = float((g.cpu().numpy() * w).sum())
            assert abs((vp - vm) / (2.0 * hstep) - want) <= 1e-6 * abs(want)


def test_objectives_agree_between_call_and_plan():
    """`__call__` (autograd-chained, the term from functional.flow_regularizer) and value_and_grad_numpy (the plan's term) return the
    same number; the keyword at construction is the setter."""
    b = K.built_patch("bilinear-area")
    h, obj = patch_objective(b)
    spec = b["spec"]
    shift = tuple(max(spec["pad"][k] - 1, 0) * spec["sw"][k] for k in (0, 1))
    kw_obj = PatchFlowObjective(h, spec["t_scale"], spec["patch_image_size"], spec["sw"], spec["sw"], shift, cost="hybrid",
                                cost_with_weight=dict({n: w for n, w in spec["terms"]}, total_variation=spec["tv_weight"]), blur_sigma=spec["sigma"],
                                omit_boundary=spec["omit"], flow_regularizer=b["reg"])
    obj.set_flow_regularizer(b["reg"])
    assert kw_obj.has_native_plan and kw_obj.has_exact_hvp and obj.has_exact_hvp
    loss_n, grad_n = obj.value_and_grad_numpy(b["x"])
    loss_k, grad_k = kw_obj.value_and_grad_numpy(b["x"])
    x = torch.tensor(b["x"], dtype=torch.float64, device="cuda", requires_grad=True)
    loss = obj(x)
    (grad,) = torch.autograd.grad(loss, x)
    hv_t = obj.hvp(x.detach(), dev(b["v"])).cpu().numpy()  # the autograd-chained product carries the term too
    e = (abs(loss.item() - loss_n) / abs(loss_n), rel_max(grad.cpu().numpy(), grad_n), abs(loss_k - loss_n) / abs(loss_n), rel_max(grad_k, grad_n),
         rel_max(hv_t, obj.hvp_numpy(b["x"], b["v"])))
    print(f"[flowreg] PatchFlowObjective: __call__ vs plan loss {e[0]:.2e} grad {e[1]:.2e}; keyword vs setter loss {e[2]:.2e} grad {e[3]:.2e}; "
          f"tensor hvp vs plan {e[4]:.2e}")
    assert max(e) <= TOL and abs(loss.item() - b["loss"]) <= TOL * abs(b["loss"])
    del obj, kw_obj
    h.close()
    for pid in ("affine-area", "similarity-burgers-area"):
        b = K.built_basis(pid)
        h, obj = G.make_objective(b["case"], b["ev"], b["spec"])
        obj.set_flow_regularizer(b["reg"])
        loss_n, grad_n = obj.value_and_grad_numpy(b["theta"])
        x = torch.tensor(b["theta"], dtype=torch.float64, device="cuda", requires_grad=True)
        loss = obj(x)
        (grad,) = torch.autograd.grad(loss, x)
        e = (abs(loss.item() - loss_n) / abs(loss_n), rel_max(grad.cpu().numpy(), grad_n))
        print(f"[flowreg] FlowBasisObjective {pid}: __call__ vs plan loss {e[0]:.2e} grad {e[1]:.2e}")
        assert max(e) <= TOL and obj.has_exact_hvp
        del obj
        h.close()


# ---- 7. the solver classes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pyramid", "mixed", "time-aware"])
def test_solver_classes_with_and_without_the_key(kind, monkeypatch):
    """One optimize() per solver class with solver.flow_regularizer: finite flow, and the term reached every objective's plan.  Without
    the key: not one set_flow_regularizer call, library or Python."""
    calls = []
    real = PatchFlowObjective.set_flow_regularizer
    monkeypatch.setattr(PatchFlowObjective, "set_flow_regularizer", lambda self, cfg: calls.append(cfg) or real(self, cfg))
    size = (66, 90) if kind == "pyramid" else (68, 90)
    ev = E.utils.generate_structured_events(6000, size[0], size[1], (4.2, -2.7), n_dots=40, tmin=0.0, tmax=0.05, seed=22)
    ev = np.ascontiguousarray(ev[np.argsort(ev[:, 2], kind="stable")])
    plain = K.make_solver(kind, None)
    best_plain = plain.optimize(ev)
    assert calls == []
    slv = K.make_solver(kind, K.REG)
    best = slv.optimize(ev)
    assert calls and all(c == K.REG for c in calls)
    flow, flow_plain = slv.motion_to_dense_flow(best), plain.motion_to_dense_flow(best_plain)
    assert np.isfinite(flow).all() and flow.shape == flow_plain.shape
    print(f"[flowreg] solver {kind}: {len(calls)} objective(s) carry the term; max |flow| {np.abs(flow).max():.4g} (without the key {np.abs(flow_plain).max():.4g})")
