"""Flow-basis plan on the device: the leaf kernels of csrc/cmax_basis_kernels.h (cmax_basis_to_dense), cmax_basis_plan_create and the
patch-plan calls on the plan it returns, and the Python layer (functional.basis_to_dense, solver.FlowBasisObjective).

What is held to what:
  1. the leaf kernels against numpy's fp64 einsum on the same numbers: forward to the rounding of an fp64 sum of K terms (both
     computations carry one: (2 K + 2) 2^-53 sum_k |theta_k B_k|, plus half an fp32 ulp where the output is fp32), adjoint to 1e-12 of the
     largest entry, one-hot cotangents EXACTLY (a product by one and sums with zeros), both bit-identical on a second call;
  2. the plan's loss and gradient against tests/_basis_ref.plan at the project's TOL = 1e-4 (of the largest entry, as every parity test
     here measures a field; and again with every entry divided by max|B_k|, so that no parametrisation hides an entry);
  3. the product against _basis_ref.plan(v=...) on batches without the events a cell border makes ambiguous, at the same 1e-4;
  4. bit-repeatability on a deterministic handle; the descent rule on such a handle (tests/_descent_ref.py);
  5. the Python layer, scipy's Newton-CG through TorchWrapper, the refusals.
Every figure is printed before it is asserted; the parity figures are collected in profiles/basis_plan_parity.txt by
tools/probe_basis_plan.py."""
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
from event_based_optical_flow_amd.solver import FlowBasisObjective, scipy_autograd  # noqa: E402

import _basis_cases as B  # noqa: E402
import _basis_gpu as G  # noqa: E402
import _basis_ref  # noqa: E402
import _descent_ref  # noqa: E402

TOL = 1e-4
HERE = os.path.dirname(os.path.abspath(__file__))
EPS64, EPS32 = 2.0 ** -53, 2.0 ** -24


def rel_max(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def dev(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


# ---- 1. leaf kernels ---------------------------------------------------------------------------------------------------------------------
def leaf_forward(theta, basis):
    K, _, H, W = basis.shape
    out = torch.full((2, H, W), 5.0, dtype=basis.dtype, device="cuda")
    _lib.check(_lib.load().cmax_basis_to_dense(theta.data_ptr(), basis.data_ptr(), F._code(basis), K, H, W, 0, out.data_ptr(), F._stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def leaf_adjoint(g, basis):
    K, _, H, W = basis.shape
    out = torch.full((K,), 5.0, dtype=torch.float64, device="cuda")
    _lib.check(_lib.load().cmax_basis_to_dense(g.data_ptr(), basis.data_ptr(), F._code(basis), K, H, W, 1, out.data_ptr(), F._stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("size", B.LEAF_SIZES, ids=[f"{h}x{w}" for h, w in B.LEAF_SIZES])
def test_leaf_kernels_against_fp64_einsum(size, dtype):
    H, W = size
    n = 2 * H * W
    for K in B.LEAF_K:
        rng = np.random.default_rng(100 * K + H)
        Bn = B.smooth_basis(K, size, 20 + K)  # exact in fp32: both dtypes hold these numbers
        theta = rng.normal(0.0, 3.0, K)
        g = B.C.f32(rng.normal(size=(2, H, W)))
        basis, th, gd = dev(Bn, dtype), dev(theta), dev(g, dtype)
        # forward
        ref = np.einsum("k,kchw->chw", theta, Bn)
        bound = (2 * K + 2) * EPS64 * np.einsum("k,kchw->chw", np.abs(theta), np.abs(Bn)) + (EPS32 * np.abs(ref) if dtype == torch.float32 else 0.0)
        out = leaf_forward(th, basis)
        worst = float((np.abs(out.astype(np.float64) - ref) / np.maximum(bound, 1e-300)).max())
        again = leaf_forward(th, basis)
        # adjoint
        aref = np.einsum("kchw,chw->k", Bn, g)
        adj = leaf_adjoint(gd, basis)
        e_adj = rel_max(adj, aref)
        adj_again = leaf_adjoint(gd, basis)
        # <B theta, g> = <theta, B^T g>, on the device's own numbers
        lhs, rhs = float((out.astype(np.float64) * g).sum()), float((theta * adj).sum())
        e_id = abs(lhs - rhs) / float(np.abs(out.astype(np.float64) * g).sum())
        print(f"[basis] leaf {size} K={K} {str(dtype)[6:]}: forward {worst:.2f} of its rounding bound, adjoint rel err {e_adj:.1e}, "
              f"<B theta, g> vs <theta, B^T g> {e_id:.1e}")
        assert worst <= 1.0 and e_adj <= 1e-12
        assert np.array_equal(out, again) and np.array_equal(adj, adj_again)
        assert e_id <= (1e-12 if dtype == torch.float64 else 1e-6)  # (fp32 output: the forward is rounded to fp32 once)
    # one-hot cotangents at the corners of both planes and on either side of every chunk seam: the adjoint returns a column of B exactly
    K = 7
    Bn = B.smooth_basis(K, size, 20 + K)
    basis = dev(Bn, dtype)
    flat = Bn.reshape(K, n)
    corners = [c * H * W + i * W + j for c in (0, 1) for i in (0, H - 1) for j in (0, W - 1)]
    picks = sorted(set(corners) | set(B.seam_elements(n)))
    for e in picks:
        g = torch.zeros(n, dtype=dtype, device="cuda")
        g[e] = 1.0
        assert np.array_equal(leaf_adjoint(g, basis), flat[:, e]), (size, e)
    print(f"[basis] leaf {size} {str(dtype)[6:]}: {len(picks)} one-hot cotangents exact (seams at multiples of {B.ADJ_CHUNK})")


def test_autograd_function_is_the_two_kernels():
    size, K = (27, 40), 6
    Bn = B.smooth_basis(K, size, 3)
    rng = np.random.default_rng(8)
    theta, g = rng.normal(size=K), rng.normal(size=(2,) + size)
    for dtype in (torch.float32, torch.float64):
        basis = dev(Bn, dtype)
        th = dev(theta).requires_grad_()
        out = F.basis_to_dense(th, basis)
        assert out.dtype == dtype and out.shape == (2,) + size
        (gt,) = torch.autograd.grad((out * dev(g, dtype)).sum(), th)
        assert gt.dtype == torch.float64
        e_f = rel_max(out.detach().cpu().numpy(), np.einsum("k,kchw->chw", theta, Bn))
        e_b = rel_max(gt.cpu().numpy(), np.einsum("kchw,chw->k", Bn, dev(g, dtype).cpu().numpy().astype(np.float64)))
        print(f"[basis] functional.basis_to_dense {str(dtype)[6:]}: forward {e_f:.1e} backward {e_b:.1e}")
        assert e_f <= (1e-15 if dtype == torch.float64 else 1e-7) and e_b <= 1e-12
    with pytest.raises(ValueError, match="fields"):
        F.basis_to_dense(dev(theta[:-1]), dev(Bn))
    with pytest.raises(ValueError, match="K, 2, H, W"):
        F.basis_to_dense(dev(theta), dev(Bn[:, 0]))


# ---- 2. plan evaluation ------------------------------------------------------------------------------------------------------------------
def plan_errors(b, loss, grad):
    bmax = np.abs(b["spec"]["basis"]).reshape(len(grad), -1).max(axis=1)
    return abs(loss - b["loss"]) / abs(b["loss"]), rel_max(grad, b["grad"]), rel_max(grad / bmax, b["grad"] / bmax)


@pytest.mark.parametrize("cid", list(B.PLAN))
def test_plan_value_and_gradient(cid):
    c = B.PLAN[cid]
    b = B.built_plan(c)
    h, obj = G.make_objective(c, b["ev"], b["spec"])
    loss, grad = obj.value_and_grad_numpy(b["theta"])
    e_loss, e_grad, e_scaled = plan_errors(b, loss, grad)
    per_entry = float((np.abs(grad - b["grad"]) / np.maximum(np.abs(b["grad"]), 1e-300)).max())
    print(f"[basis] plan {cid}: K {len(grad)}, rel err loss {e_loss:.2e} grad {e_grad:.2e} (per max|B_k|: {e_scaled:.2e}; worst single entry "
          f"relative to itself {per_entry:.2e})")
    assert e_loss <= TOL and e_grad <= TOL and e_scaled <= TOL, (cid, e_loss, e_grad, e_scaled)
    loss_v, none = obj.value_and_grad_numpy(b["theta"], want_grad=False)
    assert none is None and abs(loss_v - b["loss"]) <= TOL * abs(b["loss"])
    del obj
    h.close()


def test_plan_graph_replay_in_a_child_process():
    """CMAX_PLAN_GRAPHS=1 is read when a plan is created: a fresh process with it set, six evaluations and products (replayed from the
    fourth on), every one of them at the gate."""
    c = B.PLAN[B.GRAPH_CASE]
    b = B.built_plan(c)
    v = B.hvp_tangents(c, b["theta"])["random"]
    hv_ref = _basis_ref.plan(b["theta"], b["ev"], b["spec"], v=v)[2]
    env = dict(os.environ, CMAX_PLAN_GRAPHS="1")
    run = subprocess.run([sys.executable, os.path.join(HERE, "_basis_plan_worker.py"), c["id"]], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    out = json.loads(run.stdout.strip().splitlines()[-1])
    assert out["enabled"] and out["n_graphs"] >= 2, out["n_graphs"]
    worst = [0.0, 0.0, 0.0]
    for call in out["calls"]:
        e = plan_errors(b, call["loss"], np.array(call["grad"]))
        worst = [max(worst[0], e[0]), max(worst[1], e[1], e[2]), max(worst[2], rel_max(call["hv"], hv_ref))]
    # (the product here is on the unfiltered batch: measured, gated in test_plan_product on filtered ones)
    print(f"[basis] plan {c['id']}, graph replay ({out['n_graphs']} graphs): worst rel err loss {worst[0]:.2e} grad {worst[1]:.2e}; Hv {worst[2]:.2e}")
    assert worst[0] <= TOL and worst[1] <= TOL
    first = out["calls"][0]
    for call in out["calls"][1:]:  # a replayed sequence computes what the eager one did (fp32 atomics: run-to-run noise only)
        assert abs(call["loss"] - first["loss"]) <= 1e-6 * abs(first["loss"]) and rel_max(call["hv"], first["hv"]) <= 1e-3


# ---- 3. the product ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(B.HVP))
def test_plan_product(cid):
    c = B.HVP[cid]
    b = B.built_hvp(c)
    assert b["dropped"] <= B.DROP_CAP
    h, obj = G.make_objective(c, b["ev"], b["spec"])
    loss, grad = obj.value_and_grad_numpy(b["theta"])
    e_loss, e_grad, e_scaled = plan_errors(b, loss, grad)
    assert e_loss <= TOL and e_grad <= TOL and e_scaled <= TOL
    bmax = np.abs(b["spec"]["basis"]).reshape(len(grad), -1).max(axis=1)
    for name, v in b["v"].items():
        hv = obj.hvp_numpy(b["theta"], v)
        ref = b["hv"][name]
        if name == "zero":
            assert not np.any(hv) and not np.any(ref)
            continue
        e, e_s = rel_max(hv, ref), rel_max(hv / bmax, ref / bmax)
        print(f"[basis] product {cid} {name}: {len(b['ev'])} events (dropped {b['dropped']:.5f}), rel err Hv {e:.2e} (per max|B_k|: {e_s:.2e})")
        assert e <= TOL and e_s <= TOL, (cid, name, e, e_s)
    del obj
    h.close()


# ---- 4. deterministic handles --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["affine-27x40-two", "similarity-27x40-burgers", "K64-27x40-f32basis"])
def test_deterministic_handle_is_bit_repeatable(cid):
    c = B.PLAN[cid]
    ev, theta, spec = B.inputs(c)
    v = B.hvp_tangents(c, theta)["random"]
    h, obj = G.make_objective(c, ev, spec, deterministic=True)
    l0, g0 = obj.value_and_grad_numpy(theta)
    hv0 = obj.hvp_numpy(theta, v)
    l1, g1 = obj.value_and_grad_numpy(theta)
    hv1 = obj.hvp_numpy(theta, v)
    assert l0 == l1 and np.array_equal(g0, g1) and np.array_equal(hv0, hv1) and np.any(hv0)
    del obj
    h.close()


N_ITER, LR, LR_STEP, LR_DECAY, MOMENTUM = 6, 0.05, 2, 0.5, 0.9  # three learning rates occur (tests/test_gpu_descent.py)
METHODS = {"sgd": dict(method="SGD", momentum=MOMENTUM), "adam": dict(method="Adam")}


@pytest.mark.parametrize("mid", list(METHODS))
@pytest.mark.parametrize("cid", ["affine-27x40-two", "similarity-27x40-burgers"])
def test_descent_rule_on_a_bit_repeatable_handle(cid, mid):
    """Every traced iterate of `descend` re-evaluated on the same deterministic handle (the same bits the loop saw), the optimiser's state
    rebuilt with tests/_descent_ref.py: fp64 rounding and FMA contraction are all that separates the two."""
    c = B.PLAN[cid]
    ev, theta0, spec = B.inputs(c)
    h, obj = G.make_objective(c, ev, spec, deterministic=True)
    res = obj.descend(theta0, trace=True, n_iter=N_ITER, lr=LR, lr_step=LR_STEP, lr_decay=LR_DECAY, **METHODS[mid])
    assert res.trace.shape == (N_ITER + 1, theta0.size) and res.n_done == N_ITER and np.isfinite(res.loss_history).all()
    np.testing.assert_array_equal(res.trace[0], theta0)
    np.testing.assert_array_equal(res.x_last, res.trace[N_ITER])
    best, best_it = _descent_ref.best_of(res.loss_history)
    assert res.best_iter == best_it and res.best_loss == best
    np.testing.assert_array_equal(res.x_best, res.trace[best_it])
    kw = METHODS[mid]
    opt, state = _descent_ref.options(kw["method"], lr=LR, lr_step=LR_STEP, lr_decay=LR_DECAY, momentum=kw.get("momentum", 0.0)), {}
    e_x = e_loss = 0.0
    for it in range(N_ITER):
        loss, grad = obj.value_and_grad_numpy(res.trace[it])
        expected = _descent_ref.step(state, res.trace[it], grad, it, opt)
        e_x = max(e_x, np.abs(res.trace[it + 1] - expected).max() / max(1.0, np.abs(expected).max()))
        e_loss = max(e_loss, abs(res.loss_history[it] - loss) / abs(loss))
    moved = np.abs(res.x_last - theta0).max()
    print(f"[basis] descent rule {cid} {mid}: moved {moved:.3e}, worst step error {e_x:.2e} of max(1, |x|inf), loss history {e_loss:.2e}, "
          f"best {res.best_loss:.6g} at {res.best_iter}")
    assert moved > 0.0 and e_x <= 1e-10 and e_loss <= 1e-12
    del obj
    h.close()


# ---- 5. the Python layer -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["affine-27x40-two", "similarity-27x40-burgers", "K64-27x40-f32basis"])
def test_autograd_chained_path_agrees_with_the_plan(cid):
    c = B.PLAN[cid]
    b = B.built_plan(c)
    h, obj = G.make_objective(c, b["ev"], b["spec"])
    loss_n, grad_n = obj.value_and_grad_numpy(b["theta"])
    x = torch.tensor(b["theta"], dtype=torch.float64, device="cuda", requires_grad=True)
    loss = obj(x)
    (grad,) = torch.autograd.grad(loss, x)
    e_loss, e_grad = abs(loss.item() - loss_n) / abs(loss_n), rel_max(grad.cpu().numpy(), grad_n)
    r_loss, r_grad, _ = plan_errors(b, loss.item(), grad.cpu().numpy())
    print(f"[basis] autograd-chained {cid}: vs the plan loss {e_loss:.2e} grad {e_grad:.2e}; vs the reference loss {r_loss:.2e} grad {r_grad:.2e}")
    assert e_loss <= TOL and e_grad <= TOL and r_loss <= TOL and r_grad <= TOL
    flow = obj.dense_flow(x.detach())
    assert flow.shape == ((b["spec"]["T"], 2) if b["spec"]["time_aware"] else (2,)) + c["size"]
    assert rel_max(flow.cpu().numpy(), _basis_ref.device_motion(b["theta"], dict(b["spec"], round32=False))) <= 1e-6
    del obj
    h.close()


def test_model_names_inv_weights_and_other_arguments():
    size = (27, 40)
    ev = B.batch(size)
    t_scale = float(ev[:, 2].max() - ev[:, 2].min())
    h = E.CMaxHandle(size).set_events(ev)
    obj = FlowBasisObjective(h, t_scale, "affine", cost="image_variance")
    assert obj.has_native_plan and obj.basis.dtype == torch.float64 and tuple(obj.basis.shape) == (6, 2) + size
    theta = np.array(B.DISPLACEMENT["affine"]) / t_scale
    l0, g0 = obj.value_and_grad_numpy(theta)
    obj.set_t_scale(0.5 * t_scale)  # the same displacement field from twice the parameters
    l1, g1 = obj.value_and_grad_numpy(2.0 * theta)
    assert abs(l1 - l0) <= 1e-5 * abs(l0) and rel_max(2.0 * g1, g0) <= 1e-3
    assert obj.flow_bound(theta) == pytest.approx(float((np.abs(theta) * obj.bmax).sum()) * 0.5 * t_scale)
    for bad in (theta[:-1], np.zeros(7)):
        with pytest.raises(ValueError, match="fields"):
            obj.value_and_grad_numpy(bad)
        with pytest.raises(ValueError, match="fields"):
            obj.hvp_numpy(theta, bad)
        with pytest.raises(ValueError, match="fields"):
            obj.descend(bad, n_iter=2)
    rot = FlowBasisObjective(h, t_scale, "rotation", cost="image_variance", calib=(60.0, 60.0, 19.5, 13.0))
    assert rot.has_native_plan and np.isfinite(rot.value_and_grad_numpy(np.array([0.3, -0.2, 0.5]))[1]).all()
    inv = FlowBasisObjective(h, t_scale, "similarity", cost="hybrid", cost_with_weight={"image_variance": "inv", "gradient_magnitude": 1.0})
    assert not inv.has_native_plan and not inv.has_exact_hvp  # the fall-back: the autograd-chained path
    x = torch.tensor(np.array(B.DISPLACEMENT["similarity"]) / t_scale, dtype=torch.float64, device="cuda", requires_grad=True)
    (g,) = torch.autograd.grad(inv(x), x)
    assert g.shape == (4,) and bool(torch.isfinite(g).all()) and bool(g.abs().max() > 0)
    with pytest.raises(NotImplementedError, match="native plan"):
        inv.descend(np.zeros(4))
    with pytest.raises(ValueError, match="total_variation"):
        FlowBasisObjective(h, t_scale, "affine", cost="hybrid", cost_with_weight={"image_variance": 1.0, "total_variation": 0.01})
    with pytest.raises(ValueError, match="basis must be"):
        FlowBasisObjective(h, t_scale, np.zeros((3, 2, 5, 5)))
    with pytest.raises(ValueError, match="1 .. 64"):
        FlowBasisObjective(h, t_scale, np.zeros((65, 2) + size))
    del obj, rot, inv
    h.close()


def test_newton_cg_on_events_of_a_known_similarity():
    """scipy_autograd.minimize(..., "Newton-CG") through TorchWrapper, as for a PatchFlowObjective: events generated from a known
    similarity field, start at the true translation with zero zoom and rotation.  The end must be below the start and below the best
    pure translation; the parameter error is printed, not gated (nobody has measured it)."""
    size = B.SIM_SIZE
    ev = B.similarity_events()
    t_scale = float(ev[:, 2].max() - ev[:, 2].min())
    true = np.array(B.SIM_TRUE) / B.PERIOD
    h = E.CMaxHandle(size).set_events(ev)
    obj = FlowBasisObjective(h, t_scale, "similarity", cost="image_variance", blur_sigma=1.0)
    start = true * np.array([1.0, 1.0, 0.0, 0.0])
    loss_start = obj.value_and_grad_numpy(start)[0]
    res = scipy_autograd.minimize(obj, start, method="Newton-CG", precision="float64", torch_device="cuda", options={"maxiter": 30})
    loss_end = obj.value_and_grad_numpy(res.x)[0]
    trans = FlowBasisObjective(h, t_scale, "translation", cost="image_variance", blur_sigma=1.0)
    res_t = scipy_autograd.minimize(trans, start[:2], method="Newton-CG", precision="float64", torch_device="cuda", options={"maxiter": 30})
    loss_trans = min(trans.value_and_grad_numpy(res_t.x)[0], trans.value_and_grad_numpy(start[:2])[0])
    err = (res.x - true) * t_scale  # displacement over the batch: pixels for the translation, pixels per pixel for zoom and rotation
    print(f"[basis] Newton-CG similarity: loss {loss_start:.6g} at the start, {loss_trans:.6g} at the best pure translation, {loss_end:.6g} at the end "
          f"({res.nit} iterations, {res.nfev} evaluations, {res.nhev} products); parameter error x t_scale: translation {np.abs(err[:2]).max():.3f} px, "
          f"zoom {err[2]:+.4f}, rotation {err[3]:+.4f} (true {B.SIM_TRUE})")
    assert loss_end < loss_start and loss_end < loss_trans
    del obj, trans
    h.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def _create(h, d, basis):
    plan = ctypes.c_void_p()
    rc = _lib.load().cmax_basis_plan_create(h._h, ctypes.byref(d), basis.data_ptr(), F._stream(), ctypes.byref(plan))
    return rc, _lib.load().cmax_last_error() or b"", plan


def test_refusals_of_the_new_entries():
    size = (20, 28)
    ev = B.batch(size)
    t_scale = float(ev[:, 2].max() - ev[:, 2].min())
    h = E.CMaxHandle(size).set_events(ev)
    obj = FlowBasisObjective(h, t_scale, "affine", cost="image_variance")
    lib = _lib.load()
    big = torch.zeros((65, 2) + size, dtype=torch.float64, device="cuda")
    for K in (0, 65):
        d = obj._descriptor()
        d.K = K
        rc, msg, plan = _create(h, d, big)
        assert rc == _lib.EINVAL and b"K" in msg and not plan.value, (K, rc, msg)
    d = obj._descriptor()
    d.scale_later = 1
    rc, msg, plan = _create(h, d, obj.basis)
    assert rc == _lib.EINVAL and b"scale_later" in msg and not plan.value
    d = obj._descriptor()
    d.basis_dtype = 2
    rc, msg, plan = _create(h, d, obj.basis)
    assert rc == _lib.EINVAL and b"basis_dtype" in msg and not plan.value
    # the leaf entry
    out = torch.zeros((2,) + size, dtype=torch.float64, device="cuda")
    theta = torch.zeros(65, dtype=torch.float64, device="cuda")
    for K in (0, 65):
        assert lib.cmax_basis_to_dense(theta.data_ptr(), big.data_ptr(), _lib.F64, K, size[0], size[1], 0, out.data_ptr(), F._stream()) == _lib.EINVAL
        assert b"K" in lib.cmax_last_error()
    assert lib.cmax_basis_to_dense(theta.data_ptr(), big.data_ptr(), 2, 6, size[0], size[1], 0, out.data_ptr(), F._stream()) == _lib.EINVAL
    torch.cuda.synchronize()
    assert not bool(out.any())  # nothing was launched
    # a handle that holds a communicator
    h.comm_init(force_rccl=True)
    rc, msg, plan = _create(h, obj._descriptor(), obj.basis)
    assert rc == _lib.EUNSUPPORTED and b"communicator" in msg and not plan.value
    with pytest.raises(NotImplementedError, match="communicator"):
        FlowBasisObjective(h, t_scale, "affine", cost="image_variance")
    h.comm_destroy()
    # a weighted handle, at creation and (a plan made earlier) at every call
    h.set_event_weights(np.full(len(ev), 0.5))
    rc, msg, plan = _create(h, obj._descriptor(), obj.basis)
    assert rc == _lib.EUNSUPPORTED and b"per-event weights" in msg and not plan.value
    with pytest.raises(NotImplementedError, match="per-event weights"):
        FlowBasisObjective(h, t_scale, "affine", cost="image_variance")
    theta = np.array(B.DISPLACEMENT["affine"]) / t_scale
    with pytest.raises(NotImplementedError, match="per-event weights"):
        obj.value_and_grad_numpy(theta)
    h.set_event_weights(None)
    assert np.isfinite(obj.value_and_grad_numpy(theta)[0])
    assert lib.cmax_sizeof_basis_objective() == ctypes.sizeof(_lib.CmaxBasisObjective)
    del obj
    h.close()
