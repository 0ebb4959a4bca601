"""Depth plan on the device: the leaf kernels of csrc/cmax_depth_kernels.h (cmax_depth_to_dense, _tan, _adj, _adj2), cmax_depth_plan_create
and the patch-plan calls on the plan it returns, and the Python layer (functional.depth_to_dense, solver.DepthEgoMotionObjective).

The error of a field is measured as tests/test_gpu_basis_plan.py measures it: the largest difference over the largest entry of the
reference (`rel_max`); a vector of unknowns x = [a | b | s] is measured as a whole AND block by block, so that the block with the largest
entries hides no other.  Gates, the project's: the fp64 leaf 1e-10, the fp32 leaf and every quantity of a plan 1e-4.  References:
tests/_depth_ref.py (torch fp64 on the CPU; Q is tests/_patch_ref.patch_to_dense), anchored in tests/test_depth_reference.py.
Every figure is printed before it is asserted; tools/probe_depth_plan.py collects the worst per family in profiles/depth_plan_parity.txt."""
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
from event_based_optical_flow_amd.solver import DepthEgoMotionObjective  # noqa: E402

import _depth_cases as D  # noqa: E402
import _depth_gpu as G  # noqa: E402
import _depth_ref  # noqa: E402
import _descent_ref  # noqa: E402
import _flowreg_ref  # noqa: E402
import _patch_cases as C  # noqa: E402

TOL = 1e-4
LEAF_TOL = {torch.float64: 1e-10, torch.float32: 1e-4}
HERE = os.path.dirname(os.path.abspath(__file__))


def rel_max(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def blocks(x, Ka, Kb):
    return [x[:Ka], x[Ka:Ka + Kb], x[Ka + Kb:]] if Kb else [x[:Ka], x[Ka + Kb:]]


def rel_blocks(got, want, Ka, Kb):
    """The worst of `rel_max` over the whole vector and over each of its blocks a, b, s (a block the reference leaves at zero must be zero)."""
    worst = rel_max(got, want)
    for g, w in zip(blocks(np.asarray(got), Ka, Kb), blocks(np.asarray(want), Ka, Kb)):
        if np.any(w):
            worst = max(worst, rel_max(g, w))
        else:
            assert not np.any(g)
    return worst


def dev(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


# ---- 1. leaf kernels ---------------------------------------------------------------------------------------------------------------------
class Leaf:
    """The four leaf entries on one geometry and one pair of bases, every buffer pre-filled so that an element left unwritten shows."""

    def __init__(self, spec, dtype):
        self.spec, self.dtype = spec, dtype
        self.A, self.B = dev(spec["A"], dtype), dev(spec["B"], dtype)
        self.Ka, self.Kb = spec["A"].shape[0], spec["B"].shape[0]
        self.geo = D.geometry_six(spec)
        self.size = spec["size"]
        self.ns = self.geo[0] * self.geo[1]
        self.lib = _lib.load()

    def _ints(self):
        return (F._code(self.A), self.Ka, self.Kb) + self.geo + tuple(self.size)

    def _split(self, x):
        x = dev(x)
        return x[:self.Ka].contiguous(), x[self.Ka:self.Ka + self.Kb].contiguous(), x[self.Ka + self.Kb:].contiguous()

    def _bp(self, t):
        return t.data_ptr() if self.Kb else None

    def forward(self, x):
        a, b, s = self._split(x)
        out = torch.full((2,) + tuple(self.size), 5.0, dtype=self.dtype, device="cuda")
        _lib.check(self.lib.cmax_depth_to_dense(a.data_ptr(), self._bp(b), s.data_ptr(), self.A.data_ptr(), self._bp(self.B), *self._ints(), out.data_ptr(),
                                                F._stream()))
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def tangent(self, x, u):
        a, b, s = self._split(x)
        da, db, ds = self._split(u)
        out = torch.full((2,) + tuple(self.size), 5.0, dtype=self.dtype, device="cuda")
        _lib.check(self.lib.cmax_depth_to_dense_tan(a.data_ptr(), s.data_ptr(), da.data_ptr(), self._bp(db), ds.data_ptr(), self.A.data_ptr(), self._bp(self.B),
                                                    *self._ints(), out.data_ptr(), F._stream()))
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def _outs(self):
        return (torch.full((self.Ka,), 5.0, dtype=torch.float64, device="cuda"), torch.full((max(self.Kb, 1),), 5.0, dtype=torch.float64, device="cuda"),
                torch.full((self.ns,), 5.0, dtype=torch.float64, device="cuda"))

    def _join(self, oa, ob, os_):
        torch.cuda.synchronize()
        return np.concatenate([oa.cpu().numpy(), ob.cpu().numpy()[:self.Kb], os_.cpu().numpy()])

    def adjoint(self, x, g):
        a, b, s = self._split(x)
        g = g if isinstance(g, torch.Tensor) else dev(g, self.dtype)
        oa, ob, os_ = self._outs()
        _lib.check(self.lib.cmax_depth_to_dense_adj(a.data_ptr(), s.data_ptr(), g.data_ptr(), self.A.data_ptr(), self._bp(self.B), *self._ints(), oa.data_ptr(),
                                                    self._bp(ob), os_.data_ptr(), F._stream()))
        return self._join(oa, ob, os_)

    def adjoint2(self, x, u, g, dg):
        a, b, s = self._split(x)
        da, db, ds = self._split(u)
        g, dg = dev(g, self.dtype), dev(dg, self.dtype)
        oa, ob, os_ = self._outs()
        _lib.check(self.lib.cmax_depth_to_dense_adj2(a.data_ptr(), s.data_ptr(), da.data_ptr(), ds.data_ptr(), g.data_ptr(), dg.data_ptr(), self.A.data_ptr(),
                                                     self._bp(self.B), *self._ints(), oa.data_ptr(), self._bp(ob), os_.data_ptr(), F._stream()))
        return self._join(oa, ob, os_)


LEAF_IDS = [f"{g}-{s[0]}x{s[1]}" for g, s in D.LEAF_CASES]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("gid,size", D.LEAF_CASES, ids=LEAF_IDS)
def test_leaf_kernels_against_the_reference(gid, size, dtype):
    tol = LEAF_TOL[dtype]
    worst = dict(forward=0.0, tangent=0.0, adjoint=0.0, adjoint2=0.0)
    for Ka, Kb in D.LEAF_K:
        spec, x, u, g, dg = D.leaf_inputs(gid, size, Ka, Kb)
        ref = _depth_ref.leaf(x, spec, g=g, u=u, dg=dg)
        L = Leaf(spec, dtype)
        out, tan = L.forward(x), L.tangent(x, u)
        adj, adj2 = L.adjoint(x, g), L.adjoint2(x, u, g, dg)
        e = dict(forward=rel_max(out, ref["D"]), tangent=rel_max(tan, ref["tan"]), adjoint=rel_blocks(adj, ref["adj"], Ka, Kb),
                 adjoint2=rel_blocks(adj2, ref["adj2"], Ka, Kb))
        # <J u, g> = <u, J^T g> on the device's own numbers
        lhs, rhs = float((tan.astype(np.float64) * g).sum()), float((u * adj).sum())
        e_id = abs(lhs - rhs) / float(np.abs(tan.astype(np.float64) * g).sum())
        print(f"[depth] leaf {gid} {size} Ka={Ka} Kb={Kb} {str(dtype)[6:]}: " + ", ".join(f"{k} {v:.1e}" for k, v in e.items()) + f", <J u, g> vs <u, J^T g> {e_id:.1e}")
        for k, v in e.items():
            worst[k] = max(worst[k], v)
            assert v <= tol, (gid, size, Ka, Kb, k, v)
        assert e_id <= (1e-12 if dtype == torch.float64 else 1e-6)
        # repeatability: the adjoints, run twice, give the same bits
        assert np.array_equal(adj, L.adjoint(x, g)) and np.array_equal(adj2, L.adjoint2(x, u, g, dg)) and np.array_equal(out, L.forward(x))
    print(f"[depth] leaf {gid} {size} {str(dtype)[6:]} worst: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("gid,size", D.LEAF_CASES, ids=LEAF_IDS)
def test_leaf_adjoint_of_one_hot_cotangents(gid, size, dtype):
    """One-hot cotangents on both components at tests/_patch_cases.band_pixels (the lines that bound a cell's band in k_grid_adj) and on both
    sides of every chunk seam of k_depth_adj: the reference by its closed form, J^T e = (rho A_k[e], B_j[e], U[e] Q^T e_pixel)."""
    Ka, Kb = 3, 5
    spec, x, _, _, _ = D.leaf_inputs(gid, size, Ka, Kb)
    H, W = size
    L = Leaf(spec, dtype)
    xt = torch.as_tensor(x)
    a, b, s = _depth_ref.split(xt, spec)
    rho = _depth_ref.Q(s, spec).numpy()
    U = np.einsum("k,kchw->chw", a.numpy(), spec["A"])
    sg = s.clone().requires_grad_()
    picks = sorted(set(C.band_pixels(gid, size)) | set(D.seam_pixels(size)))
    worst = 0.0
    for n, (i, j) in enumerate(picks):
        c = n % 2
        (qcol,) = torch.autograd.grad(_depth_ref.Q(sg, spec)[i, j], sg)
        want = np.concatenate([rho[i, j] * spec["A"][:, c, i, j], spec["B"][:, c, i, j], U[c, i, j] * qcol.numpy().reshape(-1)])
        g = torch.zeros((2, H, W), dtype=dtype, device="cuda")
        g[c, i, j] = 1.0
        e = rel_blocks(L.adjoint(x, g), want, Ka, Kb)
        worst = max(worst, e)
        assert e <= LEAF_TOL[dtype], (gid, size, (c, i, j), e)
    print(f"[depth] leaf {gid} {size} {str(dtype)[6:]}: {len(picks)} one-hot cotangents, worst {worst:.1e}")


def test_autograd_function_is_the_two_kernels():
    gid, size, Ka, Kb = "3x4-odd", (27, 40), 3, 3
    spec, x, _, g, _ = D.leaf_inputs(gid, size, Ka, Kb)
    ref = _depth_ref.leaf(x, spec, g=g)
    geo = D.geometry_six(spec)
    for dtype in (torch.float32, torch.float64):
        A, Bm = dev(spec["A"], dtype), dev(spec["B"], dtype)
        xt = dev(x).requires_grad_()
        a, b, s = xt[:Ka], xt[Ka:Ka + Kb], xt[Ka + Kb:].reshape(spec["patch_image_size"])
        out = F.depth_to_dense(a, b, s, A, Bm, geo)
        assert out.dtype == dtype and out.shape == (2,) + size
        (gx,) = torch.autograd.grad((out * dev(g, dtype)).sum(), xt)
        e_f, e_b = rel_max(out.detach().cpu().numpy(), ref["D"]), rel_blocks(gx.cpu().numpy(), ref["adj"], Ka, Kb)
        print(f"[depth] functional.depth_to_dense {str(dtype)[6:]}: forward {e_f:.1e} backward {e_b:.1e}")
        assert e_f <= LEAF_TOL[dtype] and e_b <= LEAF_TOL[dtype]
        # no B: None and an empty basis are the same thing
        o0 = F.depth_to_dense(a.detach(), None, s.detach(), A, None, {"patch_image_size": geo[:2], "pad": geo[2:4], "sliding_window": geo[4:]})
        o1 = F.depth_to_dense(a.detach(), b.detach()[:0], s.detach(), A, Bm[:0], geo)
        assert torch.equal(o0, o1)
    with pytest.raises(ValueError, match="elements"):
        F.depth_to_dense(dev(x[:2]), dev(x[3:6]), dev(x[6:]), dev(spec["A"]), dev(spec["B"]), geo)
    with pytest.raises(ValueError, match="Ka, 2, H, W"):
        F.depth_to_dense(dev(x[:3]), dev(x[3:6]), dev(x[6:]), dev(spec["A"][:, 0]), dev(spec["B"]), geo)
    with pytest.raises(ValueError, match="geometry"):
        F.depth_to_dense(dev(x[:3]), dev(x[3:6]), dev(x[6:]), dev(spec["A"]), dev(spec["B"]), geo[:5])


# ---- 2. plan evaluation ------------------------------------------------------------------------------------------------------------------
def plan_errors(b, loss, grad):
    return abs(loss - b["loss"]) / abs(b["loss"]), rel_blocks(grad, b["grad"], 3, 3)


def objective_of(c, b, **kw):
    return G.make_objective(b["ev"], b["spec"], exact=c["exact"], basis_dtype=c["basis_dtype"], **kw)


@pytest.mark.parametrize("cid", list(D.PLAN))
def test_plan_value_and_gradient(cid):
    c = D.PLAN[cid]
    b = D.built_plan(c)
    h, obj = objective_of(c, b)
    assert obj.nx == b["x"].size and obj.A.dtype == (torch.float32 if c["basis_dtype"] == "float32" else torch.float64)
    loss, grad = obj.value_and_grad_numpy(b["x"])
    e_loss, e_grad = plan_errors(b, loss, grad)
    print(f"[depth] plan {cid}: nx {len(grad)}, rel err loss {e_loss:.2e} grad {e_grad:.2e} (the worst of the whole vector and of the blocks a, b, s)")
    assert e_loss <= TOL and e_grad <= TOL, (cid, e_loss, e_grad)
    loss_v, none = obj.value_and_grad_numpy(b["x"], want_grad=False)
    assert none is None and abs(loss_v - b["loss"]) <= TOL * abs(b["loss"])
    del obj
    h.close()


def test_plan_graph_replay_in_a_child_process():
    """CMAX_PLAN_GRAPHS=1 is read when a plan is created: a fresh process with it set, six evaluations and products (replayed from the
    fourth on), every evaluation at the gate."""
    c = D.PLAN[D.GRAPH_CASE]
    b = D.built_plan(c)
    env = dict(os.environ, CMAX_PLAN_GRAPHS="1")
    run = subprocess.run([sys.executable, os.path.join(HERE, "_depth_plan_worker.py"), c["id"]], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    out = json.loads(run.stdout.strip().splitlines()[-1])
    assert out["enabled"] and out["n_graphs"] >= 2, out["n_graphs"]
    worst = [0.0, 0.0]
    for call in out["calls"]:
        e = plan_errors(b, call["loss"], np.array(call["grad"]))
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
    print(f"[depth] plan {c['id']}, graph replay ({out['n_graphs']} graphs): worst rel err loss {worst[0]:.2e} grad {worst[1]:.2e}")
    assert worst[0] <= TOL and worst[1] <= TOL
    first = out["calls"][0]
    for call in out["calls"][1:]:  # a replayed sequence computes what the eager one did (fp32 atomics: run-to-run noise only)
        assert abs(call["loss"] - first["loss"]) <= 1e-6 * abs(first["loss"]) and rel_max(call["hv"], first["hv"]) <= 1e-3 and np.any(first["hv"])


# ---- 3. the product, without and with a flow regulariser ---------------------------------------------------------------------------------
@pytest.mark.parametrize("reg", [None, "divergence"], ids=["plain", "flowreg"])
@pytest.mark.parametrize("cid", list(D.HVP))
def test_plan_product(cid, reg):
    c = D.HVP[cid]
    b = D.built_hvp(c)
    assert b["dropped"] <= D.DROP_CAP
    spec, x = b["spec"], b["x"]
    h, obj = objective_of(c, b)
    want_loss, want_grad, want_hv = b["loss"], b["grad"], dict(b["hv"])
    if reg:
        obj.set_flow_regularizer(D.FLOW_REG)
        dense_of = lambda xt: _depth_ref.dense(xt, spec)  # noqa: E731
        for name, v in b["v"].items():
            r, rg, rh = _flowreg_ref.plan_term(x, dense_of, D.FLOW_REG, spec["t_scale"], v=v)
            want_hv[name] = b["hv"][name] + rh
        want_loss, want_grad = b["loss"] + r, b["grad"] + rg
        assert abs(r) > 1e-6 * abs(b["loss"]) and np.abs(rg).max() > 1e-6 * np.abs(b["grad"]).max()  # the term is there
    loss, grad = obj.value_and_grad_numpy(x)
    e_loss, e_grad = abs(loss - want_loss) / abs(want_loss), rel_blocks(grad, want_grad, 3, 3)
    print(f"[depth] product case {cid} {reg}: {len(b['ev'])} events (dropped {b['dropped']:.5f}), rel err loss {e_loss:.2e} grad {e_grad:.2e}")
    assert e_loss <= TOL and e_grad <= TOL
    for name, v in b["v"].items():
        hv = obj.hvp_numpy(x, v)
        if name == "zero":
            assert not np.any(hv) and not np.any(want_hv[name])
            continue
        e = rel_blocks(hv, want_hv[name], 3, 3)
        print(f"[depth] product {cid} {reg} {name}: rel err Hv {e:.2e} (the worst of the whole vector and of the blocks a, b, s)")
        assert e <= TOL, (cid, reg, name, e)
    hv_t = obj.hvp(torch.as_tensor(x), torch.as_tensor(b["v"]["random"]))  # `hvp_numpy` on tensors
    assert hv_t.shape == (x.size,) and hv_t.dtype == torch.float64 and rel_blocks(hv_t.numpy(), want_hv["random"], 3, 3) <= TOL
    del obj
    h.close()


# ---- 4. deterministic handles: repeatability, the descent rule, the L-BFGS rule ----------------------------------------------------------
@pytest.mark.parametrize("cid", ["cam-27x40-two", "cam-27x40-burgers", "cam-27x40-f32basis"])
def test_deterministic_handle_is_bit_repeatable(cid):
    c = D.PLAN[cid]
    ev, x, spec = D.inputs(c)
    v = D.hvp_tangents(c, x, spec)["random"]
    h, obj = G.make_objective(ev, spec, deterministic=True, exact=c["exact"], basis_dtype=c["basis_dtype"])
    l0, g0 = obj.value_and_grad_numpy(x)
    hv0 = obj.hvp_numpy(x, v)
    l1, g1 = obj.value_and_grad_numpy(x)
    hv1 = obj.hvp_numpy(x, v)
    assert l0 == l1 and np.array_equal(g0, g1) and np.array_equal(hv0, hv1) and np.any(hv0)
    del obj
    h.close()


N_ITER, LR, LR_STEP, LR_DECAY, MOMENTUM = 6, 0.05, 2, 0.5, 0.9  # three learning rates occur (tests/test_gpu_descent.py)
METHODS = {"sgd": dict(method="SGD", momentum=MOMENTUM), "adam": dict(method="Adam")}


@pytest.mark.parametrize("mid", list(METHODS))
@pytest.mark.parametrize("cid", ["cam-27x40-two", "cam-27x40-burgers"])
def test_descent_rule_on_a_bit_repeatable_handle(cid, mid):
    """Every traced iterate of `descend` re-evaluated on the same deterministic handle (the same bits the loop saw), the optimiser's state
    rebuilt with tests/_descent_ref.py, as tests/test_gpu_basis_plan.py does."""
    c = D.PLAN[cid]
    ev, x0, spec = D.inputs(c)
    h, obj = G.make_objective(ev, spec, deterministic=True)
    res = obj.descend(x0, trace=True, n_iter=N_ITER, lr=LR, lr_step=LR_STEP, lr_decay=LR_DECAY, **METHODS[mid])
    assert res.trace.shape == (N_ITER + 1, x0.size) and res.n_done == N_ITER and np.isfinite(res.loss_history).all()
    np.testing.assert_array_equal(res.trace[0], x0)
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
    moved = np.abs(res.x_last - x0).max()
    print(f"[depth] descent rule {cid} {mid}: moved {moved:.3e}, worst step error {e_x:.2e} of max(1, |x|inf), loss history {e_loss:.2e}, "
          f"best {res.best_loss:.6g} at {res.best_iter}")
    assert moved > 0.0 and e_x <= 1e-10 and e_loss <= 1e-12
    del obj
    h.close()


def test_lbfgs_rule_on_a_bit_repeatable_handle():
    """cmax_patch_plan_lbfgs on the depth plan, teacher-forced through tests/_lbfgs_ref.py exactly as tests/test_gpu_lbfgs.py holds the
    basis plan to its rules."""
    from test_gpu_lbfgs import teacher_forced
    c = D.PLAN["cam-27x40-two"]
    ev, x0, spec = D.inputs(c)
    h, obj = G.make_objective(ev, spec, deterministic=True)
    kw = dict(n_eval=12, history=3, gtol=1e-9, max_move=20.0, step0=1.0, max_ls=10)
    res = obj.minimize_lbfgs(x0, trace=True, **kw)
    teacher_forced("depth", res, np.asarray(x0, dtype=np.float64).reshape(-1), kw, obj.value_and_grad_numpy)
    assert res.nit > kw["history"]  # the ring wrapped
    del obj
    h.close()


# ---- 5. the Python layer -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["cam-27x40-two", "cam-27x40-burgers", "cam-27x40-f32basis"])
def test_autograd_chained_path_agrees_with_the_plan(cid):
    c = D.PLAN[cid]
    b = D.built_plan(c)
    h, obj = objective_of(c, b)
    loss_n, grad_n = obj.value_and_grad_numpy(b["x"])
    x = torch.tensor(b["x"], dtype=torch.float64, device="cuda", requires_grad=True)
    loss = obj(x)
    (grad,) = torch.autograd.grad(loss, x)
    e_loss, e_grad = abs(loss.item() - loss_n) / abs(loss_n), rel_blocks(grad.cpu().numpy(), grad_n, 3, 3)
    r_loss, r_grad = plan_errors(b, loss.item(), grad.cpu().numpy())
    print(f"[depth] autograd-chained {cid}: vs the plan loss {e_loss:.2e} grad {e_grad:.2e}; vs the reference loss {r_loss:.2e} grad {r_grad:.2e}")
    assert e_loss <= TOL and e_grad <= TOL and r_loss <= TOL and r_grad <= TOL
    flow = obj.dense_flow(x.detach())
    assert flow.shape == ((b["spec"]["T"], 2) if b["spec"]["time_aware"] else (2,)) + c["size"]
    assert rel_max(flow.cpu().numpy(), _depth_ref.device_motion(b["x"], dict(b["spec"], round32=False))) <= 1e-6
    rho = obj.inverse_depth(x.detach()).cpu().numpy()
    assert rel_max(rho, _depth_ref.Q(torch.as_tensor(b["x"][6:]).reshape(b["spec"]["patch_image_size"]), b["spec"]).numpy()) <= 1e-12
    del obj
    h.close()


def test_camera_bases_gauge_and_other_arguments():
    size = (27, 40)
    c = D.PLAN["cam-27x40-one"]
    ev, x, spec = D.inputs(c)
    t_scale = spec["t_scale"]
    h = E.CMaxHandle(size).set_events(ev)
    g = C.GEOMETRY["3x4-odd"]
    shift = tuple((g["pad"][k] - 1) * g["sw"][k] for k in (0, 1))
    obj = DepthEgoMotionObjective(h, t_scale, g["patch_image_size"], g["sw"], g["sw"], shift, calib=spec["calib"], cost="image_variance")
    assert obj.has_native_plan and obj.has_exact_hvp and obj.A.dtype == torch.float64 and (obj.Ka, obj.Kb, obj.nx) == (3, 3, 18) and obj.pad == g["pad"]
    a, b, s = obj.split(x)
    assert a.shape == (3,) and b.shape == (3,) and s.shape == (3, 4)
    l0, g0 = obj.value_and_grad_numpy(x)
    # the gauge: the same field from (lambda a, s / lambda); `canonical` picks |a| = 1
    z = obj.canonical(x)
    l1, g1 = obj.value_and_grad_numpy(z)
    lam = np.linalg.norm(a)
    assert abs(np.linalg.norm(z[:3]) - 1.0) <= 1e-15 and abs(l1 - l0) <= 1e-5 * abs(l0)
    assert rel_max(g1[:3] / lam, g0[:3]) <= 1e-3 and rel_max(g1[6:] * lam, g0[6:]) <= 1e-3
    assert rel_max(obj.flow_field(dev(z)).cpu().numpy(), obj.flow_field(dev(x)).cpu().numpy()) <= 1e-14
    bound = (np.abs(s).max() * (np.abs(a) * obj.amax).sum() + (np.abs(b) * obj.bmax).sum()) * t_scale
    assert obj.flow_bound(x) == pytest.approx(bound) and float(obj.flow_field(dev(x)).abs().max()) <= bound
    obj.set_t_scale(0.5 * t_scale)  # the same displacement field from twice the velocities
    y = np.concatenate([2.0 * x[:6], x[6:]])
    l2, g2 = obj.value_and_grad_numpy(y)
    assert abs(l2 - l0) <= 1e-5 * abs(l0) and rel_max(g2[6:], g0[6:]) <= 1e-3
    for bad in (x[:-1], np.zeros(19)):
        with pytest.raises(ValueError, match="unknowns"):
            obj.value_and_grad_numpy(bad)
        with pytest.raises(ValueError, match="unknowns"):
            obj.hvp_numpy(x, bad)
        with pytest.raises(ValueError, match="unknowns"):
            obj.descend(bad, n_iter=2)
    kw = dict(patch_image_size=g["patch_image_size"], patch_size=g["sw"], sliding_window=g["sw"], patch_shift=shift)
    inv = DepthEgoMotionObjective(h, t_scale, calib=spec["calib"], cost="hybrid", cost_with_weight={"image_variance": "inv", "gradient_magnitude": 1.0}, **kw)
    assert not inv.has_native_plan and not inv.has_exact_hvp  # the fall-back: the autograd-chained path
    xt = dev(x).requires_grad_()
    (gi,) = torch.autograd.grad(inv(xt), xt)
    assert gi.shape == (18,) and bool(torch.isfinite(gi).all()) and bool(gi.abs().max() > 0)
    with pytest.raises(NotImplementedError, match="native plan"):
        inv.minimize_lbfgs(x)
    with pytest.raises(ValueError, match="total_variation"):
        DepthEgoMotionObjective(h, t_scale, calib=spec["calib"], cost="hybrid", cost_with_weight={"image_variance": 1.0, "total_variation": 0.01}, **kw)
    with pytest.raises(ValueError, match="bilinear"):
        DepthEgoMotionObjective(h, t_scale, calib=spec["calib"], cost="image_variance", filter_type="nearest", **kw)
    with pytest.raises(ValueError, match="one of the two"):
        DepthEgoMotionObjective(h, t_scale, cost="image_variance", **kw)
    with pytest.raises(ValueError, match="A must be"):
        DepthEgoMotionObjective(h, t_scale, bases=(np.zeros((3, 2, 5, 5)), None), cost="image_variance", **kw)
    with pytest.raises(ValueError, match="Ka \\+ Kb"):
        DepthEgoMotionObjective(h, t_scale, bases=(np.zeros((60, 2) + size), np.zeros((5, 2) + size)), cost="image_variance", **kw)
    no_b = DepthEgoMotionObjective(h, t_scale, bases=(spec["A"], None), cost="image_variance", **kw)  # Kb = 0
    assert no_b.nx == 15 and np.isfinite(no_b.value_and_grad_numpy(np.concatenate([x[:3], x[6:]]))[1]).all()
    del obj, inv, no_b
    h.close()


def test_lbfgs_recovers_the_depth_of_a_two_level_scene():
    """The recovery scene of tests/_depth_cases.py: from the start that knows the camera's motion and takes the mean depth everywhere,
    `minimize_lbfgs` must end with a lower loss than it started with and with a mean end-point error of D, over the pixels that hold events,
    below half the start's -- the criterion tests/test_depth_reference.py verified for the reference with SciPy's L-BFGS-B."""
    sc = D.scene()
    h, obj = G.make_objective(sc["ev"], sc["spec"])
    loss_start = obj.value_and_grad_numpy(sc["x_start"])[0]
    e_start = D.scene_error(sc["x_start"], sc)
    res = obj.minimize_lbfgs(sc["x_start"], n_eval=100, history=8, gtol=1e-7, max_move=10.0)
    loss_end = obj.value_and_grad_numpy(res.x)[0]
    e_end = D.scene_error(res.x, sc)
    print(f"[depth] recovery scene: loss {loss_start:.6g} -> {loss_end:.6g} ({res.nit} iterations, {res.nfev} evaluations, status {res.status}); mean end-point "
          f"error over the pixels that hold events {e_start:.3f} px -> {e_end:.3f} px; |a| {np.linalg.norm(res.x[:3]):.4f} (true "
          f"{np.linalg.norm(sc['x_true'][:3]):.4f})")
    assert loss_end < loss_start
    assert e_end < 0.5 * e_start
    del obj
    h.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def _create(h, d, A, Bm):
    plan = ctypes.c_void_p()
    rc = _lib.load().cmax_depth_plan_create(h._h, ctypes.byref(d), A.data_ptr(), Bm.data_ptr(), F._stream(), ctypes.byref(plan))
    return rc, _lib.load().cmax_last_error() or b"", plan


def test_refusals_of_the_new_entries():
    c = D.PLAN["cam-27x40-one"]
    ev, x, spec = D.inputs(c)
    h, obj = G.make_objective(ev, spec)
    lib = _lib.load()
    size = spec["size"]
    big = torch.zeros((65, 2) + size, dtype=torch.float64, device="cuda")
    for Ka, Kb, word in ((0, 3, b"Ka"), (65, 0, b"Ka"), (3, -1, b"Kb"), (3, 62, b"Ka + Kb")):
        d = obj._descriptor()
        d.Ka, d.Kb = Ka, Kb
        rc, msg, plan = _create(h, d, big, big)
        assert rc == _lib.EINVAL and word in msg and not plan.value, (Ka, Kb, rc, msg)
    for field, value, word in (("scale_later", 1, b"scale_later"), ("filter_type", _lib.FILTER_NEAREST, b"nearest"), ("basis_dtype", 2, b"basis_dtype"),
                               ("tv_weight", 0.01, b"total variation"), ("ph", 0, b"sizes"), ("sw_w", 0, b"sizes"), ("pad_h", -1, b"sizes")):
        d = obj._descriptor()
        setattr(d, field, value)
        rc, msg, plan = _create(h, d, obj.A, obj.B)
        assert rc == _lib.EINVAL and word in msg and not plan.value, (field, rc, msg)
    # the leaf entries: nothing is launched
    geo = obj.geometry
    out = torch.zeros((2,) + size, dtype=torch.float64, device="cuda")
    xs = torch.zeros(65 + 12, dtype=torch.float64, device="cuda")
    p = xs.data_ptr()
    for Ka, Kb in ((0, 3), (65, 0), (3, 62), (3, -1)):
        assert lib.cmax_depth_to_dense(p, p, p, big.data_ptr(), big.data_ptr(), _lib.F64, Ka, Kb, *geo, *size, out.data_ptr(), F._stream()) == _lib.EINVAL
        assert b"Ka" in lib.cmax_last_error()
        assert lib.cmax_depth_to_dense_adj(p, p, out.data_ptr(), big.data_ptr(), big.data_ptr(), _lib.F64, Ka, Kb, *geo, *size, p, p, p, F._stream()) == _lib.EINVAL
    assert lib.cmax_depth_to_dense(p, p, p, big.data_ptr(), big.data_ptr(), 2, 3, 3, *geo, *size, out.data_ptr(), F._stream()) == _lib.EINVAL
    assert lib.cmax_depth_to_dense_tan(p, p, p, p, p, big.data_ptr(), None, _lib.F64, 3, 3, *geo, *size, out.data_ptr(), F._stream()) == _lib.EINVAL  # Kb > 0, no B
    torch.cuda.synchronize()
    assert not bool(out.any()) and not bool(xs.any())
    # a handle that holds a communicator
    h.comm_init(force_rccl=True)
    rc, msg, plan = _create(h, obj._descriptor(), obj.A, obj.B)
    assert rc == _lib.EUNSUPPORTED and b"communicator" in msg and not plan.value
    g = C.GEOMETRY[c["gid"]]
    shift = tuple((g["pad"][k] - 1) * g["sw"][k] for k in (0, 1))
    with pytest.raises(NotImplementedError, match="communicator"):
        DepthEgoMotionObjective(h, spec["t_scale"], g["patch_image_size"], g["sw"], g["sw"], shift, calib=spec["calib"], cost="image_variance")
    h.comm_destroy()
    # a weighted handle, at creation and (a plan made earlier) at every call
    h.set_event_weights(np.full(len(ev), 0.5))
    rc, msg, plan = _create(h, obj._descriptor(), obj.A, obj.B)
    assert rc == _lib.EUNSUPPORTED and b"per-event weights" in msg and not plan.value
    with pytest.raises(NotImplementedError, match="per-event weights"):
        obj.value_and_grad_numpy(x)
    with pytest.raises(NotImplementedError, match="per-event weights"):
        obj.hvp_numpy(x, np.ones_like(x))
    h.set_event_weights(None)
    assert np.isfinite(obj.value_and_grad_numpy(x)[0])
    assert lib.cmax_sizeof_depth_objective() == ctypes.sizeof(_lib.CmaxDepthObjective)
    del obj
    h.close()
