"""The fused focus losses (mean square, Laplacian magnitude, Hessian magnitude: k_stats / k_gimage / k_stats_tan / k_gimage_tan over
FocusStencil, and the fused k_stats_gimage_st) against the fp64 reference of tests/_focus_ref.py on the cases of tests/_focus_cases.py.

Gate: the project's 1e-4, scaled as tests/test_gpu_fused.py and tests/test_gpu_hvp_parity.py scale theirs:
    loss      |L - L_ref| / |L_ref|            <= 1e-4
    gradient  max|g - g_ref| / max|g_ref|      <= 1e-4
    product   max|Hv - Hv_ref| / max|Hv_ref|   <= 1e-4
The measured errors are printed (on an MI355X: loss <= 6.5e-7, gradient <= 2.9e-6, product <= 8.5e-6 over all cases).  Both image-side forms are held to it: the default (k_stats_gimage_st) in this process, and the separate
k_stats + k_gimage launches (CMAX_NO_FUSED_FOCUS=1, read once per process) in a child (tests/_focus_worker.py)."""
import ctypes
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
from event_based_optical_flow_amd.cmax import ContrastObjective  # noqa: E402

import _focus_cases as C  # noqa: E402
import _focus_ref as R  # noqa: E402
from _focus_worker import launches  # noqa: E402
from _weighted_ref import weight_set  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
CHILD_LIMIT_S = 120
DEV = "cuda"


def rel_max(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def by_id(cid):
    return C.ALL[cid]


@pytest.mark.parametrize("cid", list(C.ALL))
def test_value_gradient_and_product_against_the_fp64_reference(cid):
    c = by_id(cid)
    b = C.built(c)
    assert b["dropped"] <= C.DROP_CAP
    h, desc = C.handle(c, b["ev"]), C.descriptor(c)
    res, grad = h.evaluate(desc, b["motion"])
    vres, _ = h.evaluate(desc, b["motion"], want_grad=False)  # value only: the separate statistics launch
    hv = h.hvp(desc, b["motion"], b["v"]).double().cpu().numpy()
    e_loss, e_vloss = abs(res[0].item() - b["loss"]) / abs(b["loss"]), abs(vres[0].item() - b["loss"]) / abs(b["loss"])
    e_grad, e_hv = rel_max(grad.cpu().numpy(), b["grad"]), rel_max(hv, b["hv"])
    print(f"[focus] {cid}: {len(b['ev'])} events, dropped {b['dropped']:.4f}, rel err loss {e_loss:.2e} (value only {e_vloss:.2e}) "
          f"grad {e_grad:.2e} Hv {e_hv:.2e}")
    h.close()
    assert e_loss <= TOL and e_vloss <= TOL and e_grad <= TOL, (cid, e_loss, e_vloss, e_grad)
    assert e_hv <= TOL, (cid, e_hv)


def test_separate_launches_in_a_child_process(tmp_path):
    env = dict(os.environ)
    env["CMAX_NO_FUSED_FOCUS"] = "1"
    out = str(tmp_path / "separate.npz")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_focus_worker.py"), out], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=CHILD_LIMIT_S)
    assert p.returncode == 0, f"child ended with status {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    got = dict(np.load(out))
    for c in C.CASES:
        b, cid = C.built(c), c["id"]
        e_loss, e_grad = abs(float(got[cid + "/loss"]) - b["loss"]) / abs(b["loss"]), rel_max(got[cid + "/grad"], b["grad"])
        print(f"[focus] separate launches {cid}: rel err loss {e_loss:.2e} grad {e_grad:.2e}")
        assert e_loss <= TOL and e_grad <= TOL, (cid, e_loss, e_grad)
    # the child ran k_stats + k_gimage, this process the one fused kernel (booked under "stats")
    c = C.CASES[0]
    b = C.built(c)
    here = launches(c, b["ev"], b["motion"])
    assert here.get("stats", 0) == 1 and here.get("gimage", 0) == 0, here
    assert int(got["profile/stats"]) == 1 and int(got["profile/gimage"]) == 1, {k: v for k, v in got.items() if k.startswith("profile/")}


def test_focus_costs_have_no_raw_form_and_refuse_unknown_codes():
    c = by_id("ms-plain-2dof-8x32-s0")
    b = C.built(c)
    h, desc = C.handle(c, b["ev"]), C.descriptor(c)
    assert not h.has_raw(desc)
    assert h.has_raw(E.make_descriptor("gradient_magnitude", c["model"]))
    desc.cost = 5  # CMAX_EINVAL, which the Python layer raises as CmaxError
    with pytest.raises(_lib.CmaxError) as e:
        h.evaluate(desc, b["motion"])
    assert e.value.code == _lib.EINVAL
    with pytest.raises(_lib.CmaxError) as e:
        F.contrast(torch.zeros(4, 4, device=DEV), 5, False)
    assert e.value.code == _lib.EINVAL
    with pytest.raises(KeyError):
        E.make_descriptor("range_magnitude", c["model"])
    h.close()


def test_weighted_handle():
    c = by_id("lap-norm-dense-17x40-s1-pad2")
    b = C.built(c)
    w = weight_set("uniform", b["ev"], seed=3)
    ev = torch.as_tensor(b["ev"])
    m = torch.as_tensor(b["motion"]).clone().requires_grad_()
    loss = R.objective(ev, m, c["model"], c["size"], weights=torch.as_tensor(w), **C.ref_kwargs(c))
    (g,) = torch.autograd.grad(loss, m)
    h, desc = C.handle(c, b["ev"]), C.descriptor(c)
    h.set_event_weights(w)
    res, grad = h.evaluate(desc, b["motion"])
    ref_loss = float(loss.detach())
    e_loss, e_grad = abs(res[0].item() - ref_loss) / abs(ref_loss), rel_max(grad.cpu().numpy(), g.numpy())
    print(f"[focus] weighted {c['id']}: rel err loss {e_loss:.2e} grad {e_grad:.2e}")
    h.close()
    assert e_loss <= TOL and e_grad <= TOL


def test_weight_and_event_gradients_of_the_laplacian():
    c = by_id("lap-plain-2dof-9x33-s0")
    b = C.built(c)
    ev = torch.as_tensor(b["ev"]).clone().requires_grad_()
    w = torch.ones(len(b["ev"]), dtype=torch.float64, requires_grad=True)
    m = torch.as_tensor(b["motion"])
    loss = R.objective(ev, m, c["model"], c["size"], weights=w, **C.ref_kwargs(c))
    g_ev, g_w = torch.autograd.grad(loss, (ev, w))
    h, desc = C.handle(c, b["ev"]), C.descriptor(c)
    _, _, gw = h.evaluate_weight_grad(desc, b["motion"])
    ge = h.events_grad(desc, b["motion"]).cpu().numpy()
    e_w, e_ev = rel_max(gw.cpu().numpy(), g_w.numpy()), rel_max(ge[:, :3], g_ev.numpy()[:, :3])
    print(f"[focus] {c['id']}: rel err dL/dw {e_w:.2e} dL/d(event) {e_ev:.2e}")
    h.close()
    assert not ge[:, 3].any()
    assert e_w <= TOL and e_ev <= TOL


@pytest.mark.parametrize("cid", ["hes-plain-dense-17x40-s0", "lap-multi-voxel3-37x53-s1", "ms-norm-2dof-9x33-s1-pad2-maximize"])
def test_deterministic_handle(cid):
    c = by_id(cid)
    b = C.built(c)
    h, desc = C.handle(c, b["ev"], deterministic=True), C.descriptor(c)
    assert h.deterministic
    res, grad = h.evaluate(desc, b["motion"])
    res2, grad2 = h.evaluate(desc, b["motion"])
    e_loss, e_grad = abs(res[0].item() - b["loss"]) / abs(b["loss"]), rel_max(grad.cpu().numpy(), b["grad"])
    print(f"[focus] deterministic {cid}: rel err loss {e_loss:.2e} grad {e_grad:.2e}")
    # result[]: loss, v_k, v_orig -- the rest is never written and holds what the allocation held (as tests/test_gpu_determinism.py)
    defined = [0] + list(range(1, 1 + desc.n_ref)) + ([5] if desc.normalized else [])
    r1, r2 = res.cpu().numpy()[defined], res2.cpu().numpy()[defined]
    g1, g2 = grad.cpu().numpy(), grad2.cpu().numpy()
    h.close()
    assert e_loss <= TOL and e_grad <= TOL
    assert r1.tobytes() == r2.tobytes(), (r1, r2)
    assert g1.tobytes() == g2.tobytes(), (g1, g2)


def test_batch_of_three_equals_three_single_calls():
    c = by_id("hes-norm-2dof-17x40-s1-border")
    b = C.built(c)
    h, desc = C.handle(c, b["ev"]), C.descriptor(c)
    motions = np.stack([b["motion"], b["motion"] * 0.5, b["motion"] + np.array([0.37, -0.61])])
    results, grads = h.evaluate_batch(desc, motions)
    for k in range(3):
        res, grad = h.evaluate(desc, motions[k])
        # the same kernels candidate by candidate; the statistics are summed with atomics, whose order is not fixed
        assert abs(results[k, 0].item() - res[0].item()) <= 1e-9 * abs(res[0].item())
        assert rel_max(grads[k].cpu().numpy(), grad.cpu().numpy()) <= 1e-6
    h.close()


def test_descend_takes_the_references_sgd_steps():
    c = by_id("ms-plain-2dof-37x53-s0-border-maximize")
    b = C.built(c)
    h = C.handle(c, b["ev"])
    obj = ContrastObjective(h, c["model"], cost=c["cost"], direction="minimize", sigma=float(c["sigma"]), omit_boundary=c["omit"])
    lr, n_iter = 0.5, 5
    out = obj.descend(b["motion"], method="SGD", n_iter=n_iter, lr=lr, trace=True)
    x = np.array(b["motion"], dtype=np.float64)
    kw = dict(C.ref_kwargs(c), direction="minimize")
    for it in range(n_iter):
        # (an iterate that puts an event on a cell border would make the two sides differ by more than rounding: none does here)
        loss, g, _ = R.value_grad_hvp(b["ev"], x, c["model"], c["size"], **kw)
        assert abs(out.loss_history[it] - loss) <= TOL * abs(loss), (it, out.loss_history[it], loss)
        x = x - lr * g
    e = rel_max(out.x_last, x)
    print(f"[focus] descend {c['id']}: {out.n_done} steps, rel err of the last iterate {e:.2e}")
    h.close()
    assert out.n_done == n_iter and e <= TOL


def test_patch_flow_objective_on_the_native_plan():
    """multi_focal_normalized_laplacian_magnitude + 0.01 total_variation on a 2 x 3 patch grid: value, gradient and H v of the native plan
    against the composition of tests/_patch_ref.py (patch grid -> dense flow, total variation) with the focus reference."""
    import _patch_ref as P
    from event_based_optical_flow_amd.solver.patch_objective import PatchFlowObjective

    size, sw, grid, cost = (32, 48), (16, 16), (2, 3), "multi_focal_normalized_laplacian_magnitude"
    spec = dict(size=size, patch_image_size=grid, sw=sw, pad=P.patch_pad(sw, sw), t_scale=1.0)
    rng = np.random.default_rng(21)
    x = C.f32(rng.uniform(-4.0, 4.0, 2 * grid[0] * grid[1]) + 0.137)
    v = C.f32(rng.normal(0.0, 1.0, x.shape))
    ev = E.utils.generate_events(C.N_EVENTS, size[0], size[1], 0.0, C.PERIOD, seed=21)
    dirs = R.cost_directions(cost)
    dmotion = P.device_motion(x, spec)
    ev, dropped = R.drop_ambiguous(ev, dmotion, "dense-flow", size, dirs, R.border_margin(ev, dmotion, "dense-flow", size, dirs))
    assert dropped <= C.DROP_CAP

    evt = torch.as_tensor(ev)
    xt = torch.as_tensor(x).clone().requires_grad_()
    loss = R.objective(evt, P.motion(xt, spec), "dense-flow", size, cost=cost, sigma=1) + 0.01 * P.total_variation(xt.reshape(2, *grid), True)
    (g,) = torch.autograd.grad(loss, xt, create_graph=True)
    (hv,) = torch.autograd.grad((g * torch.as_tensor(v)).sum(), xt)

    h = E.CMaxHandle(size).set_events(ev)
    obj = PatchFlowObjective(h, 1.0, grid, sw, sw, (0, 0), cost="hybrid", cost_with_weight={cost: 1.0, "total_variation": 0.01}, blur_sigma=1.0)
    assert obj.has_native_plan and obj.pad == tuple(spec["pad"])
    got_loss, got_grad = obj.value_and_grad_numpy(x)
    got_hv = obj.hvp_numpy(x, v)
    ref_loss = float(loss.detach())
    e_loss, e_grad, e_hv = abs(got_loss - ref_loss) / abs(ref_loss), rel_max(got_grad, g.detach().numpy()), rel_max(got_hv, hv.numpy())
    print(f"[focus] patch plan: {len(ev)} events, dropped {dropped:.4f}, rel err loss {e_loss:.2e} grad {e_grad:.2e} Hv {e_hv:.2e}")
    del obj
    h.close()
    assert e_loss <= TOL and e_grad <= TOL and e_hv <= TOL


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("shape,omit", [((1, 1), False), ((2, 2), False), ((4, 4), False), ((4, 4), True), ((8, 8), True), ((9, 33), False), ((9, 33), True)])
@pytest.mark.parametrize("kind", R.KINDS)
def test_leaf_operator(kind, shape, omit, dtype):
    code = {"mean_square": _lib.COST_MEAN_SQUARE, "laplacian_magnitude": _lib.COST_LAPLACIAN, "hessian_magnitude": _lib.COST_HESSIAN}[kind]
    img = np.random.default_rng(11).normal(0.0, 2.0, shape).astype(np.float32).astype(np.float64)
    t = torch.as_tensor(img).clone().requires_grad_()
    want = R.focus_value(t, kind, omit)
    (gwant,) = torch.autograd.grad(3.0 * want, t)
    x = torch.tensor(img, dtype=dtype, device=DEV, requires_grad=True)
    got = F.contrast(x, code, omit)
    (ggot,) = torch.autograd.grad(3.0 * got, x)
    # fp64: the same arithmetic up to summation order; fp32: the value and G are rounded to fp32 once on the way out
    tol = 1e-12 if dtype == torch.float64 else 2.0 ** -23
    assert got.dtype == dtype and ggot.dtype == dtype
    assert abs(got.item() - want.item()) <= tol * max(abs(want.item()), 1e-300), (got.item(), want.item())
    assert rel_max(ggot.double().cpu().numpy(), gwant.numpy()) <= tol
