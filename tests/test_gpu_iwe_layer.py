"""The IWE layer -- cmax_iwes, cmax_iwes_vjp, cmax_iwes_jvp, cmax_iwes_vjp_tan, CMaxHandle.iwes*, fused_iwes and the custom-cost forms of
ContrastObjective / PatchFlowObjective -- against the fp64 autograd of tests/_iwe_ref.py (anchored without a GPU by
tests/test_iwe_reference.py), on every branch a small batch reaches: three models, voxel T = 2 and 5, blur, one and three reference
times, reference time 0.3, fractional sources, padding, off-sensor 2-DoF events, raw time, the un-warped image, the clipped window with
and without time slabs, unweighted and weighted handles -- and, in fresh child processes (tests/_iwe_layer_worker.py), the big and mid
segment layouts.

Gate: TOL = 1e-4 of the largest entry, the project's plain gate, on every image, VJP, grad_w, JVP image and vjp_tan.  The weight sets
`uniform`, `polarity`, `zeros` and the 100 : 1 set `w100` (the edge of the documented range min|w != 0| / wmax >= 0.01) are held to it;
the 1000 : 1 set `hdr` is outside that range and only printed.  Motions, tangents and image cotangents are fp32 values on both sides;
events within fp32 rounding of a cell border are removed beforehand (tests/_hvp_cases.py; their share is capped at 0.5 % by
tests/test_iwe_reference.py).  Measured errors: profiles/iwe_layer_parity.txt.

STATE: every call re-derives windows and cells from the motion it is given, so a backward pass computes with the handle's state (event
order, weights) AT BACKWARD TIME; only another batch (set_events) is refused (RuntimeError).  test_interleaved_* pin both.

Child processes (one at a time, each under its own limit, no further child after a failed one).  Durations measured on the first
green run on an MI355X, and the limits derived from them (5 x, at least 60 s):
    big   CMAX_BIG_SEG=1                  2.5 s   -> limit 60 s
    big   CMAX_BIG_SEG=1 CMAX_COMPACT=0   2.9 s   -> limit 60 s
    mid   CMAX_MID_SEG=1                  3.2 s   -> limit 60 s"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import event_based_optical_flow_amd as E  # noqa: E402
from event_based_optical_flow_amd.solver import PatchFlowObjective  # noqa: E402
from event_based_optical_flow_amd.solver.scipy_autograd import minimize  # noqa: E402

import _hvp_cases as C  # noqa: E402
import _iwe_cases as IC  # noqa: E402
import _iwe_ref as IR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
CHILD_LIMIT_S = {("big", 0): 60, ("big", 1): 60, ("mid", 0): 60}


def rel_max(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def host(t):
    return t.double().cpu().numpy()


def make_handle(c, b, w=None):
    h = E.CMaxHandle(c["size"], c["pad"])
    if c["outside"]:
        h.set_keep_outside(True)
    tr = b["t_range"]
    h.set_events(b["ev"], tmin=tr[0] if tr else None, tmax=tr[1] if tr else None, time_bin=c["T"], on_dropped="ignore", weights=w)
    assert h.n_events == len(b["ev"])
    if c["slabs"]:
        h.set_time_slabs(c["slabs"])
    return h


def layer_errors(h, b):
    """Relative errors of the four calls (and grad_w) against the reference answers in b."""
    cfg, cot = b["cfg"], b["cot"]
    m, v = b["motion"], b["v"]
    imgs = h.iwes(m, **cfg)
    gm, gw = h.iwes_vjp(m, gimages=cot["G"], want_grad_w=True, **cfg)
    jv = h.iwes_jvp(m, tangent=v, **cfg)
    vt = h.iwes_vjp_tan(m, tangent=v, gimages=cot["G"], gimages_tan=cot["Gp"], **cfg)
    vt0 = h.iwes_vjp_tan(m, tangent=v, gimages=cot["G"], gimages_tan=None, **cfg)
    err = dict(images=max(rel_max(host(imgs[k]), b["images"][k]) for k in range(imgs.shape[0])), vjp=rel_max(host(gm), b["gm"]),
               grad_w=rel_max(host(gw), b["gw"]), jvp=max(rel_max(host(jv[k]), b["jv"][k]) for k in range(jv.shape[0])),
               vjp_tan=rel_max(host(vt), b["vt"]), mixed=rel_max(host(vt0), b["vt_mixed"]))
    return err, imgs


def report(cid, wname, h, b, err):
    info = h.work_list_info()
    print(f"[iwe layer] {cid} w={wname}: {len(b['ev'])} events, {info['segments']} segments of <= {info['segment_events']}, dropped {b['dropped']:.5f}, rel err "
          + " ".join(f"{k} {v:.2e}" for k, v in err.items()))


@pytest.mark.parametrize("cid", [c["id"] for c in IC.CASES])
def test_layer_against_the_fp64_reference(cid):
    c = IC.ALL[cid]
    b = IC.built(c)
    h = make_handle(c, b)
    err, imgs = layer_errors(h, b)
    report(cid, "none", h, b, err)
    cfg = b["cfg"]
    for k, direction in enumerate(cfg["directions"]):  # image k is what cmax_iwe returns for that reference time
        one = h.iwe(b["motion"], c["model"], direction, c["normalize_t"], c["sigma"])
        assert rel_max(host(imgs[k]), host(one)) <= 1e-5, (cid, k)
    if cfg["with_orig"]:
        assert rel_max(host(imgs[-1]), host(h.iwe(None, None, sigma=c["sigma"]))) <= 1e-5
    h.close()
    assert all(e <= TOL for e in err.values()), (cid, err)


@pytest.mark.parametrize("wname", ["uniform", "polarity", "zeros", "w100", "hdr"])
@pytest.mark.parametrize("cid", IC.WEIGHTED)
def test_weighted_layer_against_the_fp64_reference(cid, wname):
    """The WEIGHTED instantiations of k_vote_tan / k_grad_hvp (and the weighted K1 / gathers behind them)."""
    c = IC.ALL[cid]
    b = IC.built(c, wname)
    h = make_handle(c, b, b["w"])
    assert h.weighted
    err, _ = layer_errors(h, b)
    report(cid, wname, h, b, err)
    h.close()
    if wname != "hdr":  # 1000 : 1 is outside the supported range of the fixed-point votes: reported, not gated
        assert all(e <= TOL for e in err.values()), (cid, wname, err)


@pytest.mark.parametrize("cid", [IC.CASES[0]["id"], IC.WEIGHTED[1], IC.WEIGHTED[-1]])
def test_special_cotangents(cid):
    """G one-hot on the pixel with most votes, G non-zero only in the border rows / columns and the padding, G = 0 (exact zeros)."""
    c = IC.ALL[cid]
    b = IC.built(c)
    h = make_handle(c, b)
    cfg, L, m, v = b["cfg"], b["layer"], b["motion"], b["v"]
    for kind in ("onehot", "border"):
        G = b["cot"][kind]
        gm_ref, gw_ref = L.vjp(G)
        gm, gw = h.iwes_vjp(m, gimages=G, want_grad_w=True, **cfg)
        vt = h.iwes_vjp_tan(m, tangent=v, gimages=G, gimages_tan=G, **cfg)
        e = (rel_max(host(gm), gm_ref), rel_max(host(gw), gw_ref), rel_max(host(vt), L.vjp_tan(v, G, G)))
        print(f"[iwe layer] {cid} G={kind}: rel err vjp {e[0]:.2e} grad_w {e[1]:.2e} vjp_tan {e[2]:.2e}")
        assert max(e) <= TOL, (cid, kind, e)
    Z = np.zeros_like(b["cot"]["G"])
    gm, gw = h.iwes_vjp(m, gimages=Z, want_grad_w=True, **cfg)
    assert not host(gm).any() and not host(gw).any()
    assert not host(h.iwes_vjp_tan(m, tangent=v, gimages=Z, gimages_tan=Z, **cfg)).any()
    assert not host(h.iwes_jvp(m, tangent=np.zeros_like(v), **cfg)).any()
    # a zero tangent leaves J^T G'
    vt = h.iwes_vjp_tan(m, tangent=np.zeros_like(v), gimages=b["cot"]["G"], gimages_tan=b["cot"]["G"], **cfg)
    assert rel_max(host(vt), b["gm"]) <= TOL
    h.close()


@pytest.mark.parametrize("model,T", [("2d-translation", 0), ("dense-flow", 0), ("dense-flow-voxel", 3)])
def test_empty_handle_gives_zeros(model, T):
    h = E.CMaxHandle(C.BASE).set_events(np.zeros((0, 4)), time_bin=T)
    motion = np.array([3.0, -2.0]) if model == "2d-translation" else np.ones(((T,) if T else ()) + (2,) + C.BASE)
    cfg = dict(motion_model=model, directions=("first", "last"), sigma=1.0, with_orig=True)
    imgs = h.iwes(motion, **cfg)
    G = torch.ones_like(imgs)
    gm, gw = h.iwes_vjp(motion, gimages=G, want_grad_w=True, **cfg)
    assert tuple(imgs.shape) == (3,) + C.BASE and not host(imgs).any() and not host(gm).any() and gw.numel() == 0
    assert not host(h.iwes_jvp(motion, tangent=np.ones_like(motion), **cfg)).any()
    assert not host(h.iwes_vjp_tan(motion, tangent=np.ones_like(motion), gimages=G, gimages_tan=G, **cfg)).any()
    h.close()


def test_refusals():
    """Deterministic handles and handles with a communicator: NotImplementedError with the library's text, for the four new calls."""
    c = IC.CASES[0]
    b = IC.built(c)
    cfg, m, v, G = b["cfg"], b["motion"], b["v"], b["cot"]["G"]
    for prepare, undo in ((lambda h: h.set_deterministic(True), lambda h: h.set_deterministic(False)),
                          (lambda h: h.comm_init(force_rccl=True), lambda h: h.comm_destroy())):
        h = make_handle(c, b)
        prepare(h)
        for call in (lambda: h.iwes(m, **cfg), lambda: h.iwes_vjp(m, gimages=G, **cfg), lambda: h.iwes_jvp(m, tangent=v, **cfg),
                     lambda: h.iwes_vjp_tan(m, tangent=v, gimages=G, gimages_tan=G, **cfg)):
            with pytest.raises(NotImplementedError):
                call()
        undo(h)
        h.close()


# ---- interleaving: nothing an earlier call left on the handle is relied on ---------------------------------------------------------
def _grad_of(imgs, G, inputs):
    return torch.autograd.grad((imgs * torch.as_tensor(G, dtype=torch.float32, device=imgs.device)).sum(), inputs)


def test_interleaved_forwards_and_an_objective_between_forward_and_backward():
    c = next(x for x in IC.CASES if x["model"] == "dense-flow" and x["n"] == 30_000 and x["group"] == "matrix")
    b = IC.built(c)
    h = make_handle(c, b)
    cfg, G = b["cfg"], b["cot"]["G"]
    m1 = torch.tensor(b["motion"], dtype=torch.float32, device="cuda", requires_grad=True)
    m2 = torch.tensor(C.f32(b["motion"] * 0.5 + 0.25), dtype=torch.float32, device="cuda", requires_grad=True)
    A = E.fused_iwes(h, m1, **cfg)
    B = E.fused_iwes(h, m2, **cfg)
    desc = E.make_descriptor("gradient_magnitude", c["model"], sigma=1.0)
    h.evaluate(desc, m2.detach() * 2.0)  # other windows, other images on the handle
    (ga,) = _grad_of(A, G, m1)
    (gb,) = _grad_of(B, G, m2)
    L2 = IR.Layer(b["ev"], host(m2.detach()), c["model"], c["size"], cfg["directions"], None, sigma=c["sigma"], outer_padding=c["pad"],
                  normalize_t=c["normalize_t"], t_range=b["t_range"], with_orig=cfg["with_orig"])
    assert rel_max(host(ga), b["gm"]) <= TOL and rel_max(host(gb), L2.vjp(G)[0]) <= TOL
    assert rel_max(host(B.detach()), L2.images()) <= TOL
    h.close()


def test_interleaved_state_changes_use_the_state_at_backward_time():
    """set_time_slabs(4) between forward and backward: the same numbers from another event order.  set_event_weights(None) between
    forward and backward: the backward pass is the UNWEIGHTED handle's (documented: the state at backward time).  set_events: refused."""
    c = next(x for x in IC.CASES if x["model"] == "2d-translation" and x["n"] == 30_000 and x["group"] == "matrix")
    bw, b = IC.built(c, "uniform"), IC.built(c)
    h = make_handle(c, bw, bw["w"])
    cfg, G = b["cfg"], b["cot"]["G"]
    m = torch.tensor(b["motion"], dtype=torch.float64, device="cuda", requires_grad=True)
    A = E.fused_iwes(h, m, **cfg)
    assert rel_max(host(A.detach()), bw["images"]) <= TOL
    h.set_time_slabs(4)
    (g,) = torch.autograd.grad((A * torch.as_tensor(G, dtype=torch.float32, device="cuda")).sum(), m, retain_graph=True)
    assert rel_max(host(g), bw["gm"]) <= TOL
    h.set_event_weights(None)
    (g,) = torch.autograd.grad((A * torch.as_tensor(G, dtype=torch.float32, device="cuda")).sum(), m, retain_graph=True)
    assert rel_max(host(g), b["gm"]) <= TOL
    h.set_events(b["ev"], on_dropped="ignore")
    with pytest.raises(RuntimeError, match="another batch"):
        torch.autograd.grad(A.sum(), m)
    h.close()


# ---- end to end: costs written in torch on the layer --------------------------------------------------------------------------------
E2E = [c["id"] for c in C.CASES if c["group"] == "matrix" and (c["n"] <= 2000 or c["cost"] in (C.COSTS[0], C.COSTS[5]))]


def _tensor_motion(c, b):
    dtype = torch.float64 if c["model"] == "2d-translation" else torch.float32
    return torch.tensor(b["motion"], dtype=dtype, device="cuda", requires_grad=True)


@pytest.mark.parametrize("cid", E2E)
def test_builtin_costs_written_in_torch(cid):
    """ContrastObjective(cost=callable): loss, gradient and torch.autograd.functional.vhp against _hvp_ref.value_grad_hvp."""
    c = C.ALL[cid]
    b = C.built(c)
    h = make_handle(c, b)
    obj = E.ContrastObjective(h, c["model"], cost=IR.torch_cost(c["cost"], c["omit"], c["direction"]), sigma=float(c["sigma"]),
                              omit_boundary=c["omit"], normalize_t=c["normalize_t"], warp_direction=c["warp_direction"])
    m = _tensor_motion(c, b)
    loss = obj(m)
    (g,) = torch.autograd.grad(loss, m)
    v = torch.tensor(b["v"], dtype=m.dtype, device="cuda").reshape(m.shape)
    _, hv = torch.autograd.functional.vhp(lambda x: obj(x), m.detach(), v)
    hv2 = obj.hvp(m.detach(), v)
    e = (abs(loss.item() - b["loss"]) / abs(b["loss"]), rel_max(host(g), b["grad"]), rel_max(host(hv), b["hv"]), rel_max(host(hv2), b["hv"]))
    print(f"[iwe layer] torch cost {cid}: rel err loss {e[0]:.2e} grad {e[1]:.2e} vhp {e[2]:.2e} hvp() {e[3]:.2e}")
    h.close()
    assert max(e) <= TOL, (cid, e)


@pytest.mark.parametrize("cid", IC.WEIGHTED[:3])
def test_weighted_costs_written_in_torch(cid):
    """fused_iwes(weights=w): loss, dL/dmotion, dL/dw and the vhp in the motion against tests/_iwe_ref.py."""
    c = IC.ALL[cid]
    b = IC.built(c, "uniform")
    cfg = b["cfg"]
    cost = IR.torch_cost(c["cost"], c["omit"], c["direction"])
    keys = ["forward_iwe", "backward_iwe", "middle_iwe"] if len(cfg["directions"]) == 3 else ["iwe"]

    def loss_of(imgs):
        arg = {key: imgs[k] for k, key in enumerate(keys)}
        arg["omit_boundary"] = c["omit"]
        if cfg["with_orig"]:
            arg["orig_iwe"] = imgs[len(keys)]
        return cost(arg)

    mr, wr = IR._t(b["motion"]).requires_grad_(), IR._t(b["w"]).requires_grad_()
    lr = loss_of(IR.images_t(IR._t(b["ev"]), mr, wr, c["model"], c["size"], cfg["directions"], sigma=c["sigma"], outer_padding=c["pad"],
                             normalize_t=c["normalize_t"], t_range=b["t_range"], with_orig=cfg["with_orig"]))
    gm_r, gw_r = torch.autograd.grad(lr, (mr, wr), create_graph=True)
    (hv_r,) = torch.autograd.grad((gm_r * IR._t(b["v"]).reshape(mr.shape)).sum(), mr)
    h = make_handle(c, b)
    m = _tensor_motion(c, b)
    w = torch.tensor(b["w"], dtype=torch.float64, device="cuda", requires_grad=True)
    loss = loss_of(E.fused_iwes(h, m, weights=w, **cfg))
    gm, gw = torch.autograd.grad(loss, (m, w), create_graph=True)
    (hv,) = torch.autograd.grad((gm * torch.tensor(b["v"], dtype=m.dtype, device="cuda").reshape(m.shape)).sum(), m)
    e = (abs(loss.item() - lr.item()) / abs(lr.item()), rel_max(host(gm.detach()), gm_r.detach().numpy()), rel_max(host(gw.detach()), gw_r.detach().numpy()),
         rel_max(host(hv), hv_r.numpy()))
    print(f"[iwe layer] weighted torch cost {cid}: rel err loss {e[0]:.2e} grad {e[1]:.2e} grad_w {e[2]:.2e} vhp {e[3]:.2e}")
    with pytest.raises(NotImplementedError):  # a second derivative through the weights
        torch.autograd.grad(gw.sum(), m)
    # the same through ContrastObjective(cost=callable)(motion, weights=w)
    obj = E.ContrastObjective(h, c["model"], cost=cost, sigma=float(c["sigma"]), omit_boundary=c["omit"], normalize_t=c["normalize_t"],
                              warp_direction=c["warp_direction"])
    l2 = obj(m, weights=w)
    g2m, g2w = torch.autograd.grad(l2, (m, w))
    e2 = (abs(l2.item() - lr.item()) / abs(lr.item()), rel_max(host(g2m), gm_r.detach().numpy()), rel_max(host(g2w), gw_r.detach().numpy()))
    h.close()
    assert max(e) <= TOL, (cid, e)
    assert max(e2) <= TOL, (cid, e2)


def test_a_registered_cost_without_a_kernel():
    """A CostBase subclass (Charbonnier mean) -- as an instance, and by name after registration (removed again: tests/test_host_logic.py
    compares the registry with FUSED_COSTS) -- against the same expression on the reference's images."""

    class CharbonnierMean(E.costs.CostBase):
        name = "charbonnier_mean"
        required_keys = ["iwe", "omit_boundary"]

        def calculate(self, arg):
            v = IR.charbonnier_mean(arg["iwe"])
            return v if self.direction == "minimize" else -v

    c = next(x for x in IC.CASES if x["model"] == "dense-flow" and x["n"] == 30_000 and x["group"] == "matrix" and x["cost"] == C.COSTS[0])
    b = IC.built(c)
    mr = IR._t(b["motion"]).requires_grad_()
    lr = IR.charbonnier_mean(IR.images_t(IR._t(b["ev"]), mr, torch.ones(len(b["ev"]), dtype=torch.float64), c["model"], c["size"], ("first",),
                                         sigma=c["sigma"], outer_padding=c["pad"])[0])
    (gr,) = torch.autograd.grad(lr, mr, create_graph=True)
    (hr,) = torch.autograd.grad((gr * IR._t(b["v"])).sum(), mr)
    h = make_handle(c, b)
    E.costs.functions["charbonnier_mean"] = CharbonnierMean
    try:
        with pytest.raises(KeyError):
            E.ContrastObjective(h, c["model"], cost="no_such_cost")
        for cost in (CharbonnierMean(), "charbonnier_mean"):
            obj = E.ContrastObjective(h, c["model"], cost=cost, sigma=float(c["sigma"]))
            m = _tensor_motion(c, b)
            loss = obj(m)
            (g,) = torch.autograd.grad(loss, m)
            hv = obj.hvp(m.detach(), torch.tensor(b["v"], dtype=torch.float32, device="cuda"))
            e = (abs(loss.item() - lr.item()) / abs(lr.item()), rel_max(host(g), gr.detach().numpy()), rel_max(host(hv), hr.numpy()))
            print(f"[iwe layer] charbonnier {c['id']}: rel err loss {e[0]:.2e} grad {e[1]:.2e} hvp {e[2]:.2e}")
            assert max(e) <= TOL, e
    finally:
        del E.costs.functions["charbonnier_mean"]
        h.close()


def test_newton_cg_on_a_custom_cost_patch_objective_recovers_the_generating_velocity():
    """The check of tests/test_gpu_solver.py::test_minimize_recovers_the_generating_velocity on the same scene, through a
    PatchFlowObjective whose cost is a torch callable: no native plan, exact Hessian-vector products by double backward."""
    size, vel = (96, 128), np.array([9.0, -6.0])
    ev = E.utils.generate_structured_events(60000, size[0], size[1], tuple(vel), n_dots=120, jitter=0.3, seed=5)
    h = E.CMaxHandle(size).set_events(ev)
    obj = PatchFlowObjective(h, 1.0, (1, 1), size, size, (0, 0), cost=IR.torch_cost("image_variance"), blur_sigma=1)
    assert not obj.has_native_plan and obj.has_exact_hvp
    res = minimize(obj, vel * 0.7, method="Newton-CG", precision="float64", torch_device="cuda", options={"xtol": 1e-7, "maxiter": 60})
    h.close()
    assert np.abs(res.x - vel).max() < 0.35, res
    assert np.linalg.norm(res.jac) < 0.05


# ---- non-default segment layouts: read once per process from the environment, so each runs in a child of its own -------------------
_child_failed = []


def _run_child(layout, k, tmp_path):
    if _child_failed:
        pytest.fail(f"not started: an earlier layout child failed ({_child_failed[0]})")
    env = dict(os.environ)
    for name in ("CMAX_BIG_SEG", "CMAX_MID_SEG", "CMAX_COMPACT"):
        env.pop(name, None)
    env.update(C.LAYOUT_ENV[layout][k])
    out = str(tmp_path / f"{layout}{k}.npz")
    t0 = time.time()
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_iwe_layer_worker.py"), layout, out], env=env, cwd=ROOT,
                           capture_output=True, text=True, timeout=CHILD_LIMIT_S[(layout, k)])
    except subprocess.TimeoutExpired as e:
        _child_failed.append(f"{layout} {k}: timed out")
        pytest.fail(f"layout child {layout} {C.LAYOUT_ENV[layout][k]} exceeded {CHILD_LIMIT_S[(layout, k)]} s\n{e.stderr}")
    print(f"[iwe layer] child {layout} {C.LAYOUT_ENV[layout][k]}: {time.time() - t0:.1f} s")
    if p.returncode != 0:
        _child_failed.append(f"{layout} {k}: exit status {p.returncode}")
        pytest.fail(f"layout child {layout} {C.LAYOUT_ENV[layout][k]} ended with status {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    return dict(np.load(out))


@pytest.mark.parametrize("layout,k", [("big", 0), ("big", 1), ("mid", 0)], ids=["big", "big-uncompacted", "mid"])
def test_forced_segment_layouts(layout, k, tmp_path):
    """CMAX_BIG_SEG=1 (4088-event segments, b512), the same without the compacted event order, CMAX_MID_SEG=1 (3064-event segments,
    m512).  The child asserts the segment size it ran with."""
    got = _run_child(layout, k, tmp_path)
    for i, c in enumerate(IC.LAYOUT_CASES[layout]):
        assert int(got[c["id"] + "/segment_events"]) == C.LAYOUT_SEGMENT_EVENTS[layout]
        for wname in (("none", "uniform") if i == 0 else ("none",)):
            b, key = IC.built(c, wname), f"{c['id']}/{wname}"
            err = dict(images=rel_max(got[key + "/images"], b["images"]), vjp=rel_max(got[key + "/gm"], b["gm"]), grad_w=rel_max(got[key + "/gw"], b["gw"]),
                       jvp=rel_max(got[key + "/jv"], b["jv"]), vjp_tan=rel_max(got[key + "/vt"], b["vt"]))
            print(f"[iwe layer] {c['id']} w={wname} {C.LAYOUT_ENV[layout][k]}: {len(b['ev'])} events, {int(got[c['id'] + '/segments'])} segments of <= "
                  f"{int(got[c['id'] + '/segment_events'])}, rel err " + " ".join(f"{n} {v:.2e}" for n, v in err.items()))
            assert all(e <= TOL for e in err.values()), (c["id"], wname, err)
