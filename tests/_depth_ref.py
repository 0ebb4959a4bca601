"""TEST INFRASTRUCTURE ONLY: the fp64 value the depth plan (csrc/cmax_depth_kernels.h, cmax_depth_plan_create of csrc/cmax_solver.hip) is
held to.

torch on the CPU in fp64, autograd supplies every derivative:
    Q        the interpolation of the depth grid IS -tests/_patch_ref.patch_to_dense on one plane (the patch map negates, Q does not)
    motion   D = ((Q s) sum_k a_k A_k + sum_j b_j B_j) t_scale in fp64 [-> tests/_flow_ref.voxel when time-aware], then WHAT THE DEVICE HOLDS:
             rounded to fp32 once and chained straight-through (tests/_patch_ref._as_device_holds; spec "round32", default True)
    loss     the weighted sum of the fused terms of tests/_hvp_ref.objective on that motion
    plan     loss, gradient and H v as tests/_basis_ref.plan returns them, for x = [a | b | s]
Nothing of the terms or the voxel chain is restated here.  Anchored by tests/test_depth_reference.py."""
import numpy as np
import torch

import _flow_ref
import _hvp_ref
import _patch_ref


def _t(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64))


def Q(s, spec):
    """s [ph,pw] tensor -> rho [H,W]."""
    two = torch.stack([s, torch.zeros_like(s)])
    return -_patch_ref.patch_to_dense(two, spec["size"], spec["sw"], spec["pad"])[0]


def split(x, spec):
    Ka, Kb = spec["A"].shape[0], spec["B"].shape[0]
    ph, pw = spec["patch_image_size"]
    assert x.numel() == Ka + Kb + ph * pw
    return x[:Ka], x[Ka:Ka + Kb], x[Ka + Kb:].reshape(ph, pw)


def dense(x, spec):
    """Unscaled D [2,H,W] as a differentiable tensor."""
    a, b, s = split(x.reshape(-1), spec)
    D = Q(s, spec)[None] * torch.einsum("k,kchw->chw", a, _t(spec["A"]))
    if spec["B"].shape[0]:
        D = D + torch.einsum("k,kchw->chw", b, _t(spec["B"]))
    return D


def motion(x, spec):
    """The motion the fused terms see: [2,H,W] or [T,2,H,W].  spec: A, B, patch_image_size, sw, pad, size, t_scale, round32 and, time-aware,
    T / scheme / t0."""
    held = _patch_ref._as_device_holds if spec.get("round32", True) else (lambda m: m)
    D = dense(x, spec) * spec["t_scale"]
    if not spec.get("time_aware"):
        return held(D)
    return held(_flow_ref.voxel(D, spec["T"], spec["scheme"], spec["t0"]))


def loss(x, events, spec):
    m = motion(x, spec)
    model = "dense-flow-voxel" if spec.get("time_aware") else "dense-flow"
    out = 0.0
    for cost, w in spec["terms"]:
        out = out + w * _hvp_ref.objective(events, m, model, spec["size"], cost=cost, sigma=spec["sigma"], omit_boundary=spec.get("omit", True))
    return out


def plan(x, events, spec, v=None):
    """-> (loss, grad [nx], H v or None) in fp64 numpy."""
    ev = _t(events)
    xt = _t(x).reshape(-1).clone().requires_grad_()
    val = loss(xt, ev, spec)
    (g,) = torch.autograd.grad(val, xt, create_graph=v is not None)
    hv = None
    if v is not None:
        hv = torch.zeros_like(xt)
        if g.requires_grad:
            (h,) = torch.autograd.grad((g * _t(v).reshape(-1)).sum(), xt, allow_unused=True)
            hv = hv if h is None else h
        hv = hv.detach().numpy().copy()
    return float(val.detach()), g.detach().numpy().copy(), hv


def device_motion(x, spec):
    with torch.no_grad():
        return motion(_t(x).reshape(-1), spec).numpy().copy()


# ---- the leaf operators, by autograd on `dense` ------------------------------------------------------------------------------------
def leaf(x, spec, g=None, u=None, dg=None):
    """-> dict(D, and where the inputs are given: adj = J^T g, tan = J u, adj2 = J^T dg + (dJ[u])^T g), fp64 numpy."""
    xt = _t(x).reshape(-1).clone().requires_grad_()
    D = dense(xt, spec)
    out = dict(D=D.detach().numpy().copy())
    if g is not None:
        (adj,) = torch.autograd.grad((D * _t(g)).sum(), xt, create_graph=u is not None)
        out["adj"] = adj.detach().numpy().copy()
    if u is not None:
        ut = _t(u).reshape(-1)
        w = torch.zeros_like(D, requires_grad=True)
        (jt,) = torch.autograd.grad((D * w).sum(), xt, create_graph=True)
        (tan,) = torch.autograd.grad((jt * ut).sum(), w)
        out["tan"] = tan.detach().numpy().copy()
        if g is not None and dg is not None:
            (second,) = torch.autograd.grad((adj * ut).sum(), xt)  # (dJ[u])^T g
            (first,) = torch.autograd.grad((dense(xt, spec) * _t(dg)).sum(), xt)
            out["adj2"] = (first + second).detach().numpy().copy()
    return out
