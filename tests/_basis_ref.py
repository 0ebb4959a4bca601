"""TEST INFRASTRUCTURE ONLY: the fp64 value the flow-basis plan (csrc/cmax_basis_kernels.h, cmax_basis_plan_create of
csrc/cmax_solver.hip) is held to.

torch on the CPU in fp64, autograd supplies every derivative:
    motion   D = (sum_k theta_k B_k) t_scale in fp64 [-> tests/_flow_ref.voxel when time-aware], then WHAT THE DEVICE HOLDS: the field
             the fused terms see is rounded to fp32 once and chained straight-through (tests/_patch_ref._as_device_holds; spec
             "round32", default True).  As in tests/_patch_ref.motion the rounding is the last step: a time-aware plan propagates the
             fp64 displacement field and rounds the voxel.
    loss     the weighted sum of the fused terms of tests/_hvp_ref.objective on that motion -- tests/_patch_ref.loss without the
             total variation (a basis has no patch grid)
    plan     loss, gradient and H v as tests/_patch_ref.plan returns them
Nothing of the terms or the voxel is restated here.  Anchored by tests/test_basis_reference.py: the translation basis IS the
"2d-translation" warp, and a basis made of the columns of tests/_patch_ref.patch_to_dense reproduces tests/_patch_ref.plan."""
import numpy as np
import torch

import _flow_ref
import _hvp_ref
import _patch_ref


def _basis(spec):
    return torch.as_tensor(np.ascontiguousarray(spec["basis"], dtype=np.float64))


def motion(theta, spec):
    """The motion the fused terms see, as a differentiable tensor: [2,H,W] or [T,2,H,W].  spec: basis [K,2,H,W], t_scale, round32
    and, time-aware, T / scheme / t0."""
    held = _patch_ref._as_device_holds if spec.get("round32", True) else (lambda m: m)
    D = torch.einsum("k,kchw->chw", theta.reshape(-1), _basis(spec)) * spec["t_scale"]
    if not spec.get("time_aware"):
        return held(D)
    return held(_flow_ref.voxel(D, spec["T"], spec["scheme"], spec["t0"]))


def loss(theta, events, spec):
    """spec: size, basis, t_scale, terms [(cost, weight)], sigma, omit and the keys of `motion`."""
    m = motion(theta, spec)
    model = "dense-flow-voxel" if spec.get("time_aware") else "dense-flow"
    out = 0.0
    for cost, w in spec["terms"]:
        out = out + w * _hvp_ref.objective(events, m, model, spec["size"], cost=cost, sigma=spec["sigma"], omit_boundary=spec.get("omit", True))
    return out


def plan(theta, events, spec, v=None):
    """-> (loss, grad [K], H v or None) in fp64 numpy."""
    ev = torch.as_tensor(np.ascontiguousarray(events, dtype=np.float64))
    xt = torch.as_tensor(np.ascontiguousarray(theta, dtype=np.float64)).reshape(-1).clone().requires_grad_()
    val = loss(xt, ev, spec)
    (g,) = torch.autograd.grad(val, xt, create_graph=v is not None)
    hv = None
    if v is not None:
        vt = torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64)).reshape(-1)
        hv = torch.zeros_like(xt)
        if g.requires_grad:
            (h,) = torch.autograd.grad((g * vt).sum(), xt, allow_unused=True)
            hv = hv if h is None else h
        hv = hv.detach().numpy().copy()
    return float(val.detach()), g.detach().numpy().copy(), hv


def device_motion(theta, spec):
    """`motion` as fp64 numpy (what the border filter of the product tests warps with)."""
    with torch.no_grad():
        return motion(torch.as_tensor(np.ascontiguousarray(theta, dtype=np.float64)).reshape(-1), spec).numpy().copy()
