"""TEST INFRASTRUCTURE ONLY: the fp64 value the solver side (csrc/cmax_patch_kernels.h, k_patch_tail and the patch plan of
csrc/cmax_solver.hip) is held to.

A torch-CPU restatement of what PatchFlowObjective hands the optimiser, written from the reference's formulas so that autograd supplies
every derivative:
    patch_to_dense      interpolate_dense_flow_from_patch_tensor (src/solver/patch_contrast_base.py:462-506), literally: negate,
                        replicate-pad, F.interpolate(bilinear, align_corners=False), centre crop
    total_variation     TotalVariation.calculate_torch (src/costs/total_variation.py:60-75, 110-126): mean |Sobel / 8| over the four
                        responses of a [2, ph, pw] grid, zero-padded correlation, cropped by one cell only when omit and ph > 2 and pw > 2;
                        torch.abs has the sub-gradient 0 at 0
    plan                cmax_patch_plan_evaluate / _hvp: D = P x [-> voxel] -> sum of the fused terms + w_tv TV(x); the fused terms come
                        from tests/_hvp_ref.py, the voxel from tests/_flow_ref.py, neither is restated here
The fused terms are evaluated on the motion THE DEVICE HOLDS: the plan interpolates and propagates in fp64 and rounds the displacement
field (or voxel) to fp32 once; the reference rounds it the same way and chains through the rounding straight-through
(tests/test_gpu_hvp_parity.py does the same for a bare flow).  Anchored to the C oracle and the committed fixtures by
tests/test_patch_reference.py."""
import numpy as np
import torch

import _flow_ref
import _hvp_ref

_SOBEL_ROW = torch.tensor([[-1.0, -2.0, -1.0], [0.0, 0.0, 0.0], [1.0, 2.0, 1.0]], dtype=torch.float64)


def patch_pad(patch_size, sliding_window, patch_shift=(0, 0)):
    """pad_h, pad_w (patch_contrast_base.py:470-479)."""
    return tuple(int(patch_size[k] / 2 // sliding_window[k]) + patch_shift[k] // sliding_window[k] + 1 for k in range(2))


def patch_to_dense(m, size, sw, pad):
    """m [2, ph, pw] fp64 tensor -> [2, H, W]."""
    H, W = int(size[0]), int(size[1])
    _, ph, pw = m.shape
    gh, gw = ph + 2 * int(pad[0]), pw + 2 * int(pad[1])
    p = torch.nn.functional.pad((-m)[None], (int(pad[1]), int(pad[1]), int(pad[0]), int(pad[0])), mode="replicate")
    up = torch.nn.functional.interpolate(p, size=(gh * int(sw[0]), gw * int(sw[1])), mode="bilinear", align_corners=False)[0]
    h1, w1 = (gh * int(sw[0])) // 2 - H // 2, (gw * int(sw[1])) // 2 - W // 2
    assert h1 >= 0 and w1 >= 0 and h1 + H <= up.shape[1] and w1 + W <= up.shape[2], "the up-sampled grid does not cover the sensor"
    return up[:, h1:h1 + H, w1:w1 + W]


def patch_to_dense_numpy(m, size, sw, pad):
    return patch_to_dense(torch.as_tensor(np.ascontiguousarray(m, dtype=np.float64)), size, sw, pad).numpy().copy()


def patch_to_dense_adj_numpy(gflow, patch_image_size, size, sw, pad):
    """P^T gflow by autograd."""
    m = torch.zeros((2, int(patch_image_size[0]), int(patch_image_size[1])), dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad((patch_to_dense(m, size, sw, pad) * torch.as_tensor(np.ascontiguousarray(gflow, dtype=np.float64))).sum(), m)
    return g.numpy().copy()


def total_variation(x, omit):
    """x [2, ph, pw] fp64 tensor -> scalar tensor."""
    _, ph, pw = x.shape
    k = torch.stack([_SOBEL_ROW, _SOBEL_ROW.t()])[:, None]
    g = torch.nn.functional.conv2d(x[:, None], k, padding=1) / 8.0  # [2 channels, 2 responses, ph, pw]
    if omit and ph > 2 and pw > 2:
        g = g[..., 1:-1, 1:-1]
    return torch.mean(torch.abs(g))


def total_variation_numpy(x, omit):
    """-> (TV, dTV/dx) in fp64 numpy."""
    xt = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64)).clone().requires_grad_()
    tv = total_variation(xt, omit)
    (g,) = torch.autograd.grad(tv, xt)
    return float(tv.detach()), g.numpy().copy()


def _as_device_holds(m):
    """fp32-rounded values, the derivative of the identity."""
    return m + (m.detach().float().double() - m.detach())


def motion(x, spec):
    """The motion the fused terms see, as a differentiable tensor: [2,H,W] or [T,2,H,W], rounded to fp32 straight-through."""
    ph, pw = spec["patch_image_size"]
    held = _as_device_holds if spec.get("round32", True) else (lambda m: m)  # round32 False: the reference solver's own fp64 chain
    D = patch_to_dense(x.reshape(2, ph, pw), spec["size"], spec["sw"], spec["pad"])
    if not spec.get("time_aware"):
        return held(D * spec["t_scale"])
    T, scheme, t0 = spec["T"], spec["scheme"], spec["t0"]
    if spec.get("scale_later"):
        s = D.max()
        return held(s * _flow_ref.voxel(D * spec["t_scale"] / s, T, scheme, t0))
    return held(_flow_ref.voxel(D * spec["t_scale"], T, scheme, t0))


def loss(x, events, spec, with_tv=True):
    """spec: size, patch_image_size, sw, pad, t_scale, terms [(cost, weight)], sigma, tv_weight, tv_omit and, time-aware, T / scheme /
    t0 / scale_later.  events [n, 4] fp64 tensor, x [2 ph pw] fp64 tensor."""
    m = motion(x, spec)
    model = "dense-flow-voxel" if spec.get("time_aware") else "dense-flow"
    out = 0.0
    for cost, w in spec["terms"]:
        out = out + w * _hvp_ref.objective(events, m, model, spec["size"], cost=cost, sigma=spec["sigma"], omit_boundary=spec.get("omit", True))
    if with_tv and spec.get("tv_weight", 0.0) != 0.0:
        ph, pw = spec["patch_image_size"]
        out = out + spec["tv_weight"] * total_variation(x.reshape(2, ph, pw), spec.get("tv_omit", True))
    return out


def plan(x, events, spec, v=None, with_tv=True):
    """-> (loss, grad [2 ph pw], H v or None) in fp64 numpy: one backward pass, and a second one through it when `v` is given."""
    ev = torch.as_tensor(np.ascontiguousarray(events, dtype=np.float64))
    xt = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64)).reshape(-1).clone().requires_grad_()
    val = loss(xt, ev, spec, with_tv)
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


def device_motion(x, spec):
    """The fp32 motion of `motion` as fp64 numpy (what the border filter of the Hessian-vector tests warps with)."""
    with torch.no_grad():
        return motion(torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64)).reshape(-1), spec).numpy().copy()
