"""TEST INFRASTRUCTURE ONLY: the fp64 value the nearest patch filter and the single-scale patch solvers (solver/mixed.py) are held to.

A torch-CPU restatement chained from the existing references (tests/_patch_ref.py for the bilinear interpolation and the total
variation, tests/_flow_ref.py for the voxel, tests/_hvp_ref.py for the fused terms), so that autograd supplies every derivative:
    patch_to_dense      interpolate_dense_flow_from_patch_tensor (src/solver/patch_contrast_base.py:462-506) with `patch.filter_type`:
                        negate, replicate-pad, resize by the integer factors, centre crop.  "nearest": pixel (r, c) of the resized array
                        takes padded cell (r // sw_h, c // sw_w) -- an indexed copy, written as indexing so that nothing here goes
                        through F.interpolate (tests/test_mixed_reference.py holds the index rule to F.interpolate's own map)
    loss / plan         objective_scipy of the single-scale solvers (src/solver/patch_contrast_mixed.py:184-208): D = P (x t_scale)
                        [-> voxel] -> the fused terms + w_tv TV(x); `spec["filter"]` selects the filter
Anchored to tests/golden/solver_mixed.npz by tests/test_mixed_reference.py."""
import numpy as np
import torch

import _flow_ref
import _hvp_ref
import _patch_ref


def nearest_index(n_out, sw):
    """Padded cell of every line of the resized array along one axis: dst // sw."""
    return np.arange(int(n_out)) // int(sw)


def patch_to_dense(m, size, sw, pad, filter_type="bilinear"):
    """m [2, ph, pw] fp64 tensor -> [2, H, W]."""
    if filter_type == "bilinear":
        return _patch_ref.patch_to_dense(m, size, sw, pad)
    assert filter_type == "nearest", filter_type
    H, W = int(size[0]), int(size[1])
    _, ph, pw = m.shape
    gh, gw = ph + 2 * int(pad[0]), pw + 2 * int(pad[1])
    p = torch.nn.functional.pad((-m)[None], (int(pad[1]), int(pad[1]), int(pad[0]), int(pad[0])), mode="replicate")[0]
    rows = torch.as_tensor(nearest_index(gh * int(sw[0]), sw[0]))
    cols = torch.as_tensor(nearest_index(gw * int(sw[1]), sw[1]))
    up = p[:, rows][:, :, cols]
    h1, w1 = (gh * int(sw[0])) // 2 - H // 2, (gw * int(sw[1])) // 2 - W // 2
    assert h1 >= 0 and w1 >= 0 and h1 + H <= up.shape[1] and w1 + W <= up.shape[2], "the up-sampled grid does not cover the sensor"
    return up[:, h1:h1 + H, w1:w1 + W]


def patch_to_dense_numpy(m, size, sw, pad, filter_type="bilinear"):
    return patch_to_dense(torch.as_tensor(np.ascontiguousarray(m, dtype=np.float64)), size, sw, pad, filter_type).numpy().copy()


def patch_to_dense_adj_numpy(gflow, patch_image_size, size, sw, pad, filter_type="bilinear"):
    """P^T gflow by autograd."""
    m = torch.zeros((2, int(patch_image_size[0]), int(patch_image_size[1])), dtype=torch.float64, requires_grad=True)
    dense = patch_to_dense(m, size, sw, pad, filter_type)
    (g,) = torch.autograd.grad((dense * torch.as_tensor(np.ascontiguousarray(gflow, dtype=np.float64))).sum(), m)
    return g.numpy().copy()


def motion(x, spec):
    """The motion the fused terms see: [2,H,W] or [T,2,H,W]; rounded to fp32 straight-through unless spec["round32"] is False (the
    reference solver's own fp64 chain).  The interpolation is linear: P (x t_scale) = (P x) t_scale."""
    ph, pw = spec["patch_image_size"]
    held = _patch_ref._as_device_holds if spec.get("round32", True) else (lambda m: m)
    filt = spec.get("filter", "bilinear")
    if spec.get("time_aware") and spec.get("scale_later"):
        # the PLAN's scale_later (the pyramid solver's map, tests/_patch_ref.motion) under the filter; the single-scale solvers refuse it
        D = patch_to_dense(x.reshape(2, ph, pw), spec["size"], spec["sw"], spec["pad"], filt)
        s = D.max()
        return held(s * _flow_ref.voxel(D * spec["t_scale"] / s, spec["T"], spec["scheme"], spec["t0"]))
    D = patch_to_dense(x.reshape(2, ph, pw) * spec["t_scale"], spec["size"], spec["sw"], spec["pad"], filt)
    if not spec.get("time_aware"):
        return held(D)
    return held(_flow_ref.voxel(D, spec["T"], spec["scheme"], spec["t0"]))


def loss(x, events, spec, with_tv=True):
    m = motion(x, spec)
    model = "dense-flow-voxel" if spec.get("time_aware") else "dense-flow"
    out = 0.0
    for cost, w in spec["terms"]:
        out = out + w * _hvp_ref.objective(events, m, model, spec["size"], cost=cost, sigma=spec["sigma"], omit_boundary=spec.get("omit", True))
    if with_tv and spec.get("tv_weight", 0.0) != 0.0:
        ph, pw = spec["patch_image_size"]
        out = out + spec["tv_weight"] * _patch_ref.total_variation(x.reshape(2, ph, pw), spec.get("tv_omit", True))
    return out


def plan(x, events, spec, v=None, with_tv=True):
    """-> (loss, grad [2 ph pw], H v or None) in fp64 numpy, as tests/_patch_ref.plan."""
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
    with torch.no_grad():
        return motion(torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64)).reshape(-1), spec).numpy().copy()


def prepare_patch(image_size, patch_size, sliding_window):
    """patch_image_size of prepare_patch (patch_contrast_base.py:86-92)."""
    return tuple(len(np.arange(0, image_size[k] - patch_size[k] + sliding_window[k], sliding_window[k])) for k in (0, 1))
