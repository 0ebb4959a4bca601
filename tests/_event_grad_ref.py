"""TEST INFRASTRUCTURE ONLY: the fp64 values dL/d(event) of the fused objective (cmax_objective_event_grad) is held to.

Two references:
  events_grad_autograd   the reference's `events.grad` [n, 4] (its solvers mark the events as a leaf, src/solver/patch_contrast_mixed.py:166):
                         torch fp64 autograd through tests/_hvp_ref.objective with ev.requires_grad_() -- that restatement is anchored on
                         the oracle at 1e-10 and is differentiable in ev (source pixel and bin are integers: piecewise constant;
                         t.min() / t.max() are on the tape).  Unweighted only.
  event_grad_objective   what the C entry itself returns -- grad_events [n, 3] = (dL/dx, dL/dy, C = sum_k dL/d dt_k) and csum[k] -- COMPOSED
                         from the committed oracle the way tests/_weighted_ref.py composes the loss: orc.vote_bwd(..., w) per reference
                         time plus the orig_iwe term (tests/_weight_grad_ref.orig_image_grad), dt-derivative from the warp's own formula.
                         Weighted or not.
tests/test_event_grad_reference.py holds them against each other (through cmax.compose_events_grad) and against finite differences."""
import numpy as np
import torch

from oracle import oracle as orc

import _hvp_ref
from _weight_grad_ref import orig_image_grad
from _weighted_ref import weighted_objective

# the descriptor's order of reference times (cmax._COST_TABLE): multi-focal = last, first, middle
_MULTI_KEYS = ("forward_iwe", "iwe", "middle_iwe")


def events_grad_autograd(events, motion, model, size, **kw):
    """-> (loss, events.grad [n, 4]) in fp64 numpy."""
    ev = torch.as_tensor(np.ascontiguousarray(events, dtype=np.float64)).clone().requires_grad_()
    m = torch.as_tensor(np.ascontiguousarray(motion, dtype=np.float64))
    loss = _hvp_ref.objective(ev, m, model, size, **kw)
    (g,) = torch.autograd.grad(loss, ev)
    return float(loss.detach()), g.numpy().copy()


def event_grad_objective(events, motion, motion_model, image_size, weight=1.0, cost="image_variance", sigma=0, outer_padding=0,
                         omit_boundary=True, direction="minimize", normalize_t=True, warp_direction="first"):
    """weighted_objective's dictionary plus "grad_events" [n, 3] and "csum" [4]."""
    out = weighted_objective(events, motion, motion_model, image_size, weight, cost=cost, sigma=sigma, outer_padding=outer_padding,
                             omit_boundary=omit_boundary, direction=direction, normalize_t=normalize_t, want_grad=True,
                             warp_direction=warp_direction)
    ev = orc._ev4(events)
    n = ev.shape[0]
    w = np.ascontiguousarray(weight, dtype=np.float64) if isinstance(weight, np.ndarray) else float(weight)
    m = np.asarray(motion, dtype=np.float64)
    merged = {}
    for k, g in out["image_grads"].items():  # iwe and backward_iwe alias the same tensor in the reference: gradients add
        kk = "iwe" if k == "backward_iwe" else k
        merged[kk] = merged.get(kk, 0) + g
    if "orig_iwe" in out["iwes"] and "orig_iwe" not in merged:
        merged["orig_iwe"] = orig_image_grad(cost, out["iwes"], omit_boundary, direction)
    order = _MULTI_KEYS if cost.startswith("multi_focal") else ("iwe",)
    ge, csum = np.zeros((n, 3)), np.zeros(4)
    H, W = int(image_size[0]), int(image_size[1])
    src = ev[:, 0].astype(np.int64) * W + ev[:, 1].astype(np.int64)  # (the C cast: toward zero)
    for key, G in merged.items():
        G = np.ascontiguousarray(G, dtype=np.float64)
        if sigma > 0:
            G = orc.blur3_adj(G, sigma)
        if key == "orig_iwe":
            gx, gy = orc.vote_bwd(ev, image_size, G, outer_padding, w)
            ge[:, 0] += gx
            ge[:, 1] += gy
            continue
        xy, aux = orc.warp_event(ev, motion, motion_model, warp_direction if key == "iwe" else orc._KEY_DIRECTION[key], image_size, normalize_t)
        gx, gy = orc.vote_bwd(xy, image_size, G, outer_padding, w)
        if motion_model == "2d-translation":  # x' = x + dt theta
            c = gx * m[0] + gy * m[1]
        elif motion_model == "dense-flow":  # x' = x - dt F[:, src]
            f = m.reshape(2, H * W)
            c = -(gx * f[0][src] + gy * f[1][src])
        else:
            f = m.reshape(m.shape[0], 2, H * W)
            b = aux["bin"].astype(np.int64)
            ok = b >= 0
            bb = np.where(ok, b, 0)
            c = -np.where(ok, gx * f[bb, 0, src] + gy * f[bb, 1, src], 0.0)
        ge[:, 0] += gx
        ge[:, 1] += gy
        ge[:, 2] += c
        csum[order.index(key)] = c.sum()
    out["grad_events"], out["csum"] = ge, csum
    return out


def reference_fractions(cost, warp_direction="first"):
    """The reference times of `cost` as fractions of the batch period, in the descriptor's order."""
    f = {"first": 0.0, "middle": 0.5, "last": 1.0}
    if cost.startswith("multi_focal"):
        return [1.0, 0.0, 0.5]
    return [f[warp_direction] if isinstance(warp_direction, str) else float(warp_direction)]
