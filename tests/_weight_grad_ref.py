"""The fp64 value dL/dw of the fused objective is held to, COMPOSED from the committed oracle the way tests/_weighted_ref.py composes the
loss: weighted_objective gives the image gradients; per reference time G = blur3_adj(dL/d image) is interpolated at the warped events by
orc.vote_bwd(..., want_gw=True) (gw of orc_vote_bwd in oracle/cmax_oracle.c: the derivative of the weighted vote with respect to the
event's weight, NOT multiplied by it), and the same on the un-warped events with the gradient of orig_iwe where the cost reads it."""
import numpy as np

from oracle import oracle as orc

from _weighted_ref import weighted_objective


def orig_image_grad(cost, iwes, omit_boundary, direction):
    """dL/d orig_iwe of a normalised / multi-focal cost, from the oracle's own contrast and its image gradient (orc._base_cost).  The
    oracle's cost_and_image_grads leaves this image out -- it does not depend on the motion -- but it is a weighted vote too:
    L = sum_k m_k v2 / v1_k (minimize) or sum_k m_k v1_k / v2 (multi-focal "maximize": negated), v2 the contrast of orig_iwe, which is
    not boundary-cropped for the variance (oracle.py, _cost_and_image_grads)."""
    kind = "var" if cost.endswith("image_variance") else "gm"
    v2, G2 = orc._base_cost(kind, iwes["orig_iwe"], omit_boundary if kind == "gm" else False)
    if cost.startswith("multi_focal"):
        members = [(k, m) for k, m in (("forward_iwe", 1.0), ("backward_iwe", 1.0), ("middle_iwe", 2.0)) if k in iwes]
    else:
        members = [("iwe", 1.0)]
    coef = 0.0
    for key, mult in members:
        v1, _ = orc._base_cost(kind, iwes[key], omit_boundary)
        coef += mult / v1 if direction == "minimize" else -mult * v1 / (v2 * v2)
    if cost.startswith("multi_focal") and direction == "maximize":
        coef = -coef
    return coef * G2


def weight_grad_objective(events, motion, motion_model, image_size, weight, cost="image_variance", sigma=0, outer_padding=0,
                          omit_boundary=True, direction="minimize", normalize_t=True, warp_direction="first", with_orig=True):
    """weighted_objective's dictionary plus "grad_w" [n].  with_orig=False leaves the un-warped image's term out (what a
    implementation that forgets it would return: used to show that a test sees the term)."""
    out = weighted_objective(events, motion, motion_model, image_size, weight, cost=cost, sigma=sigma, outer_padding=outer_padding,
                             omit_boundary=omit_boundary, direction=direction, normalize_t=normalize_t, want_grad=True,
                             warp_direction=warp_direction)
    ev = orc._ev4(events)
    w = np.ascontiguousarray(weight, dtype=np.float64) if isinstance(weight, np.ndarray) else float(weight)
    merged = {}
    for k, g in out["image_grads"].items():  # iwe and backward_iwe alias the same tensor in the reference: gradients add
        kk = "iwe" if k == "backward_iwe" else k
        merged[kk] = merged.get(kk, 0) + g
    if "orig_iwe" in out["iwes"] and "orig_iwe" not in merged:
        merged["orig_iwe"] = orig_image_grad(cost, out["iwes"], omit_boundary, direction)
    total = np.zeros(ev.shape[0])
    for key, G in merged.items():
        if key == "orig_iwe":
            if not with_orig:
                continue
            xy = ev
        else:
            xy, _ = orc.warp_event(ev, motion, motion_model, warp_direction if key == "iwe" else orc._KEY_DIRECTION[key], image_size,
                                   normalize_t)
        G = np.ascontiguousarray(G, dtype=np.float64)
        if sigma > 0:
            G = orc.blur3_adj(G, sigma)
        _, _, gw = orc.vote_bwd(xy, image_size, G, outer_padding, w, want_gw=True)
        total += gw
    out["grad_w"] = total
    return out
