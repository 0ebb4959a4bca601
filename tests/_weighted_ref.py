"""The fp64 value the weighted fused objective is held to, COMPOSED from the committed oracle (oracle/oracle.py) -- the steps of
orc.objective with the per-event weight applied exactly where the reference's bilinear_vote_tensor applies it
(src/event_image_converter.py:330-331, 365-372): warp_event -> vote(weight=w) per reference time (and of the un-warped events where the
cost reads orig_iwe) -> blur3 -> cost_and_image_grads -> blur3_adj -> vote_bwd(weight=w) -> motion_grad.  With w == 1 it reproduces
orc.objective (tests/test_weights_host.py): the composition is the oracle's, not a second implementation."""
import numpy as np

from oracle import oracle as orc


def weighted_objective(events, motion, motion_model, image_size, weight, cost="image_variance", sigma=0, outer_padding=0,
                       omit_boundary=True, direction="minimize", normalize_t=True, want_grad=True, warp_direction="first"):
    ev = orc._ev4(events)
    w = np.ascontiguousarray(weight, dtype=np.float64) if isinstance(weight, np.ndarray) else float(weight)
    keys = orc.required_keys(cost, None)
    iwes, ctx = {}, {}

    def image(xy):
        img = orc.vote(xy, image_size, outer_padding, w)
        return orc.blur3(img, sigma) if sigma > 0 else img

    if "orig_iwe" in keys:
        iwes["orig_iwe"] = image(ev)
    need = [k for k in ("iwe", "backward_iwe", "forward_iwe", "middle_iwe") if k in keys]
    if "iwe" in need or "backward_iwe" in need:
        need = [k for k in need if k not in ("iwe", "backward_iwe")] + ["iwe"]
    for key in need:
        warped, aux = orc.warp_event(ev, motion, motion_model, warp_direction if key == "iwe" else orc._KEY_DIRECTION[key], image_size,
                                     normalize_t)
        ctx[key] = (warped, aux)
        iwes[key] = image(warped)
        if key == "iwe":
            iwes["backward_iwe"] = iwes[key]
    loss, image_grads, _ = orc.cost_and_image_grads(cost, iwes, omit_boundary, direction, None, None)
    out = {"loss": loss, "iwes": iwes, "image_grads": image_grads, "grad": None}
    if not want_grad:
        return out
    merged = {}
    for k, g in image_grads.items():  # iwe and backward_iwe alias the same tensor in the reference: gradients add
        kk = "iwe" if k == "backward_iwe" else k
        merged[kk] = merged.get(kk, 0) + g
    total = None
    for key, G in merged.items():
        if key not in ctx:
            continue
        warped, aux = ctx[key]
        if sigma > 0:
            G = orc.blur3_adj(G, sigma)
        gx, gy = orc.vote_bwd(warped, image_size, G, outer_padding, w)
        g = orc.motion_grad(ev, motion, motion_model, aux, gx, gy)
        total = g if total is None else total + g
    if total is None:
        total = np.zeros_like(np.asarray(motion, dtype=np.float64))
    out["grad"] = total
    return out


def weight_set(name, events, seed=0):
    """The weight sets of the parity tests."""
    rng = np.random.default_rng(seed)
    n = events.shape[0]
    if name == "uniform":
        return rng.uniform(0.2, 3.0, n)
    if name == "polarity":
        return np.where(events[:, 3] > 0, 1.0, -1.0)
    if name == "zeros":  # about 10 % zeros
        w = rng.uniform(0.2, 3.0, n)
        w[rng.uniform(0, 1, n) < 0.1] = 0.0
        return w
    if name == "hdr":  # one weight 1000 x the rest: exercises the normalisation by wmax
        w = rng.uniform(0.5, 1.0, n)
        w[n // 3] = 1000.0
        return w
    raise KeyError(name)
