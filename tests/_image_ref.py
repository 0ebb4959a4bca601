"""TEST INFRASTRUCTURE ONLY: the fp64 values the image-side kernels are held to (tests/test_gpu_image_side.py).

Whole-call evaluations are compared with the committed oracle (orc.objective), as in tests/test_gpu_fused.py.  For an image the CALLER
supplies -- cmax_objective_finish on objective_vote(...) + offset -- `objective_from_images` composes the pieces of tests/_hvp_ref.py
(warp, vote, blur, contrasts, the normalised and multi-focal forms) into the same loss evaluated on vote(ev, m) + offsets[k], before
the blur.  The offset is a constant, so autograd's gradient in m is the gather of G(image + offset) at the events' warped positions:
what cmax_objective_finish computes.  tests/test_image_reference.py anchors it: zero offsets give _hvp_ref.objective exactly, and with
offsets its gradient agrees with central finite differences.

`conditioning` is the criterion for a cancelling gradient: |g|_inf over the largest sum of the per-event absolute contributions."""
import numpy as np
import torch

from oracle import oracle as orc

import _hvp_ref as R


def objective_from_images(ev, m, model, size, offsets, cost="image_variance", sigma=0, outer_padding=0, omit_boundary=True, direction="minimize",
                          warp_direction="first", normalize_t=True, t_range=None, images_out=None):
    """_hvp_ref.objective with offsets[k] ([Hp, Wp], fp64) added to the votes of image slot k: one slot per reference time in the cost's
    own order (multi-focal: last, first, middle), then the un-warped image of a normalised cost.  images_out: a list that receives the
    images the contrasts were evaluated on (blurred when sigma > 0), detached, in slot order."""
    size, pad = (int(size[0]), int(size[1])), R._pad2(outer_padding)
    if not (cost.endswith("image_variance") or cost.endswith("gradient_magnitude")):
        raise KeyError(cost)
    kind = R._variance if cost.endswith("image_variance") else R._gradmag
    normalized, multi = "normalized" in cost, cost.startswith("multi_focal")
    refs = R._REFS[3 if multi else 1]
    assert len(offsets) == len(refs) + (1 if normalized else 0)
    offsets = [torch.as_tensor(np.ascontiguousarray(o, dtype=np.float64)) for o in offsets]

    def image(x, y, slot):
        img = R._vote(x, y, size, pad) + offsets[slot]
        img = R._blur3(img, sigma) if sigma > 0 else img
        if images_out is not None:
            images_out.append(img.detach().numpy().copy())
        return img

    def contrast(slot, key_direction):
        x, y, _ = R._warp(ev, m, model, size, key_direction, normalize_t, t_range)
        return kind(image(x, y, slot), omit_boundary)

    if not normalized:
        v = contrast(0, warp_direction)
        return -v if direction == "minimize" else v
    v1s = [contrast(k, warp_direction if key is None else key) for k, (key, _) in enumerate(refs)]
    v2 = kind(image(ev[:, 0], ev[:, 1], len(refs)), omit_boundary if kind is R._gradmag else False)
    loss = 0.0
    for v1, (_, mult) in zip(v1s, refs):
        loss = loss + mult * (v2 / v1 if direction == "minimize" else v1 / v2)
    return -loss if (multi and direction == "maximize") else loss


def value_grad_images(events, motion, model, size, offsets, **kw):
    """-> (loss, grad, [images]) in fp64 numpy"""
    ev = torch.as_tensor(np.ascontiguousarray(events, dtype=np.float64))
    m = torch.as_tensor(np.ascontiguousarray(motion, dtype=np.float64)).clone().requires_grad_()
    images = []
    loss = objective_from_images(ev, m, model, size, offsets, images_out=images, **kw)
    (g,) = torch.autograd.grad(loss, m)
    return float(loss.detach()), g.numpy().copy(), images


def vote_images(events, motion, model, size, cost, outer_padding=0):
    """the raw votes of every image slot, fp64 [n_slots, Hp, Wp]"""
    with torch.no_grad():
        ev = torch.as_tensor(np.ascontiguousarray(events, dtype=np.float64))
        m = torch.as_tensor(np.ascontiguousarray(motion, dtype=np.float64))
        size, pad = (int(size[0]), int(size[1])), R._pad2(outer_padding)
        out = []
        for d in R.cost_directions(cost):
            x, y, _ = R._warp(ev, m, model, size, d, True, None)
            out.append(R._vote(x, y, size, pad).numpy())
        if "normalized" in cost:
            out.append(R._vote(ev[:, 0], ev[:, 1], size, pad).numpy())
    return np.stack(out)


_IWE_KEYS = {1: ("iwe",), 3: ("forward_iwe", "iwe", "middle_iwe")}  # slot order of the handle's images (multi-focal: last, first, middle)


def oracle_images(ref, cost):
    """the images of an orc.objective result in slot order (what CMaxHandle.last_iwe(k) returns)"""
    return [ref["iwes"][k] for k in _IWE_KEYS[3 if cost.startswith("multi_focal") else 1]]


def coverage(events, motion, model, size, cost, outer_padding=0):
    """[n_ref, Hp, Wp] bool: the pixels of the padded image that are a bilinear corner of at least one event, per reference time, from
    the reference's warped coordinates."""
    (H, W), (ph, pw) = (int(size[0]), int(size[1])), R._pad2(outer_padding)
    Hp, Wp = H + 2 * ph, W + 2 * pw
    out = []
    for d in R.cost_directions(cost):
        x, y = R._warped_numpy(events, motion, model, size, d)
        r0, c0 = np.floor(x + 1e-6).astype(np.int64) + ph, np.floor(y + 1e-6).astype(np.int64) + pw
        hit = np.zeros((Hp, Wp), dtype=bool)
        for dr, dc in ((0, 0), (1, 0), (0, 1), (1, 1)):
            r, c = r0 + dr, c0 + dc
            ok = (r >= 0) & (r < Hp) & (c >= 0) & (c < Wp)
            hit[r[ok], c[ok]] = True
        out.append(hit)
    return np.stack(out)


def conditioning(events, motion, model, size, ref, sigma=0, outer_padding=0):
    """|g|_inf / max_j sum_e |contribution of event e to g_j|, from an orc.objective result: j a component of theta (2-DoF) or of one
    pixel's flow (dense).  Below 1e-3 the gradient is a cancelling sum and no fp32 evaluation can be held to 1e-4 of it."""
    ev = orc._ev4(events)
    merged = {}
    for k, g in ref["image_grads"].items():
        kk = "iwe" if k == "backward_iwe" else k
        merged[kk] = merged.get(kk, 0) + g
    H, W = int(size[0]), int(size[1])
    total = np.zeros(2) if model == "2d-translation" else np.zeros((2, H * W))
    for key, G in merged.items():
        if key == "orig_iwe":
            continue
        warped, aux = orc.warp_event(ev, motion, model, orc._KEY_DIRECTION[key], size, True)
        G = np.ascontiguousarray(G, dtype=np.float64)
        if sigma > 0:
            G = orc.blur3_adj(G, sigma)
        gx, gy = orc.vote_bwd(warped, size, G, outer_padding)
        ax, ay = np.abs(aux["dt"] * gx), np.abs(aux["dt"] * gy)
        if model == "2d-translation":
            total += np.array([ax.sum(), ay.sum()])
        else:
            src = ev[:, 0].astype(np.int64) * W + ev[:, 1].astype(np.int64)
            np.add.at(total[0], src, ax)
            np.add.at(total[1], src, ay)
    return float(np.abs(ref["grad"]).max() / max(total.max(), 1e-300))


def fp32_statistics_error(events, motion, model, size, ref, omit_boundary, outer_padding=0):
    """-> (loss, gradient): the relative error a variance contrast and a normalised cost's gradient pick up when sum I^2 over Omega is
    made of fp32 terms (the deferred 2-DoF variance).  v = (sum I^2 - (sum I)^2 / n) / (n - 1), so one fp32 rounding
    u = 2^-24 of sum I^2 is kappa u of v, kappa = sum I^2 / sum (I - mean)^2.  A normalised cost is sum_k m_k v2 / v1_k: its gradient
    g = sum_k g_k has g_k ~ v2 / v1_k^2, off by (2 kappa_k + kappa_orig) u each; the plain variance's gradient 2 (I - mean) / (n - 1) does
    not read sum I^2.  From an orc.objective result, in fp64; sigma = 0 (the deferred path has no blur)."""
    u = 2.0 ** -24

    def kappa(img, omit):
        om = np.asarray(img, dtype=np.float64)
        om = om[1:-1, 1:-1] if omit else om
        return float((om * om).sum() / max(((om - om.mean()) ** 2).sum(), 1e-300))

    ks = {k: kappa(img, omit_boundary if k != "orig_iwe" else False) for k, img in ref["iwes"].items()}  # (the un-warped variance is not cropped)
    e_loss = max(ks.values()) * u
    if "orig_iwe" not in ks:
        return e_loss, 0.0
    ev = orc._ev4(events)
    merged = {}
    for k, g in ref["image_grads"].items():
        kk = "iwe" if k == "backward_iwe" else k
        merged[kk] = merged.get(kk, 0) + g
    total = 0.0
    for key, G in merged.items():
        if key == "orig_iwe":
            continue
        warped, aux = orc.warp_event(ev, motion, model, orc._KEY_DIRECTION[key], size, True)
        gx, gy = orc.vote_bwd(warped, size, np.ascontiguousarray(G, dtype=np.float64), outer_padding)
        gk = orc.motion_grad(ev, motion, model, aux, gx, gy)
        total += (2.0 * ks[key] + ks["orig_iwe"]) * u * float(np.abs(gk).max())
    return e_loss, total / float(np.abs(ref["grad"]).max())
