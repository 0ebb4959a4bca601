"""TEST INFRASTRUCTURE ONLY: the fp64 value the fused focus losses (CMAX_COST_MEAN_SQUARE / _LAPLACIAN / _HESSIAN) are held to.

Three torch `kind` functions -- conv2d with the stencil of include/cmax_hip.h on the zero-padded image, crop to Omega, mean -- plugged
into the warp / vote / blur / normalised / multi-focal composition of tests/_hvp_ref.py (its stages are imported, not copied; only the
few lines that compose them are restated here, with the un-warped image cropped like the warped one: the gradient-magnitude rule).
Value, gradient and H v as there: one backward pass, and a second one through it.  `weights` (per-event, vote-linear as in
tests/_weighted_ref.py) and the events themselves may carry requires_grad for dL/dw and dL/d(event)."""
import numpy as np
import torch

from _hvp_ref import _REFS, _blur3, _pad2, _vote, _warp, border_margin, cost_directions, drop_ambiguous  # noqa: F401

_T = lambda rows: torch.tensor(rows, dtype=torch.float64)  # noqa: E731
# (weight c_s, stencil S_s) per response; rows of a stencil are image rows r - 1, r, r + 1
STENCILS = {
    "mean_square": [(1.0, _T([[0, 0, 0], [0, 1, 0], [0, 0, 0]]))],
    "laplacian_magnitude": [(1.0, _T([[0, 1, 0], [1, -4, 1], [0, 1, 0]]))],
    "hessian_magnitude": [(1.0, _T([[0, 1, 0], [0, -2, 0], [0, 1, 0]])), (1.0, _T([[0, 0, 0], [1, -2, 1], [0, 0, 0]])),
                          (2.0, _T([[0.25, 0, -0.25], [0, 0, 0], [-0.25, 0, 0.25]]))],
}
KINDS = tuple(STENCILS)


def kind_of(cost):
    for k in KINDS:
        if cost.endswith(k):
            return k
    raise KeyError(cost)


def focus_value(img, kind, omit):
    """(1/n) sum_Omega sum_s c_s (S_s * img)^2, img read as zero outside itself (conv2d is a correlation: the stencil as written)."""
    total = 0.0
    for c, s in STENCILS[kind]:
        r = torch.nn.functional.conv2d(img[None, None], s[None, None].to(img.dtype), padding=1)[0, 0]
        if omit:
            r = r[1:-1, 1:-1]
        total = total + c * torch.mean(r ** 2)
    return total


def _vote_weighted(x, y, size, pad, w):
    """_hvp_ref._vote with every event's four shares multiplied by its weight (the vote is linear in it)."""
    (H, W), (ph, pw) = size, pad
    Hp, Wp = H + 2 * ph, W + 2 * pw
    fx, fy = torch.floor(x + 1e-6), torch.floor(y + 1e-6)
    a, b = x - fx, y - fy
    r0, c0 = fx.long() + ph, fy.long() + pw
    img = torch.zeros(Hp * Wp, dtype=x.dtype)
    for dr, dc, share in ((0, 0, (1 - a) * (1 - b)), (1, 0, a * (1 - b)), (0, 1, (1 - a) * b), (1, 1, a * b)):
        r, c = r0 + dr, c0 + dc
        ok = (r >= 0) & (r < Hp) & (c >= 0) & (c < Wp)
        img = img.scatter_add(0, torch.where(ok, r * Wp + c, torch.zeros_like(r)), torch.where(ok, w * share, torch.zeros_like(share)))
    return img.reshape(Hp, Wp)


def objective(ev, m, model, size, cost, sigma=0, outer_padding=0, omit_boundary=True, direction="minimize", warp_direction="first",
              normalize_t=True, t_range=None, weights=None):
    """The loss as a torch scalar, differentiable (twice) in `m`, and in `ev` / `weights` where they require it."""
    size, pad = (int(size[0]), int(size[1])), _pad2(outer_padding)
    kind = kind_of(cost)
    normalized, multi = "normalized" in cost, cost.startswith("multi_focal")

    def image(x, y):
        img = _vote(x, y, size, pad) if weights is None else _vote_weighted(x, y, size, pad, weights)
        return _blur3(img, sigma) if sigma > 0 else img

    def contrast(key_direction):
        x, y, _ = _warp(ev, m, model, size, key_direction, normalize_t, t_range)
        return focus_value(image(x, y), kind, omit_boundary)

    if not normalized:
        v = contrast(warp_direction)
        return -v if direction == "minimize" else v
    v2 = focus_value(image(ev[:, 0], ev[:, 1]), kind, omit_boundary)
    loss = 0.0
    for key_direction, mult in _REFS[3 if multi else 1]:
        v1 = contrast(warp_direction if key_direction is None else key_direction)
        loss = loss + mult * (v2 / v1 if direction == "minimize" else v1 / v2)
    return -loss if (multi and direction == "maximize") else loss


def value_grad_hvp(events, motion, model, size, v=None, **kw):
    """-> (loss, grad, Hv or None) in fp64 numpy."""
    ev = torch.as_tensor(np.ascontiguousarray(events, dtype=np.float64))
    m = torch.as_tensor(np.ascontiguousarray(motion, dtype=np.float64)).clone().requires_grad_()
    loss = objective(ev, m, model, size, **kw)
    (g,) = torch.autograd.grad(loss, m, create_graph=v is not None)
    hv = None
    if v is not None:
        vt = torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64)).reshape(m.shape)
        (hv,) = torch.autograd.grad((g * vt).sum(), m, allow_unused=True)
        hv = (torch.zeros_like(m) if hv is None else hv).detach().numpy().copy()
    return float(loss.detach()), g.detach().numpy().copy(), hv


def numpy_loops(img, kind, omit):
    """The definitions of include/cmax_hip.h as direct loops (the anchor of focus_value)."""
    H, W = img.shape
    at = lambda r, c: float(img[r, c]) if 0 <= r < H and 0 <= c < W else 0.0  # noqa: E731
    i0 = 1 if omit else 0
    total, n = 0.0, 0
    for r in range(i0, H - i0):
        for c in range(i0, W - i0):
            n += 1
            if kind == "mean_square":
                total += at(r, c) ** 2
            elif kind == "laplacian_magnitude":
                total += (at(r - 1, c) + at(r + 1, c) + at(r, c - 1) + at(r, c + 1) - 4.0 * at(r, c)) ** 2
            else:
                hrr = at(r - 1, c) - 2.0 * at(r, c) + at(r + 1, c)
                hcc = at(r, c - 1) - 2.0 * at(r, c) + at(r, c + 1)
                hrc = 0.25 * (at(r + 1, c + 1) - at(r + 1, c - 1) - at(r - 1, c + 1) + at(r - 1, c - 1))
                total += hrr ** 2 + 2.0 * hrc ** 2 + hcc ** 2
    return total / n
