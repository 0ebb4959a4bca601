"""TEST INFRASTRUCTURE ONLY: the fp64 value the exact Hessian-vector product (cmax_objective_hvp) is held to.

A differentiable torch-CPU restatement of the fused objective, written from the committed oracle (oracle/oracle.py composes the
stages, oracle/cmax_oracle.c states each of them) in the style of oracle/torch_cpu.py, which stays as it is because bench.py times it:
    reference time and dt       orc_reftime / orc_calculate_dt
    warps                       orc_warp_2dof / orc_warp_dense / orc_warp_voxel (the bin from the event's dt, edges k / T)
    votes                       orc_vote: cell floor(x' + 1e-6), fractions from the un-padded coordinate, corners masked by the PADDED image
    blur                        orc_blur3: three taps, reflect-101, separable
    costs                       orc_variance (unbiased), orc_gradmag (Sobel / 8 on the zero-padded image), and what
                                oracle._cost_and_image_grads makes of them: sign, normalised and multi-focal forms
Loss and gradient are anchored to orc.objective at 1e-10, the product to the committed vhp fixtures at 1e-9
(tests/test_hvp_reference.py); the product itself is a double backward, i.e. what torch.autograd.functional.vhp computes."""
import numpy as np
import torch

from _border import MARGIN

_SOBEL_ROW = torch.tensor([[-1.0, -2.0, -1.0], [0.0, 0.0, 0.0], [1.0, 2.0, 1.0]], dtype=torch.float64)
_FRACTION = {"first": 0.0, "middle": 0.5, "last": 1.0}
# which reference times a cost reads: (key direction, multiplier); None stands for the caller's warp_direction
_REFS = {1: ((None, 1.0),), 3: (("last", 1.0), ("first", 1.0), ("middle", 2.0))}


def _pad2(outer_padding):
    if isinstance(outer_padding, (int, float)):
        return int(outer_padding), int(outer_padding)
    return int(outer_padding[0]), int(outer_padding[1])


def cost_directions(cost, warp_direction="first"):
    """The reference times `cost` warps to."""
    return ["last", "first", "middle"] if cost.startswith("multi_focal") else [warp_direction]


def _dt(t, direction, normalize_t, t_range):
    lo, hi = (t.min(), t.max()) if t_range is None else (torch.as_tensor(t_range[0], dtype=t.dtype), torch.as_tensor(t_range[1], dtype=t.dtype))
    if direction == "first":
        tref = lo
    elif direction == "last":
        tref = hi
    else:
        tref = lo + (hi - lo) * float(_FRACTION.get(direction, direction))
    dt = t - tref
    if normalize_t:
        dt = dt / ((hi - tref) - (lo - tref))
    return dt


def _bins(dt, T):
    lo, hi = dt.min(), dt.max()
    b = torch.full(dt.shape, -1, dtype=torch.long)
    for k in range(T):  # later bins overwrite, the last edge lies beyond every event
        upper = (float(k + 1) / float(T)) * (hi - lo) + lo if k + 1 < T else hi + 1e3
        b = torch.where(((float(k) / float(T)) * (hi - lo) + lo <= dt) & (dt < upper), torch.full_like(b, k), b)
    return b


def _warp(ev, m, model, size, direction, normalize_t, t_range):
    """-> (x', y', dt): rows, columns and the time each event is moved by."""
    H, W = size
    x, y = ev[:, 0], ev[:, 1]
    dt = _dt(ev[:, 2], direction, normalize_t, t_range)
    if model == "2d-translation":
        return x + dt * m[0], y + dt * m[1], dt
    src = x.long() * W + y.long()  # .long() truncates toward zero like the C cast
    if model == "dense-flow":
        flat = m.reshape(2, H * W)
        return x - dt * flat[0][src], y - dt * flat[1][src], dt
    if model == "dense-flow-voxel":
        T = m.shape[0]
        b = _bins(dt, T)
        flat = m.reshape(T, 2, H * W)
        ok = b >= 0
        bb = torch.where(ok, b, torch.zeros_like(b))
        fx = torch.where(ok, flat[bb, 0, src], torch.zeros_like(dt))
        fy = torch.where(ok, flat[bb, 1, src], torch.zeros_like(dt))
        return x - dt * fx, y - dt * fy, dt
    raise KeyError(model)


def _vote(x, y, size, pad):
    (H, W), (ph, pw) = size, pad
    Hp, Wp = H + 2 * ph, W + 2 * pw
    fx, fy = torch.floor(x + 1e-6), torch.floor(y + 1e-6)
    a, b = x - fx, y - fy
    r0, c0 = fx.long() + ph, fy.long() + pw
    img = torch.zeros(Hp * Wp, dtype=x.dtype)
    for dr, dc, w in ((0, 0, (1 - a) * (1 - b)), (1, 0, a * (1 - b)), (0, 1, (1 - a) * b), (1, 1, a * b)):
        r, c = r0 + dr, c0 + dc
        ok = (r >= 0) & (r < Hp) & (c >= 0) & (c < Wp)
        img = img.scatter_add(0, torch.where(ok, r * Wp + c, torch.zeros_like(r)), torch.where(ok, w, torch.zeros_like(w)))
    return img.reshape(Hp, Wp)


def _reflect101(img, dim):
    n = img.shape[dim]
    idx = torch.cat([torch.tensor([1 if n > 1 else 0]), torch.arange(n), torch.tensor([n - 2 if n > 1 else 0])])
    return img.index_select(dim, idx)


def _blur3(img, sigma):
    e = float(np.exp(-0.5 * (1.0 / sigma) * (1.0 / sigma)))
    k0, k1 = e / (1.0 + 2.0 * e), 1.0 / (1.0 + 2.0 * e)
    p = _reflect101(img, 1)
    img = k0 * p[:, :-2] + k1 * p[:, 1:-1] + k0 * p[:, 2:]
    p = _reflect101(img, 0)
    return k0 * p[:-2] + k1 * p[1:-1] + k0 * p[2:]


def _variance(img, omit):
    return torch.var(img[1:-1, 1:-1] if omit else img)  # unbiased, like the reference's tensors


def _gradmag(img, omit):
    k = torch.stack([_SOBEL_ROW, _SOBEL_ROW.t()])[:, None]
    g = torch.nn.functional.conv2d(img[None, None], k, padding=1)[0] / 8.0  # Sobel of the whole image, zero padding
    if omit:
        g = g[:, 1:-1, 1:-1]
    return torch.mean(g[0] ** 2 + g[1] ** 2)


def objective(ev, m, model, size, cost="image_variance", sigma=0, outer_padding=0, omit_boundary=True, direction="minimize",
              warp_direction="first", normalize_t=True, t_range=None):
    """The loss as a torch scalar, differentiable (twice) in `m`.  ev [n, 4] and m are fp64 tensors.  t_range: the (t_min, t_max) of the
    whole batch when `ev` is a time slice of it."""
    size, pad = (int(size[0]), int(size[1])), _pad2(outer_padding)
    kind = _variance if cost.endswith("image_variance") else _gradmag
    if not (cost.endswith("image_variance") or cost.endswith("gradient_magnitude")):
        raise KeyError(cost)
    normalized, multi = "normalized" in cost, cost.startswith("multi_focal")

    def image(x, y):
        img = _vote(x, y, size, pad)
        return _blur3(img, sigma) if sigma > 0 else img

    def contrast(key_direction):
        x, y, _ = _warp(ev, m, model, size, key_direction, normalize_t, t_range)
        return kind(image(x, y), omit_boundary)

    if not normalized:
        v = contrast(warp_direction)
        return -v if direction == "minimize" else v
    # the un-warped image: the variance reads it un-cropped, the gradient magnitude crops both
    v2 = kind(image(ev[:, 0], ev[:, 1]), omit_boundary if kind is _gradmag else False)
    loss = 0.0
    for key_direction, mult in _REFS[3 if multi else 1]:
        v1 = contrast(warp_direction if key_direction is None else key_direction)
        loss = loss + mult * (v2 / v1 if direction == "minimize" else v1 / v2)
    return -loss if (multi and direction == "maximize") else loss


def value_grad_hvp(events, motion, model, size, v, **kw):
    """-> (loss, grad, Hv) in fp64 numpy: gradient by one backward pass, H v by a second one through it."""
    ev = torch.as_tensor(np.ascontiguousarray(events, dtype=np.float64))
    m = torch.as_tensor(np.ascontiguousarray(motion, dtype=np.float64)).clone().requires_grad_()
    vt = torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64)).reshape(m.shape)
    if ev.shape[0] == 0:
        return 0.0, np.zeros(m.shape), np.zeros(m.shape)
    loss = objective(ev, m, model, size, **kw)
    (g,) = torch.autograd.grad(loss, m, create_graph=True)
    if g.requires_grad:
        (hv,) = torch.autograd.grad((g * vt).sum(), m, allow_unused=True)
    else:
        hv = None
    hv = torch.zeros_like(m) if hv is None else hv
    return float(loss.detach()), g.detach().numpy().copy(), hv.detach().numpy().copy()


def _warped_numpy(events, motion, model, size, direction, normalize_t=True, t_range=None):
    with torch.no_grad():
        ev = torch.as_tensor(np.ascontiguousarray(events, dtype=np.float64))
        m = torch.as_tensor(np.ascontiguousarray(motion, dtype=np.float64))
        x, y, _ = _warp(ev, m, model, (int(size[0]), int(size[1])), direction, normalize_t, t_range)
    return x.numpy(), y.numpy()


def max_displacement(events, motion, model, size, directions, normalize_t=True, t_range=None):
    ev = np.asarray(events, dtype=np.float64)
    d = 0.0
    for direction in directions:
        x, y = _warped_numpy(ev, motion, model, size, direction, normalize_t, t_range)
        if len(x):
            d = max(d, float(np.abs(x - ev[:, 0]).max()), float(np.abs(y - ev[:, 1]).max()))
    return d


def border_margin(events, motion, model, size, directions, normalize_t=True, t_range=None):
    """_border.MARGIN is sized for displacements up to 40 px (the ulp of the fp32 product dt * flow grows with it)."""
    return MARGIN * max(1.0, max_displacement(events, motion, model, size, directions, normalize_t, t_range) / 40.0)


def drop_ambiguous(events, motion, model, size, directions, margin, normalize_t=True, t_range=None):
    """-> (events_kept, share_dropped).  Removes the events whose warped coordinate, at any reference time in `directions`, lies within
    `margin` of a cell border of floor(x' + 1e-6): across it the gradient has a kink, so the product is not defined there, and an fp32
    evaluation may legitimately pick the other cell (tests/_border.py).  Events that do not move at all are exempt: they are exact on
    both sides.  Computed from this reference alone.  Dropping the first or the last event moves every normalised time, so the filter
    is applied until it removes nothing."""
    ev = np.asarray(events, dtype=np.float64)
    n0 = ev.shape[0]
    for _ in range(16):
        bad = np.zeros(ev.shape[0], dtype=bool)
        for direction in directions:
            x, y = _warped_numpy(ev, motion, model, size, direction, normalize_t, t_range)
            moved = (x != ev[:, 0]) | (y != ev[:, 1])
            for c in (x, y):
                s = c + 1e-6
                f = s - np.floor(s)
                bad |= moved & (np.minimum(f, 1.0 - f) < margin)
        if not bad.any():
            break
        ev = ev[~bad]
    else:
        raise AssertionError("drop_ambiguous: the filter does not settle (a motion that puts the first or last event on a cell border?)")
    return ev, (n0 - ev.shape[0]) / max(n0, 1)
