"""TEST INFRASTRUCTURE ONLY: the fp64 values the IWE layer (cmax_iwes, cmax_iwes_vjp, cmax_iwes_jvp, cmax_iwes_vjp_tan) is held to.

A torch-CPU restatement in fp64 that takes the warp, the blur and the padding rule of tests/_hvp_ref.py as they are (imported, not
copied) and adds the one thing that file lacks: a vote whose four bilinear shares are multiplied by a per-event weight w, which is on the
autograd tape like the motion.  Every derivative is autograd's:
    VJP      grad of <G, I(m, w)> in m and in w
    JVP      torch.autograd.functional.jvp of m -> I(m)
    vjp_tan  grad_m <grad_m <G, I>, u>  +  grad_m <G', I>      ( = d/d(eps) [ J(m + eps u)^T (G + eps G') ] at eps = 0 )
tests/test_iwe_reference.py anchors it to the committed oracle, to _hvp_ref.value_grad_hvp and to finite differences without a GPU."""
import numpy as np
import torch

from _hvp_ref import _blur3, _pad2, _warp


def vote_weighted(x, y, size, pad, w):
    """_hvp_ref._vote with the shares multiplied by w: cell floor(x' + 1e-6), fractions from the un-padded coordinate, corners masked by
    the PADDED image."""
    (H, W), (ph, pw) = size, pad
    Hp, Wp = H + 2 * ph, W + 2 * pw
    fx, fy = torch.floor(x + 1e-6), torch.floor(y + 1e-6)
    a, b = x - fx, y - fy
    r0, c0 = fx.long() + ph, fy.long() + pw
    img = torch.zeros(Hp * Wp, dtype=x.dtype)
    for dr, dc, share in ((0, 0, (1 - a) * (1 - b)), (1, 0, a * (1 - b)), (0, 1, (1 - a) * b), (1, 1, a * b)):
        r, c = r0 + dr, c0 + dc
        ok = (r >= 0) & (r < Hp) & (c >= 0) & (c < Wp)
        img = img.scatter_add(0, torch.where(ok, r * Wp + c, torch.zeros_like(r)), torch.where(ok, share * w, torch.zeros_like(share)))
    return img.reshape(Hp, Wp)


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64))


def images_t(ev, m, w, model, size, directions, sigma=0, outer_padding=0, normalize_t=True, t_range=None, with_orig=False):
    """[K, Hp, Wp] as a torch tensor, differentiable (twice) in m and (once is all anybody asks) in w.  ev, m, w: fp64 tensors."""
    size, pad = (int(size[0]), int(size[1])), _pad2(outer_padding)

    def image(x, y):
        img = vote_weighted(x, y, size, pad, w)
        return _blur3(img, sigma) if sigma > 0 else img

    out = []
    for direction in directions:
        x, y, _ = _warp(ev, m, model, size, direction, normalize_t, t_range)
        out.append(image(x, y))
    if with_orig:
        out.append(image(ev[:, 0], ev[:, 1]))
    return torch.stack(out)


class Layer:
    """One batch, one motion, one set of weights: images, VJP, JVP and vjp_tan in fp64 numpy."""

    def __init__(self, events, motion, model, size, directions=("first",), weights=None, **kw):
        self.ev = _t(events)
        self.m0 = _t(motion)
        self.w0 = torch.ones(self.ev.shape[0], dtype=torch.float64) if weights is None else _t(weights)
        self.model, self.size, self.directions, self.kw = model, size, tuple(directions), kw
        self.n_ref = len(self.directions)

    def _images(self, m, w):
        return images_t(self.ev, m, w, self.model, self.size, self.directions, **self.kw)

    def images(self):
        with torch.no_grad():
            return self._images(self.m0, self.w0).numpy()

    def vjp(self, G):
        """-> (grad_motion, grad_w): gradient of <G, I(m, w)>; G the shape of images()."""
        m, w = self.m0.clone().requires_grad_(), self.w0.clone().requires_grad_()
        s = (self._images(m, w) * _t(G)).sum()
        gm, gw = torch.autograd.grad(s, (m, w), allow_unused=True)
        gm = torch.zeros_like(m) if gm is None else gm
        gw = torch.zeros_like(w) if gw is None else gw
        return gm.numpy().copy(), gw.numpy().copy()

    def jvp(self, u):
        """-> J u, [n_ref, Hp, Wp] (the un-warped image has no tangent)."""
        kw = dict(self.kw)
        kw["with_orig"] = False
        f = lambda m: images_t(self.ev, m, self.w0, self.model, self.size, self.directions, **kw)  # noqa: E731
        _, t = torch.autograd.functional.jvp(f, self.m0, _t(u).reshape(self.m0.shape))
        return t.numpy().copy()

    def vjp_tan(self, u, G, Gp=None):
        """-> d/d(eps) [ J(m + eps u)^T (G + eps G') ] at eps = 0 (G' = None: 0, the mixed term alone)."""
        m = self.m0.clone().requires_grad_()
        I = self._images(m, self.w0)
        (g,) = torch.autograd.grad((I * _t(G)).sum(), m, create_graph=True)
        out = torch.zeros_like(m)
        if g.requires_grad:
            (mixed,) = torch.autograd.grad((g * _t(u).reshape(m.shape)).sum(), m, allow_unused=True, retain_graph=Gp is not None)
            if mixed is not None:
                out = out + mixed
        if Gp is not None:
            (lin,) = torch.autograd.grad((I * _t(Gp)).sum(), m, allow_unused=True)
            if lin is not None:
                out = out + lin
        return out.detach().numpy().copy()


def torch_cost(cost, omit_boundary=True, direction="minimize"):
    """The built-in costs re-expressed in torch on the reference's arg dict (images [Hp, Wp] of any float dtype, upcast to fp64 first):
    what a user of fused_iwes / ContrastObjective(cost=callable) would write.  required_keys follow the package's cost table."""
    gradmag = cost.endswith("gradient_magnitude")
    normalized, multi = "normalized" in cost, cost.startswith("multi_focal")

    def value(img, omit):
        img = img.double()
        if gradmag:  # Sobel / 8 of the whole image with zero padding, then the crop (_hvp_ref._gradmag, on the image's device)
            k = torch.stack([torch.tensor([[-1.0, -2.0, -1.0], [0.0, 0.0, 0.0], [1.0, 2.0, 1.0]], dtype=torch.float64, device=img.device)] * 2)
            k[1] = k[0].t()
            g = torch.nn.functional.conv2d(img[None, None], k[:, None], padding=1)[0] / 8.0
            if omit:
                g = g[:, 1:-1, 1:-1]
            return torch.mean(g[0] ** 2 + g[1] ** 2)
        return torch.var(img[1:-1, 1:-1] if omit else img)

    def f(arg):
        omit = arg.get("omit_boundary", omit_boundary)
        if not normalized:
            v = value(arg["iwe"], omit)
            return -v if direction == "minimize" else v
        v2 = value(arg["orig_iwe"], omit if gradmag else False)  # the variance reads the un-warped image un-cropped
        refs = (("forward_iwe", 1.0), ("backward_iwe", 1.0), ("middle_iwe", 2.0)) if multi else (("iwe", 1.0),)
        loss = 0.0
        for key, mult in refs:
            v1 = value(arg[key], omit)
            loss = loss + mult * (v2 / v1 if direction == "minimize" else v1 / v2)
        return -loss if (multi and direction == "maximize") else loss

    f.required_keys = (["forward_iwe", "backward_iwe", "middle_iwe", "orig_iwe", "omit_boundary"] if multi
                       else ["iwe", "orig_iwe", "omit_boundary"] if normalized else ["iwe", "omit_boundary"])
    return f


def charbonnier_mean(img, eps=1e-3):
    """A cost the package has no kernel for: mean over the whole image of sqrt(I^2 + eps^2) (robust, smooth at 0), fp64."""
    img = img.double()
    return torch.sqrt(img * img + eps * eps).mean()


def weight_set_100(events, seed=0):
    """The edge of the documented supported range min|w != 0| / wmax >= 0.01: weights log-uniform in [0.01, 1], both ends present."""
    rng = np.random.default_rng(seed)
    n = events.shape[0]
    w = 10.0 ** rng.uniform(-2.0, 0.0, n)
    if n >= 2:
        w[0], w[n // 2] = 1.0, 0.01
    return w
