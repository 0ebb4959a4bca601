"""TEST INFRASTRUCTURE ONLY: the fp64 value the flow regularisers (csrc/cmax_flowreg_kernels.h; cmax_flow_regularizer[_tan] and the
plan term of csrc/cmax_solver.hip) are held to.

The reference has no counterpart, so this is a torch-CPU restatement of the formulas of include/cmax_hip.h, written so that autograd
supplies every derivative:
    F [2,H,W], F[0] along rows, F[1] along columns; Omega the interior, n = (H-2)(W-2); central differences on Omega
        a = dF0/dr, b = dF0/dc, c = dF1/dr, d = dF1/dc
    psi(u) = sqrt(u^2 + eps^2) - eps with psi' and psi'' as the definition states them (autograd's own second derivative cancels six digits
        at eps = 1e-3); eps = 0: |u| (torch.abs: derivative 0 at 0, second derivative 0)
    divergence  R = mean_Omega psi(a + d)
    area        R = mean_Omega [psi(A(+s) - 1) + psi(A(-s) - 1)] / 2,  A(sigma) = 1 - sigma (a + d) + sigma^2 (a d - b c)
Anchored by tests/test_flowreg_reference.py: a tabulated linear field F = M (x - x0) has a + d = tr M and A(sigma) = det(I - sigma M)
at every pixel of Omega, and central finite differences of the value and of the gradient."""
import numpy as np
import torch

KINDS = ("divergence", "area")


def derivatives(F):
    """F [2,H,W] tensor -> (a, b, c, d), each [H-2, W-2]."""
    a = 0.5 * (F[0, 2:, 1:-1] - F[0, :-2, 1:-1])
    b = 0.5 * (F[0, 1:-1, 2:] - F[0, 1:-1, :-2])
    c = 0.5 * (F[1, 2:, 1:-1] - F[1, :-2, 1:-1])
    d = 0.5 * (F[1, 1:-1, 2:] - F[1, 1:-1, :-2])
    return a, b, c, d


class _PsiPrime(torch.autograd.Function):
    """psi' = u / sqrt(u^2 + eps^2) with psi'' = eps^2 / (u^2 + eps^2)^(3/2) as the definition states it.  Autograd's own derivative of
    u / sqrt(.) is 1 / sqrt(.) - u^2 / (.)^(3/2): two terms of size 1 whose difference is eps^2 -- at eps = 1e-3 it keeps six digits, less
    than the gate asks of the device."""

    @staticmethod
    def forward(ctx, u, eps):
        den = torch.sqrt(u * u + eps * eps)
        ctx.save_for_backward(den)
        ctx.eps = eps
        return u / den

    @staticmethod
    def backward(ctx, g):
        (den,) = ctx.saved_tensors
        return g * (ctx.eps * ctx.eps) / (den * den * den), None


class _Psi(torch.autograd.Function):
    """psi = sqrt(u^2 + eps^2) - eps, taken as u^2 / (sqrt(u^2 + eps^2) + eps) (no cancellation where |u| << eps), eps > 0."""

    @staticmethod
    def forward(ctx, u, eps):
        ctx.save_for_backward(u)
        ctx.eps = eps
        return u * u / (torch.sqrt(u * u + eps * eps) + eps)

    @staticmethod
    def backward(ctx, g):
        (u,) = ctx.saved_tensors
        return g * _PsiPrime.apply(u, ctx.eps), None


def psi(u, eps):
    if eps == 0.0:
        return torch.abs(u)
    return _Psi.apply(u, float(eps))


def arguments(F, kind, s=1.0):
    """The arguments u of psi at every pixel of Omega: [1 or 2, H-2, W-2]."""
    a, b, c, d = derivatives(F)
    if kind == "divergence":
        return (a + d)[None]
    assert kind == "area", kind
    tr, det = a + d, a * d - b * c
    return torch.stack([-sg * tr + sg * sg * det for sg in (s, -s)])  # A(sigma) - 1


def value(F, kind, eps=0.0, s=1.0):
    """F [2,H,W] fp64 tensor -> scalar tensor."""
    assert F.dim() == 3 and F.shape[0] == 2 and F.shape[1] >= 3 and F.shape[2] >= 3
    u = arguments(F, kind, s)
    return psi(u, eps).sum(dim=0).mean() / u.shape[0]


def _t(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64))


def value_grad(F, kind, eps=0.0, s=1.0):
    """-> (R, dR/dF [2,H,W]) in fp64 numpy."""
    Ft = _t(F).clone().requires_grad_()
    val = value(Ft, kind, eps, s)
    (g,) = torch.autograd.grad(val, Ft)
    return float(val.detach()), g.numpy().copy()


def product(F, dF, kind, eps=0.0, s=1.0):
    """(grad^2 R)[dF] in fp64 numpy: a second backward pass through the first (zero where the gradient is piecewise constant)."""
    Ft = _t(F).clone().requires_grad_()
    (g,) = torch.autograd.grad(value(Ft, kind, eps, s), Ft, create_graph=True)
    if not g.requires_grad:
        return np.zeros(tuple(Ft.shape))
    (h,) = torch.autograd.grad((g * _t(dF)).sum(), Ft, allow_unused=True)
    return np.zeros(tuple(Ft.shape)) if h is None else h.numpy().copy()


def extended(F, dF, kind, eps=0.0, s=1.0):
    """(R, dR/dF, (grad^2 R)[dF]) from the same formulas in numpy's long double (64-bit mantissa on x86), derivatives written out by
    hand: what the fp64 autograd reference above is itself measured against (its sums over the two signs of sigma cancel up to seven
    digits where eps << |u|).  -> long double arrays."""
    L = np.longdouble
    F, dF, eps = np.asarray(F, dtype=L), np.asarray(dF, dtype=L), L(eps)
    half = L(0.5)

    def diffs(G):
        return (half * (G[0, 2:, 1:-1] - G[0, :-2, 1:-1]), half * (G[0, 1:-1, 2:] - G[0, 1:-1, :-2]),
                half * (G[1, 2:, 1:-1] - G[1, :-2, 1:-1]), half * (G[1, 1:-1, 2:] - G[1, 1:-1, :-2]))

    def psi_all(u):
        if eps == 0:
            return np.abs(u), np.sign(u), np.zeros_like(u)
        den = np.sqrt(u * u + eps * eps)
        return u * u / (den + eps), u / den, eps * eps / (den * den * den)

    (a, b, c, d), (da, db, dc, dd) = diffs(F), diffs(dF)
    e, p, dp = np.zeros_like(a), [np.zeros_like(a) for _ in range(4)], [np.zeros_like(a) for _ in range(4)]
    if kind == "divergence":
        v, d1, d2 = psi_all(a + d)
        e, p[0], p[3], dp[0], dp[3] = v, d1, d1, d2 * (da + dd), d2 * (da + dd)
        scale = L(1)
    else:
        for sg in (L(s), -L(s)):
            s2 = sg * sg
            v, d1, d2 = psi_all(-sg * (a + d) + s2 * (a * d - b * c))
            ua, ub, uc, ud = -sg + s2 * d, -s2 * c, -s2 * b, -sg + s2 * a
            du = d2 * (ua * da + ub * db + uc * dc + ud * dd)
            e = e + v
            for k, (uk, hk) in enumerate(((ua, s2 * dd), (ub, -s2 * dc), (uc, -s2 * db), (ud, s2 * da))):
                p[k] = p[k] + d1 * uk
                dp[k] = dp[k] + du * uk + d1 * hk
        scale = half
    scale = scale / L(a.size)

    def transpose(q):
        g = np.zeros(F.shape, dtype=L)
        g[0, 2:, 1:-1] += half * q[0]
        g[0, :-2, 1:-1] -= half * q[0]
        g[0, 1:-1, 2:] += half * q[1]
        g[0, 1:-1, :-2] -= half * q[1]
        g[1, 2:, 1:-1] += half * q[2]
        g[1, :-2, 1:-1] -= half * q[2]
        g[1, 1:-1, 2:] += half * q[3]
        g[1, 1:-1, :-2] -= half * q[3]
        return g * scale

    return e.sum() * scale, transpose(p), transpose(dp)


def own_error(F, dF, kind, eps=0.0, s=1.0):
    """The autograd reference's distance from `extended`, as the tests measure a field: (value, gradient, product), each relative to its
    largest entry; None without an extended precision (long double = double)."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        return None
    v, g, hv = extended(F, dF, kind, eps, s)
    v64, g64 = value_grad(F, kind, eps, s)
    hv64 = product(F, dF, kind, eps, s)

    def rel(x, ref):
        m = np.abs(ref).max()
        return float(np.abs(x - ref).max() / m) if m > 0 else float(np.abs(x).max())

    return rel(np.asarray(v64), np.asarray(v)), rel(g64, g), rel(hv64, hv)


def min_abs_argument(F, kind, s=1.0):
    """min over Omega (and both signs of sigma) of |u|: below ~1e-6 an eps = 0 case would test the sign of rounding noise."""
    with torch.no_grad():
        return float(arguments(_t(F), kind, s).abs().min())


def linear_field(M, x0, size):
    """F = M (x - x0) tabulated on the sensor: F[k](r, c) = M[k][0] (r - x0[0]) + M[k][1] (c - x0[1])."""
    H, W = size
    r, c = np.meshgrid(np.arange(H, dtype=np.float64) - x0[0], np.arange(W, dtype=np.float64) - x0[1], indexing="ij")
    M = np.asarray(M, dtype=np.float64)
    return np.stack([M[0, 0] * r + M[0, 1] * c, M[1, 0] * r + M[1, 1] * c])


def closed_form(M, kind, eps=0.0, s=1.0):
    """R of a linear field: the same argument at every pixel."""
    M = np.asarray(M, dtype=np.float64)

    def p(u):
        return abs(u) if eps == 0.0 else float(np.sqrt(u * u + eps * eps) - eps)

    if kind == "divergence":
        return p(np.trace(M))
    return 0.5 * (p(np.linalg.det(np.eye(2) - s * M) - 1.0) + p(np.linalg.det(np.eye(2) + s * M) - 1.0))


# ---- the plan term: weight * R(t_scale * map x) and its derivatives with respect to x, by autograd through the map ----------------------
def plan_term(x, dense_of, reg, t_scale, v=None):
    """dense_of: differentiable map x [nx] tensor -> D [2,H,W] (tests/_mixed_ref.patch_to_dense, a basis sum).  reg: dict(kind, weight, eps,
    s).  -> (weight R, its gradient [nx], its product with v or None) in fp64 numpy."""
    xt = _t(x).reshape(-1).clone().requires_grad_()
    val = reg["weight"] * value(dense_of(xt) * t_scale, reg["kind"], reg.get("eps", 0.0), reg.get("s", 1.0))
    (g,) = torch.autograd.grad(val, xt, create_graph=v is not None)
    hv = None
    if v is not None:
        hv = np.zeros(xt.numel())
        if g.requires_grad:
            (h,) = torch.autograd.grad((g * _t(v).reshape(-1)).sum(), xt, allow_unused=True)
            hv = hv if h is None else h.numpy().copy()
    return float(val.detach()), g.detach().numpy().copy(), hv
