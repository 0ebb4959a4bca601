"""TEST INFRASTRUCTURE ONLY: the fp64 value the time-aware flow kernels (csrc/cmax_flow.hip, csrc/cmax_flow_dual.h) are held to.

A torch-CPU restatement of one propagation step and of the voxel chain, written as whole-array tensor operations from the formulas
the kernels cite, so that autograd supplies every derivative -- first and second order -- with torch's own tie rules:
    signed step         s = sign(dt), tau = |dt|, f = s F, out = s f_new; dt == 0 is the identity
    differences         back: f[k] - f[k-1], forw: f[k+1] - f[k], both ZERO where the neighbour is outside the image
    upwind              f_new = f - tau (max(u,0) d_row_back f + min(u,0) d_row_forw f + max(v,0) d_col_back f + min(v,0) d_col_forw f)
    burgers             u_new = u - tau (max(v,0) d_col_back u + min(v,0) d_col_forw u + B(u along rows)), v likewise with rows <-> columns,
                        B(w) = (w^2 sign(w) - max(sign(w_back),0) w_back^2 - min(sign(w_forw),0) w_forw^2) / 2 on REPLICATE-padded neighbours
    ties                torch.maximum / minimum(x, 0) hand 1/2 of the gradient to x at x == 0; torch.sign has no gradient
    chain               V[t0] = F, steps of -1/T down to bin 0 and of +1/T up to bin T-1
(channel 0 = u moves along rows, channel 1 = v along columns.)  Anchored to the C oracle and to the golden fixtures of the reference
by tests/test_flow_reference.py."""
import torch

SCHEMES = ("burgers", "upwind")


def t0_index(T, t0):
    """Bin of the given flow: "first", "middle" (T // 2, as the operators place it) or the index itself."""
    if t0 == "first":
        return 0
    if t0 == "middle":
        return T // 2
    t0 = int(t0)
    assert 0 <= t0 < T
    return t0


def _zeros_line(x, dim):
    return torch.zeros_like(x.narrow(dim, 0, 1))


def _d_back(x, dim):  # x[k] - x[k-1]; 0 at k = 0
    return torch.cat([_zeros_line(x, dim), torch.diff(x, dim=dim)], dim=dim)


def _d_forw(x, dim):  # x[k+1] - x[k]; 0 at the last k
    return torch.cat([torch.diff(x, dim=dim), _zeros_line(x, dim)], dim=dim)


def _rep_back(x, dim):  # x[k-1], the first line repeated
    n = x.shape[dim]
    return torch.cat([x.narrow(dim, 0, 1), x.narrow(dim, 0, n - 1)], dim=dim)


def _rep_forw(x, dim):  # x[k+1], the last line repeated
    n = x.shape[dim]
    return torch.cat([x.narrow(dim, 1, n - 1), x.narrow(dim, n - 1, 1)], dim=dim)


def _pos(x):
    return torch.maximum(x, torch.zeros_like(x))


def _neg(x):
    return torch.minimum(x, torch.zeros_like(x))


def _burgers_term(w, dim):
    wb, wf = _rep_back(w, dim), _rep_forw(w, dim)
    return (w * w * torch.sign(w) + _pos(torch.sign(wb)) * (-(wb * wb)) - _neg(torch.sign(wf)) * (wf * wf)) / 2.0


def step(F, dt, scheme):
    """One explicit step of length dt (either sign) of a [2,H,W] flow."""
    assert scheme in SCHEMES and F.dim() == 3 and F.shape[0] == 2
    if dt == 0:
        return F.clone()
    s, tau = (1.0 if dt > 0 else -1.0), abs(float(dt))
    u, v = s * F[0], s * F[1]
    if scheme == "burgers":
        nu = u - tau * (_pos(v) * _d_back(u, 1) + _neg(v) * _d_forw(u, 1) + _burgers_term(u, 0))
        nv = v - tau * (_pos(u) * _d_back(v, 0) + _neg(u) * _d_forw(v, 0) + _burgers_term(v, 1))
    else:
        nu = u - tau * (_pos(u) * _d_back(u, 0) + _neg(u) * _d_forw(u, 0) + _pos(v) * _d_back(u, 1) + _neg(v) * _d_forw(u, 1))
        nv = v - tau * (_pos(u) * _d_back(v, 0) + _neg(u) * _d_forw(v, 0) + _pos(v) * _d_back(v, 1) + _neg(v) * _d_forw(v, 1))
    return torch.stack([nu * s, nv * s])


def voxel(F, T, scheme, t0="middle"):
    """[T,2,H,W]: F placed in bin t0 and propagated to both ends."""
    t0 = t0_index(T, t0)
    dt = 1.0 / T
    bins = [None] * T
    bins[t0] = F
    for i in range(t0, 0, -1):
        bins[i - 1] = step(bins[i], -dt, scheme)
    for i in range(t0, T - 1):
        bins[i + 1] = step(bins[i], dt, scheme)
    return torch.stack(bins)


def step_vjp(X, dt, scheme, g, create_graph=False):
    """J(X)^T g of `step` at X."""
    X = X if X.requires_grad else X.detach().requires_grad_()
    (out,) = torch.autograd.grad(step(X, dt, scheme), X, grad_outputs=g, create_graph=create_graph)
    return out


def _sweep(T, t0):
    """(input bin, bin of the upstream gradient, dt) of every step, in the order of the adjoint sweep: outermost first on each side."""
    dt = 1.0 / T
    return [(i, i + 1, dt) for i in range(T - 2, t0 - 1, -1)] + [(i, i - 1, -dt) for i in range(1, t0 + 1)]


def adj_at(V, gV, scheme, t0="middle"):
    """dL/dF of the chain, every step linearised AT THE GIVEN VOXEL: lambda = gV; lambda[i] += J(V[i])^T lambda[neighbour].
    The selectors (sign, max / min) are decided by the V passed in -- the kernels read the saved voxel the same way."""
    T = V.shape[0]
    t0 = t0_index(T, t0)
    lam = [g.clone() for g in gV.detach()]
    for i, nxt, dt in _sweep(T, t0):
        lam[i] = lam[i] + step_vjp(V[i].detach(), dt, scheme, lam[nxt])
    return lam[t0]


def tan(F, dF, T, scheme, t0="middle"):
    """(V, dV): the voxel and its directional derivative along dF."""
    V, dV = torch.autograd.functional.jvp(lambda f: voxel(f, T, scheme, t0), F.detach(), dF.detach())
    return V.detach(), dV.detach()


def adj_tan_at(V, dV, gV, dgV, scheme, t0="middle"):
    """(gF, dgF): `adj_at` and its directional derivative along (dV, dgV), bin by bin:
    dlambda[i] += J(V[i])^T dlambda[neighbour] + (d/dV[i] [J(V[i])^T lambda[neighbour]]) . dV[i]."""
    T = V.shape[0]
    t0 = t0_index(T, t0)
    lam = [g.clone() for g in gV.detach()]
    dlam = [g.clone() for g in dgV.detach()]
    for i, nxt, dt in _sweep(T, t0):
        h, dh = torch.autograd.functional.jvp(lambda x, g: step_vjp(x, dt, scheme, g, create_graph=True), (V[i].detach(), lam[nxt]),
                                              (dV[i].detach(), dlam[nxt]))
        lam[i] = lam[i] + h.detach()
        dlam[i] = dlam[i] + dh.detach()
    return lam[t0], dlam[t0]
