"""TEST INFRASTRUCTURE ONLY: inputs and the fp64 yardstick of the multi-start descent (cmax_objective_descend_batch), shared by
tests/test_descent_batch_reference.py (no GPU: the start table is fit for its Adam gate) and tests/test_gpu_descent_batch.py.

The events are the recipe of tests/test_gpu_descent.py::two_dof_events, restated (a test module is not imported): 1500 generate_events
seed 7 plus 2500 generate_structured_events velocity (4, -3), 12 dots, seed 8, on 40 x 56, clipped, stably sorted by time."""
import numpy as np
import torch

import event_based_optical_flow_amd as E

import _descent_ref
import _hvp_ref

SIZE = (40, 56)
N_ITER, LR, LR_STEP, LR_DECAY, MOMENTUM = 6, 0.05, 2, 0.5, 0.9  # three learning rates occur
SCHEDULE = dict(n_iter=N_ITER, lr=LR, lr_step=LR_STEP, lr_decay=LR_DECAY)
METHODS = {"sgd": dict(method="SGD", momentum=MOMENTUM), "adam": dict(method="Adam")}
GRAD_TOL = 1e-4  # the project's gradient gate (tests/test_gpu_descent.py)

# Adam's step bound needs the entries of every reference gradient within a factor 4 of each other (tests/test_gpu_descent.py): these
# nine starts keep max|g| / min|g| at 1.14 .. 2.77 along their fp64 trajectories (asserted <= 3 without a GPU)
ADAM_STARTS = np.array([(1.0, -1.0), (0.5, 0.5), (-2.0, -2.0), (6.0, -4.0), (-3.0, 1.5), (5.0, -2.0), (2.0, 2.0), (-3.0, -3.0), (7.0, -5.0)])
# rejected for Adam (their ratio exceeds 4 somewhere); SGD's bound needs no such condition
SGD_EXTRA_STARTS = np.array([(2.5, -1.5), (-1.0, 2.0), (3.0, 1.0), (4.0, -2.0), (1.5, 1.5), (1.0, -3.0), (-0.5, -1.5)])

_EVENTS = []
_REF = {}


def events():
    if not _EVENTS:
        H, W = SIZE
        a = E.utils.generate_events(1500, H, W, 0.0, 0.05, seed=7)
        b = E.utils.generate_structured_events(2500, H, W, (4.0, -3.0), n_dots=12, tmin=0.0, tmax=0.05, seed=8)
        ev = np.concatenate([a, b])
        ev[:, 0], ev[:, 1] = np.clip(ev[:, 0], 0, H - 1), np.clip(ev[:, 1], 0, W - 1)
        _EVENTS.append(np.ascontiguousarray(ev[np.argsort(ev[:, 2], kind="stable")]))
    return _EVENTS[0]


def sgd_starts(K):
    """K = 64: the 8 x 8 grid in [-3.5, 3.5]^2; smaller K: the first K of the Adam table followed by the starts rejected for it."""
    if K == 64:
        g = np.linspace(-3.5, 3.5, 8)
        return np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    table = np.concatenate([ADAM_STARTS, SGD_EXTRA_STARTS])
    assert K <= len(table)
    return table[:K].copy()


def ref_options(mid):
    kw = METHODS[mid]
    return _descent_ref.options(kw["method"], lr=LR, lr_step=LR_STEP, lr_decay=LR_DECAY, momentum=kw.get("momentum", 0.0))


def reference(theta, cost="image_variance", sigma=0):
    """fp64 (loss, gradient) at theta: tests/_hvp_ref.objective + autograd.  Computed once per (theta, cost, sigma) and shared."""
    theta = np.asarray(theta, dtype=np.float64)
    key = (theta.tobytes(), cost, sigma)
    if key not in _REF:
        m = torch.tensor(theta, requires_grad=True)
        loss = _hvp_ref.objective(torch.as_tensor(events()), m, "2d-translation", SIZE, cost=cost, sigma=sigma)
        (g,) = torch.autograd.grad(loss, m)
        _REF[key] = (float(loss.detach()), g.numpy().copy())
    loss, g = _REF[key]
    return loss, g.copy()


def ref_trajectory(theta0, mid, n_iter=N_ITER):
    """The fp64 trajectory from theta0: -> (iterates [n_iter + 1, 2], losses [n_iter], gradients [n_iter, 2])."""
    opt, state, x = ref_options(mid), {}, np.asarray(theta0, dtype=np.float64).copy()
    xs, losses, grads = [x.copy()], [], []
    for it in range(n_iter):
        loss, g = reference(x)
        x = _descent_ref.step(state, x, g, it, opt)
        xs.append(x.copy())
        losses.append(loss)
        grads.append(g)
    return np.stack(xs), np.array(losses), np.stack(grads)
