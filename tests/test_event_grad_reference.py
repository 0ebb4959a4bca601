"""dL/d(event) of the fused objective, without a GPU: the two fp64 references the GPU tests use (tests/_event_grad_ref.py) against each other
and against central finite differences of orc.objective, the Python composition of `events.grad` (cmax.compose_events_grad) against
autograd with reference-made inputs, and the C ABI entry declared, exported and bound.

Finite differences.  Step h in x and y (pixels); in t a step that moves the warped coordinates by about h pixels as well,
h_t = h * period / max |motion| (an event's own time moves its own warp; the first and the last event move everybody's through t.min() /
t.max()).  A central quotient of a loss evaluated in fp64 is off by the rounding of the two losses over the step, <= 64 eps |L| / h_step
(64: the loss is a ratio of sums of a few thousand terms, each rounded), plus the truncation h^2 |L'''| / 6: inside a cell the image is
bilinear in the coordinates, the contrasts quadratic in the image and the normalised costs ratios of them, so third derivatives are of
the order of the first per pixel^2 -- the test budgets 10 h^2 relative to the largest entry.  With h = 1e-5 that is 1e-9 + rounding.
The events are seeded; no warped coordinate comes within 1e-3 of a cell border (asserted), so no step crosses a kink."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import oracle as orc

import _hvp_ref
from _event_grad_ref import event_grad_objective, events_grad_autograd, reference_fractions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = (24, 32)
COSTS = ["image_variance", "gradient_magnitude", "normalized_image_variance", "normalized_gradient_magnitude",
         "multi_focal_normalized_image_variance", "multi_focal_normalized_gradient_magnitude"]
MODELS = ["2d-translation", "dense-flow", "dense-flow-voxel"]
AGREE_TOL = 1e-10  # the figure _hvp_ref.objective is anchored on the oracle with
FD_H = 1e-5
EPS = 2.0 ** -52


def _case(model, seed=5, n=300):
    rng = np.random.default_rng(seed)
    ev = np.stack([rng.uniform(0, SIZE[0] - 1, n), rng.uniform(0, SIZE[1] - 1, n), np.sort(rng.uniform(0.0, 0.05, n)),
                   rng.integers(0, 2, n).astype(np.float64)], axis=1)
    if model == "2d-translation":
        motion = np.array([7.0, -9.0])
    elif model == "dense-flow":
        motion = rng.normal(0, 6, (2,) + SIZE)
    else:
        motion = rng.normal(0, 6, (2, 2) + SIZE)
    return ev, motion


def _compose(ref, ev, cost, normalize_t=True, warp_direction="first"):
    from event_based_optical_flow_amd.cmax import compose_events_grad

    out = compose_events_grad(torch.as_tensor(ref["grad_events"]), torch.as_tensor(ref["csum"]), torch.as_tensor(ev[:, 2]),
                              reference_fractions(cost, warp_direction), normalize_t)
    return out.numpy()


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("cost", COSTS)
def test_references_agree_and_composition_matches_autograd(model, cost):
    """event_grad_objective (oracle-composed, w = 1) -> compose_events_grad == autograd's events.grad, per column."""
    ev, motion = _case(model)
    sigma = 1 if "gradient" in cost else 0
    loss, want = events_grad_autograd(ev, motion, model, SIZE, cost=cost, sigma=sigma)
    ref = event_grad_objective(ev, motion, model, SIZE, 1.0, cost=cost, sigma=sigma)
    got = _compose(ref, ev, cost)
    assert abs(ref["loss"] - loss) <= AGREE_TOL * abs(loss)
    assert np.all(got[:, 3] == 0) and np.all(want[:, 3] == 0)
    for c in range(3):
        e = _rel(got[:, c], want[:, c])
        print(f"[event grad] references {model} {cost} sigma {sigma} column {c}: rel err {e:.2e}")
        assert e <= AGREE_TOL, (model, cost, c, e)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("warp_direction", ["first", "middle", "last"])
def test_composition_without_normalize_t(model, warp_direction):
    """normalize_t = False: the routed terms come from csum[k] -- the multi-focal cost has three reference times."""
    ev, motion = _case(model)
    motion = motion * 20.0  # pixels per second over a 0.05 s batch
    # (the multi-focal cost has its own three reference times, whatever warp_direction says: it runs with the default)
    for cost, wd in (("multi_focal_normalized_image_variance", "first"), ("image_variance", warp_direction)):
        kw = dict(cost=cost, sigma=0, normalize_t=False, warp_direction=wd)
        _, want = events_grad_autograd(ev, motion, model, SIZE, **kw)
        got = _compose(event_grad_objective(ev, motion, model, SIZE, 1.0, **kw), ev, cost, False, wd)
        for c in range(3):
            e = _rel(got[:, c], want[:, c])
            print(f"[event grad] raw time {model} {cost} {wd} column {c}: rel err {e:.2e}")
            assert e <= AGREE_TOL, (model, cost, c, e)


def test_ties_at_the_extremes_share_evenly():
    ev, motion = _case("2d-translation")
    ev[1, 2] = ev[0, 2]
    ev[-3:, 2] = ev[-1, 2]
    _, want = events_grad_autograd(ev, motion, "2d-translation", SIZE, cost="image_variance")
    got = _compose(event_grad_objective(ev, motion, "2d-translation", SIZE, 1.0, cost="image_variance"), ev, "image_variance")
    assert _rel(got[:, 2], want[:, 2]) <= AGREE_TOL


def test_a_fixed_time_range_routes_nothing():
    from event_based_optical_flow_amd.cmax import compose_events_grad

    ev, motion = _case("2d-translation")
    ref = event_grad_objective(ev, motion, "2d-translation", SIZE, 1.0, cost="image_variance")
    t_range = (float(ev[:, 2].min()), float(ev[:, 2].max()))
    got = compose_events_grad(torch.as_tensor(ref["grad_events"]), torch.as_tensor(ref["csum"]), torch.as_tensor(ev[:, 2]), [0.0], True, t_range).numpy()
    assert np.allclose(got[:, 2], ref["grad_events"][:, 2] / (t_range[1] - t_range[0]), rtol=1e-14, atol=0)


def _fd(ev, motion, model, cost, sigma, i, c, step):
    lo, hi = ev.copy(), ev.copy()
    hi[i, c] += step
    lo[i, c] -= step
    lp = orc.objective(hi, motion, model, SIZE, cost=cost, sigma=sigma, want_grad=False)["loss"]
    lm = orc.objective(lo, motion, model, SIZE, cost=cost, sigma=sigma, want_grad=False)["loss"]
    return (lp - lm) / (2 * step)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("cost", COSTS)
def test_references_against_finite_differences(model, cost):
    ev, motion = _case(model)
    sigma = 1 if "gradient" in cost else 0
    directions = _hvp_ref.cost_directions(cost)
    frac = ev[:, :2] + 1e-6 - np.floor(ev[:, :2] + 1e-6)  # the un-warped positions (orig_iwe) keep 1e-3 from a cell border as well
    ev = ev[(np.minimum(frac, 1 - frac) > 1e-3).all(axis=1)]
    ev, _ = _hvp_ref.drop_ambiguous(ev, motion, model, SIZE, directions, 1e-3)
    for c in (0, 1):  # the un-warped positions too (orig_iwe)
        f = ev[:, c] + 1e-6 - np.floor(ev[:, c] + 1e-6)
        assert np.minimum(f, 1 - f).min() > 10 * FD_H
    n = ev.shape[0]
    loss, want = events_grad_autograd(ev, motion, model, SIZE, cost=cost, sigma=sigma)
    period = ev[:, 2].max() - ev[:, 2].min()
    h_t = FD_H * period / np.abs(motion).max()
    idx = [0, n - 1, 1, n // 3, n // 2, n - 2]  # first and last: the min / max routing
    for c, step in ((0, FD_H), (1, FD_H), (2, h_t)):
        scale = np.abs(want[:, c]).max()
        tol = 64 * EPS * abs(loss) / step / scale + 10 * FD_H ** 2
        fd = np.array([_fd(ev, motion, model, cost, sigma, i, c, step) for i in idx])
        e = np.abs(fd - want[idx, c]).max() / scale
        print(f"[event grad] fd {model} {cost} sigma {sigma} column {c}: step {step:.2e} rel err {e:.2e} (tolerance {tol:.2e})")
        assert e <= tol, (model, cost, c, e, tol)


def test_entry_is_declared_and_bound():
    from event_based_optical_flow_amd import _lib

    header = open(os.path.join(ROOT, "include", "cmax_hip.h")).read()
    assert re.search(r"\bint\s+cmax_objective_event_grad\s*\(", header)
    assert "cmax_objective_event_grad" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["cmax_objective_event_grad"][1]) == 9
    assert hasattr(_lib.load(), "cmax_objective_event_grad")
