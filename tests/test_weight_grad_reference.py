"""dL/dw of the fused objective, without a GPU: the fp64 reference the GPU tests use (tests/_weight_grad_ref.py) against central finite
differences of the weighted loss in the weights, over all six fused costs; and the C ABI entry is declared, exported and bound.

Step and tolerance of the finite differences come from the sweep the test prints (profiles/weight_grad_parity.txt keeps a copy): the
image is linear in w, so the plain costs are quadratic in w and the central difference has no truncation error -- only the rounding
eps * |L| / step; the normalised costs are ratios of quadratics (truncation ~ step^2).  Over steps 1e-2 .. 1e-7 the error relative
to max |dL/dw|, the worst of the 18 cases per step, is 4.9e-7, 5.0e-9, 1.6e-9, 3.5e-8, 3.0e-7, 4.3e-6: the floor lies at step 1e-4.  The
test uses step 1e-4 and asserts 1e-7 -- two orders above that floor and three below the GPU gate.  CMAX_WEIGHT_GRAD_SWEEP=1 prints the sweep."""
import os
import re

import numpy as np
import pytest

from _weight_grad_ref import weight_grad_objective
from _weighted_ref import weighted_objective

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = (24, 32)
COSTS = ["image_variance", "gradient_magnitude", "normalized_image_variance", "normalized_gradient_magnitude",
         "multi_focal_normalized_image_variance", "multi_focal_normalized_gradient_magnitude"]
FD_STEP, FD_TOL = 1e-4, 1e-7


def _case(model, seed=3):
    rng = np.random.default_rng(seed)
    n = 500
    ev = np.stack([rng.uniform(0, SIZE[0] - 1, n), rng.uniform(0, SIZE[1] - 1, n), np.sort(rng.uniform(0.0, 0.05, n)),
                   rng.integers(0, 2, n).astype(np.float64)], axis=1)
    w = rng.uniform(0.2, 3.0, n)
    w[::9] = 0.0  # weight-0 events have a derivative too
    if model == "2d-translation":
        motion = np.array([37.0, -52.0])
    elif model == "dense-flow":
        motion = rng.normal(0, 40, (2,) + SIZE)
    else:
        motion = rng.normal(0, 40, (2, 2) + SIZE)
    return ev, w, motion


def _fd(ev, w, motion, model, cost, sigma, idx, step):
    out = np.empty(len(idx))
    for j, i in enumerate(idx):
        wp, wm = w.copy(), w.copy()
        wp[i] += step
        wm[i] -= step
        lp = weighted_objective(ev, motion, model, SIZE, wp, cost=cost, sigma=sigma, want_grad=False)["loss"]
        lm = weighted_objective(ev, motion, model, SIZE, wm, cost=cost, sigma=sigma, want_grad=False)["loss"]
        out[j] = (lp - lm) / (2 * step)
    return out


@pytest.mark.parametrize("model", ["2d-translation", "dense-flow", "dense-flow-voxel"])
@pytest.mark.parametrize("cost", COSTS)
def test_reference_against_finite_differences(model, cost):
    ev, w, motion = _case(model)
    sigma = 1 if "gradient" in cost else 0
    ref = weight_grad_objective(ev, motion, model, SIZE, w, cost=cost, sigma=sigma)["grad_w"]
    idx = np.concatenate([np.arange(0, 90, 9), np.arange(1, 500, 50)])  # ten weight-0 events and ten others
    assert (w[idx[:10]] == 0).all() and np.abs(ref[idx[:10]]).max() > 0
    scale = np.abs(ref).max()
    sweep = os.environ.get("CMAX_WEIGHT_GRAD_SWEEP")
    for step in ((1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7) if sweep else ()):
        e = np.abs(_fd(ev, w, motion, model, cost, sigma, idx, step) - ref[idx]).max() / scale
        print(f"[weight grad] fd sweep {model} {cost} sigma {sigma}: step {step:g} rel err {e:.2e}")
    err = np.abs(_fd(ev, w, motion, model, cost, sigma, idx, FD_STEP) - ref[idx]).max() / scale
    print(f"[weight grad] fd {model} {cost} sigma {sigma}: step {FD_STEP:g} rel err {err:.2e}")
    assert err <= FD_TOL, (model, cost, err)


GOLDEN_TOL = 1e-9  # of the largest entry: the project's fp64-against-fixture figure (tests/test_hvp_reference.py)


@pytest.mark.parametrize("mname,model", [("2dof", "2d-translation"), ("dense", "dense-flow"), ("voxel", "dense-flow-voxel")])
@pytest.mark.parametrize("cost,sigma", [("image_variance", 0), ("gradient_magnitude", 1), ("normalized_image_variance", 0),
                                        ("multi_focal_normalized_gradient_magnitude", 1)])
def test_reference_against_the_reference_fixture(mname, model, cost, sigma):
    """tests/golden/weight_grad.npz: `weight.grad` of the reference itself (tests/golden/gen_golden_weight_grad.py)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "weight_grad.npz"))
    size = tuple(int(v) for v in g["image_size"])
    tag = f"{mname}__{cost}__s{sigma}"
    ref = weight_grad_objective(g["events"], g["motion_" + mname], model, size, g["weights"], cost=cost, sigma=sigma)
    want = g[tag + "__grad_w"]
    e_loss = abs(ref["loss"] - float(g[tag + "__loss"])) / abs(float(g[tag + "__loss"]))
    e_gw = np.abs(ref["grad_w"] - want).max() / np.abs(want).max()
    print(f"[weight grad] fixture {tag}: rel err loss {e_loss:.2e} grad_w {e_gw:.2e}")
    assert e_loss <= GOLDEN_TOL and e_gw <= GOLDEN_TOL, (tag, e_loss, e_gw)


def test_orig_term_matters_for_normalised_costs():
    ev, w, motion = _case("2d-translation")
    full = weight_grad_objective(ev, motion, "2d-translation", SIZE, w, cost="normalized_image_variance")["grad_w"]
    part = weight_grad_objective(ev, motion, "2d-translation", SIZE, w, cost="normalized_image_variance", with_orig=False)["grad_w"]
    assert np.abs(full - part).max() > 0.1 * np.abs(full).max()


def test_entry_is_declared_and_bound():
    from event_based_optical_flow_amd import _lib

    header = open(os.path.join(ROOT, "include", "cmax_hip.h")).read()
    assert re.search(r"\bint\s+cmax_objective_weight_grad\s*\(", header)
    assert "cmax_objective_weight_grad" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["cmax_objective_weight_grad"][1]) == 8
    assert hasattr(_lib.load(), "cmax_objective_weight_grad")
