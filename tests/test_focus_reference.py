"""The focus losses without a GPU: the fp64 reference of tests/_focus_ref.py against direct loops over the definitions of
include/cmax_hip.h, its gradients against central differences, the two cost registries, the constants of header and _lib, and the
share of events the GPU cases drop (tests/_focus_cases.py)."""
import os
import re

import numpy as np
import pytest
import torch

from event_based_optical_flow_amd import _lib, cmax, costs

import _focus_cases as C
import _focus_ref as R
import _hvp_ref as HR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINE = {p + k for k in R.KINDS for p in ("", "normalized_", "multi_focal_normalized_")}


@pytest.mark.parametrize("shape,omit", [((5, 7), False), ((5, 7), True), ((3, 3), False), ((3, 3), True)])
@pytest.mark.parametrize("kind", R.KINDS)
def test_kinds_against_direct_loops(kind, shape, omit):
    img = np.random.default_rng(3).normal(0.0, 2.0, shape)
    got = float(R.focus_value(torch.as_tensor(img), kind, omit))
    want = R.numpy_loops(img, kind, omit)
    assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (got, want)


@pytest.mark.parametrize("omit", [False, True])
@pytest.mark.parametrize("kind", R.KINDS)
def test_kind_gradients_against_central_differences(kind, omit):
    img = np.random.default_rng(4).normal(0.0, 2.0, (5, 7))
    t = torch.as_tensor(img).clone().requires_grad_()
    (g,) = torch.autograd.grad(R.focus_value(t, kind, omit), t)
    fd, eps = np.zeros_like(img), 1e-5
    for idx in np.ndindex(*img.shape):
        hi, lo = img.copy(), img.copy()
        hi[idx] += eps
        lo[idx] -= eps
        fd[idx] = (R.numpy_loops(hi, kind, omit) - R.numpy_loops(lo, kind, omit)) / (2 * eps)
    # the forms are quadratic: the central difference is exact up to rounding, ~1e-16 |v| / eps
    assert np.abs(g.numpy() - fd).max() <= 1e-8 * max(1.0, np.abs(fd).max())


def test_weighted_vote_with_unit_weights_is_the_plain_vote():
    rng = np.random.default_rng(5)
    x, y = torch.as_tensor(rng.uniform(-1.0, 9.0, 200)), torch.as_tensor(rng.uniform(-1.0, 12.0, 200))
    a = HR._vote(x, y, (8, 11), (1, 1))
    b = R._vote_weighted(x, y, (8, 11), (1, 1), torch.ones(200, dtype=torch.float64))
    assert torch.equal(a, b)


def test_registries():
    assert set(costs.focus_functions) == NINE and len(costs.focus_functions) == 9
    assert len(costs.functions) == 7 and not (set(costs.functions) & NINE)
    assert set(cmax.FOCUS_COSTS) == NINE and not (set(cmax.FUSED_COSTS) & NINE)
    for name, cls in costs.focus_functions.items():
        assert cls.name == name and issubclass(cls, costs.CostBase)
    h = costs.HybridCost("minimize", {"laplacian_magnitude": 1.0, "image_variance": 0.5, "multi_focal_normalized_hessian_magnitude": "inv"})
    assert isinstance(h.cost_func["laplacian_magnitude"]["func"], costs.focus_functions["laplacian_magnitude"])
    assert isinstance(h.cost_func["image_variance"]["func"], costs.functions["image_variance"])
    assert "orig_iwe" in h.required_keys and "middle_iwe" in h.required_keys
    with pytest.raises(KeyError):
        costs.HybridCost("minimize", {"no_such_cost": 1.0})
    with pytest.raises(ValueError):
        costs.focus_functions["mean_square"](direction="sideways")


def test_descriptors_of_the_focus_names():
    codes = {"mean_square": 2, "laplacian_magnitude": 3, "hessian_magnitude": 4}
    for kind, code in codes.items():
        d = cmax.make_descriptor(kind, "2d-translation", warp_direction="middle")
        assert (d.cost, d.normalized, d.n_ref, d.negate, d.ref_mode[0]) == (code, 0, 1, 0, _lib.REF_FRAC)
        d = cmax.make_descriptor("normalized_" + kind, "dense-flow", direction="maximize")
        assert (d.cost, d.normalized, d.n_ref, d.minimize, d.negate) == (code, 1, 1, 0, 0)
        d = cmax.make_descriptor("multi_focal_normalized_" + kind, "dense-flow-voxel", direction="maximize", time_bin=3)
        assert (d.cost, d.normalized, d.n_ref, d.negate, d.T) == (code, 1, 3, 1, 3)
        assert [d.mult[k] for k in range(3)] == [1.0, 1.0, 2.0]
    with pytest.raises(KeyError):
        cmax.make_descriptor("entropy", "2d-translation")


def test_header_constants_match_lib():
    text = open(os.path.join(ROOT, "include", "cmax_hip.h")).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(CMAX_COST_\w+)\s+(\d+)", text)}
    assert defs == {"CMAX_COST_VARIANCE": _lib.COST_VARIANCE, "CMAX_COST_GRADMAG": _lib.COST_GRADMAG, "CMAX_COST_MEAN_SQUARE": _lib.COST_MEAN_SQUARE,
                    "CMAX_COST_LAPLACIAN": _lib.COST_LAPLACIAN, "CMAX_COST_HESSIAN": _lib.COST_HESSIAN}
    assert (_lib.COST_MEAN_SQUARE, _lib.COST_LAPLACIAN, _lib.COST_HESSIAN) == (2, 3, 4)
    assert int(re.search(r"#define\s+CMAX_ABI_VERSION\s+(\d+)", text).group(1)) == 4
    assert _lib.load().cmax_abi_version() == 4


@pytest.mark.parametrize("cid", list(C.ALL))
def test_the_gpu_cases_drop_few_events_and_move_them_little(cid):
    c = C.ALL[cid]
    b = C.inputs(c)
    assert b["dropped"] <= C.DROP_CAP, (cid, b["dropped"])
    assert len(b["ev"]) >= 0.95 * C.N_EVENTS
    assert HR.max_displacement(b["ev"], b["motion"], c["model"], c["size"], R.cost_directions(c["cost"])) <= 10.0
