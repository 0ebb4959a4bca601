"""Per-event weights, what can be checked without a GPU: the reference composition of the weighted tests IS the oracle's (w == 1
reproduces orc.objective), polarity_weights, the Python-side argument validation, and the header's symbols."""
import os
import re

import numpy as np
import pytest
import torch

import event_based_optical_flow_amd as E
from event_based_optical_flow_amd import _lib
from event_based_optical_flow_amd.cmax import prepare_event_weights
from event_based_optical_flow_amd.utils.event_utils import polarity_weights
from oracle import oracle as orc

from _weighted_ref import weighted_objective

SIZE = (24, 32)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("model", ["2d-translation", "dense-flow", "dense-flow-voxel"])
@pytest.mark.parametrize("cost", ["image_variance", "gradient_magnitude", "normalized_image_variance",
                                  "multi_focal_normalized_gradient_magnitude"])
@pytest.mark.parametrize("sigma", [0, 1])
def test_helper_is_the_oracle_at_unit_weight(model, cost, sigma):
    ev = E.utils.generate_events(3000, SIZE[0], SIZE[1], 0.0, 0.05, seed=5)
    if model == "2d-translation":
        motion = np.array([3.3, -2.1])
    elif model == "dense-flow":
        motion = E.utils.generate_smooth_flow(SIZE, 3, seed=6)
    else:
        motion = np.stack([E.utils.generate_smooth_flow(SIZE, 3, seed=7 + t) for t in range(4)])
    ref = orc.objective(ev, motion, model, SIZE, cost=cost, sigma=sigma)
    for w in (1.0, np.ones(ev.shape[0])):
        got = weighted_objective(ev, motion, model, SIZE, w, cost=cost, sigma=sigma)
        assert abs(got["loss"] - ref["loss"]) <= 1e-12 * abs(ref["loss"])
        assert rel(got["grad"], ref["grad"]) <= 1e-12
        assert rel(got["iwes"]["iwe"], ref["iwes"]["iwe"]) <= 1e-12


def test_polarity_weights():
    ev = E.utils.generate_events(1000, 20, 20, seed=3)
    w = polarity_weights(ev)
    assert w.shape == (1000,) and w.dtype == ev.dtype
    assert np.array_equal(w, np.where(ev[:, 3] > 0, 1.0, -1.0))
    assert set(np.unique(w)) == {-1.0, 1.0}
    ev32 = torch.from_numpy(ev.astype(np.float32))
    wt = polarity_weights(ev32)
    assert wt.dtype == torch.float32 and np.array_equal(wt.numpy(), w.astype(np.float32))
    ev[:, 3] = np.where(ev[:, 3] > 0, 1.0, -1.0)  # (-1, +1) polarities give the same signs
    assert np.array_equal(polarity_weights(ev), w)


def test_weight_argument_validation():
    with pytest.raises(ValueError, match=r"\[n\]"):
        prepare_event_weights(np.ones((5, 2)), 5)
    with pytest.raises(ValueError, match=r"\[n\]"):
        prepare_event_weights(np.ones(4), 5)
    with pytest.raises(ValueError, match="finite"):
        prepare_event_weights(np.array([1.0, np.nan, 2.0]), 3)
    with pytest.raises(ValueError, match="finite"):
        prepare_event_weights(torch.tensor([1.0, float("inf")]), 2)
    with pytest.raises(TypeError):
        prepare_event_weights([1.0, 2.0], 2)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the message raised where no device exists")
def test_weights_need_a_gpu():
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # valid weights: the copy to the device is what fails
        prepare_event_weights(np.ones(3), 3)


def test_header_declares_the_weight_entry_points():
    text = open(os.path.join(ROOT, "include", "cmax_hip.h")).read()
    assert re.search(r"int cmax_set_event_weights\(cmax_handle_t h, const void \*weights, int dtype, int64_t n, cmax_stream_t stream\);", text)
    assert re.search(r"int cmax_batch_weighted\(cmax_handle_t h, int \*weighted, double \*wmax_host\);", text)
    assert re.search(r"#define CMAX_EUNSUPPORTED -6", text) and _lib.EUNSUPPORTED == -6
    assert "cmax_set_event_weights" in _lib.SIGNATURES and "cmax_batch_weighted" in _lib.SIGNATURES
    assert re.search(r"#define CMAX_ABI_VERSION 4\b", text) and _lib.ABI_VERSION == 4  # no struct layout changed
