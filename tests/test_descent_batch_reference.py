"""Multi-start descent (cmax_objective_descend_batch), what can be checked without a GPU: the ABI (declared / bound / exported, version
unchanged); the refusals that come before any launch -- with a null handle and no device; that the table of Adam starts the GPU tests
use is fit for their gate (a condition on the INPUTS: the entries of every fp64 reference gradient along every trajectory within a factor
3 of each other, where the GPU gate needs 4); the host logic of solver.translation_search.refine_translation / grid_search_translation's
refine_top and of the solver key patch.global_best_refine, with the library calls replaced."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from event_based_optical_flow_amd import _lib, build, solver
from event_based_optical_flow_amd.solver import common, mixed, pyramid
from event_based_optical_flow_amd.solver import translation_search as ts

import _descent_batch_cases as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cmax_hip.h")
NAME = "cmax_objective_descend_batch"


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    text = open(HEADER).read()
    assert re.search(r"#define CMAX_ABI_VERSION 4\b", text) and _lib.ABI_VERSION == 4  # a new entry point, no layout changed
    assert re.search(r"#define CMAX_DESCENT_MAX_STARTS 64\b", text) and _lib.DESCENT_MAX_STARTS == 64
    proto = re.search(r"/\*((?:(?!\*/).)*)\*/\s*#define CMAX_DESCENT_MAX_STARTS 64\s*int cmax_objective_descend_batch\(cmax_handle_t h, "
                      r"const cmax_objective_t \*desc_host, const double \*theta0_host, int K,\s*const cmax_descent_t \*descent, "
                      r"cmax_descent_result_t \*res_host,", text, re.S)
    assert proto, "prototype"
    assert "src/solver/base.py:840-881" in proto.group(1)  # the entry cites the function it replaces
    assert "8 * K * (32 + n_iter" in proto.group(1)        # and says how large its state is
    lib = _lib.load()
    assert lib.cmax_abi_version() == 4
    assert NAME in _lib.SIGNATURES and getattr(lib, NAME).argtypes == _lib.SIGNATURES[NAME][1]
    P = ctypes.POINTER
    assert _lib.SIGNATURES[NAME] == (ctypes.c_int, [ctypes.c_void_p, P(_lib.CmaxObjective), ctypes.c_void_p, ctypes.c_int, P(_lib.CmaxDescent)] + [ctypes.c_void_p] * 6)
    exported = subprocess.run(["nm", "-D", "--defined-only", build.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T %s$" % NAME, exported, re.M)


# ---- refusals before any launch ----------------------------------------------------------------------------------------------------------
def _good():
    return _lib.descent_descriptor("Adam", n_iter=6, lr=0.05, lr_step=2, lr_decay=0.5)


# (the table of tests/test_descent_reference.py, restated)
BAD = [
    ("method", 7, "method"), ("n_iter", 0, "n_iter"), ("n_iter", 4097, "n_iter"), ("lr", 0.0, "lr "), ("lr", float("nan"), "lr "),
    ("lr", float("inf"), "lr "), ("lr_decay", -0.5, "lr_decay"), ("lr_decay", float("inf"), "lr_decay"), ("eps", 0.0, "eps"),
    ("eps", float("nan"), "eps"), ("lr_step", 0, "lr_step"), ("momentum", 1.0, "momentum"), ("momentum", -0.1, "momentum"),
    ("beta1", 1.0, "beta1"), ("beta1", float("nan"), "beta1"), ("beta2", 1.5, "beta2"), ("beta2", -1e-3, "beta2"),
]


@pytest.mark.parametrize("field,value,word", BAD, ids=[f"{f}={v}" for f, v, _ in BAD])
def test_bad_descriptors_are_refused_before_any_gpu_call(field, value, word):
    """No handle, no device: the descriptor is checked first and the message names the field."""
    lib = _lib.load()
    d = _good()
    setattr(d, field, value)
    res, buf = (_lib.CmaxDescentResult * 2)(), np.zeros(64)
    p = buf.ctypes.data
    rc = lib.cmax_objective_descend_batch(None, None, p, 2, ctypes.byref(d), res, p, p, p, None, None)
    assert rc == _lib.EINVAL == -1
    msg = lib.cmax_last_error().decode()
    assert "objective_descend_batch" in msg and "bad descent descriptor" in msg and word in msg, msg


def test_other_refusals_with_a_null_handle():
    lib = _lib.load()
    d, res, buf, desc = _good(), (_lib.CmaxDescentResult * 2)(), np.zeros(64), _lib.CmaxObjective()
    p, dref = buf.ctypes.data, ctypes.byref(desc)
    fn = lib.cmax_objective_descend_batch
    assert fn(None, dref, p, 2, None, res, p, p, p, None, None) == _lib.EINVAL
    assert "null descriptor" in lib.cmax_last_error().decode()
    for K in (0, -1, 65):
        assert fn(None, dref, p, K, ctypes.byref(d), res, p, p, p, None, None) == _lib.EINVAL
        assert "1 <= K <= 64" in lib.cmax_last_error().decode()
    calls = {
        "handle": lambda: fn(None, dref, p, 2, ctypes.byref(d), res, p, p, p, None, None),
        "desc": lambda: fn(None, None, p, 2, ctypes.byref(d), res, p, p, p, None, None),
        "theta0": lambda: fn(None, dref, None, 2, ctypes.byref(d), res, p, p, p, None, None),
        "res": lambda: fn(None, dref, p, 2, ctypes.byref(d), None, p, p, p, None, None),
        "x_last": lambda: fn(None, dref, p, 2, ctypes.byref(d), res, None, p, p, None, None),
        "x_best": lambda: fn(None, dref, p, 2, ctypes.byref(d), res, p, None, p, None, None),
        "history": lambda: fn(None, dref, p, 2, ctypes.byref(d), res, p, p, None, None, None),
    }
    for what, call in calls.items():
        assert call() == _lib.EINVAL, what
        assert "objective_descend_batch: null pointer" in lib.cmax_last_error().decode(), what


# ---- the start table is fit for its Adam gate -----------------------------------------------------------------------------------------------
def test_adam_starts_keep_the_gradient_entries_within_a_factor_three():
    """Adam's step bound in tests/test_gpu_descent_batch.py holds once the reference gradient's entries are within a factor 4 of each other;
    along the fp64 trajectory of every start of the table they stay within 3, which leaves room for the GPU's iterates to differ."""
    assert B.ADAM_STARTS.shape == (9, 2) and B.events().shape == (4000, 4)
    worst = {}
    for start in B.ADAM_STARTS:
        xs, losses, grads = B.ref_trajectory(start, "adam")
        ratios = np.abs(grads).max(axis=1) / np.abs(grads).min(axis=1)
        worst[tuple(float(v) for v in start)] = float(ratios.max())
        assert np.isfinite(losses).all() and np.abs(xs[-1] - start).max() > 0.0
    print("[descent-batch] max|g| / min|g| along the fp64 Adam trajectories: " + ", ".join(f"{s}: {r:.2f}" for s, r in worst.items()))
    print(f"[descent-batch] range {min(worst.values()):.2f} .. {max(worst.values()):.2f}")
    assert max(worst.values()) <= 3.0, worst


# ---- host logic of the refinement ---------------------------------------------------------------------------------------------------------
class FakeHandle:
    def __init__(self, n_events=100):
        self.n_events = n_events
        self.slab_requests = []

    def auto_time_slabs(self, displacement_px):
        self.slab_requests.append(float(displacement_px))
        return 0


class FakeResult:
    def __init__(self, x_best, best_loss):
        self.x_best, self.best_loss = np.asarray(x_best, dtype=np.float64), float(best_loss)


@pytest.fixture
def fake_objective(monkeypatch):
    """translation_search.ContrastObjective replaced: descend_batch records its calls and answers from `losses` (per start, in order),
    every trajectory ending 0.25 / -0.5 away from its start."""
    log = {"calls": [], "made": [], "losses": None}

    class FakeObjective:
        def __init__(self, handle, model, cost="image_variance", cost_with_weight=None, sigma=0.0):
            log["made"].append(dict(model=model, cost=cost, cost_with_weight=cost_with_weight, sigma=sigma))

        def descend_batch(self, thetas, **kw):
            thetas = np.asarray(thetas)
            log["calls"].append((thetas.copy(), kw))
            losses = log["losses"] if log["losses"] is not None else -np.arange(len(thetas), dtype=np.float64)
            return [FakeResult(t + np.array([0.25, -0.5]), l) for t, l in zip(thetas, losses)]

    monkeypatch.setattr(ts, "ContrastObjective", FakeObjective)
    return log


def test_refine_translation_units_and_winner(fake_objective):
    h, starts = FakeHandle(), np.array([[10.0, -20.0], [0.0, 0.0], [30.0, 40.0], [-10.0, 10.0]])
    fake_objective["losses"] = [3.0, float("nan"), 1.0, 1.0]  # the FIRST minimum wins; a NaN never
    guess, results = ts.refine_translation(h, 0.05, starts, method="SGD", n_iter=7, lr=0.1, cost="image_variance", sigma=0)
    (thetas, kw), = fake_objective["calls"]
    np.testing.assert_allclose(thetas, starts * 0.05, rtol=0, atol=0)  # the descent runs in warp units
    assert kw == dict(method="SGD", n_iter=7, lr=0.1) and len(results) == 4
    np.testing.assert_allclose(guess, (starts[2] * 0.05 + [0.25, -0.5]) / 0.05, rtol=1e-15)  # x_best / t_scale of start 2
    assert h.slab_requests == [pytest.approx(40.0 * 0.05 + 0.1 * 7)]  # time slabs once, from max |theta0| + lr n_iter
    fake_objective["losses"] = [float("inf"), float("nan"), float("inf"), float("nan")]
    guess, _ = ts.refine_translation(h, 0.05, starts)
    np.testing.assert_array_equal(guess, starts[0])  # no finite loss: the first start as it came
    fake_objective["losses"] = [float("inf"), 2.0, float("nan"), 2.0]
    guess, _ = ts.refine_translation(h, 0.05, starts)
    np.testing.assert_allclose(guess, (starts[1] * 0.05 + [0.25, -0.5]) / 0.05, rtol=1e-15)


def test_refine_translation_without_anything_to_descend_on(fake_objective):
    starts = np.array([[10.0, -20.0], [0.0, 0.0]])
    for h, t_scale in ((FakeHandle(), 0.0), (FakeHandle(0), 0.05)):
        guess, results = ts.refine_translation(h, t_scale, starts)
        np.testing.assert_array_equal(guess, starts[0])
        assert results == [] and h.slab_requests == []
    assert fake_objective["calls"] == [] and fake_objective["made"] == []
    with pytest.raises(ValueError, match="at least one start"):
        ts.refine_translation(FakeHandle(), 0.05, np.zeros((0, 2)))


def test_refine_translation_drops_total_variation_of_a_hybrid(fake_objective):
    ts.refine_translation(FakeHandle(), 0.05, np.ones((2, 2)), cost="hybrid", cost_with_weight={"gradient_magnitude": 1.0, "total_variation": 0.01}, sigma=1)
    assert fake_objective["made"][-1] == dict(model="2d-translation", cost="gradient_magnitude", cost_with_weight=None, sigma=1)
    two = {"gradient_magnitude": 1.0, "image_variance": 0.5}
    ts.refine_translation(FakeHandle(), 0.05, np.ones((2, 2)), cost="hybrid", cost_with_weight=two)  # left to ContrastObjective's own refusals
    assert fake_objective["made"][-1]["cost"] == "hybrid" and fake_objective["made"][-1]["cost_with_weight"] == two


def _grid(monkeypatch, table):
    """candidate_losses replaced by a table [len(fx), len(fy)] (x outer, y inner)."""
    seen = []

    def fake_losses(handle, cand, t_scale, **kw):
        seen.append(kw)
        return np.asarray(table, dtype=np.float64).reshape(-1).copy()

    monkeypatch.setattr(ts, "candidate_losses", fake_losses)
    return seen


def test_grid_search_picks_its_starts_in_stable_order(fake_objective, monkeypatch):
    nan = float("nan")
    table = [[5.0, 1.0, nan], [1.0, 3.0, 0.5], [0.5, nan, 4.0]]  # field (0, 10, 20)^2: minimum 0.5 first at (10, 20), then (20, 0)
    _grid(monkeypatch, table)
    h, field = FakeHandle(), np.array([0.0, 10.0, 20.0])
    plain, loss = ts.grid_search_translation(h, 1.0, field)
    np.testing.assert_array_equal(plain, [10.0, 20.0])
    assert fake_objective["calls"] == []  # refine_top = 0: not one call more
    guess, loss2, results = ts.grid_search_translation(h, 1.0, field, refine_top=4, refine=dict(method="Adam", n_iter=3, lr=0.05), cost="image_variance", sigma=0, chunk=16)
    np.testing.assert_array_equal(loss, loss2)
    (thetas, kw), = fake_objective["calls"]
    # 0.5 (10, 20), 0.5 (20, 0), 1.0 (0, 10), 1.0 (10, 0): equal losses keep the grid's order, the grid's own pick is start 0
    np.testing.assert_array_equal(thetas, [[10.0, 20.0], [20.0, 0.0], [0.0, 10.0], [10.0, 0.0]])
    assert kw == dict(method="Adam", n_iter=3, lr=0.05) and len(results) == 4
    np.testing.assert_array_equal(guess, thetas[3] + [0.25, -0.5])  # the fake's losses fall with the start's index
    # fewer finite candidates than k: all seven of them, no NaN among the starts
    fake_objective["calls"].clear()
    ts.grid_search_translation(h, 1.0, field, refine_top=50)
    (thetas, _), = fake_objective["calls"]
    assert thetas.shape == (7, 2) and {tuple(t) for t in thetas} == {(0, 0), (0, 10), (10, 0), (10, 10), (10, 20), (20, 0), (20, 20)}
    # no finite candidate: the reference's zeros(2), nothing refined
    fake_objective["calls"].clear()
    _grid(monkeypatch, np.full((3, 3), nan))
    guess, _, results = ts.grid_search_translation(h, 1.0, field, refine_top=4)
    np.testing.assert_array_equal(guess, np.zeros(2))
    assert results == [] and fake_objective["calls"] == []


def test_whole_image_guess_refines_only_when_asked(fake_objective, monkeypatch):
    table = np.arange(900.0).reshape(30, 30)[::-1].copy()  # minimum at the grid's last row
    _grid(monkeypatch, table)
    h = FakeHandle()
    out = common.whole_image_guess(h, 0.05, cost="image_variance", cost_with_weight=None, sigma=0)
    assert len(out) == 2 and fake_objective["calls"] == []
    np.testing.assert_array_equal(out[0], [140.0, -150.0])
    guess, loss, results = common.whole_image_guess(h, 0.05, refine=dict(top_k=3, n_iter=20, method="Adam", lr=0.02), cost="image_variance", cost_with_weight=None, sigma=0)
    (thetas, kw), = fake_objective["calls"]
    np.testing.assert_allclose(thetas, np.array([[140.0, -150.0], [140.0, -140.0], [140.0, -130.0]]) * 0.05)
    assert kw == dict(method="Adam", n_iter=20, lr=0.02) and len(results) == 3 and loss.shape == (30, 30)
    assert common.global_best_refine({"patch": {"initialize": "global-best"}}) is None
    assert common.global_best_refine({"patch": {"global_best_refine": {"top_k": 2}}}) == {"top_k": 2}
    with pytest.raises(KeyError, match="unknown keys"):
        common.global_best_refine({"patch": {"global_best_refine": {"topk": 2}}})


PARAMS = {"trans_x": {"min": -150, "max": 150}, "trans_y": {"min": -150, "max": 150}}
COMMON = {"motion_model": "2d-translation", "warp_direction": "first", "parameters": ["trans_x", "trans_y"], "cost": "image_variance", "outer_padding": 0,
          "iwe": {"method": "bilinear_vote", "blur_sigma": 0}}
OPT_CFG = {"n_iter": 5, "method": "Adam", "max_iter": 25, "parameters": PARAMS}
REFINE = {"top_k": 4, "n_iter": 20, "method": "Adam", "lr": 0.05}


def make(kind, refine):
    patch = {"initialize": "global-best"}
    if refine is not None:
        patch["global_best_refine"] = dict(refine)
    if kind == "pyramid":
        cfg = dict(COMMON, method="pyramidal_patch_contrast_maximization", time_aware=False,
                   patch=dict(patch, scale=3, crop_height=64, crop_width=80, filter_type="bilinear"))
        return solver.collections["pyramidal_patch_contrast_maximization"]((66, 90), {}, cfg, dict(OPT_CFG), {}, None)
    time_aware = kind == "time-aware"
    cfg = dict(COMMON, time_aware=time_aware, patch=dict(patch, size=16, sliding_window=16, filter_type="bilinear"))
    if time_aware:
        cfg.update(time_bin=10, flow_interpolation="burgers", t0_flow_location="middle")
        return solver.collections["time_aware_mixed_patch_contrast_maximization"]((68, 90), {}, cfg, dict(OPT_CFG), {}, None)
    return solver.MixedPatchContrastMaximization((68, 90), {}, cfg, dict(OPT_CFG), {}, None)


@pytest.mark.parametrize("refine", [None, REFINE], ids=["absent", "present"])
@pytest.mark.parametrize("kind", ["pyramid", "mixed", "time-aware"])
def test_solver_classes_read_the_key(kind, refine, monkeypatch):
    """All three solver classes hand patch.global_best_refine to whole_image_guess for "global-best" -- and None when the key is absent,
    which is the call they made before (whole_image_guess then makes none of its own, see above)."""
    seen = []

    def fake_guess(handle, t_scale, refine=None, **search_cost):
        seen.append((refine, search_cost))
        out = (np.array([10.0, -20.0]), np.zeros((30, 30)))
        return out if refine is None else out + (["per-start results"],)

    slv = make(kind, refine)
    events = np.array([[1.0, 2.0, 0.0, 1.0], [3.0, 4.0, 0.05, 0.0]])
    if kind == "pyramid":
        monkeypatch.setattr(pyramid, "whole_image_guess", fake_guess)
        guess = slv.initialize_guess_from_whole_image(FakeHandle(), 0.05)
        entry = slv.search_history[-1][1:]
    else:
        monkeypatch.setattr(mixed, "whole_image_guess", fake_guess)
        monkeypatch.setattr(slv, "_translation_handle", lambda ev: FakeHandle())
        guess = slv.initialize_guess_from_whole_image(events)
        entry = slv.search_history[-1]
    np.testing.assert_array_equal(guess, [10.0, -20.0])
    (got, search_cost), = seen
    assert got == refine and search_cost == dict(cost="image_variance", cost_with_weight=search_cost["cost_with_weight"], sigma=0)
    assert entry[0] == "global-best" and len(entry) == (3 if refine is None else 4)
