"""The handle's and the patch plan's owning buffers (csrc/cmax_buffers.h).

Accounting: CMaxHandle.workspace_bytes is the HBM the handle holds NOW -- a handle that saw a small batch first reports what a
handle that saw only the large one reports.  Regrowth: every buffer that grows on demand gives, after a small request and then a larger
one, what a fresh handle gives for the larger one -- bit for bit in deterministic mode; the entries that have no deterministic mode are
compared at the tolerance their own tests use (tests/test_gpu_weights.py, test_gpu_weight_grad.py, test_gpu_event_grad.py,
test_gpu_iwe_layer.py, test_gpu_fused.py, test_gpu_solver.py: 1e-4 of the largest entry).  64 x 64 sensor, 2 000 and 20 000 events."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import event_based_optical_flow_amd as E  # noqa: E402
from event_based_optical_flow_amd.solver import PatchFlowObjective  # noqa: E402

SIZE = (64, 64)
N_A, N_B = 2_000, 20_000
TOL = 1e-4
THETA = np.array([7.0, -4.5])


@pytest.fixture(scope="module")
def batches():
    ev = E.utils.generate_structured_events(N_B, SIZE[0], SIZE[1], (9.0, -6.0), n_dots=60, seed=11, dtype=np.float32)
    a = np.ascontiguousarray(ev[::N_B // N_A][:N_A])
    assert a.shape[0] == N_A and ev.dtype == np.float32 and (ev[:, :2] == np.round(ev[:, :2])).all()
    return a, ev


def flow_of(seed, *lead):
    rng = np.random.default_rng(seed)
    return rng.uniform(-6.0, 6.0, lead + (2,) + SIZE)


def handle(ev, deterministic=False, **kw):
    h = E.CMaxHandle(SIZE)
    if deterministic:
        h.set_deterministic(True)
    return h.set_events(ev, **kw)


def host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def assert_same(got, want, exact, what, result_first=True):
    """got / want: tuples of arrays (None entries skipped).  result_first: entry 0 is a result block [..., 8], of which the loss
    ([..., 0]) is compared -- an objective writes only the slots its descriptor uses."""
    if result_first:
        got, want = (got[0][..., :1],) + tuple(got[1:]), (want[0][..., :1],) + tuple(want[1:])
    for i, (g, w) in enumerate(zip(got, want)):
        if g is None and w is None:
            continue
        g, w = host(g), host(w)
        assert g.shape == w.shape, (what, i)
        if exact:
            assert g.tobytes() == w.tobytes(), (what, i, np.abs(g.astype(np.float64) - w.astype(np.float64)).max())
        else:
            err = np.abs(g.astype(np.float64) - w.astype(np.float64)).max()
            assert err <= TOL * np.abs(w.astype(np.float64)).max(), (what, i, err)


# ---- accounting -----------------------------------------------------------------------------------------------------------------
def test_workspace_bytes_are_the_live_bytes(batches):
    a, b = batches
    desc = E.make_descriptor("image_variance", "2d-translation")
    h1 = handle(b)
    h2 = handle(a)
    small = h2.workspace_bytes
    segs_a = h2.work_list_info()["segments"]
    h2.set_events(b)
    assert segs_a <= h2.work_list_info()["segments"] == h1.work_list_info()["segments"]
    print(f"[buffers] workspace: {small} bytes with {N_A} events, {h1.workspace_bytes} with {N_B}, {h2.workspace_bytes} after both")
    assert small < h1.workspace_bytes
    assert h2.workspace_bytes == h1.workspace_bytes
    h2.set_events(a)  # fits: nothing is given back, nothing is taken
    assert h2.workspace_bytes == h1.workspace_bytes
    h2.set_events(b)
    figures = []
    for _ in range(3):
        h2.evaluate(desc, THETA)
        figures.append(h2.workspace_bytes)
    assert figures[1] == figures[2] >= h1.workspace_bytes
    v = np.array([1.0, -0.5])
    h2.hvp(desc, THETA, v)  # the second-order scratch, on first use
    first = h2.workspace_bytes
    assert first > figures[2]
    h2.hvp(desc, THETA, v)
    h2.evaluate(desc, THETA)
    assert h2.workspace_bytes == first


# ---- regrowth keeps results -----------------------------------------------------------------------------------------------------
def test_events_regrow(batches):
    a, b = batches
    desc = E.make_descriptor("image_variance", "2d-translation", sigma=1.0)
    h = handle(a, deterministic=True)
    h.evaluate(desc, THETA)
    h.set_events(b)
    assert_same(h.evaluate(desc, THETA), handle(b, deterministic=True).evaluate(desc, THETA), True, "events")


def test_candidate_batch_regrows(batches):
    desc = E.make_descriptor("image_variance", "2d-translation")
    thetas = np.array([(7.0, -4.5), (3.0, 1.0), (-6.5, 2.25), (0.5, 0.25), (9.0, -6.0)])
    h = handle(batches[1])
    h.evaluate_batch(desc, thetas[:2])
    assert_same(h.evaluate_batch(desc, thetas), handle(batches[1]).evaluate_batch(desc, thetas), False, "evaluate_batch")
    # ... and behind a longer work list, which drops the workspace (its layout follows the segments)
    h = handle(batches[0])
    h.evaluate_batch(desc, thetas)
    h.set_events(batches[1])
    assert_same(h.evaluate_batch(desc, thetas), handle(batches[1]).evaluate_batch(desc, thetas), False, "evaluate_batch after a new work list")


def test_iwes_vjp_zero_tangent_regrows(batches):
    g = np.random.default_rng(3).uniform(-1.0, 1.0, (1,) + SIZE)
    flow = flow_of(5)
    h = handle(batches[1])
    h.iwes_vjp(THETA, "2d-translation", g)
    got = h.iwes_vjp(flow, "dense-flow", g)
    assert_same(got[:1], handle(batches[1]).iwes_vjp(flow, "dense-flow", g)[:1], False, "iwes_vjp", result_first=False)


def test_host_gradient_regrows(batches):
    flow = flow_of(6)
    h = handle(batches[1], deterministic=True)
    h.evaluate_host(E.make_descriptor("image_variance", "2d-translation"), THETA)
    desc = E.make_descriptor("image_variance", "dense-flow", sigma=1.0)
    assert_same(h.evaluate_host(desc, flow), handle(batches[1], deterministic=True).evaluate_host(desc, flow), True, "evaluate_host")


@pytest.mark.parametrize("exact_flow", [False, True])
def test_dense_then_voxel_regrow(batches, exact_flow):
    """Deterministic flow gradients (the fixed-point accumulators), with exact_flow the split planes of an fp64 motion as well."""
    T = 3
    flow, voxel = flow_of(7), flow_of(8, T)
    dense = E.make_descriptor("image_variance", "dense-flow", sigma=1.0)
    vox = E.make_descriptor("image_variance", "dense-flow-voxel", sigma=1.0, time_bin=T)
    h = handle(batches[1], deterministic=True)
    h.evaluate(dense, flow, exact_flow=exact_flow)
    h.set_time_bins(T)
    fresh = handle(batches[1], deterministic=True)
    fresh.set_time_bins(T)
    assert_same(h.evaluate(vox, voxel, exact_flow=exact_flow), fresh.evaluate(vox, voxel, exact_flow=exact_flow), True, "voxel gradient")


@pytest.mark.parametrize("entry", ["evaluate_weight_grad", "evaluate_event_grad"])
def test_per_event_gradients_regrow(batches, entry):
    a, b = batches
    desc = E.make_descriptor("image_variance", "2d-translation", sigma=1.0)
    h = handle(a)
    getattr(h, entry)(desc, THETA)
    h.set_events(b)
    assert_same(getattr(h, entry)(desc, THETA), getattr(handle(b), entry)(desc, THETA), False, entry)


def test_event_weights_regrow(batches):
    a, b = batches
    desc = E.make_descriptor("image_variance", "2d-translation", sigma=1.0)
    w = np.random.default_rng(9).uniform(0.25, 2.0, N_B).astype(np.float32)
    h = handle(a, weights=w[:N_A])
    h.evaluate(desc, THETA)
    h.set_events(b, weights=w)
    assert_same(h.evaluate(desc, THETA), handle(b, weights=w).evaluate(desc, THETA), False, "set_event_weights")


def test_patch_search_regrows(batches):
    rng = np.random.default_rng(10)
    boxes = np.array([[16 * (p // 4), 16 * (p // 4) + 16, 16 * (p % 4), 16 * (p % 4) + 16] for p in range(16)])
    cand = rng.uniform(-200.0, 200.0, (16, 3, 2))
    h = handle(batches[1])
    h.patch_search(boxes[:4], (16, 16), cand[:4], 1.0)
    got = h.patch_search(boxes, (16, 16), cand, 1.0)
    want = handle(batches[1]).patch_search(boxes, (16, 16), cand, 1.0)
    assert_same(got[1:], want[1:], False, "patch_search", result_first=False)  # (gm, count; the loss is their quotient)


# ---- patch plan -----------------------------------------------------------------------------------------------------------------
def _plan(golden, handle_):
    gs, case = golden("solver_scale_later"), "burgers_s3"
    ev = golden("solver_objective")["events"]
    return PatchFlowObjective(handle_, float(ev[:, 2].max() - ev[:, 2].min()), gs[case + "__patch_image_size"], gs[case + "__patch_size"],
                              gs[case + "__sliding_window"], gs[case + "__patch_shift"], cost="hybrid",
                              cost_with_weight={"multi_focal_normalized_gradient_magnitude": 1.0, "total_variation": 0.01}, blur_sigma=1,
                              time_aware=True, time_bin=10, flow_interpolation=str(gs[case + "__flow_interpolation"]),
                              t0_flow_location=str(gs[case + "__t0_flow_location"]), scale_later=True)


def test_patch_plan_first_use_buffers_and_destroy(golden):
    """A time-aware scale_later plan: its second-order buffers come with the first Hessian-vector product.  Twice on one plan against a
    fresh plan (deterministic handle: bit for bit); a plan is destroyed with and without them."""
    g, gs = golden("solver_objective"), golden("solver_scale_later")
    h = E.CMaxHandle(tuple(int(v) for v in g["image_size"]))
    h.set_deterministic(True)
    h.set_events(g["events"], time_bin=10)
    x, v = (np.asarray(gs["burgers_s3__" + k], dtype=np.float64).reshape(-1) for k in ("x", "v"))

    def run(obj):
        loss, grad = obj.value_and_grad_numpy(x)
        return np.float64(loss), grad, obj.hvp_numpy(x, v)

    obj = _plan(golden, h)
    assert obj.has_native_plan and obj.has_exact_hvp
    first, second = run(obj), run(obj)
    assert_same(second, first, True, "second call on one plan", result_first=False)
    del obj  # destroyed with the second-order buffers
    fresh = _plan(golden, h)
    assert_same(run(fresh), first, True, "fresh plan", result_first=False)
    del fresh
    unused = _plan(golden, h)
    unused.value_and_grad_numpy(x)
    del unused  # ... and without them
    torch.cuda.synchronize()
    assert_same(run(_plan(golden, h)), first, True, "after the destroyed plans", result_first=False)
