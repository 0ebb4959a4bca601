"""The head of the event kernels (csrc/cmax_event_kernels.inc: k_vote, k_grad): theta, the batch's time extremes and K1's published
window are read through the kernels' leading parameters at entry, beside the segment descriptor, and every wave -- a dead one too --
issues its event loads unconditionally.  Everything here goes against the fp64 oracle (oracle.objective) at the project's plain gate,
1e-4 relative on loss and gradient, on a 48 x 64 sensor, at the smallest shapes at which that head can go wrong:

  dead waves          batches of 1, 2 and 3 events (every wave but the first holds no event and loads the segment's last pair)
  the buffer's end    a last segment that starts at an odd index and ends at the buffer's last event
  theta's dtype       fp32 and fp64 (read in either form through the same pair of loads)
  time normalisation  normalize_t on and off (the period comes from the preloaded pointer to the batch's extremes)
  reference times     three of them (blockIdx.y: d[y], the windows at zy > 0)
  candidates          cmax_objective_batch with three motions (blockIdx.z * z_motion through the preloaded pointer)
  theta in place      overwritten on the device between two calls of one prepared call
  flow models         one dense and one voxel evaluation (the flow's pointer is the preloaded one)
  weights             a weighted handle
  graphs              one evaluation captured with torch.cuda.graph and replayed twice

Layouts: up to 512 segments run the 256-thread kernels (t256: four waves, so three dead ones in the tiny batches); the cases of
test_t512_* hold 150 000 events, which the host cuts into more than 512 segments of at most 293 events -- the 512-thread kernels of
the headline (t512: eight waves of 256 slots each, the first full, the second partly filled, six dead).

A batch of ONE event has no period: with normalize_t the reference divides 0 by 0 (the oracle returns a NaN gradient), so that batch
is evaluated without it -- there dt = t - t_ref = 0 exactly and the gradient is exactly zero, on both sides.
Oracle references are computed once per case and shared.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import event_based_optical_flow_amd as E  # noqa: E402
from oracle import oracle as orc  # noqa: E402

from _weighted_ref import weighted_objective  # noqa: E402

TOL = 1e-4
SIZE = (48, 64)
MODEL = "2d-translation"
THETA = (7.3, -4.1)
THETAS3 = ((7.3, -4.1), (-2.6, 9.4), (0.4, -0.3))
T_BINS = 4


def rel_max(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def uniform_events():
    ev = E.utils.generate_events(20_000, SIZE[0], SIZE[1], 0.0, 0.05, seed=102)
    ev.setflags(write=False)
    return ev


@functools.lru_cache(maxsize=None)
def tiny_events(n):
    """n events well inside the sensor, on integer pixels, at distinct times."""
    rng = np.random.default_rng(300 + n)
    ev = np.empty((n, 4))
    ev[:, 0] = rng.integers(12, SIZE[0] - 12, n)
    ev[:, 1] = rng.integers(12, SIZE[1] - 12, n)
    ev[:, 2] = 0.01 + 0.04 * np.arange(n) / max(n - 1, 1)
    ev[:, 3] = 1.0
    ev.setflags(write=False)
    return ev


@functools.lru_cache(maxsize=None)
def odd_tail_events():
    """2295 events in the sensor's first 16 x 16 tile, 200 in the first tile of the next tile row.  A batch this small is cut into
    segments of at most 256 events: the first tile becomes nine segments of 255, and the second tile's segment starts at the odd index
    2295 and ends at the buffer's last event."""
    rng = np.random.default_rng(77)
    n_a, n_b = 2295, 200
    ev = np.empty((n_a + n_b, 4))
    ev[:n_a, 0] = rng.integers(0, 16, n_a)
    ev[n_a:, 0] = rng.integers(16, 32, n_b)
    ev[:, 1] = rng.integers(0, 16, n_a + n_b)
    ev[:, 2] = rng.uniform(0.0, 0.05, n_a + n_b)
    ev[:, 3] = 1.0
    ev = ev[rng.permutation(n_a + n_b)]
    ev.setflags(write=False)
    return ev


@functools.lru_cache(maxsize=None)
def reference(events, theta, cost="image_variance", normalize_t=True):
    ev = {"uniform": uniform_events, "odd_tail": odd_tail_events}[events]() if isinstance(events, str) else tiny_events(events)
    r = orc.objective(ev, np.asarray(theta, np.float64), MODEL, SIZE, cost=cost, sigma=0, normalize_t=normalize_t)
    return r["loss"], r["grad"]


def gate(label, res, grad, ref):
    loss, g = ref
    res, grad = np.asarray(res, np.float64), np.asarray(grad, np.float64)
    e_loss = abs(res[0] - loss) / abs(loss)
    e_grad = rel_max(grad, g)
    print(f"[head loads] {label}: loss {res[0]:.9e} oracle {loss:.9e} rel err {e_loss:.2e}; gradient rel err {e_grad:.2e}")
    assert e_loss <= TOL and e_grad <= TOL, (label, e_loss, e_grad)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@pytest.mark.parametrize("n", [1, 2, 3])
def test_dead_waves(n):
    """Segments of one to n events (events of different tile rows do not share one): the first wave holds them, every other wave is dead
    and re-reads the segment's last pair."""
    normalize_t = n > 1  # (one event has no period: see the module's docstring)
    ev = tiny_events(n)
    h = E.CMaxHandle(SIZE).set_events(ev)
    assert 1 <= h.work_list_info()["segments"] <= n
    desc = E.make_descriptor("image_variance", MODEL, normalize_t=normalize_t)
    ref = reference(n, THETA, normalize_t=normalize_t)
    for rep in range(2):  # (the vote images are double-buffered)
        res, grad = h.evaluate(desc, np.array(THETA))
        res, grad = res.cpu().numpy(), grad.cpu().numpy()
        if n == 1:
            e_loss = abs(res[0] - ref[0]) / abs(ref[0])
            print(f"[head loads] 1 event #{rep}: loss rel err {e_loss:.2e}; gradient {grad} (oracle {ref[1]})")
            assert e_loss <= TOL and np.all(ref[1] == 0.0) and np.all(grad == 0.0), (e_loss, grad)
        else:
            gate(f"{n} events #{rep}", res, grad, ref)
    h.close()


def test_last_segment_starts_odd_and_ends_the_buffer():
    ev = odd_tail_events()
    h = E.CMaxHandle(SIZE).set_events(ev)
    _, group_starts = h.packed_events()
    starts = np.unique(group_starts)
    assert h.work_list_info()["segments"] == 10 and starts[-1] == ev.shape[0] and starts[-2] == 2295, (h.work_list_info(), starts)
    for theta in (THETA, (0.0, 0.0)):
        res, grad = h.evaluate(E.make_descriptor("image_variance", MODEL), np.array(theta))
        gate(f"odd tail theta {theta}", res.cpu().numpy(), grad.cpu().numpy(), reference("odd_tail", theta))
    h.close()


@pytest.fixture(scope="module")
def handle():
    h = E.CMaxHandle(SIZE).set_events(uniform_events())
    yield h
    h.close()


@pytest.mark.parametrize("normalize_t", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_theta_dtype_and_time_normalisation(handle, dtype, normalize_t):
    theta = np.asarray(THETA) / (1.0 if normalize_t else 0.05)  # (pixels per second over the batch's 50 ms: the same displacements)
    if dtype == torch.float32:
        theta = f32(theta)
    m = dev(theta).to(dtype)
    desc = E.make_descriptor("image_variance", MODEL, normalize_t=normalize_t)
    res, grad = handle.evaluate(desc, m)
    gate(f"theta {dtype} normalize_t {normalize_t}", res.cpu().numpy(), grad.cpu().numpy(),
         reference("uniform", tuple(float(v) for v in theta), normalize_t=normalize_t))


@functools.lru_cache(maxsize=None)
def many_events():
    ev = E.utils.generate_events(150_000, SIZE[0], SIZE[1], 0.0, 0.05, seed=103)
    ev.setflags(write=False)
    return ev


@functools.lru_cache(maxsize=None)
def many_reference(theta, normalize_t):
    r = orc.objective(many_events(), np.asarray(theta, np.float64), MODEL, SIZE, cost="image_variance", sigma=0, normalize_t=normalize_t)
    return r["loss"], r["grad"]


@pytest.fixture(scope="module")
def handle_t512():
    h = E.CMaxHandle(SIZE).set_events(many_events())
    info = h.work_list_info()
    assert info["segments"] > 512 and info["segment_events"] == 2040, info  # (vote_layout / grad_layout: t512)
    yield h
    h.close()


@pytest.mark.parametrize("normalize_t", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_t512_theta_dtype_and_time_normalisation(handle_t512, dtype, normalize_t):
    """The 512-thread kernels: six dead waves per workgroup, theta in both dtypes, the period from the preloaded pointer."""
    theta = np.asarray(THETA) / (1.0 if normalize_t else 0.05)
    if dtype == torch.float32:
        theta = f32(theta)
    res, grad = handle_t512.evaluate(E.make_descriptor("image_variance", MODEL, normalize_t=normalize_t), dev(theta).to(dtype))
    gate(f"t512 theta {dtype} normalize_t {normalize_t}", res.cpu().numpy(), grad.cpu().numpy(),
         many_reference(tuple(float(v) for v in theta), normalize_t))


def test_t512_unaligned_fp32_theta(handle_t512):
    """An fp32 theta that is only 4-byte aligned (a slice of the caller's tensor) is read dword by dword."""
    buf = dev(np.concatenate([[0.0], f32(THETA)])).to(torch.float32)
    m = buf[1:]
    assert m.data_ptr() % 8 == 4
    call, res, grad = handle_t512.prepare(E.make_descriptor("image_variance", MODEL), m)
    assert call.motion_is_callers
    call()
    gate("t512 unaligned theta", res.cpu().numpy(), grad.cpu().numpy(), many_reference(tuple(float(v) for v in f32(THETA)), True))


def test_three_reference_times(handle):
    cost = "multi_focal_normalized_image_variance"
    res, grad = handle.evaluate(E.make_descriptor(cost, MODEL), np.array(THETA))
    gate("three reference times", res.cpu().numpy(), grad.cpu().numpy(), reference("uniform", THETA, cost=cost))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_batch_of_three_candidates(handle, dtype):
    """Each candidate of cmax_objective_batch against the oracle at its own theta, and against its own single evaluation."""
    thetas = f32(THETAS3) if dtype == torch.float32 else np.asarray(THETAS3)
    desc = E.make_descriptor("image_variance", MODEL)
    results, grads = handle.evaluate_batch(desc, dev(thetas).to(dtype))
    results, grads = results.cpu().numpy(), grads.cpu().numpy()
    for k in range(3):
        ref = reference("uniform", tuple(float(v) for v in thetas[k]))
        gate(f"batch {dtype} candidate {k}", results[k], grads[k], ref)
        res1, grad1 = handle.evaluate(desc, dev(thetas[k]).to(dtype))
        res1, grad1 = res1.cpu().numpy(), grad1.cpu().numpy()
        gate(f"single {dtype} candidate {k}", res1, grad1, ref)
        d_loss, d_grad = abs(results[k][0] - res1[0]) / abs(res1[0]), rel_max(grads[k], grad1)
        print(f"[head loads] candidate {k}: batch against single: loss {d_loss:.2e} gradient {d_grad:.2e}")
        assert d_loss <= TOL and d_grad <= TOL, (k, d_loss, d_grad)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_theta_overwritten_in_place(handle, dtype):
    first, second = THETAS3[0], THETAS3[1]
    m = dev(np.asarray(first)).to(dtype)
    call, res, grad = handle.prepare(E.make_descriptor("image_variance", MODEL), m)
    assert call.motion_is_callers
    call()
    ref = reference("uniform", tuple(float(v) for v in m.double().cpu().numpy()))
    gate(f"prepared {dtype}, first theta", res.cpu().numpy(), grad.cpu().numpy(), ref)
    m.copy_(dev(np.asarray(second)).to(dtype))
    call()
    ref = reference("uniform", tuple(float(v) for v in m.double().cpu().numpy()))
    gate(f"prepared {dtype}, theta overwritten", res.cpu().numpy(), grad.cpu().numpy(), ref)


@pytest.mark.parametrize("model", ["dense-flow", "dense-flow-voxel"])
def test_flow_models(model):
    voxel = model == "dense-flow-voxel"
    ev = uniform_events()
    if voxel:
        motion = f32(np.stack([E.utils.generate_smooth_flow(SIZE, 6, seed=11 + t) for t in range(T_BINS)]))
    else:
        motion = f32(E.utils.generate_smooth_flow(SIZE, 6, seed=11))
    h = E.CMaxHandle(SIZE).set_events(ev, time_bin=T_BINS if voxel else 0)
    res, grad = h.evaluate(E.make_descriptor("image_variance", model, time_bin=T_BINS if voxel else 0), motion)
    r = orc.objective(ev, motion, model, SIZE, cost="image_variance", sigma=0)
    gate(model, res.cpu().numpy(), grad.double().cpu().numpy(), (r["loss"], r["grad"]))
    h.close()


@pytest.mark.parametrize("weights", ["ones", "uniform"])
def test_weighted_handle(weights):
    """Weights of one everywhere run the weighted kernels against oracle.objective itself; varying weights go against the oracle's own
    steps with the weight applied where the reference applies it (tests/_weighted_ref.py, equal to oracle.objective at w = 1:
    tests/test_weights_host.py)."""
    ev = uniform_events()
    w = np.ones(ev.shape[0]) if weights == "ones" else np.random.default_rng(5).uniform(0.2, 3.0, ev.shape[0])
    h = E.CMaxHandle(SIZE).set_events(ev, weights=w)
    assert h.weighted
    res, grad = h.evaluate(E.make_descriptor("image_variance", MODEL), np.array(THETA))
    if weights == "ones":
        ref = reference("uniform", THETA)
    else:
        r = weighted_objective(ev, np.asarray(THETA), MODEL, SIZE, w, cost="image_variance", sigma=0)
        ref = (r["loss"], r["grad"])
    gate(f"weights {weights}", res.cpu().numpy(), grad.cpu().numpy(), ref)
    h.close()


def test_graph_capture_replayed_twice(handle):
    """One evaluation captured, replayed twice.  The handle's vote images are double-buffered -- an evaluation clears the image of the
    next one -- so the captured evaluation finds its image clear again after any one other evaluation: an eager call sits between the
    two replays (it is held to the oracle as well)."""
    m = dev(np.asarray(THETA))
    call, res, grad = handle.prepare(E.make_descriptor("image_variance", MODEL), m)
    ref = reference("uniform", THETA)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for label in ("first replay", "eager", "second replay"):
        res.zero_()
        grad.zero_()
        if label == "eager":
            call()
        else:
            g.replay()
        torch.cuda.synchronize()
        gate(f"graph, {label}", res.cpu().numpy(), grad.cpu().numpy(), ref)
