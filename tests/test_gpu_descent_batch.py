"""Multi-start descent (cmax_objective_descend_batch; k_finish_raw_step_batch of csrc/cmax_fused.hip): K independent SGD / Adam
trajectories of a 2-DoF objective per library call, with tests/test_gpu_descent.py's method and gates -- the bookkeeping exact per candidate,
and every traced iterate of every candidate held to the fp64 reference (loss, gradient) there (tests/_hvp_ref.py, tests/_weighted_ref.py on
the weighted handle):
  SGD   step error <= lr_it 1e-4 |g_ref|inf / (1 - momentum): linear in g, the project's 1e-4 gradient gate carried through the momentum sum;
  Adam  once the reference gradient's entries are within a factor 4 of each other (asserted; the table of starts keeps them within 3 on the
        CPU, tests/test_descent_batch_reference.py), every entry of the step within 2e-3 |expected step| + 1e-12: the gate gives 4e-4 per
        entry, the step carries the error of m plus half that of v;
  loss history within 1e-4 relative.
Which path ran is read off the workspace: the shared-launch path allocates cmax_objective_batch's workspace for K candidates (at least the
two sets of K x n_ref vote images), the candidate-by-candidate path allocates the descent state and nothing else.  Every figure is printed
before it is asserted.  No non-finite or absurd theta is sent anywhere: the stop rule's device code is shared with the single-start kernels
and covered there."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import event_based_optical_flow_amd as E  # noqa: E402
from event_based_optical_flow_amd import _lib, solver  # noqa: E402
from event_based_optical_flow_amd.solver import common  # noqa: E402
from event_based_optical_flow_amd.solver import translation_search as ts  # noqa: E402

import _descent_batch_cases as B  # noqa: E402
import _descent_ref  # noqa: E402
from _weighted_ref import weighted_objective  # noqa: E402

N_ITER, SIZE = B.N_ITER, B.SIZE


def state_bytes(K, n_iter=N_ITER, trace=True):
    """include/cmax_hip.h, cmax_objective_descend_batch: the handle-owned descent state."""
    return 8 * K * (32 + n_iter + (2 * (n_iter + 1) if trace else 0))


def image_bytes(K, n_ref=1):
    """A lower bound of cmax_objective_batch's workspace for K candidates: its two sets of K x n_ref fp32 vote images, without padding."""
    return 2 * K * n_ref * SIZE[0] * SIZE[1] * 4


def weights(n):
    return np.random.default_rng(5).uniform(0.5, 1.0, n)


def weighted_reference(theta, cost="image_variance", sigma=0):
    ev = B.events()
    out = weighted_objective(ev, np.asarray(theta), "2d-translation", SIZE, weights(len(ev)), cost=cost, sigma=sigma)
    return float(out["loss"]), np.asarray(out["grad"], dtype=np.float64).reshape(-1)


def setup(cost="image_variance", sigma=0, weighted=False, deterministic=False):
    h = E.CMaxHandle(SIZE)
    if deterministic:
        h.set_deterministic(True)
    h.set_events(B.events())
    if weighted:
        h.set_event_weights(torch.as_tensor(weights(len(B.events())), device="cuda"))
    obj = E.ContrastObjective(h, "2d-translation", cost=cost, sigma=sigma)
    h.evaluate(obj.terms[0][2], torch.tensor([0.5, -0.5], dtype=torch.float64, device="cuda"))  # (the evaluation's own lazy workspaces first)
    return h, obj


def check_bookkeeping(res, x0, n_iter=N_ITER, schedule=B.SCHEDULE):
    """What does not depend on the gradients (tests/test_gpu_descent.py::check_bookkeeping), for ONE candidate: its argmin is of its own history."""
    assert res.trace.shape == (n_iter + 1, 2) and res.loss_history.shape == (n_iter,)
    assert res.n_done == n_iter and np.isfinite(res.loss_history).all()
    np.testing.assert_array_equal(res.trace[0], x0)
    np.testing.assert_array_equal(res.x_last, res.trace[n_iter])
    best, best_it = _descent_ref.best_of(res.loss_history)
    assert res.best_iter == best_it == int(np.argmin(res.loss_history)) and res.best_loss == best
    np.testing.assert_array_equal(res.x_best, res.trace[best_it])
    assert res.last_lr == _descent_ref.learning_rate(n_iter - 1, dict(lr=schedule["lr"], lr_step=schedule["lr_step"], lr_decay=schedule["lr_decay"]))


def check_against_reference(label, results, starts, mid, reference=B.reference, n_iter=N_ITER):
    """Every candidate, every iteration: bookkeeping, then the step and the loss against the fp64 reference at the traced iterate."""
    assert len(results) == len(starts)
    opt = B.ref_options(mid)
    worst_step = worst_loss = worst_ratio = 0.0
    for z, (res, x0) in enumerate(zip(results, starts)):
        check_bookkeeping(res, x0, n_iter)
        state = {}
        for it in range(n_iter):
            loss_ref, g_ref = reference(res.trace[it])
            expected = _descent_ref.step(state, res.trace[it], g_ref, it, opt)
            e_loss = abs(res.loss_history[it] - loss_ref) / abs(loss_ref)
            worst_loss = max(worst_loss, e_loss)
            if mid == "sgd":
                tol = _descent_ref.learning_rate(it, opt) * B.GRAD_TOL * np.abs(g_ref).max() / (1.0 - B.MOMENTUM)
                err = np.abs(res.trace[it + 1] - expected).max()
                worst_step = max(worst_step, err / tol)
                if err > tol or e_loss > B.GRAD_TOL:
                    print(f"[descent-batch] {label} candidate {z} it {it}: theta {res.trace[it]}, g_ref {g_ref}, step error {err:.3e} (bound {tol:.3e}), loss rel err {e_loss:.2e}")
                assert err <= tol, (label, z, it, err, tol)
            else:
                ratio = np.abs(g_ref).max() / np.abs(g_ref).min()
                step, want = res.trace[it + 1] - res.trace[it], expected - res.trace[it]
                err = np.abs(step - want)
                worst_ratio = max(worst_ratio, ratio)
                worst_step = max(worst_step, (err / (2e-3 * np.abs(want) + 1e-12)).max())
                if ratio > 4.0 or (err > 2e-3 * np.abs(want) + 1e-12).any() or e_loss > B.GRAD_TOL:
                    print(f"[descent-batch] {label} candidate {z} it {it}: theta {res.trace[it]}, g_ref {g_ref} (ratio {ratio:.2f}), step {step}, expected {want}, loss rel err {e_loss:.2e}")
                assert ratio <= 4.0, (label, z, it, ratio)
                assert (err <= 2e-3 * np.abs(want) + 1e-12).all(), (label, z, it, step, want)
            assert e_loss <= B.GRAD_TOL, (label, z, it, e_loss)
    extra = f", worst gradient ratio {worst_ratio:.2f}" if mid == "adam" else ""
    print(f"[descent-batch] {label}: {len(starts)} candidates x {n_iter} iterations, worst step error {worst_step:.3f} of its bound, worst loss rel err {worst_loss:.2e}{extra}")


def _bytes(res):
    return (res.x_best.tobytes(), res.x_last.tobytes(), res.loss_history.tobytes(), res.trace.tobytes(), res.best_loss, res.best_iter, res.n_done, res.last_lr)


# ---- 1. the shared-launch path, SGD ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 5, 64])
def test_fast_path_sgd(K):
    """64 distinct starts: a wrong candidate stride or a shared control block cannot pass.  The path is read off the workspace: on a handle
    that never ran a batch the call must have allocated cmax_objective_batch's workspace for K candidates besides its own state."""
    h, obj = setup()
    starts = B.sgd_starts(K)
    before = h.workspace_bytes
    results = obj.descend_batch(starts, trace=True, **B.SCHEDULE, **B.METHODS["sgd"])
    grown = h.workspace_bytes - before
    print(f"[descent-batch] sgd K {K}: workspace grew by {grown} bytes, {state_bytes(K)} of them the descent state, at least {image_bytes(K)} expected for the batch")
    assert grown - state_bytes(K) >= image_bytes(K)  # the shared-launch path ran
    check_against_reference(f"fast sgd K {K}", results, starts, "sgd")
    assert len({r.trace.tobytes() for r in results}) == K  # K distinct trajectories
    h.close()


# ---- 2. the shared-launch path, Adam --------------------------------------------------------------------------------------------------------
def test_fast_path_adam():
    h, obj = setup()
    before = h.workspace_bytes
    results = obj.descend_batch(B.ADAM_STARTS, trace=True, **B.SCHEDULE, **B.METHODS["adam"])
    assert h.workspace_bytes - before - state_bytes(9) >= image_bytes(9)  # the shared-launch path ran
    check_against_reference("fast adam K 9", results, B.ADAM_STARTS, "adam")
    # without a trace: the same numbers at run-to-run accuracy (fp32 atomics), the smaller state fits into the buffer that is there
    before = h.workspace_bytes
    quiet = obj.descend_batch(B.ADAM_STARTS, **B.SCHEDULE, **B.METHODS["adam"])
    assert h.workspace_bytes == before and all(q.trace is None for q in quiet)
    e = max(np.abs(q.loss_history - r.loss_history).max() / np.abs(r.loss_history).max() for q, r in zip(quiet, results))
    print(f"[descent-batch] adam without a trace: loss histories differ by {e:.2e}")
    assert e <= 1e-5
    h.close()


# ---- 3. independence of the control blocks --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mid", list(B.METHODS))
def test_candidates_are_independent(mid):
    """Every candidate's best_iter / best_loss follow its OWN history (check_bookkeeping, per candidate), and the table reversed returns every
    start's result at the reversed index: held to the same reference by the same bound, and printed against the first run."""
    h, obj = setup()
    starts = B.ADAM_STARTS
    fwd = obj.descend_batch(starts, trace=True, **B.SCHEDULE, **B.METHODS[mid])
    rev = obj.descend_batch(starts[::-1].copy(), trace=True, **B.SCHEDULE, **B.METHODS[mid])
    print(f"[descent-batch] {mid}: best_iter per candidate {[r.best_iter for r in fwd]}, reversed run {[r.best_iter for r in rev[::-1]]}")
    check_against_reference(f"independence {mid} forward", fwd, starts, mid)
    check_against_reference(f"independence {mid} reversed", rev[::-1], starts, mid)
    d_x = max(np.abs(a.trace - b.trace).max() for a, b in zip(fwd, rev[::-1]))
    d_l = max(np.abs(a.loss_history - b.loss_history).max() / np.abs(a.loss_history).max() for a, b in zip(fwd, rev[::-1]))
    print(f"[descent-batch] {mid}: forward vs reversed table, largest difference of an iterate {d_x:.3e}, of a loss {d_l:.2e} relative")
    assert len({r.best_loss for r in fwd}) == len(starts)  # nine histories, nine minima
    h.close()


# ---- 4. the candidate-by-candidate path ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mid", list(B.METHODS))
@pytest.mark.parametrize("cost,sigma", [("image_variance", 0), ("normalized_gradient_magnitude", 1)], ids=["variance", "normalized-gm"])
def test_general_path_equals_single_calls_on_a_deterministic_handle(cost, sigma, mid):
    """Bit-repeatable, so `descend_batch` must return bit for bit what K `descend` calls return: trace, history, result block."""
    h, obj = setup(cost, sigma, deterministic=True)
    starts = B.ADAM_STARTS[:3]
    singles = [obj.descend(s, trace=True, **B.SCHEDULE, **B.METHODS[mid]) for s in starts]
    before = h.workspace_bytes
    batch = obj.descend_batch(starts, trace=True, **B.SCHEDULE, **B.METHODS[mid])
    assert h.workspace_bytes - before == state_bytes(3)  # the descent state and nothing else: candidate by candidate
    for z, (one, got) in enumerate(zip(singles, batch)):
        check_bookkeeping(got, starts[z])
        assert _bytes(got) == _bytes(one), (cost, mid, z)
    again = obj.descend_batch(starts, trace=True, **B.SCHEDULE, **B.METHODS[mid])
    assert [_bytes(r) for r in again] == [_bytes(r) for r in batch]
    print(f"[descent-batch] deterministic {cost} {mid}: 3 starts, batch == single calls bit for bit; moved {max(np.abs(r.x_last - s).max() for r, s in zip(batch, starts)):.3e}")
    h.close()


@pytest.mark.parametrize("mid", list(B.METHODS))
def test_one_start_on_a_default_handle(mid):
    """K = 1 runs as cmax_objective_descend runs (the single-start finishing kernel); no batch workspace is allocated."""
    h, obj = setup()
    before = h.workspace_bytes
    results = obj.descend_batch(B.ADAM_STARTS[:1], trace=True, **B.SCHEDULE, **B.METHODS[mid])
    assert h.workspace_bytes - before == state_bytes(1)
    check_against_reference(f"K 1 {mid}", results, B.ADAM_STARTS[:1], mid)
    h.close()


@pytest.mark.parametrize("mid", list(B.METHODS))
def test_weighted_handle(mid):
    """Per-event weights: the general K1 -> statistics -> K3 sequence and the update launch behind it, candidate by candidate."""
    h, obj = setup(weighted=True)
    starts = B.ADAM_STARTS[:3]
    before = h.workspace_bytes
    results = obj.descend_batch(starts, trace=True, **B.SCHEDULE, **B.METHODS[mid])
    assert h.workspace_bytes - before == state_bytes(3)
    check_against_reference(f"weighted {mid}", results, starts, mid, reference=weighted_reference)
    h.close()


# ---- 5. state hygiene ---------------------------------------------------------------------------------------------------------------------
def rel_max(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max()


def test_state_hygiene():
    """cmax_objective_batch shares its double-buffered workspace with the multi-start descent: evaluations of 8 fixed candidates before,
    between and after three descents (K 5 x 6 iterations; K 3 x 5, whose odd count flips the buffer parity; K 16) agree with the fp64 reference
    and with each other at run-to-run accuracy, and so do a single-start `descend` and an `evaluate`.  Every observation also takes the two
    host paths, which share one pinned block with the descents: an `evaluate_host` whose results are copied (a dense flow's gradient) and,
    directly behind it, one whose results are polled (the 2-DoF objective), each against `evaluate` of the same motion at the same run-to-run
    bounds.  The state buffer grows by exactly what the header documents, and only when a call needs more than is there."""
    h, obj = setup()
    desc = obj.terms[0][2]
    fixed = torch.tensor(B.sgd_starts(64)[3::8].copy(), dtype=torch.float64, device="cuda")  # 8 of the 8 x 8 grid
    theta1 = torch.tensor([1.5, -2.5], dtype=torch.float64, device="cuda")
    refs = [B.reference(t) for t in fixed.cpu().numpy()]
    ref_loss, ref_grad = np.array([r[0] for r in refs]), np.stack([r[1] for r in refs])

    dense = E.ContrastObjective(h, "dense-flow", cost="image_variance").terms[0][2]
    rows, cols = torch.meshgrid(torch.arange(SIZE[0], dtype=torch.float32), torch.arange(SIZE[1], dtype=torch.float32), indexing="ij")
    flow = torch.stack([3.0 + 0.02 * rows - 0.01 * cols, -2.0 + 0.015 * cols]).cuda()  # [2, H, W], a few pixels over the batch

    def observe():
        results, grads = h.evaluate_batch(desc, fixed)
        r1, g1 = h.evaluate(desc, theta1)
        rd, gd = h.evaluate(dense, flow)
        # the host paths share the handle's pinned block with both descents: a copied result whose payload (the flow gradient, 17920
        # bytes) is far longer than the block's head, and IMMEDIATELY behind it a polled one, which waits on the run counter in that head
        hd, hgd = h.evaluate_host(dense, flow)
        hp, hgp = h.evaluate_host(desc, theta1)
        e_copy = abs(hd[0] - rd[0].item()) / abs(rd[0].item()), rel_max(hgd, gd.cpu().numpy())
        e_poll = abs(hp[0] - r1[0].item()) / abs(r1[0].item()), rel_max(hgp, g1.cpu().numpy())
        print(f"[descent-batch] hygiene, evaluate_host vs evaluate: copied (dense flow) loss {e_copy[0]:.2e} grad {e_copy[1]:.2e}; "
              f"polled (2-DoF) behind it loss {e_poll[0]:.2e} grad {e_poll[1]:.2e}")
        assert hgd.shape == (2,) + SIZE and hgd.dtype == np.float32 and hgp.shape == (2,) and hgp.dtype == np.float64
        assert e_copy[0] <= 1e-6 and e_copy[1] <= 1e-5
        assert e_poll[0] <= 1e-6 and e_poll[1] <= 1e-5
        one = obj.descend(B.ADAM_STARTS[0], trace=True, **B.SCHEDULE, **B.METHODS["sgd"])
        return results[:, 0].cpu().numpy(), grads.cpu().numpy(), float(r1[0].item()), g1.cpu().numpy(), one

    h.evaluate_batch(desc, torch.zeros((16, 2), dtype=torch.float64, device="cuda"))  # the batch workspace at its final size
    seen = [observe()]
    base = h.workspace_bytes
    sizes = []
    for K, n_iter in ((5, 6), (3, 5), (16, 6)):
        starts = B.sgd_starts(16)[:K]
        results = obj.descend_batch(starts, trace=True, **dict(B.SCHEDULE, n_iter=n_iter), **B.METHODS["sgd"])
        check_against_reference(f"hygiene K {K} n_iter {n_iter}", results, starts, "sgd", n_iter=n_iter)
        sizes.append(h.workspace_bytes - base)
        seen.append(observe())
    print(f"[descent-batch] hygiene: state bytes after K 5 / K 3 / K 16: {sizes}")
    assert sizes == [state_bytes(5), state_bytes(5), state_bytes(16)]  # a smaller K (and n_iter) allocates nothing
    obj.descend_batch(B.sgd_starts(5), **B.SCHEDULE, **B.METHODS["adam"])
    assert h.workspace_bytes - base == state_bytes(16)
    loss0, grad0, l1_0, g1_0, one0 = seen[0]
    for i, (loss, grad, l1, g1, one) in enumerate(seen):
        e_ref = (np.abs(loss - ref_loss) / np.abs(ref_loss)).max(), max(rel_max(grad[k], ref_grad[k]) for k in range(8))
        e_run = (np.abs(loss - loss0) / np.abs(loss0)).max(), max(rel_max(grad[k], grad0[k]) for k in range(8))
        e_one = abs(l1 - l1_0) / abs(l1_0), rel_max(g1, g1_0)
        print(f"[descent-batch] hygiene, observation {i}: 8 candidates vs fp64 loss {e_ref[0]:.2e} grad {e_ref[1]:.2e}; vs observation 0 loss {e_run[0]:.2e} "
              f"grad {e_run[1]:.2e}; evaluate vs observation 0 loss {e_one[0]:.2e} grad {e_one[1]:.2e}")
        assert max(e_ref) <= 1e-4
        assert e_run[0] <= 1e-6 and e_run[1] <= 1e-5
        assert e_one[0] <= 1e-6 and e_one[1] <= 1e-5
        check_against_reference(f"hygiene, single-start descend {i}", [one], B.ADAM_STARTS[:1], "sgd")
    h.close()


# ---- 6. time slabs ------------------------------------------------------------------------------------------------------------------------
def test_time_slabs():
    """The batch in two time slabs (another work list, the same kernels).  Which path runs follows deferred_applies on that work list and
    is not asserted here: the workspace growth is printed."""
    h, obj = setup()
    h.set_time_slabs(2)
    starts = B.sgd_starts(5)
    before = h.workspace_bytes
    results = obj.descend_batch(starts, trace=True, **B.SCHEDULE, **B.METHODS["sgd"])
    print(f"[descent-batch] time slabs: workspace grew by {h.workspace_bytes - before} bytes ({state_bytes(5)} of them the descent state)")
    assert h.time_slabs == 2
    check_against_reference("2 time slabs, sgd K 5", results, starts, "sgd")
    h.close()


# ---- 7. the solver side ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    h, obj = setup()
    with pytest.raises(ValueError, match=r"\[K, 2\]"):
        obj.descend_batch(np.zeros(3))
    dense = E.ContrastObjective(h, "dense-flow", cost="image_variance")
    with pytest.raises(NotImplementedError, match="2-DoF"):
        dense.descend_batch(np.zeros((2, 2)))
    hybrid = E.ContrastObjective(h, "2d-translation", cost="hybrid", cost_with_weight={"image_variance": 1.0, "gradient_magnitude": 0.5})
    with pytest.raises(NotImplementedError, match="ONE fused term"):
        hybrid.descend_batch(np.zeros((2, 2)))
    bad = _lib.CmaxObjective.from_buffer_copy(dense.terms[0][2])
    with pytest.raises(_lib.CmaxError, match="2-DoF descriptors only"):
        h.descend_batch(bad, np.zeros((2, 2)), _lib.descent_descriptor("Adam", n_iter=3))
    assert obj.descend_batch(np.zeros((0, 2))) == []
    many = obj.descend_batch(np.tile(B.ADAM_STARTS, (8, 1))[:70], n_iter=2)  # 70 starts: calls of 64 and 6
    assert len(many) == 70 and all(r.n_done == 2 for r in many)
    e = max(abs(many[k].loss_history[0] - many[k + 63].loss_history[0]) / abs(many[k].loss_history[0]) for k in range(7))  # the same start in both calls
    print(f"[descent-batch] 70 starts in two calls: equal starts across the calls differ by {e:.2e} in their first loss")
    assert e <= 1e-6
    h.close()


def test_whole_image_guess_with_refinement():
    """Start 0 is the grid's own pick and iteration 0 evaluates it, so the refined guess cannot be worse than the pick -- up to the
    run-to-run accuracy of two evaluations -- and on a batch whose motion lies between grid points it leaves the grid."""
    H, W = SIZE
    ev = E.utils.generate_structured_events(4000, H, W, (4.2, -2.7), n_dots=12, tmin=0.0, tmax=0.05, seed=21)
    ev = np.ascontiguousarray(ev[np.argsort(ev[:, 2], kind="stable")])
    t_scale = float(ev[:, 2].max() - ev[:, 2].min())
    h = E.CMaxHandle(SIZE).set_events(ev)
    cost = dict(cost="image_variance", cost_with_weight=None, sigma=0)
    pick, grid_loss = common.whole_image_guess(h, t_scale, **cost)
    guess, grid_loss2, results = common.whole_image_guess(h, t_scale, refine=dict(top_k=4, n_iter=20, method="Adam", lr=0.05), **cost)
    assert len(results) == 4 and all(isinstance(r, _lib.DescentResult) and r.n_done == 20 for r in results)
    np.testing.assert_allclose(results[0].loss_history[0], grid_loss.min(), rtol=1e-6)  # start 0 is the grid's pick
    loss_guess, loss_pick = ts.candidate_losses(h, np.stack([guess, pick]), t_scale, **cost)
    print(f"[descent-batch] global-best: grid pick {pick} (loss {loss_pick:.8g}) -> refined {guess} (loss {loss_guess:.8g}); per start "
          f"{[(r.best_iter, round(r.best_loss, 6)) for r in results]}; motion of the batch {np.array([4.2, -2.7]) / t_scale}")
    assert loss_guess <= loss_pick + 1e-6 * abs(loss_pick)
    assert np.abs(guess - pick).max() > 0.0 and np.abs(guess / 10.0 - np.round(guess / 10.0)).max() > 1e-6  # off the grid
    h.close()


PARAMS = {"trans_x": {"min": -150, "max": 150}, "trans_y": {"min": -150, "max": 150}}
COMMON = {"motion_model": "2d-translation", "warp_direction": "first", "parameters": ["trans_x", "trans_y"], "cost": "hybrid", "outer_padding": 0,
          "cost_with_weight": {"multi_focal_normalized_gradient_magnitude": 1.0, "total_variation": 0.01},
          "iwe": {"method": "bilinear_vote", "blur_sigma": 1}}
OPT_CFG = {"n_iter": 5, "method": "Adam", "max_iter": 25, "parameters": PARAMS}
SOLVER_SIZE = (66, 90)


def _pyramid(refine=None):
    patch = {"initialize": "global-best", "scale": 3, "crop_height": 64, "crop_width": 80, "filter_type": "bilinear"}
    if refine:
        patch["global_best_refine"] = refine
    cfg = dict(COMMON, method="pyramidal_patch_contrast_maximization", time_aware=False, patch=patch)
    slv = solver.collections["pyramidal_patch_contrast_maximization"](SOLVER_SIZE, {}, cfg, dict(OPT_CFG), {}, None)
    slv._handle = E.CMaxHandle(SOLVER_SIZE).set_keep_outside(False).set_deterministic(True)  # bit-repeatable: the comparisons below are exact
    return slv


def test_solver_without_and_with_the_key(monkeypatch):
    """Without patch.global_best_refine the solver makes no descend_batch call and two instances agree bit for bit (a deterministic
    handle); with it, the refined guess is what the coarsest scale starts from."""
    H, W = SOLVER_SIZE
    ev = E.utils.generate_structured_events(6000, H, W, (4.2, -2.7), n_dots=40, tmin=0.0, tmax=0.05, seed=22)
    ev = np.ascontiguousarray(ev[np.argsort(ev[:, 2], kind="stable")])
    calls = []
    real = E.CMaxHandle.descend_batch
    monkeypatch.setattr(E.CMaxHandle, "descend_batch", lambda self, *a, **kw: calls.append(len(a[1])) or real(self, *a, **kw))
    plain = []
    for _ in range(2):
        slv = _pyramid()
        plain.append(slv.optimize(ev))
        assert len(slv.search_history[0]) == 4 and slv.search_history[0][1] == "global-best"  # (scale, kind, losses, guess) as before
        plain_history = slv.search_history[0]
    assert calls == []
    for s in plain[0]:
        np.testing.assert_array_equal(plain[0][s], plain[1][s])
    slv = _pyramid({"top_k": 3, "n_iter": 10, "method": "Adam", "lr": 0.05})
    motion = slv.optimize(ev)
    s, kind, loss, guess, results = slv.search_history[0]
    pick, grid_min = plain_history[3], float(np.nanmin(loss))
    print(f"[descent-batch] pyramid with the key: grid pick {pick} (loss {grid_min:.8g}) -> {guess}; per start {[(r.best_iter, round(r.best_loss, 8)) for r in results]}")
    assert calls == [3] and kind == "global-best" and len(results) == 3 and sorted(motion) == sorted(plain[0])
    np.testing.assert_array_equal(loss, plain_history[2])  # the grid itself is the one the solver searched before
    # (total_variation is 0 for one translation: the fused term the descent steps on is the grid's loss; start 0 is the grid's pick)
    assert min(r.best_loss for r in results) <= grid_min + 1e-6 * abs(grid_min)
