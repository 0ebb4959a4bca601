"""dL/d(event) of the fused objective (cmax_objective_event_grad, CMaxHandle.evaluate_event_grad / events_grad, ContrastObjective(..., events=)):
against the fp64 references of tests/_event_grad_ref.py at the project's plain gate, max|delta| / max|ref| <= 1e-4 PER COLUMN, the
reference taken on the motion the device holds; `result` and `grad` of the same call at the same gate.

  grad_events [n, 3] and csum   against event_grad_objective (composed from the committed oracle; weighted or not)
  events_grad() [n, 4]          against events_grad_autograd (torch fp64 autograd, the reference's `events.grad`; unweighted)

No event is filtered: like the motion gradient the entry follows the cells K1 decided in fp64.  csum[k] is a sum over all events of
terms that each carry the gate's error, so it is held to 1e-4 of max(|csum_k|, sqrt(n) max_e |c_{e,k}|) -- the size a sum of n
independent roundings of that magnitude has; what it feeds, the time column of events_grad, is under the plain gate.
Measured errors are printed."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import event_based_optical_flow_amd as E  # noqa: E402
from event_based_optical_flow_amd import _lib  # noqa: E402
from event_based_optical_flow_amd import functional as F  # noqa: E402

import _event_grad_worker as W  # noqa: E402
from _event_grad_ref import event_grad_objective, events_grad_autograd  # noqa: E402
from _weighted_ref import weight_set  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
SIZE = (40, 56)
COSTS = ["image_variance", "gradient_magnitude", "normalized_image_variance", "normalized_gradient_magnitude",
         "multi_focal_normalized_image_variance", "multi_focal_normalized_gradient_magnitude"]
MODELS = [("2d-translation", 0), ("dense-flow", 0), ("dense-flow-voxel", 2), ("dense-flow-voxel", 5)]
MODEL_IDS = ["2dof", "dense", "voxel2", "voxel5"]


def f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def rel_max(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def motion_for(model, size, T=0, seed=11, mag=8):
    if model == "2d-translation":
        return np.array([7.3, -4.1])
    if model == "dense-flow":
        return f32(E.utils.generate_smooth_flow(size, mag, seed=seed))
    return f32(np.stack([E.utils.generate_smooth_flow(size, mag, seed=seed + t) for t in range(T)]))


def gate(tag, got, ref, n_ref=1):
    res, grad, ge, csum = got
    ge, csum = np.asarray(ge.double().cpu()), np.asarray(csum.cpu())
    e = [abs(res[0].item() - ref["loss"]) / abs(ref["loss"]), rel_max(grad.double().cpu().numpy(), ref["grad"])]
    e += [rel_max(ge[:, c], ref["grad_events"][:, c]) for c in range(3)]
    n = max(ge.shape[0], 1)
    cs = np.abs(csum - ref["csum"]).max() / max(np.abs(ref["csum"]).max(), np.sqrt(n) * np.abs(ref["grad_events"][:, 2]).max() / n_ref, 1e-300)
    print(f"[event grad] {tag}: rel err loss {e[0]:.2e} grad {e[1]:.2e} x {e[2]:.2e} y {e[3]:.2e} C {e[4]:.2e} csum {cs:.2e}")
    assert max(e) <= TOL and cs <= TOL, (tag, e, cs)
    assert (csum[n_ref:] == 0).all()


def check_case(tag, h, ev, w, model, size, cost, sigma, pad=0, T=0, full=None, **kw):
    """full: also events_grad() [n, 4] against autograd (unweighted handles; default: whenever w is 1.0)."""
    motion = kw.pop("motion", None)
    motion = motion_for(model, size, T) if motion is None else motion
    desc = E.make_descriptor(cost, model, sigma=sigma, time_bin=T, **kw)
    ref = event_grad_objective(ev, motion, model, size, w, cost=cost, sigma=sigma, outer_padding=pad, **kw)
    got = h.evaluate_event_grad(desc, motion)
    gate(tag, got, ref, desc.n_ref)
    if full if full is not None else isinstance(w, float):
        _, want = events_grad_autograd(ev, motion, model, size, cost=cost, sigma=sigma, outer_padding=pad, **kw)
        g4 = h.events_grad(desc, motion).cpu().numpy()
        e = [rel_max(g4[:, c], want[:, c]) for c in range(3)]
        print(f"[event grad] {tag}: events.grad rel err x {e[0]:.2e} y {e[1]:.2e} t {e[2]:.2e}")
        assert max(e) <= TOL and (g4[:, 3] == 0).all(), (tag, e)
    return got, ref


def events(n, size=SIZE, seed=21):
    return E.utils.generate_events(n, size[0], size[1], 0.0, 0.05, seed=seed)


@pytest.mark.parametrize("n", [60, 2000, 30_000])
@pytest.mark.parametrize("model,T", MODELS, ids=MODEL_IDS)
def test_parity(model, T, n):
    """3 models (voxel T = 2 and 5) x 6 costs x sigma in {0, 1} x both directions per batch size."""
    ev = events(n)
    h = E.CMaxHandle(SIZE).set_events(ev, time_bin=T)
    for cost in COSTS:
        for sigma in (0, 1):
            for direction in ("minimize", "maximize"):
                check_case(f"{model} T {T} n {n} {cost} sigma {sigma} {direction}", h, ev, 1.0, model, SIZE, cost, sigma, T=T, direction=direction)
    h.close()


@pytest.mark.parametrize("wname", ["uniform", "polarity", "zeros"])
@pytest.mark.parametrize("model,T", MODELS[:3], ids=MODEL_IDS[:3])
def test_weighted_handles(model, T, wname):
    ev = events(30_000)
    w = weight_set(wname, ev, seed=31)
    h = E.CMaxHandle(SIZE).set_events(ev, time_bin=T, weights=w)
    for cost, sigma in (("image_variance", 0), ("gradient_magnitude", 1), ("normalized_image_variance", 1), ("multi_focal_normalized_gradient_magnitude", 0)):
        check_case(f"weighted {wname} {model} {cost} sigma {sigma}", h, ev, w, model, SIZE, cost, sigma, T=T)
    h.close()


def _off_sensor_batch(n=30_000):
    rng = np.random.default_rng(91)
    ev = events(n, seed=90)
    out = rng.random(ev.shape[0]) < 0.33
    ev[out, 0] = rng.uniform(-25.0, SIZE[0] + 25.0, int(out.sum()))
    ev[out, 1] = rng.uniform(-25.0, SIZE[1] + 25.0, int(out.sum()))
    off = (np.floor(ev[:, 0]) < 0) | (np.floor(ev[:, 0]) >= SIZE[0]) | (np.floor(ev[:, 1]) < 0) | (np.floor(ev[:, 1]) >= SIZE[1])
    ext = [int(np.argmin(ev[:, 2])), int(np.argmax(ev[:, 2]))]  # (the batch's time extremes stay on the sensor)
    off[ext] = False
    ev[ext, :2] = [[3.0, 4.0], [5.0, 6.0]]
    return ev, off


def test_dropped_events_keep_zero_rows():
    ev, off = _off_sensor_batch()
    assert off.sum() > 1000
    h = E.CMaxHandle(SIZE).set_keep_outside(False)
    h.set_events(ev, on_dropped="ignore")
    assert h.batch_info()["dropped"] == int(off.sum())
    motion = motion_for("dense-flow", SIZE)
    ref = event_grad_objective(ev[~off], motion, "dense-flow", SIZE, 1.0, cost="gradient_magnitude", sigma=1)
    res, grad, ge, csum = h.evaluate_event_grad(E.make_descriptor("gradient_magnitude", "dense-flow", sigma=1), motion)
    assert (ge[torch.from_numpy(off).cuda()] == 0).all()
    gate("dropped events", (res, grad, ge[torch.from_numpy(~off).cuda()], csum), ref)
    h.close()


@pytest.mark.parametrize("pad", [0, 6])
def test_kept_off_sensor_events_two_dof(pad):
    ev, off = _off_sensor_batch()
    h = E.CMaxHandle(SIZE, outer_padding=pad).set_keep_outside(True).set_events(ev, on_dropped="ignore")
    assert h.batch_info()["outside"] == int(off.sum()) and h.batch_info()["fractional"]
    theta = np.array([17.0, -21.0])
    for cost, sigma in (("image_variance", 0), ("normalized_gradient_magnitude", 1)):
        check_case(f"kept off-sensor events, pad {pad}, {cost}", h, ev, 1.0, "2d-translation", SIZE, cost, sigma, pad=pad, motion=theta)
    with pytest.raises(_lib.CmaxError):  # dense models stay refused on such a batch
        h.evaluate_event_grad(E.make_descriptor("image_variance", "dense-flow"), np.zeros((2,) + SIZE, np.float32))
    h.close()


@pytest.mark.parametrize("model,T", MODELS[:3], ids=MODEL_IDS[:3])
def test_kernel_branches(model, T):
    """Fractional sources with padding 3, omit_boundary=False and maximize, reference times middle / last / 0.3, normalize_t=False.  The
    fractions are seeded uniform in [0.001, 0.998]: an un-warped event is never within fp32 rounding of a cell border."""
    rng = np.random.default_rng(101)
    ev = events(30_000, seed=102)
    ev[:, 0] = np.floor(ev[:, 0]) + rng.uniform(0.001, 0.998, ev.shape[0])
    ev[:, 1] = np.floor(ev[:, 1]) + rng.uniform(0.001, 0.998, ev.shape[0])
    h = E.CMaxHandle(SIZE, outer_padding=3).set_events(ev, time_bin=T)
    assert h.batch_info()["fractional"]
    check_case(f"{model} frac pad 3", h, ev, 1.0, model, SIZE, "gradient_magnitude", 1, pad=3, T=T)
    check_case(f"{model} frac pad 3 no omit maximize", h, ev, 1.0, model, SIZE, "normalized_image_variance", 1, pad=3, T=T, omit_boundary=False, direction="maximize")
    check_case(f"{model} frac pad 3 multi-focal maximize", h, ev, 1.0, model, SIZE, "multi_focal_normalized_image_variance", 0, pad=3, T=T, direction="maximize")
    for wd in ("middle", "last", 0.3):
        check_case(f"{model} frac pad 3 reference time {wd}", h, ev, 1.0, model, SIZE, "image_variance", 0, pad=3, T=T, warp_direction=wd)
    if model != "dense-flow-voxel":
        m = f32(motion_for(model, SIZE) / 0.05)
        for cost in ("image_variance", "multi_focal_normalized_image_variance"):  # csum routes dL/dt through t.min() / t.max() here
            check_case(f"{model} frac pad 3 normalize_t False {cost}", h, ev, 1.0, model, SIZE, cost, 1, pad=3, normalize_t=False, motion=m)
    h.close()


@pytest.mark.parametrize("model", ["2d-translation", "dense-flow"])
def test_clipped_window(model):
    """150 px over the batch on 130 x 173: corners outside the LDS window are read from global memory; with and without time slabs."""
    size = (130, 173)
    ev = events(120_000, size, seed=61)
    motion = np.array([150.0, -140.0]) if model == "2d-translation" else f32(E.utils.generate_smooth_flow(size, 150, grid=3, seed=62))
    h = E.CMaxHandle(size).set_events(ev)
    check_case(f"clipped window {model}", h, ev, 1.0, model, size, "image_variance", 0, motion=motion)
    check_case(f"clipped window {model} normalised", h, ev, 1.0, model, size, "normalized_gradient_magnitude", 1, motion=motion)
    h.set_time_slabs(4)
    check_case(f"clipped window {model}, 4 slabs", h, ev, 1.0, model, size, "image_variance", 0, motion=motion)
    h.close()


def test_reorderings():
    ev = events(30_000, seed=61)
    w = weight_set("zeros", ev, seed=62)
    h = E.CMaxHandle(SIZE).set_events(ev, weights=w)
    h.set_time_slabs(4)
    check_case("4 slabs, dense", h, ev, w, "dense-flow", SIZE, "gradient_magnitude", 1)
    check_case("4 slabs, 2-DoF", h, ev, w, "2d-translation", SIZE, "normalized_image_variance", 0)
    h.set_time_bins(5)
    check_case("binned, voxel", h, ev, w, "dense-flow-voxel", SIZE, "image_variance", 0, T=5)
    check_case("binned, dense", h, ev, w, "dense-flow", SIZE, "multi_focal_normalized_gradient_magnitude", 1)
    h.set_time_bins(0)
    check_case("un-binned again", h, ev, w, "dense-flow", SIZE, "image_variance", 1)
    h.close()


@pytest.mark.parametrize("which,env", [("small", {"CMAX_BIG_SEG": "1"}), ("small", {"CMAX_BIG_SEG": "1", "CMAX_COMPACT": "0"}), ("small", {"CMAX_MID_SEG": "1"}),
                                       ("mid", {"CMAX_MID_SEG": "1"})], ids=["big", "big-uncompacted", "mid-30000", "mid"])
def test_forced_segment_layouts(which, env, tmp_path):
    """b512 (with and without the compact event copy) and m512, each in a child process of its own (tests/_event_grad_worker.py).  The
    30 000-event batch takes big segments when told to; mid segments are only ever cut from a batch of at least 256 full segments, so
    CMAX_MID_SEG=1 is run on the 30 000-event case (where it must change nothing) AND on the batch that gets the m512 layout."""
    e = dict(os.environ)
    for name in ("CMAX_BIG_SEG", "CMAX_MID_SEG", "CMAX_COMPACT"):
        e.pop(name, None)
    e.update(env)
    out = str(tmp_path / "got.npz")
    p = subprocess.run(["timeout", "-k", "10", "100", sys.executable, os.path.join(ROOT, "tests", "_event_grad_worker.py"), which, out], env=e, cwd=ROOT,
                       capture_output=True, text=True)
    assert p.returncode == 0, f"{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    got = dict(np.load(out))
    assert int(got["segment_events"]) == (4088 if "CMAX_BIG_SEG" in env else 3064 if which == "mid" else 2040)
    ev, size = W.batch(which)
    for model, cost, sigma in W.CASES:
        ref = event_grad_objective(ev, W.motion_for(model, size), model, size, 1.0, cost=cost, sigma=sigma)
        tag = f"{model}/{cost}"
        gate(f"{which} {env} {tag}", (torch.tensor([float(got[tag + '/loss'])]), torch.from_numpy(got[tag + "/grad"]), torch.from_numpy(got[tag + "/grad_events"]),
                                      torch.from_numpy(got[tag + "/csum"])), ref)


def test_empty_handle():
    h = E.CMaxHandle(SIZE).set_events(np.zeros((0, 4)))
    desc = E.make_descriptor("image_variance", "2d-translation")
    res, grad, ge, csum = h.evaluate_event_grad(desc, np.array([1.0, 2.0]))
    assert ge.shape == (0, 3) and res[0].item() == 0.0 and float(grad.abs().max()) == 0.0 and float(csum.abs().max()) == 0.0
    assert h.events_grad(desc, np.array([1.0, 2.0])).shape == (0, 4)
    h.close()


def test_result_and_grad_equal_evaluate():
    """`result` and `grad` against evaluate() on the same handle, to the run-to-run spread of fp32 atomics (1e-6 / 1e-5 as for dL/dw)."""
    ev = events(30_000)
    h = E.CMaxHandle(SIZE).set_events(ev)
    for model, cost, sigma in (("2d-translation", "image_variance", 0), ("dense-flow", "image_variance", 1), ("dense-flow", "normalized_image_variance", 0),
                               ("2d-translation", "multi_focal_normalized_gradient_magnitude", 1)):
        motion = motion_for(model, SIZE)
        desc = E.make_descriptor(cost, model, sigma=sigma)
        raw = h.has_raw(desc)
        r0, g0 = h.evaluate(desc, motion)
        r1, g1, _, _ = h.evaluate_event_grad(desc, motion)
        r2, g2 = h.evaluate(desc, motion)
        for r, g in ((r1, g1), (r2, g2)):
            assert abs(r[0].item() - r0[0].item()) <= 1e-6 * abs(r0[0].item()), (model, cost)
            assert rel_max(g.double().cpu().numpy(), g0.double().cpu().numpy()) <= 1e-5, (model, cost)
        assert h.has_raw(desc) == raw and not h.weighted
    h.close()


def test_two_fresh_handles_give_the_same_bits():
    """Behind the evaluation the entry adds nothing that depends on an order: the gather stores, the scatter sums the planes in index order,
    csum is a fixed tree.  The images it gathers from are K1's, flushed with fp32 atomics of multiples of 2^-20: those sums are exact --
    the same bits in any order -- while a pixel holds fewer than 16 events (2^24 units), and so are the fp64 statistics of a 40 x 56
    image (nine workgroups on eight lines: at most two commutative additions per line).  The 2000-event batch of the parity tests
    (0.9 events per pixel; asserted below 16) therefore must give the same bits on every fresh handle.  The 30 000-event batch has
    pixels above 16, where the image itself moves in its last bit from run to run: there the two handles agree to the spread
    tests/test_gpu_weight_grad.py allows for that noise (1e-5 of the largest entry)."""
    cases = (("2d-translation", 0, "multi_focal_normalized_image_variance", 0), ("dense-flow", 0, "gradient_magnitude", 1),
             ("dense-flow-voxel", 5, "normalized_image_variance", 0))
    for n in (2000, 30_000):
        ev = events(n)
        for model, T, cost, sigma in cases:
            motion = motion_for(model, SIZE, T)
            desc = E.make_descriptor(cost, model, sigma=sigma, time_bin=T)
            # the largest pixel of the raw (un-blurred) images of this case, every reference time and the un-warped image, from the reference
            peak = max(float(v.max()) for v in event_grad_objective(ev, motion, model, SIZE, 1.0, cost=cost, sigma=0)["iwes"].values())
            out = []
            for _ in range(2):
                h = E.CMaxHandle(SIZE).set_events(ev, time_bin=T)
                _, _, ge, csum = h.evaluate_event_grad(desc, motion)
                out.append((ge.cpu().numpy().copy(), csum.cpu().numpy().copy()))
                h.close()
            assert np.abs(out[0][0]).max() > 0
            if n == 2000:
                assert peak < 16.0, (model, cost, peak)
                assert np.array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32)), (model, cost)
                assert np.array_equal(out[0][1].view(np.uint64), out[1][1].view(np.uint64)), (model, cost)
            else:
                e = [rel_max(out[1][0][:, c], out[0][0][:, c]) for c in range(3)]
                print(f"[event grad] two fresh handles, {n} events {model} {cost}: largest pixel {peak:.1f}, rel diff x {e[0]:.1e} y {e[1]:.1e} C {e[2]:.1e}")
                assert max(e) <= 1e-5, (model, cost, e)


def test_public_interface():
    ev = events(30_000)
    th = np.array([7.3, -4.1])
    h = E.CMaxHandle(SIZE).set_events(ev)
    obj = E.ContrastObjective(h, "2d-translation", cost="normalized_gradient_magnitude", sigma=1)
    theta = torch.tensor(th, dtype=torch.float64, device="cuda", requires_grad=True)
    evt = torch.tensor(ev, dtype=torch.float64, device="cuda", requires_grad=True)
    loss = obj(theta, events=evt)
    loss.backward()
    ref_loss, want = events_grad_autograd(ev, th, "2d-translation", SIZE, cost="normalized_gradient_magnitude", sigma=1)
    ref = event_grad_objective(ev, th, "2d-translation", SIZE, 1.0, cost="normalized_gradient_magnitude", sigma=1)
    e = [abs(loss.item() - ref_loss) / abs(ref_loss), rel_max(theta.grad.cpu().numpy(), ref["grad"])] + [rel_max(evt.grad[:, c].cpu().numpy(), want[:, c]) for c in range(3)]
    print("[event grad] public interface: rel err loss %.2e grad %.2e x %.2e y %.2e t %.2e" % tuple(e))
    assert max(e) <= TOL and evt.grad.shape == (ev.shape[0], 4) and float(evt.grad[:, 3].abs().max()) == 0.0
    with pytest.raises(ValueError, match="handle's batch"):
        obj(theta, events=evt[:-1])
    # combined with weights=: all three leaves in one backward
    from _weight_grad_ref import weight_grad_objective

    wn = weight_set("zeros", ev, seed=131)
    w = torch.tensor(wn, dtype=torch.float64, device="cuda", requires_grad=True)
    theta.grad, evt.grad = None, None
    obj = E.ContrastObjective(h, "2d-translation", cost="image_variance")
    obj(theta, weights=w, events=evt).backward()
    ref = event_grad_objective(ev, th, "2d-translation", SIZE, wn, cost="image_variance")
    ref_w = weight_grad_objective(ev, th, "2d-translation", SIZE, wn, cost="image_variance")
    e = [rel_max(theta.grad.cpu().numpy(), ref["grad"]), rel_max(w.grad.cpu().numpy(), ref_w["grad_w"])] + [rel_max(evt.grad[:, c].cpu().numpy(), ref["grad_events"][:, c]) for c in range(2)]
    print("[event grad] public interface, weights and events: rel err grad %.2e grad_w %.2e x %.2e y %.2e" % tuple(e))
    assert max(e) <= TOL
    h.close()


def test_refusals_and_the_c_entry():
    ev = events(2000)
    theta = np.array([7.3, -4.1])
    desc = E.make_descriptor("image_variance", "2d-translation")
    h = E.CMaxHandle(SIZE).set_events(ev)
    h.set_deterministic(True)
    with pytest.raises(NotImplementedError, match="deterministic"):
        h.evaluate_event_grad(desc, theta)
    h.set_deterministic(False)
    want = h.evaluate_event_grad(desc, theta)[2].cpu().numpy()
    # the C entry through ctypes, and a wrong n
    lib = _lib.load()
    m = torch.tensor(theta, dtype=torch.float64, device="cuda")
    d = type(desc).from_buffer_copy(desc)
    d.motion_dtype = _lib.F64
    res = torch.empty(8, dtype=torch.float64, device="cuda")
    csum = torch.empty(4, dtype=torch.float64, device="cuda")
    ge = torch.empty((ev.shape[0], 3), dtype=torch.float32, device="cuda")
    rc = lib.cmax_objective_event_grad(h._h, ctypes.byref(d), m.data_ptr(), res.data_ptr(), None, ge.data_ptr(), ev.shape[0] - 1, csum.data_ptr(), F._stream())
    assert rc == -1 and b"n must equal" in lib.cmax_last_error()
    assert lib.cmax_objective_event_grad(h._h, ctypes.byref(d), m.data_ptr(), res.data_ptr(), None, ge.data_ptr(), ev.shape[0], csum.data_ptr(), F._stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(ge.cpu().numpy(), want)
    h.comm_init(force_rccl=True)  # a real one-rank communicator
    with pytest.raises(NotImplementedError, match="communicator"):
        h.evaluate_event_grad(desc, theta)
    h.comm_destroy()
    h.close()
