"""dL/dw of the fused objective (cmax_objective_weight_grad, CMaxHandle.evaluate_weight_grad, ContrastObjective(..., weights=)): against the
fp64 value composed from the committed oracle (tests/_weight_grad_ref.py) at the project's plain gate, max|delta| / max|ref| <= 1e-4, the
reference taken on the motion the device holds; `result` and `grad` of the same call at the same gate.  dL/dw is continuous across cell
borders, so no event is excluded from any comparison.  Measured errors are printed."""
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

import _weight_grad_worker as W  # noqa: E402
from _weight_grad_ref import weight_grad_objective  # noqa: E402
from _weighted_ref import weight_set  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
SIZE = (64, 80)
COSTS = ["image_variance", "gradient_magnitude", "normalized_image_variance", "normalized_gradient_magnitude",
         "multi_focal_normalized_image_variance", "multi_focal_normalized_gradient_magnitude"]
MODELS = ["2d-translation", "dense-flow", "dense-flow-voxel"]
T_BINS = 4


def f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def rel_max(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def motion_for(model, size, seed=11, mag=8):
    if model == "2d-translation":
        return np.array([7.3, -4.1])
    if model == "dense-flow":
        return f32(E.utils.generate_smooth_flow(size, mag, seed=seed))
    return f32(np.stack([E.utils.generate_smooth_flow(size, mag, seed=seed + t) for t in range(T_BINS)]))


def gate(tag, got, ref):
    res, grad, gw = got
    e_loss = abs(res[0].item() - ref["loss"]) / abs(ref["loss"])
    e_grad = rel_max(grad.double().cpu().numpy(), ref["grad"])
    e_gw = rel_max(gw.double().cpu().numpy(), ref["grad_w"])
    print(f"[weight grad] {tag}: rel err loss {e_loss:.2e} grad {e_grad:.2e} grad_w {e_gw:.2e}")
    assert e_loss <= TOL and e_grad <= TOL and e_gw <= TOL, (tag, e_loss, e_grad, e_gw)
    return e_gw


def check_case(tag, h, ev, w, model, size, cost, sigma, pad=0, **kw):
    motion = kw.pop("motion", None)
    motion = motion_for(model, size) if motion is None else motion
    desc = E.make_descriptor(cost, model, sigma=sigma, time_bin=T_BINS if model == "dense-flow-voxel" else 0, **kw)
    ref = weight_grad_objective(ev, motion, model, size, w, cost=cost, sigma=sigma, outer_padding=pad, **kw)
    got = h.evaluate_weight_grad(desc, motion)
    gate(tag, got, ref)
    return got, ref


@pytest.fixture(scope="module")
def small():
    yield E.utils.generate_events(150_000, SIZE[0], SIZE[1], 0.0, 0.05, seed=21)


@pytest.mark.parametrize("wname", ["uniform", "polarity", "zeros", "hdr"])
@pytest.mark.parametrize("model", MODELS)
def test_parity(small, model, wname):
    """3 models x 6 costs x sigma in {0, 1} per weight set."""
    ev = small
    w = weight_set(wname, ev, seed=31)
    h = E.CMaxHandle(SIZE).set_events(ev, time_bin=T_BINS if model == "dense-flow-voxel" else 0, weights=w)
    for cost in COSTS:
        for sigma in (0, 1):
            (res, grad, gw), ref = check_case(f"{model} {wname} {cost} sigma {sigma}", h, ev, w, model, SIZE, cost, sigma)
            if wname == "zeros":  # the value is not multiplied by w: weight-0 events have a derivative
                z = w == 0
                g0, r0 = gw.double().cpu().numpy()[z], ref["grad_w"][z]
                assert np.abs(g0).max() > 0 and np.abs(r0).max() > 0
                assert np.abs(g0 - r0).max() <= TOL * np.abs(ref["grad_w"]).max()
    h.close()


@pytest.mark.parametrize("model", MODELS)
def test_unweighted_handle_means_unit_weights(small, model):
    ev = small
    h = E.CMaxHandle(SIZE).set_events(ev, time_bin=T_BINS if model == "dense-flow-voxel" else 0)
    assert not h.weighted
    for cost, sigma in (("image_variance", 0), ("gradient_magnitude", 1), ("normalized_image_variance", 1), ("multi_focal_normalized_image_variance", 0)):
        check_case(f"unweighted {model} {cost} sigma {sigma}", h, ev, 1.0, model, SIZE, cost, sigma)
    assert not h.weighted
    h.close()


def test_the_unwarped_term(small):
    """normalized_image_variance: the un-warped image is a weighted vote too.  The reference without that term differs from the full
    one by far more than the gate on this input, and the device agrees with the full one."""
    ev = small
    w = weight_set("uniform", ev, seed=35)
    motion = motion_for("dense-flow", SIZE)
    h = E.CMaxHandle(SIZE).set_events(ev, weights=w)
    for direction in ("minimize", "maximize"):
        full = weight_grad_objective(ev, motion, "dense-flow", SIZE, w, cost="normalized_image_variance", direction=direction)
        part = weight_grad_objective(ev, motion, "dense-flow", SIZE, w, cost="normalized_image_variance", direction=direction, with_orig=False)
        d = rel_max(part["grad_w"], full["grad_w"])
        print(f"[weight grad] un-warped term, {direction}: the reference without it differs by {d:.2e}")
        assert d > 100 * TOL
        got = h.evaluate_weight_grad(E.make_descriptor("normalized_image_variance", "dense-flow", direction=direction), motion)
        gate(f"un-warped term {direction}", got, full)
    h.close()


def test_permuting_events_and_weights_permutes_grad_w(small):
    ev = small
    w = weight_set("uniform", ev, seed=51)
    perm = np.random.default_rng(52).permutation(ev.shape[0])
    motion = motion_for("dense-flow", SIZE)
    desc = E.make_descriptor("gradient_magnitude", "dense-flow", sigma=1)
    out = []
    for e, ww in ((ev, w), (ev[perm], w[perm])):
        h = E.CMaxHandle(SIZE).set_events(e, tmin=float(ev[:, 2].min()), tmax=float(ev[:, 2].max()), weights=ww)
        out.append(h.evaluate_weight_grad(desc, motion)[2].double().cpu().numpy())
        h.close()
    assert np.abs(out[1] - out[0][perm]).max() <= 1e-5 * np.abs(out[0]).max()  # (fp32 atomics in the image: order-of-additions noise)


def test_reorderings():
    size, n = (128, 160), 300_000
    ev = E.utils.generate_events(n, size[0], size[1], 0.0, 0.05, seed=61)
    w = weight_set("zeros", ev, seed=62)
    h = E.CMaxHandle(size).set_events(ev, weights=w)
    h.set_time_slabs(4)
    check_case("4 slabs, dense", h, ev, w, "dense-flow", size, "gradient_magnitude", 1)
    check_case("4 slabs, 2-DoF", h, ev, w, "2d-translation", size, "normalized_image_variance", 0)
    h.set_time_bins(T_BINS)
    check_case("binned, voxel", h, ev, w, "dense-flow-voxel", size, "image_variance", 0)
    check_case("binned, dense", h, ev, w, "dense-flow", size, "multi_focal_normalized_gradient_magnitude", 1)
    h.set_time_bins(0)
    check_case("un-binned again", h, ev, w, "dense-flow", size, "image_variance", 1)
    h.close()


def _off_sensor_batch():
    rng = np.random.default_rng(91)
    ev = E.utils.generate_events(60_000, SIZE[0], SIZE[1], 0.0, 0.05, seed=90)
    out = rng.random(ev.shape[0]) < 0.33
    ev[out, 0] = rng.uniform(-25.0, SIZE[0] + 25.0, int(out.sum()))
    ev[out, 1] = rng.uniform(-25.0, SIZE[1] + 25.0, int(out.sum()))
    off = (np.floor(ev[:, 0]) < 0) | (np.floor(ev[:, 0]) >= SIZE[0]) | (np.floor(ev[:, 1]) < 0) | (np.floor(ev[:, 1]) >= SIZE[1])
    ext = [int(np.argmin(ev[:, 2])), int(np.argmax(ev[:, 2]))]  # (the batch's time extremes stay on the sensor)
    off[ext] = False
    ev[ext, :2] = [[3.0, 4.0], [5.0, 6.0]]
    return ev, off


def test_dropped_events_get_zero():
    ev, off = _off_sensor_batch()
    assert off.sum() > 1000
    w = weight_set("uniform", ev, seed=72)
    h = E.CMaxHandle(SIZE).set_keep_outside(False)
    h.set_events(ev, on_dropped="ignore", weights=w)
    assert h.batch_info()["dropped"] == int(off.sum())
    motion = motion_for("dense-flow", SIZE)
    ref = weight_grad_objective(ev[~off], motion, "dense-flow", SIZE, w[~off], cost="gradient_magnitude", sigma=1)
    res, grad, gw = h.evaluate_weight_grad(E.make_descriptor("gradient_magnitude", "dense-flow", sigma=1), motion)
    gw = gw.double().cpu().numpy()
    assert (gw[off] == 0).all()
    gate("dropped events", (res, grad, torch.from_numpy(gw[~off])), ref)
    h.close()


@pytest.mark.parametrize("pad", [0, 6])
def test_kept_off_sensor_events_two_dof(pad):
    ev, off = _off_sensor_batch()
    w = weight_set("zeros", ev, seed=73)
    h = E.CMaxHandle(SIZE, outer_padding=pad).set_keep_outside(True).set_events(ev, on_dropped="ignore", weights=w)
    assert h.batch_info()["outside"] == int(off.sum()) and h.batch_info()["fractional"]
    theta = np.array([17.0, -21.0])
    for cost, sigma in (("image_variance", 0), ("normalized_gradient_magnitude", 1)):
        check_case(f"kept off-sensor events, pad {pad}, {cost}", h, ev, w, "2d-translation", SIZE, cost, sigma, pad=pad, motion=theta)
    with pytest.raises(_lib.CmaxError):  # dense models stay refused on such a batch
        h.evaluate_weight_grad(E.make_descriptor("image_variance", "dense-flow"), np.zeros((2,) + SIZE, np.float32))
    h.close()


@pytest.mark.parametrize("model", MODELS)
def test_kernel_branches(model):
    """Fractional sources with padding 3, omit_boundary=False and maximize, reference times middle / last / 0.3, normalize_t=False."""
    rng = np.random.default_rng(101)
    ev = E.utils.generate_events(100_000, SIZE[0], SIZE[1], 0.0, 0.05, seed=102)
    ev[:, 0] = np.clip(np.floor(ev[:, 0]) + rng.uniform(0, 0.999, ev.shape[0]), 0, SIZE[0] - 1e-3)
    ev[:, 1] = np.clip(np.floor(ev[:, 1]) + rng.uniform(0, 0.999, ev.shape[0]), 0, SIZE[1] - 1e-3)
    w = weight_set("zeros", ev, seed=103)
    h = E.CMaxHandle(SIZE, outer_padding=3).set_events(ev, time_bin=T_BINS if model == "dense-flow-voxel" else 0, weights=w)
    assert h.batch_info()["fractional"]
    check_case(f"{model} frac pad 3", h, ev, w, model, SIZE, "gradient_magnitude", 1, pad=3)
    check_case(f"{model} frac pad 3 no omit maximize", h, ev, w, model, SIZE, "normalized_image_variance", 1, pad=3, omit_boundary=False, direction="maximize")
    check_case(f"{model} frac pad 3 multi-focal maximize", h, ev, w, model, SIZE, "multi_focal_normalized_image_variance", 0, pad=3, direction="maximize")
    for wd in ("middle", "last", 0.3):
        check_case(f"{model} frac pad 3 reference time {wd}", h, ev, w, model, SIZE, "image_variance", 0, pad=3, warp_direction=wd)
    if model != "dense-flow-voxel":
        m = motion_for(model, SIZE)
        check_case(f"{model} frac pad 3 normalize_t False", h, ev, w, model, SIZE, "image_variance", 1, pad=3, normalize_t=False, motion=f32(m / 0.05))
    h.close()


@pytest.mark.parametrize("model", ["2d-translation", "dense-flow"])
def test_clipped_window(model):
    """150 px over the batch on 130 x 173: corners outside the LDS window are read from global memory; with and without time slabs."""
    size, n = (130, 173), 120_000
    ev = E.utils.generate_events(n, size[0], size[1], 0.0, 0.05, seed=61)
    w = weight_set("uniform", ev, seed=63)
    motion = np.array([150.0, -140.0]) if model == "2d-translation" else f32(E.utils.generate_smooth_flow(size, 150, grid=3, seed=62))
    h = E.CMaxHandle(size).set_events(ev, weights=w)
    check_case(f"clipped window {model}", h, ev, w, model, size, "image_variance", 0, motion=motion)
    check_case(f"clipped window {model} normalised", h, ev, w, model, size, "normalized_gradient_magnitude", 1, motion=motion)
    h.set_time_slabs(4)
    check_case(f"clipped window {model}, 4 slabs", h, ev, w, model, size, "image_variance", 0, motion=motion)
    h.close()


@pytest.mark.parametrize("env", [{"CMAX_BIG_SEG": "1"}, {"CMAX_BIG_SEG": "1", "CMAX_COMPACT": "0"}, {"CMAX_MID_SEG": "1"}], ids=["big", "big-uncompacted", "mid"])
def test_forced_segment_layouts(env, tmp_path):
    """b512 (with and without the compact event copy) and m512, each in a child process of its own (tests/_weight_grad_worker.py)."""
    e = dict(os.environ)
    for name in ("CMAX_BIG_SEG", "CMAX_MID_SEG", "CMAX_COMPACT"):
        e.pop(name, None)
    e.update(env)
    layout = "big" if "CMAX_BIG_SEG" in env else "mid"
    out = str(tmp_path / "got.npz")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_weight_grad_worker.py"), layout, out], env=e, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, f"{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    got = dict(np.load(out))
    assert int(got["segment_events"]) == (4088 if "CMAX_BIG_SEG" in env else 3064)
    ev, w, size = W.batch(layout)
    for model, cost, sigma in W.CASES:
        ref = weight_grad_objective(ev, W.motion_for(model, size), model, size, w, cost=cost, sigma=sigma)
        tag = f"{model}/{cost}"
        gate(f"{env} {tag}", (torch.tensor([float(got[tag + '/loss'])]), torch.from_numpy(got[tag + "/grad"]), torch.from_numpy(got[tag + "/grad_w"])), ref)


def test_sparse_batches():
    """20 000 events (short runs per pixel: the strided dense K3) and 60 events."""
    for n in (20_000, 60):
        ev = E.utils.generate_events(n, SIZE[0], SIZE[1], 0.0, 0.05, seed=111)
        w = weight_set("uniform", ev, seed=112)
        h = E.CMaxHandle(SIZE).set_events(ev, weights=w)
        for model in ("2d-translation", "dense-flow"):
            check_case(f"{n} events {model}", h, ev, w, model, SIZE, "image_variance", 0)
            check_case(f"{n} events {model} normalised", h, ev, w, model, SIZE, "normalized_gradient_magnitude", 1)
        h.close()


def test_empty_handle():
    h = E.CMaxHandle(SIZE).set_events(np.zeros((0, 4)))
    res, grad, gw = h.evaluate_weight_grad(E.make_descriptor("image_variance", "2d-translation"), np.array([1.0, 2.0]))
    assert gw.shape == (0,) and res[0].item() == 0.0 and float(grad.abs().max()) == 0.0
    # from C, an empty batch may hand over no grad_w at all
    desc = E.make_descriptor("image_variance", "2d-translation")
    m = torch.tensor([1.0, 2.0], dtype=torch.float32, device="cuda")
    out = torch.ones(8, dtype=torch.float64, device="cuda")
    assert _lib.load().cmax_objective_weight_grad(h._h, ctypes.byref(desc), m.data_ptr(), out.data_ptr(), None, None, 0, F._stream()) == 0
    torch.cuda.synchronize()
    assert out[0].item() == 0.0
    h.close()


def test_refusals(small):
    ev = small
    theta = np.array([7.3, -4.1])
    desc = E.make_descriptor("image_variance", "2d-translation")
    h = E.CMaxHandle(SIZE).set_events(ev)
    h.set_deterministic(True)
    with pytest.raises(NotImplementedError, match="deterministic"):
        h.evaluate_weight_grad(desc, theta)
    h.set_deterministic(False)
    h.evaluate_weight_grad(desc, theta)
    # a wrong n
    lib = _lib.load()
    m = torch.tensor(theta, dtype=torch.float64, device="cuda")
    d = type(desc).from_buffer_copy(desc)
    d.motion_dtype = _lib.F64
    res = torch.empty(8, dtype=torch.float64, device="cuda")
    gw = torch.empty(ev.shape[0], dtype=torch.float32, device="cuda")
    rc = lib.cmax_objective_weight_grad(h._h, ctypes.byref(d), m.data_ptr(), res.data_ptr(), None, gw.data_ptr(), ev.shape[0] - 1, F._stream())
    assert rc == -1 and b"n must equal" in lib.cmax_last_error()
    assert lib.cmax_objective_weight_grad(h._h, ctypes.byref(d), m.data_ptr(), res.data_ptr(), None, gw.data_ptr(), ev.shape[0], F._stream()) == 0
    torch.cuda.synchronize()
    h.comm_init(force_rccl=True)  # a real one-rank communicator
    with pytest.raises(NotImplementedError, match="communicator"):
        h.evaluate_weight_grad(desc, theta)
    h.comm_destroy()
    h.close()


@pytest.mark.parametrize("weighted", [False, True])
def test_nothing_else_moved(small, weighted):
    """`evaluate` before and after an evaluate_weight_grad call on one handle agree to the order-of-additions noise, and has_raw stays."""
    ev = small
    h = E.CMaxHandle(SIZE).set_events(ev, weights=weight_set("uniform", ev, seed=121) if weighted else None)
    for model, cost, sigma in (("2d-translation", "image_variance", 0), ("dense-flow", "image_variance", 1), ("dense-flow", "normalized_image_variance", 0),
                               ("2d-translation", "multi_focal_normalized_gradient_magnitude", 1)):
        motion = motion_for(model, SIZE)
        desc = E.make_descriptor(cost, model, sigma=sigma)
        raw = h.has_raw(desc)
        r0, g0 = h.evaluate(desc, motion)
        r0, g0 = r0[0].item(), g0.double().cpu().numpy().copy()
        h.evaluate_weight_grad(desc, motion)
        r1, g1 = h.evaluate(desc, motion)
        assert abs(r1[0].item() - r0) <= 1e-6 * abs(r0), (model, cost)
        assert rel_max(g1.double().cpu().numpy(), g0) <= 1e-5, (model, cost)
        assert h.has_raw(desc) == raw and h.weighted == weighted
    h.close()


def test_public_interface(small):
    ev = small
    wn = weight_set("zeros", ev, seed=131)
    th = np.array([7.3, -4.1])
    h = E.CMaxHandle(SIZE).set_events(ev)
    obj = E.ContrastObjective(h, "2d-translation", cost="gradient_magnitude", sigma=1)
    theta = torch.tensor(th, dtype=torch.float64, device="cuda", requires_grad=True)
    w = torch.tensor(wn, dtype=torch.float64, device="cuda", requires_grad=True)
    loss = obj(theta, weights=w)
    loss.backward()
    ref = weight_grad_objective(ev, th, "2d-translation", SIZE, wn, cost="gradient_magnitude", sigma=1)
    e = (abs(loss.item() - ref["loss"]) / abs(ref["loss"]), rel_max(theta.grad.cpu().numpy(), ref["grad"]), rel_max(w.grad.cpu().numpy(), ref["grad_w"]))
    print(f"[weight grad] public interface, plain: rel err loss {e[0]:.2e} grad {e[1]:.2e} grad_w {e[2]:.2e}")
    assert max(e) <= TOL
    # hybrid: an "inv" member plus total_variation (which does not depend on w)
    cww = {"image_variance": "inv", "gradient_magnitude": 0.5, "total_variation": 0.1}
    obj = E.ContrastObjective(h, "2d-translation", cost="hybrid", cost_with_weight=cww, sigma=1)
    theta.grad, w.grad = None, None
    flow = torch.tensor(np.random.default_rng(5).normal(0, 1, (2, 4, 5)), dtype=torch.float64, device="cuda")
    loss = obj(theta, coarse_flow=flow, weights=w)
    loss.backward()
    a = weight_grad_objective(ev, th, "2d-translation", SIZE, wn, cost="image_variance", sigma=1)
    b = weight_grad_objective(ev, th, "2d-translation", SIZE, wn, cost="gradient_magnitude", sigma=1)
    tv = E.functional.total_variation(flow, True).item()
    ref_loss = 1.0 / a["loss"] + 0.5 * b["loss"] + 0.1 * tv
    ref_g = -a["grad"] / a["loss"] ** 2 + 0.5 * b["grad"]
    ref_gw = -a["grad_w"] / a["loss"] ** 2 + 0.5 * b["grad_w"]
    e = (abs(loss.item() - ref_loss) / abs(ref_loss), rel_max(theta.grad.cpu().numpy(), ref_g), rel_max(w.grad.cpu().numpy(), ref_gw))
    print(f"[weight grad] public interface, hybrid: rel err loss {e[0]:.2e} grad {e[1]:.2e} grad_w {e[2]:.2e}")
    assert max(e) <= TOL
    h.close()


def test_gradient_descent_on_the_weights(small):
    """Ten steps on w alone lower the loss monotonically on a fixed batch."""
    ev = small
    h = E.CMaxHandle(SIZE).set_events(ev)
    obj = E.ContrastObjective(h, "2d-translation", cost="image_variance")
    theta = torch.tensor([7.3, -4.1], dtype=torch.float64, device="cuda")
    w = torch.ones(ev.shape[0], dtype=torch.float64, device="cuda", requires_grad=True)
    losses = []
    for _ in range(11):
        loss = obj(theta, weights=w)
        (g,) = torch.autograd.grad(loss, w)
        losses.append(loss.item())
        with torch.no_grad():
            w -= 0.02 * g / g.abs().max()
    print("[weight grad] descent on w:", " ".join(f"{v:.6g}" for v in losses))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    h.close()
