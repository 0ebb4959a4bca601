"""The exact Hessian-vector product (cmax_objective_hvp: k_vote_tan / k_vote_tan2, k_stats_tan, k_gimage_tan, k_grad_hvp) against the fp64
double backward of tests/_hvp_ref.py, on every branch of those kernels that a small batch reaches: fractional sources, padding, events
from off the sensor, the clipped window, several reference times, raw time, the image border, the deterministic integer path, time
slabs, time slices -- and, in fresh child processes (tests/_layout_worker.py), the big and mid segment layouts.

Gate: rel_max(Hv, Hv_ref) <= HVP_TOL = 1e-4 of the largest entry, the gate of tests/test_gpu_solver.py; loss and gradient of the same
handle at the plain 1e-4 gate, so that a failure can be put down to the product or to the evaluation.  Motions and tangents are fp32
values on both sides; events within fp32 rounding of a cell border are removed beforehand (the product is not defined there;
tests/test_hvp_reference.py caps their share at 0.5 %).  Measured errors: profiles/hvp_parity.txt.

Child processes (one at a time, no further child after a failed one).  Durations measured on the first green run on an MI355X, and the
limits derived from them (5 x, at least 60 s):
    big   CMAX_BIG_SEG=1                  3.1 s   -> limit 60 s
    big   CMAX_BIG_SEG=1 CMAX_COMPACT=0   3.8 s   -> limit 60 s
    mid   CMAX_MID_SEG=1                  3.5 s   -> limit 60 s
The mid batch is the one the issue proposes (256 x 256, 600 000 uniform events): the host's rule picks 3064-event segments for it."""
import ctypes
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import event_based_optical_flow_amd as E  # noqa: E402
from event_based_optical_flow_amd import _lib  # noqa: E402
from event_based_optical_flow_amd import functional as F  # noqa: E402
from oracle import oracle as orc  # noqa: E402

import _hvp_cases as C  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
HVP_TOL = 1e-4
CHILD_LIMIT_S = {("big", 0): 60, ("big", 1): 60, ("mid", 0): 60}


def rel_max(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def make_handle(c, b):
    h = E.CMaxHandle(c["size"], c["pad"])
    if c["outside"]:
        h.set_keep_outside(True)
    if c["deterministic"]:
        h.set_deterministic(True)
    tr = b["t_range"]
    h.set_events(b["ev"], tmin=tr[0] if tr else None, tmax=tr[1] if tr else None, time_bin=c["T"], on_dropped="ignore")
    assert h.n_events == len(b["ev"])
    if c["slabs"]:
        h.set_time_slabs(c["slabs"])
    desc = E.make_descriptor(c["cost"], c["model"], direction=c["direction"], sigma=float(c["sigma"]), omit_boundary=c["omit"],
                             normalize_t=c["normalize_t"], time_bin=c["T"], warp_direction=c["warp_direction"])
    return h, desc


def report(cid, h, b, e_loss, e_grad, e_hv, layout="default"):
    info = h.work_list_info()
    print(f"[hvp parity] {cid}: {len(b['ev'])} events, {info['segments']} segments of <= {info['segment_events']} ({layout}), "
          f"dropped {b['dropped']:.5f}, rel err loss {e_loss:.2e} grad {e_grad:.2e} Hv {e_hv:.2e}")


def check_case(c):
    b = C.built(c)
    h, desc = make_handle(c, b)
    res, grad = h.evaluate(desc, b["motion"])
    hv = h.hvp(desc, b["motion"], b["v"]).double().cpu().numpy()
    e_loss = abs(res[0].item() - b["loss"]) / abs(b["loss"])
    e_grad, e_hv = rel_max(grad.cpu().numpy(), b["grad"]), rel_max(hv, b["hv"])
    report(c["id"], h, b, e_loss, e_grad, e_hv)
    assert e_loss <= TOL and e_grad <= TOL, (c["id"], e_loss, e_grad)
    assert e_hv <= HVP_TOL, (c["id"], e_hv)
    return h, desc, b, hv


@pytest.mark.parametrize("cid", [c["id"] for c in C.CASES if c["group"] not in ("det", "slices")])
def test_hvp_against_the_fp64_reference(cid):
    h, desc, b, hv = check_case(C.ALL[cid])
    h.close()


@pytest.mark.parametrize("cid", [c["id"] for c in C.CASES if c["group"] == "det"])
def test_deterministic_hvp_against_the_fp64_reference(cid):
    """The integer path: the same gate, and two calls give the same bytes."""
    h, desc, b, hv = check_case(C.ALL[cid])
    assert h.deterministic
    again = h.hvp(desc, b["motion"], b["v"]).double().cpu().numpy()
    assert hv.tobytes() == again.tobytes()
    h.close()


@pytest.mark.parametrize("cid", ["matrix-2dof-gm-s0-n30000", "matrix-dense-iv-s1-n30000", "matrix-voxel5-gm-s1-n30000"])
def test_hvp_is_linear_in_the_tangent(cid):
    """The tangent is brought to unit max-norm for the fixed-point votes: 1e-6 v and 1e6 v against the scaled reference; v = 0 gives
    exact zeros."""
    c = C.ALL[cid]
    b = C.built(c)
    h, desc = make_handle(c, b)
    for scale in (1e-6, 1e6):
        # (the reference is linear in v; rounding the scaled tangent to fp32 moves an entry by 6e-8 of itself, far below the gate)
        hv = h.hvp(desc, b["motion"], b["v"] * scale).double().cpu().numpy()
        assert rel_max(hv, scale * b["hv"]) <= HVP_TOL, (cid, scale, rel_max(hv, scale * b["hv"]))
    z = h.hvp(desc, b["motion"], np.zeros_like(b["v"])).cpu().numpy()
    assert z.shape == b["hv"].shape and not z.any()
    h.close()


@pytest.mark.parametrize("model,T", [("2d-translation", 0), ("dense-flow", 0), ("dense-flow-voxel", 3)])
def test_empty_handle_gives_zeros(model, T):
    h = E.CMaxHandle(C.BASE).set_events(np.zeros((0, 4)), time_bin=T)
    motion = np.array([3.0, -2.0]) if model == "2d-translation" else np.ones(((T,) if T else ()) + (2,) + C.BASE)
    desc = E.make_descriptor("image_variance", model, sigma=1.0, time_bin=T)
    hv = h.hvp(desc, motion, np.ones_like(motion)).cpu().numpy()
    assert hv.shape == motion.shape and not hv.any()
    h.close()


def _hvp_dist(h, desc, motion, v):
    d = type(desc).from_buffer_copy(desc)
    d.motion_dtype = _lib.F32
    m = torch.tensor(motion, dtype=torch.float32, device="cuda").contiguous()
    umax = float(np.abs(v).max())
    t = torch.tensor(v / umax, dtype=torch.float32, device="cuda").contiguous()
    hv = torch.empty(2, dtype=torch.float64, device="cuda") if d.model == _lib.MODEL_2DOF else torch.empty(tuple(m.shape), dtype=torch.float32, device="cuda")
    _lib.check(_lib.load().cmax_objective_hvp_dist(h._h, ctypes.byref(d), m.data_ptr(), t.data_ptr(), hv.data_ptr(), F._stream()))
    torch.cuda.synchronize()
    return hv.double().cpu().numpy() * umax


@pytest.mark.parametrize("cid", [c["id"] for c in C.CASES if c["group"] == "slices"])
def test_time_slice_through_a_one_rank_communicator(cid):
    """A handle that holds one HALF of a batch with the whole batch's (t_min, t_max), raw time.  The product is not linear in the events, so
    the two halves' products do not add up to the whole batch's; what holds is that cmax_objective_hvp_dist on a real one-rank
    communicator (images, tangent images and product all-reduced) gives the product of the slice as the reference warps it: to the
    whole batch's first event."""
    c = C.ALL[cid]
    h, desc, b, hv = check_case(c)
    h.comm_init(force_rccl=True)
    assert h.comm_info()[:2] == (1, 0) and h.comm_info()[2] > 0
    hv_d = _hvp_dist(h, desc, b["motion"], b["v"])
    h.comm_destroy()
    h.close()
    assert rel_max(hv_d, b["hv"]) <= HVP_TOL, (cid, rel_max(hv_d, b["hv"]))


# ---- non-default segment layouts: read once per process from the environment, so each runs in a child of its own -------------------
_child_failed = []


def _run_child(layout, k, tmp_path):
    if _child_failed:
        pytest.fail(f"not started: an earlier layout child failed ({_child_failed[0]})")
    env = dict(os.environ)
    for name in ("CMAX_BIG_SEG", "CMAX_MID_SEG", "CMAX_COMPACT"):
        env.pop(name, None)
    env.update(C.LAYOUT_ENV[layout][k])
    out = str(tmp_path / f"{layout}{k}.npz")
    t0 = time.time()
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_layout_worker.py"), layout, out], env=env, cwd=ROOT,
                           capture_output=True, text=True, timeout=CHILD_LIMIT_S[(layout, k)])
    except subprocess.TimeoutExpired as e:
        _child_failed.append(f"{layout} {k}: timed out")
        pytest.fail(f"layout child {layout} {C.LAYOUT_ENV[layout][k]} exceeded {CHILD_LIMIT_S[(layout, k)]} s\n{e.stderr}")
    print(f"[hvp parity] child {layout} {C.LAYOUT_ENV[layout][k]}: {time.time() - t0:.1f} s")
    if p.returncode != 0:
        _child_failed.append(f"{layout} {k}: exit status {p.returncode}")
        pytest.fail(f"layout child {layout} {C.LAYOUT_ENV[layout][k]} ended with status {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    return dict(np.load(out))


@pytest.mark.parametrize("layout,k", [("big", 0), ("big", 1), ("mid", 0)], ids=["big", "big-uncompacted", "mid"])
def test_forced_segment_layouts_against_the_references(layout, k, tmp_path):
    """CMAX_BIG_SEG=1 (4088-event segments: K1 / K3 b512, voxel K3 b1024, k_vote_tan / k_grad_hvp b512), the same without the compacted
    event order, and CMAX_MID_SEG=1 (3064-event segments, m512): loss, gradient and IWE against orc.objective, the product against
    _hvp_ref, at the gates above.  The child asserts the segment size it ran with."""
    got = _run_child(layout, k, tmp_path)
    for c in C.LAYOUT_CASES[layout]:
        b, cid = C.built(c), c["id"]
        assert int(got[cid + "/segment_events"]) == C.LAYOUT_SEGMENT_EVENTS[layout]
        ref = orc.objective(b["ev"], b["motion"], c["model"], c["size"], cost=c["cost"], sigma=c["sigma"], warp_direction=c["warp_direction"])
        key = "forward_iwe" if c["cost"].startswith("multi_focal") else "iwe"  # reference time 0 of a multi-focal cost is "last"
        e_loss = abs(float(got[cid + "/loss"]) - ref["loss"]) / abs(ref["loss"])
        e_grad, e_iwe, e_hv = rel_max(got[cid + "/grad"], ref["grad"]), rel_max(got[cid + "/iwe"], ref["iwes"][key]), rel_max(got[cid + "/hv"], b["hv"])
        print(f"[hvp parity] {cid} {C.LAYOUT_ENV[layout][k]}: {len(b['ev'])} events, {int(got[cid + '/segments'])} segments of <= "
              f"{int(got[cid + '/segment_events'])}, dropped {b['dropped']:.5f}, rel err loss {e_loss:.2e} grad {e_grad:.2e} iwe {e_iwe:.2e} Hv {e_hv:.2e}")
        assert e_loss <= TOL and e_grad <= TOL and e_iwe <= TOL, (cid, e_loss, e_grad, e_iwe)
        assert e_hv <= HVP_TOL, (cid, e_hv)
