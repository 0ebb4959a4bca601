#!/usr/bin/env python
"""What does dL/d(event) (cmax_objective_event_grad) cost on top of an evaluation?  cmax_objective and cmax_objective_event_grad on the SAME
unweighted handle and batch, timed with HIP events on the launch stream over windows of back-to-back calls (a warm-up first; the median
of the windows).  Rows: 1M events 2-DoF variance (260 x 346), 5M events dense gradient magnitude (sigma 1), and a normalised cost (1M
events, 2-DoF normalised variance: the un-warped image is voted, turned into G_orig and gathered as two more planes).  Writes
profiles/event_grad_cost.txt.  usage: tools/probe_event_grad.py [row ...]"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import event_based_optical_flow_amd as E
from event_based_optical_flow_amd import _lib
from event_based_optical_flow_amd import functional as F

ROWS = {
    "2dof_var_1M": dict(n=1_000_000, size=(260, 346), model="2d-translation", cost="image_variance", sigma=0.0),
    "dense_gm_5M": dict(n=5_000_000, size=(260, 346), model="dense-flow", cost="gradient_magnitude", sigma=1.0),
    "2dof_nvar_1M": dict(n=1_000_000, size=(260, 346), model="2d-translation", cost="normalized_image_variance", sigma=0.0),
}


def time_us(call, windows=7, steps=40):
    for _ in range(60):
        call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            call()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / steps * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


lines = []
lib = _lib.load()
for name in sys.argv[1:] or list(ROWS):
    c = ROWS[name]
    H, W = c["size"]
    ev = torch.from_numpy(E.utils.generate_events(c["n"], H, W, 0.0, 0.05, seed=46)).cuda()
    if c["model"] == "2d-translation":
        motion = torch.tensor([20.0, -12.0], dtype=torch.float32, device="cuda")
    else:
        motion = torch.from_numpy(E.utils.generate_smooth_flow((H, W), 20, seed=1046).astype(np.float32)).cuda()
    h = E.CMaxHandle((H, W)).set_events(ev)
    desc = E.make_descriptor(c["cost"], c["model"], sigma=c["sigma"])
    plain, _res, grad = h.prepare(desc, motion)
    res2 = torch.empty(8, dtype=torch.float64, device="cuda")
    grad2 = torch.empty_like(grad)
    ge = torch.empty((c["n"], 3), dtype=torch.float32, device="cuda")
    csum = torch.empty(4, dtype=torch.float64, device="cuda")
    m, d2 = h._motion_arg(desc, motion)

    def with_ge():
        rc = lib.cmax_objective_event_grad(h._h, ctypes.byref(d2), m.data_ptr(), res2.data_ptr(), grad2.data_ptr(), ge.data_ptr(), c["n"], csum.data_ptr(), F._stream())
        if rc:
            _lib.check(rc)

    t0, t1 = time_us(plain), time_us(with_ge)
    info = h.work_list_info()
    lines.append("%-13s cmax_objective             %8.1f us  (windows %.1f .. %.1f)   %d events, %d segments of <= %d" % (name, t0[0], t0[1], t0[2], c["n"], info["segments"], info["segment_events"]))
    lines.append("%-13s cmax_objective_event_grad  %8.1f us  (windows %.1f .. %.1f)" % (name, t1[0], t1[1], t1[2]))
    lines.append("%-13s event_grad / objective = %.3f" % (name, t1[0] / t0[0]))
    print("\n".join(lines[-3:]), flush=True)
    h.close()
    del ev, ge
os.makedirs("profiles", exist_ok=True)
with open("profiles/event_grad_cost.txt", "w") as f:
    f.write("tools/probe_event_grad.py -- cmax_objective vs cmax_objective_event_grad on the same unweighted handle and batch (HIP events, median of 7 windows of 40)\n")
    f.write("\n".join(lines) + "\n")
