#!/usr/bin/env python
"""What do per-event weights (cmax_set_event_weights) cost an evaluation?  One evaluation on the SAME handle and batch, unweighted and
weighted (uniform random weights in [0.2, 3]), timed with HIP events over windows of back-to-back evaluations, plus K1 / K3 from the
library's per-class brackets.  Rows: cfg2's shape (1M events, 260 x 346, 2-DoF variance -- the unweighted handle takes the deferred
2-DoF path, the weighted one the general vote -> statistics -> gather path), cfg3's shape (5M, dense gradient magnitude), cfg5 at 20M
(720p, dense variance, big segments + compact events).  Writes profiles/weights_cost.txt.  usage: tools/probe_weights.py [row ...]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import event_based_optical_flow_amd as E

ROWS = {
    "cfg2": dict(n=1_000_000, size=(260, 346), model="2d-translation", cost="image_variance", sigma=0.0),
    "cfg3": dict(n=5_000_000, size=(260, 346), model="dense-flow", cost="gradient_magnitude", sigma=1.0),
    "cfg5_20M": dict(n=20_000_000, size=(720, 1280), model="dense-flow", cost="image_variance", sigma=0.0),
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
    return float(np.median(ts))


def classes_us(h, call):
    h.set_profiling(True, repeat=8)
    for _ in range(10):
        call()
    torch.cuda.synchronize()
    p = h.read_profile()
    h.set_profiling(False)
    return {q: v[0] / max(v[1], 1) * 1e3 for q, v in p.items() if v[1]}


lines = []
for name in sys.argv[1:] or list(ROWS):
    c = ROWS[name]
    H, W = c["size"]
    ev = torch.from_numpy(E.utils.generate_events(c["n"], H, W, 0.0, 0.05, seed=46)).cuda()
    if c["model"] == "2d-translation":
        motion = torch.tensor([20.0, -12.0], dtype=torch.float32, device="cuda")
    else:
        motion = torch.from_numpy(E.utils.generate_smooth_flow((H, W), 20, seed=1046).astype(np.float32)).cuda()
    w = torch.from_numpy(np.random.default_rng(47).uniform(0.2, 3.0, c["n"]).astype(np.float32)).cuda()
    h = E.CMaxHandle((H, W)).set_events(ev)
    desc = E.make_descriptor(c["cost"], c["model"], sigma=c["sigma"])
    call, _res, _grad = h.prepare(desc, motion)
    out = {}
    for tag, weights in (("unweighted", None), ("weighted", w), ("unweighted again", None)):
        h.set_event_weights(weights)
        out[tag] = (time_us(call), classes_us(h, call))
    info = h.work_list_info()
    for tag, (t, k) in out.items():
        lines.append("%-9s %-17s %8.1f us per evaluation  (K1 %6.1f  image %5.1f  K3 %6.1f)   %d events, %d segments of <= %d" % (
            name, tag, t, k.get("vote", 0), k.get("stats", 0) + k.get("gimage", 0), k.get("grad", 0), c["n"], info["segments"], info["segment_events"]))
    lines.append("%-9s weighted / unweighted = %.3f" % (name, out["weighted"][0] / out["unweighted"][0]))
    print("\n".join(lines[-4:]), flush=True)
    h.close()
    del ev, w
os.makedirs("profiles", exist_ok=True)
with open("profiles/weights_cost.txt", "w") as f:
    f.write("tools/probe_weights.py -- one evaluation, unweighted vs weighted, same handle and batch (HIP events, median of 7 windows of 40)\n")
    f.write("\n".join(lines) + "\n")
