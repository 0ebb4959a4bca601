#!/usr/bin/env python
"""What does a cost written in torch on fused_iwes cost against the fused kernels it stands in for, and against the leaf operators?
On ONE handle per row -- cfg2's shape (1M events, 260 x 346, 2-DoF) and one dense shape (1M events, 260 x 346, dense flow, sigma 1) -- a
torch variance (minus the unbiased variance of the image without its border, the fused image_variance re-expressed) is timed
    forward + backward   through fused_iwes                  against cmax_objective (value + gradient)
    vhp                  torch.autograd.functional.vhp        against cmax_objective_hvp
    forward + backward   through the leaf operators           (F.warp_events -> F.vote [-> F.gaussian_blur3]: [n,4] warped events materialised,
                                                                unsorted vote and gather)
with HIP events on the launch stream over windows of back-to-back calls (a warm-up first; the median of the windows).  The layer's
figures include torch's autograd and its image-side kernels.  Writes profiles/iwe_layer_cost.txt.  usage: tools/probe_iwe_layer.py [row ...]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import event_based_optical_flow_amd as E
from event_based_optical_flow_amd import functional as F

ROWS = {
    "cfg2_2dof_1M": dict(n=1_000_000, size=(260, 346), model="2d-translation", sigma=0.0),
    "dense_1M_s1": dict(n=1_000_000, size=(260, 346), model="dense-flow", sigma=1.0),
}


def time_us(call, windows=7, steps=20, warm=20):
    for _ in range(warm):
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


def torch_variance(img):
    return -torch.var(img[1:-1, 1:-1])


lines = []
for name in sys.argv[1:] or list(ROWS):
    c = ROWS[name]
    H, W = c["size"]
    ev = torch.from_numpy(E.utils.generate_events(c["n"], H, W, 0.0, 0.05, seed=46)).cuda()
    if c["model"] == "2d-translation":
        motion = torch.tensor([20.0, -12.0], dtype=torch.float32, device="cuda")
    else:
        motion = torch.from_numpy(E.utils.generate_smooth_flow((H, W), 20, seed=1046).astype(np.float32)).cuda()
    tangent = torch.from_numpy(np.random.default_rng(48).normal(0, 1, tuple(motion.shape)).astype(np.float32)).cuda()
    h = E.CMaxHandle((H, W)).set_events(ev)
    desc = E.make_descriptor("image_variance", c["model"], sigma=c["sigma"])
    fused, res, grad = h.prepare(desc, motion)
    m = motion.clone().requires_grad_()

    def layer_fwd_bwd():
        loss = torch_variance(E.fused_iwes(h, m, c["model"], sigma=c["sigma"])[0])
        return loss, torch.autograd.grad(loss, m)[0]

    def layer_vhp():
        return torch.autograd.functional.vhp(lambda x: torch_variance(E.fused_iwes(h, x, c["model"], sigma=c["sigma"])[0]), motion, tangent)[1]

    ev32 = ev.to(torch.float32)

    def leaf_fwd_bwd():
        warped = F.warp_events(ev32, m, c["model"], (H, W), "first", True)
        img = F.vote(warped, (H, W))
        if c["sigma"] > 0:
            img = F.gaussian_blur3(img, c["sigma"])
        loss = torch_variance(img)
        return loss, torch.autograd.grad(loss, m)[0]

    # the three paths agree before anything is timed
    fused()
    l1, g1 = layer_fwd_bwd()
    l2, g2 = leaf_fwd_bwd()
    hv1, hv0 = layer_vhp(), h.hvp(desc, motion, tangent)
    rel = lambda a, b: float((a.double() - b.double()).abs().max() / b.double().abs().max())  # noqa: E731
    check = "loss %.1e / %.1e, grad %.1e / %.1e (layer / leaf vs cmax_objective), vhp %.1e (vs cmax_objective_hvp)" % (
        abs(l1.item() - res[0].item()) / abs(res[0].item()), abs(l2.item() - res[0].item()) / abs(res[0].item()), rel(g1.reshape(grad.shape), grad),
        rel(g2.reshape(grad.shape), grad), rel(hv1.reshape(hv0.shape), hv0))
    t = {"cmax_objective (value + gradient)": time_us(fused), "torch variance on fused_iwes, forward + backward": time_us(layer_fwd_bwd),
         "torch variance on the leaf operators, forward + backward": time_us(leaf_fwd_bwd),
         "cmax_objective_hvp": time_us(lambda: h.hvp(desc, motion, tangent)), "vhp of the torch variance on fused_iwes": time_us(layer_vhp)}
    info = h.work_list_info()
    lines.append("%s: %d events, %d x %d, %s, sigma %g, %d segments of <= %d; agreement: %s" % (name, c["n"], H, W, c["model"], c["sigma"], info["segments"],
                                                                                          info["segment_events"], check))
    for k, v in t.items():
        lines.append("  %-58s %9.1f us  (windows %.1f .. %.1f)" % (k, v[0], v[1], v[2]))
    a, b, cc = t["cmax_objective (value + gradient)"][0], t["torch variance on fused_iwes, forward + backward"][0], t["torch variance on the leaf operators, forward + backward"][0]
    lines.append("  layer / objective = %.2f   leaf / layer = %.2f   layer vhp / cmax_objective_hvp = %.2f" % (
        b / a, cc / b, t["vhp of the torch variance on fused_iwes"][0] / t["cmax_objective_hvp"][0]))
    print("\n".join(lines[-7:]), flush=True)
    h.close()
    del ev, ev32
os.makedirs("profiles", exist_ok=True)
with open("profiles/iwe_layer_cost.txt", "w") as f:
    f.write("tools/probe_iwe_layer.py -- a torch cost on fused_iwes against the fused kernels and against the leaf operators, one handle per row "
            "(HIP events, median of 7 windows of 20; python and autograd overhead included in every torch path)\n")
    f.write("\n".join(lines) + "\n")
