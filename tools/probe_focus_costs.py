#!/usr/bin/env python
"""What do the fused focus losses (mean_square, laplacian_magnitude, hessian_magnitude) cost?  1M events, 260 x 346, 2-DoF and dense flow,
sigma 0 and 1; per cost, microseconds per value + gradient and per Hessian-vector product
    1. natively, default form                       (k_stats_gimage_st between K1 and K3)
    2. natively with CMAX_NO_FUSED_FOCUS=1          (k_stats + k_gimage: read once per process, so a child of this program measures it)
    3. the same loss written in torch on fused_iwes (what a user had before the costs were fused; forward + backward, vhp)
    4. beside them, native gradient_magnitude at the same shape
with HIP events on the launch stream over windows of back-to-back calls (a warm-up first; the median of the windows).
Writes profiles/focus_costs_cost.txt.  usage: tools/probe_focus_costs.py            (--child: print the native rows as JSON and stop)"""
import json
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import event_based_optical_flow_amd as E

N, SIZE = 1_000_000, (260, 346)
ROWS = [(model, sigma) for model in ("2d-translation", "dense-flow") for sigma in (0.0, 1.0)]
COSTS = ["mean_square", "laplacian_magnitude", "hessian_magnitude"]
STENCILS = {
    "mean_square": [(1.0, [[0, 0, 0], [0, 1, 0], [0, 0, 0]])],
    "laplacian_magnitude": [(1.0, [[0, 1, 0], [1, -4, 1], [0, 1, 0]])],
    "hessian_magnitude": [(1.0, [[0, 1, 0], [0, -2, 0], [0, 1, 0]]), (1.0, [[0, 0, 0], [1, -2, 1], [0, 0, 0]]),
                          (2.0, [[0.25, 0, -0.25], [0, 0, 0], [-0.25, 0, 0.25]])],
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
    return float(np.median(ts))


def torch_focus(kind):
    ks = [(c, torch.tensor(s, dtype=torch.float32, device="cuda")[None, None]) for c, s in STENCILS[kind]]

    def loss(img):  # minus the mean over the image without its border, as the fused cost with direction "minimize"
        return -sum(c * torch.mean(torch.nn.functional.conv2d(img[None, None], k, padding=1)[0, 0, 1:-1, 1:-1] ** 2) for c, k in ks)

    return loss


def setup(model):
    H, W = SIZE
    ev = torch.from_numpy(E.utils.generate_events(N, H, W, 0.0, 0.05, seed=46)).cuda()
    if model == "2d-translation":
        motion = torch.tensor([20.0, -12.0], dtype=torch.float32, device="cuda")
    else:
        motion = torch.from_numpy(E.utils.generate_smooth_flow((H, W), 20, seed=1046).astype(np.float32)).cuda()
    tangent = torch.from_numpy(np.random.default_rng(48).normal(0, 1, tuple(motion.shape)).astype(np.float32)).cuda()
    return E.CMaxHandle((H, W)).set_events(ev), motion, tangent


def native_rows(costs):
    out = {}
    for model, sigma in ROWS:
        h, motion, tangent = setup(model)
        for cost in costs:
            desc = E.make_descriptor(cost, model, sigma=sigma)
            call, res, grad = h.prepare(desc, motion)
            out[f"{model}|{sigma}|{cost}"] = (time_us(call), time_us(lambda: h.hvp(desc, motion, tangent)))
        h.close()
    return out


if "--child" in sys.argv:
    print("JSON " + json.dumps(native_rows(COSTS)))
    sys.exit(0)

fused = native_rows(COSTS + ["gradient_magnitude"])
env = dict(os.environ, CMAX_NO_FUSED_FOCUS="1")
child = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=600)
if child.returncode != 0:
    sys.exit(f"the CMAX_NO_FUSED_FOCUS child ended with status {child.returncode}\n{child.stderr[-3000:]}")
separate = json.loads(next(line for line in child.stdout.splitlines() if line.startswith("JSON "))[5:])

lines = []
for model, sigma in ROWS:
    h, motion, tangent = setup(model)
    m = motion.clone().requires_grad_()
    gm = fused[f"{model}|{sigma}|gradient_magnitude"]
    lines.append(f"{model}, sigma {sigma:g}: {N} events, {SIZE[0]} x {SIZE[1]}; native gradient_magnitude {gm[0]:.1f} us value + gradient, {gm[1]:.1f} us hvp")
    for cost in COSTS:
        fn = torch_focus(cost)

        def fwd_bwd():
            loss = fn(E.fused_iwes(h, m, model, sigma=sigma)[0])
            return loss, torch.autograd.grad(loss, m)[0]

        def vhp():
            return torch.autograd.functional.vhp(lambda x: fn(E.fused_iwes(h, x, model, sigma=sigma)[0]), motion, tangent)[1]

        desc = E.make_descriptor(cost, model, sigma=sigma)
        res, grad = h.evaluate(desc, motion)
        l3, g3 = fwd_bwd()
        agree = (abs(l3.item() - res[0].item()) / abs(res[0].item()), float((g3.reshape(grad.shape).double() - grad.double()).abs().max() / grad.double().abs().max()))
        key = f"{model}|{sigma}|{cost}"
        t3 = (time_us(fwd_bwd), time_us(vhp))
        lines.append("  %-20s value + gradient: fused %7.1f us  separate %7.1f us  torch on fused_iwes %7.1f us  (fused / gradient_magnitude %.2f)   "
                     "hvp: native %7.1f us  torch %7.1f us   agreement of route 3: loss %.1e grad %.1e" % (
                         cost, fused[key][0], separate[key][0], t3[0], fused[key][0] / gm[0], fused[key][1], t3[1], agree[0], agree[1]))
        print(lines[-1], flush=True)
    h.close()
os.makedirs("profiles", exist_ok=True)
with open("profiles/focus_costs_cost.txt", "w") as f:
    f.write("tools/probe_focus_costs.py -- the fused focus losses: default form (k_stats_gimage_st), separate launches (CMAX_NO_FUSED_FOCUS=1, in a "
            "child process), the same loss in torch on fused_iwes, and native gradient_magnitude (HIP events, median of 7 windows of 20; python "
            "and autograd overhead included in the torch route)\n")
    f.write("\n".join(lines) + "\n")
