#!/usr/bin/env python
"""Wall time of `optimize(events)` of the time-aware single-scale solver (solver/mixed.py, registry name
"time_aware_mixed_patch_contrast_maximization") beside the pyramid solver, at the shape of BASELINE configs[0]: 260 x 346, 30k
events per batch, hybrid cost (multi-focal normalised gradient magnitude + 0.01 TV), blur sigma 1, Burgers T = 10 at "middle",
Newton-CG with max_iter 25, on the synthetic scene of tools/bench_solver_optimize.py (dots moving along a smooth flow).
Single scale: patch.size / sliding_window 16/16 (a 17 x 22 grid) and 16/8 (32 x 43, overlapping windows), filter bilinear and nearest,
patch.initialize "zero", "random" (seed 46, as the pyramid's row) and "global-best" (its 900-candidate search is part of the time).
Nothing is gated on these figures.
    python tools/probe_mixed_solver.py [out.txt]      (default: profiles/mixed_solver.txt)"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import event_based_optical_flow_amd as E  # noqa: E402
from event_based_optical_flow_amd import solver  # noqa: E402

H, W, N = 260, 346, 30000
REPS = 4


def scene():
    rng = np.random.default_rng(11)
    V = E.utils.generate_smooth_flow((H, W), 12.0, grid=3, seed=12)  # pixel displacement over the batch
    n_dots = 1500
    cx, cy = rng.uniform(8, H - 8, n_dots), rng.uniform(8, W - 8, n_dots)
    dot = rng.integers(0, n_dots, N)
    tau = np.sort(rng.uniform(0, 1, N))
    vx, vy = V[0, cx.astype(int), cy.astype(int)][dot], V[1, cx.astype(int), cy.astype(int)][dot]
    x = np.clip(np.round(cx[dot] + tau * vx + rng.normal(0, 0.4, N)), 0, H - 1)
    y = np.clip(np.round(cy[dot] + tau * vy + rng.normal(0, 0.4, N)), 0, W - 1)
    t_scale = 0.05
    ev = np.stack([x, y, tau * t_scale, rng.integers(0, 2, N).astype(float)], 1)
    mask = np.zeros((H, W), bool)
    mask[x.astype(int), y.astype(int)] = True
    mask[:8] = mask[-8:] = False
    mask[:, :8] = mask[:, -8:] = False
    return ev, V, mask, t_scale


def config(method, patch):
    slv_cfg = {"method": method, "time_aware": True, "time_bin": 10, "flow_interpolation": "burgers", "t0_flow_location": "middle",
               "patch": patch, "motion_model": "2d-translation", "warp_direction": "first", "parameters": ["trans_x", "trans_y"],
               "cost": "hybrid", "outer_padding": 0,
               "cost_with_weight": {"multi_focal_normalized_gradient_magnitude": 1.0, "total_variation": 0.01},
               "iwe": {"method": "bilinear_vote", "blur_sigma": 1}}
    opt_cfg = {"n_iter": 40, "method": "Newton-CG", "max_iter": 25,
               "parameters": {"trans_x": {"min": -150, "max": 150}, "trans_y": {"min": -150, "max": 150}}}
    return slv_cfg, opt_cfg


def run(name, method, patch, ev, V, mask, t_scale):
    slv = solver.collections[method]((H, W), {}, *config(method, patch), {}, None)
    times = []
    for _ in range(REPS):  # one solver for all repetitions, like main.py's loop over a sequence
        np.random.seed(46)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        best = slv.optimize(ev)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    results = [r for r in slv.history[-1:]] if method.startswith("time_aware") else [r for _, r in slv.history]
    nfev, njev, nhev = (sum(getattr(r, k, 0) for r in results) for k in ("nfev", "njev", "nhev"))
    flow = slv.get_original_flow_from_time_aware_flow_voxel(slv.motion_to_dense_flow(best) * t_scale)
    aee = np.sqrt(((flow - V) ** 2).sum(0))[mask].mean()
    dof = 2 * slv.n_patch if hasattr(slv, "n_patch") else 2 * slv.total_n_patch
    return ("%-40s DoF %5d  optimize(): %.3f s (first call, then the same solver again: %s)  f/g/Hv callbacks %d/%d/%d  status %d  "
            "final loss %.5f  end-point error %.2f px" % (name, dof, min(times), ", ".join("%.3f" % t for t in times), nfev, njev, nhev,
                                                          results[-1].status, float(results[-1].fun), aee))


def main(out_path):
    ev, V, mask, t_scale = scene()
    aee0 = np.sqrt((V ** 2).sum(0))[mask].mean()
    lines = ["optimize() of the time-aware single-scale solver beside the pyramid solver: %d x %d, %d events, Burgers T = 10, Newton-CG max_iter 25"
             % (H, W, N),
             "device %s; end-point error of the zero flow: %.2f px; pyramid: patch.scale 5, crop 256 x 336, initialize random (seed 46); "
             "loss at x = 0: 4.0 (four focal ratios of 1)" % (torch.cuda.get_device_name(0), aee0), ""]
    lines.append(run("pyramid (scales 1..4)", "pyramidal_patch_contrast_maximization",
                     {"initialize": "random", "scale": 5, "crop_height": 256, "crop_width": 336, "filter_type": "bilinear"}, ev, V, mask, t_scale))
    for size, sw in ((16, 16), (16, 8)):
        for filt in ("bilinear", "nearest"):
            for start in ("zero", "random", "global-best"):
                lines.append(run(f"single scale {size}/{sw} {filt} {start}", "time_aware_mixed_patch_contrast_maximization",
                                 {"initialize": start, "size": size, "sliding_window": sw, "filter_type": filt}, ev, V, mask, t_scale))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mixed_solver.txt"))
