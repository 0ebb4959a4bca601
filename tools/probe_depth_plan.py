#!/usr/bin/env python
"""Cost of the depth plan (cmax_depth_plan_create + cmax_patch_plan_evaluate / _hvp / _descend; solver.DepthEgoMotionObjective) with the
camera bases (Ka = Kb = 3) over a 16 x 16 grid of inverse depth, beside what it is compared with:
    plan        one library call per value + gradient / per product (value_and_grad_numpy, hvp_numpy)
    chained     the same objective's autograd-chained path: DepthEgoMotionObjective.__call__ + torch.autograd.grad (functional.depth_to_dense
                -> ContrastObjective, one Python-level call per stage; it has no exact product: the difference quotient of two gradients)
    basis plan  solver.FlowBasisObjective with the six fields [A | B] on the same batch: the linear map this change leaves as it was
    Adam        microseconds per iteration of `descend` (one call, n iterations)
on cfg2's sensor (260 x 346) with 1M events (image variance, sigma 1) and on the 30k-event YAML shape (multi-focal normalised gradient
magnitude, sigma 1).  Time: HIP events around windows of calls, as bench.py takes it (every window between synchronisations, the MEDIAN
window reported), after warm-up calls of the same shape.  Nothing here is a gate.
    python tools/probe_depth_plan.py [out.txt]              (GPU box; default profiles/depth_plan_cost.txt)
    python tools/probe_depth_plan.py --parity [out.txt]     runs tests/test_gpu_depth_plan.py and keeps the worst figure per test family
                                                            (default profiles/depth_plan_parity.txt)"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W = 260, 346
GRID, WINDOW_SW = (16, 16), (16, 21)  # 16 x 16 cells of 16 x 21 pixels (+ one cell of padding): the YAML grid of the patch solver
STEPS, WINDOWS, N_ADAM = 100, 5, 500
CALIB = (400.0, 400.0, (W - 1) / 2.0, (H - 1) / 2.0)
A_DISP, B_DISP = (3.0, -2.0, 1.0), (0.5, -0.4, 0.6)  # px over the batch at the focal length / at unit image coordinates, rho around 1
SHAPES = [("cfg2 sensor, 1M events, image_variance sigma 1", 1_000_000, "image_variance"),
          ("30k-event YAML shape, multi_focal_normalized_gradient_magnitude sigma 1", 30_000, "multi_focal_normalized_gradient_magnitude")]


def timed(fn, steps=STEPS, windows=WINDOWS, warm=5):
    """Median over `windows` of (HIP-event time of `steps` calls) / steps, in microseconds."""
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(windows):
        torch.cuda.synchronize()
        ev0.record()
        for _ in range(steps):
            fn()
        ev1.record()
        torch.cuda.synchronize()
        out.append(ev0.elapsed_time(ev1) * 1e3 / steps)
    return sorted(out)[len(out) // 2]


def cost(path):
    import numpy as np
    import torch
    import event_based_optical_flow_amd as E
    from event_based_optical_flow_amd.solver import DepthEgoMotionObjective, FlowBasisObjective

    lines = [f"Depth plan, camera bases (Ka = Kb = 3), grid {GRID[0]} x {GRID[1]} (nx = {6 + GRID[0] * GRID[1]}), {H} x {W}, microseconds per call "
             f"(tools/probe_depth_plan.py, MI355X;", f"HIP events around {WINDOWS} windows of {STEPS} calls after 5 warm-up calls, median window; Adam: "
             f"{N_ADAM} iterations per call, 3 calls).  Not gated.", ""]
    A, B = E.utils.motion_field_basis((H, W), CALIB)
    for title, n, cost_name in SHAPES:
        ev = E.utils.generate_events(n, H, W, 0.0, 0.05, seed=46)
        h = E.CMaxHandle((H, W)).set_events(ev)
        t_scale = float(ev[:, 2].max() - ev[:, 2].min())
        obj = DepthEgoMotionObjective(h, t_scale, GRID, WINDOW_SW, WINDOW_SW, calib=CALIB, cost=cost_name, blur_sigma=1.0)
        rng = np.random.default_rng(1)
        a, b = np.array(A_DISP) / CALIB[0] / t_scale, np.array(B_DISP) / CALIB[0] / t_scale
        x0 = np.concatenate([a, b, rng.uniform(0.6, 1.4, GRID[0] * GRID[1])])
        v = rng.normal(size=x0.size)
        xt = torch.tensor(x0, dtype=torch.float64, device="cuda", requires_grad=True)
        vt = torch.tensor(v, dtype=torch.float64, device="cuda")
        basis = FlowBasisObjective(h, t_scale, np.concatenate([A, B]), cost=cost_name, blur_sigma=1.0)
        theta = np.concatenate([a, b])
        vb = v[:6]

        def chained(point):
            (g,) = torch.autograd.grad(obj(point), point)
            return g

        def quotient():
            hstep = 1e-3 / float(vt.abs().max())
            return (chained((xt.detach() + hstep * vt).requires_grad_()) - chained((xt.detach() - hstep * vt).requires_grad_())) / (2 * hstep)

        rows = [("value + gradient", timed(lambda: obj.value_and_grad_numpy(x0)), timed(lambda: chained(xt)), timed(lambda: basis.value_and_grad_numpy(theta))),
                ("product", timed(lambda: obj.hvp_numpy(x0, v)), timed(quotient), timed(lambda: basis.hvp_numpy(theta, vb)))]
        adam = {}
        for name, o, start in (("depth", obj, x0), ("basis", basis, theta)):
            o.descend(start, method="Adam", n_iter=N_ADAM, lr=1e-3, lr_step=N_ADAM)  # warm-up: the descent's buffers
            torch.cuda.synchronize()
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(3):
                res = o.descend(start, method="Adam", n_iter=N_ADAM, lr=1e-3, lr_step=N_ADAM)
            ev1.record()
            torch.cuda.synchronize()
            adam[name] = (ev0.elapsed_time(ev1) * 1e3 / (3 * N_ADAM), res.loss_history[0], res.loss_history[-1])
        lines += [title, "                     depth plan   chained (depth_to_dense)   basis plan, 6 fields"]
        lines += [f"  {name:<17} {p:10.1f}   {c:12.1f}             {q:12.1f}" for name, p, c, q in rows]
        lines += [f"  Adam iteration    {adam['depth'][0]:10.1f}   {'-':>12}             {adam['basis'][0]:12.1f}   (depth: loss {adam['depth'][1]:.6g} -> "
                  f"{adam['depth'][2]:.6g}; basis: {adam['basis'][1]:.6g} -> {adam['basis'][2]:.6g})", ""]
        del obj, basis
        h.close()
    lines += ["product, chained column: the difference quotient of two chained gradients (that route has no exact product through the map).",
              "basis plan column: FlowBasisObjective on the fields [A | B], measured in the same process; its kernels and its launch sequence are the",
              "parent commit's (profiles/depth_plan_resources.txt: no kernel of the unit changed)."]
    text = "\n".join(lines) + "\n"
    open(path, "w").write(text)
    print(text)


def parity(path):
    run = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_depth_plan.py"), "-q", "-s", "-m", "gpu"], cwd=ROOT,
                         capture_output=True, text=True, timeout=900)
    figures = [line[line.index("[depth]"):] for line in run.stdout.splitlines() if "[depth]" in line]
    figures += [line[line.index("[lbfgs]"):] for line in run.stdout.splitlines() if "[lbfgs] depth" in line]
    families = {}  # the word behind the tag names the family (leaf lines: with their dtype); its worst figure is the largest LABELLED error
    labelled = re.compile(r"(?:forward|tangent|adjoint2?|backward|loss|grad|Hv|error|history|alpha)\s+(\d\.\d+e[-+]\d+)")
    for line in figures:
        words = line.split(":")[0].split()
        family = "lbfgs rule" if words[0] == "[lbfgs]" else words[1] + (" " + words[-1] if words[1] == "leaf" and words[-1].startswith("float") else "") + (" (worst)" if "worst" in words else "")
        nums = [float(m) for m in labelled.findall(line.split(":", 1)[1] if ":" in line else "")]
        if nums and "worst" not in words:
            families[family] = max(families.get(family, 0.0), max(nums))
    tail = run.stdout.strip().splitlines()[-1] if run.stdout.strip() else ""
    head = ["Depth plan against its fp64 references: the figures tests/test_gpu_depth_plan.py prints before it asserts (tools/probe_depth_plan.py --parity, MI355X).",
            "Gates: fp64 leaf 1e-10, fp32 leaf 1e-4, plan loss / gradient / product 1e-4 (of the largest entry: of the whole vector and of each block a, b, s),",
            "descent steps 1e-10, L-BFGS trial points 1e-9.  The recovery scene: loss lower, mean end-point error below half the start's.", f"pytest: {tail}", "",
            "worst figure per family (the largest error any line of the family prints):"]
    head += [f"  {k:<40} {v:.2e}" for k, v in sorted(families.items())] + ["", "every line:"]
    text = "\n".join(head + figures) + "\n"
    open(path, "w").write(text)
    print(text)
    sys.exit(run.returncode)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--parity"]
    if "--parity" in sys.argv:
        parity(args[0] if args else os.path.join(ROOT, "profiles", "depth_plan_parity.txt"))
    else:
        cost(args[0] if args else os.path.join(ROOT, "profiles", "depth_plan_cost.txt"))
