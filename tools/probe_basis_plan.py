#!/usr/bin/env python
"""Cost of the flow-basis plan (cmax_basis_plan_create + cmax_patch_plan_evaluate / _hvp / _descend; solver.FlowBasisObjective) for the
affine model, K = 6, against what a caller had before it and against the floor:
    plan        one library call per value + gradient / per product (value_and_grad_numpy, hvp_numpy)
    chained     FlowBasisObjective.__call__ + torch.autograd.grad: functional.basis_to_dense -> ContrastObjective, one Python-level call per stage
    einsum      the same objective as it could be written before the feature existed: torch.einsum -> ContrastObjective("dense-flow") -> autograd
                (neither chained route has an exact product through the map: theirs is the difference quotient of two gradients)
    floor       a bare cmax_objective / cmax_objective_hvp on the dense flow (CMaxHandle.evaluate / .hvp): no map at all
    Adam        microseconds per iteration of `descend` (one call, n iterations) against the same loop driven from the host (one
                value_and_grad_numpy per iteration + the update in numpy)
on cfg2's sensor (260 x 346) with 1M events (image variance, sigma 1) and on the 30k-event YAML shape (multi-focal normalised gradient
magnitude, sigma 1).  Host clock around calls that end in a wait, after warm-up calls of the same shape.  Nothing here is a gate.
    python tools/probe_basis_plan.py [out.txt]              (GPU box; default profiles/basis_plan_cost.txt)
    python tools/probe_basis_plan.py --parity [out.txt]     runs tests/test_gpu_basis_plan.py and keeps the figures it prints
                                                            (default profiles/basis_plan_parity.txt)"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W = 260, 346
REPS, N_ADAM = 200, 500
DISPLACEMENT = (2.0, -1.5, 0.010, -0.006, 0.005, 0.012)  # theta * t_scale, flow_basis("affine") order: up to ~4 px at the sensor's corners
SHAPES = [("cfg2 sensor, 1M events, image_variance sigma 1", 1_000_000, "image_variance"),
          ("30k-event YAML shape, multi_focal_normalized_gradient_magnitude sigma 1", 30_000, "multi_focal_normalized_gradient_magnitude")]


def timed(fn, reps=REPS, warm=5):
    """Every call is followed by a wait for the device: the plan's calls end in one of their own, the others get torch's."""
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def adam_update(state, x, g, it, lr=0.05, b1=0.9, b2=0.999, eps=1e-8):
    import numpy as np
    state["m"] = b1 * state.get("m", 0.0) + (1 - b1) * g
    state["v"] = b2 * state.get("v", 0.0) + (1 - b2) * g * g
    t = it + 1
    return x - (lr / (1 - b1 ** t)) * state["m"] / (np.sqrt(state["v"]) / np.sqrt(1 - b2 ** t) + eps)


def cost(path):
    import numpy as np
    import torch
    import event_based_optical_flow_amd as E
    from event_based_optical_flow_amd import functional as Fn
    from event_based_optical_flow_amd.solver import FlowBasisObjective

    lines = ["Flow-basis plan, affine model (K = 6), 260 x 346, microseconds per call (tools/probe_basis_plan.py, MI355X; host clock around "
             f"{REPS} calls after 5 warm-up calls,", f"every call ends in a wait; Adam: {N_ADAM} iterations per call, 3 calls).  Not gated.", ""]
    for title, n, cost_name in SHAPES:
        ev = E.utils.generate_events(n, H, W, 0.0, 0.05, seed=46)
        h = E.CMaxHandle((H, W)).set_events(ev)
        t_scale = float(ev[:, 2].max() - ev[:, 2].min())
        obj = FlowBasisObjective(h, t_scale, "affine", cost=cost_name, blur_sigma=1.0)
        theta = np.array(DISPLACEMENT) / t_scale
        v = np.random.default_rng(1).normal(size=6)
        x = torch.tensor(theta, dtype=torch.float64, device="cuda", requires_grad=True)
        vt = torch.tensor(v, dtype=torch.float64, device="cuda")
        basis = obj.basis
        bare = E.ContrastObjective(h, "dense-flow", cost=cost_name, sigma=1.0)
        desc = bare.terms[0][2]
        flow = obj.dense_flow(x.detach()).float().contiguous()
        tangent = (Fn.basis_to_dense(vt, basis) * t_scale).float()
        tangent = (tangent / tangent.abs().max()).contiguous()

        def chained(point):
            (g,) = torch.autograd.grad(obj(point), point)
            return g

        def einsum(point):
            (g,) = torch.autograd.grad(bare(torch.einsum("k,kchw->chw", point, basis) * t_scale), point)
            return g

        def quotient(grad_fn):
            hstep = 1e-3 / float(vt.abs().max())
            return (grad_fn((x.detach() + hstep * vt).requires_grad_()) - grad_fn((x.detach() - hstep * vt).requires_grad_())) / (2 * hstep)

        rows = [
            ("value + gradient", timed(lambda: obj.value_and_grad_numpy(theta)), timed(lambda: chained(x)), timed(lambda: einsum(x)),
             timed(lambda: h.evaluate(desc, flow, want_grad=True))),
            ("product", timed(lambda: obj.hvp_numpy(theta, v)), timed(lambda: quotient(chained)), timed(lambda: quotient(einsum)),
             timed(lambda: h.hvp(desc, flow, tangent))),
        ]
        t0 = time.perf_counter()
        for _ in range(3):
            res = obj.descend(theta, method="Adam", n_iter=N_ADAM, lr=0.05, lr_step=N_ADAM)
        adam_dev = (time.perf_counter() - t0) / (3 * N_ADAM) * 1e6

        def host_loop():
            xh, state, loss = theta.copy(), {}, 0.0
            for it in range(N_ADAM):
                loss, g = obj.value_and_grad_numpy(xh)
                xh = adam_update(state, xh, g, it)
            return loss

        t0 = time.perf_counter()
        for _ in range(3):
            last = host_loop()
        adam_host = (time.perf_counter() - t0) / (3 * N_ADAM) * 1e6
        lines += [title, "                     plan     chained (basis_to_dense)   einsum + ContrastObjective   floor (bare dense flow)"]
        lines += [f"  {name:<17} {a:8.1f}   {b:12.1f}               {c:12.1f}                {d:12.1f}" for name, a, b, c, d in rows]
        lines += [f"  Adam iteration    descend {adam_dev:8.1f}   host-driven loop {adam_host:8.1f}   (last loss {res.loss_history[-1]:.6g} / {last:.6g})", ""]
        del obj
        h.close()
    lines += ["product, chained / einsum columns: the difference quotient of two chained gradients (those routes have no exact product through the map)."]
    text = "\n".join(lines) + "\n"
    open(path, "w").write(text)
    print(text)


def parity(path):
    run = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_basis_plan.py"), "-q", "-s", "-m", "gpu"], cwd=ROOT,
                         capture_output=True, text=True, timeout=900)
    figures = [line[line.index("[basis]"):] for line in run.stdout.splitlines() if "[basis]" in line]
    tail = run.stdout.strip().splitlines()[-1] if run.stdout.strip() else ""
    head = ["Flow-basis plan against its fp64 references: the figures tests/test_gpu_basis_plan.py prints before it asserts (tools/probe_basis_plan.py --parity, MI355X).",
            "Gates: leaf forward <= 1 rounding bound, adjoint <= 1e-12, plan loss / gradient / product <= 1e-4 (of the largest entry, and per max|B_k|),",
            "descent steps <= 1e-10.  The Newton-CG parameter error is recorded, not gated.", f"pytest: {tail}", ""]
    text = "\n".join(head + figures) + "\n"
    open(path, "w").write(text)
    print(text)
    sys.exit(run.returncode)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--parity"]
    if "--parity" in sys.argv:
        parity(args[0] if args else os.path.join(ROOT, "profiles", "basis_plan_parity.txt"))
    else:
        cost(args[0] if args else os.path.join(ROOT, "profiles", "basis_plan_cost.txt"))
