#!/usr/bin/env python
"""Records of the flow regulariser (cmax_patch_plan_set_flow_regularizer; functional.flow_regularizer).  Nothing here is a gate.
    python tools/probe_flow_regularizer.py [out.txt]             cost (default profiles/flow_regularizer_cost.txt): microseconds per
        evaluate, product and Adam iteration of a plan with the term against THE SAME PLAN without it on the same handle (the term is set and
        removed between the timed blocks), at the 30k-event YAML patch plan (16 x 16 patches, hybrid + TV) and at the affine basis plan
        with 1M events, both at 260 x 346; beside them the torch route a caller had before: autograd through functional.patch_to_dense /
        basis_to_dense and a torch restatement of the term, value + gradient of the term alone
    python tools/probe_flow_regularizer.py --parity [out.txt]    runs tests/test_gpu_flow_regularizer.py and keeps the figures it prints
        (default profiles/flow_regularizer_parity.txt)
    python tools/probe_flow_regularizer.py --collapse [out.txt]  events of a pure translation, the similarity basis, Adam from a contracted
        zoom: final zoom and loss without the term and with the area term at two weights (default profiles/flow_regularizer_collapse.txt)
Host clock around calls that end in a wait, after warm-up calls of the same shape."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W = 260, 346
REPS, N_ADAM = 200, 300
AFFINE = (2.0, -1.5, 0.010, -0.006, 0.005, 0.012)  # theta * t_scale, flow_basis("affine") order (tools/probe_basis_plan.py)
REGS = [dict(kind="divergence", weight=0.1, eps=1e-3), dict(kind="area", weight=0.1, eps=1e-3, s=1.0)]


def timed(fn, reps=REPS, warm=5):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def torch_term(flow, kind, eps, s):
    """The term in plain torch ops on the device: what a caller could write without the kernels."""
    import torch
    a = 0.5 * (flow[0, 2:, 1:-1] - flow[0, :-2, 1:-1])
    b = 0.5 * (flow[0, 1:-1, 2:] - flow[0, 1:-1, :-2])
    c = 0.5 * (flow[1, 2:, 1:-1] - flow[1, :-2, 1:-1])
    d = 0.5 * (flow[1, 1:-1, 2:] - flow[1, 1:-1, :-2])
    psi = (lambda u: torch.sqrt(u * u + eps * eps) - eps)
    if kind == "divergence":
        return psi(a + d).mean()
    tr, det = a + d, a * d - b * c
    return 0.5 * (psi(-s * tr + s * s * det) + psi(s * tr + s * s * det)).mean()


def plan_rows(obj, x, v, with_tv=None):
    kw = {} if with_tv is None else {"with_tv": with_tv}
    t_eval = timed(lambda: obj.value_and_grad_numpy(x))
    t_hvp = timed(lambda: obj.hvp_numpy(x, v))
    t0 = time.perf_counter()
    for _ in range(3):
        obj.descend(x, method="Adam", n_iter=N_ADAM, lr=0.05, lr_step=N_ADAM, **kw)
    return t_eval, t_hvp, (time.perf_counter() - t0) / (3 * N_ADAM) * 1e6


def cost(path):
    import numpy as np
    import torch
    import event_based_optical_flow_amd as E
    from event_based_optical_flow_amd import functional as Fn
    from event_based_optical_flow_amd.solver import FlowBasisObjective, PatchFlowObjective

    lines = ["Flow regulariser on a plan, 260 x 346, microseconds per call (tools/probe_flow_regularizer.py, MI355X; host clock around "
             f"{REPS} calls after 5 warm-up calls,", f"every call ends in a wait; Adam: {N_ADAM} iterations per descend call, 3 calls).  The plan "
             "without the term is the same plan on the same handle, the term removed.  Not gated.", ""]

    def block(title, obj, x, v, field_of):
        rows = [("without the term",) + plan_rows(obj, x, v)]
        for reg in REGS:
            obj.set_flow_regularizer(reg)
            rows.append((f"{reg['kind']} (eps {reg['eps']:g})",) + plan_rows(obj, x, v))
        obj.set_flow_regularizer(None)
        rows.append(("without, again",) + plan_rows(obj, x, v))
        out = [title, "                          value + gradient    product    Adam iteration (descend)"]
        out += [f"  {name:<24} {a:10.1f}      {b:8.1f}     {c:8.1f}" for name, a, b, c in rows]
        xt = torch.tensor(x, dtype=torch.float64, device="cuda", requires_grad=True)
        for reg in REGS:
            kind, eps, s = reg["kind"], reg["eps"], reg.get("s", 1.0)
            t_kernel = timed(lambda: torch.autograd.grad(Fn.flow_regularizer(field_of(xt), kind, eps, s), xt))
            t_torch = timed(lambda: torch.autograd.grad(torch_term(field_of(xt), kind, eps, s), xt))
            out.append(f"  the term alone through autograd on the map, value + gradient, {kind}: functional.flow_regularizer {t_kernel:8.1f}   "
                       f"torch ops {t_torch:8.1f}")
        return out + [""]

    ev = E.utils.generate_events(30000, H, W, 0.0, 0.05, seed=46)
    h = E.CMaxHandle((H, W)).set_events(ev)
    plan = PatchFlowObjective(h, 0.05, (16, 16), (16, 21), (16, 21), (2, 5), cost="hybrid",
                              cost_with_weight={"multi_focal_normalized_gradient_magnitude": 1.0, "total_variation": 0.01}, blur_sigma=1)
    rng = np.random.default_rng(2)
    x = rng.normal(0.0, 40.0, 512)
    lines += block("30k-event YAML patch plan (16 x 16 patches, hybrid + TV, 512 unknowns)", plan, x, rng.normal(size=512), plan.flow_field)
    del plan
    h.close()
    ev = E.utils.generate_events(1_000_000, H, W, 0.0, 0.05, seed=46)
    h = E.CMaxHandle((H, W)).set_events(ev)
    t_scale = float(ev[:, 2].max() - ev[:, 2].min())
    basis = FlowBasisObjective(h, t_scale, "affine", cost="image_variance", blur_sigma=1.0)
    lines += block("affine basis plan (K = 6), 1M events, image_variance sigma 1", basis, np.array(AFFINE) / t_scale, rng.normal(size=6), basis.flow_field)
    del basis
    h.close()
    text = "\n".join(lines) + "\n"
    open(path, "w").write(text)
    print(text)


def parity(path):
    run = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_flow_regularizer.py"), "-q", "-s", "-m", "gpu"], cwd=ROOT,
                         capture_output=True, text=True, timeout=900)
    figures = [line[line.index("[flowreg]"):] for line in run.stdout.splitlines() if "[flowreg]" in line]
    tail = run.stdout.strip().splitlines()[-1] if run.stdout.strip() else ""
    head = ["Flow regulariser against its fp64 references: the figures tests/test_gpu_flow_regularizer.py prints before it asserts "
            "(tools/probe_flow_regularizer.py --parity, MI355X).",
            "Gates: leaf value / gradient / product <= 1e-10 on fp64 fields and <= 1e-4 on fp32 fields (of the largest entry); plan loss / gradient / "
            "product <= 1e-4;", "descent steps <= 1e-10, loss history <= 1e-12.", f"pytest: {tail}", ""]
    text = "\n".join(head + figures) + "\n"
    open(path, "w").write(text)
    print(text)
    sys.exit(run.returncode)


def collapse(path):
    """Not gated, and no statement about end-point error (there is no dataset here): what the term does to the zoom of a similarity model
    on events that hold none."""
    import numpy as np
    import event_based_optical_flow_amd as E
    from event_based_optical_flow_amd.solver import FlowBasisObjective

    size, n, period, motion = (68, 90), 6000, 0.05, (4.0, -3.0)
    ev = E.utils.generate_structured_events(n, size[0], size[1], motion, n_dots=60, tmin=0.0, tmax=period, seed=5)
    ev = np.ascontiguousarray(ev[np.argsort(ev[:, 2], kind="stable")])
    t_scale = float(ev[:, 2].max() - ev[:, 2].min())
    h = E.CMaxHandle(size).set_events(ev)
    obj = FlowBasisObjective(h, t_scale, "similarity", cost="image_variance", blur_sigma=1.0)
    # flow_basis("similarity"): translation (2), zoom, rotation; D = b + z (r, c) + ..., warped by x' = x - dt D: z > 0 contracts
    truth = np.array([motion[0], motion[1], 0.0, 0.0]) / period
    lines = [f"Event collapse on a similarity model (tools/probe_flow_regularizer.py --collapse, MI355X): {len(ev)} events of a pure translation {motion} px over the",
             f"batch on {size[0]} x {size[1]}, image_variance sigma 1 (minimised: -variance), Adam 400 iterations lr 0.05 from the true translation with a zoom of",
             "z0 x t_scale per batch.  theta x t_scale is printed: translation in px over the batch, zoom and rotation in px per px.  Recorded, not gated; the",
             "effect on end-point error is not measured (no dataset).", ""]
    at_truth = obj.value_and_grad_numpy(truth)[0]
    lines.append(f"contrast loss at the true motion (zoom 0): {at_truth:.6f}")
    for z0 in (0.2, 0.5):
        start = truth + np.array([0.0, 0.0, z0 / t_scale, 0.0])
        lines += ["", f"start zoom {z0:+.2f}: contrast loss {obj.value_and_grad_numpy(start)[0]:.6f}",
                  "  term                      final translation      zoom      rotation    total loss    contrast loss     R(area)"]
        for weight in (None, 1.0, 10.0):
            obj.set_flow_regularizer(None if weight is None else dict(kind="area", weight=weight, eps=1e-3, s=1.0))
            res = obj.descend(start, method="Adam", n_iter=400, lr=0.05, lr_step=400)
            total = obj.value_and_grad_numpy(res.x_last)[0]
            obj.set_flow_regularizer(None)
            contrast = obj.value_and_grad_numpy(res.x_last)[0]
            obj.set_flow_regularizer(dict(kind="area", weight=1.0, eps=1e-3, s=1.0))
            r_area = obj.value_and_grad_numpy(res.x_last)[0] - contrast
            obj.set_flow_regularizer(None)
            th = res.x_last * t_scale
            name = "none" if weight is None else f"area, weight {weight:g}"
            lines.append(f"  {name:<24} ({th[0]:+7.3f}, {th[1]:+7.3f})   {th[2]:+8.4f}   {th[3]:+8.4f}   {total:11.6f}   {contrast:11.6f}   {r_area:10.6f}")
    del obj
    h.close()
    text = "\n".join(lines) + "\n"
    open(path, "w").write(text)
    print(text)


if __name__ == "__main__":
    flags = [a for a in sys.argv[1:] if a.startswith("--")]
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--parity" in flags:
        parity(args[0] if args else os.path.join(ROOT, "profiles", "flow_regularizer_parity.txt"))
    elif "--collapse" in flags:
        collapse(args[0] if args else os.path.join(ROOT, "profiles", "flow_regularizer_collapse.txt"))
    else:
        cost(args[0] if args else os.path.join(ROOT, "profiles", "flow_regularizer_cost.txt"))
