#!/usr/bin/env python
"""Cost and effect of the device-resident L-BFGS (cmax_patch_plan_lbfgs / cmax_objective_lbfgs: a budget of evaluations per library
call, every decision in k_lbfgs_step, one wait at the end).  Nothing is gated on these figures.
  1. microseconds per evaluation inside the call against the same plan's Adam iteration inside `descend` (the difference is
     k_lbfgs_step against k_descent_step), on the 30k-event YAML plan, cfg2's 2-DoF shape and the affine basis plan at 1M events; the
     one-pass Gram form (what ships) against the textbook two-loop form (CMAX_LBFGS_TWO_LOOP=1, read once per process: every variant
     runs in a child process of its own and the variants alternate);
  2. the same solve driven from the host: tests/_lbfgs_ref.minimize over value_and_grad_numpy, and SciPy's L-BFGS-B at the same budget;
  3. optimize() of the three solver classes with "Newton-CG" beside "device-L-BFGS" at several budgets: wall time and final loss.
Every figure is a host clock around calls that end in the library's own wait, after warm-up calls of the same shape.
    python tools/probe_lbfgs.py [out.txt]        (GPU box; default profiles/lbfgs_cost.txt)"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
H, W = 260, 346
N_EVAL, REPS, ROUNDS, HOST_ROUNDS = 512, 3, 2, 5
LBFGS = dict(history=8, gtol=0.0, max_move=400.0, step0=1.0, max_ls=10)
BUDGETS = (25, 50, 100, 200)


def timed(fn, reps=REPS, warm=1):
    for _ in range(warm):
        fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) / reps, out


def counts(res):
    return "%d accepted / %d rejected / %d reset / %d idle, %s" % tuple([int((res.code == c).sum()) for c in (1, 2, 3, 4)] + [res.status])


def yaml_plan():
    import numpy as np
    import event_based_optical_flow_amd as E
    from event_based_optical_flow_amd.solver import PatchFlowObjective
    from probe_mixed_solver import scene

    ev, _, _, t_scale = scene()  # 30k events of dots moving along a smooth flow: the contrast has curvature
    h = E.CMaxHandle((H, W)).set_events(ev)
    plan = PatchFlowObjective(h, t_scale, (16, 16), (16, 21), (16, 21), (2, 5), cost="hybrid",
                              cost_with_weight={"multi_focal_normalized_gradient_magnitude": 1.0, "total_variation": 0.01}, blur_sigma=1)
    return h, plan, np.random.default_rng(0).uniform(-20, 20, 512)


def live_pair(descend, lbfgs):
    """A pilot solve finds how many evaluations are live (an evaluation behind a termination is idle: its step runs neither reduction form);
    Adam and L-BFGS are then timed at THAT budget, so both figures carry the same per-call overhead.  -> (n, adam us, lbfgs us, result)"""
    pilot = lbfgs(N_EVAL)
    n = pilot.nfev - 1 if pilot.status != "BUDGET" else N_EVAL  # (the terminating evaluation excluded: every timed evaluation steps)
    reps = max(REPS, min(40, (4 * N_EVAL) // n))
    sec_a, _ = timed(lambda: descend(n), reps=reps)
    sec_l, res = timed(lambda: lbfgs(n), reps=reps)
    return n, sec_a / n * 1e6, sec_l / n * 1e6, res


def child_cost():
    import numpy as np
    import event_based_optical_flow_amd as E
    from event_based_optical_flow_amd.solver import FlowBasisObjective

    out = {"two_loop": "CMAX_LBFGS_TWO_LOOP" in os.environ}
    h, plan, x0 = yaml_plan()
    n, a, l, res = live_pair(lambda n: plan.descend(x0, method="Adam", n_iter=n, lr=0.05, lr_step=n), lambda n: plan.minimize_lbfgs(x0, n_eval=n, **LBFGS))
    out["plan"] = dict(n=n, adam_us=a, lbfgs_us=l, counts=counts(res), loss=[float(res.loss_history[0]), res.fun])
    h.close()
    ev = E.utils.generate_events(1_000_000, H, W, 0.0, 0.05, seed=46)  # cfg2's shape, as tools/probe_descent.py
    h = E.CMaxHandle((H, W)).set_events(ev)
    obj = E.ContrastObjective(h, "2d-translation", cost="image_variance")
    theta0 = np.array([12.3, -7.7])
    n, a, l, res = live_pair(lambda n: obj.descend(theta0, method="Adam", n_iter=n, lr=0.05, lr_step=n),
                             lambda n: obj.minimize_lbfgs(theta0, n_eval=n, **dict(LBFGS, max_move=20.0)))
    out["two_dof"] = dict(n=n, adam_us=a, lbfgs_us=l, counts=counts(res), loss=[float(res.loss_history[0]), res.fun])
    basis = FlowBasisObjective(h, 0.05, "affine", cost="image_variance")
    t0 = np.array([40.0, -30.0, 1.0, -2.0, 0.5, 1.5])
    n, a, l, res = live_pair(lambda n: basis.descend(t0, method="Adam", n_iter=n, lr=0.05, lr_step=n),
                             lambda n: basis.minimize_lbfgs(t0, n_eval=n, **dict(LBFGS, max_move=50.0)))
    out["basis"] = dict(n=n, adam_us=a, lbfgs_us=l, counts=counts(res), loss=[float(res.loss_history[0]), res.fun])
    del basis
    h.close()
    print("PROBE " + json.dumps(out))


def child_host():
    import scipy.optimize

    import _lbfgs_ref as R

    out = {}
    h, plan, x0 = yaml_plan()
    for n in (64, 256):
        kw = dict(LBFGS, n_eval=n)
        solves = {
            "device": lambda: plan.minimize_lbfgs(x0, **kw),
            "ref": lambda: R.minimize(plan.value_and_grad_numpy, x0, R.descriptor(**kw)),
            "scipy": lambda: scipy.optimize.minimize(plan.value_and_grad_numpy, x0, jac=True, method="L-BFGS-B",
                                                     options={"maxfun": n, "maxiter": n, "maxcor": 8, "gtol": 0.0, "ftol": 0.0}),
        }
        ms, last = {k: [] for k in solves}, {}
        for rnd in range(HOST_ROUNDS + 1):  # the three alternate; the first round warms up
            for k, fn in solves.items():
                t0 = time.perf_counter()
                last[k] = fn()
                if rnd:
                    ms[k].append((time.perf_counter() - t0) * 1e3)
        out[str(n)] = dict(device_ms=[min(ms["device"]), max(ms["device"])], device_loss=last["device"].fun, device_nit=last["device"].nit,
                           ref_ms=[min(ms["ref"]), max(ms["ref"])], ref_loss=last["ref"]["fun"], ref_nit=last["ref"]["nit"],
                           scipy_ms=[min(ms["scipy"]), max(ms["scipy"])], scipy_loss=float(last["scipy"].fun), scipy_nfev=int(last["scipy"].nfev))
    out["loss0"] = float(plan.value_and_grad_numpy(x0)[0])
    h.close()
    print("PROBE " + json.dumps(out))


def child_solvers():
    import numpy as np
    import torch
    from event_based_optical_flow_amd import solver
    from probe_mixed_solver import scene

    ev, _, _, _ = scene()
    common = {"motion_model": "2d-translation", "warp_direction": "first", "parameters": ["trans_x", "trans_y"], "cost": "hybrid", "outer_padding": 0,
              "cost_with_weight": {"multi_focal_normalized_gradient_magnitude": 1.0, "total_variation": 0.01}, "iwe": {"method": "bilinear_vote", "blur_sigma": 1}}
    kinds = {
        "pyramid": ("pyramidal_patch_contrast_maximization", dict(time_aware=False, patch={"initialize": "random", "scale": 5, "crop_height": 256,
                                                                                          "crop_width": 336, "filter_type": "bilinear"})),
        "mixed": ("mixed_patch_contrast_maximization", dict(time_aware=False, patch={"initialize": "random", "size": 16, "sliding_window": 16, "filter_type": "bilinear"})),
        "time-aware": ("time_aware_mixed_patch_contrast_maximization", dict(time_aware=True, time_bin=10, flow_interpolation="burgers", t0_flow_location="middle",
                                                                            patch={"initialize": "random", "size": 16, "sliding_window": 16, "filter_type": "bilinear"})),
    }
    out = {}
    for kind, (name, extra) in kinds.items():
        cls = solver.collections[name] if name in solver.collections else solver.MixedPatchContrastMaximization
        variants = [("Newton-CG", 25)] + [("device-L-BFGS", b) for b in BUDGETS]
        slvs = []
        for method, budget in variants:
            opt = {"n_iter": budget, "method": method, "max_iter": 25, "lbfgs": {"max_move": 400.0},
                   "parameters": {"trans_x": {"min": -150, "max": 150}, "trans_y": {"min": -150, "max": 150}}}
            if method != "device-L-BFGS":
                opt.pop("lbfgs")
            slvs.append(cls((H, W), {}, dict(common, method=name, **extra), opt, {}, None))
        times = [[] for _ in variants]
        for rep in range(REPS + 1):  # the variants alternate; the first round warms up
            for i, slv in enumerate(slvs):
                np.random.seed(46)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                slv.optimize(ev)
                torch.cuda.synchronize()
                if rep:
                    times[i].append((time.perf_counter() - t0) * 1e3)
        rows = []
        for (method, budget), slv, t in zip(variants, slvs, times):
            last = slv.history[-1][1] if kind == "pyramid" else slv.history[-1]
            rows.append(dict(method=method, budget=budget, ms=[min(t), max(t)], loss=float(last.fun), status=str(getattr(last, "status", ""))))
        out[kind] = rows
    print("PROBE " + json.dumps(out))


def run_child(flag, env):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), flag], env=env, capture_output=True, text=True, timeout=500)
    line = [l for l in p.stdout.splitlines() if l.startswith("PROBE ")]
    if p.returncode or not line:
        sys.exit(f"child {flag} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-3000:]}")
    return json.loads(line[0][6:])


def main(path):
    base = dict(os.environ)
    base.pop("CMAX_LBFGS_TWO_LOOP", None)
    runs = []
    for _ in range(ROUNDS):
        for two_loop in (False, True):
            runs.append(run_child("--cost", dict(base, CMAX_LBFGS_TWO_LOOP="1") if two_loop else base))
    host = run_child("--host", base)
    slv = run_child("--solvers", base)
    lines = [
        "Device-resident L-BFGS (tools/probe_lbfgs.py, MI355X; host clock around calls that end in the library's own wait, after a warm-up call; history 8,",
        "gtol 0; every line of the first table is one child process, the one-pass Gram form and the two-loop form alternate).",
        "",
        "1. microseconds per LIVE evaluation inside the call: a pilot solve of %d evaluations finds the budget n at which no evaluation is idle (an" % N_EVAL,
        "   evaluation behind a termination runs neither reduction form); Adam inside `descend` (n iterations) | L-BFGS inside `minimize_lbfgs` (n evaluations),",
        "   both timed at that n over max(%d, 4 * %d / n) calls, so both carry the same per-call overhead (one wait, the copies in and out)" % (REPS, N_EVAL),
        "form of k_lbfgs_step       | 30k-event YAML plan (512 DoF)   | cfg2 shape, 2-DoF (1M events)   | affine basis plan, 1M events (6 DoF)",
        "                           |    n     Adam   L-BFGS          |    n     Adam   L-BFGS          |    n     Adam   L-BFGS",
    ]
    for r in runs:
        lines.append("%-26s | %4d  %7.2f  %7.2f          | %4d  %7.2f  %7.2f          | %4d  %7.2f  %7.2f" % (
            "two-loop (2k+1 reductions)" if r["two_loop"] else "one-pass Gram (ships)", r["plan"]["n"], r["plan"]["adam_us"], r["plan"]["lbfgs_us"],
            r["two_dof"]["n"], r["two_dof"]["adam_us"], r["two_dof"]["lbfgs_us"], r["basis"]["n"], r["basis"]["adam_us"], r["basis"]["lbfgs_us"]))
    for r in runs[:2]:
        lines.append("   %s, the timed solves: plan %s, loss %.5f -> %.5f; 2-DoF %s, loss %.5f -> %.5f; basis %s, loss %.5f -> %.5f" % (
            "two-loop" if r["two_loop"] else "Gram", r["plan"]["counts"], *r["plan"]["loss"], r["two_dof"]["counts"], *r["two_dof"]["loss"],
            r["basis"]["counts"], *r["basis"]["loss"]))
    lines += ["   (the 2-DoF Adam column runs the fused finishing kernel k_finish_raw_step; L-BFGS takes the general sequence and a step launch; where n is",
              "   small the per-call overhead is a large part of both figures: read the DIFFERENCE of a row's two columns, and the two forms against each other)", "",
              "2. the same solve on the YAML plan driven from the host, milliseconds per solve (min .. max of %d rounds in which the three alternate, after a" % HOST_ROUNDS,
              "   warm-up round) and final loss (loss at x0 %.5f)" % host["loss0"],
              "budget | device-resident | tests/_lbfgs_ref.minimize over value_and_grad_numpy | SciPy L-BFGS-B (maxcor 8, maxfun = budget)"]
    for n in ("64", "256"):
        r = host[n]
        lines.append("%6s | %6.2f .. %6.2f ms  loss %.5f (%d steps) | %6.2f .. %6.2f ms  loss %.5f (%d steps) | %6.2f .. %6.2f ms  loss %.5f (%d evaluations)" % (
            n, *r["device_ms"], r["device_loss"], r["device_nit"], *r["ref_ms"], r["ref_loss"], r["ref_nit"], *r["scipy_ms"], r["scipy_loss"], r["scipy_nfev"]))
    lines += ["", "3. optimize() of the solver classes on the 30k-event scene of tools/probe_mixed_solver.py (initialize random, seed 46), milliseconds (min .. max of %d" % REPS,
              "alternating runs) and the final loss of the finest scale; Newton-CG: max_iter 25; device-L-BFGS: optimizer.n_iter = budget per scale, max_move 400"]
    for kind, rows in slv.items():
        for r in rows:
            lines.append("%-11s %-14s budget %4d | %8.2f .. %8.2f ms | final loss %.5f %s" % (kind, r["method"], r["budget"], r["ms"][0], r["ms"][1], r["loss"], r["status"]))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write(text)
    print(text)


if __name__ == "__main__":
    if "--cost" in sys.argv:
        child_cost()
    elif "--host" in sys.argv:
        child_host()
    elif "--solvers" in sys.argv:
        child_solvers()
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "lbfgs_cost.txt"))
