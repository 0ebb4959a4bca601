#!/usr/bin/env python
"""Cost of one iteration of the device-resident descent (cmax_objective_descend / cmax_patch_plan_descend: n iterations per library
call, one wait at the end) against the same Adam loop driven from the host, one evaluation per call:
    cfg2's shape: 1M events, 260 x 346, 2-DoF image variance   -- host loop: cmax_objective_host + numpy Adam + theta to the device;
                  at lr 0.05 (theta walks to the optimum) and at lr 1e-12 (theta stays where bench.py evaluates)
    the 30k-event YAML plan: 16 x 16 patches, hybrid + TV      -- host loop: cmax_patch_plan_evaluate + numpy Adam
and, for the 2-DoF entry, the fused finishing kernel (k_finish_raw_step) against the separate finish + step launches
(CMAX_DESCENT_NO_FUSED_STEP=1, read once per process: each variant runs in a child process of its own, the variants alternate).
Every figure is a host clock around calls that end in the library's own wait, after warm-up calls of the same shape; the timed window of
each figure is at least REPS calls of N iterations.
    python tools/probe_descent.py [out.txt]        (GPU box; default profiles/descent_cost.txt)"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W = 260, 346
N_2DOF, N_PLAN, REPS, ROUNDS = 4096, 1000, 5, 2
ADAM = dict(lr=0.05, b1=0.9, b2=0.999, eps=1e-8)
FIXED_LR = 1e-12


def adam_update(state, x, g, it, lr=ADAM["lr"]):
    import numpy as np
    state["m"] = ADAM["b1"] * state.get("m", 0.0) + (1 - ADAM["b1"]) * g
    state["v"] = ADAM["b2"] * state.get("v", 0.0) + (1 - ADAM["b2"]) * g * g
    t = it + 1
    return x - (lr / (1 - ADAM["b1"] ** t)) * state["m"] / (np.sqrt(state["v"]) / np.sqrt(1 - ADAM["b2"] ** t) + ADAM["eps"])


def timed(fn, reps=REPS, warm=2):
    for _ in range(warm):
        fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) / reps, out


def child():
    import numpy as np
    import torch
    import event_based_optical_flow_amd as E
    from event_based_optical_flow_amd.solver import PatchFlowObjective

    out = {"fused_step": "CMAX_DESCENT_NO_FUSED_STEP" not in os.environ}
    # ---- row 1: cfg2's shape
    ev = E.utils.generate_events(1_000_000, H, W, 0.0, 0.05, seed=46)
    h = E.CMaxHandle((H, W)).set_events(ev)
    obj = E.ContrastObjective(h, "2d-translation", cost="image_variance")
    theta0 = np.array([12.3, -7.7])
    theta_dev = torch.tensor(theta0, dtype=torch.float64, device="cuda")
    call, result, grad = h.prepare_host(obj.terms[0][2], theta_dev)

    def host_loop(lr):
        x, state, hist = theta0.copy(), {}, []
        for it in range(N_2DOF):
            call.motion.copy_(torch.from_numpy(x))
            call()
            hist.append(result[0])
            x = adam_update(state, x, grad, it, lr)
        return x, hist

    # lr 0.05: theta walks to the optimum and the image sharpens on the way; lr 1e-12: theta stays where bench.py evaluates
    for tag, lr in (("", ADAM["lr"]), ("_fixed", FIXED_LR)):
        sec, res = timed(lambda: obj.descend(theta0, method="Adam", n_iter=N_2DOF, lr=lr, lr_step=N_2DOF))
        out[f"two_dof{tag}_descend_us"] = sec / N_2DOF * 1e6
        sec, (x_host, hist) = timed(lambda: host_loop(lr))
        out[f"two_dof{tag}_host_us"] = sec / N_2DOF * 1e6
        out[f"two_dof{tag}_last_loss"] = [float(res.loss_history[-1]), float(hist[-1])]  # the two loops descend the same objective
    h.close()
    # ---- row 2: the 30k-event YAML plan
    ev = E.utils.generate_events(30000, H, W, 0.0, 0.05, seed=46)
    h = E.CMaxHandle((H, W)).set_events(ev)
    plan = PatchFlowObjective(h, 0.05, (16, 16), (16, 21), (16, 21), (2, 5), cost="hybrid",
                              cost_with_weight={"multi_focal_normalized_gradient_magnitude": 1.0, "total_variation": 0.01}, blur_sigma=1)
    x0 = np.random.default_rng(0).uniform(-100, 100, 512)
    sec, res = timed(lambda: plan.descend(x0, method="Adam", n_iter=N_PLAN, lr=ADAM["lr"], lr_step=N_PLAN))
    out["plan_descend_us"] = sec / N_PLAN * 1e6

    def plan_host_loop():
        x, state, loss = x0.copy(), {}, 0.0
        for it in range(N_PLAN):
            loss, g = plan.value_and_grad_numpy(x)
            x = adam_update(state, x, g, it)
        return loss

    sec, loss = timed(plan_host_loop)
    out["plan_host_us"] = sec / N_PLAN * 1e6
    out["plan_last_loss"] = [float(res.loss_history[-1]), float(loss)]
    print("PROBE " + json.dumps(out))


def main(path):
    runs = []
    for _ in range(ROUNDS):  # the variants alternate
        for fused in (True, False):
            env = dict(os.environ)
            env.pop("CMAX_DESCENT_NO_FUSED_STEP", None)
            if not fused:
                env["CMAX_DESCENT_NO_FUSED_STEP"] = "1"
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=600)
            line = [l for l in p.stdout.splitlines() if l.startswith("PROBE ")]
            if p.returncode or not line:
                sys.exit(f"child failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            runs.append(json.loads(line[0][6:]))
    lines = [
        "Device-resident descent against the host-driven loop, microseconds per Adam iteration (tools/probe_descent.py, MI355X; host clock",
        f"around {REPS} calls after 2 warm-up calls; {N_2DOF} iterations per call for the 2-DoF rows, {N_PLAN} for the plan; every line is one child process,",
        "the fused / separate variants alternate).  descend: one cmax_objective_descend / cmax_patch_plan_descend call; host loop: one",
        "cmax_objective_host / cmax_patch_plan_evaluate call per iteration + the same update in numpy.",
        "",
        "cfg2 shape = 1M events, 260 x 346, 2-DoF image variance, theta0 = (12.3, -7.7); lr 0.05: theta walks to the optimum over the call (the image",
        f"sharpens on the way); lr {FIXED_LR:g}: theta stays at theta0, where bench.py evaluates.  Plan = the 30k-event YAML objective, 512 DoF, lr 0.05.",
        "",
        "finish of the 2-DoF iteration       | cfg2 shape, lr 0.05     | cfg2 shape, theta fixed  | 30k-event YAML plan",
        "                                    | descend    host loop    | descend    host loop     | descend    host loop",
    ]
    for r in runs:
        name = "k_finish_raw_step (fused)        " if r["fused_step"] else "k_finish_raw + k_descent_step    "
        lines.append(f"{name}   | {r['two_dof_descend_us']:7.2f}    {r['two_dof_host_us']:7.2f}      | {r['two_dof_fixed_descend_us']:7.2f}    {r['two_dof_fixed_host_us']:7.2f}       "
                     f"| {r['plan_descend_us']:7.2f}    {r['plan_host_us']:7.2f}")
    lines += ["", "(the plan columns do not depend on the variant: they show the run-to-run spread)",
              "last loss of the device loop / the host loop, first run: 2-DoF %r, theta fixed %r, plan %r" % (
                  runs[0]["two_dof_last_loss"], runs[0]["two_dof_fixed_last_loss"], runs[0]["plan_last_loss"])]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write(text)
    print(text)


if __name__ == "__main__":
    if "--child" in sys.argv:
        child()
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "descent_cost.txt"))
