#!/usr/bin/env python
"""Cost of a candidate-iteration of the multi-start descent (cmax_objective_descend_batch: K trajectories per call, the K candidates of an
iteration in the launches of one) at cfg2's shape -- 1M events, 260 x 346, 2-DoF image variance -- for K in 1, 2, 4, 8, 16, 32, 64, beside
    K sequential cmax_objective_descend calls in the same process (the single-start entry, whose kernels this entry leaves as they were:
    profiles/descent_batch_resources.txt), and
    cmax_objective_batch's time per evaluation at the same K: the floor, the same launches without a step.
Starts: the theta bench.py evaluates at, spread by up to +-1 px (start 0 is that theta itself); Adam with lr 1e-12, so every trajectory
stays where it started and the figures compare with the "theta fixed" column of profiles/descent_cost.txt (tools/probe_descent.py, whose
procedure this follows).  Every figure is a host clock around calls that end in the library's own wait (the evaluations: a stream
synchronisation behind the last call), after a warm-up call of the same shape; the three variants of a K alternate inside a round and every
round is a child process of its own.
    python tools/probe_descent_batch.py [out.txt]        (GPU box; default profiles/descent_batch_cost.txt)"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W = 260, 346
KS = (1, 2, 4, 8, 16, 32, 64)
N_ITER, REPS, ROUNDS = 4096, 3, 2  # (the shortest timed window, K = 1: 3 x 4096 x 16 us = 0.2 s)
FIXED_LR = 1e-12
THETA = (12.3, -7.7)


def timed(fn, reps=REPS, warm=1):
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

    ev = E.utils.generate_events(1_000_000, H, W, 0.0, 0.05, seed=46)
    h = E.CMaxHandle((H, W)).set_events(ev)
    obj = E.ContrastObjective(h, "2d-translation", cost="image_variance")
    desc = obj.terms[0][2]
    spread = np.random.default_rng(3).uniform(-1.0, 1.0, (max(KS), 2))
    spread[0] = 0.0
    starts = np.array(THETA) + spread
    kw = dict(method="Adam", n_iter=N_ITER, lr=FIXED_LR, lr_step=N_ITER)
    out = {}
    for K in KS:
        th = starts[:K]
        sec, res = timed(lambda: obj.descend_batch(th, **kw))
        out[f"batch_{K}"] = sec / (N_ITER * K) * 1e6
        sec, one = timed(lambda: [obj.descend(t, **kw) for t in th])
        out[f"single_{K}"] = sec / (N_ITER * K) * 1e6
        call, results, grads = h.prepare_batch(desc, torch.tensor(th, dtype=torch.float64, device="cuda"))

        def evaluations():
            for _ in range(N_ITER):
                call()
            torch.cuda.current_stream().synchronize()
            return results

        sec, _ = timed(evaluations)
        out[f"eval_{K}"] = sec / (N_ITER * K) * 1e6
        # the two loops descend the same objective: last loss of candidate K - 1 (batched, single)
        out[f"loss_{K}"] = [float(res[K - 1].loss_history[-1]), float(one[K - 1].loss_history[-1])]
    h.close()
    print("PROBE " + json.dumps(out))


def main(path):
    runs = []
    for _ in range(ROUNDS):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, timeout=500)
        line = [l for l in p.stdout.splitlines() if l.startswith("PROBE ")]
        if p.returncode or not line:
            sys.exit(f"child failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
        runs.append(json.loads(line[0][6:]))
    lines = [
        "Multi-start descent, microseconds per candidate-iteration (tools/probe_descent_batch.py, MI355X; host clock around",
        f"{REPS} calls after 1 warm-up call; Adam, {N_ITER} iterations per call, lr {FIXED_LR:g}: every trajectory stays at its start).",
        f"cfg2 shape = 1M events, 260 x 346, 2-DoF image variance; starts = theta {THETA} spread by up to +-1 px.  One child process per round.",
        "  descend_batch : one cmax_objective_descend_batch call with K starts          / (K x iterations)",
        "  K x descend   : K sequential cmax_objective_descend calls, one start each    / (K x iterations)",
        "  batch eval    : cmax_objective_batch with K candidates, called `iterations` times, one wait / (K x iterations): the floor",
        "",
        "   K | round | descend_batch   K x descend   batch eval | descend_batch / K x descend",
    ]
    for K in KS:
        for i, r in enumerate(runs):
            b, s, e = r[f"batch_{K}"], r[f"single_{K}"], r[f"eval_{K}"]
            lines.append(f"  {K:2d} |   {i}   |   {b:8.2f}      {s:8.2f}      {e:8.2f}  |   {b / s:5.2f}")
    lines += ["", "(K = 1 takes the single-start path inside the batched entry: the row shows what the entry's own copies and wait cost)",
              "last loss of the last candidate, batched / single, first round: " + ", ".join(f"K {K}: {runs[0][f'loss_{K}']}" for K in (1, 8, 64))]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write(text)
    print(text)


if __name__ == "__main__":
    if "--child" in sys.argv:
        child()
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "descent_batch_cost.txt"))
