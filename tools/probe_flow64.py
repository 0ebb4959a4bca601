#!/usr/bin/env python
"""fp64 dense flow at the boundary (exact_flow=True): what it changes and what it costs.  Needs the GPU.  usage: tools/probe_flow64.py [parity] [cost]

parity  a random, UN-SNAPPED batch at the size of a cfg5 shard (2.5M events, 720 x 1280, fp64 per-pixel random flow of 20 px): the gradient
        of the fp32 path (the flow rounded to fp32) and of the exact path, both against the oracle at the caller's fp64 flow -- how much the
        rounding of the flow moves a real-size gradient -- and the events whose cell differs under the two flows (two oracle warps).
cost    on one handle, interleaved: cmax_objective with the fp32 flow against the fp64 flow (the split launch included), at the cfg5 shard
        and on a 1M-event batch; the patch plan with and without exact_flow (value_and_grad_numpy, hvp_numpy) at cfg1's shape (30k events,
        260 x 346, 16 x 16 patches) and on a 1M-event batch; the share of events K1 decides again in fp64 (the margin is the same in both
        modes: exact_margin_coef covers the flow's own rounding, so the candidates are the same events), restated in numpy."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import event_based_optical_flow_amd as E  # noqa: E402
from event_based_optical_flow_amd.solver import PatchFlowObjective  # noqa: E402
from oracle import oracle as orc  # noqa: E402


def f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def rel_max(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max())


def batch(n, size, seed):
    rng = np.random.default_rng(seed)
    ev = np.empty((n, 4))
    ev[:, 0], ev[:, 1] = rng.integers(0, size[0], n), rng.integers(0, size[1], n)
    ev[:, 2], ev[:, 3] = np.sort(rng.uniform(0.0, 0.05, n)), rng.integers(0, 2, n)
    return ev


def random_flow64(size, mag, seed):
    return np.random.default_rng(seed).uniform(-mag, mag, (2,) + tuple(size))  # fp64 draws: not representable in fp32


def candidate_share(ev, F, size):
    """Share of events within K1's margin of a cell border (reference time first, integral sources): 1.5 eps 4 |f|_max of the event."""
    warped, _ = orc.warp_event(ev, F, "dense-flow", "first", size, True)
    ix, iy = ev[:, 0].astype(np.int64), ev[:, 1].astype(np.int64)
    fm = np.maximum(np.abs(F[0, ix, iy]), np.abs(F[1, ix, iy]))
    m = 1.5 * 2.0 ** -24 * 4.0 * fm
    fr = (warped[:, :2] + 1e-6) - np.floor(warped[:, :2] + 1e-6)
    near = ((fr < m[:, None]) | (fr > 1.0 - m[:, None])).any(axis=1)
    return float(near.mean())


def parity():
    size, n = (720, 1280), 2_500_000
    ev, F = batch(n, size, 1), random_flow64(size, 20.0, 2)
    ref = orc.objective(ev, F, "dense-flow", size)
    ref32 = orc.objective(ev, f32(F), "dense-flow", size)
    c64 = np.floor(orc.warp_event(ev, F, "dense-flow", "first", size)[0][:, :2] + 1e-6)
    c32 = np.floor(orc.warp_event(ev, f32(F), "dense-flow", "first", size)[0][:, :2] + 1e-6)
    flips = int((c64 != c32).any(axis=1).sum())
    h = E.CMaxHandle(size).set_events(ev)
    desc = E.make_descriptor("image_variance", "dense-flow")
    Fd = torch.tensor(F, dtype=torch.float64, device="cuda")
    _, g32 = h.evaluate(desc, Fd.float())
    _, g64 = h.evaluate(desc, Fd, exact_flow=True)
    g32, g64 = g32.double().cpu().numpy(), g64.double().cpu().numpy()
    print(f"parity: un-snapped batch, {n} events on {size[0]} x {size[1]}, fp64 random flow of 20 px, image_variance (informational, not a test)")
    print(f"  events whose cell differs under the fp64 flow and under f32(flow): {flips} of {n} ({flips / n:.1e})")
    print(f"  gradient against the oracle at the fp64 flow, relative to its largest entry:  fp32 path {rel_max(g32, ref['grad']):.2e}   exact path {rel_max(g64, ref['grad']):.2e}")
    print(f"  the oracle itself at f32(flow) against the oracle at the fp64 flow: {rel_max(ref32['grad'], ref['grad']):.2e};  fp32 path against the oracle at "
          f"f32(flow): {rel_max(g32, ref32['grad']):.2e}")
    bad32 = int((np.abs(g32 - ref["grad"]) > 1e-4 * np.abs(ref["grad"]).max()).sum())
    bad64 = int((np.abs(g64 - ref["grad"]) > 1e-4 * np.abs(ref["grad"]).max()).sum())
    print(f"  gradient entries beyond the gate of 1e-4 (of {g32.size}): fp32 path {bad32}, exact path {bad64}")
    h.close()


def timed(calls, reps=200, rounds=5):
    """Interleaved: per round every call `reps` times between two events -> {name: (min, median, max) us per call}."""
    out = {k: [] for k in calls}
    for fn in calls.values():
        for _ in range(20):
            fn()
    for _ in range(rounds):
        for name, fn in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b) * 1e3 / reps)
    return {k: (min(v), float(np.median(v)), max(v)) for k, v in out.items()}


def wall(fn, reps=100, rounds=5):
    for _ in range(5):
        fn()
    ts = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / reps * 1e3)
    return min(ts), float(np.median(ts)), max(ts)


def cost():
    print("cost: cmax_objective (value + gradient) per call, one handle, fp32 flow and fp64 flow interleaved, 5 rounds of 200 calls: min / median / max us")
    for tag, size, n, cost_name in (("cfg5 shard", (720, 1280), 2_500_000, "image_variance"), ("1M events, 260 x 346", (260, 346), 1_000_000, "image_variance"),
                                    ("cfg3: 5M events, 480 x 640, gradient_magnitude", (480, 640), 5_000_000, "gradient_magnitude")):
        ev, F = batch(n, size, 3), random_flow64(size, 20.0, 4)
        h = E.CMaxHandle(size).set_events(ev)
        desc = E.make_descriptor(cost_name, "dense-flow")
        Fd = torch.tensor(F, dtype=torch.float64, device="cuda")
        c32, _, _ = h.prepare(desc, Fd.float())
        c64, _, _ = h.prepare(desc, Fd, exact_flow=True)
        t = timed({"fp32": c32, "fp64": c64})
        share = candidate_share(ev[:: max(1, n // 500_000)], F, size)
        print(f"  {tag}: fp32 {t['fp32'][0]:.1f} / {t['fp32'][1]:.1f} / {t['fp32'][2]:.1f}   fp64 (split launch included) {t['fp64'][0]:.1f} / {t['fp64'][1]:.1f} / "
              f"{t['fp64'][2]:.1f}   median + {t['fp64'][1] - t['fp32'][1]:.1f} us ({100.0 * (t['fp64'][1] / t['fp32'][1] - 1.0):+.1f} %);  events K1 decides again in "
              f"fp64, either mode: {share:.1e}")
        h.close()
    print("cost: the patch plan per call (host round trip included), with and without exact_flow, 5 rounds of 100 calls: min / median / max ms")
    cww = {"multi_focal_normalized_gradient_magnitude": 1.0, "total_variation": 0.01}
    H, W = 260, 346
    for n in (30_000, 1_000_000):
        ev = E.utils.generate_events(n, H, W, 0.0, 0.05, seed=46)
        x = np.random.default_rng(0).uniform(-100, 100, 512)
        v = np.random.default_rng(1).normal(size=512)
        for ta in (False, True):
            row = {}
            for exact in (False, True):
                h = E.CMaxHandle((H, W)).set_events(ev, time_bin=10 if ta else 0)
                obj = PatchFlowObjective(h, 0.05, (16, 16), (16, 21), (16, 21), (2, 5), cost="hybrid", cost_with_weight=cww, blur_sigma=1, time_aware=ta,
                                         time_bin=10, exact_flow=exact)
                row[exact] = (wall(lambda: obj.value_and_grad_numpy(x)), wall(lambda: obj.hvp_numpy(x, v)))
                del obj
                h.close()
            for k, name in ((0, "value_and_grad_numpy"), (1, "hvp_numpy")):
                a, b = row[False][k], row[True][k]
                print(f"  {n} events, {'burgers T=10' if ta else 'plain'}, {name}: default {a[0]:.3f} / {a[1]:.3f} / {a[2]:.3f}   exact_flow {b[0]:.3f} / {b[1]:.3f} / "
                      f"{b[2]:.3f}   median {100.0 * (b[1] / a[1] - 1.0):+.1f} %")


if __name__ == "__main__":
    which = sys.argv[1:] or ["parity", "cost"]
    torch.cuda.set_device(0)
    if "parity" in which:
        parity()
    if "cost" in which:
        cost()
