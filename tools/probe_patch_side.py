#!/usr/bin/env python
"""The measured errors of the solver side against the fp64 references of tests/_patch_ref.py and tests/_search_ref.py, on the case table
of tests/_patch_cases.py: the worst figure per group, next to the gate tests/test_gpu_patch_side.py asserts for it.  Runs the tests' own
measuring functions, so the figures are the ones the assertions see.  Writes profiles/patch_side_parity.txt.
usage: tools/probe_patch_side.py [leaf] [plan] [tv] [hvp] [search]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import _patch_cases as C  # noqa: E402
import test_gpu_patch_side as T  # noqa: E402

groups = sys.argv[1:] or ["leaf", "plan", "tv", "hvp", "search"]
lines = []


def emit(text):
    lines.append(text)
    print(text, flush=True)


if "leaf" in groups:
    for dtype in (torch.float64, torch.float32):
        worst = np.zeros(3)
        where = [None] * 3
        for gid, size in C.LEAF_CASES:
            e = T.measure_leaf(gid, size, dtype)
            for k in range(3):
                if e[k] >= worst[k]:
                    worst[k], where[k] = e[k], f"{gid} {size[0]}x{size[1]}"
        tol = T.LEAF_TOL[dtype]
        emit(f"leaf {str(dtype).split('.')[1]}, {len(C.LEAF_CASES)} geometries: forward {worst[0]:.2e} ({where[0]}; gate {tol[0]:g}), adjoint {worst[1]:.2e} "
             f"({where[1]}; gate {tol[1]:g}), one-hot adjoints at the band limits {worst[2]:.2e} ({where[2]}; gate {tol[1]:g})")
if "plan" in groups:
    worst, where = np.zeros(2), [None] * 2
    for c in C.PLAN_CASES:
        h, obj, b, loss, grad, e_loss, e_grad = T.measure_plan(c)
        emit(f"  plan {c['id']}: loss {e_loss:.2e} gradient {e_grad:.2e}")
        for k, e in enumerate((e_loss, e_grad)):
            if e >= worst[k]:
                worst[k], where[k] = e, c["id"]
        del obj
        h.close()
    emit(f"plan value and gradient, {len(C.PLAN_CASES)} cases: loss {worst[0]:.2e} ({where[0]}), gradient {worst[1]:.2e} ({where[1]}); gate {T.TOL:g}")
if "tv" in groups:
    for side, grids in (("LDS path (2 ph pw <= 4096)", [g for g in C.TV_GRIDS if 2 * g[0] * g[1] <= C.TAIL_LDS]),
                        ("global-memory path", [g for g in C.TV_GRIDS if 2 * g[0] * g[1] > C.TAIL_LDS])):
        worst, where = np.zeros(2), [None] * 2
        for pis in grids:
            for omit in (True, False):
                for kind, e_tv, bound_tv, tv, e_dtv, bound_dtv, dtv in T.measure_tail_tv(pis, omit):
                    for k, (e, ref) in enumerate(((e_tv, tv), (e_dtv, dtv))):
                        r = e / ref if ref > 0 else (0.0 if e == 0 else np.inf)
                        if r >= worst[k]:
                            worst[k], where[k] = r, f"{pis[0]}x{pis[1]} omit {omit} {kind}"
        emit(f"tail TV alone, {side}, {len(grids)} grids x 2 x {len(C.TV_MOTIONS)} motions: value {worst[0]:.2e} of the TV term ({where[0]}), "
             f"sub-gradient {worst[1]:.2e} of its largest entry ({where[1]}); gate {T.TV_TOL:g} or the subtraction's eps64 (|contrast| + |TV|)")
if "hvp" in groups:
    worst, where = {}, {}
    for c in C.HVP_CASES:
        b, e = T.measure_hvp(c)
        emit(f"  hvp {c['id']}: dropped {b['dropped']:.5f}, loss {e['loss']:.2e} gradient {e['grad']:.2e} Hv random {e['random']:.2e} one-hot {e['one-hot']:.2e}")
        for k, v in e.items():
            if v >= worst.get(k, 0.0):
                worst[k], where[k] = v, c["id"]
    emit(f"plan HVP, {len(C.HVP_CASES)} cases: random tangent {worst['random']:.2e} ({where['random']}), one-hot {worst['one-hot']:.2e} ({where['one-hot']}); "
         f"gate {T.HVP_TOL:g}; zero tangent: exact zeros")
if "search" in groups:
    for hd in C.SEARCH_HANDLES:
        rows = T.measure_search(hd)
        g = max(rows, key=lambda r: r[2])
        l = max(rows, key=lambda r: r[3])
        emit(f"search {hd['id']}, {len(rows)} (image, sigma) x {len(C.SEARCH_BOXES)} boxes x {len(C.SEARCH_CANDIDATES)} candidates: count exact, gm {g[2]:.2e} of its "
             f"row's largest (image {g[0]} sigma {g[1]}), loss {l[3]:.2e} (image {l[0]} sigma {l[1]}); gate {T.TOL:g}")
    gm, count, gm_r, count_r = T.measure_capacity()
    emit(f"search at 8191 votes on one cell: count {int(count[0])}, gm rel err {np.abs(gm / gm_r - 1.0).max():.2e}; bound 4 x 2^-24 = {4 * 2.0**-24:.2e}")
os.makedirs("profiles", exist_ok=True)
with open("profiles/patch_side_parity.txt", "w") as f:
    f.write("tools/probe_patch_side.py -- the solver side against the fp64 references (tests/_patch_ref.py, tests/_search_ref.py) on the table of "
            "tests/_patch_cases.py; worst figure per group, the case it occurs at, and the gate tests/test_gpu_patch_side.py asserts\n")
    f.write("\n".join(lines) + "\n")
