"""Fixtures of the single-scale patch solvers and of the nearest patch filter, from the reference itself (imported in place through
ref_import, never copied):  python tests/golden/gen_golden_mixed.py  ->  tests/golden/solver_mixed.npz, tests/golden/nearest_leaf.npz

What is pinned
  * MixedPatchContrastMaximization (src/solver/patch_contrast_mixed.py) and TimeAwarePatchContrastMaximization
    (src/solver/time_aware_patch_contrast.py, the registry's "time_aware_mixed_patch_contrast_maximization") on a 68 x 90 sensor with
    3000 events: patch.size / sliding_window 16/16, 16/8 (overlapping windows) and [20, 24]/[10, 8]; patch.filter_type bilinear and
    nearest; time-ignorant (the mixed class), Burgers T = 10 at "middle" and upwind T = 5 at "first" (the time-aware class).  Per
    configuration: patch_image_size, pad, a random x, objective_scipy's loss, its autograd gradient and torch.autograd.functional.vhp
    along a random v; per geometry and filter the dense flow of that x.
  * for 16/16, time-aware Burgers, bilinear: every candidate loss and the pick of initialize_guess_from_whole_image ("global-best")
    and initialize_guess_from_patch ("grid-best" on patch n_patch // 2 - 1), and one complete optimize() from patch.initialize "zero"
    with Newton-CG and max_iter 25 (the nearest filter too).
  * the leaf with the nearest filter (interpolate_dense_flow_from_patch_tensor, src/solver/patch_contrast_base.py:462-506): the index
    map, the dense flow and the autograd VJP on sw in {1, 2, 3, 5, 16, 25} x grids of 1 .. 4 cells and the geometries of
    tests/_patch_cases.py.

One more shim, installed HERE, in this process only (recorded in the fixtures' `shims` field like the three of ref_import.py):
  (4) torchvision.transforms.functional.resize(img, size, NEAREST) -> F.interpolate(size=..., mode="nearest")
        (torchvision's published algorithm for tensors; ref_import's shim (2) ignores the interpolation mode)
"""
import logging
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                   # tests/: _patch_cases
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the repository: the package _patch_cases imports
import ref_import  # noqa: E402

src = ref_import.import_reference()
from gen_golden import SEED, _moving_dot_events  # noqa: E402  (the scene generator the other solver fixtures use)

SHIMS = ref_import.SHIMS + "; resize(nearest) -> F.interpolate(size, mode='nearest')"
H, W, N_EVENTS, PERIOD = 68, 90, 3000, 0.05
GEOMETRIES = (("16_16", 16, 16), ("16_8", 16, 8), ("20x24_10x8", [20, 24], [10, 8]))
VARIANTS = (("plain", None), ("burgers", dict(time_bin=10, flow_interpolation="burgers", t0_flow_location="middle")),
            ("upwind", dict(time_bin=5, flow_interpolation="upwind", t0_flow_location="first")))
REGISTRY_NAME = "time_aware_mixed_patch_contrast_maximization"
# The random x of the objective fixtures, in pixel / second.  The explicit upwind / Burgers steps of the voxel chain (dt = 1 / time_bin)
# are stable while (|u| + |v|) dt <= 1 pixel of displacement -- the CFL condition of a first-order upwind step in two dimensions.  The
# fixture's smallest time_bin is 5, so |u|, |v| <= 2.5 px over the 0.05 s batch: |x| <= 50 px / s.  Beyond it the chain amplifies the
# jumps the nearest filter puts between cells without bound: at +-300 px / s (15 px, what solver_objective.npz uses on the smooth bilinear
# flow of the pyramid solver) the reference's own voxel reaches 1e11 px on this sensor.  Such a point says nothing about a solver, and it is
# not where an optimiser goes (optimize() below ends within 6.2 px); gen_solver asserts that no bin outgrows the given flow.
X_RANGE = 40.0


def install_nearest_shim():
    import torchvision.transforms.functional as tvf

    bilinear = tvf.resize

    def resize(img, size, interpolation=None, **kw):
        if interpolation != "nearest":  # ref_import's InterpolationMode stub: plain strings
            return bilinear(img, size, interpolation=interpolation, **kw)
        squeeze = img.dim() == 3
        if squeeze:
            img = img[None]
        out = torch.nn.functional.interpolate(img, size=list(size), mode="nearest")
        return out[0] if squeeze else out

    tvf.resize = resize
    from src.solver import patch_contrast_base
    patch_contrast_base.transforms.functional.resize = resize


def solver_config(size, sliding_window, filter_type, variant, initialize="random"):
    c = {"method": REGISTRY_NAME, "time_aware": variant is not None,
         "patch": {"initialize": initialize, "size": size, "sliding_window": sliding_window, "filter_type": filter_type},
         "motion_model": "2d-translation", "warp_direction": "first", "parameters": ["trans_x", "trans_y"],
         "cost": "hybrid", "outer_padding": 0,
         "cost_with_weight": {"multi_focal_normalized_gradient_magnitude": 1.0, "total_variation": 0.01},
         "iwe": {"method": "bilinear_vote", "blur_sigma": 1}}
    if variant is not None:
        c.update(variant)
    return c


OPT_CFG = {"n_iter": 40, "method": "Newton-CG", "max_iter": 25,
           "parameters": {"trans_x": {"min": -150, "max": 150}, "trans_y": {"min": -150, "max": 150}}}


def reference_solver(size, sliding_window, filter_type, variant, initialize="random"):
    from src import solver as ref_solver

    cfg = solver_config(size, sliding_window, filter_type, variant, initialize)
    cls = ref_solver.collections[REGISTRY_NAME] if variant is not None else ref_solver.MixedPatchContrastMaximization
    slv = cls((H, W), {}, cfg, dict(OPT_CFG), {}, None)
    slv._device = "cpu"
    return slv


def pad_of(slv):
    return [int(slv.patch_size[k] / 2 // slv.sliding_window[k]) + slv.patch_shift[k] // slv.sliding_window[k] + 1 for k in (0, 1)]


def gen_solver(ev):
    rng = np.random.default_rng(SEED + 21)
    out = {"events": ev, "image_size": np.array([H, W]), "period": np.array(PERIOD), "registry_name": np.array(REGISTRY_NAME)}
    names = []
    for gname, size, sw in GEOMETRIES:
        x = v = None
        for filt in ("bilinear", "nearest"):
            for vname, variant in VARIANTS:
                slv = reference_solver(size, sw, filt, variant)
                slv.events = torch.from_numpy(ev).double().requires_grad_()
                ph, pw = slv.patch_image_size
                if x is None:  # one x and one v per geometry: the filters and variants are compared on the same point
                    x = rng.uniform(-X_RANGE, X_RANGE, 2 * ph * pw)  # pixel / second: +-2 px over the batch, see X_RANGE
                    v = rng.normal(size=x.shape)
                k = f"{gname}__{filt}__{vname}"
                names.append(k)
                tx = torch.from_numpy(x).requires_grad_()
                loss = slv.objective_scipy(tx, suppress_log=True)
                (g,) = torch.autograd.grad(loss, tx)
                loss2, hv = torch.autograd.functional.vhp(lambda z: slv.objective_scipy(z, suppress_log=True), torch.from_numpy(x), torch.from_numpy(v))
                assert abs(loss2.item() - loss.item()) <= 1e-12 * abs(loss.item())
                out[k + "__x"], out[k + "__v"] = x, v
                out[k + "__loss"], out[k + "__grad"], out[k + "__vhp"] = np.array(loss.item()), g.numpy(), hv.numpy()
                out[k + "__patch_image_size"] = np.array([ph, pw])
                out[k + "__patch_size"], out[k + "__sliding_window"] = np.array(slv.patch_size), np.array(slv.sliding_window)
                out[k + "__pad"] = np.array(pad_of(slv))
                out[k + "__n_patch"] = np.array(slv.n_patch)
                if vname == "plain":  # the dense flow depends on geometry and filter only
                    out[f"{gname}__{filt}__dense"] = slv.interpolate_dense_flow_from_patch_tensor(torch.from_numpy(x)).numpy()
                grow = 1.0
                if variant is not None:  # the propagation must stay in its stable range (X_RANGE): no bin outgrows the given flow
                    with torch.no_grad():
                        voxel = slv.motion_to_dense_flow(torch.from_numpy(x) * PERIOD)
                    grow = float(voxel.abs().max() / (np.abs(x).max() * PERIOD))
                    assert grow <= 1.5, (k, grow)
                print(k, (ph, pw), "loss", loss.item(), "|g|", float(g.abs().max()), "|Hv|", float(hv.abs().max()), "max |voxel| / max |flow|", grow)
    out["configs"] = np.array(names)
    return out


def gen_initialisers(ev, out):
    """global-best / grid-best of the time-aware class on 16/16 (patch_contrast_base.py:126-187 through patch_contrast_mixed.py:142-157)."""
    from src import utils

    slv = reference_solver(16, 16, "bilinear", VARIANTS[1][1])

    def losses(events_np, field):
        slv.events = torch.from_numpy(events_np).double().requires_grad_()
        grid = np.zeros((len(field), len(field)))
        for i in range(len(field)):
            for j in range(len(field)):
                guess = torch.from_numpy(np.array([field[i], field[j]])).double().requires_grad_()
                grid[i, j] = float(slv.objective_scipy_for_patch(guess, suppress_log=True))
        return grid

    logging.disable(logging.INFO)
    best_w = slv.initialize_guess_from_whole_image(ev)
    out["whole__field"] = np.arange(-150, 150, 10)
    out["whole__best"] = best_w.detach().numpy()
    out["whole__loss"] = losses(ev, out["whole__field"])
    index = slv.n_patch // 2 - 1
    best_p = slv.initialize_guess_from_patch(ev, patch_index=index)
    pt = slv.patches[index]
    cropped = utils.crop_event(ev, pt.x_min, pt.x_max, pt.y_min, pt.y_max)
    out["patch__index"], out["patch__box"] = np.array(index), np.array([pt.x_min, pt.x_max, pt.y_min, pt.y_max])
    out["patch__n_events"] = np.array(len(cropped))
    out["patch__field"] = np.arange(-150, 150, 30)
    out["patch__best"] = best_p.detach().numpy()
    out["patch__loss"] = losses(cropped, out["patch__field"])
    logging.disable(logging.NOTSET)
    print("global-best", out["whole__best"], "grid-best", out["patch__best"], "patch", index, "events", len(cropped))


def gen_optimize(ev, out):
    """optimize() of the time-aware class on 16/16 from patch.initialize "zero": Newton-CG, gtol 1e-7, maxiter 25, float64."""
    cwd = os.getcwd()
    for filt in ("bilinear", "nearest"):
        slv = reference_solver(16, 16, filt, VARIANTS[1][1], initialize="zero")
        xs = []
        with tempfile.TemporaryDirectory() as tmp:  # utils.profile writes optimize.prof into the working directory
            os.chdir(tmp)
            try:
                logging.disable(logging.INFO)
                objective = slv.objective_scipy

                def traced(x, *a, **kw):
                    xs.append(np.asarray(x.detach()).copy())
                    return objective(x, *a, **kw)

                slv.objective_scipy = traced
                best = slv.optimize(ev)
            finally:
                logging.disable(logging.NOTSET)
                os.chdir(cwd)
        slv.objective_scipy = objective
        k = f"optimize__{filt}"
        best = np.asarray(best)
        out[k + "__x"] = best
        out[k + "__loss"] = np.array(float(slv.objective_scipy(torch.from_numpy(best.reshape(-1)), suppress_log=True)))
        out[k + "__loss0"] = np.array(float(slv.objective_scipy(torch.zeros(best.size, dtype=torch.float64), suppress_log=True)))
        out[k + "__dense"] = slv.interpolate_dense_flow_from_patch_tensor(torch.from_numpy(best.reshape(-1))).numpy()  # pixel / second
        # the distinct points the objective was evaluated at, in order (the trajectory; a run that parts from it can be located)
        trace = [xs[0]]
        for x in xs[1:]:
            if not np.array_equal(x, trace[-1]):
                trace.append(x)
        out[k + "__trace"] = np.stack(trace)
        print(k, "loss0", float(out[k + "__loss0"]), "->", float(out[k + "__loss"]), "points", len(trace), "max |x| px", np.abs(best).max() * PERIOD)


def leaf_geometries():
    """(id, patch_image_size, pad, sw, size): the small table of the issue plus tests/_patch_cases.py's."""
    import _patch_cases as C

    rows = []
    for sw in (1, 2, 3, 5, 16, 25):
        for n in (1, 2, 3, 4):
            rows.append((f"sw{sw}-n{n}", (n, n), (1, 1), (sw, sw), (n * sw + (1 if sw > 1 else 0), n * sw)))
    for gid, size in C.LEAF_CASES:
        g = C.GEOMETRY[gid]
        rows.append((f"{gid}-{size[0]}x{size[1]}", g["patch_image_size"], g["pad"], g["sw"], size))
    return rows


def gen_leaf():
    from src import solver as ref_solver

    rng = np.random.default_rng(SEED + 22)
    out, ids = {}, []
    slv = reference_solver(16, 16, "nearest", None)
    for gid, pis, pad, sw, size in leaf_geometries():
        # the reference's own function on an object whose geometry is set by hand: pad = patch_size / 2 // sw + shift // sw + 1
        slv.image_shape, slv.patch_image_size, slv.sliding_window = tuple(size), tuple(pis), tuple(sw)
        slv.patch_size, slv.patch_shift = (0, 0), ((pad[0] - 1) * sw[0], (pad[1] - 1) * sw[1])
        if min(pad) == 0:  # pad 0 is below what the reference's formula gives: such a geometry has no reference value
            continue
        assert pad_of(slv) == list(pad), (gid, pad_of(slv), pad)
        m = np.asarray(rng.normal(0, 30.0, (2,) + tuple(pis)), dtype=np.float32).astype(np.float64)
        cot = np.asarray(rng.normal(size=(2,) + tuple(size)), dtype=np.float32).astype(np.float64)
        tm = torch.from_numpy(m).requires_grad_()
        dense = slv.interpolate_dense_flow_from_patch_tensor(tm)
        (vjp,) = torch.autograd.grad((dense * torch.from_numpy(cot)).sum(), tm)
        gh, gw = pis[0] + 2 * pad[0], pis[1] + 2 * pad[1]
        rows = torch.nn.functional.interpolate(torch.arange(gh, dtype=torch.float64).reshape(1, 1, gh, 1).expand(1, 1, gh, gw).contiguous(),
                                               size=[gh * sw[0], gw * sw[1]], mode="nearest")[0, 0, :, 0]
        cols = torch.nn.functional.interpolate(torch.arange(gw, dtype=torch.float64).reshape(1, 1, 1, gw).expand(1, 1, gh, gw).contiguous(),
                                               size=[gh * sw[0], gw * sw[1]], mode="nearest")[0, 0, 0, :]
        ids.append(gid)
        out[gid + "__geometry"] = np.array(list(pis) + list(pad) + list(sw) + list(size))
        # motion and cotangent are fp32 values, and the nearest dense flow is a negated copy of the motion: stored as float32, exactly
        d = dense.detach().numpy()
        assert np.array_equal(d.astype(np.float32).astype(np.float64), d)
        out[gid + "__motion"], out[gid + "__cotangent"] = m.astype(np.float32), cot.astype(np.float32)
        out[gid + "__dense"], out[gid + "__vjp"] = d.astype(np.float32), vjp.numpy()
        out[gid + "__rows"], out[gid + "__cols"] = rows.numpy().astype(np.int32), cols.numpy().astype(np.int32)
    out["ids"] = np.array(ids)
    out["shims"], out["seed"] = np.array(SHIMS), np.array(SEED + 22)
    np.savez_compressed(os.path.join(HERE, "nearest_leaf.npz"), **out)
    print("nearest_leaf:", len(ids), "geometries")


if __name__ == "__main__":
    install_nearest_shim()
    which = sys.argv[1:] or ["leaf", "solver"]
    if "leaf" in which:
        gen_leaf()
    if "solver" in which:
        rng = np.random.default_rng(SEED + 20)

        def flow_fn(cx, cy):  # pixel per batch period, smooth across the sensor: ~(5, -3) px = (100, -60) px / s, inside the grids' box
            return 5.0 + 1.0 * cx / H - 0.5 * cy / W, -3.0 + 0.8 * cy / W + 0.5 * cx / H

        ev = _moving_dot_events(N_EVENTS, H, W, flow_fn, rng, n_dots=60, period=PERIOD)
        ev[0, 2], ev[-1, 2] = 0.0, PERIOD
        out = gen_solver(ev)
        gen_initialisers(ev, out)
        gen_optimize(ev, out)
        out["shims"], out["seed"] = np.array(SHIMS), np.array(SEED + 20)
        np.savez_compressed(os.path.join(HERE, "solver_mixed.npz"), **out)
