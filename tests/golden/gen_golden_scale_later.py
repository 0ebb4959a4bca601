"""Generate tests/golden/solver_scale_later.npz by RUNNING THE REFERENCE with `solver.scale_later: True`.

Run in the build container only (needs the reference checkout, see ref_import.py):
    python tests/golden/gen_golden_scale_later.py
Data only.  Events, image size and the patch motions are READ from solver_objective.npz (and flow_error.npz for the
metrics case), so the numbers sit beside the `scale_later: False` ones.  The reference is imported in place through
ref_import.py (stubs + 3 shims); the numpy branch of motion_to_dense_flow additionally needs the cv2.resize shim of
gen_golden.py's flow_error fixture (recorded as `extra_shim`).

What is pinned (src/solver/patch_contrast_pyramid.py:452, 464-516 with self.scale_later, src/solver/base.py:219-224):
  per case   x, loss, grad (objective_scipy + torch.autograd.grad), v, vhp (torch.autograd.functional.vhp), scale = D.max(),
             n_ties (pixels of D equal to the maximum), loss_off (the same x with scale_later: False), x_factor, and the flow
             voxel motion_to_dense_flow(x, t_scale) from the tensor and from the numpy branch.  A full [10,2,68,90] fp64 voxel
             is ~1 MB, so the voxels are stored on the pixel lattice rows[::VOX_STRIDE[0]], cols[::VOX_STRIDE[1]] (all bins,
             both components); `voxel_branch_diff` is the largest difference of the two branches over the FULL voxel.
  flow_error calculate_flow_error / calculate_fwl_pred of the reference solver (numpy branch) on flow_error.npz's scene.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

src = ref_import.import_reference()
from src import solver as ref_solver  # noqa: E402

SEED = 46
TEST_TOL = 1e-4          # tests/test_gpu_solver.py:16
SEPARATION = 100 * TEST_TOL  # |loss(scale_later) - loss(off)| must exceed this (relative): a build ignoring the flag must fail
VOX_STRIDE = (4, 6)
EXTRA_SHIM = "cv2.resize(INTER_LINEAR) -> F.interpolate(bilinear, align_corners=False)"


def install_cv2_resize():
    """shim (4) of gen_golden.py:891-901: the numpy branch of the patch interpolation calls cv2.resize(src, None, None, fx, fy,
    INTER_LINEAR) (patch_contrast_base.py:438-453) -> half-pixel-centre bilinear up-sampling = shim (2)'s arithmetic."""
    import cv2

    def _cv2_resize(src_img, dsize, dst=None, fx=0, fy=0, interpolation=1):
        assert dsize is None and interpolation == cv2.INTER_LINEAR
        t = torch.from_numpy(np.ascontiguousarray(src_img))[None, None]
        size = [int(round(src_img.shape[0] * fy)), int(round(src_img.shape[1] * fx))]
        return torch.nn.functional.interpolate(t, size=size, mode="bilinear", align_corners=False)[0, 0].numpy()

    cv2.resize = _cv2_resize


def ref_solver_for(H, W, scale_later, flow_interpolation="burgers", t0="middle", scale=4):
    """The reference's PyramidalPatchContrastMaximization with the shipped Burgers YAML parameters on an H x W sensor."""
    slv_cfg = {
        "method": "pyramidal_patch_contrast_maximization", "time_aware": True, "scale_later": scale_later,
        "time_bin": 10, "flow_interpolation": flow_interpolation, "t0_flow_location": t0,
        "patch": {"initialize": "random", "scale": scale, "crop_height": 64, "crop_width": 80, "filter_type": "bilinear"},
        "motion_model": "2d-translation", "warp_direction": "first", "parameters": ["trans_x", "trans_y"],
        "cost": "hybrid", "outer_padding": 0,
        "cost_with_weight": {"multi_focal_normalized_gradient_magnitude": 1.0, "total_variation": 0.01},
        "iwe": {"method": "bilinear_vote", "blur_sigma": 1},
    }
    opt_cfg = {"n_iter": 40, "method": "Newton-CG", "max_iter": 25,
               "parameters": {"trans_x": {"min": -150, "max": 150}, "trans_y": {"min": -150, "max": 150}}}
    slv = ref_solver.collections["pyramidal_patch_contrast_maximization"]((H, W), {}, slv_cfg, opt_cfg, {}, None)
    slv._device = "cpu"
    assert slv.scale_later == bool(scale_later)
    return slv


def sub(voxel):
    return np.ascontiguousarray(np.asarray(voxel)[..., ::VOX_STRIDE[0], ::VOX_STRIDE[1]])


def one_case(out, name, ev, H, W, x0, patch_scale, flow_interpolation, t0, rng, want_ties):
    te = torch.from_numpy(ev)
    t_scale = float(ev[:, 2].max() - ev[:, 2].min())
    on = ref_solver_for(H, W, True, flow_interpolation, t0)
    off = ref_solver_for(H, W, False, flow_interpolation, t0)
    for slv in (on, off):
        slv.overload_patch_configuration(patch_scale)
        slv.current_scale = patch_scale
    ph, pw = on.patch_image_size
    factor = 1.0
    while True:
        x = x0 * factor
        tx = torch.from_numpy(x).requires_grad_()
        loss = on.objective_scipy(tx, te, {}, suppress_log=True)
        loss_off = off.objective_scipy(torch.from_numpy(x), te, {}, suppress_log=True).item()
        if abs(loss.item() - loss_off) > SEPARATION * abs(loss.item()):
            break
        factor *= 2.0  # the rescaled field is nearly stationary under the propagation: enlarge x until the two maps separate
        assert factor <= 64.0, (name, loss.item(), loss_off)
    (g,) = torch.autograd.grad(loss, tx)
    v = torch.from_numpy(rng.normal(size=x.shape))
    loss2, hv = torch.autograd.functional.vhp(lambda z: on.objective_scipy(z, te, {}, suppress_log=True), torch.from_numpy(x), v)
    assert abs(loss2.item() - loss.item()) <= 1e-12 * abs(loss.item())
    dense = on.interpolate_dense_flow_from_patch_tensor(torch.from_numpy(x))
    scale = dense.max().item()
    n_ties = int((dense == dense.max()).sum().item())
    if want_ties == "one":
        assert n_ties == 1, (name, n_ties)
    elif want_ties == "many":
        assert n_ties > 1, (name, n_ties)
    motion = x.reshape(2, ph, pw)
    vox_t = on.motion_to_dense_flow({patch_scale: torch.from_numpy(motion)}, t_scale).numpy()
    vox_n = np.asarray(on.motion_to_dense_flow({patch_scale: motion.copy()}, t_scale))
    assert vox_t.shape == vox_n.shape == (10, 2, H, W)
    out[name + "__x"] = x
    out[name + "__x_factor"] = np.array(factor)
    out[name + "__loss"] = np.array(loss.item())
    out[name + "__loss_off"] = np.array(loss_off)
    out[name + "__grad"] = g.numpy()
    out[name + "__v"] = v.numpy()
    out[name + "__vhp"] = hv.numpy()
    out[name + "__scale"] = np.array(scale)
    out[name + "__n_ties"] = np.array(n_ties)
    out[name + "__voxel_tensor"] = sub(vox_t)
    out[name + "__voxel_numpy"] = sub(vox_n)
    out[name + "__voxel_branch_diff"] = np.array(np.abs(vox_t - vox_n).max())
    out[name + "__patch_scale"] = np.array(patch_scale)
    out[name + "__flow_interpolation"] = np.array(flow_interpolation)
    out[name + "__t0_flow_location"] = np.array(t0)
    out[name + "__patch_image_size"] = np.array([ph, pw])
    out[name + "__patch_size"] = np.array(on.patch_size)
    out[name + "__sliding_window"] = np.array(on.sliding_window)
    out[name + "__patch_shift"] = np.array(on.patch_shift)
    print(f"{name}: loss {loss.item():.6f} (off {loss_off:.6f}), scale {scale:.4f}, n_ties {n_ties}, x_factor {factor}, "
          f"branches differ by {out[name + '__voxel_branch_diff']:.2e}")


def gen_flow_error(out):
    g = np.load(os.path.join(HERE, "flow_error.npz"))
    H, W = (int(v) for v in g["image_size"])
    period = float(g["timescale"])
    ev, gt_flow = g["events"], g["gt_flow"]
    slv = ref_solver_for(H, W, True, scale=3)
    s = int(g["burgers__scale"])
    assert s == slv.patch_scales - 1
    slv.overload_patch_configuration(s)
    slv.current_scale = s
    best = {s: g["burgers__motion"]}
    with_mask = slv.calculate_flow_error(best, gt_flow, timescale=period, events=ev)
    without = slv.calculate_flow_error(best, gt_flow, timescale=period)
    pred_only = slv.calculate_fwl_pred(best, ev, period)
    dense = np.asarray(slv.motion_to_dense_flow(best, period))
    assert np.abs(dense - g["burgers__dense"]).max() > SEPARATION * np.abs(dense).max()  # not the scale_later: False voxel
    out["flow_error__dense"] = sub(dense)
    for k, v in with_mask.items():
        out[f"flow_error__mask__{k}"] = np.array(float(v))
    for k, v in without.items():
        out[f"flow_error__nomask__{k}"] = np.array(float(v))
    out["flow_error__fwl_pred_only"] = np.array(float(pred_only["PRED_FWL"]))
    print("flow_error", {k: round(float(v), 5) for k, v in with_mask.items()})


def main():
    install_cv2_resize()
    g = np.load(os.path.join(HERE, "solver_objective.npz"))
    H, W = (int(v) for v in g["image_size"])
    ev = g["events"]
    rng = np.random.default_rng(SEED + 20)
    out = {"vox_stride": np.array(VOX_STRIDE), "separation": np.array(SEPARATION)}
    # 1. Burgers, t0 middle, both pinned scales, the fixture's x.  Neither is in generic position: the replicate padding spreads
    # the value of a border patch over the band of pixels outside the outermost patch centres, so a maximum of D = -P x that sits
    # on a border patch is attained on a plateau (every tied pixel has the same interpolation row).  Scale 1 always is (its 2 x 2
    # patches are all corners), and the fixture's x of scale 3 has its largest entry on an edge patch.  `interior_s3` is that x with
    # the largest entry of -x moved to an interior patch: ONE arg-max pixel.
    one_case(out, "burgers_s1", ev, H, W, g["burgers_s1__x"], 1, "burgers", "middle", rng, "many")
    one_case(out, "burgers_s3", ev, H, W, g["burgers_s3__x"], 3, "burgers", "middle", rng, None)
    x = g["burgers_s3__x"].copy()
    x[3 * 8 + 4] = -(np.abs(x).max() + 40.0)
    one_case(out, "interior_s3", ev, H, W, x, 3, "burgers", "middle", rng, "one")
    # 2. the other scheme, the other t0
    one_case(out, "upwind_s1", ev, H, W, g["burgers_s1__x"], 1, "upwind", "middle", rng, "many")
    one_case(out, "burgers_first_s1", ev, H, W, g["burgers_s1__x"], 1, "burgers", "first", rng, "many")
    # 3. plateau: the largest entry of D = -P x sits on a corner patch, whose value the replicate padding spreads over the border
    x = g["burgers_s3__x"].copy()
    x[0] = -(np.abs(x).max() + 40.0)
    one_case(out, "plateau_s3", ev, H, W, x, 3, "burgers", "middle", rng, "many")
    # 4. negative scale: every entry of x positive -> D < 0 -> s < 0
    one_case(out, "negative_s3", ev, H, W, np.abs(g["burgers_s3__x"]) + 20.0, 3, "burgers", "middle", rng, None)
    assert float(out["negative_s3__scale"]) < 0
    # 5. the metrics main.py asks for
    gen_flow_error(out)
    out["cases"] = np.array(["burgers_s1", "burgers_s3", "interior_s3", "upwind_s1", "burgers_first_s1", "plateau_s3", "negative_s3"])
    out["shims"] = np.array(ref_import.SHIMS)
    out["extra_shim"] = np.array(EXTRA_SHIM)
    out["seed"] = np.array(SEED + 20)
    path = os.path.join(HERE, "solver_scale_later.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
