"""Coarse-to-fine patch solver on the GPU objective (SURVEY.md section 8f rank 4 -- a "next" row).

Same constructor signature, config keys, registry name and return value as the reference's
`PyramidalPatchContrastMaximization` (src/solver/patch_contrast_pyramid.py:31-67, 149-177), so
`solver.collections["pyramidal_patch_contrast_maximization"](image_shape, calib, solver_cfg,
optimizer_cfg, output_cfg, None).optimize(events)` works as in `main.py:141-179`.

What is the same: the patch grids per scale (prepare_patch / prepare_pyramidal_patch, lines 69-100),
the objective per scale (`PatchFlowObjective` == `objective_scipy`, pinned by golden fixtures), the
SciPy method and options, warm start from the previous frame, fine-to-coarse feedback.
The per-patch re-initialisation at finer scales (initialize_guess_from_optuna_sampling, lines 320-353) uses the
reference's small-patch cost (calculate_cost_for_small_patch, 372-414: pinned by tests/golden/patch_search.npz) and
the reference's search box (sampling_initial, 417-428) -- but the trial points come from a regular grid scored in
one GPU launch (CMaxHandle.patch_search / cmax_patch_search) instead of Optuna's sequential TPE sampler.
What differs, and is NOT pinned against the reference (its dependencies are absent from this image and
its trajectories depend on Optuna's TPE sampler):
  * WHICH points of the search box are tried (grid vs. TPE), hence the starting point of the finer scales;
  * skimage.transform.pyramid_expand / pyramid_reduce (lines 220-222, 265-267) are restated with
    scipy.ndimage (order-1 zoom + Gaussian sigma = 2*2/6, 'reflect') on the tiny [2,ph,pw] arrays.
These are host-side operations on a few hundred numbers between scales, not part of the hot path.
"""
import logging
import os
from typing import Dict, Optional

import numpy as np
import scipy.ndimage as ndi

from ..cmax import CMaxHandle
from . import scipy_autograd
from .patch_objective import PatchFlowObjective
from .common import (DESCENT_OPTIMIZERS, DEVICE_QUASI_NEWTON, SCIPY_OPTIMIZERS, PatchSolverCommon, _check_key_and_bool, flow_regularizer_config, calculate_flow_error_numpy,  # noqa: F401
                     check_opt_method, global_best_refine, one_patch_guess, lbfgs_config, run_descent, run_lbfgs, whole_image_guess)

logger = logging.getLogger(__name__)


def search_box(m0: np.ndarray, abs_range: float = 10.0):
    """sampling_initial (patch_contrast_pyramid.py:417-428): per component the interval spanned by
    {0.8 m, m - 10, 1.2 m, m + 10}.  m0 [...]: -> (lo, hi) of the same shape."""
    c = np.stack([0.8 * m0, m0 - abs_range, 1.2 * m0, m0 + abs_range])
    return c.min(axis=0), c.max(axis=0)


def pyramid_expand(motion: np.ndarray) -> np.ndarray:
    """[2,h,w] -> [2,2h,2w]: skimage.transform.pyramid_expand(channel_axis=0) restated on scipy.ndimage -- order-1 resize
    (skimage's mode "reflect" is ndimage's "mirror" for the resampling step), then Gaussian smoothing with
    sigma = 2 * upscale / 6, for which skimage hands its mode string to ndimage unchanged ("reflect").  skimage is not
    in this image: the mapping follows its source as recalled, unpinned."""
    out = np.stack([ndi.zoom(c, 2, order=1, mode="mirror", grid_mode=True) for c in motion])
    return np.stack([ndi.gaussian_filter(c, 2 * 2 / 6.0, mode="reflect") for c in out])


def pyramid_reduce(motion: np.ndarray) -> np.ndarray:
    """[2,h,w] -> [2,ceil(h/2),ceil(w/2)]: Gaussian smoothing (sigma = 2 * downscale / 6, ndimage "reflect") then order-1
    down-sampling (ndimage "mirror"), as skimage.transform.pyramid_reduce does."""
    sm = np.stack([ndi.gaussian_filter(c, 2 * 2 / 6.0, mode="reflect") for c in motion])
    shape = (int(np.ceil(motion.shape[1] / 2)), int(np.ceil(motion.shape[2] / 2)))
    return np.stack([ndi.zoom(c, (shape[0] / c.shape[0], shape[1] / c.shape[1]), order=1, mode="mirror", grid_mode=True)
                     for c in sm])


class PyramidalPatchContrastMaximization(PatchSolverCommon):
    def __init__(self, image_shape: tuple, calibration_parameter: dict, solver_config: dict = {},
                 optimizer_config: dict = {}, output_config: dict = {}, visualize_module=None):
        self.image_shape = tuple(image_shape)
        self.calib_param = calibration_parameter
        self.slv_config = solver_config
        self.opt_config = optimizer_config
        self.out_config = output_config
        self.visualizer = visualize_module
        self.opt_method = optimizer_config["method"]
        check_opt_method(self.opt_method)
        if self.opt_method in DEVICE_QUASI_NEWTON:
            lbfgs_config(optimizer_config)  # (unknown keys of optimizer.lbfgs: KeyError, at construction)
        self.padding = solver_config["outer_padding"] if "outer_padding" in solver_config else 0
        self.iwe_config = solver_config["iwe"]
        if self.iwe_config["method"] != "bilinear_vote":
            raise NotImplementedError("the fused objective accumulates with bilinear_vote")
        self.motion_model = solver_config["motion_model"]
        self.motion_vector_size = 2
        self.cost_name = solver_config["cost"]
        self.cost_weight = solver_config.get("cost_with_weight") if self.cost_name == "hybrid" else None
        self.normalize_t_in_batch = True
        # time-aware set-up (src/solver/base.py:211-228)
        self.is_time_aware = _check_key_and_bool(solver_config, "time_aware")
        if self.is_time_aware:
            self.time_bin = solver_config["time_bin"]
            self.flow_interpolation = solver_config["flow_interpolation"]
            self.t0_flow_location = solver_config["t0_flow_location"]
            self.scale_later = _check_key_and_bool(solver_config, "scale_later")  # "Scaling before upwind", base.py:219-224
        else:
            self.time_bin, self.flow_interpolation, self.t0_flow_location = 0, "burgers", "middle"
            self.scale_later = False  # (the reference never reads the key without time_aware)
        # optional, absent = False: the fused terms see the float64 flow / voxel this solver optimises in, not its fp32 rounding
        # (PatchFlowObjective(exact_flow=True): the border cells of the reference's float64 arithmetic)
        self.exact_flow = _check_key_and_bool(solver_config, "exact_flow")
        self.flow_regularizer = flow_regularizer_config(solver_config, self.scale_later)  # optional, absent = None: no such term
        # pyramid (patch_contrast_pyramid.py:50-61)
        patch = solver_config["patch"]
        self.filter_type = patch["filter_type"]
        self.coarest_scale = 1
        self.patch_scales = patch["scale"]
        self.cropped_image_shape = (patch["crop_height"], patch["crop_width"])
        self.patch_shift = ((self.image_shape[0] - self.cropped_image_shape[0]) // 2,
                            (self.image_shape[1] - self.cropped_image_shape[1]) // 2)
        self.scaled_patch_size, self.scaled_patch_image_size, self.scaled_n_patch = {}, {}, {}
        for s in range(self.coarest_scale, self.patch_scales):
            size = (self.cropped_image_shape[0] // (2 ** s), self.cropped_image_shape[1] // (2 ** s))
            self.scaled_patch_size[s] = size
            # patch centres: np.arange(0, image - patch + slide, slide) + patch/2 with slide == patch (lines 87-91)
            self.scaled_patch_image_size[s] = (len(np.arange(0, self.cropped_image_shape[0], size[0])),
                                               len(np.arange(0, self.cropped_image_shape[1], size[1])))
            self.scaled_n_patch[s] = self.scaled_patch_image_size[s][0] * self.scaled_patch_image_size[s][1]
        self.total_n_patch = sum(self.scaled_n_patch.values())
        self.previous_frame_best_estimation: Optional[Dict[int, np.ndarray]] = None
        self.history = []  # (scale, OptimizeResult -- or, optimizer.method "SGD" / "Adam", the DescentResult)
        self.search_history = []  # (scale, candidates, loss, picked index) of the per-patch re-initialisation
        self._handle: Optional[CMaxHandle] = None
        self._objectives: Dict[int, PatchFlowObjective] = {}
        self._warper = self._imager = None  # built on first use by the metric / picture methods below
        self.iwe_visualize_max_scale = solver_config.get("max_scale", 50)

    # -- reference API (the warm start, metrics and pictures: PatchSolverCommon) ----------------------
    def initialize_random(self, n_patch: int) -> np.ndarray:
        x0 = np.random.rand(self.motion_vector_size, n_patch).astype(np.float64)
        p = self.opt_config["parameters"]
        x0[0] = x0[0] * (p["trans_x"]["max"] - p["trans_x"]["min"]) + p["trans_x"]["min"]
        x0[1] = x0[1] * (p["trans_y"]["max"] - p["trans_y"]["min"]) + p["trans_y"]["min"]
        return x0

    def optimize(self, events: np.ndarray) -> Dict[int, np.ndarray]:
        """events [n,4] (x row, y col, t, p) -> {scale: motion [2, ph, pw]} in pixel per time unit."""
        logger.info(f"DoF is {self.motion_vector_size * self.total_n_patch}")
        # one handle and one objective per scale for the life of the solver: the device workspaces, the sorted-event
        # buffers and the native plans are reused from frame to frame (main.py runs one solver over a whole sequence)
        if self._handle is None:
            # the per-scale objective warps with a DENSE flow: an event whose source pixel is off the sensor has no flow value (the
            # reference's gather indexes out of bounds there, src/warp.py:303-307) -- asked to be dropped while packing, and ...
            self._handle = CMaxHandle(self.image_shape, self.padding).set_keep_outside(False)
        # ... on_dropped="raise" (VERDICT r3 #8): a solver must not diverge from the reference silently
        handle = self._handle.set_events(events, time_bin=self.time_bin, on_dropped="raise")
        t = events[:, 2]
        t_scale = float(t.max() - t.min()) if self.normalize_t_in_batch else 1.0
        self.slab_history = []  # (scale, slab count in force when the scale's optimisation ended): large motions, DESIGN section 2
        best: Dict[int, np.ndarray] = {}
        self.history = []
        self.search_history = []
        for s in range(self.coarest_scale, self.patch_scales):
            pis = self.scaled_patch_image_size[s]
            objective = self._objectives.get(s)
            if objective is None:
                objective = self._objectives[s] = PatchFlowObjective(
                    handle, t_scale, pis, self.scaled_patch_size[s], self.scaled_patch_size[s], self.patch_shift,
                    cost=self.cost_name, cost_with_weight=self.cost_weight, blur_sigma=self.iwe_config["blur_sigma"],
                    time_aware=self.is_time_aware, time_bin=self.time_bin, flow_interpolation=self.flow_interpolation,
                    t0_flow_location=self.t0_flow_location, filter_type=self.filter_type, scale_later=self.scale_later,
                    exact_flow=self.exact_flow, flow_regularizer=self.flow_regularizer)
            else:
                objective.set_t_scale(t_scale)
            if self.previous_frame_best_estimation is not None and s == self.coarest_scale:
                x0 = np.copy(self.previous_frame_best_estimation[s]).reshape(-1)
            elif s > self.coarest_scale:
                x0 = pyramid_expand(best[s - 1])[:, : pis[0], : pis[1]].reshape(-1)
                if self.previous_frame_best_estimation is not None:
                    x0 = (x0 + self.previous_frame_best_estimation[s].reshape(-1)) / 2
                x0 = self.initialize_guess_from_patch_search(handle, s, x0)
            elif self.slv_config["patch"]["initialize"] == "zero":
                x0 = np.zeros(2 * self.scaled_n_patch[s])
            elif self.slv_config["patch"]["initialize"] == "global-best":  # patch_contrast_pyramid.py:292-297
                best_guess = self.initialize_guess_from_whole_image(handle, t_scale)
                x0 = np.tile(best_guess[None], (self.scaled_n_patch[s], 1)).T.reshape(-1)
            elif self.slv_config["patch"]["initialize"] == "grid-best":  # patch_contrast_pyramid.py:298-305
                best_guess = self.initialize_guess_from_patch(events, s, self.scaled_n_patch[s] // 2 - 1)
                x0 = np.tile(best_guess[None], (self.scaled_n_patch[s], 1)).T.reshape(-1)
            else:
                x0 = self.initialize_random(self.scaled_n_patch[s]).reshape(-1)
            if self.opt_method in DESCENT_OPTIMIZERS:  # run_torch's loop, device-resident, once per scale; the motion is x_best
                res = run_descent(objective, x0, self.opt_method, self.opt_config)
            elif self.opt_method in DEVICE_QUASI_NEWTON:  # L-BFGS, device-resident, once per scale; the motion is the last accepted point
                res = run_lbfgs(objective, x0, self.opt_config)
            else:
                res = scipy_autograd.minimize(objective, x0, method=self.opt_method, precision="float64",
                                              torch_device=str(handle.device),
                                              options={"gtol": 1e-5, "disp": False, "maxiter": self.opt_config["max_iter"]}
                                              if self.opt_method in ("Newton-CG", "BFGS", "CG", "L-BFGS-B", "trust-ncg", "trust-krylov")
                                              else {"maxiter": self.opt_config["max_iter"]})
            logger.info(f"Scale {s}: loss {res.fun}")
            self.history.append((s, res))
            self.slab_history.append((s, handle.time_slabs))
            best[s] = np.asarray(res.x).reshape((2,) + pis)
        self._last_handle, self._last_t_scale = handle, t_scale
        return self.update_coarse_from_fine(best)

    # -- grid initialisers of the coarsest scale: K candidates per library call ------------------------------------------
    def initialize_guess_from_whole_image(self, handle: CMaxHandle, t_scale: float) -> np.ndarray:
        """patch.initialize: "global-best" (src/solver/patch_contrast_base.py:164-187): the best of the 30 x 30 translations
        np.arange(-150, 150, 10)^2 for the WHOLE batch under the solver's own cost, warped as one 2-DoF motion (`motion * t_scale`,
        objective_scipy_for_patch 244-271).  900 objective evaluations in the reference, 900 / 32 cmax_objective_batch calls here,
        the batch in time slabs while the candidates are large (CMaxHandle.auto_time_slabs)."""
        if self.is_time_aware:
            raise NotImplementedError("global-best initialisation on a time-binned handle is not built (the 2-DoF search wants slabs)")
        # a 2-DoF warp would keep events from off the sensor; this handle dropped them on request (and raised if there were any)
        # (optional key patch.global_best_refine: the best grid points refined by a multi-start descent, the per-start results recorded)
        guess, loss, *refined = whole_image_guess(handle, t_scale, refine=global_best_refine(self.slv_config), **self._search_cost())
        self.search_history.append((self.coarest_scale, "global-best", loss, guess) + tuple(refined))
        logger.info(f"Initial value: best_guess = {guess}")
        return guess

    def initialize_guess_from_patch(self, events: np.ndarray, s: int, patch_index: int) -> np.ndarray:
        """patch.initialize: "grid-best" (src/solver/patch_contrast_base.py:126-162): np.arange(-150, 150, 30)^2 on the events of ONE
        patch (utils.crop_event with the patch's bounds), its own time span as t_scale; warper and imager stay full-size."""
        if self.is_time_aware:
            raise NotImplementedError("grid-best initialisation on a time-binned handle is not built")
        guess, loss = one_patch_guess(events, self.patch_boxes(s)[patch_index], self.image_shape, self.padding, self.normalize_t_in_batch,
                                      **self._search_cost())
        if loss is None:
            return guess
        self.search_history.append((s, "grid-best", loss, guess))
        logger.info(f"Initial value: best_guess = {guess}")
        return guess

    def patch_boxes(self, s: int) -> np.ndarray:
        """[n_patch, 4] = x_min, x_max, y_min, y_max of scale s: FlowPatch bounds (src/types/flow_patch.py:29-42) of the
        centres prepare_patch lays out (patch_contrast_base.py:86-105).  As in the reference, these boxes live on the
        CROPPED grid without the (image - crop) / 2 shift the dense interpolation applies (patch_contrast_pyramid.py:
        325-335 crops the raw events with them)."""
        h, w = self.scaled_patch_size[s]
        cx = np.arange(0, self.cropped_image_shape[0], h) + h / 2
        cy = np.arange(0, self.cropped_image_shape[1], w) + w / 2
        xx, yy = np.meshgrid(cx, cy, indexing="ij")
        xx, yy = xx.reshape(-1), yy.reshape(-1)
        return np.stack([(xx - np.ceil(h / 2)).astype(int), (xx + np.floor(h / 2)).astype(int),
                         (yy - np.ceil(w / 2)).astype(int), (yy + np.floor(w / 2)).astype(int)], axis=1)

    def initialize_guess_from_patch_search(self, handle: CMaxHandle, s: int, motion0: np.ndarray) -> np.ndarray:
        """Role of initialize_guess_from_optuna_sampling (patch_contrast_pyramid.py:320-353): per patch, the best
        translation inside sampling_initial's box around motion0 under the small-patch cost; patches with <= 10 events
        keep motion0.  n_iter / (s - coarsest) trials per patch like the reference, placed on a g x g grid
        (g = ceil(sqrt(trials)), or patch["search_grid"]) plus motion0 itself; all patches and trials in one launch."""
        m0 = np.asarray(motion0, dtype=np.float64).reshape(2, -1)  # [2, n_patch]
        n_patch = m0.shape[1]
        size = self.scaled_patch_size[s]
        if self.padding:
            # the reference's small-patch imager is padded by outer_padding (EventImageConverter(scaled_size, outer_padding));
            # cmax_patch_search votes into the un-padded patch image.  No shipped YAML uses a padding: refuse rather than
            # score the candidates on a different image
            raise NotImplementedError("per-patch re-initialisation with outer_padding != 0 is not built")
        if 2 * size[0] * size[1] * 4 > 64 * 1024 - 256:  # patch image beyond the workgroup's LDS (scale 1 of a large crop)
            logger.info(f"Scale {s}: patch {size} too large for the batched search, keeping the expanded motion")
            return m0.reshape(-1)
        trials = max(1, int(np.ceil(self.opt_config["n_iter"] / (s - self.coarest_scale))))
        g = int(self.slv_config["patch"].get("search_grid", int(np.ceil(np.sqrt(trials)))))
        if g <= 0:  # search_grid: 0 switches the re-initialisation off (A/B runs)
            return m0.reshape(-1)
        lo, hi = search_box(m0)  # [2, n_patch]
        u = np.linspace(0.0, 1.0, g) if g > 1 else np.array([0.5])
        gx = lo[0][:, None] + (hi[0] - lo[0])[:, None] * u[None, :]  # [n_patch, g]
        gy = lo[1][:, None] + (hi[1] - lo[1])[:, None] * u[None, :]
        cand = np.stack([np.repeat(gx, g, axis=1), np.tile(gy, (1, g))], axis=-1)  # [n_patch, g*g, 2]
        cand = np.concatenate([m0.T[:, None, :], cand], axis=1)
        loss, _, count = handle.patch_search(self.patch_boxes(s), size, cand, self.iwe_config["blur_sigma"])
        loss = loss.cpu().numpy()
        # the reference turns a NaN loss into 0.0 (calculate_cost_for_small_patch / objective_initial,
        # patch_contrast_pyramid.py:376-378, 411-414) -- under "minimize" that trial then wins; mirrored as it is
        loss[np.isnan(loss)] = 0.0
        pick = loss.argmin(axis=1)
        m1 = cand[np.arange(n_patch), pick].T.copy()  # [2, n_patch]
        keep = count.cpu().numpy() <= 10
        m1[:, keep] = m0[:, keep]
        self.search_history.append((s, cand, loss, pick))
        return m1.reshape(-1)

    def update_coarse_from_fine(self, motion_per_scale: dict) -> dict:
        """patch_contrast_pyramid.py:205-222: the finest motion, and below it the reduced OPTIMISED motion of the next finer
        scale -- keys finest ... coarsest - 1, exactly the reference's (the extra key coarsest - 1 is never read)."""
        finest, coarsest = max(motion_per_scale), min(motion_per_scale)
        refined = {finest: motion_per_scale[finest]}
        for i in range(finest, coarsest - 1, -1):
            refined[i - 1] = pyramid_reduce(motion_per_scale[i])
        return refined

    def motion_to_dense_flow(self, motion_per_scale: dict, t_scale: float = 1.0) -> np.ndarray:
        """Finest-scale motion -> dense flow [2,H,W] in pixel per time unit (patch_contrast_pyramid.py:464-516); time-aware solvers:
        the flow voxel [time_bin,2,H,W] propagated from it at displacement scale (flow * t_scale through the Burgers / upwind chain,
        divided by t_scale again); with `scale_later` the flow is also divided by its signed maximum before the chain and the voxel
        multiplied by it afterwards (the numpy branch of lines 489-504)."""
        import torch

        from .. import functional as F
        from ..utils.flow_utils import construct_dense_flow_voxel_torch
        from .patch_objective import patch_pad

        s = max(motion_per_scale)
        ps = self.scaled_patch_size[s]
        m = torch.as_tensor(np.asarray(motion_per_scale[s]), dtype=torch.float64, device="cuda")
        dense = F.patch_to_dense(m, self.image_shape, ps, patch_pad(ps, ps, self.patch_shift), self.filter_type)
        if not self.is_time_aware:
            return dense.cpu().numpy()
        scale = F.field_max(dense) if self.scale_later else 1.0
        voxel = construct_dense_flow_voxel_torch(dense * t_scale / scale, self.time_bin, self.flow_interpolation,
                                                 t0_location=self.t0_flow_location) * scale / t_scale
        return voxel.cpu().numpy()
