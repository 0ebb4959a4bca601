"""Single-scale patch solvers on the GPU objective.

Same constructor signature, config keys, registry name and return value as the reference's
`MixedPatchContrastMaximization` (src/solver/patch_contrast_mixed.py:17-208) and `TimeAwarePatchContrastMaximization`
(src/solver/time_aware_patch_contrast.py:12-79, registered as "time_aware_mixed_patch_contrast_maximization" in
src/solver/__init__.py:14-19): ONE patch grid at one scale, laid out by `patch.size` and `patch.sliding_window` (overlapping
windows allowed), optimised by `scipy_autograd.minimize` from one of the `patch.initialize` starting points.

What is the same: the grid (prepare_patch, src/solver/patch_contrast_base.py:73-105), the padding and the filter of the patch ->
dense interpolation (462-506, `patch.filter_type` "bilinear" or "nearest"), the objective (objective_scipy, patch_contrast_mixed.py:
184-208 == one `PatchFlowObjective`), SciPy's options (gtol 1e-7, maxiter, float64), the warm start, the grid initialisers.
What is refused, with the reason in the exception: `solver.scale_later` on these classes (the reference rescales by the maximum of the
PATCH ARRAY, time_aware_patch_contrast.py:52-55, the plan by the maximum of the DENSE FLOW -- different maps), Optuna (absent).
"""
import logging
from typing import Optional

import numpy as np

from ..cmax import CMaxHandle
from . import scipy_autograd
from .common import (DESCENT_OPTIMIZERS, DEVICE_QUASI_NEWTON, PatchSolverCommon, _check_key_and_bool, check_opt_method, flow_regularizer_config, global_best_refine, one_patch_guess,
                     lbfgs_config, run_descent, run_lbfgs, whole_image_guess)
from .patch_objective import PatchFlowObjective, patch_pad

logger = logging.getLogger(__name__)


def _pair(value, what: str) -> tuple:
    """set_patch_size_and_sliding_window (patch_contrast_base.py:51-71): an int or a list."""
    if isinstance(value, int):
        return (value, value)
    if isinstance(value, list):
        return tuple(value)
    raise TypeError(f"Unsupported type for {what}.")


class MixedPatchContrastMaximization(PatchSolverCommon):
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
        self.motion_model_keys = ["trans_x", "trans_y"]  # Warp.get_key_names("2d-translation")
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
            if _check_key_and_bool(solver_config, "scale_later"):
                raise NotImplementedError(
                    "solver.scale_later is not built for the single-scale patch solvers: the reference divides the flow by the maximum of "
                    "the PATCH ARRAY there (time_aware_patch_contrast.py:52-55), the native plan's scale_later by the maximum of the "
                    "DENSE FLOW (patch_contrast_pyramid.py:489-490) -- a different map, not substituted silently")
        else:
            self.time_bin, self.flow_interpolation, self.t0_flow_location = 0, "burgers", "middle"
        self.scale_later = False
        self.exact_flow = _check_key_and_bool(solver_config, "exact_flow")  # optional, as in the pyramid solver
        self.flow_regularizer = flow_regularizer_config(solver_config)  # optional, as in the pyramid solver
        # one grid at one scale (patch_contrast_base.py:36-49, patch_contrast_mixed.py:45-54)
        patch = solver_config["patch"]
        if patch.get("initialize") == "optuna-sampling":
            raise NotImplementedError("patch.initialize 'optuna-sampling' is not built: Optuna is not a dependency of this package")
        self.filter_type = patch["filter_type"]
        self.patch_shift = (0, 0)
        self.patch_size = _pair(patch["size"], "patch")
        self.sliding_window = _pair(patch["sliding_window"], "sliding_window")
        self.patch_image_size = self.prepare_patch(self.image_shape, self.patch_size, self.sliding_window)
        self.n_patch = self.patch_image_size[0] * self.patch_image_size[1]
        self._patch_motion_model_keys = [f"patch{i}_{k}" for i in range(self.n_patch) for k in self.motion_model_keys]
        self.previous_frame_best_estimation: Optional[np.ndarray] = None
        self.history = []         # OptimizeResult (optimizer.method "SGD" / "Adam": DescentResult) per frame
        self.search_history = []  # (initialiser, losses of every candidate, pick) per frame
        self._handle: Optional[CMaxHandle] = None
        self._search_handle: Optional[CMaxHandle] = None  # un-binned twin of a time-binned handle, for the 2-DoF grid search
        self._objective: Optional[PatchFlowObjective] = None
        self._warper = self._imager = None
        self.iwe_visualize_max_scale = solver_config.get("max_scale", 50)

    # -- geometry ----------------------------------------------------------------------------------------------
    @staticmethod
    def prepare_patch(image_size, patch_size, sliding_window) -> tuple:
        """(ph, pw) of prepare_patch (patch_contrast_base.py:86-92): one patch per centre
        np.arange(0, image - patch + slide, slide) + patch / 2 along each axis."""
        return (len(np.arange(0, image_size[0] - patch_size[0] + sliding_window[0], sliding_window[0])),
                len(np.arange(0, image_size[1] - patch_size[1] + sliding_window[1], sliding_window[1])))

    def patch_boxes(self) -> np.ndarray:
        """[n_patch, 4] = x_min, x_max, y_min, y_max: FlowPatch bounds (src/types/flow_patch.py:29-42) of the centres, row-major
        over the grid like the reference's `patches` dict."""
        (h, w), (sh, sw) = self.patch_size, self.sliding_window
        cx = np.arange(0, self.image_shape[0] - h + sh, sh) + h / 2
        cy = np.arange(0, self.image_shape[1] - w + sw, sw) + w / 2
        xx, yy = np.meshgrid(cx, cy, indexing="ij")
        xx, yy = xx.reshape(-1), yy.reshape(-1)
        return np.stack([(xx - np.ceil(h / 2)).astype(int), (xx + np.floor(h / 2)).astype(int),
                         (yy - np.ceil(w / 2)).astype(int), (yy + np.floor(w / 2)).astype(int)], axis=1)

    @property
    def pad(self) -> tuple:
        return patch_pad(self.patch_size, self.sliding_window, self.patch_shift)

    # -- starting points (patch_contrast_base.py:108-187, patch_contrast_mixed.py:134-164) ----------------------------
    def initialize_random(self) -> np.ndarray:
        x0 = np.random.rand(self.motion_vector_size, self.n_patch).astype(np.float64)
        p = self.opt_config["parameters"]
        x0[0] = x0[0] * (p["trans_x"]["max"] - p["trans_x"]["min"]) + p["trans_x"]["min"]
        x0[1] = x0[1] * (p["trans_y"]["max"] - p["trans_y"]["min"]) + p["trans_y"]["min"]
        return x0

    def initialize_zeros(self) -> np.ndarray:
        return np.zeros((self.motion_vector_size, self.n_patch), dtype=np.float64)

    def _translation_handle(self, events: np.ndarray) -> CMaxHandle:
        """The handle the 2-DoF search runs on: the solver's own, or -- that one being time-binned -- an un-binned second handle
        holding the same batch (the 2-DoF search wants time slabs), kept across frames like the first."""
        if not self.is_time_aware:
            return self._handle
        if self._search_handle is None:
            self._search_handle = CMaxHandle(self.image_shape, self.padding).set_keep_outside(False)
        return self._search_handle.set_events(events, on_dropped="raise")

    def initialize_guess_from_whole_image(self, events: np.ndarray) -> np.ndarray:
        """patch.initialize "global-best": common.whole_image_guess over the whole batch; with the optional key patch.global_best_refine
        its best grid points are refined by a multi-start descent (the per-start results are then recorded behind the guess)."""
        guess, loss, *refined = whole_image_guess(self._translation_handle(events), self._batch_t_scale(events),
                                                  refine=global_best_refine(self.slv_config), **self._search_cost())
        self.search_history.append(("global-best", loss, guess) + tuple(refined))
        logger.info(f"Initial value: best_guess = {guess}")
        return guess

    def initialize_guess_from_patch(self, events: np.ndarray, patch_index: int = 1) -> np.ndarray:
        """patch.initialize "grid-best": common.one_patch_guess on the events of patch `patch_index`."""
        guess, loss = one_patch_guess(events, self.patch_boxes()[patch_index], self.image_shape, self.padding, self.normalize_t_in_batch,
                                      **self._search_cost())
        self.search_history.append(("grid-best", loss, guess))
        logger.info(f"Initial value: best_guess = {guess}")
        return guess

    def initial_motion(self, events: np.ndarray) -> np.ndarray:
        if self.previous_frame_best_estimation is not None:
            return np.copy(self.previous_frame_best_estimation).reshape(-1)
        how = self.slv_config["patch"]["initialize"]
        if how == "random":
            return self.initialize_random().reshape(-1)
        if how == "zero":
            return self.initialize_zeros().reshape(-1)
        if how == "global-best":
            return np.tile(self.initialize_guess_from_whole_image(events)[None], (self.n_patch, 1)).T.reshape(-1)
        if how == "grid-best":
            return np.tile(self.initialize_guess_from_patch(events, self.n_patch // 2 - 1)[None], (self.n_patch, 1)).T.reshape(-1)
        raise NotImplementedError(f"patch.initialize {how!r}")

    # -- objective and optimisation ----------------------------------------------------------------------------------
    def prepare_objective(self, events: np.ndarray) -> PatchFlowObjective:
        """The batch onto the solver's handle and its duration into the solver's ONE objective (objective_scipy,
        patch_contrast_mixed.py:184-208): both live as long as the solver (main.py runs one solver over a sequence)."""
        if self._handle is None:
            # dense-flow warps: an event whose source pixel is off the sensor has no flow value; dropped while packing on request,
            # and on_dropped="raise" so that the solver never diverges from the reference silently (as the pyramid solver does)
            self._handle = CMaxHandle(self.image_shape, self.padding).set_keep_outside(False)
        handle = self._handle.set_events(events, time_bin=self.time_bin, on_dropped="raise")
        t_scale = self._batch_t_scale(events) if self.normalize_t_in_batch else 1.0
        if self._objective is None:
            self._objective = PatchFlowObjective(
                handle, t_scale, self.patch_image_size, self.patch_size, self.sliding_window, self.patch_shift,
                cost=self.cost_name, cost_with_weight=self.cost_weight, blur_sigma=self.iwe_config["blur_sigma"],
                time_aware=self.is_time_aware, time_bin=self.time_bin, flow_interpolation=self.flow_interpolation,
                t0_flow_location=self.t0_flow_location, filter_type=self.filter_type, scale_later=False, exact_flow=self.exact_flow,
                flow_regularizer=self.flow_regularizer)
        else:
            self._objective.set_t_scale(t_scale)
        return self._objective

    def optimize(self, events: np.ndarray) -> np.ndarray:
        """events [n,4] (x row, y col, t, p) -> motion [2, ph, pw] in pixel per time unit (run_scipy, patch_contrast_mixed.py:133-182)."""
        logger.info(f"DoF is {self.motion_vector_size * self.n_patch}")
        objective = self.prepare_objective(events)
        motion0 = self.initial_motion(events)
        if self.opt_method in DESCENT_OPTIMIZERS:  # run_torch's loop (src/solver/base.py:840-881), device-resident; the motion is x_best
            res = run_descent(objective, motion0, self.opt_method, self.opt_config)
        elif self.opt_method in DEVICE_QUASI_NEWTON:  # L-BFGS, device-resident; the motion is the last accepted point
            res = run_lbfgs(objective, motion0, self.opt_config)
        else:
            res = scipy_autograd.minimize(objective, motion0, method=self.opt_method, precision="float64",
                                          torch_device=str(self._handle.device),
                                          options={"gtol": 1e-7, "disp": False, "maxiter": self.opt_config["max_iter"]}
                                          if self.opt_method in ("Newton-CG", "BFGS", "CG", "L-BFGS-B", "trust-ncg", "trust-krylov")
                                          else {"maxiter": self.opt_config["max_iter"]})
        logger.info(f"End optimization: loss {res.fun}")
        self.history.append(res)
        return np.asarray(res.x).reshape((self.motion_vector_size,) + self.patch_image_size)

    def motion_to_dense_flow(self, motion: np.ndarray, t_scale: float = 1.0) -> np.ndarray:
        """A result [2, ph, pw] -> dense flow [2,H,W] in pixel per time unit (patch_contrast_base.py:392-460); time-aware solvers:
        the flow voxel [time_bin,2,H,W] propagated from it at displacement scale (flow * t_scale through the Burgers / upwind chain,
        divided by t_scale again), what objective_scipy warps with."""
        import torch

        from .. import functional as F
        from ..utils.flow_utils import construct_dense_flow_voxel_torch

        m = torch.as_tensor(np.asarray(motion), dtype=torch.float64, device="cuda").reshape((2,) + self.patch_image_size)
        dense = F.patch_to_dense(m, self.image_shape, self.sliding_window, self.pad, self.filter_type)
        if not self.is_time_aware:
            return dense.cpu().numpy()
        voxel = construct_dense_flow_voxel_torch(dense * t_scale, self.time_bin, self.flow_interpolation,
                                                 t0_location=self.t0_flow_location) / t_scale
        return voxel.cpu().numpy()


class TimeAwarePatchContrastMaximization(MixedPatchContrastMaximization):
    def __init__(self, image_shape: tuple, calibration_parameter: dict, solver_config: dict = {},
                 optimizer_config: dict = {}, output_config: dict = {}, visualize_module=None):
        super().__init__(image_shape, calibration_parameter, solver_config, optimizer_config, output_config, visualize_module)
        assert self.is_time_aware
