"""What the patch solvers share besides their optimisation loops: the methods `main.py` calls on a solver (metrics, pictures, the
warm start) and the two grid initialisers of `patch.initialize` ("global-best", "grid-best").  `PyramidalPatchContrastMaximization`
(pyramid.py) and the single-scale classes of mixed.py derive from `PatchSolverCommon`; a subclass provides `motion_to_dense_flow`."""
import logging
import os
from typing import Optional

import numpy as np

from ..cmax import CMaxHandle
from .translation_search import ONE_PATCH_FIELD, WHOLE_IMAGE_FIELD, grid_search_translation

logger = logging.getLogger(__name__)

SCIPY_OPTIMIZERS = ["Nelder-Mead", "Powell", "CG", "BFGS", "Newton-CG", "L-BFGS-B", "TNC", "COBYLA", "SLSQP",
                    "trust-constr", "dogleg", "trust-ncg", "trust-exact", "trust-krylov"]
# first-order methods of the reference's TORCH_OPTIMIZERS (src/solver/base.py:38-52) that run as a device-resident loop
# (PatchFlowObjective.descend: n_iter iterations per library call); the other eleven names are not built
DESCENT_OPTIMIZERS = ["SGD", "Adam"]
# quasi-Newton methods that run as a device-resident loop (PatchFlowObjective.minimize_lbfgs: a budget of optimizer.n_iter evaluations per
# library call; not in the reference, whose "LBFGS" is torch.optim's and is not built)
DEVICE_QUASI_NEWTON = ["device-L-BFGS"]
LBFGS_KEYS = ("history", "gtol", "max_move", "c1", "shrink", "max_ls", "step0")  # optimizer.lbfgs


def check_opt_method(method: str):
    """The solver classes' `optimizer.method`: a SciPy method or a device-resident first-order method; everything else -- the rest of
    the reference's TORCH_OPTIMIZERS, Optuna -- raises NotImplementedError with what is built."""
    if method == "optuna":
        raise NotImplementedError("opt_method 'optuna' is not built: Optuna is not a dependency of this package "
                                  f"(SciPy methods and the device-resident {DESCENT_OPTIMIZERS})")
    if method not in SCIPY_OPTIMIZERS and method not in DESCENT_OPTIMIZERS and method not in DEVICE_QUASI_NEWTON:
        raise NotImplementedError(f"Optimizer {method} is not supported (SciPy methods, and of torch.optim the device-resident {DESCENT_OPTIMIZERS} only; "
                                  f"the device-resident quasi-Newton solve is {DEVICE_QUASI_NEWTON})")


def run_descent(objective, x0: np.ndarray, method: str, opt_config: dict):
    """SolverBase.run_torch (src/solver/base.py:840-881) with its constants: lr 0.05, StepLR(n_iter, 0.1), optimizer.n_iter iterations,
    torch's defaults for the optimiser itself -- one PatchFlowObjective.descend call.  -> _lib.DescentResult (its x is x_best)."""
    return objective.descend(x0, method=method, n_iter=int(opt_config["n_iter"]), lr=0.05, lr_step=None, lr_decay=0.1)


def lbfgs_config(opt_config: dict) -> dict:
    """The optional key optimizer.lbfgs: {history, gtol, max_move, c1, shrink, max_ls, step0} (not in the reference); {} when absent."""
    cfg = opt_config.get("lbfgs") or {}
    unknown = sorted(set(cfg) - set(LBFGS_KEYS))
    if unknown:
        raise KeyError(f"optimizer.lbfgs: unknown keys {unknown} (known: {list(LBFGS_KEYS)})")
    return dict(cfg)


def run_lbfgs(objective, x0: np.ndarray, opt_config: dict):
    """optimizer.method "device-L-BFGS": one PatchFlowObjective.minimize_lbfgs call with a budget of optimizer.n_iter evaluations (the key
    run_torch reads) and the optional optimizer.lbfgs values.  -> _lib.LbfgsResult (its x is the last accepted point)."""
    return objective.minimize_lbfgs(x0, n_eval=int(opt_config["n_iter"]), **lbfgs_config(opt_config))


def _check_key_and_bool(config: dict, key: str) -> bool:
    return key in config.keys() and bool(config[key])


REFINE_KEYS = ("top_k", "n_iter", "method", "lr")  # patch.global_best_refine


def global_best_refine(slv_config: dict) -> Optional[dict]:
    """The optional solver key patch.global_best_refine: {top_k, n_iter, method, lr} (not in the reference): None when absent."""
    refine = slv_config.get("patch", {}).get("global_best_refine")
    if refine is None:
        return None
    unknown = sorted(set(refine) - set(REFINE_KEYS))
    if unknown:
        raise KeyError(f"patch.global_best_refine: unknown keys {unknown} (known: {list(REFINE_KEYS)})")
    return dict(refine)


def flow_regularizer_config(slv_config: dict, scale_later: bool = False) -> Optional[dict]:
    """The optional solver key solver.flow_regularizer: {kind: divergence | area, weight, eps, s} (not in the reference; the remedy
    for event collapse, PatchFlowObjective.set_flow_regularizer): None when absent -- the solver then makes not one call more.
    Checked here, at construction: the parameters, and `scale_later`, whose flow is rescaled by its maximum."""
    cfg = slv_config.get("flow_regularizer")
    if cfg is None:
        return None
    from .. import _lib

    _lib.flow_regularizer_from_config(cfg)  # raises on unknown keys / kinds and bad parameters
    if scale_later:
        raise NotImplementedError("solver.flow_regularizer is not built with solver.scale_later: that flow is divided by its maximum before "
                                  "the propagation and multiplied by it afterwards, so the regularised field would not be the one the events are warped by")
    return dict(cfg)


def whole_image_guess(handle: CMaxHandle, t_scale: float, refine: Optional[dict] = None, **search_cost):
    """patch.initialize: "global-best" (src/solver/patch_contrast_base.py:164-187): the best of the 30 x 30 translations
    np.arange(-150, 150, 10)^2 for the WHOLE batch under the solver's own cost, warped as one 2-DoF motion (`motion * t_scale`,
    objective_scipy_for_patch 244-271).  900 objective evaluations in the reference, 900 / 32 cmax_objective_batch calls here,
    the batch in time slabs while the candidates are large (CMaxHandle.auto_time_slabs).  -> (guess [2], losses [30, 30])
    refine = {top_k (4), n_iter, method, lr} (patch.global_best_refine; None: exactly the calls above, nothing more): the top_k best grid
    points are the starts of a multi-start descent (translation_search.refine_translation), start 0 being the grid's pick -- so the
    refined guess is never worse than it.  -> (guess [2], losses [30, 30], per-start DescentResults)"""
    if refine is None:
        return grid_search_translation(handle, t_scale, WHOLE_IMAGE_FIELD, **search_cost)
    refine = dict(refine)
    top_k = int(refine.pop("top_k", 4))
    return grid_search_translation(handle, t_scale, WHOLE_IMAGE_FIELD, refine_top=top_k, refine=refine, **search_cost)


def one_patch_guess(events: np.ndarray, box, image_shape, padding: int, normalize_t: bool = True, **search_cost):
    """patch.initialize: "grid-best" (src/solver/patch_contrast_base.py:126-162): np.arange(-150, 150, 30)^2 on the events of ONE
    patch (utils.crop_event with the patch's bounds `box` = x_min, x_max, y_min, y_max), its own time span as t_scale; warper and
    imager stay full-size.  -> (guess [2], losses [10, 10] or None when the patch holds no event)"""
    x0, x1, y0, y1 = box
    m = (x0 <= events[:, 0]) & (events[:, 0] < x1) & (y0 <= events[:, 1]) & (events[:, 1] < y1)
    cropped = events[m]
    if len(cropped) == 0:  # "No events in the patch": every loss is 0, the first candidate wins
        return np.array([float(ONE_PATCH_FIELD[0]), float(ONE_PATCH_FIELD[0])]), None
    t_scale = float(cropped[:, 2].max() - cropped[:, 2].min()) if normalize_t else 1.0
    sub = CMaxHandle(image_shape, padding).set_events(cropped)
    try:
        return grid_search_translation(sub, t_scale, ONE_PATCH_FIELD, **search_cost)
    finally:
        sub.close()


class PatchSolverCommon:
    # -- reference API ---------------------------------------------------------------------------
    def set_previous_frame_best_estimation(self, previous_best):
        self.previous_frame_best_estimation = previous_best.copy() if isinstance(previous_best, dict) else np.copy(previous_best)

    def _search_cost(self) -> dict:
        return {"cost": self.cost_name, "cost_with_weight": self.cost_weight, "sigma": self.iwe_config["blur_sigma"]}

    # -- what main.py calls on a solver besides optimize(): metrics and (optional) pictures ---------------------------------------
    # (src/solver/base.py:230-250, 272-420, 543-660 and their overrides in patch_contrast_pyramid.py:518-660.)  The arithmetic of the
    # metrics is the library's (Warp / EventImageConverter / costs over the HIP kernels) plus host NumPy for the end-point errors;
    # the pictures are drawn by whatever `visualize_module` the caller passed -- without one every visualize_* returns at once.
    @property
    def motion_model_for_dense_warp(self) -> str:
        return "dense-flow-voxel" if self.is_time_aware else "dense-flow"

    @property
    def warper(self):
        if self._warper is None:
            from ..warp import Warp

            self._warper = Warp(self.image_shape, calculate_feature=True, normalize_t=self.normalize_t_in_batch, calib_param=self.calib_param)
        return self._warper

    @property
    def imager(self):
        if self._imager is None:
            from ..event_image_converter import EventImageConverter

            self._imager = EventImageConverter(self.image_shape, outer_padding=self.padding)
        return self._imager

    def get_original_flow_from_time_aware_flow_voxel(self, flow_voxel: np.ndarray) -> np.ndarray:
        """[(b,) time_bin, 2, H, W] -> the slice the flow was given at (src/solver/base.py:230-250)."""
        if flow_voxel.ndim == 4:
            flow_voxel = flow_voxel[None]
        if self.t0_flow_location == "first":
            orig_ind = 0
        elif self.t0_flow_location == "middle":
            orig_ind = flow_voxel.shape[1] // 2
        else:
            raise NotImplementedError(f"t0_flow_location {self.t0_flow_location}")
        return np.squeeze(flow_voxel[:, orig_ind])

    def create_clipped_iwe_for_visualization(self, events: np.ndarray, max_scale=50) -> np.ndarray:
        """src/solver/base.py:272-291: un-blurred IWE as an inverted 8-bit picture, padding cut off."""
        assert events.shape[-1] <= 4, "this function is for events"
        if hasattr(events, "detach"):
            events = events.clone().detach().cpu().numpy()
        im = self.imager.create_image_from_events_numpy(events, method=self.iwe_config["method"], sigma=0)
        clipped_iwe = 255 - np.clip(max_scale * im, 0, 255).astype(np.uint8)
        if self.padding > 0:
            clipped_iwe = clipped_iwe[self.padding: -self.padding, self.padding: -self.padding]
        return clipped_iwe

    @staticmethod
    def _batch_t_scale(events: np.ndarray) -> float:
        return float(np.max(events[:, 2]) - np.min(events[:, 2]))

    def visualize_one_batch_warp(self, events: np.ndarray, warp: Optional[dict] = None):
        """patch_contrast_pyramid.py:518-536."""
        if self.visualizer is None:
            return
        flow = None
        if warp is not None:
            flow = self.motion_to_dense_flow(warp)
            if self.normalize_t_in_batch:
                flow = flow * self._batch_t_scale(events)
            events, _ = self.warper.warp_event(events, flow, self.motion_model_for_dense_warp)
            if self.is_time_aware:
                flow = self.get_original_flow_from_time_aware_flow_voxel(flow)
        clipped_iwe = self.create_clipped_iwe_for_visualization(events, max_scale=self.iwe_visualize_max_scale)
        self.visualizer.visualize_image(clipped_iwe)
        if warp is not None:
            self.visualizer.visualize_optical_flow_on_event_mask(flow, events)
            self.visualizer.visualize_overlay_optical_flow_on_event(flow, clipped_iwe)

    def visualize_one_batch_warp_gt(self, events: np.ndarray, gt_warp: np.ndarray, motion_model: str = "dense-flow"):
        """src/solver/base.py:313-330; gt_warp [H, W, 2] for "dense-flow"."""
        if self.visualizer is None:
            return
        if motion_model == "dense-flow":
            gt_warp = np.transpose(gt_warp, (2, 0, 1))
        events, _ = self.warper.warp_event(events, gt_warp, motion_model=motion_model)
        clipped_iwe = self.create_clipped_iwe_for_visualization(events, max_scale=self.iwe_visualize_max_scale)
        self.visualizer.visualize_image(clipped_iwe)
        if motion_model == "dense-flow":
            self.visualizer.visualize_overlay_optical_flow_on_event(gt_warp, clipped_iwe)

    def visualize_original_sequential(self, events: np.ndarray):
        """src/solver/base.py:332-341."""
        if self.visualizer is None:
            return
        clipped_iwe = self.create_clipped_iwe_for_visualization(events, max_scale=self.iwe_visualize_max_scale)
        self.visualizer.visualize_image(clipped_iwe, file_prefix="original")

    def visualize_pred_sequential(self, events: np.ndarray, warp: dict):
        """patch_contrast_pyramid.py:538-558 (warped to the MIDDLE of the batch, as the reference's override does)."""
        if self.visualizer is None:
            return
        t_scale = self._batch_t_scale(events) if self.normalize_t_in_batch else 1.0
        flow = self.motion_to_dense_flow(warp, t_scale) * t_scale
        events, _ = self.warper.warp_event(events, flow, self.motion_model_for_dense_warp, direction="middle")
        clipped_iwe = self.create_clipped_iwe_for_visualization(events, max_scale=self.iwe_visualize_max_scale)
        if self.is_time_aware:
            flow = self.get_original_flow_from_time_aware_flow_voxel(flow)
        self.visualizer.visualize_image(clipped_iwe, file_prefix="pred_warp")
        self.visualizer.visualize_optical_flow_on_event_mask(flow, events, file_prefix="pred_masked")

    def visualize_gt_sequential(self, events: np.ndarray, gt_warp: np.ndarray, gt_type: str = "flow"):
        """src/solver/base.py:385-420; gt_warp [H, W, 2] displacement."""
        if self.visualizer is None:
            return
        if gt_type != "flow":
            raise NotImplementedError("the patch solver's ground truth is a flow")
        gt_flow = np.transpose(gt_warp, (2, 0, 1))
        events, _ = self.warper.warp_event(events, gt_flow, "dense-flow", direction="first")
        clipped_iwe = self.create_clipped_iwe_for_visualization(events, max_scale=self.iwe_visualize_max_scale)
        self.visualizer.visualize_image(clipped_iwe, file_prefix="gt_warp")
        self.visualizer.visualize_optical_flow(gt_flow[0], gt_flow[1], visualize_color_wheel=False, file_prefix="gt_flow")

    def calculate_flow_error(self, motion: dict, gt_flow: np.ndarray, timescale: float = 1.0,
                             events: Optional[np.ndarray] = None) -> dict:
        """patch_contrast_pyramid.py:560-599: EPE / nPE / AE of the predicted displacement against gt_flow [H, W, 2] (masked by
        the pixels that saw an event when `events` is given), plus the flow-warp-loss ratios of calculate_fwl."""
        gt_flow = np.transpose(gt_flow, (2, 0, 1))  # [2, H, W]
        pred_flow = self.motion_to_dense_flow(motion, timescale) * timescale
        if self.is_time_aware:
            pred_flow = self.get_original_flow_from_time_aware_flow_voxel(pred_flow)
        pred_flow = pred_flow[None]
        if events is not None:
            event_mask = self.imager.create_eventmask(events)
            if self.padding:
                event_mask = event_mask[..., self.padding: -self.padding, self.padding: -self.padding]
            fwl = self.calculate_fwl(motion, gt_flow, timescale, events)
        else:
            event_mask, fwl = None, {}
        flow_error = calculate_flow_error_numpy(gt_flow[None], pred_flow, event_mask=event_mask)
        flow_error.update(fwl)
        logger.info(f"{flow_error = } for time period {timescale} sec.")
        return flow_error

    def calculate_fwl(self, motion: dict, gt_flow: np.ndarray, timescale: float, events: np.ndarray) -> dict:
        """FWL (Stoffregen 2020) as the reference reports it, Var(IWE_orig) / Var(IWE): below 1 = sharper than the un-warped image
        (patch_contrast_pyramid.py:601-629).  gt_flow [2, H, W] displacement over the batch."""
        from .. import costs
        from ..warp import Warp

        orig_iwe = self.imager.create_iwe(events)
        gt_warper = Warp(self.image_shape, normalize_t=True)
        gt_warp, _ = gt_warper.warp_event(events, gt_flow, "dense-flow")
        gt_iwe = self.imager.create_iwe(gt_warp)
        gt_fwl = costs.NormalizedImageVariance().calculate({"orig_iwe": orig_iwe, "iwe": gt_iwe, "omit_boundary": False})
        fwl = {"GT_FWL": gt_fwl}
        fwl.update(self.calculate_fwl_pred(motion, events, timescale))
        return fwl

    def calculate_fwl_pred(self, motion: dict, events: np.ndarray, timescale: float = 1.0) -> dict:
        """patch_contrast_pyramid.py:631-660."""
        from .. import costs

        orig_iwe = self.imager.create_iwe(events)
        pred_flow = self.motion_to_dense_flow(motion, timescale) * timescale
        pred_warp, _ = self.warper.warp_event(events, pred_flow, self.motion_model_for_dense_warp)
        pred_iwe = self.imager.create_iwe(pred_warp)
        pred_fwl = costs.NormalizedImageVariance().calculate({"orig_iwe": orig_iwe, "iwe": pred_iwe, "omit_boundary": False})
        return {"PRED_FWL": pred_fwl}

    def save_flow_error_as_text(self, nth_frame: int, flow_error_dict: dict, fname: str = "flow_error_per_frame.txt"):
        """src/solver/base.py:651-660: one line per frame appended to <visualizer.save_dir>/<fname> (the working directory
        without a visualizer)."""
        save_file_name = os.path.join(self.visualizer.save_dir, fname) if self.visualizer is not None else fname
        with open(save_file_name, "a") as f:
            f.write(f"frame {nth_frame}::" + str(flow_error_dict) + "\n")


def calculate_flow_error_numpy(flow_gt: np.ndarray, flow_pred: np.ndarray, event_mask: Optional[np.ndarray] = None) -> dict:
    """End-point and angular errors of src/utils/flow_utils.py:705-758.  flow_gt / flow_pred [B, 2, H, W], event_mask [B, 1, H, W].
    Only pixels whose ground truth is finite and non-zero in both components count (and, with a mask, saw an event); n_points carries
    the reference's + 1e-5."""
    assert flow_gt.ndim == flow_pred.ndim == 4
    finite = ~np.isinf(flow_gt[:, [0]]) & ~np.isinf(flow_gt[:, [1]])
    moving = (np.abs(flow_gt[:, [0]]) > 0) & (np.abs(flow_gt[:, [1]]) > 0)
    total_mask = finite & moving
    if event_mask is not None:
        total_mask = np.logical_and(event_mask, total_mask)
    with np.errstate(invalid="ignore"):  # inf * False
        gt_masked = flow_gt * total_mask
    pred_masked = flow_pred * total_mask
    n_points = np.sum(total_mask, axis=(1, 2, 3)) + 1e-5
    errors = {}
    epe = np.linalg.norm(gt_masked - pred_masked, axis=1)
    errors["EPE"] = np.mean(np.sum(epe, axis=(1, 2)) / n_points)
    for k in (1, 2, 3, 5, 10, 20):
        errors[f"{k}PE"] = np.mean(np.sum(epe > k, axis=(1, 2)) / n_points)
    u, v = pred_masked[:, 0], pred_masked[:, 1]
    u_gt, v_gt = gt_masked[:, 0], gt_masked[:, 1]
    cosine = (1.0 + u * u_gt + v * v_gt) / (np.sqrt(1 + u * u + v * v) * np.sqrt(1 + u_gt * u_gt + v_gt * v_gt))
    errors["AE"] = np.mean(np.sum(np.arccos(cosine), axis=(1, 2)) / n_points)
    return errors
