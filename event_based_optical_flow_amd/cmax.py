"""Fused contrast-maximization objective: the hot path behind the reference's
`calculate_cost` (src/solver/patch_contrast_base.py:273-352).

`CMaxHandle` owns a `cmax_handle_t`: the batch is packed and sorted once (`set_events`), then every
objective evaluation runs warp+vote -> contrast -> gather-gradient on the GPU without
materialising warped events.  `ContrastObjective` exposes it as a differentiable callable
`loss = objective(motion)` for `scipy_autograd.minimize` / `torch.autograd.grad`.
"""
import copy
import ctypes
import logging
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from . import functional as F
from ._lib import CmaxIwes, CmaxObjective, check
from .array_types import to_device_tensor
from .costs.hybrid import combine

logger = logging.getLogger(__name__)

_COST_TABLE = {
    # name: (cost code, normalized, [(direction, multiplier), ...])  -- which IWEs get_arg_for_cost builds
    "image_variance": (_lib.COST_VARIANCE, 0, (("first", 1.0),)),
    "gradient_magnitude": (_lib.COST_GRADMAG, 0, (("first", 1.0),)),
    "normalized_image_variance": (_lib.COST_VARIANCE, 1, (("first", 1.0),)),
    "normalized_gradient_magnitude": (_lib.COST_GRADMAG, 1, (("first", 1.0),)),
    # forward = "last", backward = "first", middle x2 (multi_focal_*.py; patch_contrast_base.py:308-347)
    "multi_focal_normalized_image_variance": (_lib.COST_VARIANCE, 1, (("last", 1.0), ("first", 1.0), ("middle", 2.0))),
    "multi_focal_normalized_gradient_magnitude": (_lib.COST_GRADMAG, 1, (("last", 1.0), ("first", 1.0), ("middle", 2.0))),
}
FUSED_COSTS = tuple(_COST_TABLE)

# the focus losses (costs/focus.py, costs.focus_functions): fused like the gradient-magnitude trio, never routed to fused_iwes
_FOCUS_TABLE = {
    prefix + kind: (code, normalized, refs)
    for kind, code in (("mean_square", _lib.COST_MEAN_SQUARE), ("laplacian_magnitude", _lib.COST_LAPLACIAN),
                       ("hessian_magnitude", _lib.COST_HESSIAN))
    for prefix, normalized, refs in (("", 0, (("first", 1.0),)), ("normalized_", 1, (("first", 1.0),)),
                                     ("multi_focal_normalized_", 1, (("last", 1.0), ("first", 1.0), ("middle", 2.0))))
}
FOCUS_COSTS = tuple(_FOCUS_TABLE)


def _cost_registry():
    from . import costs  # (lazy: the costs package is imported after this module)

    return costs.functions


def make_descriptor(cost: str, motion_model: str, direction: str = "minimize", sigma: float = 0.0,
                    omit_boundary: bool = True, normalize_t: bool = True, time_bin: int = 0,
                    warp_direction: Union[str, float] = "first") -> CmaxObjective:
    """Build the cmax_objective_t for one named cost (include/cmax_hip.h)."""
    if cost not in _COST_TABLE and cost not in _FOCUS_TABLE:
        raise KeyError(f"cost {cost!r} has no fused kernel; fused costs: {FUSED_COSTS + FOCUS_COSTS}")
    if motion_model not in F.MODEL_CODES:
        raise KeyError(motion_model)
    if direction not in ("minimize", "maximize", "natural"):
        raise ValueError(f"direction should be minimize, maximize, and natural. Got {direction}.")
    code, normalized, refs = _COST_TABLE[cost] if cost in _COST_TABLE else _FOCUS_TABLE[cost]
    d = CmaxObjective()
    d.model = F.MODEL_CODES[motion_model]
    d.cost = code
    d.normalized = normalized
    d.minimize = int(direction == "minimize")
    # multi_focal_* return -loss for "maximize" (they sum iwe/orig ratios first)
    d.negate = int(len(refs) > 1 and direction == "maximize")
    d.omit_boundary = int(bool(omit_boundary))
    d.normalize_t = int(bool(normalize_t))
    d.n_ref = len(refs)
    for k, (ref_dir, mult) in enumerate(refs):
        if len(refs) == 1:
            ref_dir = warp_direction
        mode, frac = F.direction_to_ref(ref_dir)
        d.ref_mode[k] = mode
        d.ref_frac[k] = frac
        d.mult[k] = mult
    d.sigma = float(sigma)
    d.T = int(time_bin)
    return d


def prepare_event_weights(weights, n: int) -> torch.Tensor:
    """Per-event weights as the library takes them: [n] fp32 / fp64 on the device.  Shape and finiteness are checked where the data
    lives (host arrays on the host, before anything is copied); moving host data to the device needs one (require_gpu)."""
    if isinstance(weights, np.ndarray):
        w = torch.from_numpy(np.ascontiguousarray(weights))
    elif isinstance(weights, torch.Tensor):
        w = weights
    else:
        raise TypeError(f"weights must be a numpy array or a torch tensor, got {type(weights)}")
    if w.dim() != 1 or w.shape[0] != int(n):
        raise ValueError(f"weights must be [n] = [{int(n)}] (one per event, in the events' order), got {tuple(w.shape)}")
    if w.dtype not in (torch.float32, torch.float64):
        w = w.to(torch.float64)
    if w.numel() and not bool(torch.isfinite(w).all()):
        raise ValueError("weights must be finite (any sign, zero allowed)")
    return to_device_tensor(w, "weights").contiguous()


def ref_fractions(desc: CmaxObjective):
    """The reference times of an objective as fractions d_k of the batch period (first 0, last 1)."""
    return [0.0 if desc.ref_mode[k] == _lib.REF_FIRST else 1.0 if desc.ref_mode[k] == _lib.REF_LAST else float(desc.ref_frac[k])
            for k in range(desc.n_ref)]


def compose_events_grad(grad_events: torch.Tensor, csum: torch.Tensor, t: torch.Tensor, fractions: Sequence[float], normalize_t: bool,
                        t_range: Optional[Tuple[float, float]] = None) -> torch.Tensor:
    """The reference's `events.grad` [n, 4] in fp64 from what cmax_objective_event_grad returns (plain torch, any device):
    grad_events [n, 3] = (dL/dx, dL/dy, C_e = sum_k dL/d dt_{e,k}), csum[k] = sum_e dL/d dt_{e,k}, t = the batch's times, fractions =
    the objective's reference times d_k.  The x and y columns pass through and the polarity column is 0.  The time column is
    C_e * d dt/d t_e plus what autograd routes through t.min() and t.max() (src/warp.py:201-259, t_ref = t_min + d (t_max - t_min)):
        normalize_t:  dt = (t - t_ref) / P, P = t_max - t_min:  d dt/d t_e = 1 / P,  d dt/d t_min = (tau_e - 1) / P,  d dt/d t_max = -tau_e / P
                      with tau = (t - t_min) / P -- the same for every reference time, so C_e is enough;
        otherwise:    dt = t - t_ref:  d dt/d t_e = 1,  d dt/d t_min = -(1 - d_k),  d dt/d t_max = -d_k -- csum supplies the sums.
    Ties at the minimum / maximum share the routed term evenly (torch.Tensor.min / max).  t_range: the (t_min, t_max) handed to
    set_events for a time slice -- constants, nothing is routed.  Events with a non-finite time were not packed and take no part."""
    ge = grad_events.detach().to(torch.float64)
    t = t.detach().to(device=ge.device, dtype=torch.float64)
    n = ge.shape[0]
    out = torch.zeros((n, 4), dtype=torch.float64, device=ge.device)
    if n == 0:
        return out
    out[:, 0:2] = ge[:, 0:2]
    C = ge[:, 2]
    finite = torch.isfinite(t)
    if not bool(finite.any()):
        return out
    if t_range is None:
        lo, hi = t[finite].min(), t[finite].max()
    else:
        lo, hi = (torch.as_tensor(v, dtype=torch.float64, device=ge.device) for v in t_range)
    period = hi - lo
    if normalize_t:
        out[:, 2] = C / period
        tau = torch.where(finite, (t - lo) / period, torch.zeros_like(t))
        g_lo, g_hi = (C * (tau - 1.0)).sum() / period, -(C * tau).sum() / period
    else:
        out[:, 2] = C
        d = torch.as_tensor(list(fractions), dtype=torch.float64, device=ge.device)
        ck = csum.detach().to(device=ge.device, dtype=torch.float64)[: d.shape[0]]
        g_lo, g_hi = -((1.0 - d) * ck).sum(), -(d * ck).sum()
    if t_range is None:
        at_lo, at_hi = finite & (t == lo), finite & (t == hi)
        out[:, 2] += at_lo.to(torch.float64) * (g_lo / at_lo.sum()) + at_hi.to(torch.float64) * (g_hi / at_hi.sum())
    return out


def _with_motion_dtype(desc: CmaxObjective, want: int) -> CmaxObjective:
    """`desc` itself when its motion_dtype is `want`, otherwise a copy that says so (the caller's descriptor is never written)."""
    if desc.motion_dtype == want:
        return desc
    desc = CmaxObjective.from_buffer_copy(desc)
    desc.motion_dtype = want
    return desc


def _unit_tangent(tangent, shape=None):
    """(tangent / max|tangent| as contiguous fp32, max|tangent| as a 0-dim fp64 tensor): the derivative votes are fixed point, so a
    tangent crosses in unit max-norm and the caller scales the result back.  (None, 0) for a zero or empty tangent."""
    u = to_device_tensor(tangent, "tangent").detach().to(torch.float64)
    if shape is not None:
        u = u.reshape(shape)
    umax = u.abs().max() if u.numel() else torch.zeros((), dtype=torch.float64)
    if float(umax) == 0.0:
        return None, umax
    return (u / umax).to(torch.float32).contiguous(), umax


def _ptr(a):
    """Address of a device tensor or a host array as ctypes takes it; None stays None."""
    return None if a is None else a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data


class CMaxHandle:
    """One GPU workspace for one event batch (cmax_create / cmax_set_events / cmax_objective)."""

    def __init__(self, image_size: Tuple[int, int], outer_padding: Union[int, Tuple[int, int]] = 0):
        _lib.require_gpu()
        self._lib = _lib.load()
        if isinstance(outer_padding, (int, float)):
            outer_padding = (int(outer_padding), int(outer_padding))
        self.image_size = (int(image_size[0]), int(image_size[1]))
        self.outer_padding = (int(outer_padding[0]), int(outer_padding[1]))
        self.padded_size = (self.image_size[0] + 2 * self.outer_padding[0], self.image_size[1] + 2 * self.outer_padding[1])
        self._h = ctypes.c_void_p()
        check(self._lib.cmax_create(self.image_size[0], self.image_size[1], self.outer_padding[0], self.outer_padding[1],
                                    ctypes.byref(self._h)))
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.time_bin = 0
        self.time_slabs = 0  # cmax_set_time_slabs order of the current batch (0: none); reset by set_events / set_time_bins

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            if getattr(self, "_comm_init_thread", None) is not None and self._comm_init_pending():
                return  # deliberately leaked: a timed-out cmax_comm_init still holds the native handle (comm_init)
            self._lib.cmax_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------------------------------
    finds_time_extremes = True  # set_events(ev, None, None, ...) reduces t_min / t_max on the device

    def set_keep_outside(self, on: bool = True):
        """Finite events whose source pixel lies OFF the sensor (cmax_set_keep_outside; takes effect with the next set_events).
        True -- THE DEFAULT since round 5 -- keeps them: the reference's 2-DoF warp has no bounds test on the source and lets such an
        event vote wherever it warps into the padded image (src/warp.py:506-515); a dense / voxel objective (a flow has no value off
        the sensor; the reference's gather indexes out of bounds there, src/warp.py:303-307) and the patch search then REFUSE the
        batch.  False drops them while packing (counted: batch_info()["dropped"], on_dropped) -- what a caller of a dense objective
        asks for explicitly; the pyramid solver does, with on_dropped="raise"."""
        check(self._lib.cmax_set_keep_outside(self._h, int(bool(on))))
        return self

    def set_events(self, events, tmin: Optional[float] = None, tmax: Optional[float] = None, time_bin: int = 0,
                   on_dropped: str = "warn", weights=None):
        """Pack + sort one [n,4] batch (numpy or tensor, fp32/fp64).  (tmin, tmax): global batch
        extremes when this handle only holds a time slice of the batch (multi-GPU).
        on_dropped: what to do when events were NOT packed because their source pixel lies off the sensor (or is NaN) or their time
        is not finite --
        the fused path indexes source tiles and the flow field with it; the reference's 2-DoF warp would still let such an
        event vote if it warps into a padded image, its dense warp indexes out of bounds there -- "warn" (log),
        "raise" (a solver that must not diverge from the reference silently: ValueError) or "ignore".
        weights: optional [n] per-event weights (set_event_weights) -- the reference's `weight` of bilinear_vote_*."""
        if on_dropped not in ("warn", "raise", "ignore"):
            raise ValueError(f"on_dropped should be warn, raise or ignore. Got {on_dropped}.")
        ev = to_device_tensor(events, "events")
        if ev.dim() != 2 or ev.shape[1] != 4:
            raise ValueError(f"events must be [n, 4], got {tuple(ev.shape)}")
        ev = ev.contiguous()
        w = prepare_event_weights(weights, ev.shape[0]) if weights is not None else None
        have = tmin is not None and tmax is not None
        check(self._lib.cmax_set_events(self._h, ev.data_ptr(), F._code(ev), ev.shape[0], int(have),
                                        float(tmin) if have else 0.0, float(tmax) if have else 0.0, int(time_bin),
                                        F._stream()))
        self.time_bin = int(time_bin)
        self.time_slabs = 0
        self._batch_id = getattr(self, "_batch_id", 0) + 1  # fused_iwes: a backward pass refuses a handle that holds another batch
        self._n_in = int(ev.shape[0])
        self._batch_t = ev[:, 2]  # a view, no copy: events_grad routes dL/dt through t.min() / t.max() with the batch's own times
        self._batch_t_range = (float(tmin), float(tmax)) if have else None
        if w is not None:
            check(self._lib.cmax_set_event_weights(self._h, w.data_ptr(), F._code(w), w.shape[0], F._stream()))
        info = self.batch_info() if on_dropped != "ignore" else {"dropped": 0, "outside": 0}
        dropped = info["dropped"]
        if info["outside"]:
            # said HERE, at the batch, not at the first dense evaluation behind the sort: keeping off-sensor events is the
            # default since round 5 and only the 2-DoF model is defined for them
            msg = (f"cmax_set_events kept {info['outside']} of {ev.shape[0]} events whose source pixel lies off the "
                   f"{self.image_size[0]} x {self.image_size[1]} sensor (the reference's 2-DoF warp has no bounds test, src/warp.py:506-515); "
                   "dense / voxel objectives and the patch search refuse such a batch -- set_keep_outside(False) before set_events drops them")
            if on_dropped == "raise":
                raise ValueError(msg)
            logger.warning(msg)
        if dropped and on_dropped == "raise":
            raise ValueError(f"cmax_set_events dropped {dropped} of {ev.shape[0]} events whose source pixel is outside the "
                             f"{self.image_size[0]} x {self.image_size[1]} sensor (or NaN) or whose time is not finite; use the leaf operators (Warp + "
                             "EventImageConverter) for such batches, set_keep_outside() for a 2-DoF objective, or crop / pad the sensor")
        if dropped:
            logger.warning(f"cmax_set_events dropped {dropped} of {ev.shape[0]} events: source pixel outside the "
                           f"{self.image_size[0]} x {self.image_size[1]} sensor (or NaN) or time not finite; the fused path cannot keep them")
        return self

    def set_event_weights(self, weights):
        """Per-event weights [n] of the CURRENT batch, in the order of the events handed to set_events (numpy or tensor, host or
        device; cmax_set_event_weights) -- the `weight` argument of the reference's bilinear_vote_* / create_image_from_events_*
        (src/event_image_converter.py:316-372).  None clears them.  evaluate / prepare / evaluate_host / evaluate_batch / iwe /
        last_iwe and ContrastObjective then work on the weighted image; hvp, the raw and phase-split forms, evaluate_dist, comm_init,
        patch plans, patch_search and deterministic mode raise NotImplementedError with the library's text.  The next set_events
        starts unweighted; set_time_bins / set_time_slabs keep the weights."""
        if weights is None:
            check(self._lib.cmax_set_event_weights(self._h, None, 0, 0, F._stream()))
            return self
        w = prepare_event_weights(weights, getattr(self, "_n_in", 0))
        check(self._lib.cmax_set_event_weights(self._h, w.data_ptr(), F._code(w), w.shape[0], F._stream()))
        return self

    def _batch_weighted(self):
        flag, wmax = ctypes.c_int(0), ctypes.c_double(0.0)
        check(self._lib.cmax_batch_weighted(self._h, ctypes.byref(flag), ctypes.byref(wmax)))
        return bool(flag.value), wmax.value

    @property
    def weighted(self) -> bool:
        """Whether the current batch carries per-event weights."""
        return self._batch_weighted()[0]

    @property
    def weight_max(self) -> float:
        """max |w| over the packed events of a weighted batch (the normalisation of the fixed-point votes); 0.0 when unweighted."""
        return self._batch_weighted()[1]

    def batch_info(self) -> Dict[str, int]:
        """{"packed", "dropped", "fractional", "owned_groups", "outside"} of the last set_events (cmax_batch_info, cmax_batch_outside)."""
        n, d = ctypes.c_int64(0), ctypes.c_int64(0)
        f, o = ctypes.c_int(0), ctypes.c_int(0)
        check(self._lib.cmax_batch_info(self._h, ctypes.byref(n), ctypes.byref(d), ctypes.byref(f), ctypes.byref(o)))
        out = ctypes.c_int64(0)
        check(self._lib.cmax_batch_outside(self._h, ctypes.byref(out)))
        return {"packed": n.value, "dropped": d.value, "fractional": bool(f.value), "owned_groups": bool(o.value), "outside": out.value}

    def packed_events(self):
        """(packed [n, 2] int64 on the host: word 0 = row | col << 12 | top byte << 24, word 1 = bits of the fp32 normalised time;
        group starts [n_groups + 1]) of the current batch in its sorted order (cmax_debug_packed_events) -- for tests of the order."""
        n = self.n_events
        ev = torch.empty((max(n, 1), 2), dtype=torch.int32, device=self.device)
        ng = ctypes.c_int(0)
        tiles = ((self.image_size[0] + 15) // 16) * ((self.image_size[1] + 15) // 16)
        gs = torch.empty(tiles * 256 + 1, dtype=torch.int32, device=self.device)
        check(self._lib.cmax_debug_packed_events(self._h, ev.data_ptr(), gs.data_ptr(), ctypes.byref(ng), F._stream()))
        return (ev[:n].cpu().numpy().astype(np.int64) & 0xFFFFFFFF), gs[: ng.value + 1].cpu().numpy()

    WORK_LIST_FLAGS = ("big", "mid", "owned", "small_accumulators", "slab_major", "compact", "long_runs")  # CMAX_WL_*, bit 0 first
    COMPACT_STRIDE = 4 * 4096 + 4096 // 2 + 64  # bytes per compact region (b512::kCompactStride)

    def work_list(self):
        """(segments [n_segments, 4] int64 on the host: first event, count, first group, number of groups; flags {name: bool} over
        WORK_LIST_FLAGS; seg_max) of the current work list as the handle holds it after the last cut (cmax_debug_work_list) -- for tests
        of the cut."""
        n, f, m = ctypes.c_int(0), ctypes.c_uint(0), ctypes.c_int(0)
        check(self._lib.cmax_debug_work_list(self._h, None, ctypes.byref(n), ctypes.byref(f), ctypes.byref(m), F._stream()))
        segs = torch.zeros((max(n.value, 1), 4), dtype=torch.int32, device=self.device)
        check(self._lib.cmax_debug_work_list(self._h, segs.data_ptr(), None, None, None, F._stream()))
        flags = {name: bool(f.value >> k & 1) for k, name in enumerate(self.WORK_LIST_FLAGS)}
        return segs[: n.value].cpu().numpy().astype(np.int64), flags, m.value

    def compact_events(self):
        """(regions [n_segments, COMPACT_STRIDE] uint8 on the host, flag) -- the compact copy of the current work list's events and the
        flag its packing kernel raises when an event does not fit its segment's strip (cmax_debug_compact_events); the library's
        CMAX_ESTATE (RuntimeError) on a handle without a compact copy."""
        n = ctypes.c_int(0)
        check(self._lib.cmax_debug_work_list(self._h, None, ctypes.byref(n), None, None, F._stream()))
        reg = torch.zeros((max(n.value, 1), self.COMPACT_STRIDE), dtype=torch.uint8, device=self.device)
        bad = ctypes.c_int(0)
        check(self._lib.cmax_debug_compact_events(self._h, reg.data_ptr(), ctypes.byref(bad), F._stream()))
        return reg[: n.value].cpu().numpy(), bad.value

    def work_list_info(self) -> Dict[str, int]:
        """{"segments", "segment_events", "small_accumulators"} of the work list the last set_events / set_time_bins cut
        (cmax_work_list_info): one workgroup of the event kernels per segment; segment_events is 2040, 3064 (mid) or 4088 (big segments)."""
        n, e, a = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        check(self._lib.cmax_work_list_info(self._h, ctypes.byref(n), ctypes.byref(e), ctypes.byref(a)))
        return {"segments": n.value, "segment_events": e.value, "small_accumulators": bool(a.value)}

    def set_time_bins(self, time_bin: int):
        check(self._lib.cmax_set_time_bins(self._h, int(time_bin), F._stream()))
        self.time_bin = int(time_bin)
        self.time_slabs = 0

    def set_time_slabs(self, n_slab: int):
        """Large motions of a 2-DoF / dense objective: order the batch in `n_slab` time slabs (cmax_set_time_slabs); <= 1 undoes it."""
        check(self._lib.cmax_set_time_slabs(self._h, int(n_slab), F._stream()))
        self.time_bin = 0
        self.time_slabs = int(n_slab) if n_slab > 1 else 0
        return self

    def auto_time_slabs(self, displacement_px: float) -> int:
        """Put the batch into the slab order `suggest_time_slabs(displacement_px)` asks for -- with hysteresis, so that an optimiser whose
        motion hovers around a threshold does not re-sort the batch every iteration: more slabs as soon as the displacement asks for
        them (an un-slabbed 150-px evaluation costs 4x a slabbed one), fewer only once it has fallen to 0.6 of the threshold that
        would keep the current count.  What the solver classes call before every evaluation (the motion is theirs, on the host; the
        library never reads a motion back).  Binned (voxel) handles are left alone.  Returns the slab count in force."""
        if self.time_bin > 0:
            return 0
        want = self.suggest_time_slabs(displacement_px)
        cur = max(self.time_slabs, 1)
        if want > cur or (want < cur and self.suggest_time_slabs(displacement_px / 0.6) < cur):
            self.set_time_slabs(want)
        return self.time_slabs

    def suggest_time_slabs(self, displacement_px: float) -> int:
        """Slab count for a motion of up to `displacement_px` over the batch (profiles/r04_large_motion.txt: 1M events @346x260 --
        none below ~25 px, 2 up to ~45 px, 4 beyond), capped so that a (tile, slab) group keeps >= ~600 events: smaller groups make
        segments of three groups too short to pay for a workgroup."""
        want = 1 if displacement_px < 25 else (2 if displacement_px < 45 else 4)
        tiles = ((self.image_size[0] + 15) // 16) * ((self.image_size[1] + 15) // 16)
        while want > 1 and self.n_events < 600 * tiles * want:
            want //= 2
        return want

    @property
    def n_events(self) -> int:
        n = ctypes.c_int64()
        check(self._lib.cmax_handle_info(self._h, ctypes.byref(n), None))
        return n.value

    def launch_floor_us(self, pairs: int = 200) -> float:
        """Microseconds per pair of dependent EMPTY launches with the grids of K1 and K3 on the current batch (cmax_debug_launch_floor),
        bracketed by events on the current stream: the floor of the headline evaluation's launch structure, measured in this run."""
        stream = F._stream()
        check(self._lib.cmax_debug_launch_floor(self._h, 20, stream))  # warm-up
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        check(self._lib.cmax_debug_launch_floor(self._h, int(pairs), stream))
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3 / pairs

    @property
    def workspace_bytes(self) -> int:
        b = ctypes.c_int64()
        check(self._lib.cmax_handle_info(self._h, None, ctypes.byref(b)))
        return b.value

    def _motion32(self, motion) -> torch.Tensor:
        return to_device_tensor(motion, "motion").detach().to(torch.float32).contiguous()

    def _motion_arg(self, desc: CmaxObjective, motion, exact_flow: bool = False):
        """(device tensor, descriptor) for one objective call.  A 2-DoF theta that arrives in fp64 -- the dtype the
        reference's solver optimises in (src/solver/patch_contrast_pyramid.py:186) -- is handed over as it is
        (cmax_objective_t::motion_dtype = CMAX_F64): the kernels round it to fp32 for the bulk arithmetic and keep the
        doubles for the events that lie on a cell border.  So is an fp64 flow / voxel with `exact_flow=True` (the keyword of
        every method that takes a motion): the library splits it into (float)flow, which all the arithmetic reads, and the
        remainder, which only those border events read.  Everything else is fp32 on the device."""
        m = to_device_tensor(motion, "motion").detach()
        want = _lib.F64 if (m.dtype == torch.float64 and (desc.model == _lib.MODEL_2DOF or exact_flow)) else _lib.F32
        m = m.contiguous() if want == _lib.F64 else m.to(torch.float32).contiguous()
        return m, _with_motion_dtype(desc, want)

    def _grad_out(self, desc, m, host: bool = False):
        """An uninitialised buffer of the motion gradient's form (also a Hessian-vector product's): float64 [2] for the 2-DoF model,
        else float32 of the motion's shape; `desc`: a CmaxObjective or a CmaxIwes; a device tensor, or a numpy array with `host`."""
        two_dof = desc.model == _lib.MODEL_2DOF
        if host:
            return np.empty(2, dtype=np.float64) if two_dof else np.empty(tuple(m.shape), dtype=np.float32)
        if two_dof:
            return torch.empty(2, dtype=torch.float64, device=self.device)
        return torch.empty(tuple(m.shape), dtype=torch.float32, device=self.device)

    def _outputs(self, desc, m, want_grad: bool = True, host: bool = False):
        """(result double[8], grad or None): the outputs of one objective call, on the device or (host) as numpy arrays."""
        result = np.empty(8, dtype=np.float64) if host else torch.empty(8, dtype=torch.float64, device=self.device)
        return result, (self._grad_out(desc, m, host) if want_grad else None)

    def _per_event_out(self, cols: Tuple[int, ...] = (), want: bool = True):
        """(n, buffer): float32 [max(n, 1), *cols] on the device for one entry per event handed to set_events (None unless `want`);
        callers return buffer[:n] (an empty batch still hands over a valid pointer: a tensor without elements has none)."""
        n = int(getattr(self, "_n_in", 0))
        return n, (torch.empty((max(n, 1),) + cols, dtype=torch.float32, device=self.device) if want else None)

    def _prepared(self, fn, desc, m, outs, k: Optional[int] = None):
        """A prepared call `fn(handle, desc, motion[, k], *outs, stream)`: function and pointers resolved once; `call()` enqueues it on
        the current stream.  call.keepalive holds what the pointers point into, call.motion is the tensor the call reads."""
        args = (self._h, ctypes.byref(desc), m.data_ptr()) + (() if k is None else (k,)) + tuple(_ptr(o) for o in outs)
        stream = F._stream

        def call():
            rc = fn(*args, stream())
            if rc:
                check(rc)

        call.keepalive = (m, desc) + tuple(outs)
        call.motion = m
        return call

    def iwe(self, motion, motion_model: Optional[str], direction: Union[str, float] = "first",
            normalize_t: bool = True, sigma: float = 0.0) -> torch.Tensor:
        """Image of warped events, fp32 [Hp, Wp].  motion_model None -> un-warped image (orig_iwe)."""
        out = torch.empty(self.padded_size, dtype=torch.float32, device=self.device)
        if motion_model is None:
            model, mptr, T = -1, None, 0
        else:
            m = self._motion32(motion)
            model, mptr = F.MODEL_CODES[motion_model], m.data_ptr()
            T = int(m.shape[0]) if model == _lib.MODEL_VOXEL else 0
        mode, frac = F.direction_to_ref(direction)
        check(self._lib.cmax_iwe(self._h, model, mptr, T, mode, frac, int(bool(normalize_t)), float(sigma),
                                 out.data_ptr(), F._stream()))
        return out

    def evaluate(self, desc: CmaxObjective, motion, want_grad: bool = True, exact_flow: bool = False):
        """One cmax_objective call.  Returns (result double[8] on device, grad or None).
        result[0] = loss, result[1..n_ref] = raw contrasts, result[5] = contrast of orig_iwe."""
        m, desc = self._motion_arg(desc, motion, exact_flow)
        result, grad = self._outputs(desc, m, want_grad)
        check(self._lib.cmax_objective(self._h, ctypes.byref(desc), m.data_ptr(), result.data_ptr(),
                                       grad.data_ptr() if grad is not None else None, F._stream()))
        return result, grad

    def evaluate_weight_grad(self, desc: CmaxObjective, motion, want_grad: bool = True, exact_flow: bool = False):
        """One cmax_objective_weight_grad call: (result, grad or None, grad_w).  result and grad as `evaluate` returns them;
        grad_w is dL/dw, float32 [n] on the device in the order of the events handed to set_events -- the reference's `weight.grad`
        after `backward()` through create_image_from_events_*(weight=w) (src/event_image_converter.py:316-372).  It is not multiplied
        by w (an event of weight 0 has a derivative), an unweighted handle means w = 1, and events that were not packed get 0.
        Deterministic handles and handles with a communicator raise NotImplementedError with the library's text."""
        m, desc = self._motion_arg(desc, motion, exact_flow)
        result, grad = self._outputs(desc, m, want_grad)
        n, buf = self._per_event_out()
        check(self._lib.cmax_objective_weight_grad(self._h, ctypes.byref(desc), m.data_ptr(), result.data_ptr(),
                                                   grad.data_ptr() if grad is not None else None, buf.data_ptr(), n, F._stream()))
        return result, grad, buf[:n]

    def evaluate_event_grad(self, desc: CmaxObjective, motion, want_grad: bool = True, exact_flow: bool = False):
        """One cmax_objective_event_grad call: (result, grad or None, grad_events, csum).  result and grad as `evaluate` returns them;
        grad_events is float32 [n, 3] on the device in the order of the events handed to set_events: (dL/dx, dL/dy, C = sum_k dL/d dt_k),
        dt_k the event's time offset as the warp uses it -- the first two are the reference's `events.grad[:, :2]`
        (`self.events = ...requires_grad_()`, src/solver/patch_contrast_mixed.py:166), the third is what `events_grad` turns into its
        time column; csum is float64 [4]: sum_e dL/d dt_{e,k} per reference time.  An unweighted handle means w = 1, events that were not
        packed keep a row of zeros.  Deterministic handles and handles with a communicator raise NotImplementedError with the
        library's text."""
        m, desc = self._motion_arg(desc, motion, exact_flow)
        result, grad = self._outputs(desc, m, want_grad)
        n, buf = self._per_event_out((3,))
        csum = torch.empty(4, dtype=torch.float64, device=self.device)
        check(self._lib.cmax_objective_event_grad(self._h, ctypes.byref(desc), m.data_ptr(), result.data_ptr(),
                                                  grad.data_ptr() if grad is not None else None, buf.data_ptr(), n, csum.data_ptr(), F._stream()))
        return result, grad, buf[:n], csum

    def events_grad(self, desc: CmaxObjective, motion, exact_flow: bool = False) -> torch.Tensor:
        """The reference's `events.grad`, float64 [n, 4] on the device: evaluate_event_grad composed with the batch's times
        (compose_events_grad; not a hot path).  The handle keeps a VIEW of the time column handed to set_events: the batch must not
        have been modified in place since."""
        _, _, ge, csum = self.evaluate_event_grad(desc, motion, want_grad=False, exact_flow=exact_flow)
        return compose_events_grad(ge, csum, self._batch_t, ref_fractions(desc), bool(desc.normalize_t), self._batch_t_range)

    def prepare(self, desc: CmaxObjective, motion, want_grad: bool = True, dist: bool = False, exact_flow: bool = False):
        """A prepared cmax_objective (dist: cmax_objective_dist) call for an inner loop that evaluates the SAME motion
        buffer again and again (an optimiser updating it in place, a benchmark): outputs allocated once, pointers
        resolved once.  Returns (call, result, grad); `call()` enqueues one evaluation on the current stream and
        overwrites result / grad.  The call reads `call.motion`: that IS `motion` when it is already a contiguous device
        tensor of the dtype the kernels take (fp32; fp64 for a 2-DoF theta) -- otherwise it is a private converted copy, and an
        optimiser that updates its own tensor in place must write into `call.motion` instead (call.motion_is_callers tells).  `evaluate` spends ~6 us per call in Python (two allocations, tensor checks) -- as
        much as the three launches of a 1M-event 2-DoF evaluation leave the host to spare (profiles/r02_ablation.txt)."""
        m, desc = self._motion_arg(desc, motion, exact_flow)
        result, grad = self._outputs(desc, m, want_grad)
        call = self._prepared(self._lib.cmax_objective_dist if dist else self._lib.cmax_objective, desc, m, (result, grad))
        call.motion_is_callers = isinstance(motion, torch.Tensor) and motion.is_cuda and motion.data_ptr() == m.data_ptr()
        return call, result, grad

    # -- results on the host / raw sums (no finishing kernel) ---------------------------------------------------
    def evaluate_host(self, desc: CmaxObjective, motion, want_grad: bool = True, exact_flow: bool = False):
        """One cmax_objective_host call: the evaluation with its results delivered to the host, the way an optimiser
        consumes them (the reference's wrapper ends in .cpu().numpy()).  Returns (result float64[8], grad ndarray or None);
        blocks.  For the 2-DoF image-variance objective the finishing kernel writes into pinned host memory and the call polls a
        run counter behind the results: no copy engine, no driver call on the way back."""
        m, desc = self._motion_arg(desc, motion, exact_flow)
        result, grad = self._outputs(desc, m, want_grad, host=True)
        check(self._lib.cmax_objective_host(self._h, ctypes.byref(desc), m.data_ptr(), result.ctypes.data,
                                            grad.ctypes.data if grad is not None else None, F._stream()))
        return result, grad

    def prepare_host(self, desc: CmaxObjective, motion, want_grad: bool = True, exact_flow: bool = False):
        """Prepared cmax_objective_host call: (call, result, grad) with `result` / `grad` numpy arrays that every `call()`
        overwrites (it returns when they are filled)."""
        m, desc = self._motion_arg(desc, motion, exact_flow)
        result, grad = self._outputs(desc, m, want_grad, host=True)
        return self._prepared(self._lib.cmax_objective_host, desc, m, (result, grad)), result, grad

    def descend(self, desc: CmaxObjective, theta0, descent: "_lib.CmaxDescent", trace: bool = False) -> "_lib.DescentResult":
        """One cmax_objective_descend call: descent.n_iter iterations of SGD / Adam on a 2-DoF objective (the reference's run_torch,
        src/solver/base.py:840-881), theta and the optimiser's state resident in device memory, one wait at the end.  theta0: two
        numbers (host); `descent`: _lib.descent_descriptor(...).  Blocks; returns a _lib.DescentResult of host arrays."""
        theta0 = np.ascontiguousarray(np.asarray(theta0.detach().cpu() if isinstance(theta0, torch.Tensor) else theta0, dtype=np.float64).reshape(-1))
        if theta0.size != 2:
            raise ValueError(f"theta0 has {theta0.size} elements, a 2-DoF descent needs 2")
        desc = _with_motion_dtype(desc, _lib.F64)  # the iterate is fp64 in device memory
        fn, h, dref, stream = self._lib.cmax_objective_descend, self._h, ctypes.byref(desc), F._stream()
        with torch.cuda.device(self.device):
            return _lib.run_descent(lambda o, res, xl, xb, hist, tr: fn(h, dref, theta0.ctypes.data, o, res, xl, xb, hist, tr, stream), 2, descent, trace)

    def minimize_lbfgs(self, desc: CmaxObjective, theta0, lbfgs: "_lib.CmaxLbfgs", trace: bool = False) -> "_lib.LbfgsResult":
        """One cmax_objective_lbfgs call: lbfgs.n_eval evaluations of a device-resident L-BFGS with a backtracking line search on a 2-DoF
        objective (the rules: include/cmax_hip.h), theta and the optimiser's state resident in device memory.  theta0: two numbers
        (host, pixel over the batch); `lbfgs`: _lib.lbfgs_descriptor(...).  theta stays within lbfgs.max_move of theta0, so the batch's
        time slabs are decided here, ONCE, from max|theta0| + max_move (auto_time_slabs).  Blocks; returns a _lib.LbfgsResult of host arrays."""
        theta0 = np.ascontiguousarray(np.asarray(theta0.detach().cpu() if isinstance(theta0, torch.Tensor) else theta0, dtype=np.float64).reshape(-1))
        if theta0.size != 2:
            raise ValueError(f"theta0 has {theta0.size} elements, a 2-DoF solve needs 2")
        if np.isfinite(theta0).all() and np.isfinite(lbfgs.max_move):
            self.auto_time_slabs(float(np.abs(theta0).max()) + abs(float(lbfgs.max_move)))
        desc = _with_motion_dtype(desc, _lib.F64)  # the iterate is fp64 in device memory
        fn, h, dref, stream = self._lib.cmax_objective_lbfgs, self._h, ctypes.byref(desc), F._stream()
        with torch.cuda.device(self.device):
            return _lib.run_lbfgs(lambda o, res, x, hist, al, code, tr: fn(h, dref, theta0.ctypes.data, o, res, x, hist, al, code, tr, stream), 2, lbfgs, trace)

    def descend_batch(self, desc: CmaxObjective, theta0s, descent: "_lib.CmaxDescent", trace: bool = False) -> list:
        """K independent trajectories of `descend` from the starts `theta0s` [K, 2] (host): cmax_objective_descend_batch, at most
        _lib.DESCENT_MAX_STARTS = 64 starts per call (more are cut into several calls).  For the plain variance without a blur on an
        unweighted default handle the K candidates share the launches of one, every iteration; everything else runs start by start
        inside the call.  Blocks; returns a list of K _lib.DescentResult."""
        theta0s = np.ascontiguousarray(np.asarray(theta0s.detach().cpu() if isinstance(theta0s, torch.Tensor) else theta0s, dtype=np.float64))
        if theta0s.ndim != 2 or theta0s.shape[1] != 2:
            raise ValueError(f"theta0s has shape {tuple(theta0s.shape)}, the starts of a 2-DoF descent are [K, 2]")
        desc = _with_motion_dtype(desc, _lib.F64)  # the iterates are fp64 in device memory
        fn, h, dref, stream = self._lib.cmax_objective_descend_batch, self._h, ctypes.byref(desc), F._stream()
        out = []
        with torch.cuda.device(self.device):
            for b in range(0, theta0s.shape[0], _lib.DESCENT_MAX_STARTS):
                part = np.ascontiguousarray(theta0s[b:b + _lib.DESCENT_MAX_STARTS])
                k = int(part.shape[0])
                out += _lib.run_descent_batch(lambda o, res, xl, xb, hist, tr: fn(h, dref, part.ctypes.data, k, o, res, xl, xb, hist, tr, stream), k, 2, descent, trace)
        return out

    def has_raw(self, desc: CmaxObjective) -> bool:
        """Whether `desc` on the current batch has a raw form (cmax_objective_has_raw): every 2-DoF objective in the default
        (non-deterministic) mode on a non-empty batch, except a normalised plain variance."""
        return bool(self._lib.cmax_objective_has_raw(self._h, ctypes.byref(desc)))

    def prepare_raw(self, desc: CmaxObjective, motion):
        """Prepared cmax_objective_raw call: (call, raw, finalize).  `call()` enqueues K1 + K3 of one evaluation, which leave
        their partial sums in `raw` (device float64 [n_ref, RAW_DOUBLES]); `finalize()` copies `raw` to the host and returns
        (result float64[8], grad float64[2]) = cmax_finalize_raw_host -- the consumer's share of the evaluation, a few
        hundred additions."""
        m, desc = self._motion_arg(desc, motion)
        if not self.has_raw(desc):
            if self.weighted:  # what cmax_objective_raw itself answers on a weighted handle (CMAX_EUNSUPPORTED)
                raise NotImplementedError("objective_raw: not built for a handle that holds per-event weights (cmax_set_event_weights); "
                                          "set_event_weights(None) clears them")
            raise _lib.CmaxError(-1, "this objective has no raw form (2-DoF, default mode, non-empty batch; not a normalised plain variance)")
        raw = torch.empty((desc.n_ref, _lib.RAW_DOUBLES), dtype=torch.float64, device=self.device)
        host = torch.empty((desc.n_ref, _lib.RAW_DOUBLES), dtype=torch.float64).pin_memory()
        call = self._prepared(self._lib.cmax_objective_raw, desc, m, (raw,))
        fin, h, dref = self._lib.cmax_finalize_raw_host, self._h, ctypes.byref(desc)

        def finalize():
            host.copy_(raw, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            result, grad = self._outputs(desc, m, host=True)
            check(fin(h, dref, host.data_ptr(), result.ctypes.data, grad.ctypes.data))
            return result, grad

        call.keepalive += (host,)
        return call, raw, finalize

    def prepare_batch(self, desc: CmaxObjective, motions, exact_flow: bool = False):
        """Prepared cmax_objective_batch call: (call, results, grads) for K candidate motions `motions` [K, ...] (2-DoF: [K, 2]; an
        fp64 theta crosses the ABI in fp64 like in `evaluate`, and so do fp64 flows with exact_flow=True).  results float64 [K, 8], grads float64 [K, 2] | float32 [K, ...].
        The reference's gradient-free paths evaluate batches of sampled motions (src/solver/base.py:738-758); for the 2-DoF
        image-variance objective the K evaluations share one launch of each kernel (blockIdx.z = candidate)."""
        mt = to_device_tensor(motions, "motions").detach()
        K = int(mt.shape[0])
        m, desc = self._motion_arg(desc, mt, exact_flow)
        results = torch.empty((K, 8), dtype=torch.float64, device=self.device)
        if desc.model == _lib.MODEL_2DOF:
            grads = torch.empty((K, 2), dtype=torch.float64, device=self.device)
        else:
            grads = torch.empty((K,) + tuple(m.shape[1:]), dtype=torch.float32, device=self.device)
        return self._prepared(self._lib.cmax_objective_batch, desc, m, (results, grads), k=K), results, grads

    def evaluate_batch(self, desc: CmaxObjective, motions, exact_flow: bool = False):
        """(results [K, 8], grads [K, ...]) of K candidate motions: one cmax_objective_batch call."""
        call, results, grads = self.prepare_batch(desc, motions, exact_flow)
        call()
        return results, grads

    def hvp(self, desc: CmaxObjective, motion, tangent, exact_flow: bool = False) -> torch.Tensor:
        """Exact Hessian-vector product H @ tangent of the objective w.r.t. the motion (cmax_objective_hvp):
        what torch.autograd.functional.vhp gives the reference's Newton-CG.  Returns fp64 [2] (2-DoF) or
        fp32 with the motion's shape.  The motion crosses in fp32 unless exact_flow=True, which keeps the dtype it is given (an
        fp64 flow / voxel or theta then decides the border cells, as in `evaluate`)."""
        if exact_flow:
            m, desc = self._motion_arg(desc, motion, True)
        else:
            m, desc = self._motion32(motion), _with_motion_dtype(desc, _lib.F32)
        un, umax = _unit_tangent(tangent)
        hv = self._grad_out(desc, m)
        if un is None:
            return hv.zero_()
        check(self._lib.cmax_objective_hvp(self._h, ctypes.byref(desc), m.data_ptr(), un.data_ptr(), hv.data_ptr(), F._stream()))
        return hv * umax.to(hv.dtype)

    # -- the image of warped events as a differentiable layer (cmax_iwes*, see fused_iwes) ---------------------------
    def _iwes_args(self, motion, motion_model: str, directions, sigma: float, normalize_t: bool, with_orig: bool, exact_flow: bool = False):
        if motion_model not in F.MODEL_CODES:
            raise KeyError(motion_model)
        directions = (directions,) if isinstance(directions, (str, int, float)) else tuple(directions)
        if not 1 <= len(directions) <= 4:
            raise ValueError(f"1 to 4 reference times, got {len(directions)}")
        m = to_device_tensor(motion, "motion").detach()
        f64 = bool(exact_flow) and m.dtype == torch.float64 and F.MODEL_CODES[motion_model] != _lib.MODEL_2DOF  # (see _motion_arg)
        m = m.contiguous() if f64 else m.to(torch.float32).contiguous()
        d = CmaxIwes()
        d.model = F.MODEL_CODES[motion_model]
        d.normalize_t = int(bool(normalize_t))
        d.n_ref = len(directions)
        for k, ref_dir in enumerate(directions):
            d.ref_mode[k], d.ref_frac[k] = F.direction_to_ref(ref_dir)
        d.sigma = float(sigma)
        d.T = int(m.shape[0]) if d.model == _lib.MODEL_VOXEL else 0
        d.motion_dtype = _lib.F64 if f64 else _lib.F32
        d.with_orig = int(bool(with_orig))
        return m, d

    def _iwes_planes(self, t, n_planes: int, what: str) -> torch.Tensor:
        t = to_device_tensor(t, what).detach().to(torch.float32).contiguous()
        if tuple(t.shape) != (n_planes,) + self.padded_size:
            raise ValueError(f"{what} must be [{n_planes}, {self.padded_size[0]}, {self.padded_size[1]}], got {tuple(t.shape)}")
        return t

    def iwes(self, motion, motion_model: str, directions=("first",), sigma: float = 0.0, normalize_t: bool = True,
             with_orig: bool = False, exact_flow: bool = False) -> torch.Tensor:
        """The images of warped events at every reference time in `directions` in one call (cmax_iwes): fp32 [K, Hp, Wp], K =
        len(directions) (+ 1 with_orig: the un-warped image last) -- image k is what `iwe(motion, motion_model, directions[k], ...)`
        returns, the weighted image on a weighted handle."""
        m, d = self._iwes_args(motion, motion_model, directions, sigma, normalize_t, with_orig, exact_flow)
        out = torch.empty((d.n_ref + d.with_orig,) + self.padded_size, dtype=torch.float32, device=self.device)
        check(self._lib.cmax_iwes(self._h, ctypes.byref(d), m.data_ptr(), out.data_ptr(), F._stream()))
        return out

    def iwes_vjp(self, motion, motion_model: str, gimages, directions=("first",), sigma: float = 0.0, normalize_t: bool = True,
                 with_orig: bool = False, want_grad_w: bool = False, exact_flow: bool = False):
        """(sum_k J_k^T gimages[k], grad_w or None) -- cmax_iwes_vjp: the motion gradient of <gimages, iwes(motion)> with the cells
        held fixed (fp64 [2] for 2-DoF, else fp32 with the motion's shape) and, on request, its derivative with respect to the
        per-event weights (fp32 [n] in the order of the events handed to set_events, not multiplied by w).  gimages: the shape of
        `iwes`' result, the caller's dL/dI.  The result is that of the handle's state (order, weights) at the time of THIS call."""
        m, d = self._iwes_args(motion, motion_model, directions, sigma, normalize_t, with_orig, exact_flow)
        g = self._iwes_planes(gimages, d.n_ref + d.with_orig, "gimages")
        grad = self._grad_out(d, m)
        n, buf = self._per_event_out(want=want_grad_w)
        check(self._lib.cmax_iwes_vjp(self._h, ctypes.byref(d), m.data_ptr(), g.data_ptr(), grad.data_ptr(),
                                      buf.data_ptr() if want_grad_w else None, n, F._stream()))
        return grad, (buf[:n] if want_grad_w else None)

    def iwes_jvp(self, motion, motion_model: str, tangent, directions=("first",), sigma: float = 0.0, normalize_t: bool = True,
                 with_orig: bool = False, exact_flow: bool = False) -> torch.Tensor:
        """J_k tangent per reference time, fp32 [len(directions), Hp, Wp] (cmax_iwes_jvp).  The tangent is brought to unit max-norm
        for the fixed-point derivative votes and the result scaled back, as `hvp` does."""
        m, d = self._iwes_args(motion, motion_model, directions, sigma, normalize_t, False, exact_flow)
        out = torch.zeros((d.n_ref,) + self.padded_size, dtype=torch.float32, device=self.device)
        un, umax = _unit_tangent(tangent, m.shape)
        if un is None:
            return out
        check(self._lib.cmax_iwes_jvp(self._h, ctypes.byref(d), m.data_ptr(), un.data_ptr(), out.data_ptr(), F._stream()))
        return out * umax.to(torch.float32)

    def iwes_vjp_tan(self, motion, motion_model: str, tangent, gimages, gimages_tan=None, directions=("first",), sigma: float = 0.0,
                     normalize_t: bool = True, with_orig: bool = False, exact_flow: bool = False) -> torch.Tensor:
        """d/d(eps) [ J(motion + eps tangent)^T (gimages + eps gimages_tan) ] at eps = 0, summed over the reference times
        (cmax_iwes_vjp_tan); gimages_tan None = 0: the mixed term alone.  With gimages_tan = (d2 l / dI2) J tangent this is the exact
        Hessian-vector product of a loss l(iwes(motion)).  Shape and dtype of `iwes_vjp`'s gradient."""
        m, d = self._iwes_args(motion, motion_model, directions, sigma, normalize_t, with_orig, exact_flow)
        n_planes = d.n_ref + d.with_orig
        g = self._iwes_planes(gimages, n_planes, "gimages")
        gt = torch.zeros_like(g) if gimages_tan is None else self._iwes_planes(gimages_tan, n_planes, "gimages_tan")
        un, umax = _unit_tangent(tangent, m.shape)
        if un is None:  # what is left is J^T gimages_tan
            return self.iwes_vjp(motion, motion_model, gt, directions, sigma, normalize_t, with_orig, exact_flow=exact_flow)[0]
        gt = (gt / umax.to(torch.float32)).contiguous()  # linear in (tangent, gimages_tan) jointly
        out = self._grad_out(d, m)
        check(self._lib.cmax_iwes_vjp_tan(self._h, ctypes.byref(d), m.data_ptr(), un.data_ptr(), g.data_ptr(), gt.data_ptr(),
                                          out.data_ptr(), F._stream()))
        return out * umax.to(out.dtype)

    # -- phase-split form (time-sliced multi-GPU, see distributed.py) --------------------------------
    def objective_vote(self, desc: CmaxObjective, motion, exact_flow: bool = False) -> torch.Tensor:
        """Raw votes of this handle's events: fp32 [n_images, Hp, Wp] (n_ref images, plus the un-warped
        image when a normalised cost needs it).  To be all-reduced (sum) across time slices."""
        m, desc = self._motion_arg(desc, motion, exact_flow)
        images = torch.empty((5,) + self.padded_size, dtype=torch.float32, device=self.device)
        n_images = ctypes.c_int(0)
        check(self._lib.cmax_objective_vote(self._h, ctypes.byref(desc), m.data_ptr(), images.data_ptr(),
                                            ctypes.byref(n_images), F._stream()))
        return images[: n_images.value]

    def objective_finish(self, desc: CmaxObjective, motion, images: torch.Tensor, want_grad: bool = True, exact_flow: bool = False):
        """Loss from the (globally reduced) images, gradient contribution of this handle's events.
        Without a blur (sigma == 0) the handle keeps pointers into `images` instead of a copy: a later last_iwe() reads that
        tensor's memory, so keep the tensor alive (and unchanged) until then -- a freed one gives stale values with no error."""
        m, desc = self._motion_arg(desc, motion, exact_flow)
        images = images.contiguous()
        result, grad = self._outputs(desc, m, want_grad)
        check(self._lib.cmax_objective_finish(self._h, ctypes.byref(desc), m.data_ptr(), images.data_ptr(),
                                              int(images.shape[0]), result.data_ptr(),
                                              grad.data_ptr() if grad is not None else None, F._stream()))
        return result, grad

    # -- deterministic mode ------------------------------------------------------------------------------------
    def set_deterministic(self, enable: bool = True):
        """Bit-identical IWE / loss / gradient from run to run (cmax_set_deterministic): integer accumulation wherever the
        order of events, workgroups or atomics would otherwise show in the last bits.  Slower; see include/cmax_hip.h."""
        check(self._lib.cmax_set_deterministic(self._h, int(bool(enable))))
        return self

    @property
    def deterministic(self) -> bool:
        v = ctypes.c_int(0)
        check(self._lib.cmax_get_deterministic(self._h, ctypes.byref(v)))
        return bool(v.value)

    # -- in-library collectives (RCCL over xGMI, see distributed.py) -------------------------------------
    def comm_available(self) -> Tuple[bool, str]:
        """(RCCL can be bound in this process, path of the shared object it was bound from) -- cmax_comm_available, a LOCAL
        call: ranks agree on it before any of them enters the blocking cmax_comm_init."""
        buf = ctypes.create_string_buffer(1024)
        rc = self._lib.cmax_comm_available(buf, len(buf))
        return rc == 0, buf.value.decode("utf-8", "replace")

    def comm_init(self, group=None, force_rccl: bool = False, timeout_s: float = 120.0):
        """Give this handle an RCCL communicator over the ranks of the torch.distributed `group` (default: the
        world): rank 0 draws the rendezvous id (cmax_comm_unique_id), torch.distributed ships it, every rank
        calls cmax_comm_init.  After that `evaluate_dist` needs no torch.distributed call at all.
        World size 1: no communicator (evaluate_dist == evaluate) unless force_rccl, which makes a real
        1-rank communicator so that the N > 1 enqueue sequence can be exercised on one GPU.
        No rank can be left waiting for another: (1) every rank first checks LOCALLY that RCCL can be bound and the
        ranks agree on that with one MIN all-reduce -- nobody enters ncclCommInitRank unless everybody will; (2) the blocking
        cmax_comm_init runs under a watchdog (`timeout_s`): a rank whose peers never arrive raises instead of hanging, and
        the caller (TimeSlicedObjective) then agrees on the torch.distributed fall-back."""
        import threading

        import torch.distributed as dist

        have = dist.is_available() and dist.is_initialized()
        world = dist.get_world_size(group) if have else 1
        rank = dist.get_rank(group) if have else 0
        if world == 1 and not force_rccl:
            check(self._lib.cmax_comm_init(self._h, None, 1, 0))
            return self
        ok, path = self.comm_available()
        err = None if ok else _lib.CmaxError(_lib.ENODEV, self._lib.cmax_last_error().decode("utf-8", "replace"))
        ids = [None]
        if rank == 0 and ok:
            buf = ctypes.create_string_buffer(_lib.COMM_ID_BYTES)
            try:
                check(self._lib.cmax_comm_unique_id(buf))
                ids = [buf.raw]
            except _lib.CmaxError as e:  # the other ranks wait in the exchange below: tell them before raising
                err, ok = e, False
        if world > 1:
            flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=self.device if dist.get_backend(group) == "nccl" else "cpu")
            dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)  # (1) everybody, or nobody
            if int(flag.item()) == 0:
                raise err if err is not None else _lib.CmaxError(_lib.ENODEV, "RCCL is not available on another rank")
            src = dist.get_global_rank(group, 0) if group is not None else 0
            dist.broadcast_object_list(ids, src=src, group=group)
        elif err is not None:
            raise err
        if ids[0] is None:
            raise _lib.CmaxError(_lib.ECOMM, "rank 0 could not draw an RCCL rendezvous id")
        out = {}

        def init():  # (2) ncclCommInitRank blocks until all ranks have called it; ctypes releases the GIL meanwhile
            try:
                with torch.cuda.device(self.device):  # the current HIP device is per thread
                    out["rc"] = self._lib.cmax_comm_init(self._h, ids[0], world, rank)
                    out["msg"] = self._lib.cmax_last_error() if out["rc"] else b""
            except Exception as e:  # pragma: no cover
                out["exc"] = e

        t = threading.Thread(target=init, name="cmax_comm_init", daemon=True)
        t.start()
        t.join(timeout_s)
        if t.is_alive():
            # The thread is still inside ncclCommInitRank and holds the raw handle: the handle must outlive it (a
            # cmax_comm_destroy / cmax_destroy now, followed by the stuck call returning, is a use-after-free or a leaked
            # communicator).  comm_destroy / close wait for it when it has ended by then, and otherwise leave the native handle alone.
            self._comm_init_thread = t
            raise _lib.CmaxError(_lib.ECOMM, f"cmax_comm_init did not return within {timeout_s:.0f} s: a rank never reached ncclCommInitRank")
        if "exc" in out:
            raise out["exc"]
        if out.get("rc", 0):
            if out["rc"] == _lib.EUNSUPPORTED:  # refused in the handle's state (per-event weights), like `check` raises it
                raise NotImplementedError((out.get("msg") or b"").decode("utf-8", "replace"))
            raise _lib.CmaxError(out["rc"], (out.get("msg") or b"").decode("utf-8", "replace"))
        self.rccl_path = path
        return self

    def comm_set_c2_bands(self, bands: int):
        """cmax_comm_set_c2_bands: dense objectives on owned groups all-reduce the gradient in `bands` row bands behind K3."""
        check(self._lib.cmax_comm_set_c2_bands(self._h, int(bands)))
        return self

    def comm_info(self) -> Tuple[int, int, int]:
        """(nranks, rank, RCCL version) of the handle's communicator; (1, 0, 0) without one."""
        n, r, v = ctypes.c_int(1), ctypes.c_int(0), ctypes.c_int(0)
        check(self._lib.cmax_comm_info(self._h, ctypes.byref(n), ctypes.byref(r), ctypes.byref(v)))
        return n.value, r.value, v.value

    def _comm_init_pending(self) -> bool:
        """True while a timed-out cmax_comm_init is still running on this handle (see comm_init)."""
        t = getattr(self, "_comm_init_thread", None)
        if t is None:
            return False
        t.join(0.0)
        if t.is_alive():
            return True
        self._comm_init_thread = None
        return False

    def comm_destroy(self):
        if self._comm_init_pending():
            raise _lib.CmaxError(-3, "a timed-out cmax_comm_init is still running on this handle")
        check(self._lib.cmax_comm_destroy(self._h))

    def comm_allreduce(self, t: torch.Tensor, op: str = "sum") -> torch.Tensor:
        """In-place all-reduce of a contiguous fp32 / fp64 device tensor on the handle's communicator."""
        if not (t.is_cuda and t.is_contiguous()):
            raise ValueError("comm_allreduce needs a contiguous device tensor")
        check(self._lib.cmax_comm_allreduce(self._h, t.data_ptr(), t.numel(), F._code(t), {"sum": 0, "min": 1, "max": 2}[op], F._stream()))
        return t

    def evaluate_dist(self, desc: CmaxObjective, motion, want_grad: bool = True, exact_flow: bool = False):
        """One cmax_objective_dist call: the evaluation of the whole time-sliced batch, both all-reduces enqueued
        by the library between its kernels.  Same returns as `evaluate`, the same on every rank."""
        m, desc = self._motion_arg(desc, motion, exact_flow)
        result, grad = self._outputs(desc, m, want_grad)
        check(self._lib.cmax_objective_dist(self._h, ctypes.byref(desc), m.data_ptr(), result.data_ptr(),
                                            grad.data_ptr() if grad is not None else None, F._stream()))
        return result, grad

    # -- per-patch translation search (pyramid re-initialisation) ----------------------------------------
    def patch_search(self, boxes, patch_image_size: Tuple[int, int], candidates, sigma: float = 1.0):
        """Score translation candidates per patch with the reference's small-patch cost
        (calculate_cost_for_small_patch, src/solver/patch_contrast_pyramid.py:372-414) in one launch.
          boxes [n_patch, 4] = x_min, x_max, y_min, y_max (rows first, sensor coordinates; crop_event semantics)
          candidates [n_patch, n_cand, 2] pixel per unit of the raw timestamps
        -> (loss [n_patch, n_cand] = GM(un-warped) / GM(warped)  (NormalizedGradientMagnitude, "minimize"),
            gm [n_patch, n_cand + 1] raw gradient magnitudes (last column: un-warped), count [n_patch])."""
        b = torch.as_tensor(np.asarray(boxes), dtype=torch.int32).reshape(-1, 4).contiguous().to(self.device)
        c = torch.as_tensor(np.asarray(candidates) if not isinstance(candidates, torch.Tensor) else candidates)
        c = c.to(device=self.device, dtype=torch.float32).reshape(b.shape[0], -1, 2).contiguous()
        n_patch, n_cand = int(b.shape[0]), int(c.shape[1])
        gm = torch.empty((n_patch, n_cand + 1), dtype=torch.float32, device=self.device)
        count = torch.empty(n_patch, dtype=torch.int32, device=self.device)
        check(self._lib.cmax_patch_search(self._h, n_patch, b.data_ptr(), int(patch_image_size[0]), int(patch_image_size[1]),
                                          n_cand, c.data_ptr() if n_cand else None, float(sigma), gm.data_ptr(),
                                          count.data_ptr(), F._stream()))
        loss = gm[:, -1:].double() / gm[:, :-1].double()
        return loss, gm, count

    # -- per-kernel timing (bench.py roofline) ---------------------------------------------------------
    def set_profiling(self, enable, repeat: int = 1):
        """enable: bracket every hot launch with HIP events.  repeat > 1: issue each hot launch `repeat` times
        inside its bracket (amortises the bracket's dispatch latency; TIMING ONLY, results are meaningless)."""
        check(self._lib.cmax_set_profiling(self._h, (int(repeat) if repeat > 1 else 1) if enable else 0))

    def read_profile(self) -> Dict[str, Tuple[float, int]]:
        """{kernel class: (total ms, launches)} measured with HIP events on the launch stream: the four hot
        classes, "finish" (k_finish* / k_finalize) and "comm" (RCCL collectives)."""
        ms = (ctypes.c_double * _lib.PROF_CLASSES)()
        cnt = (ctypes.c_int64 * _lib.PROF_CLASSES)()
        check(self._lib.cmax_read_profile_all(self._h, ms, cnt))
        names = ("vote", "stats", "gimage", "grad", "finish", "comm")
        return {n: (ms[i], cnt[i]) for i, n in enumerate(names)}

    def last_iwe(self, k: int = 0) -> torch.Tensor:
        """Copy of the IWE of reference time k of the last evaluation (fp32 [Hp, Wp]).  After objective_finish with sigma == 0 this
        reads the `images` tensor the caller handed over, which must still be alive (see there)."""
        out = torch.empty(self.padded_size, dtype=torch.float32, device=self.device)
        check(self._lib.cmax_copy_iwe(self._h, int(k), out.data_ptr(), F._stream()))
        return out


def _chain(g: Optional[torch.Tensor], gout: torch.Tensor, dtype, device) -> Optional[torch.Tensor]:
    """The chain rule of a fused loss for one input: its stored derivative g (None: not asked for) times dL/dloss, in the input's dtype
    on the input's device."""
    return None if g is None else (g.to(dtype) * gout.to(g.device).to(dtype)).to(device)


class _FusedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, motion, handle, desc, exact_flow=False):
        need = motion.requires_grad
        result, grad = handle.evaluate(desc, motion, want_grad=need, exact_flow=exact_flow)
        ctx.grad = grad
        ctx.mdtype = motion.dtype
        ctx.mdevice = motion.device
        return result[0].to(motion.dtype if motion.dtype.is_floating_point else torch.float64)

    @staticmethod
    def backward(ctx, gout):
        return _chain(ctx.grad, gout, ctx.mdtype, ctx.mdevice), None, None, None


class _FusedWeightedFn(torch.autograd.Function):
    """The fused loss on the tape in BOTH the motion and the per-event weights (cmax_objective_weight_grad); the handle already holds
    `weights` (ContrastObjective.__call__ set them)."""

    @staticmethod
    def forward(ctx, motion, weights, handle, desc, exact_flow=False):
        result, grad, grad_w = handle.evaluate_weight_grad(desc, motion, want_grad=motion.requires_grad, exact_flow=exact_flow)
        ctx.grad = grad
        ctx.grad_w = grad_w if weights.requires_grad else None
        ctx.mdtype, ctx.mdevice = motion.dtype, motion.device
        ctx.wdtype, ctx.wdevice = weights.dtype, weights.device
        return result[0].to(motion.dtype if motion.dtype.is_floating_point else torch.float64)

    @staticmethod
    def backward(ctx, gout):
        gm = _chain(ctx.grad, gout, ctx.mdtype, ctx.mdevice)
        gw = _chain(ctx.grad_w, gout, ctx.wdtype, ctx.wdevice)
        return gm, gw, None, None, None


class _FusedEventsFn(torch.autograd.Function):
    """The fused loss on the tape in the motion, the events themselves (cmax_objective_event_grad + compose_events_grad) and, when
    given, the per-event weights (one cmax_objective_weight_grad call more); the handle already holds the batch and the weights."""

    @staticmethod
    def forward(ctx, motion, events, weights, handle, desc, exact_flow=False):
        result, grad, ge, csum = handle.evaluate_event_grad(desc, motion, want_grad=motion.requires_grad, exact_flow=exact_flow)
        ctx.grad = grad
        ctx.grad_ev = None
        if events.requires_grad:
            ctx.grad_ev = compose_events_grad(ge, csum, handle._batch_t, ref_fractions(desc), bool(desc.normalize_t), handle._batch_t_range)
        ctx.grad_w = ctx.wdtype = ctx.wdevice = None
        if weights is not None and weights.requires_grad:
            ctx.grad_w = handle.evaluate_weight_grad(desc, motion, want_grad=False, exact_flow=exact_flow)[2]
            ctx.wdtype, ctx.wdevice = weights.dtype, weights.device
        ctx.mdtype, ctx.mdevice = motion.dtype, motion.device
        ctx.edtype, ctx.edevice = events.dtype, events.device
        return result[0].to(motion.dtype if motion.dtype.is_floating_point else torch.float64)

    @staticmethod
    def backward(ctx, gout):
        gm = _chain(ctx.grad, gout, ctx.mdtype, ctx.mdevice)
        ge = _chain(ctx.grad_ev, gout, torch.float64, ctx.edevice)  # (the product in the fp64 of compose_events_grad, rounded once)
        gw = _chain(ctx.grad_w, gout, ctx.wdtype, ctx.wdevice)
        return gm, (None if ge is None else ge.to(ctx.edtype)), gw, None, None, None


class _IwesVjpFn(torch.autograd.Function):
    """Backward of fused_iwes as a function of (dL/dimages, motion) -- itself differentiable: its backward is cmax_iwes_jvp (it is
    linear in dL/dimages) and cmax_iwes_vjp_tan with G' = 0 (the mixed term)."""

    @staticmethod
    def forward(ctx, gout, motion, handle, cfg, batch_id, want_w):
        _check_batch(handle, batch_id)
        grad, grad_w = handle.iwes_vjp(motion, gimages=gout, want_grad_w=want_w, **cfg)
        ctx.handle, ctx.cfg, ctx.batch_id = handle, cfg, batch_id
        ctx.save_for_backward(gout, motion)
        ctx.set_materialize_grads(False)
        gm = grad.to(motion.dtype if motion.dtype.is_floating_point else torch.float64).reshape(motion.shape).to(motion.device)
        if grad_w is None:
            return gm, None
        return gm, grad_w

    @staticmethod
    def backward(ctx, ggm, ggw):
        if ggw is not None:
            raise NotImplementedError("fused_iwes: a second derivative through the per-event weights is not built (first order only)")
        if ggm is None:
            return None, None, None, None, None, None
        gout, motion = ctx.saved_tensors
        handle, cfg = ctx.handle, ctx.cfg
        _check_batch(handle, ctx.batch_id)
        d_gout = d_motion = None
        if ctx.needs_input_grad[0]:
            d_gout = torch.zeros_like(gout)
            d_gout[: len(cfg["directions"])] = handle.iwes_jvp(motion, tangent=ggm, **cfg).to(gout.dtype)
        if ctx.needs_input_grad[1]:
            d_motion = handle.iwes_vjp_tan(motion, tangent=ggm, gimages=gout, gimages_tan=None, **cfg)
            d_motion = d_motion.to(motion.dtype).reshape(motion.shape).to(motion.device)
        return d_gout, d_motion, None, None, None, None


def _check_batch(handle, batch_id):
    if getattr(handle, "_batch_id", 0) != batch_id:
        raise RuntimeError("fused_iwes: the handle holds another batch than the one this graph was recorded on (set_events since the "
                           "forward pass)")


class _IwesFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, motion, weights, handle, cfg):
        ctx.handle, ctx.cfg, ctx.batch_id = handle, cfg, getattr(handle, "_batch_id", 0)
        ctx.save_for_backward(motion)
        ctx.wmeta = (weights.dtype, weights.device) if weights is not None else None
        ctx.set_materialize_grads(False)
        return handle.iwes(motion, **cfg)

    @staticmethod
    def backward(ctx, gout):
        if gout is None:
            return None, None, None, None
        (motion,) = ctx.saved_tensors
        want_w = ctx.wmeta is not None and ctx.needs_input_grad[1]
        gm, gw = _IwesVjpFn.apply(gout.contiguous(), motion, ctx.handle, ctx.cfg, ctx.batch_id, want_w)
        if gw is not None:
            gw = gw.to(ctx.wmeta[0]).to(ctx.wmeta[1])
        return (gm if ctx.needs_input_grad[0] else None), gw, None, None


def fused_iwes(handle: "CMaxHandle", motion: torch.Tensor, motion_model: str, directions=("first",), sigma: float = 0.0,
               normalize_t: bool = True, with_orig: bool = False, weights: Optional[torch.Tensor] = None,
               _weights_on_handle: bool = False, exact_flow: bool = False) -> torch.Tensor:
    """The images of warped events of the handle's batch ON THE AUTOGRAD TAPE: fp32 [K, Hp, Wp] (one image per reference time in
    `directions`, then the un-warped image when with_orig) -- what the reference's `arg["iwe"]` is to its costs, so that any torch
    expression on it (a CostBase subclass, a robust or learned loss, a loss against a frame) runs on the fused path.
    Differentiable TWICE in `motion` (backward: cmax_iwes_vjp; its backward: cmax_iwes_jvp and cmax_iwes_vjp_tan), so
    torch.autograd.grad(..., create_graph=True) and torch.autograd.functional.vhp give exact Hessian-vector products (cells held fixed,
    as everywhere); differentiable ONCE in `weights` ([n] per-event weights, put on the handle by this call as ContrastObjective
    does) -- a second derivative through the weights raises NotImplementedError, and the mixed derivative d2/(dmotion dweights) is
    not on the tape.
    The graph remembers the batch it was recorded on: backward raises RuntimeError after another set_events.  Anything else that
    happened to the handle in between (time slabs, other weights, other evaluations) is allowed, and a backward pass then computes
    with the handle's state AT BACKWARD TIME (the library re-derives windows and cells from the motion in every call).
    exact_flow: a float64 flow / voxel crosses into the library as it is, in the forward pass, the backward and the double backward
    (CMaxHandle._motion_arg); the default casts it to fp32."""
    if weights is not None:
        if not isinstance(weights, torch.Tensor):
            raise TypeError(f"weights must be a torch tensor, got {type(weights)}")
        if not _weights_on_handle:  # (ContrastObjective has set them for all its terms: one gather and synchronisation per call)
            handle.set_event_weights(weights.detach())
    directions = (directions,) if isinstance(directions, (str, int, float)) else tuple(directions)
    cfg = dict(motion_model=motion_model, directions=directions, sigma=float(sigma), normalize_t=bool(normalize_t), with_orig=bool(with_orig))
    if exact_flow:  # (only then a key of cfg: the handle methods' default otherwise)
        cfg["exact_flow"] = True
    motion = to_device_tensor(motion, "motion")
    return _IwesFn.apply(motion, weights, handle, cfg)


_IWE_KEYS = ("iwe", "backward_iwe", "forward_iwe", "middle_iwe", "orig_iwe")


class _CustomTerm:
    """A cost without a fused kernel: a CostBase instance or a callable arg_dict -> 0-dim tensor, evaluated in torch on fused_iwes."""

    def __init__(self, cost, warp_direction, sigma: float, normalize_t: bool):
        self.cost = cost
        self.calculate = cost.calculate if hasattr(cost, "calculate") else cost
        keys = list(getattr(cost, "required_keys", None) or ["iwe", "omit_boundary"])
        self.keys = [k for k in keys if k in _IWE_KEYS]
        if not any(k != "orig_iwe" for k in self.keys):
            self.keys.insert(0, "iwe")
        self.wants_flow = "flow" in keys
        # the mapping of _COST_TABLE: iwe / backward_iwe -> warp_direction, forward_iwe -> "last", middle_iwe -> "middle"
        ref = {"iwe": warp_direction, "backward_iwe": warp_direction, "forward_iwe": "last", "middle_iwe": "middle"}
        self.directions, self.index = [], {}
        for k in self.keys:
            if k == "orig_iwe":
                continue
            if ref[k] not in self.directions:
                self.directions.append(ref[k])
            self.index[k] = self.directions.index(ref[k])
        self.with_orig = "orig_iwe" in self.keys
        self.sigma, self.normalize_t = float(sigma), bool(normalize_t)

    def value(self, handle, motion, motion_model, omit_boundary, coarse_flow=None, weights=None, exact_flow=False):
        imgs = fused_iwes(handle, motion, motion_model, tuple(self.directions), self.sigma, self.normalize_t, self.with_orig, weights,
                          _weights_on_handle=weights is not None, exact_flow=exact_flow)
        arg = {k: imgs[i] for k, i in self.index.items()}
        if self.with_orig:
            arg["orig_iwe"] = imgs[len(self.directions)]
        arg["omit_boundary"] = omit_boundary
        if self.wants_flow and coarse_flow is not None:
            arg["flow"] = coarse_flow
        return self.calculate(arg)


class ContrastObjective:
    """loss = objective(motion[, coarse_flow]) with the reference's cost names.

    cost: any key of costs.functions or costs.focus_functions (FOCUS_COSTS: the mean-square, Laplacian and Hessian focus losses, fused
    like the gradient-magnitude trio), or "hybrid" with cost_with_weight={name: weight | "inv"}
    (src/costs/hybrid.py).  Event-based costs run as fused kernels on `handle`; total_variation runs
    on the patch flow handed in as `coarse_flow` (patch_contrast_base.py:349-350).
    A cost WITHOUT a fused kernel -- a CostBase instance, a callable arg_dict -> 0-dim tensor, or a name registered in
    costs.functions that is not among FUSED_COSTS -- is evaluated in torch on `fused_iwes` (the images its `required_keys` name, in the
    reference's `arg` dict with `omit_boundary`; padded images, cropped only by the cost itself); its gradient and `hvp` are torch's
    backward and double backward through that layer.  Names unknown to costs.functions raise KeyError.
    exact_flow: a float64 dense flow / voxel is handed to the library unchanged (the cells of events on a cell border are then
    decided from the doubles, as for a float64 2-DoF theta); the gradient comes back in float64, cast from the fp32 output."""

    def __init__(self, handle: CMaxHandle, motion_model: str, cost: str = "image_variance",
                 cost_with_weight: Optional[Dict[str, Union[float, str]]] = None, direction: str = "minimize",
                 sigma: float = 0.0, omit_boundary: bool = True, normalize_t: bool = True,
                 warp_direction: Union[str, float] = "first", exact_flow: bool = False):
        self.handle = handle
        self.exact_flow = bool(exact_flow)  # a float64 flow / voxel crosses into the library as it is (CMaxHandle._motion_arg)
        self.motion_model = motion_model
        self.direction = direction
        self.omit_boundary = omit_boundary
        terms = cost_with_weight if cost == "hybrid" else {cost: 1.0}
        if cost == "hybrid" and not cost_with_weight:
            raise ValueError("hybrid cost needs cost_with_weight")
        self.terms = []
        for name, weight in terms.items():
            if name == "total_variation":
                self.terms.append((name, weight, None))
            elif not isinstance(name, str) or (name not in _COST_TABLE and name in _cost_registry()):
                cost_obj = _cost_registry()[name](direction=direction) if isinstance(name, str) else name
                if not (callable(cost_obj) or hasattr(cost_obj, "calculate")):
                    raise TypeError(f"cost must be a name, a CostBase instance or a callable, got {type(cost_obj)}")
                self.terms.append((name, weight, _CustomTerm(cost_obj, warp_direction, sigma, normalize_t)))
            else:
                desc = make_descriptor(name, motion_model, direction, sigma, omit_boundary, normalize_t,
                                       handle.time_bin if F.MODEL_CODES[motion_model] == _lib.MODEL_VOXEL else 0,
                                       warp_direction)
                self.terms.append((name, weight, desc))

    has_exact_hvp = True  # every fused term, numeric and "inv" weights (total_variation does not depend on `motion`); custom terms by double backward

    def _custom_hvp(self, term, weight, motion, v64):
        """H v of combine(weight, cost(fused_iwes(motion))): torch's double backward through the layer."""
        m = to_device_tensor(motion, "motion").detach().clone().requires_grad_()
        with torch.enable_grad():
            value = combine(weight, term.value(self.handle, m, self.motion_model, self.omit_boundary, exact_flow=self.exact_flow))
            (g,) = torch.autograd.grad(value, m, create_graph=True)
            if not g.requires_grad:
                return torch.zeros_like(v64)
            (hv,) = torch.autograd.grad((g * v64.reshape(g.shape).to(g.dtype)).sum(), m, allow_unused=True)
        return torch.zeros_like(v64) if hv is None else hv.detach().to(torch.float64).reshape(v64.shape)

    def hvp(self, motion: torch.Tensor, vector: torch.Tensor) -> torch.Tensor:
        """Exact Hessian-vector product w.r.t. `motion` (same shape/dtype as motion).  A term of weight w contributes
        w * H_c v (cmax_objective_hvp); an "inv" term phi(c) = 1 / c contributes phi' H_c v + phi'' <grad c, v> grad c
        with c and grad c from one cmax_objective call (src/costs/hybrid.py:51-53 differentiated twice)."""
        from .costs.hybrid import combine_derivatives

        out = None
        v64 = to_device_tensor(vector, "vector").detach().to(torch.float64)
        for name, weight, desc in self.terms:
            if desc is None:
                continue  # total_variation acts on the coarse flow, not on `motion`
            if isinstance(desc, _CustomTerm):
                hv = self._custom_hvp(desc, weight, motion, v64)
                out = hv if out is None else out + hv.reshape(out.shape)
                continue
            hv = self.handle.hvp(desc, motion, vector, exact_flow=self.exact_flow).to(torch.float64)
            if weight == "inv":
                res, grad = self.handle.evaluate(desc, motion, want_grad=True, exact_flow=self.exact_flow)
                p1, p2 = combine_derivatives("inv", res[0])
                g64 = grad.to(torch.float64).reshape(v64.shape)
                hv = p1 * hv + p2 * (g64 * v64).sum() * g64.reshape(hv.shape)
            else:
                hv = hv * float(weight)
            out = hv if out is None else out + hv
        if out is None:
            out = torch.zeros_like(vector, dtype=torch.float64)
        return out.reshape(vector.shape).to(vector.dtype if vector.dtype.is_floating_point else torch.float64)

    def descend(self, theta0, method: str = "Adam", n_iter: int = 100, lr: float = 0.05, lr_step: Optional[int] = None, lr_decay: float = 0.1,
                momentum: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8, trace: bool = False):
        """n_iter iterations of torch.optim.SGD / Adam with StepLR(lr_step, lr_decay) on this objective in ONE library call
        (CMaxHandle.descend; the reference's run_torch with its constants as defaults, src/solver/base.py:857-862; lr_step None: n_iter).
        2-DoF models with exactly one fused term of weight 1: a hybrid of several terms (or an "inv" weight, a total_variation member, a
        cost without a fused kernel) has no single fused objective whose gradient the device-side step could read -- refused."""
        desc = self._descent_term()
        return self.handle.descend(desc, theta0, _lib.descent_descriptor(method, n_iter, lr, lr_step, lr_decay, momentum, betas, eps), trace=trace)

    def minimize_lbfgs(self, theta0, n_eval: int = 32, history: int = 8, gtol: float = 1e-5, max_move: float = 10.0, max_ls: int = 10,
                       c1: float = 1e-4, shrink: float = 0.5, curv_eps: float = 1e-10, step0: float = 1.0, trace: bool = False):
        """L-BFGS with a backtracking line search on this objective in ONE library call (CMaxHandle.minimize_lbfgs; the rules:
        include/cmax_hip.h).  2-DoF models with exactly one fused term of weight 1, as `descend`.  theta stays within max_move of theta0:
        the batch's time slabs are decided ONCE, from max|theta0| + max_move (by CMaxHandle.minimize_lbfgs).  Returns a _lib.LbfgsResult."""
        desc = self._descent_term()
        return self.handle.minimize_lbfgs(desc, theta0, _lib.lbfgs_descriptor(n_eval, history, max_ls, c1, shrink, curv_eps, gtol, step0, max_move), trace=trace)

    def _descent_term(self) -> CmaxObjective:
        """The one fused term a device-resident descent steps on, or NotImplementedError with what is refused."""
        if F.MODEL_CODES[self.motion_model] != _lib.MODEL_2DOF:
            raise NotImplementedError(f"descend: 2-DoF motion models only, not {self.motion_model!r} (a patch grid descends through PatchFlowObjective.descend)")
        if len(self.terms) != 1 or self.terms[0][2] is None or isinstance(self.terms[0][2], _CustomTerm):
            raise NotImplementedError("descend: the device-resident loop steps on ONE fused term; this objective combines "
                                      f"{[name for name, _, _ in self.terms]} (several terms, total_variation or a cost without a fused kernel)")
        name, weight, desc = self.terms[0]
        if weight == "inv" or float(weight) != 1.0:
            raise NotImplementedError(f"descend: the term's weight must be 1 (got {weight!r}): the step reads the fused term's own gradient")
        return desc

    def descend_batch(self, theta0s, method: str = "Adam", n_iter: int = 100, lr: float = 0.05, lr_step: Optional[int] = None, lr_decay: float = 0.1,
                      momentum: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8, trace: bool = False) -> list:
        """`descend` from K starts `theta0s` [K, 2] as K independent trajectories in ONE library call per 64 starts (CMaxHandle.descend_batch;
        multi-start for a non-convex objective: the reference's "global-best" grid is correct only to its spacing, src/solver/
        patch_contrast_base.py:164-187).  Same arguments and refusals as `descend`; returns a list of K _lib.DescentResult.  Like `descend` it
        leaves the batch's time-slab order as the caller set it: no host stands between the iterations, so whoever wants slabs decides them
        once, for all starts, before the call (solver.translation_search.refine_translation: from max |theta0| + lr * n_iter)."""
        desc = self._descent_term()
        return self.handle.descend_batch(desc, theta0s, _lib.descent_descriptor(method, n_iter, lr, lr_step, lr_decay, momentum, betas, eps), trace=trace)

    def evaluate_candidates(self, motions, coarse_flows=None) -> torch.Tensor:
        """Loss of K candidate motions `motions` [K, ...] -> float64 [K] on the device: one cmax_objective_batch call per fused term
        (the reference's gradient-free paths score batches of sampled motions, src/solver/base.py:738-758,
        src/solver/patch_contrast_base.py:126-187).  total_variation members act on `coarse_flows` [K, 2, ph, pw]; for a 2-DoF
        translation the reference hands them a [2, 1, 1] flow, whose total variation is 0: they may be omitted there."""
        mt = to_device_tensor(motions, "motions").detach()
        K = int(mt.shape[0])
        loss = torch.zeros(K, dtype=torch.float64, device=self.handle.device)
        for name, weight, desc in self.terms:
            if desc is None:
                if coarse_flows is None:
                    if F.MODEL_CODES[self.motion_model] == _lib.MODEL_2DOF:
                        continue
                    raise KeyError("flow")
                cf = to_device_tensor(coarse_flows, "flow")
                value = torch.stack([F.total_variation(cf[k], self.omit_boundary) for k in range(K)]).to(torch.float64)
                if self.direction != "minimize":
                    value = -value
            elif isinstance(desc, _CustomTerm):
                with torch.no_grad():
                    value = torch.stack([torch.as_tensor(desc.value(self.handle, mt[k], self.motion_model, self.omit_boundary, exact_flow=self.exact_flow)).to(torch.float64)
                                         for k in range(K)]).to(self.handle.device)
            else:
                results, _ = self.handle.evaluate_batch(desc, mt, exact_flow=self.exact_flow)
                value = results[:, 0]
            loss = loss + combine(weight, value)
        return loss

    def __call__(self, motion: torch.Tensor, coarse_flow: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None,
                 events: Optional[torch.Tensor] = None) -> torch.Tensor:
        """weights: None -- the loss of the handle as it stands, differentiable in `motion`.  A tensor [n] -- per-event weights of the
        handle's batch (the reference's `weight` on the autograd tape): the loss is differentiable in `motion` AND `weights`
        (either may not require grad); hybrid members, "inv" included, follow through `combine`, total_variation does not depend on
        the weights.  Each such call pays set_event_weights: one gather plus its one synchronisation; the weights stay on the handle.
        events: an [n, 4] tensor that holds the batch the handle was given (checked by shape only) and requires grad -- the reference's
        `events` leaf (src/solver/patch_contrast_mixed.py:166): backward fills `events.grad` [n, 4] (x, y, t, polarity = 0).  May be
        combined with `weights`."""
        if weights is not None:
            if not isinstance(weights, torch.Tensor):
                raise TypeError(f"weights must be a torch tensor, got {type(weights)}")
            self.handle.set_event_weights(weights.detach())
        if events is not None:
            if not isinstance(events, torch.Tensor):
                raise TypeError(f"events must be a torch tensor, got {type(events)}")
            n = int(getattr(self.handle, "_n_in", 0))
            if tuple(events.shape) != (n, 4):
                raise ValueError(f"events must be the handle's batch, [n, 4] = [{n}, 4], got {tuple(events.shape)}")
        loss = 0.0
        for name, weight, desc in self.terms:
            if desc is None:
                if coarse_flow is None:
                    raise KeyError("flow")
                value = F.total_variation(to_device_tensor(coarse_flow, "flow"), self.omit_boundary)
                if self.direction != "minimize":
                    value = -value
            elif isinstance(desc, _CustomTerm):
                if events is not None:
                    raise NotImplementedError("dL/d(event) of a cost without a fused kernel is not built")
                value = desc.value(self.handle, motion, self.motion_model, self.omit_boundary, coarse_flow, weights, self.exact_flow)
            else:
                if events is not None:
                    value = _FusedEventsFn.apply(motion, events, weights, self.handle, desc, self.exact_flow)
                elif weights is None:
                    value = _FusedFn.apply(motion, self.handle, desc, self.exact_flow)
                else:
                    value = _FusedWeightedFn.apply(motion, weights, self.handle, desc, self.exact_flow)
            value = value.to(motion.device) if isinstance(motion, torch.Tensor) else value
            loss = loss + combine(weight, value)
        return loss
