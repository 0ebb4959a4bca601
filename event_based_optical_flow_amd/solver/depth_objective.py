"""The optimiser's objective for depth and ego-motion: the motion field of a static scene over a grid of inverse depth, entirely on the GPU.

Unknowns x = [a (Ka) | b (Kb) | s (ph pw)]: with two bases on the sensor, A [Ka,2,H,W] (the translational field per unit inverse depth)
and B [Kb,2,H,W] (what does not depend on depth: the rotational field), and Q the bilinear interpolation of the patch grid on one plane
(without the negation the patch map carries),
    rho = Q s,   D = rho * sum_k a_k A_k + sum_j b_j B_j.
Gallego, Rebecq, Scaramuzza (CVPR 2018) list depth beside motion and optical flow as applications of contrast maximisation; Shiba, Klose,
Aoki, Gallego (TPAMI 2024) put inverse depth on a patch grid and the camera motion on six global parameters.  The reference has no
counterpart (its models: 2-DoF translation, per-pixel flow, patch grid); D is warped by its dense-flow rule x' = x - dt * D[src]
(src/warp.py:263-313).  The chain is the patch objective's with the interpolation exchanged for that map:
  x -> dense flow (cmax_depth_to_dense) -> x t_scale [-> Burgers / upwind voxel (cmax_voxel_construct)] -> fused contrast objective
and the native plan (cmax_depth_plan_create, csrc/cmax_solver.hip) IS a patch plan with that map: one library call per evaluation, the
exact product (the map is a product of unknowns, so the product carries the map's second-order adjoint), the device-resident descent and
L-BFGS.

GAUGE.  (a, s) -> (lambda a, s / lambda) leaves D unchanged: the loss is constant along that line and the Hessian singular.  That is a
property of the model.  Nothing here removes it; `canonical` picks the representative with |a|_2 = 1.
NOT BUILT: regularisers on the depth grid (total variation included) and positivity of rho, the nearest filter, handles with a
communicator or per-event weights, a pyramid over the depth grid.
"""
import ctypes
from typing import Dict, Optional, Union

import numpy as np
import torch

from .. import _lib
from .. import functional as F
from ..cmax import CMaxHandle, ContrastObjective
from ..utils.flow_utils import motion_field_basis
from .patch_objective import patch_pad


class DepthEgoMotionObjective:
    def __init__(self, handle: CMaxHandle, t_scale: float, patch_image_size, patch_size, sliding_window, patch_shift=(0, 0), calib=None,
                 bases=None, cost="hybrid", cost_with_weight: Optional[Dict[str, Union[float, str]]] = None, blur_sigma: float = 1.0,
                 time_aware: bool = False, time_bin: int = 10, flow_interpolation: str = "burgers", t0_flow_location: str = "middle",
                 omit_boundary: bool = True, exact_flow: bool = False, flow_regularizer=None, filter_type: str = "bilinear"):
        """patch_image_size (ph, pw), patch_size, sliding_window, patch_shift: the grid of inverse depth, as PatchFlowObjective's grid.
        calib = (fx, fy, cx, cy): the bases are utils.flow_utils.motion_field_basis (three translational, three rotational fields, float64);
        or bases = (A, B) on the handle's sensor (numpy arrays or tensors of one dtype, float32 or float64; B may be None or have no field;
        1 <= Ka, Ka + Kb <= 64), kept on the device in their dtype.  The other arguments are FlowBasisObjective's.  There is no
        total_variation term, no `scale_later`, and only the bilinear filter.  Numeric hybrid weights of fused costs run on the native plan;
        "inv" weights and costs without a fused kernel keep the autograd-chained path of `__call__`."""
        self.handle = handle
        self.t_scale = float(t_scale)
        if filter_type != "bilinear":
            raise ValueError(f"filter_type {filter_type!r}: only the bilinear filter is built for the depth grid")
        if (calib is None) == (bases is None):
            raise ValueError("give calib = (fx, fy, cx, cy) or bases = (A, B), one of the two")
        A, B = motion_field_basis(handle.image_size, calib) if bases is None else bases
        A = torch.as_tensor(A)
        if A.dtype not in (torch.float32, torch.float64):
            A = A.to(torch.float64)
        shape = (2,) + tuple(handle.image_size)
        if A.dim() != 4 or tuple(A.shape[1:]) != shape:
            raise ValueError(f"A must be [Ka, 2, {shape[1]}, {shape[2]}], got {tuple(A.shape)}")
        B = torch.zeros((0,) + shape, dtype=A.dtype) if B is None else torch.as_tensor(B).to(A.dtype)
        if B.dim() != 4 or tuple(B.shape[1:]) != shape:
            raise ValueError(f"B must be [Kb, 2, {shape[1]}, {shape[2]}], got {tuple(B.shape)}")
        self.Ka, self.Kb = int(A.shape[0]), int(B.shape[0])
        if not (1 <= self.Ka and self.Ka + self.Kb <= _lib.BASIS_MAX_K):
            raise ValueError(f"the bases have 1 <= Ka and Ka + Kb <= {_lib.BASIS_MAX_K} fields, got Ka = {self.Ka}, Kb = {self.Kb}")
        self.A = A.to(handle.device).contiguous()
        self.B = B.to(handle.device).contiguous()
        self.patch_image_size = (int(patch_image_size[0]), int(patch_image_size[1]))
        self.sliding_window = (int(sliding_window[0]), int(sliding_window[1]))
        self.pad = patch_pad(patch_size, sliding_window, patch_shift)
        self.geometry = self.patch_image_size + self.pad + self.sliding_window
        self._ns = self.patch_image_size[0] * self.patch_image_size[1]
        self._nx = self.Ka + self.Kb + self._ns
        # max |A_k|, max |B_j|: the bound of `flow_bound`
        self.amax = self.A.abs().reshape(self.Ka, -1).amax(dim=1).to(torch.float64).cpu().numpy()
        self.bmax = self.B.abs().reshape(self.Kb, -1).amax(dim=1).to(torch.float64).cpu().numpy() if self.Kb else np.zeros(0)
        self.time_aware = bool(time_aware)
        self.time_bin = int(time_bin)
        self.flow_interpolation = flow_interpolation
        self.t0_flow_location = t0_flow_location
        if self.time_aware and handle.time_bin != self.time_bin:
            handle.set_time_bins(self.time_bin)
        model = "dense-flow-voxel" if self.time_aware else "dense-flow"
        self.exact_flow = bool(exact_flow)
        self.contrast = ContrastObjective(handle, model, cost=cost, cost_with_weight=cost_with_weight, sigma=blur_sigma,
                                          omit_boundary=omit_boundary, exact_flow=self.exact_flow)
        if any(desc is None for _, _, desc in self.contrast.terms):
            raise ValueError("total_variation is not built for the depth grid (no regulariser on the grid is)")
        self.device = handle.device  # read by scipy_autograd.TorchWrapper
        self.auto_slabs = True
        self._plan = None
        self._build_native_plan()
        self.flow_reg = None
        if flow_regularizer is not None:
            self.set_flow_regularizer(flow_regularizer)

    # -- one-call native path (cmax_depth_plan_create + cmax_patch_plan_*, csrc/cmax_solver.hip) ----------------------
    def _descriptor(self):
        """cmax_depth_objective_t of this objective, or None where only the autograd-chained path exists."""
        from ..cmax import _CustomTerm

        terms = [(w, desc) for _, w, desc in self.contrast.terms]
        if not terms or len(terms) > 4 or any(isinstance(desc, _CustomTerm) or w == "inv" for w, desc in terms):
            return None
        d = _lib.CmaxDepthObjective()
        d.n_terms = len(terms)
        d.time_aware = int(self.time_aware)
        d.T = self.time_bin if self.time_aware else 0
        d.scheme = F.SCHEME_CODES.get(self.flow_interpolation, -1) if self.time_aware else 0
        if self.time_aware and (d.scheme < 0 or self.t0_flow_location not in ("first", "middle")):
            return None
        d.t0 = (self.time_bin // 2 if self.t0_flow_location == "middle" else 0) if self.time_aware else 0
        d.H, d.W = self.handle.image_size
        d.Ka, d.Kb = self.Ka, self.Kb
        d.ph, d.pw, d.pad_h, d.pad_w, d.sw_h, d.sw_w = self.geometry
        d.basis_dtype = F._code(self.A)
        d.scale_later = 0
        d.filter_type = _lib.FILTER_BILINEAR
        d.t_scale = self.t_scale
        d.tv_weight = 0.0
        for i, (w, desc) in enumerate(terms):
            d.weight[i] = float(w)
            d.term[i] = desc
            d.term[i].motion_dtype = _lib.F64 if self.exact_flow else _lib.F32  # (a copy: the ContrastObjective's descriptors stay as they are)
        return d

    def _build_native_plan(self):
        d = self._descriptor()
        if d is None:
            return  # the autograd-chained path
        plan = ctypes.c_void_p()
        with torch.cuda.device(self.handle.device):
            _lib.check(_lib.load().cmax_depth_plan_create(self.handle._h, ctypes.byref(d), self.A.data_ptr(), self.B.data_ptr() if self.Kb else None,
                                                          F._stream(), ctypes.byref(plan)))
        self._plan = plan

    def __del__(self):
        plan, self._plan = getattr(self, "_plan", None), None
        if plan:
            try:
                _lib.load().cmax_patch_plan_destroy(plan)
            except Exception:  # interpreter shutdown
                pass

    def set_t_scale(self, t_scale: float):
        """The next batch behind the same handle has another duration."""
        self.t_scale = float(t_scale)
        if self._plan is not None:
            _lib.check(_lib.load().cmax_patch_plan_set_t_scale(self._plan, self.t_scale))

    def set_flow_regularizer(self, flow_regularizer):
        """One more term, weight * functional.flow_regularizer(F), on the displacement field F = t_scale * D(x), as
        FlowBasisObjective.set_flow_regularizer: {"kind": "divergence" | "area", "weight", "eps", "s"}; None removes the term."""
        desc = None if flow_regularizer is None else _lib.flow_regularizer_from_config(flow_regularizer)
        if self._plan is not None:
            _lib.check(_lib.load().cmax_patch_plan_set_flow_regularizer(self._plan, None if desc is None else ctypes.byref(desc)))
        self.flow_reg = desc

    def native_plan_info(self):
        """(number of captured hipGraphs, graph replay enabled) of the native plan."""
        n, ok = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(_lib.load().cmax_patch_plan_info(self._plan, ctypes.byref(n), ctypes.byref(ok)))
        return n.value, bool(ok.value)

    @property
    def has_native_plan(self) -> bool:
        """TorchWrapper calls `value_and_grad_numpy` / `hvp_numpy` when this is True."""
        return self._plan is not None

    @property
    def has_exact_hvp(self) -> bool:
        """The product exists on the native plan only: t [J^T (H_FF t J v) + (dJ[v])^T g_F], time-aware plans with the second-order
        adjoint of the voxel chain in between."""
        return self._plan is not None and self.contrast.has_exact_hvp

    # -- the unknowns ---------------------------------------------------------------------------------------------------
    @property
    def nx(self) -> int:
        return self._nx

    def _x(self, x, what="x") -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        if x.size != self._nx:
            raise ValueError(f"{what} has {x.size} elements, the model has {self._nx} unknowns ({self.Ka} + {self.Kb} + {self._ns})")
        return x

    def split(self, x):
        """x [nx] (array or tensor) -> (a [Ka], b [Kb], s [ph,pw]): views."""
        x = x.reshape(-1)
        if x.shape[0] != self._nx:
            raise ValueError(f"x has {x.shape[0]} elements, the model has {self._nx} unknowns ({self.Ka} + {self.Kb} + {self._ns})")
        return x[:self.Ka], x[self.Ka:self.Ka + self.Kb], x[self.Ka + self.Kb:].reshape(self.patch_image_size)

    def canonical(self, x):
        """The representative of x's gauge orbit with |a|_2 = 1: (a / |a|, b, s |a|).  D is unchanged.  x with a = 0 is returned as it is."""
        a, b, s = self.split(x)
        if isinstance(x, torch.Tensor):
            lam = a.norm()
            return x.reshape(-1).clone() if float(lam) == 0.0 else torch.cat([a / lam, b, (s * lam).reshape(-1)])
        lam = float(np.linalg.norm(a))
        return np.array(x, dtype=np.float64).reshape(-1) if lam == 0.0 else np.concatenate([a / lam, b, (s * lam).reshape(-1)])

    def inverse_depth(self, x: torch.Tensor) -> torch.Tensor:
        """x -> rho = Q s [H,W] on the device (float64): the interpolated inverse depth, in the gauge x is in."""
        _, _, s = self.split(x.detach().to(self.handle.device, torch.float64))
        ph, pw, pad_h, pad_w, sw_h, sw_w = self.geometry
        two = torch.stack([s, torch.zeros_like(s)]).contiguous()
        return -F.patch_to_dense(two, self.handle.image_size, (sw_h, sw_w), (pad_h, pad_w))[0]

    def flow_bound(self, x) -> float:
        """(max|s| sum_k |a_k| max|A_k| + sum_j |b_j| max|B_j|) |t_scale|: no pixel is displaced further over the batch (Q is a convex
        combination, so |Q s| <= max|s|)."""
        x = x.detach().to(torch.float64).reshape(-1).cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, dtype=np.float64).reshape(-1)
        a, b, s = self.split(np.abs(x))
        return float(s.max() * (a * self.amax).sum() + (b * self.bmax).sum()) * abs(self.t_scale)

    def ensure_time_slabs(self, x) -> int:
        """Before an evaluation at `x` the batch is put into the time-slab order its largest displacement asks for
        (CMaxHandle.auto_time_slabs), from the bound `flow_bound`.  Time-aware objectives keep their time bins."""
        if self.time_aware or not self.auto_slabs:
            return 0
        return self.handle.auto_time_slabs(self.flow_bound(x))

    # -- evaluations ----------------------------------------------------------------------------------------------------
    def value_and_grad_numpy(self, x: np.ndarray, want_grad: bool = True):
        """x [nx] float64 (host) -> (loss, gradient [nx] float64): one cmax_patch_plan_evaluate call."""
        x = self._x(x)
        self.ensure_time_slabs(x)
        loss = ctypes.c_double(0.0)
        grad = np.empty(self._nx, dtype=np.float64) if want_grad else None
        with torch.cuda.device(self.handle.device):
            _lib.check(_lib.load().cmax_patch_plan_evaluate(self._plan, x.ctypes.data, 0, ctypes.byref(loss),
                                                            grad.ctypes.data if want_grad else None, F._stream()))
        return loss.value, grad

    def hvp_numpy(self, x: np.ndarray, v: np.ndarray) -> np.ndarray:
        """Exact Hessian-vector product on host arrays: one cmax_patch_plan_hvp call."""
        x, v = self._x(x), self._x(v, "v")
        self.ensure_time_slabs(x)
        hv = np.empty(self._nx, dtype=np.float64)
        with torch.cuda.device(self.handle.device):
            _lib.check(_lib.load().cmax_patch_plan_hvp(self._plan, x.ctypes.data, v.ctypes.data, hv.ctypes.data, F._stream()))
        return hv

    def hvp(self, x: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
        """`hvp_numpy` on tensors."""
        hv = self.hvp_numpy(x.detach().cpu().numpy(), v.detach().cpu().numpy())
        return torch.as_tensor(hv, dtype=x.dtype, device=x.device).reshape(x.shape)

    def descend(self, x0: np.ndarray, method: str = "Adam", n_iter: int = 100, lr: float = 0.05, lr_step: Optional[int] = None,
                lr_decay: float = 0.1, momentum: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8, trace: bool = False):
        """n_iter iterations of torch.optim.SGD / Adam with StepLR(lr_step, lr_decay) from x0 in ONE cmax_patch_plan_descend call
        (FlowBasisObjective.descend).  Time slabs are decided ONCE, from the bound at |x0| + lr * n_iter per entry (Adam; SGD: x0 alone)."""
        if self._plan is None:
            raise NotImplementedError("descend needs the native plan (numeric hybrid weights, fused costs)")
        x0 = self._x(x0, "x0")
        descent = _lib.descent_descriptor(method, n_iter, lr, lr_step, lr_decay, momentum, betas, eps)
        self.ensure_time_slabs(np.abs(x0) + (float(lr) * int(n_iter) if method == "Adam" else 0.0))
        fn, plan, stream = _lib.load().cmax_patch_plan_descend, self._plan, F._stream()
        with torch.cuda.device(self.handle.device):
            return _lib.run_descent(lambda o, res, xl, xb, hist, tr: fn(plan, x0.ctypes.data, 0, o, res, xl, xb, hist, tr, stream),
                                    self._nx, descent, trace)

    def minimize_lbfgs(self, x0: np.ndarray, n_eval: int = 32, history: int = 8, gtol: float = 1e-5, max_move: float = 10.0, max_ls: int = 10,
                       c1: float = 1e-4, shrink: float = 0.5, curv_eps: float = 1e-10, step0: float = 1.0, trace: bool = False):
        """L-BFGS with a backtracking line search from x0 in ONE cmax_patch_plan_lbfgs call (FlowBasisObjective.minimize_lbfgs; the
        rules: include/cmax_hip.h).  Every unknown stays within max_move of x0: time slabs are decided ONCE, from the bound at
        |x0| + max_move per entry.  Returns a _lib.LbfgsResult."""
        if self._plan is None:
            raise NotImplementedError("minimize_lbfgs needs the native plan (numeric hybrid weights, fused costs)")
        x0 = self._x(x0, "x0")
        lbfgs = _lib.lbfgs_descriptor(n_eval, history, max_ls, c1, shrink, curv_eps, gtol, step0, max_move)
        self.ensure_time_slabs(np.abs(x0) + abs(float(max_move)))
        fn, plan, stream = _lib.load().cmax_patch_plan_lbfgs, self._plan, F._stream()
        with torch.cuda.device(self.handle.device):
            return _lib.run_lbfgs(lambda o, res, x, hist, al, code, tr: fn(plan, x0.ctypes.data, 0, o, res, x, hist, al, code, tr, stream),
                                  self._nx, lbfgs, trace)

    # -- the autograd-chained path ----------------------------------------------------------------------------------------
    def flow_field(self, x: torch.Tensor) -> torch.Tensor:
        """x [nx] -> the displacement field [2,H,W] over the batch, t_scale * depth_to_dense(x): what the flow regulariser acts on."""
        a, b, s = self.split(x.reshape(-1))
        return F.depth_to_dense(a, b if self.Kb else None, s, self.A, self.B if self.Kb else None, self.geometry) * self.t_scale

    def dense_flow(self, x: torch.Tensor) -> torch.Tensor:
        """x [nx] -> [2,H,W] (or [T,2,H,W]) flow in pixel per NORMALISED time, in the bases' dtype."""
        dense = self.flow_field(x)
        if self.time_aware:  # the voxel is built on the displacement field, as in PatchFlowObjective.dense_flow
            dense = F.construct_dense_flow_voxel(dense, self.time_bin, self.flow_interpolation, self.t0_flow_location)
        return dense

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        """The autograd-chained path: depth_to_dense -> ContrastObjective, one Python-level call per stage."""
        x = x.to(self.handle.device)
        self.ensure_time_slabs(x)
        loss = self.contrast(self.dense_flow(x))
        if self.flow_reg is not None:
            r = self.flow_reg
            loss = loss + r.weight * F.flow_regularizer(self.flow_field(x), r.kind, r.eps, r.s)
        return loss
