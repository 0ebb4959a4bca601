"""The optimiser's objective for a GLOBAL motion model that is linear in its parameters: theta[K] -> loss, entirely on the GPU.

The dense flow is D = sum_k theta_k B_k for a basis B [K,2,H,W] -- similarity (4 parameters), affine (6), the rotational motion field
of a calibrated camera (3), or any basis the caller brings (polynomial, PCA, learned): what lies between the 2-DoF translation and the
thousands of unknowns of a patch grid.  The reference has no counterpart (its models: 2-DoF translation, per-pixel flow, patch grid);
D is warped by its dense-flow rule x' = x - dt * D[src] (src/warp.py:263-313).  The chain is the patch objective's with the patch
interpolation P exchanged for B:
  theta -> dense flow (cmax_basis_to_dense) -> x t_scale [-> Burgers / upwind voxel (cmax_voxel_construct)]
        -> fused contrast objective (cmax_objective)
and the native plan (cmax_basis_plan_create, csrc/cmax_solver.hip) IS a patch plan with that map: one library call per evaluation,
the exact product H_theta = t^2 B^T H_flow B, the device-resident descent.
"""
import ctypes
from typing import Dict, Optional, Union

import numpy as np
import torch

from .. import _lib
from .. import functional as F
from ..cmax import CMaxHandle, ContrastObjective
from ..utils.flow_utils import flow_basis


class FlowBasisObjective:
    def __init__(self, handle: CMaxHandle, t_scale: float, basis_or_model, cost="hybrid",
                 cost_with_weight: Optional[Dict[str, Union[float, str]]] = None, blur_sigma: float = 1.0, time_aware: bool = False,
                 time_bin: int = 10, flow_interpolation: str = "burgers", t0_flow_location: str = "middle", omit_boundary: bool = True,
                 exact_flow: bool = False, calib=None, flow_regularizer=None):
        """basis_or_model: a model name of utils.flow_utils.flow_basis ("translation", "similarity", "affine", "rotation" -- the
        last with calib = (fx, fy, cx, cy)), or a basis [K,2,H,W] (numpy array or tensor, float32 or float64, 1 <= K <= 64) on the
        handle's sensor; it is kept on the device in its dtype (model names: float64).
        The other arguments are PatchFlowObjective's.  There is no patch grid, hence no total_variation term and no `scale_later`.
        Numeric hybrid weights of fused costs run on the native plan; "inv" weights and costs without a fused kernel keep the
        autograd-chained path of `__call__` (no exact product there: TorchWrapper takes a difference quotient of the gradient).
        flow_regularizer: {"kind": "divergence" | "area", "weight", "eps", "s"} or None -- `set_flow_regularizer`."""
        self.handle = handle
        self.t_scale = float(t_scale)
        if isinstance(basis_or_model, str):
            basis_or_model = flow_basis(basis_or_model, handle.image_size, calib)
        basis = torch.as_tensor(basis_or_model)
        if basis.dtype not in (torch.float32, torch.float64):
            basis = basis.to(torch.float64)
        if basis.dim() != 4 or tuple(basis.shape[1:]) != (2,) + tuple(handle.image_size):
            raise ValueError(f"the basis must be [K, 2, {handle.image_size[0]}, {handle.image_size[1]}], got {tuple(basis.shape)}")
        if not 1 <= basis.shape[0] <= _lib.BASIS_MAX_K:
            raise ValueError(f"a flow basis has 1 .. {_lib.BASIS_MAX_K} fields, got {basis.shape[0]}")
        self.basis = basis.to(handle.device).contiguous()
        self._nx = int(basis.shape[0])
        # max |B_k|: sum_k |theta_k| bmax_k bounds the flow (time slabs), as it bounds a product's tangent inside the plan
        self.bmax = self.basis.abs().reshape(self._nx, -1).amax(dim=1).to(torch.float64).cpu().numpy()
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
            raise ValueError("total_variation acts on a patch grid: a flow basis has none")
        self.device = handle.device  # read by scipy_autograd.TorchWrapper
        self.auto_slabs = True
        self._plan = None
        self._build_native_plan()
        self.flow_reg = None
        if flow_regularizer is not None:
            self.set_flow_regularizer(flow_regularizer)

    # -- one-call native path (cmax_basis_plan_create + cmax_patch_plan_*, csrc/cmax_solver.hip) ----------------------
    def _descriptor(self):
        """cmax_basis_objective_t of this objective, or None where only the autograd-chained path exists."""
        from ..cmax import _CustomTerm

        terms = [(w, desc) for _, w, desc in self.contrast.terms]
        if not terms or len(terms) > 4 or any(isinstance(desc, _CustomTerm) or w == "inv" for w, desc in terms):
            return None
        d = _lib.CmaxBasisObjective()
        d.n_terms = len(terms)
        d.time_aware = int(self.time_aware)
        d.T = self.time_bin if self.time_aware else 0
        d.scheme = F.SCHEME_CODES.get(self.flow_interpolation, -1) if self.time_aware else 0
        if self.time_aware and (d.scheme < 0 or self.t0_flow_location not in ("first", "middle")):
            return None
        d.t0 = (self.time_bin // 2 if self.t0_flow_location == "middle" else 0) if self.time_aware else 0
        d.H, d.W = self.handle.image_size
        d.K = self._nx
        d.basis_dtype = F._code(self.basis)
        d.scale_later = 0
        d.t_scale = self.t_scale
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
            _lib.check(_lib.load().cmax_basis_plan_create(self.handle._h, ctypes.byref(d), self.basis.data_ptr(), F._stream(), ctypes.byref(plan)))
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
        """One more term, weight * functional.flow_regularizer(F), on the displacement field F = t_scale * basis_to_dense(theta): a model
        with a zoom (similarity, affine, a free basis) has a contrast optimum that is not the motion -- every event shrunk onto a point
        -- and this penalty on the divergence of the flow or on the change of area under the warp is the remedy (include/cmax_hip.h).
        A dictionary {"kind": "divergence" | "area", "weight", "eps", "s"}; None removes the term.  `weight` carries the sign of the
        cost direction (a minimised loss: positive).  As PatchFlowObjective.set_flow_regularizer."""
        desc = None if flow_regularizer is None else _lib.flow_regularizer_from_config(flow_regularizer)
        if self._plan is not None:
            _lib.check(_lib.load().cmax_patch_plan_set_flow_regularizer(self._plan, None if desc is None else ctypes.byref(desc)))
        self.flow_reg = desc

    def flow_field(self, theta: torch.Tensor) -> torch.Tensor:
        """[K] parameters -> the displacement field [2,H,W] over the batch, t_scale * basis_to_dense(theta): what the flow regulariser
        acts on."""
        return F.basis_to_dense(theta.reshape(-1), self.basis) * self.t_scale

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
        """The product exists on the native plan only: H_theta = t^2 B^T H_flow B, time-aware plans with the second-order adjoint
        of the voxel chain."""
        return self._plan is not None and self.contrast.has_exact_hvp

    def _theta(self, theta, what="theta") -> np.ndarray:
        theta = np.ascontiguousarray(theta, dtype=np.float64).reshape(-1)
        if theta.size != self._nx:
            raise ValueError(f"{what} has {theta.size} elements, the basis has {self._nx} fields")
        return theta

    def flow_bound(self, theta) -> float:
        """sum_k |theta_k| max|B_k| * |t_scale|: no pixel is displaced further over the batch."""
        t = theta.detach().abs().to(torch.float64).reshape(-1).cpu().numpy() if isinstance(theta, torch.Tensor) else np.abs(np.asarray(theta, dtype=np.float64)).reshape(-1)
        return float((t * self.bmax).sum()) * abs(self.t_scale)

    def ensure_time_slabs(self, theta) -> int:
        """Before an evaluation at `theta` the batch is put into the time-slab order its largest displacement asks for
        (CMaxHandle.auto_time_slabs), from the bound `flow_bound`.  Time-aware objectives keep their time bins."""
        if self.time_aware or not self.auto_slabs:
            return 0
        return self.handle.auto_time_slabs(self.flow_bound(theta))

    def value_and_grad_numpy(self, theta: np.ndarray, want_grad: bool = True):
        """theta [K] float64 (host) -> (loss, gradient [K] float64): one cmax_patch_plan_evaluate call."""
        theta = self._theta(theta)
        self.ensure_time_slabs(theta)
        loss = ctypes.c_double(0.0)
        grad = np.empty(self._nx, dtype=np.float64) if want_grad else None
        with torch.cuda.device(self.handle.device):
            _lib.check(_lib.load().cmax_patch_plan_evaluate(self._plan, theta.ctypes.data, 0, ctypes.byref(loss),
                                                            grad.ctypes.data if want_grad else None, F._stream()))
        return loss.value, grad

    def hvp_numpy(self, theta: np.ndarray, v: np.ndarray) -> np.ndarray:
        """Exact Hessian-vector product on host arrays: one cmax_patch_plan_hvp call."""
        theta, v = self._theta(theta), self._theta(v, "v")
        self.ensure_time_slabs(theta)
        hv = np.empty(self._nx, dtype=np.float64)
        with torch.cuda.device(self.handle.device):
            _lib.check(_lib.load().cmax_patch_plan_hvp(self._plan, theta.ctypes.data, v.ctypes.data, hv.ctypes.data, F._stream()))
        return hv

    def hvp(self, theta: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
        """`hvp_numpy` on tensors."""
        hv = self.hvp_numpy(theta.detach().cpu().numpy(), v.detach().cpu().numpy())
        return torch.as_tensor(hv, dtype=theta.dtype, device=theta.device).reshape(theta.shape)

    def descend(self, theta0: np.ndarray, method: str = "Adam", n_iter: int = 100, lr: float = 0.05, lr_step: Optional[int] = None,
                lr_decay: float = 0.1, momentum: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8, trace: bool = False):
        """n_iter iterations of torch.optim.SGD / Adam with StepLR(lr_step, lr_decay) from theta0 in ONE cmax_patch_plan_descend call
        (PatchFlowObjective.descend): the iterate and the optimiser's state stay in device memory, one wait at the end.  Time slabs are
        decided ONCE, from the bound at |theta0| + lr * n_iter per entry (Adam moves an entry by about lr per step at most; SGD's steps
        have no such bound: its slabs follow theta0 alone)."""
        if self._plan is None:
            raise NotImplementedError("descend needs the native plan (numeric hybrid weights, fused costs)")
        theta0 = self._theta(theta0, "theta0")
        descent = _lib.descent_descriptor(method, n_iter, lr, lr_step, lr_decay, momentum, betas, eps)
        self.ensure_time_slabs(np.abs(theta0) + (float(lr) * int(n_iter) if method == "Adam" else 0.0))
        fn, plan, stream = _lib.load().cmax_patch_plan_descend, self._plan, F._stream()
        with torch.cuda.device(self.handle.device):
            return _lib.run_descent(lambda o, res, xl, xb, hist, tr: fn(plan, theta0.ctypes.data, 0, o, res, xl, xb, hist, tr, stream),
                                    self._nx, descent, trace)

    def minimize_lbfgs(self, theta0: np.ndarray, n_eval: int = 32, history: int = 8, gtol: float = 1e-5, max_move: float = 10.0, max_ls: int = 10,
                       c1: float = 1e-4, shrink: float = 0.5, curv_eps: float = 1e-10, step0: float = 1.0, trace: bool = False):
        """L-BFGS with a backtracking line search from theta0 in ONE cmax_patch_plan_lbfgs call (PatchFlowObjective.minimize_lbfgs; the
        rules: include/cmax_hip.h).  Every parameter stays within max_move of theta0: time slabs are decided ONCE, from the bound at
        |theta0| + max_move per entry.  Returns a _lib.LbfgsResult."""
        if self._plan is None:
            raise NotImplementedError("minimize_lbfgs needs the native plan (numeric hybrid weights, fused costs)")
        theta0 = self._theta(theta0, "theta0")
        lbfgs = _lib.lbfgs_descriptor(n_eval, history, max_ls, c1, shrink, curv_eps, gtol, step0, max_move)
        self.ensure_time_slabs(np.abs(theta0) + abs(float(max_move)))
        fn, plan, stream = _lib.load().cmax_patch_plan_lbfgs, self._plan, F._stream()
        with torch.cuda.device(self.handle.device):
            return _lib.run_lbfgs(lambda o, res, x, hist, al, code, tr: fn(plan, theta0.ctypes.data, 0, o, res, x, hist, al, code, tr, stream),
                                  self._nx, lbfgs, trace)

    def dense_flow(self, theta: torch.Tensor) -> torch.Tensor:
        """[K] parameters -> [2,H,W] (or [T,2,H,W]) flow in pixel per NORMALISED time, in the basis' dtype."""
        if theta.numel() != self._nx:
            raise ValueError(f"theta has {theta.numel()} elements, the basis has {self._nx} fields")
        dense = F.basis_to_dense(theta.reshape(-1), self.basis) * self.t_scale
        if self.time_aware:  # the voxel is built on the displacement field, as in PatchFlowObjective.dense_flow
            dense = F.construct_dense_flow_voxel(dense, self.time_bin, self.flow_interpolation, self.t0_flow_location)
        return dense

    def __call__(self, theta: torch.Tensor) -> torch.Tensor:
        """The autograd-chained path: basis_to_dense -> ContrastObjective, one Python-level call per stage."""
        theta = theta.to(self.handle.device)
        self.ensure_time_slabs(theta)
        loss = self.contrast(self.dense_flow(theta))
        if self.flow_reg is not None:
            r = self.flow_reg
            loss = loss + r.weight * F.flow_regularizer(self.flow_field(theta), r.kind, r.eps, r.s)
        return loss
