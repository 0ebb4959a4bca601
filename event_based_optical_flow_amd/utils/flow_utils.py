"""Flow helpers on the boundary.  `construct_dense_flow_voxel_torch` mirrors the reference's
function of the same name (src/utils/flow_utils.py:99-161) over the HIP kernels."""
from typing import Optional

import numpy as np
import torch

from .. import functional as F
from ..array_types import to_device_tensor


def generate_dense_optical_flow(image_size: tuple, max_val: float = 30, seed: Optional[int] = None) -> np.ndarray:
    """[2,H,W] flow ~ U(-max_val, max_val) (distribution of src/utils/flow_utils.py:20-30)."""
    return np.random.default_rng(seed).uniform(-max_val, max_val, (2,) + tuple(image_size))


def generate_smooth_flow(image_size: tuple, max_val: float = 20, grid: int = 16, seed: Optional[int] = None) -> np.ndarray:
    """Bilinear upsampling of a coarse grid x grid U(-max_val, max_val) field: the kind of flow the
    patch solver produces."""
    H, W = image_size
    g = np.random.default_rng(seed).uniform(-max_val, max_val, (2, grid, grid))
    ri = np.linspace(0, grid - 1, H)
    ci = np.linspace(0, grid - 1, W)
    r0 = np.clip(np.floor(ri).astype(int), 0, grid - 2)
    c0 = np.clip(np.floor(ci).astype(int), 0, grid - 2)
    fr = (ri - r0)[None, :, None]
    fc = (ci - c0)[None, None, :]
    g00 = g[:, r0][:, :, c0]
    g10 = g[:, r0 + 1][:, :, c0]
    g01 = g[:, r0][:, :, c0 + 1]
    g11 = g[:, r0 + 1][:, :, c0 + 1]
    return (1 - fr) * (1 - fc) * g00 + fr * (1 - fc) * g10 + (1 - fr) * fc * g01 + fr * fc * g11


FLOW_BASIS_MODELS = {"translation": 2, "similarity": 4, "affine": 6, "rotation": 3}


def flow_basis(model: str, image_size: tuple, calib=None) -> np.ndarray:
    """[K,2,H,W] float64 basis of a motion model that is linear in its parameters: the dense flow is D = sum_k theta_k B_k
    (functional.basis_to_dense, solver.FlowBasisObjective).  The reference has no such models; D is warped by its dense-flow rule
    x' = x - dt * D[src] (src/warp.py:263-313), so with u(x) = sum_k theta_k u_k(x) the velocity an event at x is moved with,
    x' = x + dt u(x), every field is B_k = -u_k.  Rows first, like every flow here: component 0 acts on the row coordinate.
    r = i - (H - 1) / 2 and c = j - (W - 1) / 2 are the coordinates of pixel (i, j) from the sensor's centre.
      "translation" (2)  u = (theta_0, theta_1): theta is the theta of the "2d-translation" warp, x' = x + dt theta, hence B = -1
      "similarity"  (4)  u = (theta_0, theta_1) + theta_2 (r, c) + theta_3 (-c, r): translation, zoom, in-plane rotation
      "affine"      (6)  u = (theta_0 + theta_2 r + theta_3 c,  theta_1 + theta_4 r + theta_5 c)
      "rotation"    (3)  calib = (fx, fy, cx, cy) in pixels, fx / cx along the columns, fy / cy along the rows.  The motion field of a
                         static scene under the camera's angular velocity theta = (w_x, w_y, w_z) (x along the columns, y along the
                         rows, z the optical axis), with x = (j - cx) / fx, y = (i - cy) / fy:
                           u_col = fx (x y w_x - (1 + x^2) w_y + y w_z),   u_row = fy ((1 + y^2) w_x - x y w_y - x w_z)"""
    if model not in FLOW_BASIS_MODELS:
        raise ValueError(f"flow_basis model {model!r}: one of {sorted(FLOW_BASIS_MODELS)}")
    H, W = int(image_size[0]), int(image_size[1])
    i, j = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    r, c = i - (H - 1) / 2.0, j - (W - 1) / 2.0
    one, zero = np.ones((H, W)), np.zeros((H, W))
    if model == "rotation":
        if calib is None or len(calib) != 4:
            raise ValueError("flow_basis('rotation') needs calib = (fx, fy, cx, cy)")
        fx, fy, cx, cy = (float(v) for v in calib)
        x, y = (j - cx) / fx, (i - cy) / fy
        u = [(fy * (1.0 + y * y), fx * x * y), (-fy * x * y, -fx * (1.0 + x * x)), (-fy * x, fx * y)]  # (u_row, u_col) per w_x, w_y, w_z
    else:
        u = [(one, zero), (zero, one)]
        if model == "similarity":
            u += [(r, c), (-c, r)]
        elif model == "affine":
            u += [(r, zero), (c, zero), (zero, r), (zero, c)]
    return np.ascontiguousarray(0.0 - np.stack([np.stack(f) for f in u]))  # (0.0 - x: no negative zeros)


def motion_field_basis(image_size: tuple, calib) -> tuple:
    """(A [3,2,H,W], B [3,2,H,W]) float64: the motion field of a static scene seen by a calibrated camera that moves, split into the part
    that scales with inverse depth and the part that does not (functional.depth_to_dense, solver.DepthEgoMotionObjective):
        u(x) = rho(x) * sum_k v_k a_k(x) + sum_j w_j b_j(x),   v = (v_x, v_y, v_z) the linear, w the angular velocity.
    calib = (fx, fy, cx, cy) and every convention of `flow_basis("rotation")`: rows first, x = (j - cx) / fx, y = (i - cy) / fy, the
    fields stored as -u (the dense-flow rule is x' = x - dt D[src]).  B IS flow_basis("rotation", image_size, calib); A is the
    translational field per unit inverse depth,
        u_col = fx (-v_x + x v_z),   u_row = fy (-v_y + y v_z)."""
    if calib is None or len(calib) != 4:
        raise ValueError("motion_field_basis needs calib = (fx, fy, cx, cy)")
    H, W = int(image_size[0]), int(image_size[1])
    fx, fy, cx, cy = (float(v) for v in calib)
    i, j = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    x, y = (j - cx) / fx, (i - cy) / fy
    zero = np.zeros((H, W))
    u = [(zero, zero - fx), (zero - fy, zero), (fy * y, fx * x)]  # (u_row, u_col) per v_x, v_y, v_z
    A = np.ascontiguousarray(0.0 - np.stack([np.stack(f) for f in u]))
    return A, flow_basis("rotation", image_size, calib)


def construct_dense_flow_voxel_torch(dense_flow: torch.Tensor, time_bin: int, scheme: str = "upwind",
                                     t0_location: str = "middle", clamp: Optional[int] = None) -> torch.Tensor:
    """[(b,) 2,H,W] flow at t0 -> [(b,) time_bin, 2, H, W] voxel, differentiable.

    Schemes "burgers" and "upwind" (the two the shipped configs can select).  The reference's other schemes ("bilinear", "max",
    "same") are not a gap: its construct_dense_flow_voxel_* hands a 4-D array to propagate_flow_to_voxel_*, which unpacks three
    dimensions -- the call raises ValueError in the reference itself."""
    t = to_device_tensor(dense_flow, "dense_flow")
    if t.dim() == 4:
        v = torch.stack([F.construct_dense_flow_voxel(t[i], time_bin, scheme, t0_location) for i in range(t.shape[0])])
    else:
        v = F.construct_dense_flow_voxel(t, time_bin, scheme, t0_location)
    if clamp is not None:
        v = torch.clamp(v, -clamp, clamp)
    return v if v.device == dense_flow.device else v.to(dense_flow.device)
