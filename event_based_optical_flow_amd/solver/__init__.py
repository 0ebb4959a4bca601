"""Optimiser-side boundary of the path: `scipy_autograd.minimize`, the GPU objectives for patch-based flow and for flow bases
(motion models linear in their parameters), for depth and ego-motion (the motion field over a grid of inverse depth) and the solver classes of the reference's registry built on it."""
from . import scipy_autograd
from .basis_objective import FlowBasisObjective
from .depth_objective import DepthEgoMotionObjective
from .mixed import MixedPatchContrastMaximization, TimeAwarePatchContrastMaximization
from .patch_objective import PatchFlowObjective, patch_pad
from .pyramid import PyramidalPatchContrastMaximization

# registry names of the reference (src/solver/__init__.py:14-19); MixedPatchContrastMaximization is importable but, as there, not registered
collections = {
    "pyramidal_patch_contrast_maximization": PyramidalPatchContrastMaximization,
    "time_aware_mixed_patch_contrast_maximization": TimeAwarePatchContrastMaximization,
}

__all__ = ["scipy_autograd", "FlowBasisObjective", "DepthEgoMotionObjective", "PatchFlowObjective", "patch_pad", "PyramidalPatchContrastMaximization",
           "MixedPatchContrastMaximization", "TimeAwarePatchContrastMaximization", "collections"]
