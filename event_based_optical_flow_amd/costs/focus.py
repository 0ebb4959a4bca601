"""Focus losses beyond the reference's seven costs (Gallego, Gehrig, Scaramuzza, "Focus is all you need", CVPR 2019):
mean square, Laplacian magnitude and Hessian magnitude of the IWE -- quadratic forms with 3 x 3 support (include/cmax_hip.h,
CMAX_COST_MEAN_SQUARE / _LAPLACIAN / _HESSIAN) -- each plain, normalised and multi-focal normalised, like the gradient-magnitude trio.

They live in a registry of their own, `focus_functions`: `costs.functions` is the reference's set of names, built by walking
CostBase's subclasses at import, so this module is imported AFTER that walk.  HybridCost looks a name up in `functions` first,
then here."""
import logging

from .. import _lib
from .base import CostBase
from ._contrast import raw_contrast

logger = logging.getLogger(__name__)

_KINDS = {
    "mean_square": _lib.COST_MEAN_SQUARE,
    "laplacian_magnitude": _lib.COST_LAPLACIAN,
    "hessian_magnitude": _lib.COST_HESSIAN,
}


def _make_trio(kind: str, code: int):
    """The three CostBase subclasses of one focus loss: plain, normalized_*, multi_focal_normalized_*."""

    class Plain(CostBase):
        name = kind
        required_keys = ["iwe", "omit_boundary"]

        def __init__(self, direction="minimize", store_history: bool = False, cuda_available=False, precision="32", *args, **kwargs):
            super().__init__(direction=direction, store_history=store_history)
            self.precision = precision

        def calculate(self, arg: dict):
            mag = self.magnitude(arg["iwe"], arg["omit_boundary"])
            return -mag if self.direction == "minimize" else mag

        def magnitude(self, iwe, omit_boundary):
            mag = raw_contrast(iwe, code, omit_boundary)
            if self.precision == "64" and hasattr(mag, "double"):
                mag = mag.double()
            return mag

    class Normalized(CostBase):
        name = "normalized_" + kind
        required_keys = ["orig_iwe", "iwe", "omit_boundary"]

        def __init__(self, direction="minimize", store_history: bool = False, cuda_available=False, precision="32", *args, **kwargs):
            super().__init__(direction=direction, store_history=store_history)
            self.plain = Plain(direction=direction, store_history=store_history, cuda_available=cuda_available, precision=precision)

        def calculate(self, arg: dict):
            return self.ratio(arg["iwe"], arg["orig_iwe"], arg["omit_boundary"])

        def ratio(self, iwe, orig_iwe, omit_boundary):
            m_iwe = self.plain.magnitude(iwe, omit_boundary)
            m_orig = self.plain.magnitude(orig_iwe, omit_boundary)  # cropped like the warped image (the gradient-magnitude rule)
            if self.direction == "minimize":
                return m_orig / m_iwe
            logger.warning("The loss is specified as maximize direction")
            return m_iwe / m_orig

    class MultiFocalNormalized(CostBase):
        name = "multi_focal_normalized_" + kind
        required_keys = ["forward_iwe", "backward_iwe", "middle_iwe", "omit_boundary", "orig_iwe"]

        def __init__(self, direction="minimize", store_history: bool = False, cuda_available=False, precision="32", *args, **kwargs):
            super().__init__(direction=direction, store_history=store_history)
            self.normalized = Normalized(direction=direction, cuda_available=cuda_available, precision=precision)

        def calculate(self, arg: dict):
            orig, omit = arg["orig_iwe"], arg["omit_boundary"]
            loss = self.normalized.ratio(arg["forward_iwe"], orig, omit) + self.normalized.ratio(arg["backward_iwe"], orig, omit)
            if arg.get("middle_iwe", None) is not None:
                loss = loss + self.normalized.ratio(arg["middle_iwe"], orig, omit) * 2
            if self.direction in ["minimize", "natural"]:
                return loss
            logger.warning("The loss is specified as maximize direction")
            return -loss

    camel = "".join(w.capitalize() for w in kind.split("_"))
    for cls, prefix in ((Plain, ""), (Normalized, "Normalized"), (MultiFocalNormalized, "MultiFocalNormalized")):
        cls.__name__ = cls.__qualname__ = prefix + camel
    return Plain, Normalized, MultiFocalNormalized


focus_functions = {cls.name: cls for kind, code in _KINDS.items() for cls in _make_trio(kind, code)}
