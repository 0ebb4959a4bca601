"""Construction of a DepthEgoMotionObjective from a spec of tests/_depth_cases.py, shared by tests/test_gpu_depth_plan.py and its child
process tests/_depth_plan_worker.py."""
import numpy as np

import event_based_optical_flow_amd as E
from event_based_optical_flow_amd.solver import DepthEgoMotionObjective


def make_objective(ev, spec, deterministic=False, exact=False, basis_dtype="float64", **more):
    h = E.CMaxHandle(spec["size"])
    if deterministic:
        h.set_deterministic(True)
    h.set_events(ev, time_bin=spec["T"] if spec["time_aware"] else 0)
    names = {name: w for name, w in spec["terms"]}
    hybrid = len(names) > 1
    dtype = np.float32 if basis_dtype == "float32" else np.float64
    bases = (np.ascontiguousarray(spec["A"], dtype=dtype), np.ascontiguousarray(spec["B"], dtype=dtype))
    # patch_size = sliding_window and a shift of (pad - 1) windows: the padding patch_pad returns is the spec's (tests/test_gpu_lbfgs.py)
    shift = tuple(max(spec["pad"][k] - 1, 0) * spec["sw"][k] for k in (0, 1))
    obj = DepthEgoMotionObjective(h, spec["t_scale"], spec["patch_image_size"], spec["sw"], spec["sw"], shift, bases=bases,
                                  cost="hybrid" if hybrid else next(iter(names)), cost_with_weight=names if hybrid else None, blur_sigma=spec["sigma"],
                                  time_aware=spec["time_aware"], time_bin=spec["T"], flow_interpolation=spec["scheme"], t0_flow_location=spec["t0"],
                                  omit_boundary=spec["omit"], exact_flow=exact, **more)
    assert obj.pad == tuple(spec["pad"]) and obj.has_native_plan and obj.has_exact_hvp
    return h, obj
