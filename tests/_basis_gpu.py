"""Construction of a FlowBasisObjective from a row of tests/_basis_cases.py, shared by tests/test_gpu_basis_plan.py and its child
process tests/_basis_plan_worker.py."""
import numpy as np

import event_based_optical_flow_amd as E
from event_based_optical_flow_amd.solver import FlowBasisObjective


def make_objective(c, ev, spec, deterministic=False):
    h = E.CMaxHandle(spec["size"])
    if deterministic:
        h.set_deterministic(True)
    h.set_events(ev, time_bin=spec["T"] if spec["time_aware"] else 0)
    names = {name: w for name, w in spec["terms"]}
    hybrid = len(names) > 1
    basis = np.ascontiguousarray(spec["basis"], dtype=np.float32 if c["basis_dtype"] == "float32" else np.float64)
    obj = FlowBasisObjective(h, spec["t_scale"], basis, cost="hybrid" if hybrid else next(iter(names)), cost_with_weight=names if hybrid else None,
                             blur_sigma=spec["sigma"], time_aware=spec["time_aware"], time_bin=spec["T"], flow_interpolation=spec["scheme"],
                             t0_flow_location=spec["t0"], omit_boundary=spec["omit"], exact_flow=c["exact"])
    assert obj.has_native_plan and obj.has_exact_hvp
    return h, obj
