"""Child process of tests/test_gpu_basis_plan.py: a flow-basis plan created with CMAX_PLAN_GRAPHS=1 in the environment (the plan
reads it once, at creation), evaluated often enough to capture and replay its launch sequences.  No reference is computed here.
    python tests/_basis_plan_worker.py <case id>   -> one JSON line: per call loss, gradient, product; the plan's graph count."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import _basis_cases as B  # noqa: E402
import _basis_gpu as G  # noqa: E402


def main(cid):
    assert os.environ.get("CMAX_PLAN_GRAPHS") == "1"
    c = B.PLAN[cid]
    ev, theta, spec = B.inputs(c)
    v = B.hvp_tangents(c, theta)["random"]
    h, obj = G.make_objective(c, ev, spec)
    calls = []
    for _ in range(6):  # a plan replays from its fourth call on
        loss, grad = obj.value_and_grad_numpy(theta)
        hv = obj.hvp_numpy(theta, v)
        calls.append({"loss": loss, "grad": np.asarray(grad).tolist(), "hv": np.asarray(hv).tolist()})
    n_graphs, enabled = obj.native_plan_info()
    del obj
    h.close()
    print(json.dumps({"calls": calls, "n_graphs": n_graphs, "enabled": enabled}))


if __name__ == "__main__":
    main(sys.argv[1])
