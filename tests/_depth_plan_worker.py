"""Child process of tests/test_gpu_depth_plan.py: a depth plan created with CMAX_PLAN_GRAPHS=1 in the environment (the plan reads it once,
at creation), evaluated often enough to capture and replay its launch sequences.  No reference is computed here.
    python tests/_depth_plan_worker.py <case id>   -> one JSON line: per call loss, gradient, product; the plan's graph count."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import _depth_cases as D  # noqa: E402
import _depth_gpu as G  # noqa: E402


def main(cid):
    assert os.environ.get("CMAX_PLAN_GRAPHS") == "1"
    c = D.PLAN[cid]
    ev, x, spec = D.inputs(c)
    v = D.hvp_tangents(c, x, spec)["random"]
    h, obj = G.make_objective(ev, spec, exact=c["exact"], basis_dtype=c["basis_dtype"])
    calls = []
    for _ in range(6):  # a plan replays from its fourth call on
        loss, grad = obj.value_and_grad_numpy(x)
        hv = obj.hvp_numpy(x, v)
        calls.append({"loss": loss, "grad": np.asarray(grad).tolist(), "hv": np.asarray(hv).tolist()})
    n_graphs, enabled = obj.native_plan_info()
    del obj
    h.close()
    print(json.dumps({"calls": calls, "n_graphs": n_graphs, "enabled": enabled}))


if __name__ == "__main__":
    main(sys.argv[1])
