"""Child process of tests/test_gpu_nearest_filter.py: a nearest-filter plan created with CMAX_PLAN_GRAPHS=1 in the environment (the
plan reads it once, at creation), evaluated often enough to capture and replay its launch sequences.
    python tests/_nearest_plan_worker.py <case id>   -> one JSON line: per call loss, gradient, product; the plan's graph count."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import _nearest_cases as N  # noqa: E402


def main(cid):
    assert os.environ.get("CMAX_PLAN_GRAPHS") == "1"
    b = N.built(cid)
    h, obj = N.make_objective(b["ev"], b["spec"], b["exact_flow"], "nearest")
    calls = []
    for _ in range(6):  # a plan replays from its fourth call on
        loss, grad = obj.value_and_grad_numpy(b["x"])
        hv = obj.hvp_numpy(b["x"], b["v"])
        calls.append({"loss": loss, "grad": grad.tolist(), "hv": hv.tolist()})
    n_graphs, enabled = obj.native_plan_info()
    del obj
    h.close()
    print(json.dumps({"calls": calls, "n_graphs": n_graphs, "enabled": enabled}))


if __name__ == "__main__":
    main(sys.argv[1])
