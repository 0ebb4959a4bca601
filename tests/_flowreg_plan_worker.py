"""Child process of tests/test_gpu_flow_regularizer.py: a basis plan created with CMAX_PLAN_GRAPHS=1 in the environment (the plan reads it
once, at creation) that carries the flow regulariser, evaluated often enough to capture and replay its launch sequences; then the term
is removed -- which must drop the captured sequences -- and the plain plan replayed likewise.  No reference is computed here.
    python tests/_flowreg_plan_worker.py <plan id>   -> one JSON line: per call loss, gradient, product; the plan's graph counts."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import _basis_cases as B  # noqa: E402
import _basis_gpu as G  # noqa: E402
import _flowreg_cases as K  # noqa: E402


def main(pid):
    assert os.environ.get("CMAX_PLAN_GRAPHS") == "1"
    _, row, reg = next(p for p in K.BASIS_PLANS if p[0] == pid)
    c = B.HVP[row]
    ev, theta, spec, _ = B.hvp_inputs(c)
    v = B.hvp_tangents(c, theta)["random"]
    h, obj = G.make_objective(c, ev, spec)
    obj.set_flow_regularizer(K.REGS[reg])
    calls, plain = [], []
    for _ in range(6):  # a plan replays from its fourth call on
        loss, grad = obj.value_and_grad_numpy(theta)
        hv = obj.hvp_numpy(theta, v)
        calls.append({"loss": loss, "grad": np.asarray(grad).tolist(), "hv": np.asarray(hv).tolist()})
    n_graphs, enabled = obj.native_plan_info()
    obj.set_flow_regularizer(None)
    n_after = obj.native_plan_info()[0]
    for _ in range(6):
        loss, grad = obj.value_and_grad_numpy(theta)
        obj.hvp_numpy(theta, v)
        plain.append({"loss": loss, "grad": np.asarray(grad).tolist()})
    n_plain = obj.native_plan_info()[0]
    del obj
    h.close()
    print(json.dumps({"calls": calls, "plain": plain, "n_graphs": n_graphs, "enabled": enabled, "n_graphs_after_removal": n_after, "n_graphs_plain": n_plain}))


if __name__ == "__main__":
    main(sys.argv[1])
