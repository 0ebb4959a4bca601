"""Child program of tests/test_gpu_focus_costs.py::test_separate_launches_in_a_child_process.

CMAX_NO_FUSED_FOCUS is read once per process (eval_plan of csrc/cmax_fused.hip), so the separate k_stats + k_gimage launches need a
process of their own.  usage: _focus_worker.py <out.npz>, with the switch in the environment.  Writes loss and gradient of every case of
tests/_focus_cases.py, and the launches per kernel class of the first one; the parent compares them with the reference."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import _focus_cases as C  # noqa: E402


def launches(c, ev, motion):
    """{kernel class: launches} of one evaluation on a fresh handle with the launch brackets on"""
    h, desc = C.handle(c, ev), C.descriptor(c)
    h.set_profiling(True)
    h.evaluate(desc, motion)
    torch.cuda.synchronize()
    counts = {k: int(v[1]) for k, v in h.read_profile().items()}
    h.set_profiling(False)
    h.close()
    return counts


def main(out_path):
    assert os.environ.get("CMAX_NO_FUSED_FOCUS") == "1"
    out = {}
    for c in C.CASES:
        b = C.inputs(c)
        h, desc = C.handle(c, b["ev"]), C.descriptor(c)
        res, grad = h.evaluate(desc, b["motion"])
        out[c["id"] + "/loss"], out[c["id"] + "/grad"] = res[0].item(), grad.double().cpu().numpy()
        h.close()
    c = C.CASES[0]
    b = C.inputs(c)
    for k, v in launches(c, b["ev"], b["motion"]).items():
        out["profile/" + k] = v
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
