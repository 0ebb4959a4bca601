"""Child program of tests/test_gpu_hvp_parity.py::test_forced_segment_layouts_against_the_references.

The segment layout switches (CMAX_BIG_SEG, CMAX_MID_SEG, CMAX_COMPACT) are read once per process, so a forced layout needs a process
of its own.  usage: _layout_worker.py <big | mid> <out.npz>, with the switches in the environment.  For every case of the layout
(tests/_hvp_cases.py) it builds the handle, asserts the segment size the layout stands for, and writes loss, gradient, IWE of
reference time 0 and the exact Hessian-vector product; the parent compares them with the references."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import event_based_optical_flow_amd as E  # noqa: E402

import _hvp_cases as C  # noqa: E402


def main(layout, out_path):
    out = {}
    for c in C.LAYOUT_CASES[layout]:
        b = C.inputs(c)
        h = E.CMaxHandle(c["size"], c["pad"]).set_events(b["ev"], time_bin=c["T"], on_dropped="ignore")
        info = h.work_list_info()
        assert info["segment_events"] == C.LAYOUT_SEGMENT_EVENTS[layout], (c["id"], info)
        desc = E.make_descriptor(c["cost"], c["model"], sigma=float(c["sigma"]), time_bin=c["T"], warp_direction=c["warp_direction"])
        res, grad = h.evaluate(desc, b["motion"])
        k = c["id"]
        out[k + "/loss"] = res[0].item()
        out[k + "/grad"] = grad.double().cpu().numpy()
        out[k + "/iwe"] = h.last_iwe(0).double().cpu().numpy()
        out[k + "/hv"] = h.hvp(desc, b["motion"], b["v"]).double().cpu().numpy()
        out[k + "/segments"], out[k + "/segment_events"] = info["segments"], info["segment_events"]
        h.close()
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
