"""Child program of tests/test_gpu_iwe_layer.py::test_forced_segment_layouts.

The segment layout switches (CMAX_BIG_SEG, CMAX_MID_SEG, CMAX_COMPACT) are read once per process, so a forced layout needs a process
of its own.  usage: _iwe_layer_worker.py <big | mid> <out.npz>, with the switches in the environment.  For every case of the layout
(tests/_iwe_cases.py) it builds the handle, asserts the segment size the layout stands for, and writes the layer's images, VJP (motion
and weights), JVP and vjp_tan -- unweighted, and for the first case also with the `uniform` weights; the parent compares them with
tests/_iwe_ref.py."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import event_based_optical_flow_amd as E  # noqa: E402

import _hvp_cases as C  # noqa: E402
import _iwe_cases as IC  # noqa: E402


def weight_names(i):
    return ("none", "uniform") if i == 0 else ("none",)


def main(layout, out_path):
    out = {}
    for i, c in enumerate(IC.LAYOUT_CASES[layout]):
        b = C.inputs(c)
        cfg = IC.layer_config(c)
        h = E.CMaxHandle(c["size"], c["pad"]).set_events(b["ev"], time_bin=c["T"], on_dropped="ignore")
        info = h.work_list_info()
        assert info["segment_events"] == C.LAYOUT_SEGMENT_EVENTS[layout], (c["id"], info)
        for wname in weight_names(i):
            w = IC.weights(wname, b["ev"])
            h.set_event_weights(w)
            k = f"{c['id']}/{wname}"
            imgs = h.iwes(b["motion"], **cfg)
            cot = IC.cotangents(c, tuple(imgs.shape))
            gm, gw = h.iwes_vjp(b["motion"], gimages=cot["G"], want_grad_w=True, **cfg)
            out[k + "/images"] = imgs.double().cpu().numpy()
            out[k + "/gm"], out[k + "/gw"] = gm.double().cpu().numpy(), gw.double().cpu().numpy()
            out[k + "/jv"] = h.iwes_jvp(b["motion"], tangent=b["v"], **cfg).double().cpu().numpy()
            out[k + "/vt"] = h.iwes_vjp_tan(b["motion"], tangent=b["v"], gimages=cot["G"], gimages_tan=cot["Gp"], **cfg).double().cpu().numpy()
        out[c["id"] + "/segments"], out[c["id"] + "/segment_events"] = info["segments"], info["segment_events"]
        h.close()
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
