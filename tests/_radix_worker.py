"""Child program of tests/test_gpu_radix_sort.py and tests/test_gpu_counting_sort.py.

CMAX_SORT, CMAX_RS_BITS and CMAX_NO_RUN_SORT are read once per process, so the radix pipeline on small batches, a digit width of its
own, and the counting sort without its run sort each need a process of their own.
usage: _radix_worker.py <out.npz> [<table module> [NAME=VALUE | NAME= ...]]
The table module (default _sort_cases) gives CASES, batch, weights and motion; NAME=VALUE is what the environment must hold, NAME= what
it must NOT hold (default CMAX_SORT=radix, with CMAX_RS_BITS as the parent chose).  For every case of the table it builds the handle,
applies the case's steps, and writes after every step the packed events with their group starts, batch_info, work_list_info and the
evaluations the case asks for; the parent does all the comparing."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import event_based_optical_flow_amd as E  # noqa: E402

C = importlib.import_module(sys.argv[2] if len(sys.argv) > 2 else "_sort_cases")
EXPECTED_ENV = [a.split("=", 1) for a in sys.argv[3:]] if len(sys.argv) > 3 else [["CMAX_SORT", "radix"]]


def record(out, key, h, c, evals):
    packed, gs = h.packed_events()
    info, wl = h.batch_info(), h.work_list_info()
    assert packed.shape[0] == info["packed"] == h.n_events and gs[-1] == info["packed"], (key, info)
    out[key + "/packed"], out[key + "/gs"] = packed, gs
    out[key + "/info"] = np.array([info["packed"], info["dropped"], int(info["fractional"]), info["outside"]], np.int64)
    out[key + "/work_list"] = np.array([wl["segments"], wl["segment_events"]], np.int64)
    for e in evals:
        desc = E.make_descriptor(e["cost"], e["model"], sigma=float(e["sigma"]), time_bin=e["T"])
        m = C.motion(c, e)
        k = f"{key}/{e['tag']}"
        if e["weight_grad"]:
            res, grad, gw = h.evaluate_weight_grad(desc, m)
            out[k + "/grad_w"] = gw.double().cpu().numpy()
        else:
            res, grad = h.evaluate(desc, m)
        out[k + "/loss"] = res[0].item()
        out[k + "/grad"] = grad.double().cpu().numpy()
        if e["model"] == "2d-translation":
            out[k + "/iwe"] = h.last_iwe(0).double().cpu().numpy()


def main(out_path):
    for name, value in EXPECTED_ENV:
        assert os.environ.get(name) == (value if value else None), (name, os.environ.get(name), value)
    out = {}
    for c in C.CASES:
        ev = C.batch(c)
        h = E.CMaxHandle(c["size"], c["pad"]).set_keep_outside(c["keep_outside"])
        tmin, tmax = c["extremes"] if c["extremes"] else (None, None)
        h.set_events(ev, tmin=tmin, tmax=tmax, time_bin=c["T"], on_dropped="ignore", weights=C.weights(c))
        record(out, f"{c['id']}/0", h, c, c["evals"].get(0, []))
        for s, (what, k) in enumerate(c["steps"], start=1):
            if what == "bins":
                h.set_time_bins(k)
            else:
                h.set_time_slabs(k)
            record(out, f"{c['id']}/{s}", h, c, c["evals"].get(s, []))
        h.close()
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
