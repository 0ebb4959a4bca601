"""Child program of tests/test_gpu_work_list.py, and the recorder its parent uses in its own process.

CMAX_BIG_SEG, CMAX_MID_SEG, CMAX_NO_OWNED, CMAX_SMALL_ACC and CMAX_COMPACT are read once per process, so every forced layout needs a
process of its own.
usage: _worklist_worker.py <out.npz> <child index of _worklist_cases.CHILD_ENV>
For every case of the child's table it builds the handle, applies the case's steps and writes after every step what the library holds:
the packed events with their group starts, the work list read-back (segments, flag word, seg_max), work_list_info and batch_info, the
compact regions with the packing flag (or the error code of a handle without a compact copy) and the evaluations the case asks for.
The parent does all the comparing."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import event_based_optical_flow_amd as E  # noqa: E402
from event_based_optical_flow_amd._lib import CmaxError  # noqa: E402

import _worklist_cases as C  # noqa: E402


def record(out, key, h, c, evals):
    packed, gs = h.packed_events()
    segs, flags, seg_max = h.work_list()
    info, wl = h.batch_info(), h.work_list_info()
    out[key + "/packed"], out[key + "/gs"], out[key + "/segs"] = packed, gs, segs
    out[key + "/flags"] = np.array([int(flags[name]) for name in h.WORK_LIST_FLAGS], np.int64)
    out[key + "/seg_max"] = np.int64(seg_max)
    out[key + "/info"] = np.array([info["packed"], int(info["owned_groups"]), wl["segments"], wl["segment_events"], int(wl["small_accumulators"]), h.n_events], np.int64)
    try:
        regions, bad = h.compact_events()
        out[key + "/compact"], out[key + "/compact_flag"] = regions, np.int64(bad)
    except CmaxError as e:
        out[key + "/compact_error"] = np.int64(e.code)
    for model in evals:
        name = {"2dof": "2d-translation", "dense": "dense-flow", "voxel": "dense-flow-voxel"}[model]
        desc = E.make_descriptor("image_variance", name, time_bin=c["T"] if model == "voxel" else 0)
        res, grad = h.evaluate(desc, C.motion(c, model))
        out[f"{key}/{model}/loss"] = res[0].item()
        out[f"{key}/{model}/grad"] = grad.double().cpu().numpy()


def run_case(out, prefix, c):
    h = E.CMaxHandle(c["size"]).set_events(np.array(C.batch(c)), tmin=0.0, tmax=1.0, time_bin=c["T"], on_dropped="ignore")
    record(out, f"{prefix}{c['id']}/0", h, c, c["evals"])
    for s, (what, k) in enumerate(c["steps"], start=1):
        if what == "bins":
            h.set_time_bins(k)
        elif what == "slabs":
            h.set_time_slabs(k)
        else:
            h.set_events(np.array(C.batch(C.BY_ID[k])), tmin=0.0, tmax=1.0, on_dropped="ignore")
        record(out, f"{prefix}{c['id']}/{s}", h, c, [])
    h.close()


def main(out_path, child):
    for name in C.SWITCHES:
        assert os.environ.get(name) == C.CHILD_ENV[child].get(name), (name, os.environ.get(name))
    out = {}
    t0 = time.time()
    for c in C.FORCED[child]:
        run_case(out, f"{C.CHILD_IDS[child]}/", c)
    out["seconds"] = np.float64(time.time() - t0)
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]))
