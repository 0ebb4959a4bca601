"""Child program of tests/test_gpu_image_side.py::test_path_switches_in_a_child_process, and the device side both share.

CMAX_NO_FUSED_BLURVAR, CMAX_NO_STATS_INSIDE, CMAX_TAN2, CMAX_NSUB and CMAX_STAT_SWEEPS are read once per process (eval_plan and stat_nsub
of csrc/cmax_fused.hip), so a switched path needs a process of its own.  usage: _image_worker.py <child> <out.npz>, with the child's
switches in the environment.  For every row of the child (tests/_image_cases.CHILDREN) it writes loss, gradient and the image of every
reference time; the parent compares them with the references.  One row per child is evaluated once more on a handle of its own with
the launch brackets on, and the launches per kernel class are written too ("profile/<class>")."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import event_based_optical_flow_amd as E  # noqa: E402

import _image_cases as C  # noqa: E402


def descriptor(c):
    return E.make_descriptor(c["cost"], c["model"], direction=c["direction"], sigma=float(c["sigma"]), omit_boundary=c["omit"], time_bin=c["T"])


def handle(c, ev, deterministic=False):
    h = E.CMaxHandle(c["size"], c["pad"])
    if deterministic:
        h.set_deterministic(True)
    h.set_events(ev, time_bin=c["T"], on_dropped="ignore")  # (the 2-DoF border set holds finite off-sensor sources: kept, the default)
    assert h.n_events == len(ev), (c["id"], h.n_events, len(ev))
    return h


def n_ref(c):
    return len(C.directions(c))


def images(h, c):
    return [h.last_iwe(k).double().cpu().numpy() for k in range(n_ref(c))]


def launches(c, ev, call):
    """{kernel class: launches} of one `call(handle, descriptor)` on a fresh handle with the launch brackets on"""
    import torch

    h, desc = handle(c, ev), descriptor(c)
    h.set_profiling(True)
    call(h, desc)
    torch.cuda.synchronize()
    counts = {k: int(v[1]) for k, v in h.read_profile().items()}
    h.set_profiling(False)
    h.close()
    return counts


def main(child, out_path):
    env, rows, mode = C.CHILDREN[child]
    for k, v in env.items():
        assert os.environ.get(k) == v, (k, os.environ.get(k))
    out = {}
    for c in rows:
        b, cid = C.built(c), c["id"]
        h, desc = handle(c, b["ev"]), descriptor(c)
        if mode == "tan2" and c["label"] == C.TAN2_NORMALISED:
            h.evaluate(desc, b["motion"])  # builds the un-warped image's statistics on the standard path; the next one takes the tangent images
        res, grad = h.evaluate(desc, b["motion"])
        out[cid + "/loss"], out[cid + "/grad"] = res[0].item(), grad.double().cpu().numpy()
        for k, img in enumerate(images(h, c)):
            out[f"{cid}/iwe{k}"] = img
        if mode == "both":
            res, _ = h.evaluate(desc, b["motion"], want_grad=False)
            out[cid + "/vloss"] = res[0].item()
            for k, img in enumerate(images(h, c)):
                out[f"{cid}/viwe{k}"] = img
        h.close()
    # 18 x 66 (an even pixel count: the default takes the statistics inside K3 there), single reference time, not normalised
    c = next((c for c in rows if c["shape"] == (18, 66) and c["pad"] == 0 and n_ref(c) == 1 and "normalized" not in c["cost"]), rows[0])
    assert n_ref(c) == 1 and "normalized" not in c["cost"]
    b = C.built(c)
    for k, v in launches(c, b["ev"], lambda h, desc: h.evaluate(desc, b["motion"])).items():
        out["profile/" + k] = v
    out["profile/id"] = c["id"]
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
