"""Child process of tests/test_gpu_weight_grad.py: one forced segment layout (CMAX_BIG_SEG / CMAX_MID_SEG / CMAX_COMPACT are read once per
process).  usage: _weight_grad_worker.py <big | mid> <out.npz>; writes result, gradient and dL/dw of the cases below and the segment size it ran with."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# mid segments are only cut from a group-aligned list whose groups hold <= 3064 events: 256 tiles of ~2340 uniform events (tests/_hvp_cases.py)
BATCH = {"big": (150_000, (96, 128)), "mid": (600_000, (256, 256))}
CASES = [("2d-translation", "image_variance", 0), ("dense-flow", "normalized_gradient_magnitude", 1)]


def batch(layout):
    import event_based_optical_flow_amd as E
    from _weighted_ref import weight_set

    n, size = BATCH[layout]
    ev = E.utils.generate_events(n, size[0], size[1], 0.0, 0.05, seed=41)
    return ev, weight_set("zeros", ev, seed=33), size


def motion_for(model, size):
    import event_based_optical_flow_amd as E

    if model == "2d-translation":
        return np.array([7.3, -4.1])
    return np.asarray(E.utils.generate_smooth_flow(size, 8, seed=11), dtype=np.float32).astype(np.float64)


def main(layout, out):
    import event_based_optical_flow_amd as E

    ev, w, size = batch(layout)
    h = E.CMaxHandle(size).set_events(ev, weights=w)
    got = {"segment_events": h.work_list_info()["segment_events"]}
    for model, cost, sigma in CASES:
        res, grad, gw = h.evaluate_weight_grad(E.make_descriptor(cost, model, sigma=sigma), motion_for(model, size))
        tag = f"{model}/{cost}"
        got[tag + "/loss"], got[tag + "/grad"], got[tag + "/grad_w"] = res[0].item(), grad.double().cpu().numpy(), gw.double().cpu().numpy()
    h.close()
    np.savez(out, **got)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
