"""Child process of tests/test_gpu_exact_cells.py: border-snapped batches (tests/_cell_cases.py) on one forced segment layout or path
(CMAX_BIG_SEG / CMAX_MID_SEG / CMAX_COMPACT / CMAX_TAN2 are read once per process).  usage: _cell_worker.py <out.npz> <case id> ...; per
case it writes loss, gradient, grad_events[:, 0:2] (CMAX_TAN2: the evaluation only -- that path has no event gradient), what
work_list_info / batch_info say about the layout the case ran on, and the launches per kernel class of one more `evaluate` on a fresh handle
with the launch brackets on ("<case>/launches/<class>"): the tangent-image path has no pass over the events for the gradient."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(out, ids):
    import event_based_optical_flow_amd as E

    import _cell_cases as C

    tan2 = os.environ.get("CMAX_TAN2") == "1"
    got = {}
    for cid in ids:
        c = C.built(cid)
        h = E.CMaxHandle(c["size"], c["pad"]).set_events(c["ev"], time_bin=c["T"], on_dropped="ignore")
        desc = E.make_descriptor(c["cost"], c["model"], sigma=float(c["sigma"]), normalize_t=c["normalize_t"], time_bin=c["T"],
                                 warp_direction=c["warp_direction"])
        info = dict(h.work_list_info(), **h.batch_info())
        for k in ("segments", "segment_events", "small_accumulators", "owned_groups", "packed"):
            got[f"{cid}/{k}"] = int(info[k])
        if tan2:
            res, grad = h.evaluate(desc, c["motion"])
        else:
            res, grad, ge, _ = h.evaluate_event_grad(desc, c["motion"])
            got[cid + "/grad_events"] = ge[:, :2].double().cpu().numpy()
        got[cid + "/loss"], got[cid + "/grad"] = res[0].item(), grad.double().cpu().numpy()
        res, grad = h.evaluate(desc, c["motion"])  # the same nibbles, followed by the plain evaluation's K3
        got[cid + "/loss2"], got[cid + "/grad2"] = res[0].item(), grad.double().cpu().numpy()
        h.close()
        import torch

        h = E.CMaxHandle(c["size"], c["pad"]).set_events(c["ev"], time_bin=c["T"], on_dropped="ignore")
        h.set_profiling(True)
        h.evaluate(desc, c["motion"])
        torch.cuda.synchronize()
        for k, v in h.read_profile().items():
            got[f"{cid}/launches/{k}"] = int(v[1])
        h.set_profiling(False)
        h.close()
    np.savez(out, **got)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
