"""Child process of tests/test_gpu_flow64.py: the fp64-flow batches of tests/_flow64_cases.py on one forced segment layout
(CMAX_BIG_SEG / CMAX_MID_SEG / CMAX_COMPACT are read once per process).  usage: _flow64_worker.py <out.npz> <case id> ...; per case it
writes loss, gradient and grad_events[:, 0:2] of evaluate_event_grad(exact_flow=True), loss and gradient of the plain evaluate behind it, of
the fp32 call on f32(flow), and what work_list_info / batch_info say about the layout the case ran on."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(out, ids):
    import torch

    import event_based_optical_flow_amd as E

    import _flow64_cases as X

    got = {}
    for cid in ids:
        c = X.built(cid)
        h = E.CMaxHandle(c["size"], c["pad"]).set_events(c["ev"], time_bin=c["T"], on_dropped="ignore")
        desc = E.make_descriptor(c["cost"], c["model"], sigma=float(c["sigma"]), normalize_t=c["normalize_t"], time_bin=c["T"],
                                 warp_direction=c["warp_direction"])
        info = dict(h.work_list_info(), **h.batch_info())
        for k in ("segments", "segment_events", "small_accumulators", "owned_groups", "packed"):
            got[f"{cid}/{k}"] = int(info[k])
        F = torch.tensor(c["motion"], dtype=torch.float64, device="cuda")
        res, grad, ge, _ = h.evaluate_event_grad(desc, F, exact_flow=True)
        got[cid + "/grad_events"] = ge[:, :2].double().cpu().numpy()
        got[cid + "/loss"], got[cid + "/grad"] = res[0].item(), grad.double().cpu().numpy()
        res, grad = h.evaluate(desc, F, exact_flow=True)
        got[cid + "/loss2"], got[cid + "/grad2"] = res[0].item(), grad.double().cpu().numpy()
        res, grad = h.evaluate(desc, F.float())
        got[cid + "/loss32"], got[cid + "/grad32"] = res[0].item(), grad.double().cpu().numpy()
        h.close()
    np.savez(out, **got)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
