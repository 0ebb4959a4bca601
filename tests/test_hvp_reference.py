"""Anchors of tests/_hvp_ref.py, the fp64 reference of the exact Hessian-vector product, on the CPU (no GPU needed):
(a) its loss and gradient equal the committed oracle's (orc.objective) on every case the GPU parity tests use -- both fp64, so only
    the order of the sums differs;
(b) its product equals every committed vhp fixture (hvp.npz, hvp_cases.npz: fp64 autograd run on the reference project);
(c) composed through costs.hybrid.combine_derivatives it equals the "inv"-weighted fixtures (hvp_inv.npz);
(d) the filter of events on a cell border (drop_ambiguous) removes at most 0.5 % of any case's batch."""
import numpy as np
import pytest

from event_based_optical_flow_amd.costs.hybrid import combine_derivatives
from oracle import oracle as orc

import _hvp_cases as C
import _hvp_ref as R

ANCHOR_TOL = 1e-10
FIXTURE_TOL = 1e-9


def rel_max(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("cid", list(C.ALL))
def test_reference_equals_the_oracle_and_drops_few_events(cid):
    c = C.ALL[cid]
    b = C.built(c)
    print(f"[hvp ref] {cid}: share_dropped {b['dropped']:.5f} (margin {b['margin']:.2e}, {len(b['ev'])} events kept)")
    assert b["dropped"] <= C.DROP_CAP, (cid, b["dropped"])
    assert np.isfinite(b["loss"]) and np.isfinite(b["hv"]).all() and np.abs(b["hv"]).max() > 0
    ev, wd = b["ev"], c["warp_direction"]
    if b["t_range"] is not None:
        # a time slice warps to the WHOLE batch's first event: for the oracle, that time as a fraction of the slice's own span
        # (not normalised, so the span itself does not enter)
        assert not c["normalize_t"] and wd == "first"
        lo, hi = ev[:, 2].min(), ev[:, 2].max()
        wd = float((b["t_range"][0] - lo) / (hi - lo))
    ref = orc.objective(ev, b["motion"], c["model"], c["size"], cost=c["cost"], sigma=c["sigma"], outer_padding=c["pad"],
                        omit_boundary=c["omit"], direction=c["direction"], normalize_t=c["normalize_t"], warp_direction=wd)
    assert abs(b["loss"] - ref["loss"]) <= ANCHOR_TOL * abs(ref["loss"]), (cid, b["loss"], ref["loss"])
    assert rel_max(b["grad"], ref["grad"]) <= ANCHOR_TOL, (cid, rel_max(b["grad"], ref["grad"]))


_MODEL_OF = {"2dof": ("2d-translation", "theta"), "dense_smooth": ("dense-flow", "flow_smooth"), "voxel": ("dense-flow-voxel", "voxel")}


def test_reference_equals_the_vhp_fixtures(golden):
    g, o, g0 = golden("hvp_cases"), golden("objective"), golden("hvp")
    size = tuple(int(v) for v in o["image_size"])
    tags = sorted(k[: -len("__vhp")] for k in g if k.endswith("__vhp"))
    assert len(tags) == 9
    for tag in tags:
        mname, cost, s = tag.split("__")
        model, mkey = _MODEL_OF[mname]
        loss, _, hv = R.value_grad_hvp(o["events"], o[mkey], model, size, g[tag + "__v"], cost=cost, sigma=int(s[1:]))
        assert abs(loss - float(g[tag + "__loss"])) <= FIXTURE_TOL * abs(float(g[tag + "__loss"])), tag
        assert rel_max(hv, g[tag + "__vhp"]) <= FIXTURE_TOL, (tag, rel_max(hv, g[tag + "__vhp"]))
    loss, _, hv = R.value_grad_hvp(g0["events"], g0["theta"], "2d-translation", tuple(int(v) for v in g0["image_size"]), g0["v"],
                                   cost="image_variance", sigma=1)
    assert abs(loss - float(g0["loss"])) <= FIXTURE_TOL * abs(float(g0["loss"]))
    assert rel_max(hv, g0["vhp"]) <= FIXTURE_TOL


@pytest.mark.parametrize("case", [0, 1, 2])
def test_reference_equals_the_inverse_weight_fixtures(golden, case):
    """Hybrid costs with an "inv" weight: phi' H_c v + phi'' <grad c, v> grad c per member, with the factors from
    costs.hybrid.combine_derivatives (plain Python: it needs no GPU)."""
    g, o = golden("hvp_inv"), golden("objective")
    k = f"case{case}"
    size = tuple(int(v) for v in o["image_size"])
    model, motion, v = str(g[k + "__model"]), o[str(g[k + "__motion_key"])], g[k + "__v"]
    loss, grad, hv = 0.0, 0.0, 0.0
    for name, w in zip(g[k + "__costs"], (str(x) for x in g[k + "__weights"])):
        c, gc, hc = R.value_grad_hvp(o["events"], motion, model, size, v, cost=str(name), sigma=1)
        weight = w if w == "inv" else float(w)
        p1, p2 = combine_derivatives(weight, c)
        loss += 1.0 / c if weight == "inv" else weight * c
        grad = grad + p1 * gc
        hv = hv + p1 * hc + p2 * float((gc * v).sum()) * gc
    assert abs(loss - float(g[k + "__loss"])) <= FIXTURE_TOL * abs(float(g[k + "__loss"]))
    assert rel_max(grad, g[k + "__grad"]) <= FIXTURE_TOL
    assert rel_max(hv, g[k + "__vhp"]) <= FIXTURE_TOL, rel_max(hv, g[k + "__vhp"])
