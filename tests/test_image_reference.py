"""The references of the image-side parity tests, without a GPU, on every row of tests/_image_cases.py:
(a) tests/_image_ref.objective_from_images with zero offsets IS _hvp_ref.objective (equal, not close);
(b) _hvp_ref.objective agrees with the committed oracle (orc.objective) on loss and gradient at 1e-10, the tolerance of
    tests/test_hvp_reference.py -- at padded shapes from 1 x 9 up, which neither had been run at;
(c) with non-zero offsets, central finite differences of objective_from_images in the motion agree with its autograd gradient (step and
    tolerance of tests/test_event_grad_reference.py);
(d) the coverage condition of the `cover` and `border` sets: every pixel of the padded image that the set can reach is a bilinear
    corner of at least one event at every reference time of the case.  `cover`: every pixel of the sensor, and with a padding every
    pixel within ceil(max displacement) of it.  `border`: every event starts within 2 pixels of the sensor's edge (2-DoF: or off the
    sensor), so what it can reach is that band -- every pixel of it, and the padding within ceil(max displacement) of the sensor;
(e) the filter of cell-border events removes at most 0.5 % of a batch, no batch exceeds 1e5 events, and no `border` row has a
    cancelling gradient (|g|_inf >= 1e-3 of the largest sum of per-event absolute contributions);
(f) no row of the deferred 2-DoF variance has a contrast so flat that the fp32 terms of its sum I^2 would take more than a quarter of the
    gate (STATISTICS_BUDGET)."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc

import _hvp_ref as R
import _image_cases as C
import _image_ref as IR

ANCHOR_TOL = 1e-10
FD_H = 1e-5
EPS = 2.0 ** -52
CONDITIONING_FLOOR = 1e-3
# The deferred 2-DoF variance (2-DoF, variance, no blur) sums I^2 from fp32 terms, so its contrast carries about
# mean^2 / variance x 2^-24 and a normalised cost's gradient twice that per reference time (_image_ref.fp32_statistics_error: one rounding's
# size, not a bound -- three reference times and the image's own rounding come on top).  A row may spend a quarter of the 1e-4 gate on it.
STATISTICS_BUDGET = 2.5e-5


def rel_max(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def test_the_table_holds_what_it_promises():
    grid = {(c["shape"], c["label"], c["omit"]) for c in C.GRID}
    assert grid == {(s, lab, o) for s in C.SHAPES for lab in C.LABELS for o in C.omits(s)}
    assert all(c["model"] == "dense-flow" and c["events"] == "cover" and c["pad"] == 0 for c in C.GRID)
    rows = dict(C.PATHS)
    rows.update({name: child_rows for name, (_, child_rows, _) in C.CHILDREN.items() if not name.startswith("sweeps")})
    rows["offsets"] = [c for _, c in C.OFFSETS]
    for pattern in C.OFFSET_PATTERNS:
        rows["offsets " + pattern] = [c for p, c in C.OFFSETS if p == pattern]
    for axis, pick in (("2-DoF", lambda c: c["model"] == "2d-translation"), ("sparse", lambda c: c["events"] == "sparse"),
                       ("border", lambda c: c["events"] == "border"), ("maximize", lambda c: c["direction"] == "maximize")):
        rows[axis] = [c for c in C.ALL.values() if pick(c) and c["label"] in C.OBJECTIVES]
    for name, rr in rows.items():
        assert {c["shape"] for c in rr} == set(C.SHAPES), name
        if name not in ("no_fused_blurvar", "no_stats_inside", "tan2"):  # (one kernel's objectives by construction)
            assert {c["label"] for c in rr} >= set(C.LABELS) or name.startswith("nsub"), name
    assert {c["shape"] for c in C.ALL.values() if c["T"] == 3} == set(C.LARGEST)
    assert any(c["shape"] == (17, 65) and c["size"] == (15, 63) and c["pad"] == 1 for c in C.ALL.values())
    for shape in C.MEAN_SHAPES:
        for omit in (True, False):
            for label in ("image_variance@1", "image_variance@0"):
                assert C.case(shape, label, omit, events="border")["id"] in {c["id"] for c in C.PATHS["default"]}


@pytest.mark.parametrize("cid", list(C.ALL))
def test_references_agree_and_the_set_covers_its_reach(cid):
    c = C.ALL[cid]
    b = C.built(c)
    ev, m = b["ev"], b["motion"]
    assert len(ev) <= C.MAX_EVENTS and b["dropped"] <= C.DROP_CAP, (cid, len(ev), b["dropped"])
    kw = C.ref_kwargs(c)
    evt = torch.as_tensor(ev)
    mt = torch.as_tensor(np.ascontiguousarray(m, dtype=np.float64)).clone().requires_grad_()
    loss = R.objective(evt, mt, c["model"], c["size"], **kw)
    (g,) = torch.autograd.grad(loss, mt)
    loss, g = float(loss.detach()), g.numpy()
    assert np.isfinite(loss) and np.isfinite(g).all() and np.abs(g).max() > 0, cid
    # (a) zero offsets: the same number
    zero = [np.zeros(c["shape"])] * C.n_slots(c)
    with torch.no_grad():
        assert float(IR.objective_from_images(evt, mt.detach(), c["model"], c["size"], zero, **kw)) == loss, cid
    # (b) the oracle
    ref = orc.objective(ev, m, c["model"], c["size"], **kw)
    e_loss, e_grad = abs(loss - ref["loss"]) / abs(ref["loss"]), rel_max(g, ref["grad"])
    assert e_loss <= ANCHOR_TOL and e_grad <= ANCHOR_TOL, (cid, e_loss, e_grad)
    line = f"[image ref] {cid}: {len(ev)} events, dropped {b['dropped']:.5f}, hvp_ref vs oracle loss {e_loss:.1e} grad {e_grad:.1e}"
    # (d) coverage
    if c["events"] != "sparse":
        hit = IR.coverage(ev, m, c["model"], c["size"], c["cost"], c["pad"])
        (H, W), pad, (Hp, Wp) = c["size"], c["pad"], c["shape"]
        reach = int(np.ceil(R.max_displacement(ev, m, c["model"], c["size"], C.directions(c))))
        r, col = np.meshgrid(np.arange(Hp) - pad, np.arange(Wp) - pad, indexing="ij")  # sensor coordinates of the padded image
        outside = np.maximum(np.maximum(-r, r - (H - 1)), np.maximum(-col, col - (W - 1)))  # > 0: that far off the sensor
        inside = np.minimum(np.minimum(r, H - 1 - r), np.minimum(col, W - 1 - col))  # >= 0: distance to the sensor's edge
        need = (outside <= reach) if c["events"] == "cover" else ((outside <= reach) & (inside < 2))
        missing = need[None] & ~hit
        assert not missing.any(), (cid, reach, np.argwhere(missing)[:8].tolist())
        line += f", reach {reach}, {int(need.sum())} of {Hp * Wp} pixels required and covered"
    # (e) conditioning of the rows that concentrate events where the mean from the vote sums matters
    if c["events"] == "border" and c["model"] != "dense-flow-voxel":
        ratio = IR.conditioning(ev, m, c["model"], c["size"], ref, c["sigma"], c["pad"])
        line += f", conditioning {ratio:.2e}"
        assert ratio >= CONDITIONING_FLOOR, (cid, ratio)
    # (f) conditioning of the contrast itself on the rows whose statistics come from fp32 terms
    if c["model"] == "2d-translation" and c["cost"].endswith("image_variance") and c["sigma"] == 0:
        e_l, e_g = IR.fp32_statistics_error(ev, m, c["model"], c["size"], ref, c["omit"], c["pad"])
        line += f", fp32 statistics: loss {e_l:.1e} gradient {e_g:.1e}"
        assert max(e_l, e_g) <= STATISTICS_BUDGET, (cid, e_l, e_g)
    print(line)


FD_CASES = [("corners", C.case((9, 33), "gradient_magnitude@1", True, model="2d-translation")),  # a 2-DoF theta
            ("checker", C.case((4, 4), "image_variance@1", True)),                               # a dense flow on a tiny shape
            ("ramp", C.case((5, 33), "multi_focal_normalized_image_variance@0", False)),        # a normalised cost
            ("inner", C.case((8, 32), "normalized_gradient_magnitude@0", True, model="2d-translation"))]


@pytest.mark.parametrize("pattern,c", FD_CASES, ids=[f"{p}-{c['id']}" for p, c in FD_CASES])
def test_offsets_gradient_against_finite_differences(pattern, c):
    """Central differences of the loss on vote + offset in the motion.  Rounding of the quotient <= 64 eps |L| / h, truncation budget
    10 h^2, relative to the largest entry (the reasoning of tests/test_event_grad_reference.py); no event within 1e-3 of a cell border."""
    b = C.built(c)
    m = b["motion"]
    ev, _ = R.drop_ambiguous(b["ev"], m, c["model"], c["size"], C.directions(c), 1e-3)
    kw = C.ref_kwargs(c)
    offs = C.offsets(pattern, c, float(IR.vote_images(ev, m, c["model"], c["size"], c["cost"], c["pad"]).max()))
    assert max(np.abs(o).max() for o in offs) > 0
    loss, grad, _ = IR.value_grad_images(ev, m, c["model"], c["size"], offs, **kw)
    plain, _, _ = IR.value_grad_images(ev, m, c["model"], c["size"], [np.zeros(c["shape"])] * len(offs), **kw)
    assert abs(loss - plain) > 1e-6 * abs(plain), "the offset does not reach the loss"
    evt = torch.as_tensor(ev)
    flat = np.abs(grad).ravel()
    idx = sorted(set([int(flat.argmax()), 0, flat.size - 1, flat.size // 2] + list(np.argsort(flat)[-3:])))
    scale = flat.max()
    tol = 64 * EPS * abs(loss) / FD_H / scale + 10 * FD_H ** 2
    worst = 0.0
    with torch.no_grad():
        for i in idx:
            d = np.zeros(m.size)
            d[i] = FD_H
            d = d.reshape(m.shape)
            lp = float(IR.objective_from_images(evt, torch.as_tensor(m + d), c["model"], c["size"], offs, **kw))
            lm = float(IR.objective_from_images(evt, torch.as_tensor(m - d), c["model"], c["size"], offs, **kw))
            worst = max(worst, abs((lp - lm) / (2 * FD_H) - grad.ravel()[i]) / scale)
    print(f"[image ref] fd {pattern} {c['id']}: {len(idx)} components, rel err {worst:.2e} (tolerance {tol:.2e})")
    assert worst <= tol, (pattern, c["id"], worst, tol)
