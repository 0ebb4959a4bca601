"""Border-snapped batches (tests/_cell_cases.py), without a GPU and without the package: the CONDITIONS every case of
tests/test_gpu_exact_cells.py has to meet -- they are conditions, not measurements: a case that misses one is changed, not the threshold --
and the negative control of that test's checker.

  distance      every snapped event outside the ladder lies within 0.25 fp32 ulp of its displacement of its border, and every snapped event
                (ladder included; every moved event of the batch, in fact) keeps at least 16 * |motion|_max * 2^-32 from every border: 16 x
                what the packed time (fp32 plus a residual byte) resolves.  An exact tie is not defined and not tested.
  flip share    the numpy fp32 restatement of the device's split-base formula (fp32_cells) takes another cell than fp64 on >= 25 % of the
                non-ladder snapped events;
  discriminating share   for >= 60 % of the snapped events the per-event gradient read from the cell across the border differs from the
                right one by >= 1e-2 of the column's largest entry: 100 x the gate;
  references    orc.objective and tests/_hvp_ref.objective agree on loss and gradient at 1e-10: both picked the same cells;
  negative control   the GPU test's own checker FAILS on a result composed from fp32_cells (the oracle's vote_bwd on coordinates nudged
                into that cell).  A checker a kernel without exact cells could pass is not done.
The figures are printed (profiles/exact_cells_parity.txt)."""
import numpy as np
import pytest

from oracle import oracle as orc

import _cell_cases as C
import _hvp_ref

IDS = [c["id"] for c in C.TABLE + C.WORKER]
AGREE_TOL = 1e-10
NO_SNAP = ("2dof-none",)
ONE = ("2dof-one", "dense-one")


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


@pytest.mark.parametrize("cid", IDS)
def test_conditions(cid):
    c = C.measured(cid)
    print(f"[cell cases] {cid}: {c['n']} events on {c['size'][0]} x {c['size'][1]}, snapped {c['n_snapped']} (ladder {c['n_ladder']}), lower {c['lower']:.2e} "
          f"min distance {c['min_dist']:.2e}, worst {c['worst_ulp']:.3f} ulp, flip share {c['flip_share']:.2f} ({c['n_flip']} events), "
          f"discriminating share {c['disc_share']:.2f}")
    assert c["ev"][0, 2] == c["ev"][:, 2].min() and c["ev"][-1, 2] == c["ev"][:, 2].max()
    assert 0 not in c["snapped"] and c["n"] - 1 not in c["snapped"] and len(np.unique(c["snapped"])) == len(c["snapped"])
    assert c["min_dist"] >= c["lower"]
    if cid in NO_SNAP:
        assert c["n_snapped"] == 0
        return
    assert c["n_snapped"] == 1 if cid in ONE else c["n_snapped"] >= 100
    if c["share"] == 1.0 and c["model"] == C.TWO:  # every slot a candidate: what did not verify is a few per cent
        assert c["n_snapped"] >= 0.85 * c["n"]
    assert c["worst_ulp"] <= 0.25
    assert c["flip_share"] >= 0.25
    assert c["disc_share"] >= 0.60
    if c["frac"]:
        assert (c["axes"] == 3).sum() >= 20  # corners
    if c["model"] != C.TWO:  # one snapped event per source pixel (and bin)
        ix, iy = C._pixel(c["ev"][c["snapped"]], c["size"])
        key = (ix * c["size"][1] + iy) * max(c["T"], 1) + (C._bins(c["ev"], c["T"])[c["snapped"]] if c["T"] else 0)
        assert len(np.unique(key)) == len(key)
    if c["model"] == C.VOXEL:  # nobody left its time bin
        orig = C.batch(c["n"], c["size"], 100 + c["seed"], c["frac"])
        assert (C._bins(orig, c["T"]) == C._bins(c["ev"], c["T"])).all()


@pytest.mark.parametrize("cid", IDS)
def test_both_references_picked_the_same_cells(cid):
    c = C.measured(cid)
    kw = C.ref_kwargs(c)
    ref = orc.objective(c["ev"], c["motion"], c["model"], c["size"], **kw)
    loss, grad, _ = _hvp_ref.value_grad_hvp(c["ev"], c["motion"], c["model"], c["size"], np.zeros_like(np.asarray(c["motion"])), **kw)
    e = [abs(loss - ref["loss"]) / abs(ref["loss"]), _rel(grad, ref["grad"])]
    print(f"[cell cases] {cid}: oracle against the torch restatement: loss {e[0]:.1e} gradient {e[1]:.1e}")
    assert max(e) <= AGREE_TOL, (cid, e)
    assert abs(c["full"]["loss"] - ref["loss"]) <= AGREE_TOL * abs(ref["loss"]) and _rel(c["full"]["grad"], ref["grad"]) <= AGREE_TOL


@pytest.mark.parametrize("cid", IDS)
def test_negative_control_fp32_cells_fail_the_checker(cid):
    c = C.measured(cid)
    right = C.event_xy_grad(c, G=c["G"])
    wrong = C.event_xy_grad(c, cells=c["cells32"], G=c["G"])
    got = c["ref"] + (wrong - right)
    C.check_per_event(f"{cid} (the reference itself)", c["ref"], c["ref"], c)
    if cid in NO_SNAP:  # nothing near a border: fp32 takes the fp64 cells, and the checker passes
        assert not (wrong - right).any()
        return
    with pytest.raises(AssertionError):
        C.check_per_event(f"{cid} (fp32 cells)", got, c["ref"], c)
    e = [_rel(got[:, k], c["ref"][:, k]) for k in range(2)]
    assert max(e) >= 100 * C.TOL, (cid, e)  # not a near miss
    if c["model"] != C.TWO:  # ... and the flow gradient of a pixel that holds a wrong event shows it too: one snapped event per pixel
        ev, m = orc._ev4(c["ev"]), np.asarray(c["motion"])
        g = np.zeros_like(m)
        for di, direction in enumerate(C.directions_of(c)):
            xy, aux = orc.warp_event(ev, m, c["model"], direction, c["size"], c["normalize_t"])
            xyw = xy.copy()
            for axis in (0, 1):
                xs = xy[:, axis] + 1e-6
                move = c["cells32"][direction][axis] - np.floor(xs).astype(np.int64)
                xyw[:, axis] = np.where(move != 0, xy[:, axis] - 2.0 * (xs - np.rint(xs)), xy[:, axis])
            gx, gy = orc.vote_bwd(xyw, c["size"], c["G"][direction], c["pad"])
            g = g + orc.motion_grad(ev, m, c["model"], aux, gx, gy)
        assert _rel(g, c["full"]["grad"]) >= 10 * C.TOL, cid


def test_fp32_cells_is_the_device_formula_on_an_easy_batch():
    """Away from borders the restatement and fp64 agree on every event (so a disagreement is a border effect, not a bug of fp32_cells)."""
    ev = C.batch(4000, C.BASE, 7)
    for model, motion, T in ((C.TWO, C.THETA, 0), (C.DENSE, C.smooth_flow(C.BASE, 8.0, 3), 0),
                             (C.VOXEL, np.stack([C.smooth_flow(C.BASE, 8.0, 3 + t) for t in range(3)]), 3)):
        for direction in ("first", "middle", 1.0 / 3.0):
            if model == C.VOXEL and direction != "first":
                continue
            warped, _ = orc.warp_event(ev, motion, model, direction, C.BASE)
            xs = warped[:, :2] + 1e-6
            far = (np.abs(xs - np.rint(xs)) > 1e-4).all(axis=1)
            r64, c64 = C.fp64_cells(ev, motion, model, C.BASE, direction)
            r32, c32 = C.fp32_cells(ev, motion, model, C.BASE, direction, T=T)
            assert far.sum() > 3900 and (r64[far] == r32[far]).all() and (c64[far] == c32[far]).all()


@pytest.mark.parametrize("model", [C.TWO, C.DENSE])
def test_batch_and_state_cases(model):
    """K = 3 motions with a snapped third each (objective_batch), and the all-snapped batch with ONE further event snapped at a second
    motion (stale nibbles): a gradient composed from the fp32 cells misses the gate at every motion."""
    b, s = C.batch_case(model), C.state_case(model)
    rows = [(f"candidate {k}", b["ev"], b["motions"][k], len(b["snapped"][k]), b["n_flip"][k]) for k in range(len(b["motions"]))]
    rows += [("state A", s["ev"], s["A"], len(s["snapped_A"]), None), ("state B", s["ev"], s["B"], 1, 1)]
    for tag, ev, motion, n_snapped, n_flip in rows:
        c = dict(C.case("x", model), ev=ev, motion=motion, size=b["size"])
        full = C.event_grad_objective(ev, motion, model, b["size"], 1.0)
        G = C.image_grads(c, full)
        cells = {"first": C.fp32_cells(ev, motion, model, b["size"], "first")}
        r64 = C.fp64_cells(ev, motion, model, b["size"], "first")
        wrong = int(((cells["first"][0] != r64[0]) | (cells["first"][1] != r64[1])).sum())
        got = full["grad_events"][:, :2] + C.event_xy_grad(c, cells, G) - C.event_xy_grad(c, None, G)
        e = max(_rel(got[:, k], full["grad_events"][:, k]) for k in range(2))
        print(f"[cell cases] {model} {tag}: snapped {n_snapped}, fp32-wrong {wrong}, per-event rel err of the fp32 cells {e:.1e}")
        assert n_snapped >= (1 if tag == "state B" else 100) and wrong >= (1 if tag == "state B" else 25) and e >= 100 * C.TOL, (tag, wrong, e)
    assert s["one"] not in s["snapped_A"]
    assert orc.objective(s["ev"], s["A"], model, s["size"])["loss"] != 0.0
