"""fp64 flows at the boundary (tests/_flow64_cases.py), without a GPU and without the package: the CONDITIONS every case of
tests/test_gpu_flow64.py has to meet -- conditions, not measurements: a case that misses one is changed, not the bound -- and the negative
control of that test's checkers.

  (a) flips      every snapped event takes another cell under the caller's fp64 flow than under f32(flow) (two oracle warps), at a
                 distance from its border between _cell_cases.lower_bound and 0.6 |dt| |r|, one per source pixel (and bin), nobody left its
                 time bin, the first and the last event untouched;
  (b) gap        orc.objective at f32(flow) and at the fp64 flow differ, in the gradient rows of the snapped events' source pixels, by
                 more than 1e-3 of the largest gradient entry: 10 x the gate -- a result computed on the rounded flow cannot pass;
  (c) control    the GPU test's own checkers (gradient, per event) FAIL on the oracle's result at f32(flow);
  (d) split      the numpy restatement of the device's split gives hi == f32(v) and |v - (hi + lo)| <= 2^-47 |v|, lo = 0 where hi is
                 not finite.
The figures are printed (profiles/flow64_parity.txt)."""
import numpy as np
import pytest

from oracle import oracle as orc

import _cell_cases as C
import _flow64_cases as X

IDS = [c["id"] for c in X.TABLE + X.WORKER]
NO_SNAP = ("dense-none",)
ONE = ("dense-one",)
GAP = 10.0 * X.TOL


@pytest.mark.parametrize("cid", IDS)
def test_snapped_events_flip_between_the_flow_and_its_rounding(cid):
    c = X.built(cid)
    ev, F, model, size, snapped = c["ev"], c["motion"], c["model"], c["size"], c["snapped"]
    assert (C.f32(F) == c["motion32"]).all() and (F != c["motion32"]).all()  # nothing of the flow is representable in fp32
    assert ev[0, 2] == ev[:, 2].min() and ev[-1, 2] == ev[:, 2].max()
    assert 0 not in snapped and c["n"] - 1 not in snapped and len(np.unique(snapped)) == len(snapped)
    low = C.lower_bound(ev, F, c["normalize_t"])
    flip = np.zeros(len(snapped), dtype=bool)
    min_dist, worst = np.inf, 0.0
    for direction in C.directions_of(c):
        c64 = C.fp64_cells(ev, F, model, size, direction, c["normalize_t"])
        c32 = C.fp64_cells(ev, c["motion32"], model, size, direction, c["normalize_t"])
        warped, aux = orc.warp_event(ev, F, model, direction, size, c["normalize_t"])
        for axis in (0, 1):
            here = c64[axis][snapped] != c32[axis][snapped]
            flip |= here
            idx = snapped[here]
            assert (np.abs(c64[axis][idx] - c32[axis][idx]) == 1).all()
            xs = warped[idx, axis] + 1e-6
            dist = np.abs(xs - np.rint(xs))
            r = np.abs(C._coef(ev, F, model, size, c["T"], axis) - C._coef(ev, c["motion32"], model, size, c["T"], axis))[idx]
            bound = np.abs(aux["dt"][idx]) * r  # the flow's rounding moves x' by |dt| |r|: a flip lies closer to its border than that
            assert (dist < bound).all()
            if len(idx):
                min_dist, worst = min(min_dist, dist.min()), max(worst, (dist / bound).max())
    print(f"[flow64 cases] {cid}: {c['n']} events on {size[0]} x {size[1]}, snapped {len(snapped)}, lower {low:.2e}, min distance {min_dist:.2e}, "
          f"largest distance / (|dt| |r|) {worst:.2f}")
    assert flip.all()
    if cid in NO_SNAP:
        assert len(snapped) == 0
        return
    assert len(snapped) == 1 if cid in ONE else len(snapped) >= 100
    assert min_dist >= low and worst <= 0.6 * 1.0001
    ix, iy = C._pixel(ev[snapped], size)
    key = (ix * size[1] + iy) * max(c["T"], 1) + (C._bins(ev, c["T"])[snapped] if c["T"] else 0)
    assert len(np.unique(key)) == len(key)
    if model == X.VOXEL:
        orig = C.batch(c["n"], size, 100 + c["seed"], c["frac"])
        assert (C._bins(orig, c["T"]) == C._bins(ev, c["T"])).all()


@pytest.mark.parametrize("cid", IDS)
def test_rounded_flow_misses_the_gate_and_fails_the_checkers(cid):
    c = X.measured(cid)
    full, full32 = c["full"], c["full32"]
    ref = orc.objective(c["ev"], c["motion"], c["model"], c["size"], **C.ref_kwargs(c))
    assert X.rel_max(full["grad"], ref["grad"]) <= 1e-10 and abs(full["loss"] - ref["loss"]) <= 1e-10 * abs(ref["loss"])
    gap = X.rounding_gap(c)
    e_all = X.rel_max(full32["grad"], full["grad"])
    per_row = X.rounding_gap(c, per_event=True)
    print(f"[flow64 cases] {cid}: gradient at f32(flow) against the fp64 flow: {gap:.2e} in the snapped rows ({e_all:.2e} anywhere), "
          f"{(per_row > GAP).mean() if len(per_row) else 0.0:.2f} of the snapped events beyond 10 x the gate; loss {abs(full32['loss'] - full['loss']) / abs(full['loss']):.1e}")
    if cid in NO_SNAP:  # the control of the control: without a flip the two motions give the same result, far inside the gate
        assert e_all <= 1e-2 * X.TOL
        X.check_field(f"{cid} at f32(flow)", full32["grad"], full["grad"])
        return
    assert gap > GAP  # (b)
    with pytest.raises(AssertionError):  # (c)
        X.check_field(f"{cid} at f32(flow) [must fail]", full32["grad"], full["grad"])
    with pytest.raises(AssertionError):
        X.check_per_event(f"{cid} at f32(flow) [must fail]", full32["grad_events"][:, :2], full["grad_events"][:, :2])
    X.check_field(f"{cid} reference against itself", full["grad"], full["grad"])


def test_batch_case_each_flow_flips_its_own_third():
    b = X.batch_case()
    for k, F in enumerate(b["flows"]):
        assert len(b["snapped"][k]) >= 100
        g64 = orc.objective(b["ev"], F, X.DENSE, b["size"])["grad"]
        g32 = orc.objective(b["ev"], C.f32(F), X.DENSE, b["size"])["grad"]
        ix, iy = C._pixel(b["ev"][b["snapped"][k]], b["size"])
        gap = np.abs(g32[:, ix, iy] - g64[:, ix, iy]).max() / np.abs(g64).max()
        print(f"[flow64 cases] batch flow {k}: snapped {len(b['snapped'][k])}, gap {gap:.2e}")
        assert gap > GAP
        with pytest.raises(AssertionError):
            X.check_field(f"batch flow {k} at f32(flow) [must fail]", g32, g64)


def test_split_restatement():
    rng = np.random.default_rng(0)
    v = np.concatenate([rng.uniform(-200.0, 200.0, 100_000), rng.normal(0.0, 1.0, 100_000) * 10.0 ** rng.uniform(-30, 30, 100_000),
                        np.array([0.0, -0.0, 1.0, 20.0 + 2.0 ** -30, 3.0e38, 1e-40, -1e-46])])
    hi, lo = X.split_numpy(v)
    assert hi.dtype == np.float32 and lo.dtype == np.float32
    assert (hi == v.astype(np.float32)).all()
    err = np.abs(v - (hi.astype(np.float64) + lo.astype(np.float64)))
    normal = np.abs(v) >= 2.0 ** -100  # (below, lo itself is a denormal fp32 or underflows: the absolute error stays under 2^-149)
    assert (err[normal] <= 2.0 ** -47 * np.abs(v[normal])).all() and (err[~normal] <= 2.0 ** -149).all()
    print(f"[flow64 cases] split: worst |v - (hi + lo)| / |v| = {(err[normal] / np.abs(v[normal])).max():.2e} (2^-47 = {2.0 ** -47:.2e})")
    bad = np.array([np.inf, -np.inf, np.nan, 1e39, -1e300])
    hi, lo = X.split_numpy(bad)
    assert not np.isfinite(hi).any() and (lo == 0).all()
    for c in (X.built("dense-random"), X.built("voxel3")):
        hi, lo = X.split_numpy(c["motion"])
        assert (hi.astype(np.float64) == c["motion32"]).all() and (lo != 0).all()
        assert np.abs(c["motion"] - (hi.astype(np.float64) + lo.astype(np.float64))).max() <= 2.0 ** -47 * np.abs(c["motion"]).max()


@pytest.mark.parametrize("kind", list(X.PLAN_KINDS))
def test_plan_on_the_rounded_field_misses_the_gate(kind):
    """The patch plan: tests/_patch_ref.plan chained in fp64 (round32 False) against the same chain on the field rounded to fp32 -- what the
    default plan evaluates.  Gradient and Hessian-vector product with respect to x sum over a patch's pixels and still move by per cent."""
    b = X.plan_case(kind)
    e = (X.rel_max(b["grad32"], b["grad"]), X.rel_max(b["hv32"], b["hv"]))
    print(f"[flow64 cases] plan {kind}: snapped {len(b['snapped'])} of {len(b['ev'])}, rounded field against the fp64 chain: grad {e[0]:.2e} hvp {e[1]:.2e}")
    assert len(b["snapped"]) >= 100 and min(e) > GAP
    for got, ref, what in ((b["grad32"], b["grad"], "grad"), (b["hv32"], b["hv"], "hvp")):
        with pytest.raises(AssertionError):
            X.check_field(f"plan {kind} on the rounded field [must fail]", got, ref, what)
