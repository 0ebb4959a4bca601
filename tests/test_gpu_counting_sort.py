"""The two-level counting sort (csrc/cmax_sort_kernels.h: k_bucket_hist, k_bucket_scatter, k_tile_sort, k_run_time_sort, k_slab_offsets,
k_slab_regroup -- the order of every batch below 8M events) at SMALL sizes, on every branch: the packed sequence word for word against
the numpy restatement of tests/_sort_ref.py, in the canonical form `R.compare_counting` writes down (keys and group starts element for
element, the words of one key as a multiset, the pixel runs of 2 .. 192 events of an un-binned handle by fp32 time).  Nothing about
the order has a tolerance; the evaluations are held to the oracle at the project's plain gate (1e-4 of the largest entry).

Two child processes (tests/_radix_worker.py with tests/_counting_cases.py as its table), one after the other and no second one after
a failed first, each started with CMAX_SORT, CMAX_RS_BITS and CMAX_NO_RUN_SORT removed from the inherited environment:
    default   nothing set
    norun     CMAX_NO_RUN_SORT=1: what k_tile_sort alone leaves on un-binned handles (every pixel run held as a multiset)
Each runs the whole case table once; the tests below are parametrised over (child, case).  After re-binning the expectation is a
function of the ORIGINAL batch and the new bin count alone, not of the packed order in front of it.

Limits: five times the measured duration of the radix test's bits6 child, times the ratio of case counts (this table over the radix
table), rounded up to whole seconds.  Durations on an MI355X (profiles/counting_small.txt):
    bits6 radix child   2.9 s for 49 cases; this table has 65: 5 * 2.9 * 65 / 49 = 19.3 -> limit 20 s for each child
    default             3.3 s
    norun               3.0 s"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc  # noqa: E402

import _counting_cases as C  # noqa: E402
import _sort_ref as R  # noqa: E402
from _weight_grad_ref import weight_grad_objective  # noqa: E402
from _weighted_ref import weighted_objective  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
CHILD_LIMIT_S = (20, 20)

_child_failed = []
_child_out = {}
_worst = {}


def rel_max(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _run_child(k, tmp_path_factory):
    if k in _child_out:
        return _child_out[k]
    if _child_failed:
        pytest.fail(f"not started: an earlier counting-sort child failed ({_child_failed[0]})")
    env = dict(os.environ)
    for name in C.ENV_NAMES:
        env.pop(name, None)
    env.update(C.CHILDREN[k])
    out = str(tmp_path_factory.mktemp("counting") / f"{C.CHILD_IDS[k]}.npz")
    expect = [f"{name}={C.CHILDREN[k].get(name, '')}" for name in C.ENV_NAMES]
    t0 = time.time()
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_radix_worker.py"), out, "_counting_cases"] + expect, env=env, cwd=ROOT,
                           capture_output=True, text=True, timeout=CHILD_LIMIT_S[k])
    except subprocess.TimeoutExpired as e:
        _child_failed.append(f"{C.CHILD_IDS[k]}: timed out")
        pytest.fail(f"counting-sort child {C.CHILD_IDS[k]} exceeded {CHILD_LIMIT_S[k]} s\n{e.stderr}")
    print(f"[counting sort] child {C.CHILD_IDS[k]} {C.CHILDREN[k]}: {time.time() - t0:.1f} s for {len(C.CASES)} cases")
    if p.returncode != 0:
        _child_failed.append(f"{C.CHILD_IDS[k]}: exit status {p.returncode}")
        pytest.fail(f"counting-sort child {C.CHILD_IDS[k]} ended with status {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    _child_out[k] = dict(np.load(out))
    return _child_out[k]


# ---- what every step of a case must leave (computed once per case, shared by both children, never written to) --------------------------
_expected = {}


def expected_steps(c):
    if c["id"] not in _expected:
        tmin, tmax = c["extremes"] if c["extremes"] else (None, None)
        _expected[c["id"]] = [R.counting_expected(C.batch(c), c["size"], T, c["keep_outside"], tmin, tmax, slabs=slabs) for T, slabs in C.step_bins(c)]
    return _expected[c["id"]]


_refs = {}


def reference(c, e):
    """The fp64 value of one evaluation of a case: the oracle on the events that survive, as the other GPU tests call it."""
    k = (c["id"], e["tag"])
    if k not in _refs:
        ev = np.asarray(C.batch(c), dtype=np.float64)
        ok = R.classify(ev, c["size"], c["keep_outside"])[0]
        w, m = C.weights(c), C.motion(c, e)
        kw = dict(cost=e["cost"], sigma=e["sigma"], outer_padding=c["pad"])
        if e["weight_grad"]:
            _refs[k] = weight_grad_objective(ev[ok], m, e["model"], c["size"], w[ok], **kw)
        elif w is not None:
            _refs[k] = weighted_objective(ev[ok], m, e["model"], c["size"], w[ok], **kw)
        else:
            _refs[k] = orc.objective(ev[ok], m, e["model"], c["size"], **kw)
    return _refs[k]


def check_evaluation(tag, child, c, e, got, key):
    ref = reference(c, e)
    loss, grad = float(got[key + "/loss"]), got[key + "/grad"]
    errs = {"loss": rel_max(loss, ref["loss"]), "grad": rel_max(grad, ref["grad"])}
    if key + "/iwe" in got:
        errs["iwe"] = rel_max(got[key + "/iwe"], ref["iwes"]["iwe"])
    if e["weight_grad"]:
        ok = R.classify(C.batch(c), c["size"], c["keep_outside"])[0]
        gw = np.zeros(ok.size)   # dL/dw in the caller's order: events that were not packed get 0
        gw[ok] = ref["grad_w"]
        errs["grad_w"] = rel_max(got[key + "/grad_w"], gw)
    print(f"[counting sort] {tag} {e['tag']}: rel err " + " ".join(f"{n} {v:.2e}" for n, v in errs.items()))
    for n, v in errs.items():
        if v > _worst.get((child, n), (0.0, ""))[0]:
            _worst[(child, n)] = (v, f"{tag} {e['tag']}")
    assert all(v <= TOL for v in errs.values()), (tag, e["tag"], errs)


@pytest.mark.parametrize("cid", [c["id"] for c in C.CASES])
@pytest.mark.parametrize("child", range(len(C.CHILDREN)), ids=C.CHILD_IDS)
def test_counting_sort(child, cid, tmp_path_factory):
    got = _run_child(child, tmp_path_factory)
    c = C.BY_ID[cid]
    steps = expected_steps(c)
    for s, x in enumerate(steps):
        key = f"{cid}/{s}"
        tag = f"{C.CHILD_IDS[child]} {cid} step {s} (T = {x['T']}{' slabs' if x['slabs'] else ''})"
        packed, gs, info = got[key + "/packed"], got[key + "/gs"], got[key + "/info"]
        if x["idx"].size == 0:
            packed = packed[:0]
        R.compare_counting(tag, packed, gs, info, x, c["size"], run_sorted=C.CHILD_RUN_SORTED[child], declared_long=c["long"] if x["T"] == 0 else ())
        if not c["distinct"]:  # tied times: no word of the packed sequence is absent from the expectation
            assert np.isin(R.words(packed[:, 0], packed[:, 1]), R.words(x["word0"], x["word1"])).all(), f"{tag}: a word no event of the batch has"
        if s > 0 and x["T"] == 0:  # back on an un-binned order: the residual bytes of step 0, recomputed from tau64
            first = got[f"{cid}/0/packed"]
            assert c["T"] == 0
            np.testing.assert_array_equal(np.sort(R.words(packed[:, 0], packed[:, 1])), np.sort(R.words(first[:, 0], first[:, 1])),
                                          err_msg=f"{tag}: words (residual byte included) against step 0")
        for e in c["evals"].get(s, []):
            if cid == "all-dropped":
                assert float(got[f"{key}/{e['tag']}/loss"]) == 0.0 and np.abs(got[f"{key}/{e['tag']}/grad"]).sum() == 0.0
            else:
                check_evaluation(tag, child, c, e, got, f"{key}/{e['tag']}")
    x = steps[0]
    if cid == "all-dropped":
        assert got[f"{cid}/0/info"][0] == 0 and not got[f"{cid}/0/gs"].any() and got[f"{cid}/0/gs"].size == R.n_groups(c["size"], 0) + 1
    if cid.startswith("dropped"):
        assert x["dropped"] == c["n"] - int(0.4 * c["n"]) + 7 + (2 if c.get("inf_times") else 0) and x["outside"] == 0
    if cid == "kept-outside":
        assert x["outside"] == 300 and x["dropped"] == 0
    if cid.startswith("fractional"):
        assert x["fractional"]
    if cid == "tied/one-time":
        assert (got[f"{cid}/0/packed"][:, 1] == 0).all() and (got[f"{cid}/0/packed"][:, 0] >> 24 == 0).all()
    if cid == "many-tiles/last-tile":
        np.testing.assert_array_equal(got[f"{cid}/0/gs"], [0] * R.n_groups(c["size"], 0) + [c["n"]])  # 4224 empty tiles in front


def test_summary():
    """Printed last: the worst evaluation errors of each child (what profiles/counting_small.txt records)."""
    for (child, n), (v, where) in sorted(_worst.items()):
        print(f"[counting sort] worst {n:6s} child {C.CHILD_IDS[child]:8s} {v:.2e}  ({where})")
    assert all(v <= TOL for v, _ in _worst.values())
