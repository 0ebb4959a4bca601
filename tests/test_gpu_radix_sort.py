"""The stable LSD radix sort (csrc/cmax_radix_sort.h, the radix branch of sort_events in csrc/cmax_batch.hip) at SMALL sizes, on every branch: the packed
order bit for bit against the numpy restatement of tests/_sort_ref.py.  A stable sort has one right answer per input, so nothing here
has a tolerance except the evaluations, which are held to the oracle at the project's plain gate (1e-4 of the largest entry).

Two child processes (tests/_radix_worker.py), one after the other and no second one after a failed first: CMAX_SORT=radix, and
CMAX_SORT=radix CMAX_RS_BITS=2 (other digit widths, other pass counts: both parities of P on both sensor sizes).  Each runs the whole
case table of tests/_sort_cases.py once; the tests below are parametrised over (child, case).  The inputs are shuffled in time: the
counting sort followed by k_run_time_sort would leave a pixel's events by time, not in input order, so a pass of the exact-order check
also proves that the child took the radix pipeline.

Durations on an MI355X, measured on a build before the pass-plan fix of sort_events and not yet on the present one (see
profiles/radix_small.txt); limits five times that, rounded up to whole seconds:
    bits6   CMAX_SORT=radix                  3.0 s   -> limit 15 s
    bits2   CMAX_SORT=radix CMAX_RS_BITS=2   2.8 s   -> limit 14 s"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import event_based_optical_flow_amd as E  # noqa: E402
from oracle import oracle as orc  # noqa: E402

import _sort_cases as C  # noqa: E402
import _sort_ref as R  # noqa: E402
from _weight_grad_ref import weight_grad_objective  # noqa: E402
from _weighted_ref import weighted_objective  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
CHILD_LIMIT_S = (15, 14)

_child_failed = []
_child_out = {}


def rel_max(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _run_child(k, tmp_path_factory):
    if k in _child_out:
        return _child_out[k]
    if _child_failed:
        pytest.fail(f"not started: an earlier radix child failed ({_child_failed[0]})")
    env = dict(os.environ)
    for name in ("CMAX_SORT", "CMAX_RS_BITS", "CMAX_NO_RUN_SORT"):
        env.pop(name, None)
    env.update(C.CHILDREN[k])
    out = str(tmp_path_factory.mktemp("radix") / f"{C.CHILD_IDS[k]}.npz")
    t0 = time.time()
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_radix_worker.py"), out], env=env, cwd=ROOT, capture_output=True,
                           text=True, timeout=CHILD_LIMIT_S[k])
    except subprocess.TimeoutExpired as e:
        _child_failed.append(f"{C.CHILD_IDS[k]}: timed out")
        pytest.fail(f"radix child {C.CHILDREN[k]} exceeded {CHILD_LIMIT_S[k]} s\n{e.stderr}")
    print(f"[radix sort] child {C.CHILDREN[k]}: {time.time() - t0:.1f} s")
    if p.returncode != 0:
        _child_failed.append(f"{C.CHILD_IDS[k]}: exit status {p.returncode}")
        pytest.fail(f"radix child {C.CHILDREN[k]} ended with status {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    _child_out[k] = dict(np.load(out))
    return _child_out[k]


# ---- what every step of a case must leave (computed once per case, shared by both children) ----------------------------------------
_expected = {}


def expected_steps(c):
    """Per step: dict(idx, word0, word1, group_start, T, slab) -- step 0 from the raw batch, every later step from the PREVIOUS packed
    sequence (the re-sort reads the packed arrays, so its input order is the previous output order)."""
    if c["id"] in _expected:
        return _expected[c["id"]]
    ev, size = C.batch(c), c["size"]
    ntc = (size[1] + 15) // 16
    tmin, tmax = c["extremes"] if c["extremes"] else (None, None)
    x = R.expected_packed(ev, size, c["T"], c["keep_outside"], tmin, tmax)
    steps = [dict(x, T=c["T"], slab=False)]
    for what, k in c["steps"]:
        p = steps[-1]
        T = k if k > 1 or what == "bins" else 0
        o = R.resort(p["row"], p["col"], p["tau64"], T, ntc)
        row, col, tau, idx, w1 = p["row"][o], p["col"][o], p["tau64"][o], p["idx"][o], p["word1"][o]
        groups = R.group_of(row, col, tau, ntc, T)
        if what == "slabs" and T > 0:
            o2, g2 = R.slab_regroup(row, col, tau, T, ntc)
            row, col, tau, idx, w1, groups = row[o2], col[o2], tau[o2], idx[o2], w1[o2], g2[o2]
        word0 = row | (col << 12) | ((R.voxel_bin(tau, T) << 24) if T > 0 else 0)
        steps.append({"idx": idx, "row": row, "col": col, "tau64": tau, "word0": word0, "word1": w1, "T": T, "slab": what == "slabs" and T > 0,
                      "group_start": R.group_starts(groups, R.n_groups(size, T)), "dropped": x["dropped"], "outside": x["outside"],
                      "fractional": x["fractional"]})
    _expected[c["id"]] = steps
    return steps


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


_counting = {}


def counting_sort(c):
    """The same batch through the DEFAULT pipeline (the counting sort at these sizes), in this process: (sorted 64-bit words, residual
    byte included; batch_info)."""
    if c["id"] not in _counting:
        h = E.CMaxHandle(c["size"], c["pad"]).set_keep_outside(c["keep_outside"]).set_events(C.batch(c), on_dropped="ignore")
        packed, _ = h.packed_events()
        info = h.batch_info()
        h.close()
        _counting[c["id"]] = (np.sort((packed[:, 0] << 32) | packed[:, 1]), info)
    return _counting[c["id"]]


def check_exact_order(tag, c, x, packed, gs, info):
    """Packed event i IS input event idx[i]: pixel, word 1 and (binned handles) the time bin; group starts element for element."""
    ev = C.batch(c)
    assert packed.shape[0] == x["idx"].size, (tag, packed.shape[0], x["idx"].size)
    assert info[0] == x["idx"].size and info[1] == x["dropped"] and bool(info[2]) == x["fractional"] and info[3] == x["outside"], (tag, info)
    row, col = packed[:, 0] & 0xFFF, (packed[:, 0] >> 12) & 0xFFF
    _, erow, ecol, _ = R.classify(ev, c["size"], c["keep_outside"])
    np.testing.assert_array_equal(row, erow[x["idx"]], err_msg=f"{tag}: row")
    np.testing.assert_array_equal(col, ecol[x["idx"]], err_msg=f"{tag}: column")
    np.testing.assert_array_equal(packed[:, 1], x["word1"], err_msg=f"{tag}: word 1")
    if x["T"] > 0:
        np.testing.assert_array_equal(packed[:, 0] >> 24, R.voxel_bin(x["tau64"], x["T"]), err_msg=f"{tag}: top byte against voxel_bin")
        np.testing.assert_array_equal(packed[:, 0], x["word0"], err_msg=f"{tag}: word 0")
    else:  # un-binned: the top byte is the residual of tau64 beyond fp32 (tau_residual8), computed from the same tau64 by both pipelines
        np.testing.assert_array_equal(packed[:, 0] >> 24, R.tau_residual8(x["tau64"]), err_msg=f"{tag}: top byte against tau_residual8")
        np.testing.assert_array_equal(packed[:, 0] & 0xFFFFFF, x["word0"], err_msg=f"{tag}: word 0")
    np.testing.assert_array_equal(gs, x["group_start"], err_msg=f"{tag}: group starts")


def check_evaluation(tag, c, e, got, key):
    ref = reference(c, e)
    loss, grad = float(got[key + "/loss"]), got[key + "/grad"]
    errs = {"loss": abs(loss - ref["loss"]) / abs(ref["loss"]), "grad": rel_max(grad, ref["grad"])}
    if key + "/iwe" in got:
        errs["iwe"] = rel_max(got[key + "/iwe"], ref["iwes"]["iwe"])
    if e["weight_grad"]:
        errs["grad_w"] = rel_max(got[key + "/grad_w"], _scatter(c, ref["grad_w"]))
    print(f"[radix sort] {tag} {e['tag']}: rel err " + " ".join(f"{n} {v:.2e}" for n, v in errs.items()))
    assert all(v <= TOL for v in errs.values()), (tag, e["tag"], errs)


def _scatter(c, gw_surv):
    """dL/dw in the caller's order: events that were not packed get 0."""
    ok = R.classify(C.batch(c), c["size"], c["keep_outside"])[0]
    out = np.zeros(ok.size)
    out[ok] = gw_surv
    return out


@pytest.mark.parametrize("cid", [c["id"] for c in C.CASES])
@pytest.mark.parametrize("child", range(len(C.CHILDREN)), ids=C.CHILD_IDS)
def test_radix_sort(child, cid, tmp_path_factory):
    got = _run_child(child, tmp_path_factory)
    c = C.BY_ID[cid]
    ev, size = C.batch(c), c["size"]
    ntc = (size[1] + 15) // 16
    steps = expected_steps(c)
    plans = []
    for s, x in enumerate(steps):
        key = f"{cid}/{s}"
        tag = f"{C.CHILD_IDS[child]} {cid} step {s}"
        packed, gs, info = got[key + "/packed"], got[key + "/gs"].astype(np.int64), got[key + "/info"]
        plans.append(R.plan_text(size, x["T"], c["n"] if s == 0 else steps[0]["idx"].size, C.CHILD_DIGIT_BITS[child], x["slab"], s > 0))
        check_exact_order(tag, c, x, packed, gs, info)
        if x["slab"]:
            prev = got[f"{cid}/{s - 1}/packed"]
            np.testing.assert_array_equal(np.sort(((packed[:, 0] & 0xFFFFFF) << 32) | packed[:, 1]), np.sort(((prev[:, 0] & 0xFFFFFF) << 32) | prev[:, 1]),
                                          err_msg=f"{tag}: (pixel, time) multiset")
            np.testing.assert_array_equal(np.sort((packed[:, 0] << 32) | packed[:, 1]), np.sort((x["word0"] << 32) | x["word1"]), err_msg=f"{tag}: word multiset")
            group = np.searchsorted(gs, np.arange(packed.shape[0]), side="right") - 1  # every group lies in one (tile row, slab, tile column)
            row, col, S = packed[:, 0] & 0xFFF, (packed[:, 0] >> 12) & 0xFFF, x["T"]
            np.testing.assert_array_equal(group, ((row >> 4) * S + (packed[:, 0] >> 24)) * ntc + (col >> 4), err_msg=f"{tag}: slab-major groups")
        for e in c["evals"].get(s, []):
            if cid == "all-dropped":
                assert float(got[f"{key}/{e['tag']}/loss"]) == 0.0 and np.abs(got[f"{key}/{e['tag']}/grad"]).sum() == 0.0
            else:
                check_evaluation(tag, c, e, got, f"{key}/{e['tag']}")
    print(f"[radix plan] {C.CHILD_IDS[child]} {cid:28s} " + "; ".join(plans))
    x = steps[0]
    row, col = x["row"], x["col"]
    if cid.startswith("plain"):
        # the expected order is NOT by time inside pixels: the counting sort + k_run_time_sort could not have produced it
        same = (row[1:] == row[:-1]) & (col[1:] == col[:-1])
        assert (x["tau64"][1:][same] < x["tau64"][:-1][same]).sum() > 1000
        np.testing.assert_array_equal(np.sort((got[f"{cid}/0/packed"][:, 0] << 32) | got[f"{cid}/0/packed"][:, 1]), counting_sort(c)[0],
                                      err_msg="the two pipelines hold different 64-bit words")
    if cid == "hot-pixel":
        for px, count in (((21, 37), 6000), ((21, 38), 3000)):
            run = x["idx"][(row == px[0]) & (col == px[1])]
            assert run.size >= count and (np.diff(run) > 0).all()  # the long runs come out in input order
            packed = got[f"{cid}/0/packed"]
            sel = ((packed[:, 0] & 0xFFF) == px[0]) & (((packed[:, 0] >> 12) & 0xFFF) == px[1])
            np.testing.assert_array_equal(packed[sel, 1], R.normalised_time(ev)[1].view(np.uint32).astype(np.int64)[run])
    if cid.startswith("one-pixel"):
        np.testing.assert_array_equal(got[f"{cid}/0/gs"], [0, c["n"]])
    if cid.startswith("dropped"):
        assert x["dropped"] == c["n"] - int(0.4 * c["n"]) + 7 + (2 if c.get("inf_times") else 0) and x["outside"] == 0
        # the drop is RawSource::classify's, shared by both pipelines: the default one (the counting sort, in this process) packs the same
        # events -- same counts, same multiset of 64-bit words
        words, info = counting_sort(c)
        assert info["packed"] == x["idx"].size and info["dropped"] == x["dropped"] and info["outside"] == 0, info
        np.testing.assert_array_equal(np.sort((got[f"{cid}/0/packed"][:, 0] << 32) | got[f"{cid}/0/packed"][:, 1]), words,
                                      err_msg="the two pipelines packed different events")
        assert np.isfinite(got[f"{cid}/0/packed"][:, 1].astype(np.uint32).view(np.float32)).all()
    if cid == "kept-outside":
        assert x["outside"] == 300 and x["dropped"] == 0
    if cid == "all-dropped":
        assert got[f"{cid}/0/info"][0] == 0 and not got[f"{cid}/0/gs"].any() and got[f"{cid}/0/gs"].size == R.n_groups(size, 0) + 1
    if cid.startswith("fractional"):
        assert x["fractional"]
