"""The host's cut into segments (`build_segments`, csrc/cmax_batch.hip; its rules: `cut_work_list`, csrc/cmax_batch_plan.h) and the compact copy of big segments (`k_pack_compact`,
csrc/cmax_event_kernels.inc), EXACTLY, in every regime: the read-backs cmax_debug_work_list / cmax_debug_compact_events against the
numpy restatement of tests/_worklist_ref.py.

Per case of tests/_worklist_cases.py (batches made from per-group histograms, the smallest that reach each branch) and per step:
  * segments, flags and seg_max equal `cut(...)`, computed from the packed events and group starts the library itself reports;
  * `check_invariants` -- what the event kernels require of any cut -- holds on the read-back;
  * work_list_info() and batch_info()["owned_groups"] report what the read-back holds;
  * where the handle holds a compact copy the regions equal `compact_expected` byte for byte and the packing flag is 0; where it does
    not, cmax_debug_compact_events answers CMAX_ESTATE.
One evaluation per regime ties the exact cut to a right answer: 2-DoF image_variance (dense image_variance too on owned lists) against
oracle.objective (binned lists: the voxel objective, a motion per time bin) at the project's plain gate, 1e-4 of the largest entry, on loss and gradient; one batch runs under the default cut
and under CMAX_BIG_SEG=1 / CMAX_NO_OWNED=1.

The forced layouts run in child processes (tests/_worklist_worker.py: the switches are read once per process), one after the other
and none after a failed one.  Durations on an MI355X (start-up of torch and the library included), limits five times that and at
least 60 s, as tests/test_gpu_hvp_parity.py derives its own (the whole module: 20 s, no test above 3.1 s):
    big            CMAX_BIG_SEG=1                  2.9 s   -> limit 60 s
    big-nocompact  CMAX_BIG_SEG=1 CMAX_COMPACT=0   2.8 s   -> limit 60 s
    mid            CMAX_MID_SEG=1                  2.8 s   -> limit 60 s
    no-owned       CMAX_NO_OWNED=1                 3.0 s   -> limit 60 s
    small-acc-0    CMAX_SMALL_ACC=0                3.0 s   -> limit 60 s
(profiles/work_list_small.txt: the '[work list]' lines this module prints with -s.)

What the cases could NOT be, by the rules of the cut itself: below 522 240 events no list is owned and the cap n / 512 (at most 1020)
holds for big segments too, so a forced big list of a few tens of thousands of events has segments of at most 256 events, 3 tiles wide;
segments 6 tiles wide and full 4088-event segments need 522 240 events -- the ratio cases (natural) and the forced 534k-event batch."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import event_based_optical_flow_amd as E  # noqa: E402,F401
from oracle import oracle as orc  # noqa: E402

import _worklist_cases as C  # noqa: E402
import _worklist_ref as R  # noqa: E402
import _worklist_worker as W  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
ESTATE = -3
CHILD_LIMIT_S = (60, 60, 60, 60, 60)
MODELS = {"2dof": "2d-translation", "dense": "dense-flow", "voxel": "dense-flow-voxel"}

_child_failed = []
_child_out = {}
_here = {}
_refs = {}


def rel_max(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _run_child(k, tmp_path_factory):
    if k in _child_out:
        return _child_out[k]
    if _child_failed:
        pytest.fail(f"not started: an earlier work-list child failed ({_child_failed[0]})")
    env = dict(os.environ)
    for name in C.SWITCHES:
        env.pop(name, None)
    env.update(C.CHILD_ENV[k])
    out = str(tmp_path_factory.mktemp("worklist") / f"{C.CHILD_IDS[k]}.npz")
    t0 = time.time()
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_worklist_worker.py"), out, str(k)], env=env, cwd=ROOT, capture_output=True,
                           text=True, timeout=CHILD_LIMIT_S[k])
    except subprocess.TimeoutExpired as e:
        _child_failed.append(f"{C.CHILD_IDS[k]}: timed out")
        pytest.fail(f"work-list child {C.CHILD_ENV[k]} exceeded {CHILD_LIMIT_S[k]} s\n{e.stderr}")
    print(f"[work list] child {C.CHILD_IDS[k]} {C.CHILD_ENV[k]}: {time.time() - t0:.1f} s")
    if p.returncode != 0:
        _child_failed.append(f"{C.CHILD_IDS[k]}: exit status {p.returncode}")
        pytest.fail(f"work-list child {C.CHILD_ENV[k]} ended with status {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    _child_out[k] = dict(np.load(out))
    return _child_out[k]


def _run_here(c):
    """The case in this process (no switch set), once."""
    if c["id"] not in _here:
        for name in C.SWITCHES:
            assert name not in os.environ, f"{name} is set: the default cut cannot be tested in this process"
        out = {}
        W.run_case(out, "", c)
        _here[c["id"]] = out
    return _here[c["id"]]


def reference(c, model):
    root = C.BY_ID[c["batch_of"]] if c["batch_of"] else c
    k = (root["id"], model)
    if k not in _refs:
        _refs[k] = orc.objective(np.asarray(C.batch(c)), C.motion(c, model), MODELS[model], c["size"], cost="image_variance", sigma=0)
    return _refs[k]


def step_layouts(c):
    """(T, slab) of the handle after every step."""
    out = [(c["T"], False)]
    for what, k in c["steps"]:
        out.append((k, False) if what == "bins" else ((k if k > 1 else 0, k > 1) if what == "slabs" else (0, False)))
    return out


def check_step(tag, got, key, size, T, slab, env):
    packed, gs, segs = got[key + "/packed"], got[key + "/gs"].astype(np.int64), got[key + "/segs"]
    flags = {name: bool(v) for name, v in zip(R.FLAGS, got[key + "/flags"])}
    seg_max, info = int(got[key + "/seg_max"]), got[key + "/info"]
    ntr, ntc = C.tiles(size)
    n = packed.shape[0]
    long_runs = R.long_runs_of(packed, T)
    want_segs, want_flags, want_max, why = R.cut_with_reasons(gs, n, ntr, ntc, T, slab, long_runs, env)
    print(f"[work list] {tag:78s} n={n} groups={gs.size - 1} segments={segs.shape[0]} seg_max={seg_max} "
          f"flags={'+'.join(k for k in R.FLAGS if flags[k]) or '-'} rule={why['big_rule']} cap={why['seg_cap']} split={why['split_groups']}")
    assert flags == want_flags, (tag, flags, want_flags, why)
    assert seg_max == want_max, (tag, seg_max, want_max, why)
    assert segs.shape == want_segs.shape, (tag, segs.shape, want_segs.shape, why)
    np.testing.assert_array_equal(segs, want_segs, err_msg=f"{tag}: segments")
    R.check_invariants(segs, flags, packed, gs, dict(ntr=ntr, ntc=ntc, T=T, slab=slab, seg_max=seg_max))
    # reporting: [packed, owned_groups, segments, segment_events, small_accumulators, n_events]
    assert list(info) == [n, int(flags["owned"]), segs.shape[0], seg_max, int(flags["small_accumulators"]), n], (tag, list(info))
    if flags["compact"]:
        assert int(got[key + "/compact_flag"]) == 0, f"{tag}: k_pack_compact flagged an event outside its segment's strip"
        regions = got[key + "/compact"]
        want = R.compact_expected(packed, segs, ntc)
        assert regions.shape == want.shape
        if not np.array_equal(regions, want):
            bad = np.argwhere(regions.view(np.uint32) != want.view(np.uint32))
            s, wd = bad[0]
            raise AssertionError(f"{tag}: {bad.shape[0]} compact words differ; first: segment {s} {segs[s].tolist()} word {wd}: "
                                 f"{regions.view(np.uint32)[s, wd]:#010x}, expected {want.view(np.uint32)[s, wd]:#010x}")
    else:
        assert int(got[key + "/compact_error"]) == ESTATE, f"{tag}: no compact copy, yet cmax_debug_compact_events did not answer CMAX_ESTATE"
    return flags, why


def check_case(prefix, c, got, env):
    for s, (T, slab) in enumerate(step_layouts(c)):
        size = c["size"]
        flags, why = check_step(f"{prefix}{c['id']} step {s}", got, f"{prefix}{c['id']}/{s}", size, T, slab, env)
        if s == 0:
            said = dict(flags, **why)
            for name, want in c["expect"].items():
                assert said[name] == want, (c["id"], name, said[name], want)
    for model in c["evals"]:
        ref = reference(c, model)
        k = f"{prefix}{c['id']}/0/{model}"
        e_loss, e_grad = abs(float(got[k + "/loss"]) - ref["loss"]) / abs(ref["loss"]), rel_max(got[k + "/grad"], ref["grad"])
        print(f"[work list] {prefix}{c['id']} {model} image_variance: rel err loss {e_loss:.2e} grad {e_grad:.2e}")
        assert e_loss <= TOL and e_grad <= TOL, (c["id"], model, e_loss, e_grad)


@pytest.mark.parametrize("cid", [c["id"] for c in C.CASES])
def test_default_cut(cid):
    c = C.BY_ID[cid]
    check_case("", c, _run_here(c), None)


FORCED = [(k, c["id"]) for k, table in enumerate(C.FORCED) for c in table]


@pytest.mark.parametrize("child,cid", FORCED, ids=[f"{C.CHILD_IDS[k]}/{cid}" for k, cid in FORCED])
def test_forced_cut(child, cid, tmp_path_factory):
    got = _run_child(child, tmp_path_factory)
    check_case(f"{C.CHILD_IDS[child]}/", C.BY_ID[f"{C.CHILD_IDS[child]}/{cid}"], got, C.CHILD_ENV[child])


def test_an_empty_batch_makes_no_cut():
    """cmax_set_events with no events cuts nothing: zero segments; the flags and seg_max stay what the last cut left, and a compact
    copy cannot be read back."""
    c = C.BY_ID["small-n-255"]
    h = E.CMaxHandle(c["size"]).set_events(np.array(C.batch(c)), tmin=0.0, tmax=1.0, on_dropped="ignore")
    before = h.work_list()
    assert before[0].shape[0] > 0
    h.set_events(np.zeros((0, 4)), tmin=0.0, tmax=1.0, on_dropped="ignore")
    segs, flags, seg_max = h.work_list()
    assert segs.shape == (0, 4) and flags == before[1] and seg_max == before[2] and h.work_list_info()["segments"] == 0
    with pytest.raises(W.CmaxError) as e:
        h.compact_events()
    assert e.value.code == ESTATE
    h.close()
