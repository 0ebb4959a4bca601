"""csrc/cmax_batch_plan.h on the CPU: the host's cut into segments (`cut_work_list`) and the radix sort's pass plan (`radix_pass_plan`) are
plain C++17 with no HIP in them.  tests/batch_plan_check.cpp (its own main, that header and nothing else of the library) is compiled with
the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer and run as a process on a file of cases; every line it prints
must EQUAL the numpy restatements `_worklist_ref.cut` and `_sort_ref.pass_plan`.  Nothing is preloaded, nothing is loaded into Python.

The cut sees nothing of a batch but its group starts, so a case is the cumulative sum of its histogram: no events are drawn.

About the refusal (`WorkList::kMidNotAligned`): the rules cannot reach it.  `mid` is only ever set where the 3064-event aligned cut
exists (mid_n > 0: every group holds at most 3064 = seg_max events), in the branch that has n >= 522 240, no slab order and no
CMAX_NO_OWNED -- which is the definition of `owned`.  A histogram whose groups exceed 3064 with `mid` forced therefore gives status 0 and
the standard cut; test_forced_mid_on_groups_above_3064 pins that, and every cut below checks its status."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _sort_cases as SC
import _sort_ref as S
import _worklist_cases as C
import _worklist_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX_FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
STATUS_OK = 0


def knobs_of(env):
    """CutKnobs as `cut_knobs_from_env` (csrc/cmax_batch.hip) fills them from a process environment."""
    env = env or {}
    return dict(big=int(env.get("CMAX_BIG_SEG", -1)), mid=int(env.get("CMAX_MID_SEG", -1)), small_acc=int(env.get("CMAX_SMALL_ACC", -1)), free_cut=-1, seg_cap=0,
                no_owned=int("CMAX_NO_OWNED" in env), compact=int(int(env.get("CMAX_COMPACT", 1)) != 0))


def slab_histogram(hist, size, S_, seed):
    """A (tile row, slab, tile column) histogram with the tile totals of `hist`: every tile's events spread over S_ slabs."""
    ntr, ntc = C.tiles(size)
    rng = np.random.default_rng(seed)
    per = np.stack([rng.multinomial(int(v), np.full(S_, 1.0 / S_)) for v in np.asarray(hist, np.int64).reshape(-1)])  # [tile, slab]
    return per.reshape(ntr, ntc, S_).transpose(0, 2, 1).reshape(-1)


def _cut_cases():
    """(id, ntr, ntc, T, slab, group_start, env): every case of the table and every forced table, the slab-major steps, an empty batch."""
    out = []
    tables = [(c["id"], c, None) for c in C.CASES] + [(f"{C.CHILD_IDS[k]}/{c['id']}", c, C.CHILD_ENV[k]) for k, t in enumerate(C.FORCED) for c in t]
    for cid, c, env in tables:
        ntr, ntc = C.tiles(c["size"])
        hist = np.asarray(c["hist"](), np.int64).reshape(-1)
        assert hist.size == ntr * ntc * max(c["T"], 1), cid
        out.append((cid, ntr, ntc, c["T"], False, np.concatenate([[0], np.cumsum(hist)]), env))
        for what, k in c["steps"]:
            if what == "slabs" and k > 1:
                h = slab_histogram(hist, c["size"], k, c["seed"] + k)
                out.append((f"{cid}/slabs{k}", ntr, ntc, k, True, np.concatenate([[0], np.cumsum(h)]), env))
    assert {"small-rebinned-and-slabbed/slabs2", "small-rebinned-and-slabbed/slabs4", "small-empty-batch"} <= {o[0] for o in out}
    out.append(("empty-binned-T4", 2, 3, 4, False, np.zeros(25, np.int64), None))
    return out


def forced_mid_above_3064():
    """17 x 17 tiles of 3100 events (895 900 events: above 522 240, below 4M), CMAX_MID_SEG=1."""
    return ("forced-mid-groups-above-3064", 17, 17, 0, False, np.arange(290, dtype=np.int64) * 3100, {"CMAX_MID_SEG": "1"})


def _plan_cases():
    """(size, T, n, digit_bits): every (size, T, n) of tests/_sort_cases.py, the re-orderings of its chains included, and two sensors."""
    keys = set()
    for c in SC.CASES:
        keys.add((c["size"], c["T"], c["n"]))
        for _, k in c["steps"]:
            keys.add((c["size"], k, c["n"]))
    for size in ((260, 346), (720, 1280)):
        for T in (0, 10, 40):
            for n in (1, 2048, 2049, 8_000_000, 64_000_000):
                keys.add((size, T, n))
    return [(size, T, n, bits) for (size, T, n) in sorted(keys) for bits in (6, 2)]


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """Builds the program, runs it once on every case; {kind: [list of ints per case]} in the order of the case lists."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("batch_plan")
    exe, cases = str(d / "batch_plan_check"), str(d / "cases.txt")
    # The sanitizer runtimes are linked statically where the compiler has them: the shared ASan runtime refuses to start in a process
    # whose environment preloads any other library, and that must not decide this test.
    for link in (["-static-libasan", "-static-libubsan"], []):
        p = subprocess.run([cxx] + CXX_FLAGS + link + [os.path.join(ROOT, "tests", "batch_plan_check.cpp"), "-o", exe], capture_output=True, text=True)
        if p.returncode == 0:
            break
    assert p.returncode == 0, p.stderr[-3000:]
    cuts = [(c, lr) for c in _cut_cases() + [forced_mid_above_3064()] for lr in (False, True)]
    plans = _plan_cases()
    with open(cases, "w") as f:
        for (cid, ntr, ntc, T, slab, gs, env), lr in cuts:
            k = knobs_of(env)
            head = [ntr, ntc, T, int(slab), int(gs[-1]), int(lr), k["big"], k["mid"], k["small_acc"], k["free_cut"], k["seg_cap"], k["no_owned"], k["compact"]]
            f.write("cut " + " ".join(map(str, head + gs.tolist())) + "\n")
        for size, T, n, bits in plans:
            ntr, ntc = C.tiles(size)
            f.write(f"plan {ntr * ntc} {T} {n} {bits}\n")
    p = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, f"rc {p.returncode}\n{p.stdout[-1000:]}\n{p.stderr[-4000:]}"
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == f"done {len(cuts) + len(plans)}", lines[-1]
    got = {"cut": [], "plan": []}
    for line in lines[:-1]:
        kind, *vals = line.split()
        got[kind].append([int(v) for v in vals])
    assert len(got["cut"]) == len(cuts) and len(got["plan"]) == len(plans)
    return {"cut": dict(zip([(c[0], lr) for c, lr in cuts], got["cut"])), "plan": dict(zip(plans, got["plan"]))}


def check_cut(case, long_runs, vals):
    cid, ntr, ntc, T, slab, gs, env = case
    status, big, mid, owned, small_acc, compact, seg_max, nseg, nrows = vals[:9]
    segs = np.array(vals[9:9 + 4 * nseg], np.int64).reshape(-1, 4)
    rows = vals[9 + 4 * nseg:]
    assert len(rows) == nrows
    want_segs, want_flags, want_seg_max = R.cut(gs, int(gs[-1]), ntr, ntc, T, slab, long_runs, env)
    assert status == STATUS_OK, cid
    np.testing.assert_array_equal(segs, want_segs, err_msg=cid)
    got_flags = dict(big=bool(big), mid=bool(mid), owned=bool(owned), small_accumulators=bool(small_acc), slab_major=bool(slab and T > 0), compact=bool(compact),
                     long_runs=bool(long_runs))
    assert tuple(got_flags) == R.FLAGS and got_flags == want_flags, (cid, got_flags, want_flags)
    assert seg_max == want_seg_max, cid
    if owned:  # the first segment of every source tile row, and the end of the list
        Tg = T if T > 0 else 1
        first_of_row = [int(np.flatnonzero(segs[:, 2] == r * ntc * Tg)[0]) for r in range(ntr)]
        assert rows == first_of_row + [nseg], cid
    else:
        assert rows == [], cid
    return got_flags


CUT_CASES = _cut_cases()


@pytest.mark.parametrize("long_runs", [False, True], ids=["short-runs", "long-runs"])
@pytest.mark.parametrize("case", CUT_CASES, ids=[c[0] for c in CUT_CASES])
def test_cut_equals_the_restatement(results, case, long_runs):
    check_cut(case, long_runs, results["cut"][(case[0], long_runs)])


def test_forced_mid_on_groups_above_3064(results):
    """No refusal and no mid list (see the module's docstring): the standard cut, groups split into equal parts."""
    case = forced_mid_above_3064()
    for lr in (False, True):
        flags = check_cut(case, lr, results["cut"][(case[0], lr)])
        assert not flags["mid"] and not flags["owned"] and not flags["big"]
        assert results["cut"][(case[0], lr)][6] == R.SEG_STD


PLAN_CASES = _plan_cases()


@pytest.mark.parametrize("size,T,n,bits", PLAN_CASES, ids=[f"{s[0]}x{s[1]}-T{T}-n{n}-bits{b}" for s, T, n, b in PLAN_CASES])
def test_pass_plan_equals_the_restatement(results, size, T, n, bits):
    planned, P, fine, nwg, rng, need, *rest = results["plan"][(size, T, n, bits)]
    nb, sh = rest[:P], rest[P:]
    want = S.pass_plan(size, T, n, bits)
    assert planned == 1
    assert dict(P=P, nb=nb, fine=bool(fine), nwg=nwg, range=rng) == {k: want[k] for k in ("P", "nb", "fine", "nwg", "range")}
    assert len(sh) == P and sh == [sum(nb[:q]) for q in range(P)]
    assert need == (1 << max(nb)) * nwg + 1
