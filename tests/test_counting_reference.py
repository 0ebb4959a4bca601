"""The numpy restatement of what the counting sort must leave (tests/_sort_ref.py: tau_residual8, counting_expected, compare_counting)
and the case table of tests/_counting_cases.py, held to themselves without a GPU: what tests/test_gpu_counting_sort.py compares the
kernels of csrc/cmax_sort_kernels.h with word for word."""
import numpy as np
import pytest

import _counting_cases as C
import _sort_ref as R


def test_residual_byte_reconstructs_tau64():
    """(word 1, byte) give tau64 back to ulp32 / 256: the rounding of the byte costs half a unit, its clip to +127 (a residual of
    exactly half an ulp upwards) at most one."""
    rng = np.random.default_rng(1)
    tau = np.concatenate([rng.uniform(0, 1, 200_000), [0.0, 1.0, 0.5, 2.0 ** -100]])
    byte = R.tau_residual8(tau)
    assert byte.min() >= 0 and byte.max() <= 255 and np.unique(byte).size == 256
    np.testing.assert_array_equal(byte[-4:-1], [0, 0, 0])
    word1 = tau.astype(np.float32).view(np.uint32).astype(np.int64)
    back, unit = R.tau_refined(word1, byte)
    ulp32 = np.spacing(np.abs(tau.astype(np.float32))).astype(np.float64)
    big = tau >= 2.0 ** -94
    np.testing.assert_array_equal(unit[big] * 256, ulp32[big])
    assert (np.abs(back - tau)[big] <= ulp32[big] / 256).all()
    assert np.abs(back - tau)[big].max() > np.abs(tau.astype(np.float32) - tau)[big].max() / 300   # (and the bound is not slack by much)
    assert (np.abs(tau.astype(np.float32).astype(np.float64) - tau)[big] > ulp32[big] / 256).mean() > 0.9  # without the byte: far off
    assert byte[-1] == 0 and back[-1] == np.float32(2.0 ** -100)  # below 2^-95 nothing is refined


def test_counting_expectation_is_the_radix_expectation_on_time_sorted_input():
    """Distinct times in time order: a stable sort leaves every pixel run by time too, so the two expectations are one sequence."""
    rng = np.random.default_rng(2)
    for size, n, T in ((C.SIZE_A, 50_000, 0), (C.SIZE_R, 20_000, 0), (C.SIZE_A, 30_000, 4), (C.SIZE_B, 30_000, 40)):
        ev = np.empty((n, 4))
        ev[:, 0], ev[:, 1] = rng.integers(0, size[0], n), rng.integers(0, size[1], n)
        ev[:, 2] = np.arange(n) * 2.0 ** -20   # distinct in fp32 after the normalisation by (n - 1) * 2^-20
        ev[:, 3] = rng.integers(0, 2, n)
        assert np.unique(R.normalised_time(ev)[1]).size == n
        x, y = R.expected_packed(ev, size, T), R.counting_expected(ev, size, T)
        np.testing.assert_array_equal(y["idx"], x["idx"])
        np.testing.assert_array_equal(y["word0"] & 0xFFFFFF if T == 0 else y["word0"], x["word0"])
        np.testing.assert_array_equal(y["word1"], x["word1"])
        np.testing.assert_array_equal(y["group_start"], x["group_start"])
        if T == 0:
            np.testing.assert_array_equal(y["word0"] >> 24, R.tau_residual8(x["tau64"]))
    # ... and on a time-shuffled batch they differ inside the pixels: the run sort's order is by time, the stable one by input index
    c = C.BY_ID["chunk-edges/64x96/12289"]
    x, y = R.expected_packed(C.batch(c), c["size"]), R.counting_expected(C.batch(c), c["size"])
    assert (x["idx"] != y["idx"]).mean() > 0.2 and (np.diff(y["word1"])[np.diff(y["key"]) == 0] > 0).all()


def test_slab_expectation_is_the_regrouped_binned_one():
    """counting_expected(slabs=True) against `slab_regroup` applied to the expectation under S bins: same events group by group."""
    c = C.BY_ID["rebin-chain/edges"]
    ev, size = C.batch(c), c["size"]
    b, s = R.counting_expected(ev, size, 4), R.counting_expected(ev, size, 4, slabs=True)
    o, g = R.slab_regroup(b["row"], b["col"], b["tau64"], 4, 6)
    np.testing.assert_array_equal(s["idx"], b["idx"][o])
    np.testing.assert_array_equal(s["group"], g[o])
    np.testing.assert_array_equal(s["group_start"], R.group_starts(g[o], R.n_groups(size, 4)))


def test_case_table():
    """Sizes, ids, and -- from the EXPECTED packed positions -- every run layout the run sort has to meet; the only runs above 192
    events in the whole table are the declared ones."""
    ids = [c["id"] for c in C.CASES]
    assert len(set(ids)) == len(ids)
    # an id this table shares with the radix table is that table's row as it is (both tables' batches are cached by id in one process)
    shared = [c for c in C.CASES if c["id"] in C.S.BY_ID]
    assert len(shared) == 12 and all({k: v for k, v in c.items() if k not in ("long", "distinct")} == C.S.BY_ID[c["id"]] for c in shared)
    seen = set()
    for c in C.CASES:
        ev = C.batch(c)
        assert ev.shape == (c["n"], 4) and c["n"] <= C.N_MAX, c["id"]
        tmin, tmax = c["extremes"] if c["extremes"] else (None, None)
        x = R.counting_expected(ev, c["size"], 0, c["keep_outside"], tmin, tmax)
        assert list(x["run_len"][x["run_len"] > R.RUN_SORT_MAX]) == c["long"], c["id"]
        if c["kind"] == "runs":
            counts = [r[2] for r in c["runs"]]
            np.testing.assert_array_equal(x["run_len"], counts)          # the packed position of every run follows from the table
            np.testing.assert_array_equal(x["run_start"], np.cumsum([0] + counts[:-1]))
            assert c["evals"][0] == [C.TWO_DOF_VAR]
            seen |= C.situations(x, c["size"])
            # input positions shuffled: no run arrives in one piece
            assert (np.diff(np.sort(x["idx"][:counts[0]])) > 1).any() or counts[0] == c["n"] or counts[0] == 1
    assert seen >= set(C.SITUATIONS), set(C.SITUATIONS) - seen
    assert sorted(c["id"] for c in C.CASES if c["long"]) == ["runs/limit", "runs/long", "runs/one-run/300"]
    # chunk edges of the bucket passes, the three key forms, empty groups, the global-atomic path
    assert {c["n"] for c in C.CASES if c["id"].startswith("chunk-edges")} == {1, 2, 4095, 4096, 4097, 8191, 8192, 8193, 12289}
    assert all(k * R.SORT_CHUNK + d in C.N_EDGES for k in (1, 2) for d in (-1, 0, 1))
    Ts = {T for c in C.CASES for T, _ in C.step_bins(c)}
    assert {0, 1, 4, 32, 33, 40, 49, 255} <= Ts and R.fine_key(32) and not R.fine_key(33)
    assert R.n_groups(C.SIZE_BIG, 0) == 4225 > R.SORT_LDS_TILES
    c = C.BY_ID["bins/255-sparse"]
    assert np.unique(R.counting_expected(C.batch(c), c["size"], 255)["group"]).size < 0.65 * R.n_groups(c["size"], 255)  # 3060 groups, 3000 events
    c = C.BY_ID["tied/64-times"]
    assert np.unique(C.batch(c)[:, 2]).size == 64 and np.unique(C.batch(C.BY_ID["tied/one-time"])[:, 2]).size == 1
    for T in (4, 33, 40, 49):  # the edges batches hold every edge k / T and one fp64 ulp either side
        tau = R.normalised_time(C.batch(C.BY_ID[f"bins/{T}"]))[0]
        edges = np.arange(1, T) / T
        assert np.isin(edges, tau).all() and np.isin(np.nextafter(edges, 0.0), tau).all() and np.isin(np.nextafter(edges, 1.0), tau).all()
    # odd and single-event buckets, empty tiles, buckets above 1024 events (several rounds of k_tile_sort) somewhere in the table
    sizes = set()
    for cid in ("chunk-edges/64x96/1", "chunk-edges/50x70/4095", "sparse-720p/0", "runs/long", "chunk-edges/64x96/12289"):
        c = C.BY_ID[cid]
        gs = R.counting_expected(C.batch(c), c["size"])["group_start"]
        sizes |= set(np.diff(gs).tolist())
    assert 0 in sizes and 1 in sizes and any(v % 2 for v in sizes if v > 1) and max(sizes) > 1024


def _planted(c, T=0, slabs=False):
    x = R.counting_expected(C.batch(c), c["size"], T, slabs=slabs)
    packed = np.stack([x["word0"], x["word1"]], axis=1)
    info = [x["idx"].size, x["dropped"], int(x["fractional"]), x["outside"]]
    return x, packed, x["group_start"].copy(), info


def _rejects(x, packed, gs, info, size, **kw):
    with pytest.raises(AssertionError):
        R.compare_counting("planted", packed, gs, info, x, size, **kw)


def test_comparison_rejects_what_it_must():
    c = C.BY_ID["runs/limit"]
    size = c["size"]
    x, packed, gs, info = _planted(c)
    R.compare_counting("correct", packed, gs, info, x, size, declared_long=c["long"])
    start, length = x["run_start"], x["run_len"]
    # two events swapped across pixels
    p = packed.copy()
    a, b = start[1] - 1, start[1]
    p[[a, b]] = p[[b, a]]
    _rejects(x, p, gs, info, size, declared_long=c["long"])
    # one event overwritten by a copy of its neighbour (same pixel; and the time order is kept: only the multiset can tell)
    p = packed.copy()
    p[start[0] + 5] = p[start[0] + 4]
    assert (np.diff(p[start[0]:start[0] + length[0], 1]) >= 0).all()
    _rejects(x, p, gs, info, size, declared_long=c["long"])
    _rejects(x, p, gs, info, size, run_sorted=False)
    # a short run out of time order: caught with the run sort on, and ONLY then (the multiset is right)
    k = int(np.flatnonzero(length == 192)[0])
    p = packed.copy()
    p[[start[k] + 7, start[k] + 100]] = p[[start[k] + 100, start[k] + 7]]
    _rejects(x, p, gs, info, size, declared_long=c["long"])
    R.compare_counting("norun", p, gs, info, x, size, run_sorted=False)
    # a wrong residual byte
    p = packed.copy()
    p[start[2] + 1, 0] ^= 1 << 24
    _rejects(x, p, gs, info, size, declared_long=c["long"])
    # a run above 192 events that nobody declared; a declared one that is not there
    _rejects(x, packed, gs, info, size, declared_long=[])
    _rejects(x, packed, gs, info, size, declared_long=[193, 300])
    # accepted: a permutation inside the declared long run
    k = int(np.flatnonzero(length == 193)[0])
    p = packed.copy()
    p[start[k]:start[k] + 193] = p[start[k]:start[k] + 193][np.random.default_rng(3).permutation(193)]
    assert (np.diff(p[start[k]:start[k] + 193, 1]) < 0).any()
    R.compare_counting("long run permuted", p, gs, info, x, size, declared_long=c["long"])
    # a lost event, a wrong count in batch_info
    _rejects(x, packed[:-1], gs, info, size, declared_long=c["long"])
    _rejects(x, packed, gs, [info[0], info[1] + 1, info[2], info[3]], size, declared_long=c["long"])

    # tied times: any order of equal fp32 times passes, a decreasing word 1 does not
    c = C.BY_ID["tied/64-times"]
    x, packed, gs, info = _planted(c)
    start, length = x["run_start"], x["run_len"]
    same = np.flatnonzero((np.diff(packed[:, 1]) == 0) & (np.diff(x["key"]) == 0))
    assert same.size > 10   # equal fp32 times inside one pixel
    x2 = dict(x, word0=x["word0"].copy())   # (64 time values: tied events are equal words; make two of them differ in the residual byte)
    x2["word0"][same[0]] ^= 1 << 24
    p = np.stack([x2["word0"], x2["word1"]], axis=1)
    R.compare_counting("tie", p, gs, info, x2, c["size"])
    p[[same[0], same[0] + 1]] = p[[same[0] + 1, same[0]]]
    R.compare_counting("tie swapped", p, gs, info, x2, c["size"])
    k = int(np.flatnonzero((length > 3) & (x["word1"][start + length - 1] > x["word1"][start]))[0])
    p = packed.copy()
    p[[start[k], start[k] + length[k] - 1]] = p[[start[k] + length[k] - 1, start[k]]]
    _rejects(x, p, gs, info, c["size"])

    # binned: a group start off by one, a wrong bin on an edge event; accepted: a permutation inside a (tile, bin) group at T = 33
    for cid, T in (("bins/4", 4), ("bins/33", 33)):
        c = C.BY_ID[cid]
        x, packed, gs, info = _planted(c, T)
        R.compare_counting("correct", packed, gs, info, x, c["size"])
        g = gs.copy()
        g[len(g) // 2] += 1
        _rejects(x, packed, g, info, c["size"])
        on_edge = np.flatnonzero((x["tau64"] * T == np.rint(x["tau64"] * T)) & (x["tau64"] > 0) & (x["tau64"] < 1))
        assert on_edge.size >= T - 1
        p = packed.copy()
        p[on_edge[0], 0] -= 1 << 24   # the bin below: where a `<` for the `<=` of the bin search would put it
        _rejects(x, p, gs, info, c["size"])
        lo, hi = [(a, b) for a, b in zip(gs[:-1], gs[1:]) if b - a > 20][0]
        p = packed.copy()
        p[lo:hi] = p[lo:hi][np.random.default_rng(4).permutation(hi - lo)]
        if T == 33:
            R.compare_counting("group permuted", p, gs, info, x, c["size"])
        else:  # fine keys: the pixels of a (tile, bin) group are ordered
            _rejects(x, p, gs, info, c["size"])
    # slabs: the group order is (tile row, slab, tile column); the tile-major sequence is rejected
    c = C.BY_ID["rebin-chain/edges"]
    x, packed, gs, info = _planted(c, 4, slabs=True)
    R.compare_counting("correct", packed, gs, info, x, c["size"])
    y, packed_b, gs_b, _ = _planted(c, 4)
    _rejects(x, packed_b, gs_b, info, c["size"])
