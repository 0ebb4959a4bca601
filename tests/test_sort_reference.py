"""The numpy restatement of the packed order (tests/_sort_ref.py) held to itself and to the oracle, without a GPU: what
tests/test_gpu_radix_sort.py compares the radix sort with bit for bit."""
import numpy as np
import pytest

import event_based_optical_flow_amd as E
from oracle import oracle as orc

import _sort_cases as C
import _sort_ref as R


@pytest.mark.parametrize("size,n,bins", [((64, 96), 50_000, 0), ((260, 346), 400_000, 0), ((48, 64), 600_000, 0), ((64, 96), 60_000, 4)])
def test_reference_order_has_the_properties_of_test_packed_order(size, n, bins):
    """The small rows of tests/test_gpu_fused.py::test_packed_order (time-sorted batches), every assertion it makes -- with a stable sort
    a pixel's events come out by time whatever the length of the run."""
    ev = E.utils.generate_events(n, size[0], size[1], 0.0, 0.05, seed=3)
    x = R.expected_packed(ev, size, bins)
    gs, row, col = x["group_start"], x["row"], x["col"]
    assert x["idx"].size == n and gs[0] == 0 and gs[-1] == n and (np.diff(gs) >= 0).all() and x["dropped"] == 0 and not x["fractional"]
    tau = x["word1"].astype(np.uint32).view(np.float32)
    tn = ((ev[:, 2] - ev[:, 2].min()) / (ev[:, 2].max() - ev[:, 2].min())).astype(np.float32)
    key_in = np.lexsort((tn, ev[:, 1].astype(np.int64), ev[:, 0].astype(np.int64)))
    key_out = np.lexsort((tau, col, row))
    np.testing.assert_array_equal(row[key_out], ev[key_in, 0].astype(np.int64))
    np.testing.assert_array_equal(col[key_out], ev[key_in, 1].astype(np.int64))
    np.testing.assert_array_equal(tau[key_out], tn[key_in])
    np.testing.assert_array_equal(x["word0"] & 0xFFF, row)
    np.testing.assert_array_equal((x["word0"] >> 12) & 0xFFF, col)
    ntc = (size[1] + 15) // 16
    tile = (row >> 4) * ntc + (col >> 4)
    group = np.searchsorted(gs, np.arange(n), side="right") - 1
    if bins == 0:
        np.testing.assert_array_equal(group, tile)
        pix = ((row & 15) << 4) | (col & 15)
        same = tile[1:] == tile[:-1]
        assert (pix[1:][same] >= pix[:-1][same]).all()
        same_run = same & (pix[1:] == pix[:-1])
        assert (tau[1:][same_run] >= tau[:-1][same_run]).all()
    else:
        np.testing.assert_array_equal(group // bins, tile)
        np.testing.assert_array_equal(group % bins, x["word0"] >> 24)


@pytest.mark.parametrize("T", [1, 4, 10, 32, 33, 40, 255])
def test_voxel_bin_is_the_oracles(T):
    """Random fp64 times and every exact edge k / T with its two fp64 neighbours, against the bins of the oracle's voxel warp
    (direction "first": normalised time = dt).  Times 0 and 1 are in the batch, so the oracle's normalisation is exact."""
    rng = np.random.default_rng(T)
    edges = np.arange(T + 1, dtype=np.float64) / T
    tau = np.concatenate([[0.0, 1.0], rng.uniform(0, 1, 20_000), edges, np.nextafter(edges[1:], 0.0), np.nextafter(edges[:-1], 1.0)])
    ev = np.zeros((tau.size, 4))
    ev[:, 2] = tau
    _, aux = orc.warp_event(ev, np.zeros((T, 2, 1, 1)), "dense-flow-voxel", "first")
    np.testing.assert_array_equal(aux["dt"], tau)
    got = R.voxel_bin(tau, T)
    np.testing.assert_array_equal(got, aux["bin"])
    np.testing.assert_array_equal(R.voxel_bin(edges[:-1], T), np.arange(T))  # an event ON edge k belongs to bin k
    assert got.min() == 0 and got.max() == T - 1 and np.unique(got).size == T


def test_a_shuffled_batch_tells_stable_from_sorted_by_time():
    """Inside pixels, the stable order of a time-shuffled batch is the input order and NOT the time order: an input that could not tell
    the two apart would let a sort that ranks a pixel's events by time pass the exact-order test."""
    c = C.BY_ID["plain/64x96/f64"]
    ev = C.batch(c)
    x = R.expected_packed(ev, c["size"])
    same = (x["row"][1:] == x["row"][:-1]) & (x["col"][1:] == x["col"][:-1])
    assert (np.diff(x["idx"])[same] > 0).all()                      # input order inside every pixel
    backwards = (np.diff(x["tau64"])[same] < 0).sum()
    assert backwards > 0.4 * same.sum(), (backwards, same.sum())    # ... which is far from the time order
    by_time = np.lexsort((x["tau64"], R.key(x["row"], x["col"], x["tau64"], 6, 0)))
    assert (x["idx"][by_time] != x["idx"]).mean() > 0.5
    # and on a time-sorted batch the two coincide (why the 9M-event rows of test_packed_order cannot see stability)
    ev2 = E.utils.generate_events(50_000, 64, 96, 0.0, 0.05, seed=3)
    y = R.expected_packed(ev2, (64, 96))
    np.testing.assert_array_equal(np.lexsort((y["tau64"], R.key(y["row"], y["col"], y["tau64"], 6, 0))), np.arange(50_000))


def test_resort_of_the_packed_sequence_is_the_sort_of_the_batch():
    """Re-binning: the un-binned order re-sorted under T = 4 is the fresh T = 4 order (the new key refines nothing the old one ordered
    differently); back under T = 0 a pixel's events stay by (bin, input index) -- NOT the fresh un-binned order, which is why every
    step of the chain is predicted from the packed sequence in front of it."""
    c = C.BY_ID["rebin-chain/64x96"]
    ev = C.batch(c)
    x = R.expected_packed(ev, c["size"])
    o = R.resort(x["row"], x["col"], x["tau64"], 4, 6)
    idx, row, col, tau = x["idx"][o], x["row"][o], x["col"][o], x["tau64"][o]
    fresh = R.expected_packed(ev, c["size"], 4)
    np.testing.assert_array_equal(idx, fresh["idx"])
    np.testing.assert_array_equal(R.group_starts(R.group_of(row, col, tau, 6, 4), R.n_groups(c["size"], 4)), fresh["group_start"])
    o = R.resort(row, col, tau, 0, 6)
    idx, row, col, tau = idx[o], row[o], col[o], tau[o]
    assert (idx != x["idx"]).mean() > 0.5
    np.testing.assert_array_equal(idx, x["idx"][np.lexsort((x["idx"], R.voxel_bin(x["tau64"], 4), R.key(x["row"], x["col"], x["tau64"], 6, 0)))])
    np.testing.assert_array_equal(R.group_starts(R.group_of(row, col, tau, 6, 0), R.n_groups(c["size"], 0)), x["group_start"])


def test_dropped_and_kept_events():
    size = (64, 96)
    ev = np.array([[3.0, 4.0, 0.0, 1], [-0.5, 4.0, 0.1, 1], [3.0, 96.0, 0.2, 0], [np.nan, 1.0, 0.3, 1], [5.0, 6.0, np.nan, 1], [63.9, 95.9, 1.0, 0],
                   [70.2, -3.0, 0.5, 1], [1e12, 3.0, 0.6, 1]])
    x = R.expected_packed(ev, size, keep_outside=False)
    assert x["dropped"] == 6 and x["outside"] == 0 and sorted(x["idx"]) == [0, 5]
    y = R.expected_packed(ev, size, keep_outside=True)
    assert y["dropped"] == 3 and y["outside"] == 3 and y["fractional"] and sorted(y["idx"]) == [0, 1, 2, 5, 6]
    at = {int(i): (int(r), int(q)) for i, r, q in zip(y["idx"], y["row"], y["col"])}
    assert at[1] == (0, 4) and at[2] == (3, 95) and at[6] == (63, 0)  # the nearest sensor pixel
    np.testing.assert_array_equal(R.normalised_time(ev)[0][[0, 5]], [0.0, 1.0])  # a NaN time does not reach the extremes
    ev[6, 2], ev[7, 2] = np.inf, -np.inf
    z = R.expected_packed(ev, size, keep_outside=True)
    assert z["dropped"] == 4 and sorted(z["idx"]) == [0, 1, 2, 5]  # ... nor does an infinite one, and its event is dropped
    np.testing.assert_array_equal(R.normalised_time(ev)[0][[0, 5]], [0.0, 1.0])


def test_case_table_reaches_every_branch():
    """The pass plans of the case table (the formula of radix_pass_plan): both parities of P on both sizes in both children, the 8-bit
    first pass (D = 256) of fine binned keys up to T = 32, coarse keys from T = 33 on, ranges that end inside a step, one group."""
    for k, bits in enumerate(C.CHILD_DIGIT_BITS):
        P = {size: R.pass_plan(size, 0, 50_000, bits)["P"] for size in (C.SIZE_A, C.SIZE_B)}
        assert P[C.SIZE_A] % 2 == 1 and P[C.SIZE_B] % 2 == 0, (bits, P)
        assert P == ({C.SIZE_A: 3, C.SIZE_B: 2} if bits == 6 else {C.SIZE_A: 7, C.SIZE_B: 6})
    for size in (C.SIZE_A, C.SIZE_B):  # the role swap of re-binning, taken and not taken on EACH size (over the two children)
        chain = [R.pass_plan(size, T, 40_000, bits)["P"] % 2 for bits in C.CHILD_DIGIT_BITS for T in (4, 40, 0, 2)]
        assert 0 in chain and 1 in chain, (size, chain)
    assert R.pass_plan(C.SIZE_A, 32, 40_000)["nb"][0] == 8 and R.fine_key(32) and not R.fine_key(33)
    assert R.pass_plan(C.SIZE_A, 33, 40_000)["nb"][0] <= 6
    assert R.pass_plan((16, 16), 0, 5000)["nb"] == [5, 4] and R.n_groups((16, 16), 0) == 1
    ids = {c["id"] for c in C.CASES}
    assert len(ids) == len(C.CASES)
    assert all(c["n"] <= 50_000 for c in C.CASES)
    for c in C.CASES:  # every builder gives distinct fp32 times inside pixels (asserted by batch) and the size it promises
        assert C.batch(c).shape == (c["n"], 4)


def test_edge_batches_need_both_loops_of_the_bin_search():
    """sort_voxel_bin starts from trunc(tau * T) and walks down, then up.  The bins-coarse batches hold every edge k / T exactly and one
    fp64 ulp either side; at T = 49 the truncation UNDER-estimates the bin of some events on an edge (the walk up is needed); at T = 33
    and 40 it never does, whatever the time."""
    for T, up in ((33, False), (40, False), (49, True)):
        c = C.BY_ID[f"bins-coarse/{T}"]
        tau = R.normalised_time(C.batch(c))[0]
        first = np.clip((tau * T).astype(np.int64), 0, T - 1)
        want = R.voxel_bin(tau, T)
        assert ((first < want).sum() > 0) == up, (T, (first < want).sum())
        edges = np.arange(1, T) / T
        assert np.isin(edges, tau).all() and np.isin(np.nextafter(edges, 0.0), tau).all() and np.isin(np.nextafter(edges, 1.0), tau).all()
