"""tests/_worklist_ref.py held on the CPU: `cut` satisfies `check_invariants` on every case of tests/_worklist_cases.py, every case reaches
the regime its name says, the hand-worked anchors hold, and the compact layout decodes back to the events.  The packed words and the
group starts come from tests/_sort_ref.py (`counting_expected`), so nothing here needs the library."""
import numpy as np
import pytest

import _sort_ref as S
import _worklist_cases as C
import _worklist_ref as R

_packed = {}


def packed_of(c):
    """(packed [n, 2], group starts) of a case's batch as cmax_set_events leaves them (canonical order inside a key)."""
    if id(c) not in _packed:
        x = S.counting_expected(C.batch(c), c["size"], c["T"], True, 0.0, 1.0)
        _packed[id(c)] = (np.stack([x["word0"], x["word1"]], axis=1), x["group_start"])
    return _packed[id(c)]


def cut_case(c, env):
    packed, gs = packed_of(c)
    ntr, ntc = C.tiles(c["size"])
    return packed, gs, R.cut_with_reasons(gs, packed.shape[0], ntr, ntc, c["T"], False, R.long_runs_of(packed, c["T"]), env)


ALL = [(c, None, c["id"]) for c in C.CASES] + [(c, C.CHILD_ENV[k], f"{C.CHILD_IDS[k]}/{c['id']}") for k, t in enumerate(C.FORCED) for c in t]


@pytest.mark.parametrize("c,env", [a[:2] for a in ALL], ids=[a[2] for a in ALL])
def test_cut_holds_the_invariants_and_reaches_its_regime(c, env):
    packed, gs, (segs, flags, seg_max, why) = cut_case(c, env)
    ntr, ntc = C.tiles(c["size"])
    hist = np.asarray(c["hist"]()).reshape(-1)
    np.testing.assert_array_equal(np.diff(gs), hist, err_msg="the batch does not have the case's histogram")
    R.check_invariants(segs, flags, packed, gs, dict(ntr=ntr, ntc=ntc, T=c["T"], slab=False, seg_max=seg_max))
    said = dict(flags, **why)
    for name, want in c["expect"].items():
        assert said[name] == want, (c["id"], name, said[name], want, said)
    n = packed.shape[0]
    assert (n < R.OWNED_MIN) == c["id"].startswith(("small-", "forced-big-32x48", "forced-big-48x160")), (c["id"], n)


def _segs(c, env=None):
    return cut_case(c, env)[2][0]


def test_anchor_equal_parts():
    """The comment's own example: a tile of 2846 events is cut into 2 x 1423, not 2040 + 806; a tile of 2041 into 1021 + 1020."""
    c = C.BY_ID["one-tile-of-2041-not-owned-standard-equal-parts"]
    _, gs, (segs, flags, seg_max, why) = cut_case(c, None)
    by_first = {int(s[0]): s for s in segs}
    a, b = by_first[int(gs[100])], by_first[int(gs[100]) + 1021]
    assert (a[1], a[2], a[3]) == (1021, 100, 1) and (b[1], b[2]) == (1020, 100)
    a, b = by_first[int(gs[101])], by_first[int(gs[101]) + 1423]
    assert (a[1], a[2], a[3]) == (1423, 101, 1) and (b[1], b[2]) == (1423, 101)
    assert int(gs[100]) + 1021 + 1020 == int(gs[101])
    # (the second part of a split group stays open: the next group joins it while it fits)
    assert not flags["owned"] and seg_max == 2040


def test_anchor_small_batch_by_hand():
    """32 x 48 (2 x 3 tiles), histogram [10, 771, 5, 0, 1285, 3], n = 2074: cap = max(256, ceil(2074 / 512)) = 256.
    tile 0: 10 | tile 1: 771 > cap -> 4 parts of 193 (192 left for the last, which tile 2's 5 events join: 197) | row 1, tile 4: 1285 ->
    6 parts of 215 (210 left, + tile 5's 3 = 213)."""
    segs = _segs(C.BY_ID["small-group-above-cap-odd-parts"])
    want = [(0, 10, 0, 1), (10, 193, 1, 1), (203, 193, 1, 1), (396, 193, 1, 1), (589, 197, 1, 2),
            (786, 215, 4, 1), (1001, 215, 4, 1), (1216, 215, 4, 1), (1431, 215, 4, 1), (1646, 215, 4, 1), (1861, 213, 4, 2)]
    np.testing.assert_array_equal(segs, np.array(want))
    assert (segs[:, 0] & 1).any()  # segments that start at odd indices


def test_anchor_tile_row_change_closes_a_segment():
    """48 x 64 (3 x 4 tiles), [90, 80, 70, 100 | 100, 40, 0, 0 | 0, 0, 0, 60]: 90 + 80 + 70 = 240 (3 tiles; + 100 would pass 256), the
    100 of tile 3 alone -- tile 4 lies in the next tile row --, 100 + 40, and the 60 of the last row."""
    segs = _segs(C.BY_ID["small-tile-row-change-inside-a-segment"])
    np.testing.assert_array_equal(segs, np.array([(0, 240, 0, 3), (240, 100, 3, 1), (340, 140, 4, 2), (480, 60, 11, 1)]))


def test_anchor_owned_lists_keep_empty_groups():
    c = C.BY_ID["owned-standard-every-tile-at-most-2040"]
    _, gs, (segs, flags, seg_max, why) = cut_case(c, None)
    assert flags["owned"] and (segs[:, 3].sum() == gs.size - 1) and (segs[:, 3] <= 3).all()
    assert segs[0].tolist() == [0, 2040, 0, 1]                     # a tile of exactly 2040 events fills its segment
    assert (np.diff(gs)[segs[segs[:, 3] > 1, 2] + 1] == 0).any()   # an empty tile rides along with its neighbour


def test_anchor_spans():
    big = _segs(C.BY_ID["ratio-4-std-equals-11-big-takes-big-owned"])
    assert set(big[:, 3].tolist()) == {2, 3, 4} and big[:, 1].max() == 3980   # 3 x 1100 | 3 x 1100 + 680 | 2 x 680
    big = _segs(C.BY_ID["ratio-above-big-owned-3-and-6-tiles-wide"])
    assert set(big[:, 3].tolist()) == {3, 6} and big[:, 1].max() == 4080   # 3 x 1100 | 6 x 680
    mid = _segs(C.BY_ID["mid/forced-mid-4-tiles-wide"], C.CHILD_ENV[2])
    assert mid[:, 3].max() == 4 and mid[:, 1].max() == 3000
    mid5 = _segs(C.BY_ID["mid/forced-mid-binned-T4-small-accumulators-5-wide"], C.CHILD_ENV[2])
    assert mid5[:, 3].max() == 5 and mid5[:, 1].max() == 5 * 481
    assert _segs(C.BY_ID["binned-T4-small-accumulators-at-481-per-group"])[:, 3].max() == 3
    assert _segs(C.BY_ID["binned-T4-479-per-group-just-below-small-accumulators"])[:, 3].max() == 4   # 4 x 479 <= 2040, span 12
    assert _segs(C.BY_ID["small-acc-0/binned-T4-481-per-group-small-accumulators-off-span-12"], C.CHILD_ENV[4])[:, 3].max() == 4
    t10 = _segs(C.BY_ID["small-binned-T10-30k-span-3T"])
    assert 12 < t10[:, 3].max() <= 30 and t10[:, 1].max() <= 256
    free = _segs(C.BY_ID["free-cut-above-2088960"])
    assert (free[:, 1] == 2040).mean() > 0.95 and free[:, 3].max() >= 2    # full segments that cross tile borders
    full = _segs(C.BY_ID["big/forced-big-odd-starts-and-full-4088-segments"], C.CHILD_ENV[0])
    assert (full[:, 1] == 4088).sum() >= 3 and (full[:, 0] & 1).any()


def test_invariants_reject_what_the_kernels_cannot_take():
    """check_invariants is the authority: every way a cut can be valid-looking and wrong must be caught."""
    c = C.BY_ID["owned-standard-every-tile-at-most-2040"]
    packed, gs, (segs, flags, seg_max, why) = cut_case(c, None)
    ntr, ntc = C.tiles(c["size"])
    geo = dict(ntr=ntr, ntc=ntc, T=0, slab=False, seg_max=seg_max)
    R.check_invariants(segs, flags, packed, gs, geo)

    def broken(segs2, flags2=flags, geo2=geo):
        with pytest.raises(AssertionError):
            R.check_invariants(segs2, flags2, packed, gs, geo2)

    two = np.flatnonzero((segs[:-1, 2] // ntc == segs[1:, 2] // ntc) & (segs[:-1, 1] > 0) & (segs[1:, 1] > 0))[0]
    merged = np.delete(segs, two + 1, axis=0)
    merged[two] = (segs[two, 0], segs[two, 1] + segs[two + 1, 1], segs[two, 2], segs[two, 3] + segs[two + 1, 3])
    broken(merged)                                                  # above seg_max
    shifted = segs.copy()
    shifted[two, 1] -= 1
    shifted[two + 1, 0] -= 1
    shifted[two + 1, 1] += 1
    broken(shifted)                                                 # owned, and a group given to two segments
    broken(shifted, dict(flags, owned=False))                       # not owned: [z, z + w) no longer the groups of the events
    broken(segs[:-1])                                               # a gap at the end
    row_end = np.flatnonzero(segs[:-1, 2] // ntc != segs[1:, 2] // ntc)[0]
    cross = np.delete(segs, row_end + 1, axis=0)
    cross[row_end] = (segs[row_end, 0], 10, segs[row_end, 2], segs[row_end, 3] + segs[row_end + 1, 3])
    broken(cross)
    broken(segs, dict(flags, mid=True))                             # flags and seg_max disagree
    c4 = C.BY_ID["ratio-above-big-owned-3-and-6-tiles-wide"]
    packed4, gs4, (segs4, flags4, seg_max4, _) = cut_case(c4, None)
    ntr4, ntc4 = C.tiles(c4["size"])
    with pytest.raises(AssertionError):                             # 6 tiles wide is for big owned lists only
        R.check_invariants(segs4, dict(flags4, owned=False), packed4, gs4, dict(ntr=ntr4, ntc=ntc4, T=0, slab=False, seg_max=seg_max4))


COMPACT = [a for a in ALL if a[0]["expect"].get("compact")]


@pytest.mark.parametrize("c,env", [a[:2] for a in COMPACT], ids=[a[2] for a in COMPACT])
def test_compact_layout_decodes_back(c, env):
    packed, gs, (segs, flags, seg_max, why) = cut_case(c, env)
    assert flags["compact"]
    _, ntc = C.tiles(c["size"])
    regions = R.compact_expected(packed, segs, ntc)
    assert regions.shape == (segs.shape[0], R.COMPACT_STRIDE) and regions.dtype == np.uint8
    row, col = packed[:, 0] & 0xFFF, (packed[:, 0] >> 12) & 0xFFF
    tau, _ = S.tau_refined(packed[:, 1], packed[:, 0] >> 24)
    words = regions.view(np.uint32).reshape(segs.shape[0], -1)
    assert (words[:, R.COMPACT_HDR // 4 + 1:] == 0).all()           # header words 1 .. 15
    seen_odd = False
    for s, (first, count, z, w) in enumerate(segs):
        r, cc, t = R.decode(regions[s])
        odd = first & 1
        seen_odd |= bool(odd)
        sl = slice(odd, odd + count)
        np.testing.assert_array_equal(r[sl], row[first:first + count])
        np.testing.assert_array_equal(cc[sl], col[first:first + count])
        want = np.minimum(tau[first:first + count], 1.0 - 2.0 ** -24)
        assert np.abs(t[sl] - want).max() <= 2.0 ** -25
        empty = np.ones(R.SLOTS, bool)
        empty[sl] = False
        assert (words[s, :R.SLOTS][empty] == 0).all()                # slot 0 of an odd start included
        nib = (words[s, R.SLOTS:R.SLOTS + R.SLOTS // 8, None] >> (4 * np.arange(8, dtype=np.uint32))) & 15
        assert (nib.reshape(-1)[empty] == 0).all() and nib.max() < w
        assert words[s, R.COMPACT_HDR // 4] == 16 * (z // ntc) | (16 * (z % ntc)) << 12
    assert seen_odd or not c["extreme"] or c["id"].startswith("ratio")
    if c["extreme"]:
        ev = C.batch(c)
        for t_in, t_out in ((0.0, 0.0), (1.0, 1.0 - 2.0 ** -24), (0.75 * 2.0 ** -24, 2.0 ** -24), (2.0 ** -100, 0.0), (2.0 ** -26 * 1.5, 0.0)):
            i = np.flatnonzero(ev[:, 2] == t_in)
            assert i.size == 1
            px = (int(ev[i[0], 0]), int(ev[i[0], 1]))
            j = np.flatnonzero((row == px[0]) & (col == px[1]) & (tau == t_in))
            assert j.size >= 1
            s = np.searchsorted(segs[:, 0], j[0], side="right") - 1
            got = R.decode(regions[s])[2][j[0] - segs[s, 0] + (segs[s, 0] & 1)]
            assert got == t_out, (t_in, got, t_out)
        assert ((packed[:, 0] >> 24) >= 128).any()                  # a negative residual byte took part
