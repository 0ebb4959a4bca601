"""The work list `cut_work_list` (csrc/cmax_batch_plan.h, called by `build_segments` of csrc/cmax_batch.hip) cuts from the group starts and the compact copy `k_pack_compact`
(csrc/cmax_event_kernels.inc) writes for big segments, restated in numpy (no GPU, no import of the package).

`cut` restates the RULES of the host's cut, constants named.  `check_invariants` is written from what the event kernels REQUIRE of any
cut -- it knows nothing of the rules and is the authority when the two disagree with the library.  `compact_expected` / `decode` are the
layout comment of "COMPACT EVENTS" and the kernels' `decode_slot`.

A segment is (first event, count, first group, number of groups).  A group is a source tile (un-binned handles), a (tile, time bin)
(binned) or a (tile row, slab, tile column) (slab-major).  `T` is the handle's number of time bins or slabs (0: un-binned)."""
import numpy as np

from _sort_ref import tau_refined

SEG_STD, SEG_MID, SEG_BIG = 2040, 3064, 4088      # kSegMax and the mid / big cuts: events per segment
OWNED_MIN = 256 * SEG_STD                          # 522 240: from here on groups can be owned, and no small-batch cap
FREE_CUT_ABOVE = 1024 * SEG_STD                    # 2 088 960: above, lists that are not owned are cut every seg_max events
BIG_FROM = 8_000_000                               # batches from here on take big segments whatever their groups
BIG_UNALIGNED_FROM = 4_000_000                     # ... and from here on when the standard cut is not group-aligned
SMALL_ACC_EVENTS = 480                             # events per (tile, bin) group on average: small accumulators
SPAN_STD, SPAN_MID, SPAN_BIG = 3, 4, 6             # source tiles per segment of an un-binned list
SPAN_BINNED, SPAN_SMALL, SPAN_SMALL_MID = 12, 3, 5 # (tile, bin) groups per segment: LDS accumulators, small ones, small ones on mid
SPARSE_SEGMENT = 512                               # kSparseSegment: the voxel K3 adds such segments straight to memory
SMALL_CAP_MIN, SMALL_CAP_DIV = 256, 512            # small batches: count <= max(256, ceil(n / 512))
RESIDENT = 1024                                    # workgroups of 512 threads the chip holds at once (the one-round mid rule)
FLAGS = ("big", "mid", "owned", "small_accumulators", "slab_major", "compact", "long_runs")

SLOTS = 4096                                       # b512::kSlots
COMPACT_PIX, COMPACT_HDR = 4 * SLOTS, 4 * SLOTS + SLOTS // 2
COMPACT_STRIDE = COMPACT_HDR + 64


def _env_int(env, name, default):
    v = (env or {}).get(name)
    if v is None:
        return default
    try:
        return int(v)
    except ValueError:
        return 0  # atoi


def _aligned_count(counts, row_groups, cut_events, span_max):
    """Segments of the group-aligned cut (`owned_count`); -1 when a group exceeds `cut_events`."""
    if counts.size and counts.max() > cut_events:
        return -1
    return len(_aligned_cut(counts, None, row_groups, cut_events, span_max))


def _aligned_cut(counts, group_start, row_groups, cut_events, span_max):
    segs = []
    ngroups = counts.size
    for r0 in range(0, ngroups, row_groups):
        g = r0
        while g < r0 + row_groups:
            gs, c = g, 0
            while g < r0 + row_groups and g - gs < span_max and c + counts[g] <= cut_events:
                c += counts[g]
                g += 1
            segs.append((int(group_start[gs]) if group_start is not None else 0, int(c), gs, g - gs))
    return segs


def small_batch_cap(n, seg_max=SEG_STD):
    """Events per segment of a list that is not cut freely: n / 512 (at least 256) below 522 240 events, else seg_max."""
    return min(seg_max, max(SMALL_CAP_MIN, -(-n // SMALL_CAP_DIV))) if n < OWNED_MIN else seg_max


def cut_with_reasons(group_start, n, ntr, ntc, T=0, slab=False, long_runs=False, env=None):
    """(segments [k, 4] int64, flags {name: bool}, seg_max, why): `why` names the rule behind every decision -- big_rule in
    {"slab", "forced", "8M", "small", "ratio", "unaligned"}, std_n / big_n / mid_n where they were counted, seg_cap, free_cut, max_groups
    and split_groups (how many groups were cut into equal parts)."""
    group_start = np.asarray(group_start, np.int64)
    slab = bool(slab) and T > 0
    Tg = T if (T > 0 and not slab) else 1          # groups per tile
    ngroups = ntr * ntc * (T if slab else Tg)
    assert group_start.size == ngroups + 1 and group_start[-1] == n, (group_start.size, ngroups, n)
    counts = np.diff(group_start)
    row_groups = ntc * Tg
    big_env, mid_env, small_env = (_env_int(env, k, -1) for k in ("CMAX_BIG_SEG", "CMAX_MID_SEG", "CMAX_SMALL_ACC"))
    no_owned = (env or {}).get("CMAX_NO_OWNED") is not None
    compact_env = _env_int(env, "CMAX_COMPACT", 1)
    why = {"std_n": None, "big_n": None, "mid_n": None}
    mid = False
    if slab:
        big, why["big_rule"] = False, "slab"
    elif big_env >= 0:
        big, why["big_rule"] = big_env != 0, "forced"
    elif n >= BIG_FROM:
        big, why["big_rule"] = True, "8M"
    elif n < OWNED_MIN:
        big, why["big_rule"] = False, "small"
    else:
        small_std = Tg > 1 and n >= SMALL_ACC_EVENTS * ngroups
        std_n = _aligned_count(counts, row_groups, SEG_STD, SPAN_STD if Tg == 1 else (SPAN_SMALL if small_std else SPAN_BINNED))
        big_n = _aligned_count(counts, row_groups, SEG_BIG, SPAN_BIG if Tg == 1 else SPAN_BINNED) if std_n >= 0 else -1
        big = 4 * std_n >= 11 * big_n if std_n >= 0 else n >= BIG_UNALIGNED_FROM
        why.update(big_rule="ratio" if std_n >= 0 else "unaligned", std_n=std_n, big_n=big_n)
        if not big and mid_env != 0 and not no_owned:
            mid_n = _aligned_count(counts, row_groups, SEG_MID, SPAN_MID if Tg == 1 else (SPAN_SMALL_MID if small_std else SPAN_BINNED))
            mid = mid_n > 0 if mid_env > 0 else (0 < mid_n <= RESIDENT and std_n > RESIDENT)
            why["mid_n"] = mid_n
    seg_max = SEG_BIG if big else (SEG_MID if mid else SEG_STD)
    max_groups = SPAN_STD if Tg == 1 else SPAN_BINNED
    free_cut = n > FREE_CUT_ABOVE
    seg_cap = small_batch_cap(n, seg_max)
    if Tg > 1 and seg_cap < SPARSE_SEGMENT:
        max_groups = max(max_groups, 3 * Tg)
    owned = n >= OWNED_MIN and not no_owned and not slab and bool((counts <= seg_max).all())
    small_acc = Tg > 1 and owned and not big and (small_env != 0 if small_env >= 0 else n >= SMALL_ACC_EVENTS * ngroups)
    assert owned or not mid, "the library refuses a mid list that is not group-aligned"
    split_groups = 0
    if owned:
        span = ((SPAN_BIG if big else (SPAN_MID if mid else SPAN_STD)) if Tg == 1
                else ((SPAN_SMALL_MID if mid else SPAN_SMALL) if small_acc else SPAN_BINNED))
        segs = _aligned_cut(counts, group_start, row_groups, seg_max, span)
    else:
        segs = []
        begin = count = g0 = g_last = 0
        row_of_begin = -1
        for g in np.flatnonzero(counts):
            g, b, c = int(g), int(group_start[g]), int(counts[g])
            trow = (g // Tg) // ntc
            if count > 0 and (trow != row_of_begin or g - g0 + 1 > max_groups or (not free_cut and count + c > seg_cap)):
                segs.append((begin, count, g0, g_last - g0 + 1))
                count = 0
            limit = seg_cap
            if not free_cut and c > seg_cap:
                parts = -(-c // seg_cap)
                limit = -(-c // parts)
                split_groups += 1
            while c > 0:
                if count == 0:
                    begin, row_of_begin, g0 = b, trow, g
                g_last = g
                take = min(c, limit - count)
                count += take
                b += take
                c -= take
                if count >= limit:
                    segs.append((begin, count, g0, g_last - g0 + 1))
                    count = 0
        if count > 0:
            segs.append((begin, count, g0, g_last - g0 + 1))
    segs = np.asarray(segs, np.int64).reshape(-1, 4)
    compact = bool(big and Tg == 1 and not slab and T == 0 and len(segs) > 0 and compact_env != 0 and long_runs)
    flags = dict(big=bool(big), mid=bool(mid), owned=bool(owned), small_accumulators=bool(small_acc), slab_major=slab, compact=compact,
                 long_runs=bool(long_runs))
    why.update(seg_cap=seg_cap, free_cut=bool(free_cut and not owned), max_groups=max_groups, split_groups=split_groups)
    return segs, flags, seg_max, why


def cut(group_start, n, ntr, ntc, T=0, slab=False, long_runs=False, env=None):
    """(segments, flags, seg_max) of the work list `build_segments` cuts.  env: what the process holds of CMAX_BIG_SEG, CMAX_MID_SEG,
    CMAX_NO_OWNED, CMAX_SMALL_ACC and CMAX_COMPACT (a dict of strings; the tuning-only switches are not modelled)."""
    return cut_with_reasons(group_start, n, ntr, ntc, T, slab, long_runs, env)[:3]


def long_runs_of(packed, T):
    """`long_runs` as the handle sets it: un-binned batches of >= 8 events per active source pixel (false on binned / slab handles)."""
    packed = np.asarray(packed, np.int64)
    if T > 0 or packed.shape[0] == 0:
        return False
    return packed.shape[0] >= 8 * np.unique(packed[:, 0] & 0xFFFFFF).size


def event_groups(packed, ntc, T, slab):
    """Group of every packed event, from the event's own word 0 (pixel, time bin)."""
    w0 = np.asarray(packed, np.int64)[:, 0]
    tr, tc, top = (w0 & 0xFFF) >> 4, ((w0 >> 12) & 0xFFF) >> 4, w0 >> 24
    if T == 0:
        return tr * ntc + tc
    return (tr * T + top) * ntc + tc if slab else (tr * ntc + tc) * T + top


def check_invariants(segs, flags, packed, group_start, geometry):
    """What the event kernels require of a work list, whatever rules cut it.  geometry: dict(ntr, ntc, T, slab, seg_max).
    Raises AssertionError naming the first violated requirement."""
    segs, gs = np.asarray(segs, np.int64).reshape(-1, 4), np.asarray(group_start, np.int64)
    packed = np.asarray(packed, np.int64).reshape(-1, 2)
    ntr, ntc, T, seg_max = geometry["ntr"], geometry["ntc"], geometry["T"], geometry["seg_max"]
    slab = bool(geometry["slab"]) and T > 0
    Tg = T if (T > 0 and not slab) else 1
    n, ngroups = packed.shape[0], gs.size - 1
    assert ngroups == ntr * ntc * max(T, 1), (ngroups, ntr, ntc, T)
    first, count, z, w = segs.T if segs.size else (np.zeros(0, np.int64),) * 4
    eg = event_groups(packed, ntc, T, slab)
    # (the group starts are those of the events: what everything below leans on)
    assert (np.diff(eg) >= 0).all() and (np.searchsorted(eg, np.arange(ngroups + 1)) == gs).all(), "group starts do not match the packed events"
    owned = flags["owned"]
    assert flags["slab_major"] == slab
    assert not (flags["big"] and flags["mid"]) and seg_max == (SEG_BIG if flags["big"] else (SEG_MID if flags["mid"] else SEG_STD))
    # ---- partition
    if n == 0 and not owned:
        assert segs.shape[0] == 0, "segments on an empty batch"
        return
    assert segs.shape[0] > 0, "no segments"
    assert (count >= 0).all() and (w >= 1).all()
    assert first[0] == 0 and (first[1:] == first[:-1] + count[:-1]).all() and first[-1] + count[-1] == n, "segments are not [0, n) in event order"
    if not owned:
        assert (count > 0).all(), "empty segment in a list that is not owned"
    else:
        assert z[0] == 0 and (z[1:] == z[:-1] + w[:-1]).all() and z[-1] + w[-1] == ngroups, "owned: a group in no or in two segments"
        assert (gs[z] == first).all() and (gs[z + w] == first + count).all(), "owned: a segment is not made of whole groups"
        assert not slab, "slab-major lists are never owned (a source pixel belongs to S groups)"
    assert (z >= 0).all() and (z + w <= ngroups).all()
    # ---- events of a segment: one tile row (slab-major: one (tile row, slab)), and [z, z + w) covers exactly their groups
    row_of_group = (lambda g: g // ntc) if slab else (lambda g: (g // Tg) // ntc)
    assert (row_of_group(z) == row_of_group(z + w - 1)).all(), "a segment's groups cross a tile row"
    ne = np.flatnonzero(count > 0)
    if ne.size:
        lo = np.minimum.reduceat(eg, first[ne])
        hi = np.maximum.reduceat(eg, first[ne])
        if owned:
            assert (lo >= z[ne]).all() and (hi < z[ne] + w[ne]).all(), "an event outside its segment's groups"
        else:
            assert (lo == z[ne]).all() and (hi == z[ne] + w[ne] - 1).all(), "[z, z + w) is not exactly the groups of the segment's events"
        tr = (packed[:, 0] & 0xFFF) >> 4
        assert (np.minimum.reduceat(tr, first[ne]) == np.maximum.reduceat(tr, first[ne])).all(), "a segment's events lie in two tile rows"
        if slab:
            top = packed[:, 0] >> 24
            assert (np.minimum.reduceat(top, first[ne]) == np.maximum.reduceat(top, first[ne])).all(), "a segment's events lie in two slabs"
    # ---- size
    assert (count <= seg_max).all(), f"a segment of {count.max()} events, seg_max {seg_max}"
    # ---- span
    if flags["mid"]:
        assert owned, "a mid list that is not owned"
    if Tg == 1:
        assert not flags["small_accumulators"]
        limit = SPAN_BIG if (flags["big"] and owned) else (SPAN_MID if flags["mid"] else SPAN_STD)
        assert (w <= limit).all(), f"a segment {w.max()} tiles wide, limit {limit}"
    elif flags["small_accumulators"]:
        assert owned and not flags["big"]
        limit = SPAN_SMALL_MID if flags["mid"] else SPAN_SMALL
        assert (w <= limit).all(), f"small accumulators: a segment {w.max()} groups wide, limit {limit}"
    else:  # 12 groups fit the LDS accumulators; a segment below 512 events that is not owned adds straight to memory: up to 3 tiles' worth
        wide = w > SPAN_BINNED
        assert not wide.any() or (not owned and (count[wide] < SPARSE_SEGMENT).all() and (w[wide] <= 3 * T).all()), "a binned segment too wide"
    # ---- lists that merge and split groups (not owned, not cut freely): the cap, and equal parts for a group above it
    if not owned and n <= FREE_CUT_ABOVE:
        cap = small_batch_cap(n, seg_max)
        assert (count <= cap).all(), f"a segment of {count.max()} events above the cap {cap}"
        c = np.diff(gs)
        starts = set(first.tolist())
        for g in np.flatnonzero(c > cap):
            parts = -(-int(c[g]) // cap)
            size = -(-int(c[g]) // parts)
            want = {int(gs[g]) + k * size for k in range(parts)}
            got = {s for s in starts if gs[g] <= s < gs[g + 1]}
            assert got == want, f"group {g} of {c[g]} events: cut at {sorted(got)}, expected {parts} parts of {size}"
    # ---- compact copy: big segments of an un-binned handle only (the kernels decode a 3-bit tile column and a 4-bit row in ONE tile row)
    if flags["compact"]:
        assert flags["big"] and T == 0 and (w <= 8).all()


def compact_expected(packed, segs, ntc):
    """The compact regions byte for byte: uint8 [n_segments, COMPACT_STRIDE]."""
    packed, segs = np.asarray(packed, np.int64).reshape(-1, 2), np.asarray(segs, np.int64).reshape(-1, 4)
    ns, n = segs.shape[0], packed.shape[0]
    first, count, z = segs[:, 0], segs[:, 1], segs[:, 2]
    words = np.zeros((ns, COMPACT_STRIDE // 4), np.uint32)
    s = np.repeat(np.arange(ns), count)
    assert s.size == n and (np.repeat(first, count) + (np.arange(n) - np.repeat(np.cumsum(count) - count, count)) == np.arange(n)).all()
    slot = np.arange(n) - (first - (first & 1))[s]
    assert (slot < SLOTS).all()
    row, col, byte = packed[:, 0] & 0xFFF, (packed[:, 0] >> 12) & 0xFFF, packed[:, 0] >> 24
    tau, _ = tau_refined(packed[:, 1], byte)
    t24 = np.clip(np.rint(tau * 16777216.0), 0, 16777215).astype(np.int64)
    words[s, slot] = (t24 << 8 | (row & 15) << 4 | (col & 15)).astype(np.uint32)
    nib = ((col >> 4) - (z % ntc)[s]) & 7
    np.add.at(words, (s, SLOTS + slot // 8), (nib << (4 * (slot % 8))).astype(np.uint32))
    words[:, COMPACT_HDR // 4] = (16 * (z // ntc) | (16 * (z % ntc)) << 12).astype(np.uint32)
    return words.view(np.uint8).reshape(ns, COMPACT_STRIDE)


def decode(region):
    """`decode_slot` of the compact path for all 4096 slots of one region (uint8 [COMPACT_STRIDE]): (row, col, tau), the time as the
    exact fp32 value (float)t24 * 2^-24.  An empty slot decodes to the region's corner pixel at time 0."""
    wd = np.ascontiguousarray(region).view(np.uint32).astype(np.int64)
    a, tiles, basexy = wd[:SLOTS], wd[SLOTS:SLOTS + SLOTS // 8], wd[COMPACT_HDR // 4]
    l = np.arange(SLOTS)
    tcol = (tiles[l >> 3] >> (4 * (l & 7))) & 7
    ixr, iyr = (a >> 4) & 15, (tcol << 4) | (a & 15)
    key = basexy + ixr + (iyr << 12)
    tau = ((a >> 8).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float64)
    return key & 0xFFF, (key >> 12) & 0xFFF, tau
