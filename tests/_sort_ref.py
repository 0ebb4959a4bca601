"""What the STABLE radix sort of csrc/cmax_radix_sort.h must leave, restated in numpy (no GPU, no import of the package).

A stable sort has one right answer per input: the events in the order of their key, equal keys in input order.  The key is the one
`rs_key` builds -- source tile (16 x 16) major, then the voxel time bin (binned handles), then the pixel inside the tile while the
handle's (bin, pixel) keys fit the counting sort's 8192 counters -- and the time bin is the one `sort_voxel_bin` assigns: the
reference's direction-"first" bin, the last k with k / T <= tau (oracle/oracle.py: orc_warp_voxel).  Events are (row, column, t, p)."""
import numpy as np

TILE_KEYS_MAX = 8192      # kTileKeysMax: (bin, pixel) keys up to T = 32
RS_MAX_DIGIT_BITS = 6     # kRsMaxDigitBits
RS_CHUNK = 2048           # kRsChunk: events per workgroup and iteration
RS_THREADS = 512          # kRsThreads
RS_MAX_GROUPS = 1024      # kRsMaxGroups
COORD_LIMIT = 1048576.0   # kept off-sensor events must be "finite, sane"


def normalised_time(ev, tmin=None, tmax=None):
    """(tau64, tau32): (t - tmin) / (tmax - tmin) in fp64 -- the extremes of the batch itself (over its FINITE times: an event whose time is
    NaN or +-inf is dropped and takes no part in them) unless they are given -- and its rounding to fp32 (word 1 of a packed event)."""
    t = np.asarray(ev)[:, 2].astype(np.float64)
    if tmin is None or tmax is None:
        ok = np.isfinite(t)
        tmin, tmax = (t[ok].min(), t[ok].max()) if ok.any() else (np.inf, -np.inf)
    per = np.float64(tmax) - np.float64(tmin)
    with np.errstate(invalid="ignore"):
        tau = (t - np.float64(tmin)) / per if per > 0 else np.zeros_like(t)
    return tau, tau.astype(np.float32)


def voxel_bin(tau64, T):
    """The last k with k / T <= tau (fp64 compares), clipped to 0 .. T - 1."""
    edges = np.arange(T, dtype=np.float64) / np.float64(T)
    k = np.searchsorted(edges, np.asarray(tau64, dtype=np.float64), side="right") - 1
    return np.clip(k, 0, T - 1).astype(np.int64)


def fine_key(T):
    return T == 0 or T * 256 <= TILE_KEYS_MAX


def group_of(row, col, tau64, ntc, T):
    tile = (np.asarray(row, np.int64) >> 4) * ntc + (np.asarray(col, np.int64) >> 4)
    return tile if T == 0 else tile * T + voxel_bin(tau64, T)


def key(row, col, tau64, ntc, T):
    row, col = np.asarray(row, np.int64), np.asarray(col, np.int64)
    group = group_of(row, col, tau64, ntc, T)
    return (group << 8) | ((row & 15) << 4) | (col & 15) if fine_key(T) else group


def stable_order(keys):
    return np.argsort(keys, kind="stable")


def n_groups(size, T):
    return ((size[0] + 15) // 16) * ((size[1] + 15) // 16) * max(T, 1)


def group_starts(groups_sorted, ngroups):
    """group_start[g] = first event of group g (empty groups take the next group's start), group_start[ngroups] = n."""
    return np.searchsorted(groups_sorted, np.arange(ngroups + 1), side="left").astype(np.int64)


def classify(ev, size, keep_outside):
    """(survives, row, col, outside): `RawSource::classify`.  An event is dropped when a coordinate or its time is not finite, or when
    it lies off the sensor and keep_outside is false; a kept off-sensor event sorts under its nearest sensor pixel."""
    ev = np.asarray(ev)
    H, W = size
    with np.errstate(invalid="ignore"):
        fx, fy = np.floor(ev[:, 0].astype(np.float64)), np.floor(ev[:, 1].astype(np.float64))
        on = (fx >= 0) & (fx < H) & (fy >= 0) & (fy < W)
        sane = (fx > -COORD_LIMIT) & (fx < COORD_LIMIT) & (fy > -COORD_LIMIT) & (fy < COORD_LIMIT)
    outside = ~on & sane & bool(keep_outside)
    ok = (on | outside) & np.isfinite(ev[:, 2].astype(np.float64))
    row = np.clip(np.where(ok, fx, 0), 0, H - 1).astype(np.int64)
    col = np.clip(np.where(ok, fy, 0), 0, W - 1).astype(np.int64)
    return ok, row, col, outside & ok


def expected_packed(ev, size, T=0, keep_outside=True, tmin=None, tmax=None):
    """The packed batch `cmax_set_events` must leave: dict of
    idx [n_packed] input index of every packed event, word0 (row | col << 12 | bin << 24; no top byte for T == 0), word1 (bits of the
    fp32 normalised time), group_start [ngroups + 1], dropped, outside, fractional, and row / col / tau64 of the packed sequence."""
    ev = np.asarray(ev)
    ntc = (size[1] + 15) // 16
    ok, row, col, outside = classify(ev, size, keep_outside)
    tau64, tau32 = normalised_time(ev, tmin, tmax)
    surv = np.flatnonzero(ok)
    idx = surv[stable_order(key(row[surv], col[surv], tau64[surv], ntc, T))]
    r, c, t64 = row[idx], col[idx], tau64[idx]
    word0 = r | (c << 12)
    if T > 0:
        word0 = word0 | (voxel_bin(t64, T) << 24)
    x, y = ev[:, 0].astype(np.float64), ev[:, 1].astype(np.float64)
    frac = bool(((x[surv] != np.floor(x[surv])) | (y[surv] != np.floor(y[surv])) | outside[surv]).any())
    return {"idx": idx, "word0": word0, "word1": tau32[idx].view(np.uint32).astype(np.int64), "row": r, "col": c, "tau64": t64,
            "group_start": group_starts(group_of(r, c, t64, ntc, T), n_groups(size, T)),
            "dropped": int(ev.shape[0] - surv.size), "outside": int(outside.sum()), "fractional": frac}


def resort(prev_row, prev_col, prev_tau64, T, ntc):
    """Re-binning (`cmax_set_time_bins`): the stable order of an already packed sequence under the key of T time bins."""
    return stable_order(key(prev_row, prev_col, prev_tau64, ntc, T))


def slab_regroup(row, col, tau64, S, ntc):
    """`cmax_set_time_slabs` after its re-sort under S bins: whole groups move to (tile row, slab, tile column) order."""
    row, col = np.asarray(row, np.int64), np.asarray(col, np.int64)
    g = ((row >> 4) * S + voxel_bin(tau64, S)) * ntc + (col >> 4)
    return stable_order(g), g


def pass_plan(size, T, n_in, digit_bits=RS_MAX_DIGIT_BITS):
    """The passes `sort_events` runs (`radix_pass_plan`, csrc/cmax_batch_plan.h): dict(P, nb [P] digit widths lowest first, fine, nwg, range)."""
    digit_bits = min(RS_MAX_DIGIT_BITS, max(2, digit_bits))
    gb = 1
    while (1 << gb) < n_groups(size, T):
        gb += 1
    nb = []

    def split(total):
        parts = -(-total // digit_bits)
        done = 0
        for q in range(parts):
            bits = -(-(total - done) // (parts - q))
            nb.append(bits)
            done += bits

    if T == 0:
        split(8 + gb)
    else:
        if fine_key(T):
            nb.append(8)
        split(gb)
    nwg = min(RS_MAX_GROUPS, max(1, -(-n_in // RS_CHUNK)))
    rng = -(-(-(-n_in // nwg)) // RS_THREADS) * RS_THREADS
    return {"P": len(nb), "nb": nb, "fine": fine_key(T), "nwg": nwg, "range": rng}


def plan_text(size, T, n_in, digit_bits, slab=False, resort=False):
    """One entry of profiles/radix_small.txt: 'coarse' marks keys without the pixel byte, 'swap' a re-sort from the packed arrays whose
    pass 0 would write the arrays it reads ((P - 1) % 2 == 0: the handle's own arrays and the staging arrays swap roles first)."""
    p = pass_plan(size, T, n_in, digit_bits)
    return (f"T={T}{' slabs' if slab else ''}{'' if p['fine'] else ' coarse'} P={p['P']} nb={p['nb']} nwg={p['nwg']}"
            f"{' swap' if resort and (p['P'] - 1) % 2 == 0 else ''}")


# ---- the two-level COUNTING sort (csrc/cmax_sort_kernels.h): what it promises, and the comparison in canonical form --------------------
# Its key sequence and its group starts are a function of the batch; the order of the events of ONE key is whatever the LDS atomics of
# k_tile_sort produced -- except on un-binned handles, where k_run_time_sort then ranks every pixel run of 2 .. kRunSortMax events by
# (fp32 time, position).  So the comparison below holds the keys and the group starts element for element, the words of one key as a
# multiset, and the short runs of an un-binned handle by time.
RUN_SORT_MAX = 192        # kRunSortMax
RUN_SORT_CHUNK = 1024     # kRunSortChunk
RUN_SORT_HALO = 200       # kRunSortHalo
SORT_CHUNK = 4096         # kSortChunk
SORT_LDS_TILES = 4096     # kSortLdsTiles


def tau_residual8(tau64):
    """`tau_residual8`: the top byte of word 0 on un-binned handles -- what fp32 cannot hold of the normalised time, in units of
    ulp(hi) / 256, as a signed byte; 0 where the biased exponent of hi = float32(tau64) is below 32."""
    tau64 = np.asarray(tau64, np.float64)
    hi = tau64.astype(np.float32)
    eb = ((hi.view(np.uint32) >> 23) & 0xFF).astype(np.int64)
    unit = np.ldexp(1.0, np.maximum(eb, 32) - 31 - 127)   # ulp(hi) / 256
    q = np.clip(np.rint((tau64 - hi.astype(np.float64)) / unit), -128, 127).astype(np.int64)
    return np.where(eb < 32, 0, q & 0xFF)


def tau_refined(word1, byte):
    """(tau, unit): the time an un-binned packed event stands for, float32(word 1) + q * ulp / 256, and that unit (0 below 2^-95)."""
    hi = np.asarray(word1, np.int64).astype(np.uint32).view(np.float32)
    eb = ((hi.view(np.uint32) >> 23) & 0xFF).astype(np.int64)
    unit = np.where(eb < 32, 0.0, np.ldexp(1.0, np.maximum(eb, 32) - 31 - 127))
    b = np.asarray(byte, np.int64)
    return hi.astype(np.float64) + np.where(b >= 128, b - 256, b) * unit, unit


def counting_key(row, col, bins, ntc, T, slabs=False):
    """The key the packed sequence is ordered by, from what a packed event itself holds (pixel, time bin): `key`, or after
    `cmax_set_time_slabs` the group (tile row, slab, tile column) in front of the pixel."""
    row, col, bins = np.asarray(row, np.int64), np.asarray(col, np.int64), np.asarray(bins, np.int64)
    if T == 0:
        group = (row >> 4) * ntc + (col >> 4)
    elif slabs:
        group = ((row >> 4) * T + bins) * ntc + (col >> 4)
    else:
        group = ((row >> 4) * ntc + (col >> 4)) * T + bins
    return ((group << 8) | ((row & 15) << 4) | (col & 15) if fine_key(T) else group), group


def pixel_runs(row, col):
    """(start, length) of every run of equal source pixel of a sequence."""
    pix = np.asarray(row, np.int64) * 4096 + np.asarray(col, np.int64)
    if pix.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    start = np.flatnonzero(np.concatenate([[True], pix[1:] != pix[:-1]]))
    return start, np.diff(np.concatenate([start, [pix.size]]))


def counting_expected(ev, size, T=0, keep_outside=True, tmin=None, tmax=None, slabs=False):
    """What the counting sort must leave for a batch under T bins (slabs: after cmax_set_time_slabs(T)), in canonical order: by key,
    and inside a key by (word 1, top byte, input index) -- for un-binned handles that IS the order of the run sort wherever the fp32
    times of a pixel are distinct.  A function of the batch and T alone: re-sorting from the packed arrays must leave the same.
    dict of idx, word0 (top byte included), word1, key, group, row, col, tau64, group_start, T, slabs, dropped, outside, fractional,
    run_start / run_len (pixel runs, T == 0)."""
    ntc = (size[1] + 15) // 16
    x = expected_packed(ev, size, T, keep_outside, tmin, tmax)
    bins = voxel_bin(x["tau64"], T) if T > 0 else np.zeros(x["idx"].size, np.int64)
    word0 = x["word0"] | (tau_residual8(x["tau64"]) << 24) if T == 0 else x["word0"]
    k, group = counting_key(x["row"], x["col"], bins, ntc, T, slabs)
    o = np.lexsort((x["idx"], word0 >> 24, x["word1"], k)) if T == 0 else np.lexsort((x["idx"], k))
    out = {name: x[name][o] for name in ("idx", "word1", "row", "col", "tau64")}
    out.update(word0=word0[o], key=k[o], group=group[o], T=T, slabs=bool(slabs and T > 0), dropped=x["dropped"], outside=x["outside"],
               fractional=x["fractional"], group_start=group_starts(group[o], n_groups(size, T)))
    if T == 0:
        out["run_start"], out["run_len"] = pixel_runs(out["row"], out["col"])
    return out


def words(word0, word1):
    return (np.asarray(word0, np.int64) << 32) | np.asarray(word1, np.int64)


def compare_counting(tag, packed, gs, info, x, size, run_sorted=True, declared_long=()):
    """The canonical comparison of a packed sequence (packed [n, 2], group starts, batch_info as (packed, dropped, fractional,
    outside)) with `counting_expected`.  Raises AssertionError at the first of:
      1 length and batch_info;  2 key sequence, element for element (keys nondecreasing, every key with its count);
      3 group starts, element for element;  4 inside every key the multiset of 64-bit words;
      5 (T == 0, run_sorted) every pixel run of 2 .. 192 events nondecreasing in word 1, and equal to the expectation word for word
        where its fp32 times are distinct;  6 the runs excused from 5 are the runs above 192 events, and their lengths in packed order
        are `declared_long`."""
    packed, gs = np.asarray(packed, np.int64), np.asarray(gs, np.int64)
    T, n = x["T"], x["idx"].size
    ntc = (size[1] + 15) // 16
    assert packed.shape[0] == n, f"{tag}: {packed.shape[0]} packed events, expected {n}"
    assert (int(info[0]), int(info[1]), bool(info[2]), int(info[3])) == (n, x["dropped"], x["fractional"], x["outside"]), f"{tag}: batch_info {list(info)}"
    row, col, top = packed[:, 0] & 0xFFF, (packed[:, 0] >> 12) & 0xFFF, packed[:, 0] >> 24
    k, _ = counting_key(row, col, top if T > 0 else 0 * top, ntc, T, x["slabs"])
    np.testing.assert_array_equal(k, x["key"], err_msg=f"{tag}: key sequence")
    assert (np.diff(k) >= 0).all(), f"{tag}: keys decrease"
    ku, kc = np.unique(k, return_counts=True)
    eu, ec = np.unique(x["key"], return_counts=True)
    np.testing.assert_array_equal(ku, eu, err_msg=f"{tag}: keys present")
    np.testing.assert_array_equal(kc, ec, err_msg=f"{tag}: events per key")
    np.testing.assert_array_equal(gs, x["group_start"], err_msg=f"{tag}: group starts")
    got, want = words(packed[:, 0], packed[:, 1]), words(x["word0"], x["word1"])
    np.testing.assert_array_equal(got[np.lexsort((got, k))], want[np.lexsort((want, x["key"]))], err_msg=f"{tag}: words inside the keys")
    if T > 0 or not run_sorted:
        assert len(declared_long) == 0 or T == 0, f"{tag}: long runs declared on a binned step"
        return
    start, length = x["run_start"], x["run_len"]
    exempt = length > RUN_SORT_MAX
    assert list(length[exempt]) == list(declared_long), f"{tag}: runs above {RUN_SORT_MAX} events {list(length[exempt])}, declared {list(declared_long)}"
    run_of = np.repeat(np.arange(start.size), length)
    held = ~exempt[run_of]                         # (a run of 1 is held by point 4 already: nothing below can add to it)
    same_run = run_of[1:] == run_of[:-1]
    back = same_run & held[1:] & (packed[1:, 1] < packed[:-1, 1])
    assert not back.any(), f"{tag}: word 1 decreases inside a run of at most {RUN_SORT_MAX} events at packed positions {np.flatnonzero(back)[:8] + 1}"
    tied = np.zeros(start.size, bool)
    tied[run_of[1:][same_run & (x["word1"][1:] == x["word1"][:-1])]] = True
    exact = held & ~tied[run_of]
    np.testing.assert_array_equal(got[exact], want[exact], err_msg=f"{tag}: runs with distinct fp32 times, word for word")
