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
    """The passes `sort_events` runs: dict(P, nb [P] digit widths lowest first, fine, nwg, range)."""
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
