// The host's decisions about a batch, as pure functions of what the device reported: the cut of the sorted events into the work list of
// the event kernels (cut_work_list) and the passes of the radix sort (radix_pass_plan), with the constants both need.  Standard C++17
// only -- no HIP, no handle, no error text -- so that tests/batch_plan_check.cpp compiles it with a host compiler, under sanitizers, and
// holds it to the numpy restatements (tests/_worklist_ref.py, tests/_sort_ref.py) without a GPU.  cmax_batch.hip is the caller of both.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace cmax {

constexpr int kSparseSegment = 512;  // voxel K3: segments below this many events add straight to memory (no LDS accumulators)
constexpr int kTile = 16;  // source-pixel tile edge of the counting sort
constexpr int kSegMax = 2040;                 // events per segment (+1 for the even-aligned start still fits 2048);
                                              // |sum of votes| <= 2040 * 2^20 < 2^31
constexpr int kSegMid = 3064, kSegBig = 4088; // ... of MID and of BIG segments (cut_work_list)
constexpr int kAccCells = 3072;               // flow-gradient accumulator cells per channel in LDS (voxel K3): 12 (tile, bin) groups
constexpr int kAccCellsDense = 768;           // the same for the dense K3 with owned tiles: 3 source tiles
constexpr int kResidentGroups = 1024;         // workgroups of 512 threads the chip holds at once
constexpr int64_t kRadixMinEvents = 8000000;  // batches from here on are ordered by the stable radix sort (cmax_radix_sort.h): 8M events 550 vs 556 us,
                                              // 12M 765 vs 875, 20M 1177 vs 1419, 64M 3483 vs 4754 (profiles/r05_set_events.txt); below, the counting sort's fewer launches win
constexpr int kTileKeysMax = 8192;  // k_tile_sort: 32 KB of counters: (bin, pixel) keys up to T = 32
// the radix sort (cmax_radix_sort.h)
constexpr int kRsThreads = 512;          // R1 / R3
constexpr int kRsSlots = 4;              // events per thread and iteration of R3 (their loads are in flight together)
constexpr int kRsChunk = kRsThreads * kRsSlots;
constexpr int kRsMaxGroups = 1024;       // workgroups per pass (four per CU: all resident)
constexpr int kRsMaxDigitBits = 6;       // (see radix_pass_plan: a pass is as fast as its output streams are few)
constexpr int kRsMaxPasses = 16;

// One work item of the event kernels: `count` consecutive sorted events from `first`, which lie in the `ngroups` groups from `group0`.
// Uploaded as an int4 (cmax_batch.hip holds the static_assert).
struct Segment {
    int first, count, group0, ngroups;
};

// What the switches of the environment say about the cut (cut_knobs_from_env, cmax_batch.hip).  A/B runs and tuning only.
struct CutKnobs {
    int big = -1;         // CMAX_BIG_SEG: >= 0 overrides the choice of big segments
    int mid = -1;         // CMAX_MID_SEG: 0 never, > 0 whenever the mid cut is group-aligned, else the one-round rule
    int small_acc = -1;   // CMAX_SMALL_ACC: >= 0 overrides the small accumulators
    int free_cut = -1;    // CMAX_FREE_CUT (tuning only): >= 0 overrides the free cut
    int seg_cap = 0;      // CMAX_SEG_CAP (tuning only): > 0: events per segment of a free-cut list
    bool no_owned = false;  // CMAX_NO_OWNED: never build the group-aligned "owned groups" list
    bool compact = true;    // CMAX_COMPACT=0: no compact copy
};

struct WorkList {
    enum Status { kOk = 0, kMidNotAligned };  // kMidNotAligned: the mid layout was chosen for a list that is not group-aligned (no list is cut)
    Status status = kOk;
    std::vector<Segment> segs;
    bool big = false;        // BIG segments: up to kSegBig events
    bool mid = false;        // MID segments: up to kSegMid events, group-aligned lists only
    bool owned = false;      // every group (empty ones included) belongs to exactly one segment
    bool small_acc = false;  // binned handle, owned groups of <= 3 groups per segment (5 on mid lists)
    bool wants_compact = false;  // big segments of an un-binned handle with long runs: the list gets its compact copy
    int seg_max = kSegMax;   // events per segment of this list
    std::vector<int> row_seg_start;  // [ntr + 1] first segment of every source tile row (owned lists only)
};

// The group-aligned cut of one tile row, groups [r0, r0 + row_groups): whole consecutive groups are merged while they number at most
// `span_max` and hold at most `cut` events; emit(first group, groups, events) per segment.  No group may exceed `cut`.
template <class Emit>
inline void cut_row_aligned(const int *group_start, int r0, int row_groups, int cut, int span_max, Emit &&emit) {
    int g = r0;
    while (g < r0 + row_groups) {
        const int gs = g;
        int c = 0;
        while (g < r0 + row_groups && g - gs < span_max && c + (group_start[g + 1] - group_start[g]) <= cut) {
            c += group_start[g + 1] - group_start[g];
            ++g;
        }
        emit(gs, g - gs, c);
    }
}

inline bool groups_fit(const int *group_start, int ngroups, int cut) {
    for (int g = 0; g < ngroups; ++g)
        if (group_start[g + 1] - group_start[g] > cut) return false;
    return true;
}

// segments of the group-aligned cut; -1: a group exceeds `cut`
inline int aligned_count(const int *group_start, int ngroups, int row_groups, int cut, int span_max) {
    if (!groups_fit(group_start, ngroups, cut)) return -1;
    int cnt = 0;
    for (int r0 = 0; r0 < ngroups; r0 += row_groups) cut_row_aligned(group_start, r0, row_groups, cut, span_max, [&](int, int, int) { ++cnt; });
    return cnt;
}

// Work list of the event kernels from the sorted events.  group_start[] = first sorted event of every group, [ngroups] = n;
// a GROUP = one source tile (un-binned handles, n_time_bin == 0), one (tile, time bin), or -- slab-major handles -- one (tile row, slab,
// tile column).  Segments: <= kSegMax consecutive sorted events (fixed-point range) inside one tile row, spanning <= 12 groups
// (the flow-gradient accumulator of the voxel K3 holds kAccCells = 12 * 256 cells).  Two regimes, measured on MI355X:
//   * batches that fill the chip several times over (> 1024 full segments): cut every kSegMax events, group
//     boundaries ignored -- every workgroup full (dense K3 of cfg3 30 -> 25 us);
//   * smaller batches are latency-bound: small groups are merged while they fit, a group with more than
//     kSegMax events is split into EQUAL parts -- group-aligned windows are tighter and no workgroup is left
//     with a small remainder (cfg2: 2040 + 806 per tile -> 2 x 1423).
// long_runs: >= 8 events per active source pixel on average (un-binned handles).
inline WorkList cut_work_list(const int *group_start, int ntr, int ntc, int n_time_bin, bool slab_major, int64_t n, bool long_runs, const CutKnobs &knobs) {
    // slab-major handles (cmax_set_time_slabs): the groups are (tile row, slab, tile column) -- ntr * S rows of ntc groups, one group per
    // "tile" of that virtual grid; cut like an un-binned list, never owned (a source pixel belongs to S groups)
    const bool slab = slab_major && n_time_bin > 0;
    const int T = (n_time_bin > 0 && !slab) ? n_time_bin : 1;  // groups per tile
    const int ngroups = ntr * ntc * (slab ? n_time_bin : T);
    const int row_groups = ntc * T;
    WorkList wl;
    // un-binned handles: a segment spans <= 3 source tiles.  Sparse tiles used to be merged up to 12 wide; the LDS
    // window of such a segment (16 * span + displacement range wide) overflowed its 4096 words as soon as the motion
    // was a few pixels, and the clipped path (bounds tests, global atomics for the overflow) made those few workgroups
    // the tail of the launch: 1M events whose lower tile rows are sparse, K1 7.5 -> 6.9 us, K3 10.4 -> 7.3 us.
    // binned handles: 12 (tile, bin) groups, what the LDS accumulators of the voxel K3 hold -- unless every segment is
    // below kSparseSegment events anyway (then that kernel adds straight to memory): up to 3 tiles' worth of groups,
    // instead of ~100-event segments cut by the span (30k events, T = 10: 312 -> 125 segments)
    // BIG segments for batches that fill the chip many times over (CMAX_BIG_SEG=0 / 1 overrides for A/B runs): the per-workgroup
    // fixed costs of the event kernels are paid once per 4088 events instead of once per 2040.  Pays from ~2000 big segments on
    // (256 CUs x 3 resident workgroups, several rounds): measured (profiles/r03_ablation.txt 8) 20M events 104.3 -> 95.0 us per
    // evaluation, 64M events 323.6 -> 292.6; 5M events (1223 segments) 38.5 -> 38.2; below that fewer, longer workgroups LOSE
    // (2.5M events @720p 30.6 -> 33.1, 2M-event voxel batch 31.4 -> 33.5).
    // Between 522k and 8M events the choice follows the work list itself (tools/probe_rounds.py, profiles/r03_ablation.txt 17): both
    // group-aligned cuts are counted, and big segments are taken when they need <= 4/11 of the standard cut's workgroups (720p: 4M
    // events = 3600 one-tile segments of 1100 events vs 1200 three-tile ones, 41.5 -> 38.7 us; voxel T = 10: 4M events 47.1 -> 41.0)
    // -- at a ratio of 2 .. 2.5 the standard cut wins (cfg5's shard 30.6 vs 33.1, cfg4 31.4 vs 33.5) -- or, from 4M events on, when
    // the standard cut is not group-aligned at all (groups above 2040 events: 720p 7M 56.4 -> 47.9 us; cfg3 37.9 -> 36.9 us).
    // MID segments (round 4; CMAX_MID_SEG=0 / 1 overrides for A/B runs): 3064 events, four source tiles or five well-filled (tile, bin)
    // groups wide.  A launch of more workgroups than the chip holds at once (256 CUs x 4 workgroups of 512 threads) runs in rounds, and
    // every round pays the ~2.5 us a workgroup waits for its first loads again (tools/timeline.py): the standard cut of cfg5's shard is
    // 1693 workgroups -- two rounds, the second two thirds full -- this one 900 in ONE round; cfg4: 1258 -> 748.  Taken when it fits one
    // round where the standard cut does not.
    if (slab) {
        wl.big = false;
    } else if (knobs.big >= 0) {
        wl.big = knobs.big != 0;
    } else if (n >= (int64_t)8000000) {
        wl.big = true;
    } else if (n < (int64_t)256 * kSegMax) {
        wl.big = false;
    } else {
        const bool small_std = T > 1 && n >= (int64_t)480 * ngroups;  // (see small_acc below)
        const int std_n = aligned_count(group_start, ngroups, row_groups, kSegMax, T == 1 ? 3 : (small_std ? kAccCellsDense / 256 : kAccCells / 256));
        const int big_n = std_n >= 0 ? aligned_count(group_start, ngroups, row_groups, kSegBig, T == 1 ? 6 : kAccCells / 256) : -1;
        wl.big = std_n >= 0 ? (int64_t)std_n * 4 >= (int64_t)big_n * 11 : n >= (int64_t)4000000;
        if (!wl.big && knobs.mid != 0 && !knobs.no_owned) {
            const int mid_n = aligned_count(group_start, ngroups, row_groups, kSegMid, T == 1 ? 4 : (small_std ? 5 : kAccCells / 256));
            wl.mid = knobs.mid > 0 ? mid_n > 0 : (mid_n > 0 && mid_n <= kResidentGroups && std_n > kResidentGroups);
        }
    }
    wl.seg_max = wl.big ? kSegBig : (wl.mid ? kSegMid : kSegMax);
    const int seg_cut = wl.seg_max;
    int max_groups = T == 1 ? 3 : kAccCells / 256;
    const bool free_cut = knobs.free_cut >= 0 ? knobs.free_cut != 0 : n > (int64_t)1024 * kSegMax;
    // batches far below one full segment per CU (the solver's 30k-event slices): a workgroup walks its events
    // 8 (4) per thread, so 2040-event segments leave 15 workgroups with long serial work on a 256-CU chip.
    // Cap the segment at n / 512 (>= 256 events): cfg1-shaped K3 13 -> 5 us.
    int seg_cap = seg_cut;
    if (n < (int64_t)256 * kSegMax) seg_cap = (int)std::min<int64_t>(seg_cut, std::max<int64_t>(256, (n + 511) / 512));
    if (knobs.seg_cap > 0 && free_cut) seg_cap = std::min(seg_cut, knobs.seg_cap & ~1);
    if (T > 1 && seg_cap < kSparseSegment) max_groups = std::max(max_groups, 3 * T);
    // Owned groups (batches of at least one full segment per CU whose groups all fit a segment): every group -- empty
    // ones included -- belongs to exactly ONE segment made of whole consecutive groups of one tile row, at most 3 tiles
    // (LDS window) / kAccCells / 256 groups (LDS accumulators).  The flow-gradient kernel of a single-reference objective
    // then stores its groups' pixels instead of adding to them (k_grad, kGradOwned), and the buffer needs no clearing.
    wl.owned = n >= (int64_t)256 * kSegMax && !knobs.no_owned && !slab && groups_fit(group_start, ngroups, seg_cut);
    // Binned handles whose groups are dense (>= 480 events per (tile, bin) group on average: four groups would not fit a segment
    // anyway): segments of <= 3 groups, so that the voxel K3 needs 768 accumulator cells per channel instead of 3072 -- 40 KB of LDS
    // per workgroup instead of 58, i.e. FOUR 512-thread workgroups per CU with 4 events per thread instead of two 1024-thread ones
    // with 2 (the per-thread fixed costs of K3 are spread over twice the events).  CMAX_SMALL_ACC=0 / 1 overrides (A/B runs).
    wl.small_acc = T > 1 && wl.owned && !wl.big && (knobs.small_acc >= 0 ? knobs.small_acc != 0 : n >= (int64_t)480 * ngroups);
    if (wl.mid && !wl.owned) {  // (the mid layout exists for group-aligned work lists only: the caller falls back to the standard cut)
        wl.mid = false;
        wl.seg_max = kSegMax;
        wl.status = WorkList::kMidNotAligned;
        return wl;
    }
    if (wl.owned) {
        // dense: kAccCellsDense (x 2 for big segments)
        const int span_max = T == 1 ? (wl.big ? 6 : (wl.mid ? 4 : 3)) : (wl.small_acc ? (wl.mid ? 5 : kAccCellsDense / 256) : kAccCells / 256);
        for (int r0 = 0; r0 < ngroups; r0 += row_groups) {
            wl.row_seg_start.push_back((int)wl.segs.size());
            cut_row_aligned(group_start, r0, row_groups, seg_cut, span_max, [&](int g0, int groups, int events) { wl.segs.push_back({group_start[g0], events, g0, groups}); });
        }
        wl.row_seg_start.push_back((int)wl.segs.size());
    }
    int begin = 0, count = 0, row_of_begin = -1, g0 = 0, g_last = 0;
    auto close = [&]() {
        if (count > 0) wl.segs.push_back({begin, count, g0, g_last - g0 + 1});
        count = 0;
    };
    for (int g = 0; g < ngroups && !wl.owned; ++g) {
        int b = group_start[g], c = group_start[g + 1] - group_start[g];
        const int trow = (g / T) / ntc;
        if (c == 0) continue;
        if (count > 0 && (trow != row_of_begin || g - g0 + 1 > max_groups || (!free_cut && count + c > seg_cap))) close();
        int limit = seg_cap;
        if (!free_cut && c > seg_cap) {
            const int parts = (c + seg_cap - 1) / seg_cap;
            limit = (c + parts - 1) / parts;
        }
        while (c > 0) {
            if (count == 0) {
                begin = b;
                row_of_begin = trow;
                g0 = g;
            }
            g_last = g;
            const int take = c < limit - count ? c : limit - count;
            count += take;
            b += take;
            c -= take;
            if (count >= limit) close();
        }
    }
    close();
    // Big segments of an un-binned handle: the compact copy the hot kernels read (4.5 B/event, one aligned region per segment).
    // CMAX_COMPACT=0 switches it off (A/B runs).
    // ... and long runs only: the dense K3 of a short-run batch that is not `owned` is kGradStrided, whose slot layout reads the 8-byte
    // events -- K1 must then warp with the same fp32 time (K3 follows K1's cells and windows without tests), so such a handle gets no compact
    // copy at all (big segments + short runs = a sparse batch on a very large sensor, or CMAX_BIG_SEG=1).
    wl.wants_compact = wl.big && n_time_bin == 0 && !wl.segs.empty() && knobs.compact && long_runs;
    return wl;
}

// The passes of the stable radix sort (cmax_radix_sort.h) over the sort key of `ntiles` source tiles and `n_time_bin` bins or slabs.
// Digits of <= kRsMaxDigitBits bits: a pass writes one stream per (workgroup, digit), and its time follows the number of streams
// (64M events: 1.41 ms per pass at 1024 digits, 0.53 at 32 -- cmax_radix_sort.h), so more, narrower passes win.
// Un-binned handles: the whole key (8 pixel bits + tile bits) in equal digits -- every digit of it follows from the source pixel
// alone.  Binned handles: the pixel byte first (the time bin, which needs the batch's extremes, sits above it), then the group bits.
// (worst case: 2-bit digits -- un-binned 8 + 16 bits = 12 passes; fine binned, pixel byte + 21 bits = 12; coarse 24 bits = 12)
struct RadixPlan {
    bool planned = false;  // false: the key needs more than kRsMaxPasses passes
    int P = 0;             // passes
    int nb[kRsMaxPasses] = {}, sh[kRsMaxPasses] = {};  // bits and shift of every pass's digit, lowest first
    bool fine = false;     // the key holds the pixel byte (un-binned, or (bin, pixel) keys that fit k_tile_sort's counters)
    int nwg = 1;           // workgroups per pass
    int64_t range = 0;     // events per workgroup (a multiple of kRsThreads)
    int64_t need = 0;      // elements of the histogram: one counter per (digit, workgroup) of the widest pass + the total
};

inline RadixPlan radix_pass_plan(int ntiles, int n_time_bin, int64_t n_in, int digit_bits) {
    const auto ceil_div = [](int64_t a, int64_t b) { return (a + b - 1) / b; };
    const int T = n_time_bin;
    digit_bits = std::min(kRsMaxDigitBits, std::max(2, digit_bits));  // (CMAX_RS_BITS, tuning only)
    RadixPlan p;
    p.fine = T == 0 || T * 256 <= kTileKeysMax;
    const int ngroups_all = ntiles * (T > 0 ? T : 1);
    int gb = 1;
    while ((1 << gb) < ngroups_all) ++gb;
    int shift = 0;
    auto split = [&](int total_bits) {
        const int parts = (int)ceil_div(total_bits, digit_bits);
        if (p.P + parts > kRsMaxPasses) return false;
        for (int q = 0, done = 0; q < parts; ++q) {
            const int bits = (int)ceil_div(total_bits - done, parts - q);
            p.nb[p.P] = bits;
            p.sh[p.P++] = shift;
            shift += bits;
            done += bits;
        }
        return true;
    };
    if (T == 0) {
        p.planned = split(8 + gb);
    } else {
        if (p.fine) {
            p.nb[p.P] = 8;
            p.sh[p.P++] = 0;
            shift = 8;
        }
        p.planned = split(gb);
    }
    int maxbits = 0;
    for (int q = 0; q < p.P; ++q) maxbits = std::max(maxbits, p.nb[q]);
    p.nwg = (int)std::min<int64_t>(kRsMaxGroups, std::max<int64_t>(1, ceil_div(n_in, kRsChunk)));
    p.range = ceil_div(ceil_div(n_in, p.nwg), kRsThreads) * kRsThreads;
    p.need = ((int64_t)1 << maxbits) * p.nwg + 1;
    return p;
}

}  // namespace cmax
