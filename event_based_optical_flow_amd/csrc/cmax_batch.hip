// The handle of the fused objective and everything done ONCE PER BATCH (cmax_set_events, cmax_set_time_bins / _slabs,
// cmax_set_event_weights): pack and order the events (cmax_sort_kernels.h, cmax_radix_sort.h -- this unit is the only one that
// includes them; the scan both pipelines use lives here), read back what the host needs, cut the sorted stream into the work list of
// the event kernels, upload it, and write the compact copy and the packed per-event weights.  What the host DECIDES on the way -- the
// cut and the radix sort's pass plan -- is cmax_batch_plan.h, plain C++ that tests/test_batch_plan_host.py runs on a CPU; this unit
// holds what launches, copies and allocates.  Everything done per evaluation is cmax_fused.hip.
#include <algorithm>

#include "cmax_fused_internal.h"
#include "cmax_sort_kernels.h"
#include "cmax_radix_sort.h"

// Environment knobs this unit reads (tuning experiments and A/B tests only; none changes results beyond rounding).  All are read once
// per process, at the first batch that gets there, except CMAX_NO_OWNED, which every cut reads again:
//   CMAX_NO_OWNED=1      never build the group-aligned "owned groups" work list (cmax_set_events)
//   CMAX_BIG_SEG=0 | 1   never / always big segments;  CMAX_MID_SEG=0 | 1  the same for mid segments;  CMAX_SMALL_ACC=0 | 1  for the small accumulators
//   CMAX_FREE_CUT=0 | 1  lists that are not owned: merge and split groups / cut every seg_max events, whatever the size (tuning only)
//   CMAX_SEG_CAP=n        free-cut work lists: events per segment (<= the layout's cap; profiles/r04_ablation.txt 18)
//   CMAX_NO_RUN_SORT=1   leave the events of a source pixel in the order the tile sort produced (no ordering by time)
//   CMAX_COMPACT=0       big segments read the plain 8-byte events instead of the 4.5-byte compact copy (fp32 time instead of 24-bit fixed point)
//   CMAX_DEBUG_COMPACT=1 cmax_set_events synchronises behind k_pack_compact and fails if an event did not fit its region's coordinates (tests read the flag
//                         with cmax_debug_compact_events instead)
//   CMAX_DEBUG_SEGS=1    one line per work list on stderr (tools/probe_rounds.py)
//   CMAX_SORT=radix | bucket   per-batch order by the stable radix sort (cmax_radix_sort.h) / the two-level counting sort, whatever the size
//   CMAX_RS_BITS=n       bits per digit of the radix sort, 2 .. 6 (tuning only)
namespace cmax {

// ---------------------------------------------------------------------------------------------
// set_events: pack + two-level sort (cmax_sort_kernels.h); the scan of the tile counts lives here
// ---------------------------------------------------------------------------------------------
__global__ void k_tmm_set(double *tmm, double lo, double hi) {
    tmm[0] = lo;
    tmm[1] = hi;
}

// Exclusive scan of counts[0..m) in place, counts[m] = total, in three small launches: sums of 2048-element
// chunks, scan of the chunk sums by one workgroup, scan inside every chunk (a single-workgroup scan of the
// 921k pixel keys of a 1280x720 sensor took 1.4 ms).
constexpr int kScanChunk = 2048;  // elements per workgroup (256 threads x 8)

// nonzero (optional): += number of keys with at least one event (one atomic per workgroup)
__global__ void __launch_bounds__(256) k_scan_sums(const int *__restrict__ counts, int m, int *__restrict__ chunk_sum, int *__restrict__ nonzero) {
    __shared__ int s_w[4], s_n[4];
    const int base = blockIdx.x * kScanChunk + threadIdx.x * 8;
    int s = 0, nz = 0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int c = base + u < m ? counts[base + u] : 0;
        s += c;
        nz += c != 0;
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        s += __shfl_xor(s, o, kWave);
        nz += __shfl_xor(nz, o, kWave);
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {
        s_w[threadIdx.x / kWave] = s;
        s_n[threadIdx.x / kWave] = nz;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        chunk_sum[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
        if (nonzero) atomicAdd(nonzero, s_n[0] + s_n[1] + s_n[2] + s_n[3]);
    }
}

// one workgroup: exclusive scan of the chunk sums in place (nchunk <= 1024 * per-thread loop), total -> *total_out
__global__ void __launch_bounds__(1024) k_scan_chunks(int *__restrict__ chunk_sum, int nchunk, int *__restrict__ total_out) {
    __shared__ int part[1024];
    const int t = threadIdx.x;
    const int per = (nchunk + 1023) / 1024;
    const int b = t * per, e = min(b + per, nchunk);
    int s = 0;
    for (int i = b; i < e; ++i) s += chunk_sum[i];
    part[t] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {  // Hillis-Steele inclusive scan of the per-thread totals
        int v = t >= o ? part[t - o] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - s;
    for (int i = b; i < e; ++i) {
        const int c = chunk_sum[i];
        chunk_sum[i] = run;
        run += c;
    }
    if (t == 1023) *total_out = part[1023];
}

__global__ void __launch_bounds__(256) k_scan_apply(int *__restrict__ counts, int m, const int *__restrict__ chunk_off) {
    __shared__ int s_w[4];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int base = blockIdx.x * kScanChunk + threadIdx.x * 8;
    int c[8], s = 0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        c[u] = base + u < m ? counts[base + u] : 0;
        s += c[u];
    }
    int incl = s;  // inclusive scan of the per-thread sums over the wave
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const int v = __shfl_up(incl, o, kWave);
        if (lane >= o) incl += v;
    }
    if (lane == kWave - 1) s_w[wave] = incl;
    __syncthreads();
    int run = chunk_off[blockIdx.x] + incl - s;
    for (int w = 0; w < wave; ++w) run += s_w[w];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        if (base + u < m) counts[base + u] = run;
        run += c[u];
    }
}

// m <= 4096: the whole scan in one workgroup (thread q owns counts[4q .. 4q+3]) instead of three launches
__global__ void __launch_bounds__(1024) k_scan_small(int *__restrict__ counts, int m) {
    __shared__ int s_w[1024 / kWave];
    const int t = threadIdx.x, lane = t & (kWave - 1), wave = t / kWave;
    int c[4], sum = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c[j] = 4 * t + j < m ? counts[4 * t + j] : 0;
        sum += c[j];
    }
    int incl = sum;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const int v = __shfl_up(incl, o, kWave);
        if (lane >= o) incl += v;
    }
    if (lane == kWave - 1) s_w[wave] = incl;
    __syncthreads();
    int run = incl - sum;
    for (int w = 0; w < wave; ++w) run += s_w[w];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (4 * t + j < m) counts[4 * t + j] = run;
        run += c[j];
    }
    if (t == 1023) counts[m] = run;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// exclusive scan of counts[0 .. m) in place, counts[m] = total (tmp: ceil(m / 2048) + 1 ints)
static void launch_scan_buf(int *counts, int m, int *tmp, hipStream_t s, int *nonzero = nullptr, int *total_out = nullptr) {
    const int nchunk = div_up(m, kScanChunk);
    hipLaunchKernelGGL(k_scan_sums, dim3(nchunk), dim3(256), 0, s, counts, m, tmp, nonzero);
    hipLaunchKernelGGL(k_scan_chunks, dim3(1), dim3(1024), 0, s, tmp, nchunk, total_out ? total_out : counts + m);
    hipLaunchKernelGGL(k_scan_apply, dim3(nchunk), dim3(256), 0, s, counts, m, tmp);
}
static void launch_scan(cmax_handle_s *h, int m, hipStream_t s, int *nonzero = nullptr) {
    if (m <= 4096 && !nonzero) {
        hipLaunchKernelGGL(k_scan_small, dim3(1), dim3(1024), 0, s, h->counts, m);
        return;
    }
    launch_scan_buf(h->counts, m, h->scan_tmp, s, nonzero);
}

// The event kernels read the sorted events in 16-byte pairs, so the pair that holds the last event of the last
// segment can reach one element past the batch.  That slot is not voted, but its pixel still indexes the flow
// field (dense / voxel warp): the two padding elements must decode to pixel (0, 0), bin 0 -- not to whatever the
// allocation held before.
static int pad_event_tail(cmax_handle_s *h, hipStream_t s) {
    CMAX_CHECK_HIP(hipMemsetAsync(h->evp + h->n, 0, 2 * sizeof(uint2), s));
    return 0;
}

// What the host reads back once per batch lives in ONE device allocation (cmax_handle_s::d_batch) and is mirrored by the pinned
// hp_read, as ints: [2 doubles] time extremes | [4] flags | [ntiles] active source pixels per tile | [ngroups + 1] group starts.
// flags: [0] any fractional source coordinate, [1] dropped events, [2] events kept from off the sensor (cmax_set_keep_outside),
// [3] raised by k_pack_compact (cmax_debug_compact_events).
struct ReadbackLayout {
    static constexpr int kTmm = 0, kFlags = 4, kActive = 8;
    static int64_t starts(int ntiles) { return kActive + ntiles; }
};

static int handle_groups(const cmax_handle_s *h) { return h->ntr * h->ntc * (h->n_time_bin > 0 ? h->n_time_bin : 1); }

static int env_int(const char *name, int unset) {
    const char *v = getenv(name);
    return v ? atoi(v) : unset;
}

static CutKnobs cut_knobs_from_env() {
    static const CutKnobs once = [] {
        CutKnobs k;
        k.big = env_int("CMAX_BIG_SEG", -1);
        k.mid = env_int("CMAX_MID_SEG", -1);
        k.small_acc = env_int("CMAX_SMALL_ACC", -1);
        k.free_cut = env_int("CMAX_FREE_CUT", -1);
        k.seg_cap = env_int("CMAX_SEG_CAP", 0);
        k.compact = env_int("CMAX_COMPACT", 1) != 0;
        return k;
    }();
    CutKnobs k = once;
    k.no_owned = getenv("CMAX_NO_OWNED") != nullptr;  // (tests switch it inside a running process)
    return k;
}

// ---- the stages of build_segments, in the order they enqueue ---------------------------------------------------------------------------
// The one device-to-host copy of a batch and what the handle keeps of it; `n_in` events went into the sort.
// overlap: launched (by the caller's functor) BEHIND the read-back copy and an event, i.e. work the GPU does while the host
// waits for that event only, cuts the segments and uploads them -- the ordering of the pixel runs by time (k_run_time_sort),
// which moves events inside their groups and leaves the group starts alone (round 3: 0.16 -> see profiles, per 1M events)
template <typename Overlap>
static int read_back_batch(cmax_handle_s *h, int64_t n_in, hipStream_t s, Overlap overlap) {
    const int ntiles = h->ntr * h->ntc;
    const int64_t nints = ReadbackLayout::starts(ntiles) + handle_groups(h) + 1;
    int rc = h->hp_read.reserve(nints);
    if (rc) return rc;
    CMAX_CHECK_HIP(hipMemcpyAsync(h->hp_read, h->d_batch, (size_t)nints * sizeof(int), hipMemcpyDeviceToHost, s));
    if (!h->read_done) CMAX_CHECK_HIP(hipEventCreateWithFlags(&h->read_done, hipEventDisableTiming));
    CMAX_CHECK_HIP(hipEventRecord(h->read_done, s));
    rc = overlap();
    if (rc) return rc;
    {  // busy-wait: hipEventSynchronize sleeps and wakes up tens of microseconds late
        hipError_t e;
        while ((e = hipEventQuery(h->read_done)) == hipErrorNotReady) {
        }
        CMAX_CHECK_HIP(e);
    }
    const int *flags = h->hp_read + ReadbackLayout::kFlags;
    h->has_frac = flags[0] != 0;
    h->n = n_in - flags[1];
    if (h->generation_counted != h->generation) {  // a new batch (re-binning keeps the count of cmax_set_events)
        h->n_dropped = flags[1];
        h->n_outside = flags[2];
        h->generation_counted = h->generation;
    }
    int64_t active = 0;  // source pixels that hold events (un-binned order)
    if (h->n_time_bin == 0)
        for (int k = 0; k < ntiles; ++k) active += h->hp_read[ReadbackLayout::kActive + k];
    h->long_runs = active > 0 && h->n >= 8 * active;
    double tmm[2];
    std::memcpy(tmm, h->hp_read + ReadbackLayout::kTmm, sizeof(tmm));
    h->tmin_host = tmm[0];
    h->tmax_host = tmm[1];
    return pad_event_tail(h, s);
}

static void adopt_work_list(cmax_handle_s *h, WorkList &wl) {
    h->big = wl.big;
    h->mid = wl.mid;
    h->owned = wl.owned;
    h->small_acc = wl.small_acc;
    h->seg_max = wl.seg_max;
    h->nseg = (int)wl.segs.size();
    h->row_seg_start.swap(wl.row_seg_start);
    static const bool debug_segs = getenv("CMAX_DEBUG_SEGS") != nullptr;  // tools/probe_rounds.py
    if (debug_segs)
        fprintf(stderr, "[cmax] work list: n=%lld groups=%d segments=%d owned=%d big=%d small_acc=%d\n", (long long)h->n, handle_groups(h), h->nseg, (int)h->owned,
                (int)h->big, (int)h->small_acc);
}

// the buffers every evaluation sizes by the work list
static int reserve_work_list(cmax_handle_s *h, hipStream_t s) {
    int rc = 0;
    if (h->nseg > h->d_segs.capacity()) {
        // the workspace of cmax_objective_batch is sized by the work list too (its layout: batch_seg_cap): allocated again on its next call
        rc = release_all(s, h->d_segs, h->d_gpart, h->d_win, h->d_shifts, h->bimg, h->braw, h->bwin, h->bshifts);
        if (rc) return rc;
        h->batch_cap = h->batch_seg_cap = 0;
    }
    bool fresh = false;
    rc = h->d_segs.reserve(&h->bytes, h->nseg, s);
    if (!rc) rc = h->d_win.reserve(&h->bytes, (int64_t)4 * h->nseg, s);
    if (!rc) rc = h->d_shifts.reserve(&h->bytes, (int64_t)4 * h->nseg * kShiftWordsMax, s, &fresh);
    if (!rc) rc = h->d_gpart.reserve(&h->bytes, (int64_t)4 * h->nseg * 2, s);
    if (rc) return rc;
    // (K3 reads an offset word only where K1 flagged its block; cleared once so that no word ever holds allocator garbage)
    if (fresh) CMAX_CHECK_HIP(hipMemsetAsync(h->d_shifts, 0, (size_t)h->d_shifts.capacity() * sizeof(unsigned), s));
    return 0;
}

static_assert(sizeof(Segment) == sizeof(int4) && offsetof(Segment, first) == offsetof(int4, x) && offsetof(Segment, count) == offsetof(int4, y) &&
                  offsetof(Segment, group0) == offsetof(int4, z) && offsetof(Segment, ngroups) == offsetof(int4, w),
              "the event kernels read a segment as an int4: (first, count, first group, groups)");

static int upload_segments(cmax_handle_s *h, const std::vector<Segment> &segs, hipStream_t s) {
    if (segs.empty()) return 0;
    // upload from pinned memory, no wait: the buffer is only rewritten after the event below has passed
    if (h->segs_copied) CMAX_CHECK_HIP(hipEventSynchronize(h->segs_copied));
    else CMAX_CHECK_HIP(hipEventCreateWithFlags(&h->segs_copied, hipEventDisableTiming));
    int rc = h->hp_segs.reserve((int64_t)segs.size());
    if (rc) return rc;
    std::memcpy(h->hp_segs, segs.data(), segs.size() * sizeof(Segment));
    CMAX_CHECK_HIP(hipMemcpyAsync(h->d_segs, h->hp_segs, segs.size() * sizeof(Segment), hipMemcpyHostToDevice, s));
    CMAX_CHECK_HIP(hipEventRecord(h->segs_copied, s));
    return 0;
}

// the compact copy of the current work list's events (k_pack_compact, cmax_event_launch.hip: the kernel is a template over the event layouts)
static int pack_compact_if_wanted(cmax_handle_s *h, bool wanted, hipStream_t s) {
    h->compact = false;
    if (!wanted) return 0;
    int rc = pack_compact_events(h, s);
    if (rc) return rc;
    static const bool debug_compact = getenv("CMAX_DEBUG_COMPACT") != nullptr;
    if (debug_compact) {  // (k_pack_compact raises d_flags[3] when an event lies outside its segment's tile row / 8-tile span: never)
        int bad = 0;
        CMAX_CHECK_HIP(hipMemcpyAsync(&bad, h->d_flags + 3, sizeof(int), hipMemcpyDeviceToHost, s));
        CMAX_CHECK_HIP(hipStreamSynchronize(s));
        if (bad) {
            set_error("k_pack_compact: an event does not fit the compact coordinates of its segment");
            return CMAX_ESTATE;
        }
    }
    h->compact = true;
    return 0;
}

// The work list of the sorted batch: read back, cut on the host (cut_work_list, cmax_batch_plan.h), upload.  One host synchronisation.
template <typename Overlap>
static int build_segments(cmax_handle_s *h, int64_t n_in, hipStream_t s, Overlap overlap) {
    int rc = read_back_batch(h, n_in, s, overlap);
    if (rc) return rc;
    const int *group_start = h->hp_read + ReadbackLayout::starts(h->ntr * h->ntc);
    WorkList wl = cut_work_list(group_start, h->ntr, h->ntc, h->n_time_bin, h->slab_major, h->n, h->long_runs, cut_knobs_from_env());
    if (wl.status == WorkList::kMidNotAligned) {
        h->mid = false;
        h->seg_max = kSegMax;
        set_error("build_segments: mid layout chosen for a work list that is not group-aligned");
        return CMAX_ESTATE;
    }
    adopt_work_list(h, wl);
    rc = reserve_work_list(h, s);
    if (!rc) rc = upload_segments(h, wl.segs, s);
    if (!rc) rc = pack_compact_if_wanted(h, wl.wants_compact, s);
    return rc;
}

// the handle's own event arrays and their staging copies change roles
static void swap_event_arrays(cmax_handle_s *h) {
    swap(h->evp, h->evp_alt);
    swap(h->rx, h->rx_alt);
    swap(h->ry, h->ry_alt);
    swap(h->rl, h->rl_alt);
    swap(h->tau64, h->tau64_alt);
    swap(h->src, h->src_alt);
}

// staging SoA of the bucket pass: as large as the handle's own arrays (cmax_set_events releases it when those grow)
static int reserve_staging(cmax_handle_s *h, hipStream_t s) {
    int rc = h->evp_alt.reserve(&h->bytes, h->evp.capacity(), s);
    if (!rc) rc = h->rx_alt.reserve(&h->bytes, h->rx.capacity(), s);
    if (!rc) rc = h->ry_alt.reserve(&h->bytes, h->ry.capacity(), s);
    if (!rc) rc = h->rl_alt.reserve(&h->bytes, h->rl.capacity(), s);
    if (!rc) rc = h->tau64_alt.reserve(&h->bytes, h->tau64.capacity(), s);
    if (!rc) rc = h->src_alt.reserve(&h->bytes, h->src.capacity(), s);
    return rc;
}

// The STABLE radix sort (cmax_radix_sort.h) by the passes of radix_pass_plan (cmax_batch_plan.h); `fin` and `stage` are the handle's
// own arrays and the staging copy on entry, and on return (they may have swapped roles) `fin` holds the sorted events.
template <typename SRC>
static int radix_sort_events(cmax_handle_s *h, const SRC &src, int64_t n_in, int first_flag, unsigned long long *keys, SortOut &stage, SortOut &fin, hipStream_t s) {
    const int ntiles = h->ntr * h->ntc, T = h->n_time_bin;
    static const int digit_bits = env_int("CMAX_RS_BITS", kRsMaxDigitBits);  // tuning only
    const RadixPlan p = radix_pass_plan(ntiles, T, n_in, digit_bits);
    CMAX_REQUIRE(p.planned, "sort_events: the radix sort's pass plan exceeds kRsMaxPasses");
    const RsKey key = {h->ntc, T, p.fine ? 1 : 0};
    const int ngroups_all = ntiles * (T > 0 ? T : 1), P = p.P, nwg = p.nwg;
    const int64_t range = p.range;
    int rc = p.need > h->rs_hist.capacity() ? release_all(s, h->rs_hist, h->rs_tmp) : 0;
    if (!rc) rc = h->rs_hist.reserve(&h->bytes, p.need, s);
    if (!rc) rc = h->rs_tmp.reserve(&h->bytes, div_up(p.need, (int64_t)kScanChunk) + 2, s);
    if (rc) return rc;
    hipLaunchKernelGGL(k_rs_clear, dim3(div_up(std::max(ntiles, 4), 256)), dim3(256), 0, s, h->d_active, ntiles, h->d_flags, first_flag, keys);
    if (!key.fine && keys)  // (the first digit needs the time bin: the batch's extremes first)
        hipLaunchKernelGGL((k_rs_time_extremes<SRC>), dim3(nwg), dim3(kRsThreads), 0, s, src, n_in, keys);
    // pass q writes buffer (P - 1 - q) % 2 (0: the handle's own arrays, 1: the staging copy), so that the last pass lands in the own arrays.
    // Re-binning reads the own arrays: when pass 0 would write them too, the two sets swap roles first (the source then IS the staging set).
    if (!std::is_same<SRC, RawSource<float>>::value && !std::is_same<SRC, RawSource<double>>::value && (P - 1) % 2 == 0) {
        swap_event_arrays(h);
        std::swap(stage, fin);
    }
    // the number of packed events (every pass's scan writes it again): where the other pipeline keeps its total, outside the histogram
    // buffer the next pass overwrites
    int *total = h->counts + ntiles;
    for (int q = 0; q < P; ++q) {
        const int nb = p.nb[q], sh = p.sh[q], D = 1 << nb, m = D * nwg;
        const SortOut &out = (P - 1 - q) % 2 == 0 ? fin : stage;
        const SortOut &in = (P - 1 - q) % 2 == 0 ? stage : fin;
        if (q == 0) hipLaunchKernelGGL((k_rs_hist_src<SRC>), dim3(nwg), dim3(kRsThreads), (size_t)D * sizeof(int), s, src, n_in, range, key, nb, h->rs_hist, h->d_flags, keys);
        else hipLaunchKernelGGL(k_rs_hist, dim3(nwg), dim3(kRsThreads), (size_t)D * sizeof(int), s, (const uint2 *)in.evp, (const int *)total, range, key, sh, nb, h->rs_hist);
        launch_scan_buf(h->rs_hist, m, h->rs_tmp, s, nullptr, total);
        const size_t lds = (size_t)D * (sizeof(int) + sizeof(unsigned long long));
        if (q == 0) hipLaunchKernelGGL((k_rs_scatter_src<SRC>), dim3(nwg), dim3(kRsThreads), lds, s, src, n_in, range, key, nb, (const int *)h->rs_hist, (const int *)h->d_flags, out);
        else hipLaunchKernelGGL(k_rs_scatter, dim3(nwg), dim3(kRsThreads), lds, s, in, (const int *)total, range, key, sh, nb, (const int *)h->rs_hist, (const int *)h->d_flags, out);
        CMAX_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_rs_meta, dim3(div_up(n_in, 256)), dim3(256), 0, s, (const uint2 *)fin.evp, (const int *)total, key, ngroups_all, h->d_tile_start,
                       T == 0 ? h->d_active : (int *)nullptr, std::max(1, ntiles), keys);
    CMAX_CHECK_LAUNCH();
    return 0;
}

// the two-level counting sort (cmax_sort_kernels.h): buckets per tile in `stage`, every tile ordered into `fin`
template <typename SRC>
static int counting_sort_events(cmax_handle_s *h, const SRC &src, int64_t n_in, int first_flag, unsigned long long *keys, const SortOut &stage, const SortOut &fin, hipStream_t s) {
    const int ntiles = h->ntr * h->ntc, T = h->n_time_bin;
    const int grid = (int)div_up(n_in, (int64_t)kSortChunk);
    hipLaunchKernelGGL(k_sort_clear, dim3(div_up(ntiles + 1, 256)), dim3(256), 0, s, h->counts, h->cursor, ntiles, h->d_flags, first_flag, keys);
    hipLaunchKernelGGL((k_bucket_hist<SRC>), dim3(grid), dim3(kSortThreads), 0, s, src, n_in, h->ntc, ntiles, h->counts, h->d_flags, keys);
    launch_scan(h, ntiles, s);
    hipLaunchKernelGGL((k_bucket_scatter<SRC>), dim3(grid), dim3(kSortThreads), 0, s, src, n_in, h->ntc, ntiles, T, h->counts, h->cursor, h->d_flags, stage);
    hipLaunchKernelGGL(k_tile_sort, dim3(ntiles), dim3(kTileSortThreads), 0, s, ntiles, T, h->counts, stage, fin, h->d_tile_start, h->d_active, h->d_flags, keys);
    CMAX_CHECK_LAUNCH();
    return 0;
}

// Order `n_in` events from `src` for h->n_time_bin (cmax_sort_kernels.h) into the handle's SoA, then build the work
// list.  first_flag: d_flags[first_flag .. 3] are cleared (0 for a new batch; 1 keeps "fractional sources" when re-binning).
template <typename SRC>
static int sort_events(cmax_handle_s *h, const SRC &src, int64_t n_in, bool reduce_time, int first_flag, hipStream_t s) {
    const int ntiles = h->ntr * h->ntc, T = h->n_time_bin;
    int rc = reserve_staging(h, s);
    if (rc) return rc;
    SortOut stage = {h->evp_alt, h->rx_alt, h->ry_alt, h->rl_alt, h->tau64_alt, h->src_alt};
    SortOut fin = {h->evp, h->rx, h->ry, h->rl, h->tau64, h->src};
    unsigned long long *keys = reduce_time ? reinterpret_cast<unsigned long long *>(h->d_tmm) : nullptr;
    // Large batches: the STABLE radix sort (cmax_radix_sort.h) -- every pass streams, the events of a pixel come out by time without
    // k_run_time_sort, and the packed order is a function of the batch alone.  Small ones (a few launches fewer) keep the counting sort.
    static const char *sort_env = getenv("CMAX_SORT");
    const bool radix = sort_env ? strcmp(sort_env, "radix") == 0 : n_in >= kRadixMinEvents;
    rc = radix ? radix_sort_events(h, src, n_in, first_flag, keys, stage, fin, s) : counting_sort_events(h, src, n_in, first_flag, keys, stage, fin, s);
    if (rc) return rc;
    if (T > 0 && h->slab_major) {  // slab-major group order (cmax_sort_kernels.h, S4b): final SoA -> staging SoA, the two swap roles
        const int ngroups = ntiles * T;
        hipLaunchKernelGGL(k_slab_offsets, dim3(1), dim3(1024), 0, s, h->d_tile_start, ngroups, h->ntc, T, h->cursor);
        hipLaunchKernelGGL(k_slab_regroup, dim3(ngroups), dim3(256), 0, s, h->d_tile_start, h->cursor, h->ntc, T, fin, stage, h->d_flags);
        CMAX_CHECK_LAUNCH();
        CMAX_CHECK_HIP(hipMemcpyAsync(h->d_tile_start, h->cursor, (size_t)(ngroups + 1) * sizeof(int), hipMemcpyDeviceToDevice, s));
        swap_event_arrays(h);
    }
    static const bool run_sort = !getenv("CMAX_NO_RUN_SORT");
    return build_segments(h, n_in, s, [&]() -> int {
        if (T == 0 && run_sort && !radix) {
            // pixel runs ordered by time: final SoA -> staging SoA, then the two swap roles (same capacities).  Runs on the GPU
            // while the host cuts the segments: it needs nothing from the host and changes nothing the host reads back.
            hipLaunchKernelGGL(k_run_time_sort, dim3(div_up(n_in, kRunSortChunk)), dim3(256), 0, s, fin, stage, h->counts + ntiles, h->d_flags);
            CMAX_CHECK_LAUNCH();
            swap_event_arrays(h);
        }
        return 0;
    });
}

bool handle_is_weighted(cmax_handle_t h) { return h && h->weighted; }

// ---- per-event weights (cmax_set_event_weights) -------------------------------------------------------------------------------
// W1: the caller's weights as fp32 in the caller's order (kept: a re-ordering of the batch gathers from them again); flags[3] != 0 if
// one of them is not finite.
template <typename T>
__global__ void __launch_bounds__(256) k_weights_keep(const T *__restrict__ w, int64_t n, float *__restrict__ w_user, unsigned *__restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = (float)w[i];
    w_user[i] = v;
    if (!(fabsf(v) <= 3.4028234e38f)) atomicOr(&flags[3], 1u);
}
// W2: packed order (slot l of a segment reads w_packed[first + l]) through the source index the sort carried, zeros in the padding behind
// the last event, and max |w| over the PACKED events (a dropped event drops its weight) as the bits of a non-negative float in flags[2].
__global__ void __launch_bounds__(256) k_weights_gather(const float *__restrict__ w_user, const int *__restrict__ src, int64_t n, int64_t n_pad,
                                                        float *__restrict__ w_packed, unsigned *__restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float v = 0.f;
    if (i < n) v = w_user[src[i]];
    if (i < n_pad) w_packed[i] = v;
    float m = fabsf(v);
    if (!(m <= 3.4028234e38f)) m = 0.f;  // (non-finite values are reported by k_weights_keep)
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, kWave));
    if ((threadIdx.x & (kWave - 1)) == 0 && m > 0.f) atomicMax(&flags[2], __float_as_uint(m));
}
// W3: (1 / wmax, wmax) for the event kernels -- plain stores of one thread
__global__ void k_weights_norm(float *__restrict__ wnorm) {
    const float wmax = __uint_as_float(reinterpret_cast<const unsigned *>(wnorm)[2]);
    wnorm[0] = wmax > 0.f ? 1.f / wmax : 0.f;
    wnorm[1] = wmax;
}

// the packed-order copy of the kept weights for the CURRENT order of the batch (after cmax_set_event_weights and after every re-ordering)
static int gather_weights(cmax_handle_s *h, hipStream_t s) {
    const int64_t n_pad = h->n + kWeightPad;
    int rc = h->w_packed.reserve(&h->bytes, n_pad, s);
    if (rc) return rc;
    unsigned *flags = reinterpret_cast<unsigned *>(h->d_wnorm.get());
    CMAX_CHECK_HIP(hipMemsetAsync(flags + 2, 0, sizeof(unsigned), s));
    hipLaunchKernelGGL(k_weights_gather, dim3(div_up(n_pad, 256)), dim3(256), 0, s, (const float *)h->w_user, (const int *)h->src, h->n, n_pad, h->w_packed, flags);
    hipLaunchKernelGGL(k_weights_norm, dim3(1), dim3(1), 0, s, h->d_wnorm);
    CMAX_CHECK_LAUNCH();
    h->orig_valid = false;  // the un-warped image is weighted too
    h->win_generation = ~(uint64_t)0;
    return 0;
}

}  // namespace cmax

using namespace cmax;

extern "C" {

int cmax_create(int H, int W, int ph, int pw, cmax_handle_t *out) {
    CMAX_REQUIRE(out != nullptr, "create: out");
    CMAX_REQUIRE(H > 0 && W > 0 && H <= 4096 && W <= 4096 && ph >= 0 && pw >= 0, "create: image size must be in 1..4096");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        set_error("no HIP device visible");
        return CMAX_ENODEV;
    }
    cmax_handle_s *h = new cmax_handle_s();
    h->H = H;
    h->W = W;
    h->ph = ph;
    h->pw = pw;
    h->Hp = H + 2 * ph;
    h->Wp = W + 2 * pw;
    CMAX_CHECK_HIP(hipGetDevice(&h->device));
    h->ntr = div_up(H, kTile);
    h->ntc = div_up(W, kTile);
    h->nkeys = h->ntr * h->ntc * kTile * kTile;
    const int64_t npix = (int64_t)h->Hp * h->Wp;
    int rc = h->imgs.reserve(&h->bytes, 2 * 5 * npix, nullptr);
    for (int k = 0; k < 5 && !rc; ++k) rc = h->iweb[k].reserve(&h->bytes, npix, nullptr);
    if (!rc) rc = h->G.reserve(&h->bytes, 4 * npix, nullptr);  // dL/dIWE of up to 4 reference times
    if (!rc) rc = h->Gt.reserve(&h->bytes, npix, nullptr);
    {
        const int ntiles = h->ntr * h->ntc;
        const int64_t nints = ReadbackLayout::starts(ntiles) + ((int64_t)ntiles * 256 + 1);  // tile starts: up to 255 time bins per tile
        if (!rc) rc = h->d_batch.reserve(&h->bytes, nints, nullptr);
        if (!rc) {
            h->d_tmm = reinterpret_cast<double *>(h->d_batch + ReadbackLayout::kTmm);
            h->d_flags = h->d_batch + ReadbackLayout::kFlags;
            h->d_active = h->d_batch + ReadbackLayout::kActive;
            h->d_tile_start = h->d_batch + ReadbackLayout::starts(ntiles);
        }
    }
    if (!rc) rc = h->d_stat.reserve(&h->bytes, kStatSlots * kStatStride, nullptr);
    if (!rc) rc = h->counts.reserve(&h->bytes, h->nkeys + 1, nullptr);
    if (!rc) rc = h->cursor.reserve(&h->bytes, h->nkeys, nullptr);
    if (!rc) rc = h->scan_tmp.reserve(&h->bytes, div_up(h->nkeys, kScanChunk) + 1, nullptr);
    if (!rc) rc = h->d_raw.reserve(&h->bytes, 4 * kRawStride, nullptr);
    if (!rc) rc = h->d_host_result.reserve(&h->bytes, 8, nullptr);
    if (!rc) rc = h->d_musum.reserve(&h->bytes, 2 * 4 * kMuStride, nullptr);
    if (!rc) rc = h->d_ticket.reserve(&h->bytes, kTicketLines * kTicketLineInts, nullptr);
    if (!rc && hipMemset(h->d_ticket, 0, kTicketLines * kTicketLineInts * sizeof(int)) != hipSuccess) {
        set_error("cmax_create: clearing the arrival counters failed");
        rc = CMAX_ENOMEM;
    }
    if (!rc && hipMemset(h->d_musum, 0, 2 * 4 * kMuStride * sizeof(double)) != hipSuccess) {
        set_error("cmax_create: clearing the accumulators failed");
        rc = CMAX_ENOMEM;
    }
    if (rc) {
        cmax_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

int cmax_destroy(cmax_handle_t h) {
    if (!h) return 0;
    comm_destroy(h->comm);
    h->comm = nullptr;
    if (h->comm_stream) (void)hipStreamDestroy(h->comm_stream);
    for (hipEvent_t e : h->band_ev) (void)hipEventDestroy(e);
    if (h->segs_copied) (void)hipEventDestroy(h->segs_copied);
    if (h->read_done) (void)hipEventDestroy(h->read_done);
    for (int c = 0; c < CMAX_PROF_CLASSES; ++c)
        for (hipEvent_t e : h->prof_ev[c]) (void)hipEventDestroy(e);
    delete h;  // (the buffers free themselves)
    return 0;
}

int cmax_set_events(cmax_handle_t h, const void *events, int dtype, int64_t n, int have_tminmax, double tmin, double tmax,
                    int n_time_bin, cmax_stream_t stream) {
    CMAX_REQUIRE(h != nullptr, "set_events: handle");
    CMAX_REQUIRE(n >= 0 && n < (int64_t)2147483647 && (n == 0 || events), "set_events: n / events");
    CMAX_REQUIRE(dtype == CMAX_F32 || dtype == CMAX_F64, "set_events: dtype");
    CMAX_REQUIRE(n_time_bin >= 0 && n_time_bin <= 255, "set_events: n_time_bin must be in 0..255");
    hipStream_t s = (hipStream_t)stream;
    h->orig_valid = false;
    h->n = 0;
    h->n_dropped = 0;
    h->n_outside = 0;
    h->weighted = false;  // weights belong to a batch (like time slabs)
    h->wmax_host = 0.0;
    h->n_in = n;
    ++h->generation;
    h->generation_counted = ~(uint64_t)0;
    {
        // All six arrays are freed before the first is allocated again.  Each one then answers for itself: an array that a failed
        // growth left empty is allocated by the next call, whatever that call's n.
        const bool grow = n > h->src.capacity();
        int rc = grow ? release_all(s, h->evp, h->rx, h->ry, h->rl, h->tau64, h->src) : 0;
        if (!rc) rc = h->evp.reserve(&h->bytes, n ? n + 2 : 0, s);  // +2: the vector loads may touch one event past the end
        if (!rc) rc = h->rx.reserve(&h->bytes, n, s);
        if (!rc) rc = h->ry.reserve(&h->bytes, n, s);
        if (!rc) rc = h->rl.reserve(&h->bytes, n, s);
        if (!rc) rc = h->tau64.reserve(&h->bytes, n, s);
        if (!rc) rc = h->src.reserve(&h->bytes, n, s);
        if (!rc && grow) rc = release_all(s, h->evp_alt, h->rx_alt, h->ry_alt, h->rl_alt, h->tau64_alt, h->src_alt);  // the staging SoA follows (sort_events)
        if (rc) return rc;
    }
    // global time extremes: given (a time slice of a larger batch), or reduced by the first sort kernel
    if (have_tminmax) {
        CMAX_REQUIRE(tmax >= tmin, "set_events: tmax < tmin");
        hipLaunchKernelGGL(k_tmm_set, dim3(1), dim3(1), 0, s, h->d_tmm, tmin, tmax);
        CMAX_CHECK_LAUNCH();
    } else if (n == 0) {
        hipLaunchKernelGGL(k_tmm_set, dim3(1), dim3(1), 0, s, h->d_tmm, (double)INFINITY, -(double)INFINITY);
        CMAX_CHECK_LAUNCH();
    }
    h->n_time_bin = n_time_bin;
    h->slab_major = false;  // the slab order is a property of the batch cmax_set_time_slabs re-ordered, not of the handle
    if (n == 0) {
        CMAX_CHECK_HIP(hipMemsetAsync(h->d_flags, 0, 4 * sizeof(int), s));
        h->has_frac = false;
        h->nseg = 0;
        return 0;
    }
    // pack + order (tile-major; by pixel or by time bin inside a tile) + work list; one host synchronisation
    const int keyed = have_tminmax ? 0 : 1;
    const int keep = h->keep_outside ? 1 : 0;
    if (dtype == CMAX_F32) return sort_events(h, RawSource<float>{(const float *)events, h->d_tmm, h->H, h->W, keyed, keep}, n, keyed != 0, 0, s);
    return sort_events(h, RawSource<double>{(const double *)events, h->d_tmm, h->H, h->W, keyed, keep}, n, keyed != 0, 0, s);
}

// Re-ordering the packed events (time bins, time slabs) makes a new work list but NOT a new batch: the events the batch dropped /
// kept from off the sensor were counted by cmax_set_events from the raw input; the re-sort reads the packed SoA with those flags
// cleared and must not overwrite the counts (the guards of the dense / voxel objectives read n_outside)
static void bump_generation_keep_counts(cmax_handle_s *h) {
    const bool counted = h->generation_counted == h->generation;
    ++h->generation;
    if (counted) h->generation_counted = h->generation;
}

// the shared tail of cmax_set_time_bins / cmax_set_time_slabs: re-order the packed events in place (through the staging SoA) for the
// handle's new n_time_bin / slab_major; [0] "fractional sources" stays what it was
static int resort_packed_events(cmax_handle_s *h, hipStream_t s) {
    bump_generation_keep_counts(h);
    if (h->n == 0) return 0;
    int rc = sort_events(h, PackedSource{h->evp, h->rx, h->ry, h->rl, h->tau64, h->has_frac ? 1 : 0, h->src}, h->n, false, 1, s);
    if (!rc && h->weighted) rc = gather_weights(h, s);  // the weights follow the new order
    return rc;
}

int cmax_set_time_bins(cmax_handle_t h, int n_time_bin, cmax_stream_t stream) {
    CMAX_REQUIRE(h != nullptr, "set_time_bins: handle");
    CMAX_REQUIRE(n_time_bin >= 0 && n_time_bin <= 255, "set_time_bins: n_time_bin must be in 0..255");
    if (n_time_bin == h->n_time_bin && !h->slab_major) return 0;
    h->n_time_bin = n_time_bin;
    h->slab_major = false;
    return resort_packed_events(h, (hipStream_t)stream);
}

int cmax_set_time_slabs(cmax_handle_t h, int n_slab, cmax_stream_t stream) {
    CMAX_REQUIRE(h != nullptr, "set_time_slabs: handle");
    CMAX_REQUIRE(n_slab >= 0 && n_slab <= 64, "set_time_slabs: n_slab must be in 0..64");
    if (n_slab <= 1) n_slab = 0;  // one slab is the un-binned order
    if (n_slab == 0 && !h->slab_major) return h->n_time_bin == 0 ? 0 : cmax_set_time_bins(h, 0, stream);
    if (n_slab == h->n_time_bin && h->slab_major) return 0;
    h->n_time_bin = n_slab;
    h->slab_major = n_slab > 0;
    return resort_packed_events(h, (hipStream_t)stream);
}

int cmax_set_event_weights(cmax_handle_t h, const void *weights, int dtype, int64_t n, cmax_stream_t stream) {
    CMAX_REQUIRE(h != nullptr, "set_event_weights: handle");
    hipStream_t s = (hipStream_t)stream;
    if (weights == nullptr) {  // back to the unweighted state: the kernels, instantiations and numbers of a handle that never had weights
        if (h->weighted) {
            h->weighted = false;
            h->wmax_host = 0.0;
            h->orig_valid = false;
            h->win_generation = ~(uint64_t)0;
            bump_generation_keep_counts(h);  // launch sequences captured in the other state (patch plans) are dropped
        }
        return 0;
    }
    CMAX_REQUIRE(dtype == CMAX_F32 || dtype == CMAX_F64, "set_event_weights: dtype");
    CMAX_REQUIRE(n == h->n_in, "set_event_weights: n must equal the n of the last cmax_set_events (one weight per event, in the caller's order)");
    if (h->deterministic) {
        set_error("set_event_weights: not built for deterministic mode (cmax_set_deterministic)");
        return CMAX_EUNSUPPORTED;
    }
    if (h->comm) {
        set_error("set_event_weights: not built for a handle with a communicator (cmax_comm_init)");
        return CMAX_EUNSUPPORTED;
    }
    if (n == 0) {
        h->weighted = true;
        h->wmax_host = 0.0;
        return 0;
    }
    int rc = h->d_wnorm.reserve(&h->bytes, 4, s);
    if (!rc) rc = h->w_user.reserve(&h->bytes, n, s);
    if (rc) return rc;
    unsigned *flags = reinterpret_cast<unsigned *>(h->d_wnorm.get());
    CMAX_CHECK_HIP(hipMemsetAsync(h->d_wnorm, 0, 4 * sizeof(float), s));
    if (dtype == CMAX_F32) hipLaunchKernelGGL((k_weights_keep<float>), dim3(div_up(n, 256)), dim3(256), 0, s, (const float *)weights, n, h->w_user, flags);
    else hipLaunchKernelGGL((k_weights_keep<double>), dim3(div_up(n, 256)), dim3(256), 0, s, (const double *)weights, n, h->w_user, flags);
    CMAX_CHECK_LAUNCH();
    rc = gather_weights(h, s);
    if (rc) return rc;
    // blocks once, like cmax_set_events: the non-finite flag and wmax for cmax_batch_weighted
    float host[4];
    CMAX_CHECK_HIP(hipMemcpyAsync(host, h->d_wnorm, sizeof(host), hipMemcpyDeviceToHost, s));
    CMAX_CHECK_HIP(hipStreamSynchronize(s));
    unsigned bad;
    std::memcpy(&bad, &host[3], sizeof(bad));
    if (bad) {
        h->weighted = false;
        h->wmax_host = 0.0;
        set_error("set_event_weights: weights must be finite in fp32, the format they are kept in (|w| <= 3.4e38; the handle is unweighted now)");
        return CMAX_EINVAL;
    }
    h->weighted = true;
    h->wmax_host = (double)host[1];
    bump_generation_keep_counts(h);
    return 0;
}

int cmax_batch_weighted(cmax_handle_t h, int *weighted, double *wmax_host) {
    CMAX_REQUIRE(h != nullptr, "batch_weighted: handle");
    if (weighted) *weighted = h->weighted ? 1 : 0;
    if (wmax_host) *wmax_host = h->weighted ? h->wmax_host : 0.0;
    return 0;
}

int cmax_batch_info(cmax_handle_t h, int64_t *n_packed, int64_t *n_dropped, int *has_fractional, int *owned_groups) {
    CMAX_REQUIRE(h != nullptr, "batch_info");
    if (n_packed) *n_packed = h->n;
    if (n_dropped) *n_dropped = h->n_dropped;
    if (has_fractional) *has_fractional = h->has_frac ? 1 : 0;
    if (owned_groups) *owned_groups = h->owned ? 1 : 0;
    return 0;
}

int cmax_set_keep_outside(cmax_handle_t h, int on) {
    CMAX_REQUIRE(h != nullptr, "set_keep_outside");
    h->keep_outside = on != 0;  // takes effect with the next cmax_set_events
    return 0;
}

int cmax_batch_outside(cmax_handle_t h, int64_t *n_outside) {
    CMAX_REQUIRE(h != nullptr && n_outside != nullptr, "batch_outside");
    *n_outside = h->n_outside;
    return 0;
}

int cmax_work_list_info(cmax_handle_t h, int *n_segments, int *segment_events, int *small_accumulators) {
    CMAX_REQUIRE(h != nullptr, "work_list_info");
    if (n_segments) *n_segments = h->nseg;
    if (segment_events) *segment_events = h->seg_max;
    if (small_accumulators) *small_accumulators = h->small_acc ? 1 : 0;
    return 0;
}

int cmax_handle_info(cmax_handle_t h, int64_t *n_events, int64_t *workspace_bytes) {
    CMAX_REQUIRE(h != nullptr, "handle_info");
    if (n_events) *n_events = h->n;
    if (workspace_bytes) *workspace_bytes = h->bytes;
    return 0;
}

int cmax_debug_packed_events(cmax_handle_t h, void *events_out, int *group_start_out, int *n_groups_host, cmax_stream_t stream) {
    CMAX_REQUIRE(h != nullptr && events_out != nullptr, "debug_packed_events");
    const int ngroups = handle_groups(h);
    if (n_groups_host) *n_groups_host = ngroups;
    if (h->n > 0) CMAX_CHECK_HIP(hipMemcpyAsync(events_out, h->evp, (size_t)h->n * sizeof(uint2), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (group_start_out && h->n == 0)  // (an empty batch is not sorted: d_tile_start holds whatever the allocation or the last batch left)
        CMAX_CHECK_HIP(hipMemsetAsync(group_start_out, 0, (size_t)(ngroups + 1) * sizeof(int), (hipStream_t)stream));
    else if (group_start_out)
        CMAX_CHECK_HIP(hipMemcpyAsync(group_start_out, h->d_tile_start, (size_t)(ngroups + 1) * sizeof(int), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

int cmax_debug_work_list(cmax_handle_t h, void *segments_out, int *n_segments_host, unsigned *flags_host, int *seg_max_host, cmax_stream_t stream) {
    CMAX_REQUIRE(h != nullptr, "debug_work_list");
    if (n_segments_host) *n_segments_host = h->nseg;
    if (flags_host)
        *flags_host = (h->big ? CMAX_WL_BIG : 0u) | (h->mid ? CMAX_WL_MID : 0u) | (h->owned ? CMAX_WL_OWNED : 0u) | (h->small_acc ? CMAX_WL_SMALL_ACC : 0u) |
                      ((h->slab_major && h->n_time_bin > 0) ? CMAX_WL_SLAB_MAJOR : 0u) | (h->compact ? CMAX_WL_COMPACT : 0u) | (h->long_runs ? CMAX_WL_LONG_RUNS : 0u);
    if (seg_max_host) *seg_max_host = h->seg_max;
    if (segments_out && h->nseg > 0)  // the list the kernels read, not the host's staging copy
        CMAX_CHECK_HIP(hipMemcpyAsync(segments_out, h->d_segs, (size_t)h->nseg * sizeof(int4), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

int cmax_debug_compact_events(cmax_handle_t h, void *regions_out, int *flag_host, cmax_stream_t stream) {
    CMAX_REQUIRE(h != nullptr && regions_out != nullptr, "debug_compact_events");
    if (!h->compact || h->nseg <= 0) {
        set_error("debug_compact_events: the current work list has no compact copy");
        return CMAX_ESTATE;
    }
    hipStream_t s = (hipStream_t)stream;
    CMAX_CHECK_HIP(hipMemcpyAsync(regions_out, h->cev, (size_t)h->nseg * (size_t)compact_region_bytes(), hipMemcpyDeviceToDevice, s));
    if (flag_host) {  // what k_pack_compact raised: an event that does not fit its segment's strip
        // (into the flag's own slot of the pinned read-back, which every cut has sized: read_back_batch)
        int *slot = h->hp_read + ReadbackLayout::kFlags + 3;
        CMAX_CHECK_HIP(hipMemcpyAsync(slot, h->d_flags + 3, sizeof(int), hipMemcpyDeviceToHost, s));
        CMAX_CHECK_HIP(hipStreamSynchronize(s));
        *flag_host = *slot;
    }
    return 0;
}

}  // extern "C"
