// Private header of the fused contrast-maximization objective: what its three translation units share on the HOST side.
//   cmax_event_launch.hip  the per-event kernels (cmax_event_kernels.inc) and their launch layer, one launcher per kernel family
//   cmax_batch.hip         the handle's lifetime and everything done once per batch: pack, sort, scan, read-back, work list, compact
//                          copy, per-event weights (the host's decisions on the way: cmax_batch_plan.h, plain C++)
//   cmax_fused.hip         everything done per evaluation: the image-side kernels and the orchestration
// Kernel arguments, the handle, the constants the host sizes buffers with, and the declarations of the host functions that cross a
// unit (hidden: none of them is exported).  Device helpers shared by the event kernels and the image-side kernels live in
// cmax_fused_device.h.  Every kernel is compiled in exactly one unit (-fno-gpu-rdc).  Each unit lists the environment knobs it reads.
#pragma once

#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "cmax_batch_plan.h"
#include "cmax_buffers.h"
#include "cmax_comm.h"
#include "cmax_common.h"

namespace cmax {

// (kTile, kSegMax, kSparseSegment, kAccCells, kAccCellsDense and the other constants the host's per-batch decisions need: cmax_batch_plan.h)
constexpr int kWinMaxW = 128;                 // widest window when the bounding box has to be clipped
constexpr int kShiftWordsMax = 512;           // words of cell offsets per (reference time, segment): 4 bits per slot of a big segment
// (votes are accumulated as signed fixed point in the LDS windows: 12.20, big segments 13.19 -- kFixNS of cmax_event_kernels.inc)

struct EvView {
    const uint2 *ev;      // .x = row | col << 12 | bin << 24 ; .y = bits of fp32 tau = (t - tmin) / (tmax - tmin)
    const float *rx;      // fractional residual of the source coordinate (nullptr if integral)
    const float *ry;
    const float2 *rl;     // ... its low part (rxl, ryl): residual = (double)rx + (double)rxl -- read only by warp_exact (events on a cell border)
    const double *tau64;  // BINNED handles (the packed word's top byte holds the voxel bin): normalised time in fp64, same order as `ev` --
                          // read only for the few events whose cell is decided in fp64 (warp_exact); null on un-binned handles, whose
                          // packed word carries the time's residual beyond fp32 (tau_refined)
};

struct WarpParams {
    int H, W, Hp, Wp, ph, pw;  // un-padded sensor, padded image, padding
    int T;                     // voxel bins
    int ntc;                   // source tiles per tile row
    float d;                   // reference time as a fraction of the batch period
    float d_lo;                // ... what fp32 could not hold of it (d64 = (double)d + (double)d_lo): read only by warp_exact
    int normalize;             // normalize_t
    int motion_f64;            // cmax_objective_t::motion_dtype == CMAX_F64.  2-DoF: `motion` points to double[2].  Dense / voxel: `motion` is the high
                               // plane of the caller's doubles and the low plane lies behind it (k_split_motion); read by the HOST only, which
                               // launches the deciding kernels' ExactFlow instantiations (phase_warp's F64FLOW)
    const double *tmm;         // device (tmin, tmax)
    const float *motion;       // theta[2] | flow[2,H,W] | voxel[T,2,H,W]
};

// Trailing kernel argument of K1, k_vote_tan and k_grad_hvp for a dense / voxel motion that crossed the boundary in fp64: selects the
// instantiation whose border branch reads the low plane (nothing is read from the value)
struct ExactFlow {
    int on;
};

// One launch of an event kernel covers every reference time of the objective (blockIdx.y): a multi-focal cost
// warps the same events to 3 reference times, and on the solver's small batches three dependent launches per
// kernel class were three times the launch latency.
struct RefArgs {
    float d[4];       // reference time as a fraction of the batch period
    float d_lo[4];    // ... its fp32 remainder (K1's fp64 cell decisions: a reference time need not be a dyadic fraction -- "random" / float directions)
    float *img[4];    // K1: vote image to fill; K3: image to gather from (dL/dIWE or the IWE itself)
    double *stat[4];  // K1: statistics accumulators to reset (or null)
    double *raw_zero; // K1: [n_ref][kRawStride] gradient-sum lines of the 2-DoF K3 of the same evaluation to reset (or null)
    float *zero[4];   // K3, deferred statistics: vote image of the NEXT evaluation to clear (or null)
    int k0;           // index of the first reference time of this launch (statistics slot, partial-sum offset)
    int4 *win;        // [n_ref][nseg] LDS windows: written by K1, read by K3 of the same evaluation (or null)
    unsigned *shifts; // [n_ref][nseg][kSlots / 8] cell offsets of the events K1 decided in fp64 (phase_warp), 8 slots per word; valid where Window::bmask says so
    int windows_only; // K1: publish the windows (and offsets) and return -- for a K3 whose vote this was not (cmax_objective_finish)
    // cmax_objective_batch: blockIdx.z = candidate motion.  Element strides between consecutive candidates (0 for every other launch):
    int64_t z_img;    // floats between their vote images (img[k] / zero[k] are candidate 0's)
    int64_t z_raw;    // doubles between their raw-sum lines (stat[k] of K1, gpart of K3)
    int z_motion;     // floats between their motions.  The ONE source: the launchers copy it into K1's leading z_motion / the 2-DoF K3's
                      // head word (where the head needs it in an SGPR); every other read, the flow models' K3 included, is of this field
    // K3, deferred statistics: pixels (zero_chunk) and float4s (zero_chunk4) of zero[k] each workgroup clears = ceil(. / nseg), set by launch_grad
    int zero_chunk, zero_chunk4;
    // K1, blurred variance with a gradient: sum_p I[p] B[p] (B = blur^T 1_Omega = b(r) b(c)) = the sum of the blurred image over
    // Omega, accumulated while the votes are flushed -- the image kernel then knows the mean before it has blurred anything
    double *musum[4];        // kMuLines accumulators (one 128-byte line each) per reference time, or null
    // K3, kFoldStatsInside: musum[k] is READ (the mean), and
    int stat_blocks;         // leading workgroups of the grid that run the statistics (a multiple of 8: the XCD map of the others holds)
    int *ticket;             // their arrival counters (kTicketLines lines, zero between launches): the last one writes the loss
    double *musum_next;      // the other buffer of the vote sums: cleared for the next evaluation
    float band_b0, band_b1;  // b(0) = b(n - 1) and b(1) = b(n - 2) of border_weight (b = 1 elsewhere)
    // deterministic mode (cmax_set_deterministic): order-free integer accumulation
    long long *img64[4];       // K1: 2^-20 fixed-point vote image, 64-bit integer atomics instead of fp32 ones (or null)
    const unsigned *imax;      // K3: bits of max |image k| per statistics slot (the bound the fixed-point scale is derived from)
    long long *g64;            // K3: 2-DoF per-segment partial sums [n_ref][nseg][2] / flow-gradient accumulators, fixed point
    double *det_inv_scale;     // K3: [4] 1 / scale used by reference time k (2-DoF) or by all of them ([0], flow gradient)
    long long n_events;        // K3: events behind one accumulator at most (fixed-point headroom)
    // K1: the flow-gradient buffer the K3 of this evaluation ADDS into (work lists that are not group-aligned), cleared slice by slice
    // behind the event loads -- so that the statistics can run inside the K3 launch there too (kFoldStatsInside) instead of in a
    // launch of their own whose second job this was
    float4 *grad_zero;
    int64_t n_grad_zero4;
    // weighted handles (cmax_set_event_weights; the WEIGHTED instantiations of K1 / K3 only): per-event weights in packed order and
    // (1 / wmax, wmax) in device memory -- K1 votes round(w / wmax * K) and folds wmax back in when it flushes, K3 multiplies dt by w
    const float *wgt;
    const float *wnorm;
};

// the image-space kernels of an evaluation cover all reference times in one launch as well (blockIdx.y)
struct ImgArgs {
    const float *in[4];  // raw votes or blurred image, per reference time
    float *blurred[4];   // blurred image to write (kernels that blur)
    float *zero[4];      // vote image of the next evaluation to clear (or null)
    float *G[4];         // dL/dIWE to write
    float chain[4];      // fused statistics + G kernels: chain factor to fold into G (a constant of a cost that is not normalised;
                         // 1 when it depends on the finished statistics and K3 applies it: kFoldScale)
};

}  // namespace cmax

struct cmax_handle_s {
    int H = 0, W = 0, ph = 0, pw = 0, Hp = 0, Wp = 0;
    int device = 0;
    int64_t bytes = 0;  // HBM held by the buffers below (cmax_handle_info): declared before them, their destructors take their bytes off
    int64_t n = 0;
    int64_t n_dropped = 0;  // events of the last batch whose source pixel was off the sensor (or NaN): not packed
    bool keep_outside = true;  // cmax_set_keep_outside (default since round 5): finite events off the sensor are packed (nearest sensor pixel + residual)
    int64_t n_outside = 0;      // ... how many of the last batch (2-DoF objectives only: a flow has no value there)
    bool has_frac = false;
    int n_time_bin = 0;
    bool slab_major = false;  // the (tile, bin) groups are ordered (tile row, time slab, tile column): cmax_set_time_slabs (large motions)
    // packed, sorted events
    cmax::DevBuf<uint2> evp;  // packed events, 8 B each, 16-byte aligned base (+2 elements of padding)
    cmax::DevBuf<float> rx, ry;
    cmax::DevBuf<float2> rl;  // low parts of (rx, ry): written and read only for batches with fractional sources
    cmax::DevBuf<double> tau64;
    cmax::DevBuf<int> src, src_alt;  // index of every packed event in the caller's array, carried through every re-ordering
    // per-event weights (cmax_set_event_weights): the caller's values in the caller's order, the same gathered into packed order (slot l of a
    // segment reads w_packed[first + l]; padded with zeros so that the event kernels load unconditionally), and the normalisation
    cmax::DevBuf<float> w_user, w_packed;
    cmax::DevBuf<float> d_wnorm;  // [0] = 1 / wmax (0 when wmax == 0), [1] = wmax = max |w|, [2] = bits of wmax (reduction), [3] = non-finite flag
    bool weighted = false;
    double wmax_host = 0.0;
    int64_t n_in = 0;          // events handed to the last cmax_set_events
    // cmax_objective_weight_grad: finished dL/dIWE images ([5][npix]: reference times 0..3, slot 4 = the un-warped image) and their
    // blur-transpose input, the per-event interpolations in packed order (one plane of gw_plane floats per image), all allocated on first use;
    // general_only: the evaluation inside that call takes the general K1 -> statistics / image kernel -> K3 path on any handle
    cmax::DevBuf<float> gw_G, gw_Gt, gw_packed;
    int64_t gw_plane = 0;
    bool general_only = false;
    // cmax_objective_event_grad: (gx, gy, c) per packed event, three planes of ge_plane floats per reference time + two for the un-warped image,
    // and the scatter's per-workgroup partial sums of c ([4][workgroups]); allocated on first use, grown on demand
    cmax::DevBuf<float> ge_packed;
    int64_t ge_plane = 0;
    cmax::DevBuf<double> ge_part;
    // staging SoA of the two-level sort (tile buckets before the per-tile ordering)
    cmax::DevBuf<uint2> evp_alt;
    cmax::DevBuf<float> rx_alt, ry_alt;
    cmax::DevBuf<float2> rl_alt;
    cmax::DevBuf<double> tau64_alt;
    // sort scratch
    cmax::DevBuf<int> counts;  // [nkeys + 1] events per tile -> tile offsets after the scan
    cmax::DevBuf<int> cursor;  // [nkeys] per-tile cursor of the bucket pass, then active source pixels per tile
    cmax::DevBuf<int> scan_tmp;  // [ceil(nkeys / 2048)] chunk sums of the scan
    cmax::DevBuf<int> rs_hist;   // radix sort (large batches): [digits][workgroups] + 1 histogram / offsets of one pass
    cmax::DevBuf<int> rs_tmp;    // ... chunk sums of its scan
    int nkeys = 0, ntr = 0, ntc = 0;
    int *d_flags = nullptr;  // [0] any fractional source coordinate, [1] dropped events, [2] events kept from off the sensor (cmax_set_keep_outside)
    bool long_runs = false;  // >= 8 events per active source pixel on average: the dense K3 reduces runs serially per thread
    bool mid = false;        // MID segments: up to 3064 events, four source tiles (five (tile, bin) groups) wide, event kernels of the m512 namespace -- when the
                             // standard cut would need more workgroups than the chip holds at once and this one does not (cut_work_list)
    bool big = false;        // BIG segments: up to 4088 events each, event kernels of the b512 / b1024 namespaces (batches of >= 8M events)
    int seg_max = cmax::kSegMax;  // events per segment of the current work list (kSegMax, kSegMid or kSegBig)
    bool small_acc = false;  // binned handle, owned groups of <= 3 groups per segment: the voxel K3 with kAccCellsDense accumulator cells (kGradOwnedSmall)
    bool owned = false;      // the work list gives every group (empty ones included) to exactly one segment, <= kAccCells / 256 groups each
    int *d_tile_start = nullptr;  // [ngroups + 1] first sorted event of every group (source tile, or (tile, time bin))
    // What the host reads back once per batch lives in ONE allocation, in this order: d_tmm (2 doubles) | d_flags (4 ints) |
    // d_active (ntiles ints) | d_tile_start (...) -- ReadbackLayout, cmax_batch.hip: one device-to-host copy instead of four (each ~4 us of copy latency)
    cmax::DevBuf<int> d_batch;   // base of that allocation (as ints)
    int *d_active = nullptr;  // [ntiles] source pixels that hold events, per tile (un-binned order; written by k_tile_sort)
    cmax::DevBuf<int4> d_segs;       // [nseg] (begin, count, first source tile, tiles spanned): work items of the event kernels
    cmax::DevBuf<int4> d_win;        // [4][nseg] LDS windows of the last objective vote (K1 -> K3 of the same evaluation)
    // compact copy of the sorted events, one region per segment of the work list (EventLoads in cmax_event_kernels.inc): big segments of
    // un-binned handles; valid for the current work list only (build_segments, cmax_batch.hip)
    cmax::DevBuf<char> cev;
    bool compact = false;
    // cmax_objective_batch: K candidate motions per launch (allocated on first use, sized for batch_cap candidates)
    cmax::DevBuf<float> bimg;        // [2 buffers][batch_cap][n_ref <= 4][npix] vote images
    cmax::DevBuf<double> braw;       // [batch_cap][4][kRawStride] raw sums
    cmax::DevBuf<int4> bwin;         // [batch_cap][4][nseg] windows
    cmax::DevBuf<unsigned> bshifts;  // [batch_cap][4][nseg][kShiftWordsMax]
    int batch_cap = 0, batch_seg_cap = 0, batch_cur = 0;
    int batch_zero[2] = {0, 0};  // the first batch_zero[b] images of buffer b are zero
    cmax::DevBuf<unsigned> d_shifts; // [4][nseg][kShiftWordsMax] cell offsets of the events that vote decided in fp64 (RefArgs::shifts)
    // what those windows were computed for: K3 reuses them only for the same motion / model / reference times
    const float *win_motion = nullptr;
    int win_model = -2, win_nref = 0, win_T = 0, win_normalize = 0;
    float win_d[4] = {0.f, 0.f, 0.f, 0.f};
    uint64_t win_generation = ~(uint64_t)0;
    int nseg = 0;
    // images
    cmax::DevBuf<float> imgs;                               // [2 buffers][5, Hp, Wp] raw votes: one per reference time + un-warped
    cmax::DevBuf<float> iweb[5];                            // blurred copies
    cmax::DevBuf<float> G, Gt;
    const float *last_iwe[4] = {nullptr, nullptr, nullptr, nullptr};
    // device scalars
    double *d_tmm = nullptr;  // [2]
    cmax::DevBuf<double> d_stat;   // [5 slots][32 sub-accumulators][2] contrast statistics (slot 4 = un-warped image)
    // the handle's own vote images are double-buffered: k_stats of evaluation e zeroes the images of
    // evaluation e+1, so the steady state needs no memset node.  zero_mask[b] bit k: image k of buffer b is zero
    int cur_buf = 0;
    unsigned zero_mask[2] = {0u, 0u};
    cmax::DevBuf<double> d_gpart;  // [4 reference times][nseg][2] per-segment 2-DoF partials
    cmax::DevBuf<double> d_raw;    // [4 reference times][kRawStride] raw sums of the deferred 2-DoF K3 (cmax_objective's own copy)
    // cmax_objective_host: device outputs + pinned staging of one evaluation whose results go straight to the host
    cmax::DevBuf<double> d_host_result;  // [8]
    cmax::DevBuf<char> d_host_grad;
    // The one pinned block of the calls that hand results to the host (cmax_objective_host, cmax_objective_descend[_batch]), in doubles.
    // A fixed head: the result block a finishing kernel or a descent's last step writes, two staged doubles (the polled 2-DoF gradient
    // coming back, theta0 going out) and the run counter those kernels store behind their results.  Everything of variable size -- the
    // gradient of cmax_objective_host's copy path, theta0[K] and the K states of a batch descent -- starts at kHpPayload: no payload
    // reaches the counter.  Kernels are given hp_out.dev() + these offsets.
    static constexpr int kHpResult = 0, kHpStaged = 8, kHpCounter = 16, kHpPayload = 24;
    cmax::PinnedBuf<double> hp_out;
    static volatile unsigned long long *hp_counter(double *block) { return reinterpret_cast<volatile unsigned long long *>(block + kHpCounter); }
    unsigned long long host_seq = 0;  // the last value a polled call had its kernel store there
    cmax::DevBuf<double> descent;     // cmax_objective_descend (on first use): theta[2] | grad[2] | pad[4] | result[8] | the descent state (cmax_descent.h)
    cmax::DevBuf<double> lbfgs;       // cmax_objective_lbfgs (on first use): theta[2] | grad[2] | pad[4] | result[8] | the L-BFGS state (cmax_lbfgs.h)
    // cmax_objective_descend_batch (on first use): theta[K][2] | grad[K][2] | pad[K][4] | result[K][8] | K descent states
    cmax::DevBuf<double> descent_batch;
    cmax::DevBuf<int> d_ticket;    // arrival counters of the statistics workgroups inside K3 (kFoldStatsInside): zero between launches
    cmax::DevBuf<double> d_musum;  // [2 buffers][4 reference times][kMuStride] K1's sums for the blurred variance (RefArgs::musum)
    int mu_buf = 0;             // buffer the next evaluation adds into (the other one is being cleared / is clear); flipped by the launch that reads the sums
    // orig-IWE cache key
    bool orig_valid = false;
    double orig_sigma = -1;
    int orig_cost = -1, orig_omit = -1;
    double tmin_host = 0.0, tmax_host = 0.0;  // batch extremes (copied once per batch)
    cmax::DevBuf<float> hvp_img;              // [6 kinds][4 reference times][Hp, Wp] scratch of cmax_objective_hvp (allocated on first use)
    cmax::DevBuf<float> iw_zero;              // cmax_iwes_vjp: a zero tangent of the motion's size (the gather of J^T G is T3 with u = 0, G' = G)
    cmax::DevBuf<double> d_stat_tan;          // [4][kStatStride] tangent statistics
    // pinned host staging of the per-batch read-back (group starts, active pixels per tile, flags, time extremes) and
    // of the work list: copies to / from pageable memory are staged by the runtime and cost a synchronisation each
    cmax::PinnedBuf<int> hp_read;
    cmax::PinnedBuf<int4> hp_segs;
    hipEvent_t segs_copied = nullptr;  // the last upload of hp_segs has left the host buffer
    hipEvent_t read_done = nullptr;    // the per-batch read-back has arrived (the stream may still be busy behind it)
    cmax::DevBuf<float2> search_range;        // (tau_min, tau_max) per patch of cmax_patch_search
    uint64_t generation = 0;  // bumped by set_events / set_time_bins (device pointers and the work list change)
    uint64_t generation_counted = ~(uint64_t)0;
    // optional per-kernel-class timing with HIP events (cmax_set_profiling)
    bool profiling = false;
    int prof_repeat = 1;  // > 1: every hot launch is issued this many times inside its event bracket (timing only)
    std::vector<hipEvent_t> prof_ev[CMAX_PROF_CLASSES];  // class -> [start0, stop0, start1, stop1, ...]
    // 2-DoF tangent images (k_vote_tan2): [2 buffers][4 reference times][I: Hp Wp | E0: (Hp + 1) Wp | F1: Hp (Wp + 1)]
    cmax::DevBuf<float> tan;
    int tan_cur = 0;
    unsigned tan_zero_mask[2] = {0u, 0u};  // bit k: planes of reference time k of buffer b are zero
    cmax::DevBuf<double> d_tanpart;        // [4][kTanBlocks][6] partial sums of k_tan_stats_var
    // time-sliced multi-GPU evaluation: this rank's RCCL communicator (cmax_comm_init), or null
    cmax::Comm *comm = nullptr;
    // C2 in row bands behind K3 (cmax_comm_set_c2_bands): the owned-group K3 of a dense objective is launched band by band (whole
    // tile rows) and every band's rows of the gradient are all-reduced on a second stream while the next band's K3 runs
    int c2_bands = 1;
    std::vector<int> row_seg_start;  // [ntr + 1] first segment of every source tile row (owned work lists only)
    hipStream_t comm_stream = nullptr;
    std::vector<hipEvent_t> band_ev;  // [bands + 1]
    // deterministic mode (cmax_set_deterministic): every accumulation that depends on the order of events, workgroups or
    // atomics is done in integers (exact, associative) -- bit-identical IWE, loss and gradient from run to run
    bool deterministic = false;
    cmax::DevBuf<long long> img64;   // [5][npix] fixed-point vote images, all zero between evaluations
    cmax::DevBuf<unsigned> d_imax;   // [kStatSlots] bits of max |image| per statistics slot
    cmax::DevBuf<long long> g64;     // fixed-point gradient accumulators (zero between evaluations)
    cmax::DevBuf<double> d_det_inv_scale;  // [4]
    cmax::DevBuf<float> Gt_det;      // [4][npix] dL/d(blurred image) of the unfused image path
    // an fp64 flow / voxel at the boundary (cmax_objective_t::motion_dtype == CMAX_F64, dense / voxel): hi plane | lo plane of the
    // caller's doubles (k_split_motion), allocated on first use
    cmax::DevBuf<float> m64;
    const void *m64_src = nullptr;  // whose split the planes hold (cmax_objective_finish: the windows of a vote are another motion's otherwise)
};

namespace cmax {

// kernel classes for cmax_set_profiling / cmax_read_profile
enum { kProfVote = 0, kProfStats = 1, kProfGimage = 2, kProfGrad = 3, kProfFinish = 4, kProfComm = 5 };
static_assert(kProfComm + 1 == CMAX_PROF_CLASSES, "profile classes");
constexpr size_t kProfMaxPairs = 16384;

// RAII: records a HIP event on the launch stream before and after the enclosed launch
struct ProfScope {
    cmax_handle_s *h;
    int cls;
    hipStream_t s;
    hipEvent_t stop = nullptr;
    ProfScope(cmax_handle_s *h_, int cls_, hipStream_t s_) : h(h_), cls(cls_), s(s_) {
        if (!h->profiling || h->prof_ev[cls].size() >= 2 * kProfMaxPairs) return;
        hipEvent_t start = nullptr;
        if (hipEventCreate(&start) != hipSuccess || hipEventCreate(&stop) != hipSuccess) {
            stop = nullptr;
            return;
        }
        (void)hipEventRecord(start, s);
        h->prof_ev[cls].push_back(start);
        h->prof_ev[cls].push_back(stop);
    }
    ~ProfScope() {
        if (stop) (void)hipEventRecord(stop, s);
    }
};

// how K3 obtains dL/dIWE: from a materialised G image; folded G = c2 (IWE - mu) with the statistics K2 left in
// `stat`; or (2-DoF) deferred -- K3 gathers the raw image and the image statistics itself, the chain factors are
// applied by k_finish_deferred, and K2 is not launched at all
constexpr int kFoldNone = 0, kFoldStats = 1, kFoldDeferred = 2, kFoldScale = 3;  // kFoldScale: G image stored without its chain factor
// kFoldStatsInside: kFoldStats for a plain (not normalised) variance whose K2 runs INSIDE the K3 launch -- the first
// RefArgs::stat_blocks workgroups of the grid are k_stats (they also write the loss), the others gather; nothing in the
// gradient waits for the statistics: the chain factor is a constant and the mean comes from K1's vote sums (RefArgs::musum)
constexpr int kFoldStatsInside = 4;
constexpr int kGradRuns = 0, kGradStrided = 1, kGradOwned = 2, kGradDet = 3, kGradOwnedSmall = 4;  // k_grad's VARIANT (see cmax_event_kernels.inc)
constexpr int kStatBlocksMax = 512;
constexpr int kStatSlots = 5;  // reference times 0..3, slot 4 = un-warped image
constexpr int kStatSub = 32;   // sub-accumulators per slot
// Every sub-accumulator sits on its OWN 128-byte line: atomics to one cache line serialise in the L2 atomic unit whatever
// their address inside it (~7 ns each).  Packed 16 bytes apart, the up to 32 sub-accumulators of a slot shared 1-4 lines, and
// the 363 workgroups of a 260 x 346 image kernel spent 5 of their 9.8 us queueing on ONE line (profiles/r02_ablation.txt).
constexpr int kSubStride = 16;  // doubles between sub-accumulators
constexpr int kStatStride = kStatSub * kSubStride;
// raw sums of the deferred 2-DoF K3 (S1x, S1y, S2x, S2y, sum I, sum I^2): kRawLines accumulators per reference time, one line each
constexpr int kRawLines = CMAX_RAW_LINES, kRawStride = CMAX_RAW_DOUBLES;
static_assert(kRawLines == kStatSub && kRawStride == kStatStride && (kRawLines & (kRawLines - 1)) == 0, "K1 resets either with the same pattern");

struct ObjParams {
    int cost, normalized, minimize, negate, omit, n_ref;
    double mult[4];
    int H, W;  // padded image
    int nsub;  // sub-accumulators in use (<= kStatSub), grows with the number of k_stats workgroups
};

// arrival counters of the statistics workgroups inside K3 (arrive_last, cmax_event_launch.hip): kTicketSubs lines + one
constexpr int kTicketSubs = 16, kTicketLines = kTicketSubs + 1, kTicketLineInts = 32;
// K1's vote sums for the blurred variance (RefArgs::musum, k_blur_stats_adj_var)
constexpr int kMuLines = 32;                      // accumulators of K1's sum (same-line atomics serialise: one line each)
constexpr int kMuStride = kMuLines * kSubStride;   // doubles per reference time

// =============================================================================================
// Exact Hessian-vector product (a18): what torch.autograd.functional.vhp returns for the
// objective (src/solver/scipy_autograd/torch_wrapper.py:51-73) -- the derivative of the analytic
// gradient along a tangent motion u with the pixel cells held fixed (floor has zero derivative):
//   H u = sum_k [ phi_k'' dv_k J^T G0_k + phi_k' ( (dJ^T/dtheta u) G0_k + J^T (dG0_k/dI) J u ) ]
//   T1 k_vote_tan   tangent image dI = J u        (votes with the derivatives of the 4 bilinear weights)
//   T2 k_stats_tan  <G0, dI> and mean(dI)  ;  k_gimage_tan  G' = phi' dG0 + phi'' dv G0
//   T3 k_grad_hvp   per event: mixed term M (da, db) with the current G + gather of G' -> J^T
// The tangent is scaled to unit max-norm by the caller so the derivative votes fit fixed point.
// =============================================================================================
struct TanParams {
    const float *u;      // tangent motion, same layout as the motion, scaled to |u|_inf = 1
    float fix, inv_fix;  // fixed-point scale of the derivative votes (set per workgroup from the arrays below)
    // one launch covers the reference times of the objective (blockIdx.y):
    float d[4], fixk[4];  // reference time as a fraction of the batch period, its fixed-point scale
    float d_lo[4];        // ... what fp32 lost of d (read by warp_exact only: these kernels decide the cells K1 decides, from d + d_lo)
    int64_t bs;           // element stride between the per-reference-time images
};

// deterministic mode of the second-order gather (k_grad_hvp): all null / zero in the default mode
struct HvpDet {
    long long *g64;        // 2-DoF: per-segment partial sums [n_ref][nseg][2]; flow models: fixed-point accumulators of the product
    const unsigned *imax;  // bits of max |G_k| at [k], of max |G'_k| at [4 + k]
    double *inv_scale;     // [4] 1 / scale of reference time k (2-DoF) or of the whole launch ([0])
    long long n_events;
    int n_ref;
};

// argument of k_fixed_to_image (deterministic mode)
struct FixedArgs {
    long long *src[5];
    float *dst[5];
    double inv_fix;  // 1 / the vote fixed point of the kernels that filled src: 2^-20, big segments 2^-19
    double inv_fixk[5];  // != 0: per-image scale instead (tangent votes: one fixed point per reference time)
};

template <int V>
using int_c = std::integral_constant<int, V>;  // (fold / variant of k_grad)

constexpr int64_t kWeightPad = 4096 + 16;  // an event kernel's unconditional loads reach at most one segment's slots behind the last event

#define CMAX_REFUSE_WEIGHTED(h, what)                                                                                                 \
    do {                                                                                                                              \
        if ((h) && (h)->weighted) {                                                                                                   \
            ::cmax::set_error("%s: not built for a handle that holds per-event weights (cmax_set_event_weights); pass weights = NULL to clear them", what); \
            return CMAX_EUNSUPPORTED;                                                                                                 \
        }                                                                                                                             \
    } while (0)

// ---- what crosses a translation unit (hidden like the solver's hooks in cmax_common.h: the export list is the C ABI alone) ------
#define CMAX_HIDDEN __attribute__((visibility("hidden")))

// The segment layouts of the event kernels (the types t256 ... b1024 of cmax_event_kernels.inc carry these ids)
enum class Layout { t256, t512, t1024, m512, b512, b1024 };

// cmax_event_launch.hip: the launch layer of the event kernels, one launcher per kernel family, instantiated there for MODEL = -1
// (launch_vote and the two gathers only: the un-warped image), CMAX_MODEL_2DOF, CMAX_MODEL_DENSE and CMAX_MODEL_VOXEL
template <int MODEL>
CMAX_HIDDEN void launch_vote(cmax_handle_s *h, const EvView &ev, const WarpParams &wp, const RefArgs &ra_in, int n_ref, hipStream_t s, int nz = 1);
template <int MODEL>
CMAX_HIDDEN void launch_grad(cmax_handle_s *h, const EvView &ev, const WarpParams &wp, const RefArgs &ra_in, int n_ref, int fold, const ObjParams &op,
                             double *gpart, float *gflow, double *result, bool owned, hipStream_t s, int seg0 = 0, int seg_n = -1, int nz = 1);
template <int MODEL>
CMAX_HIDDEN void launch_weight_gather(cmax_handle_s *h, const EvView &ev, const WarpParams &wp, const RefArgs &ra, int n_img, int plane0, hipStream_t s);
template <int MODEL>
CMAX_HIDDEN void launch_event_gather(cmax_handle_s *h, const EvView &ev, const WarpParams &wp, const RefArgs &ra_in, int n_img, int plane0, hipStream_t s);
template <int MODEL>
CMAX_HIDDEN void launch_vote_tan(cmax_handle_s *h, const EvView &ev, const WarpParams &wp, const TanParams &tp, int n_ref, float *draw, hipStream_t s,
                                 long long *draw64 = nullptr);
template <int MODEL>
CMAX_HIDDEN void launch_grad_hvp(cmax_handle_s *h, const EvView &ev, const WarpParams &wp, const TanParams &tp, int n_ref, const float *G, const float *Gp,
                                 double *gpart, float *hflow, hipStream_t s, const HvpDet &det);
CMAX_HIDDEN void launch_vote_tan2(cmax_handle_s *h, const EvView &ev, const WarpParams &wp, const RefArgs &ra, int n_ref, hipStream_t s);
CMAX_HIDDEN Layout grad_layout(const cmax_handle_s *h, int model, bool owned);
CMAX_HIDDEN int layout_threads(Layout id);
// ... and k_pack_compact behind build_segments (cmax_batch.hip): the compact copy of the current work list's events, grown on demand
CMAX_HIDDEN int pack_compact_events(cmax_handle_s *h, hipStream_t s);
CMAX_HIDDEN int64_t compact_region_bytes();  // bytes per region of that copy (the big layout's kCompactStride)
#ifdef CMAX_TIMELINE
// cmax_fused.hip: where its image kernels stamp (cmax_debug_timeline; every unit holds its own copy of the pointer)
CMAX_HIDDEN int image_timeline_set(unsigned long long *buffer);
#endif

}  // namespace cmax
