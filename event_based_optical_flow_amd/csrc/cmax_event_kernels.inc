// Event kernels of the fused objective, templates over the segment layout L (EventLayout below: workgroup size, event slots,
// LDS window).  A segment of up to 2040 events is processed by 256 threads x 8 events (t256), 512 x 4 (t512) or 1024 x 2 (t1024);
// the mid (m512) and big (b512, b1024) layouts hold longer segments.  Which layout a launch takes is decided on the host, once per
// kernel family (vote_layout, grad_layout, plain_layout in cmax_event_launch.hip, which includes this file).  Shared helpers live
// there and in cmax_fused_device.h.

template <int THREADS, int SLOTS, int WINCAP, int ACC_TILES, int ACC_SMALL_GROUPS>
struct EventLayout {
    static constexpr int kThr = THREADS;  // threads per workgroup of the event kernels
    static constexpr int kNW = kThr / 64;  // waves per workgroup
    // SLOTS: event slots per workgroup = the segment size of the host's work list + 8.  2048 (t256 / t512 / t1024), or 4096 for BIG
    // segments (b512 / b1024, round 3: batches of >= 8M events): twice the events behind one LDS window, one box reduction, one window
    // staging / flush and one segmented scan -- the per-thread fixed costs of K1 / K3 (~85 of ~300 VALU instructions per thread at four
    // events per thread) are spread over eight events.  4080 votes of 2^20 would overflow 31 bits: big segments vote in 13.19.
    static constexpr int kSlots = SLOTS;
    static constexpr int kEPT = kSlots / kThr;  // events per thread (cached in registers between the two phases)
    static constexpr int kSegMaxNS = kSlots - 8;  // events per segment
    static constexpr bool kBig = kSlots > 2048;
    static constexpr float kFixNS = kBig ? 524288.f : 1048576.f, kInvFixNS = 1.f / kFixNS;  // vote fixed point: 2^19 | 2^20
    static constexpr int kAccExp = kBig ? 18 : 19;  // block-scaled flow-gradient accumulators: 2^(kAccExp - e), <= kSegMaxNS terms per cell
    static_assert(kEPT >= 2 && (kEPT % 2) == 0, "two events per 16-byte load");
    static_assert(kSlots == 2048 || kSlots == 3072 || kSlots == 4096, "segment sizes the host cuts");
    // The MID layout (m512, round 4): 512 threads x 6 events = 3064 events per segment, FOUR source tiles (or five (tile, bin) groups)
    // wide, with a 6144-word window so that window + accumulators keep four workgroups per CU.  For batches whose standard cut needs more
    // workgroups than the chip holds at once (256 CUs x 4) while this one does not: the second round of a launch pays every workgroup's
    // ~2.5 us of start-up loads again (tools/timeline.py) -- cfg5's shard: 1693 workgroups in two rounds -> 900 in one.
    static constexpr int kWinCap = WINCAP;  // LDS window capacity in words
    static constexpr int kDummy = kWinCap;  // masked path: 64 per-lane scratch words behind the window
    static constexpr int kAccDense = 256 * ACC_TILES;  // flow-gradient accumulator cells per channel: owned dense segments span this many source tiles
    static constexpr int kAccSmall = 256 * ACC_SMALL_GROUPS;  // ... owned voxel segments of few, well-filled (tile, bin) groups (kGradOwnedSmall)
    static_assert((double)kSegMaxNS * kFixNS < 2147483648.0, "fixed-point vote accumulation would overflow");
    static constexpr int kBlkShift = kBig ? 6 : 5;  // Window::bmask: one bit per kSlots / 64 consecutive slots (see phase_warp)
    // The head of K1 / K3 that loads everything at entry, beside the segment descriptor, and whose dead waves load unconditionally
    // (k_vote, issue_event_loads): the standard segments.  Mid and big segments keep the head they had -- with the new one six dense
    // b512 and one m512 instantiation of k_grad went from 64 to 66 VGPRs, i.e. lost a wave per SIMD, a weighted b512::k_vote began to
    // spill, and the multi-round launches of big segments, which are bound by issue slots and not by the latency of their first loads,
    // lost 9 - 16 % (cfg3 31.8 -> 37.0 us, 64M events 247 -> 277): profiles/head_loads_resources.txt, profiles/head_loads_ab.txt.
    static constexpr bool kEntryHead = kSlots == 2048;
    static constexpr int kShiftWords = kSlots / 8;  // 32-bit words of cell offsets per (reference time, segment): 8 slots per word
    // compact events (see EventLoads), bytes
    static constexpr int kCompactPix = 4 * kSlots, kCompactHdr = 4 * kSlots + kSlots / 2, kCompactStride = kCompactHdr + 64;
    // K1's second launch bound (see k_vote)
    static constexpr int kVoteWaves = (kBig && kThr == 512) ? 8 : 1;
    // k_vote_tan2: window pixels per plane (3 planes + scratch = the window + 200 words of k_vote), and the tangent planes' fixed
    // point, 2^18 (big segments: 2^17)
    static constexpr int kTanCap = kWinCap == 8192 ? 2720 : kWinCap / 3 - 8;
    static constexpr float kTanFix = kBig ? 131072.f : 262144.f, kTanInvFix = 1.f / kTanFix;
};
// The layouts: distinct types, so that a kernel's name says which one it was compiled for (cmax::k_grad<cmax::t512, ...>); their
// ids (enum class Layout) are declared in cmax_fused_internal.h.
struct t256 : EventLayout<256, 2048, 8192, 3, 3> { static constexpr Layout kId = Layout::t256; };
struct t512 : EventLayout<512, 2048, 8192, 3, 3> { static constexpr Layout kId = Layout::t512; };
struct t1024 : EventLayout<1024, 2048, 8192, 3, 3> { static constexpr Layout kId = Layout::t1024; };
struct m512 : EventLayout<512, 3072, 6144, 4, 5> { static constexpr Layout kId = Layout::m512; };  // mid segments (3064 events, cmax_handle_s::mid)
struct b512 : EventLayout<512, 4096, 8192, 6, 3> { static constexpr Layout kId = Layout::b512; };  // big segments (4088 events, cmax_handle_s::big)
struct b1024 : EventLayout<1024, 4096, 8192, 6, 3> { static constexpr Layout kId = Layout::b1024; };

// Phase A of both event kernels: warp this thread's <= kEPT events (kept in registers), reduce the
// bounding box of their top-left vote corners over the workgroup and derive the LDS window.
// rc[u] packs (row + 16384) << 16 | (col + 16384); 0 marks an empty slot.
//
// The per-event work is VALU-issue bound (4 SIMDs x 16 lanes per CU; ~1M events x instructions / 16384
// lanes per clock), so the code below is written for instruction count: branch-free slots, 32-bit local
// indices, the box kept as two packed-u16 words (v_pk_min_u16 / v_pk_max_u16) and reduced with DPP row
// shifts + row broadcasts instead of ds_bpermute shuffles.
//
// `init(win)` fills the LDS window (zeroes it / stages dL/dIWE) as soon as the window is known.  K3 re-warps the
// events K1 warped with the same motion, so K1 publishes its windows (one int4 per reference time and segment) and
// K3 (KNOWN) reads them back: the window loads are then issued right behind the event loads -- their latencies
// overlap -- and the box reduction and its barrier disappear.
//
// EXACT CELLS (warp_exact).  K1 (KNOWN = false) finds the events that lie within fp32 rounding of a cell border, decides their
// cells in fp64 and publishes what K3 needs to follow it WITHOUT any fp64 arithmetic of its own: the 64-bit Window::bmask (which
// 1/64ths of the segment's slots hold an event whose cell moved) and, in the segment's `shifts` words, a nibble per slot = the cell's
// offset from the fp32 one (row | col << 2, two-bit two's complement).  `nibbles` returns this thread's own (slot u in bits [4u, 4u + 4)).
//
// The event loads of a workgroup, issued as soon as its segment has arrived: they need nothing but the segment and the event pointer,
// which a workgroup holds without having seen the kernel's argument block (kernel parameters, k_vote).  Whatever else the warp needs
// from memory -- theta, the time extremes, the argument block's words -- is loaded BESIDE the segment and has arrived with it (see
// k_vote: the compiler does not overlap these with the events of its own accord).
// Default layout: each thread holds kEPT CONSECUTIVE sorted events (slot u = local index kEPT * thread + u,
// counted from the segment start rounded down to an even index: the buffer is 16-byte aligned and padded),
// read with 16-byte loads.  Neighbouring lanes then hold events kEPT apart -- mostly different source
// pixels, so their votes rarely hit the same LDS word (K1 of cfg3 22.7 -> 18.7 us) -- and the dense gradient
// can reduce runs of equal source pixel serially in registers (k_grad).
// STRIDED: slot u = 2 j + e holds local index 2 * (kThr j + thread) + e, i.e. for a fixed slot consecutive
// lanes hold consecutive event pairs -- what the per-slot segmented scan of the dense K3 wants when runs are short.
// COMPACT EVENTS (round 5; big segments of un-binned handles, consecutive slot layout): a second copy of the sorted events laid out
// PER SEGMENT OF THE WORK LIST (k_pack_compact, once per batch behind the host's cut), 4.5 bytes per event instead of 8:
//   region of segment s = cev + s * kCompactStride:  u32 ev[kSlots] | u32 tiles[kSlots / 8] | header (64 bytes)
//   slot l of the region = local index l of the segment (the same l the 8-byte path computes: first + l = sorted event index),
//   empty slots zero;
//   ev    = tau24 << 8 | (row & 15) << 4 | (col & 15):  tau24 = the normalised time rounded ONCE (from fp32 + residual byte) to 24-bit
//           fixed point -- decoded as (float)tau24 * 2^-24, an exact fp32 value within 2^-25 of the time: the absolute error fp32 has
//           in [0.5, 1), which is what exact_margin budgets for (the one event at tau = 1 is stored as 1 - 2^-24);
//   tiles = a nibble per slot: the event's source tile column minus the segment's first (a segment lies in ONE tile row and spans
//           <= 6 source tiles);  header word 0 = 16 * tile row | (16 * first tile column) << 12.
// The hot kernels then read 4.5 B/event (the event stream IS the traffic of the large launches: 64M events 512 of 549 MB counted per
// K1), every thread's loads are 32- / 16-byte aligned whatever the segment's first event, and their addresses depend on the
// workgroup's index alone -- they are issued before the segment descriptor has arrived (one dependent round trip less at the head
// of K1 and K3).  The 8-byte array stays: the time residual byte (exact cells), re-binning, the tangent / search kernels read it.
template <class L>
struct EventLoads {
    uint4 raw[L::kEPT / 2];  // 8-byte format: kEPT / 2 event pairs; compact: tau in raw[0 .. kEPT / 4), pix behind it
    bool wave_live;  // this wave holds events (wave-uniform)
    bool compact;    // launch-uniform
    unsigned basexy; // compact: the region's header word
};
template <class L, bool STRIDED>
__device__ __forceinline__ void issue_event_loads(const uint2 *__restrict__ evp, const char *__restrict__ cev, int sidx, int4 sg, EventLoads<L> &el) {
    auto local_index = [](int u) { return STRIDED ? 2 * ((u >> 1) * L::kThr + (int)threadIdx.x) + (u & 1) : L::kEPT * (int)threadIdx.x + u; };
    const int odd = sg.x & 1, cnt = sg.y;
    el.compact = false;
    el.basexy = 0u;
    if constexpr (L::kBig && !STRIDED && (L::kEPT % 4) == 0) {
        if (cev != nullptr) {  // launch-uniform (a kernel parameter: known before the first load)
            const char *reg = cev + (int64_t)sidx * L::kCompactStride;
            const char *tp = reg + 4 * L::kEPT * (int)threadIdx.x;
#pragma unroll
            for (int j = 0; j < L::kEPT / 2; ++j) el.raw[j] = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
            for (int j = 0; j < L::kEPT / 4; ++j) el.raw[j] = *reinterpret_cast<const uint4 *>(tp + 16 * j);
            el.raw[L::kEPT / 4].x = *reinterpret_cast<const unsigned *>(reg + L::kCompactPix + 4 * ((L::kEPT * (int)threadIdx.x) >> 3));  // 8 nibbles per word
            el.basexy = *reinterpret_cast<const unsigned *>(reg + L::kCompactHdr);
            el.compact = true;
            el.wave_live = __builtin_amdgcn_readfirstlane(local_index(0)) < cnt + odd;
            return;
        }
    }
    const uint2 *seg_ev = evp + ((int64_t)sg.x - odd);
    // A wave whose first slot lies behind the segment's last event holds no event at all (segments are cut at tile
    // boundaries, so they rarely fill the 2048 slots: cfg2's 1423-event half tiles leave the fourth wave of every
    // workgroup empty).  Such a wave skips the loads, the warp arithmetic and -- through `wave_live` -- the vote /
    // gather phases of the callers; it still takes part in the barriers, the window initialisation and the flush.
    el.wave_live = __builtin_amdgcn_readfirstlane(local_index(0)) < cnt + odd;
    // All event loads are issued back to back, UNCONDITIONALLY, by dead waves too: a pair that lies behind the segment's last event
    // re-reads the segment's last pair (its slots are invalid and masked by `valid` / rc == 0 below; the flow they index is
    // in bounds; an empty segment reads the pair at its start, which the buffer's padding holds).  (With `if (l0 < cnt) raw[j] = load`
    // the compiler put every load into its own exec-masked block and waited for it there -- s_waitcnt vmcnt(0) behind each
    // global_load_dwordx4: two (512 threads) or four (256) dependent round trips to memory at the head of K1 and K3.  With the
    // loads inside `if (wave_live)` behind a zero initialisation the same happened once more behind a scalar branch: the merge of
    // the loaded registers with the zeros is a copy IN that block, and K1 waited for its events there, in front of every other
    // load of its head -- profiles/head_loads_isa.txt.  A dead wave never looks at what it loaded.)
    if constexpr (L::kEntryHead) {
        const int l_last = max((cnt + odd - 1) & ~1, 0);  // local index of the segment's last pair
#pragma unroll
        for (int j = 0; j < L::kEPT / 2; ++j) el.raw[j] = *reinterpret_cast<const uint4 *>(seg_ev + min(local_index(2 * j), l_last));
    } else {  // (mid and big segments: live waves only, see EventLayout::kEntryHead)
        const int l_last = (cnt + odd - 1) & ~1;
#pragma unroll
        for (int j = 0; j < L::kEPT / 2; ++j) el.raw[j] = make_uint4(0u, 0u, 0u, 0u);
        if (el.wave_live) {  // wave-uniform
#pragma unroll
            for (int j = 0; j < L::kEPT / 2; ++j) el.raw[j] = *reinterpret_cast<const uint4 *>(seg_ev + min(local_index(2 * j), l_last));
        }
    }
}
// word k (0 .. 3) of a 16-byte register quadruple, k a compile-time constant after unrolling
__device__ __forceinline__ unsigned quad_word(const uint4 &q, int k) { return k == 0 ? q.x : (k == 1 ? q.y : (k == 2 ? q.z : q.w)); }
// slot u of a thread's events, decoded for the warp (EvDec), whichever way they were loaded.  negd = minus the reference time, in a VGPR (tau - d is
// rounded once either way: the compact time is an exact fp32 multiple of 2^-24, so the fma rounds what the subtraction would).
template <class L>
__device__ __forceinline__ EvDec decode_slot(const EventLoads<L> &el, int u, float negd, bool voxel) {
    EvDec e;
    if (L::kBig && el.compact) {
        const unsigned a = quad_word(el.raw[u >> 2], u & 3);
        const unsigned tcol = __builtin_amdgcn_ubfe(el.raw[L::kEPT / 4].x, 4 * (((L::kEPT * (int)threadIdx.x) & 7) + u), 3);
        e.ixr = __builtin_amdgcn_ubfe(a, 4, 4);
        e.iyr = (tcol << 4) | (a & 15u);
        e.top = 0u;
        e.key = el.basexy + e.ixr + (e.iyr << 12);
        e.tmd = fmaf((float)(a >> 8), 0x1p-24f, negd);
        return e;
    }
    const int j = u >> 1;
    const uint2 p = (u & 1) ? make_uint2(el.raw[j].z, el.raw[j].w) : make_uint2(el.raw[j].x, el.raw[j].y);
    e.ixr = p.x & 0xFFFu;
    e.iyr = (p.x >> 12) & 0xFFFu;
    e.top = p.x >> 24;
    e.key = voxel ? p.x : (p.x & 0x00FFFFFFu);
    e.tmd = __uint_as_float(p.y) + negd;
    return e;
}

// WEIGHTED instantiations of K1 / K3 (cmax_set_event_weights): the weights of a thread's slots.  The array is in packed order -- slot l of a
// segment is sorted event first + l, for the plain and the compact event loads alike -- and padded with zeros behind the last event, so
// the loads are unconditional; an empty slot's value is never used (rc == 0 / dt == 0 mask it).
template <class L, bool STRIDED>
__device__ __forceinline__ void load_slot_weights(const float *__restrict__ wgt, int4 sg, float (&fw)[L::kEPT]) {
    const float *base = wgt + ((int64_t)sg.x - (sg.x & 1));
#pragma unroll
    for (int u = 0; u < L::kEPT; ++u) fw[u] = base[STRIDED ? 2 * ((u >> 1) * L::kThr + (int)threadIdx.x) + (u & 1) : L::kEPT * (int)threadIdx.x + u];
}

// One workgroup per segment: writes the segment's compact region (see EventLoads).
template <class L>
__global__ void __launch_bounds__(L::kThr) k_pack_compact(const int4 *__restrict__ segs, int nseg, const uint2 *__restrict__ evp, int ntc, char *__restrict__ cev, int *__restrict__ bad) {
    const int sidx = blockIdx.x;
    if (sidx >= nseg) return;
    const int4 sg = segs[sidx];
    const int odd = sg.x & 1, cnt = sg.y;
    const int trow = sg.z / ntc, tcol = sg.z - trow * ntc;
    const unsigned base_r = 16u * (unsigned)trow, base_c = 16u * (unsigned)tcol;
    const uint2 *seg_ev = evp + ((int64_t)sg.x - odd);
    char *reg = cev + (int64_t)sidx * L::kCompactStride;
    unsigned *out = reinterpret_cast<unsigned *>(reg), *tiles = reinterpret_cast<unsigned *>(reg + L::kCompactPix);
    if (threadIdx.x < 16) reinterpret_cast<unsigned *>(reg + L::kCompactHdr)[threadIdx.x] = threadIdx.x == 0 ? (base_r | (base_c << 12)) : 0u;
    bool wrong = false;
    for (int w = threadIdx.x; w < L::kSlots / 8; w += L::kThr) {  // eight slots = one word of tile nibbles per iteration
        unsigned nib = 0u, v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int l = 8 * w + q;
            v[q] = 0u;
            if ((unsigned)(l - odd) < (unsigned)cnt) {
                const uint2 e = seg_ev[l];
                const unsigned r = (e.x & 0xFFFu) - base_r, c = ((e.x >> 12) & 0xFFFu) - base_c;
                wrong = wrong || r >= 16u || c >= 128u;
                double t24 = rint(tau_refined(e) * 16777216.0);
                t24 = fmin(fmax(t24, 0.0), 16777215.0);
                v[q] = ((unsigned)t24 << 8) | ((r & 15u) << 4) | (c & 15u);
                nib |= ((c >> 4) & 7u) << (4 * q);
            }
        }
        reinterpret_cast<uint4 *>(out)[2 * w] = make_uint4(v[0], v[1], v[2], v[3]);
        reinterpret_cast<uint4 *>(out)[2 * w + 1] = make_uint4(v[4], v[5], v[6], v[7]);
        tiles[w] = nib;
    }
    if (wrong) atomicOr(bad, 1);  // (never: a segment lies in one tile row and spans <= 6 tiles; checked by the host in debug runs)
}

// F64FLOW (dense / voxel): the motion is the caller's fp64 flow, split -- wp.motion is its high plane, the low plane lies behind the field
// (k_split_motion); read by the border branch only.  A template argument, not a branch on wp.motion_f64: the kernels of an fp32 call
// are the ones they were (profiles/flow64_resources.txt).
//
// HEAD: what a kernel fetched at its entry, beside its segment descriptor (WarpHead: K1 and K3), or NoHead -- the kernels that read the
// batch period and theta here, through the argument block's pointers.
struct NoHead {};
struct WarpHead {
    double period;      // the batch period (1 when the times are normalised)
    double thd0, thd1;  // 2-DoF: theta as the caller holds it
};
// The head's loads through the LEADING kernel parameters (the first 14 argument dwords arrive in SGPRs: build.py), all of them
// uniform, unconditional and independent of the argument block, so that they leave with the segment descriptor's load and come back
// under its wait: the batch's time extremes and -- 2-DoF -- theta in either dtype (an fp32 theta is read twice rather than behind a
// branch: a load in a block of its own is waited for in that block).  The words are kept RAW until the caller has pinned them together
// with its segment (CMAX_HEAD_PIN): the conversions to fp64 are VALU work, and the compiler branches around them on the flags -- taken
// in front of the pin, those branches cut the loads into groups with a wait each (profiles/head_loads_isa.txt).
// flags: kHeadNormalize | kHeadMotionF64 (WarpParams::normalize / motion_f64).
constexpr int kHeadNormalize = 1, kHeadMotionF64 = 2;
struct HeadWords {
    int4 t;      // (tmin, tmax) as 32-bit words
    int2 lo, hi; // theta: fp32 (lo.x, lo.y); fp64 lo, hi
};
template <int MODEL>
__device__ __forceinline__ HeadWords load_head_words(const float *__restrict__ motion, const double *__restrict__ tmm, int flags) {
    HeadWords w;
    w.t = *reinterpret_cast<const int4 *>(tmm);  // (the handle's own d_tmm: the base of a device allocation, see warp_params)
    w.lo = make_int2(0, 0);
    w.hi = make_int2(0, 0);
    if (MODEL == CMAX_MODEL_2DOF) {
        // (dword by dword: an fp32 theta of the caller's -- a slice of a tensor -- is only 4-byte aligned)
        const int *mw = reinterpret_cast<const int *>(motion);
        const int o = (flags & kHeadMotionF64) ? 2 : 0;
        w.lo = make_int2(mw[0], mw[1]);
        w.hi = make_int2(mw[o], mw[o + 1]);
    }
    return w;
}
#define CMAX_HEAD_PIN_WORDS(HEADW) "s"((HEADW).t.x), "s"((HEADW).t.y), "s"((HEADW).t.z), "s"((HEADW).t.w), "s"((HEADW).lo.x), "s"((HEADW).lo.y), "s"((HEADW).hi.x), "s"((HEADW).hi.y)
__device__ __forceinline__ WarpHead decode_head_words(const HeadWords &w, int flags) {
    WarpHead hd;
    hd.period = (flags & kHeadNormalize) ? 1.0 : __hiloint2double(w.t.w, w.t.z) - __hiloint2double(w.t.y, w.t.x);
    if (flags & kHeadMotionF64) {
        hd.thd0 = __hiloint2double(w.lo.y, w.lo.x);
        hd.thd1 = __hiloint2double(w.hi.y, w.hi.x);
    } else {
        hd.thd0 = (double)__int_as_float(w.lo.x);
        hd.thd1 = (double)__int_as_float(w.lo.y);
    }
    return hd;
}
template <class L, int MODEL, bool FRAC, bool WANT_DT, bool STRIDED = false, bool KNOWN = false, bool F64FLOW = false, typename Init, class HEAD>
__device__ __forceinline__ Window phase_warp(const EvView &ev, const WarpParams &wp, int4 sg, EventLoads<L> &el, unsigned (&rc)[L::kEPT],
                                              float (&fa)[L::kEPT], float (&fb)[L::kEPT], float (&fdt)[L::kEPT], int (&fsrc)[L::kEPT],
                                              uint4 *s_box, const int4 *known, const unsigned *__restrict__ shifts, Init init, bool &wave_live,
                                              unsigned &nibbles, const HEAD &head) {
    constexpr bool kHead = std::is_same_v<HEAD, WarpHead>;
    constexpr bool kExact = MODEL >= 0;  // cells of events on a cell border are decided in fp64 (warp_exact); the un-warped image has no motion
    constexpr bool kFlow = MODEL == CMAX_MODEL_DENSE || MODEL == CMAX_MODEL_VOXEL;
    static_assert(!(KNOWN && !WANT_DT), "K3 re-uses K1's windows");
    static_assert(!F64FLOW || (kFlow && !KNOWN), "the low plane of an fp64 flow is read where a cell is decided");
    auto local_index = [](int u) { return STRIDED ? 2 * ((u >> 1) * L::kThr + (int)threadIdx.x) + (u & 1) : L::kEPT * (int)threadIdx.x + u; };
    const int odd = sg.x & 1, cnt = sg.y;
    const int64_t first = (int64_t)sg.x - odd;
    const uint2 *seg_ev = ev.ev + first;
    wave_live = el.wave_live;
    EvBase eb;  // compact events are relative to their segment's tile strip (the region's header), plain ones absolute
    eb.row = el.basexy & 0xFFFu;
    eb.col = el.basexy >> 12;
    eb.src = mul24_u(eb.row, (unsigned)wp.W & 0xFFFFFFu) + eb.col;
    float negd = -wp.d;
    if (L::kBig) asm volatile("" : "+v"(negd));  // (one VGPR for the whole loop: as an SGPR it is copied in front of every event's fma, whose other operands are scalar too)
    const uint4 (&raw)[L::kEPT / 2] = el.raw;
    double period;
    if constexpr (kHead) period = head.period;
    else period = wp.normalize ? 1.0 : wp.tmm[1] - wp.tmm[0];
    const float tscale = (float)period;  // (time_scale)
    const float mcoef = exact_margin_coef(wp.d, tscale);
    float th0 = 0.f, th1 = 0.f, mt = 0.f;
    double thd0 = 0.0, thd1 = 0.0;  // theta as the caller holds it: decides the cells of events on a cell border (warp_exact)
    if (MODEL == CMAX_MODEL_2DOF) {
        if constexpr (kHead) {
            thd0 = head.thd0;
            thd1 = head.thd1;
        } else if (wp.motion_f64) {  // (as 32-bit words: scalar loads, like the fp32 branch)
            const int *mw = reinterpret_cast<const int *>(wp.motion);
            thd0 = __hiloint2double(mw[1], mw[0]);
            thd1 = __hiloint2double(mw[3], mw[2]);
        } else {
            thd0 = (double)wp.motion[0];
            thd1 = (double)wp.motion[1];
        }
        th0 = (float)thd0;
        th1 = (float)thd1;
        mt = exact_margin<FRAC>(mcoef, fmaxf(fabsf(th0), fabsf(th1)));  // one margin for every event
    }
    nibbles = 0u;
    Window win;
    if (KNOWN) {  // the window and the verdicts of the K1 launch of the same evaluation (workgroup-uniform)
        win = unpack_window(*known);
        init(win);
    }
    // box of the valid slots as two packed-u16 words reduced with MAX only (identity 0 = what a DPP lane without a
    // source reads): mxp = maxima of (row, col), mnq = maxima of the complemented fields, i.e. ~minima
    unsigned mnq = 0u, mxp = 0u;
    // Does one of this thread's events lie within fp32 rounding of a cell border?  K1 keeps the smallest and the largest fraction --
    // two VALU instructions per event (v_min3 / v_max3), a third for the largest flow component of the flow models (the rounding
    // of dt * f scales with it) -- and compares once per thread (1e-5 .. 1e-4 of the events are candidates).
    float amin = 0.5f, amax = 0.5f, fmt = 0.f;
    // FULL WAVES (round 6, VALU diet).  A segment's events are its first cnt slots (from `odd` on), so only the wave that holds the
    // segment's end -- and, for an odd start, the first -- has empty slots.  The loop below therefore warps EVERY slot (an index add,
    // a compare and two selects per event less: 4 of ~85 VALU instructions per event in K1 of the big segments) and the empty slots
    // are masked behind it, in those waves only.  What an empty slot holds is harmless to the box of the vote corners, which is
    // taken over all slots: a zero word of the compact copy (the strip's first pixel at tau = 0), a re-read of the segment's last
    // pair, or -- odd start -- a copy of the segment's first event (issue_event_loads); the window is a superset of the votes.
    // (Two copies of the loop -- with and without validity -- were tried first: the 512 x 8 kernels then need 80 VGPRs or spill to
    // scratch, and either costs far more than the selects: K3 of 20M events 46 -> 59 us, 64M 129 -> 189.)
    // (K3 keeps the selects inside its loop: freed of them, the scheduler of the 512 x 8 kernel keeps more loads in flight and takes 78
    // VGPRs instead of 64 -- six waves per SIMD --, and bounded to 64 it spills)
    constexpr bool kMaskInside = KNOWN;
    unsigned mnp = 0xFFFFFFFFu;  // minima of (row, col) as packed u16 (v_pk_min_u16); complemented into mnq behind the loop
    const int wl0 = __builtin_amdgcn_readfirstlane(local_index(0));
    const bool wave_full = !STRIDED && wl0 >= odd && wl0 + kWave * L::kEPT - odd <= cnt;  // (wave-uniform)
    if (!wave_live) {  // wave-uniform
#pragma unroll
        for (int u = 0; u < L::kEPT; ++u) {
            rc[u] = 0u;
            fa[u] = 0.f;
            fb[u] = 0.f;
            if (WANT_DT) {
                fdt[u] = 0.f;
                fsrc[u] = 0;
            }
        }
    } else {
        // The box of the vote corners is taken over ALL slots and empty ones are masked behind the loop: an empty slot must not hold a
        // FOREIGN event (of another tile row, possibly).  Two slots of the plain 8-byte loads can: the one in front of a segment that
        // starts at an odd index (the previous segment's last event) and the second slot of the pair that holds an odd end (the next
        // segment's first) -- they get a copy of their pair's other, valid event; whatever that adds to the box is a cell the segment
        // votes into anyway.  Here, where the loads are consumed (not behind their issue: that would put a wait in front of every load
        // that follows), and in the waves that hold such a slot only.
        if (!kMaskInside && !wave_full && !(L::kBig && el.compact)) {  // wave-uniform
            const int end = cnt + odd, l_last = (end - 1) & ~1;
#pragma unroll
            for (int j = 0; j < L::kEPT / 2; ++j) {
                if (min(local_index(2 * j), l_last) + 1 >= end) {
                    el.raw[j].z = el.raw[j].x;
                    el.raw[j].w = el.raw[j].y;
                }
            }
            if (odd && local_index(0) == 0) {
                el.raw[0].x = el.raw[0].z;
                el.raw[0].y = el.raw[0].w;
            }
        }
#pragma unroll
        for (int u = 0; u < L::kEPT; ++u) {
            const int l = local_index(u);
            // kMaskInside (K3) | fractional batches (guards the residual loads): the slot's validity, here; else every slot is warped
            const bool valid = (!kMaskInside && !FRAC) || (unsigned)(l - odd) < (unsigned)cnt;
            const EvDec e = decode_slot<L>(el, u, negd, MODEL == CMAX_MODEL_VOXEL);
            // empty slots run the same arithmetic on a zero event (finite values, in-bounds flow reads)
            const Warped w = warp_one<MODEL, FRAC>(ev, e, eb, first + l, valid, wp, tscale, th0, th1);
            if (kExact && !KNOWN) {
                amin = fminf(fminf(amin, w.a), w.b);
                amax = fmaxf(fmaxf(amax, w.a), w.b);
                if (kFlow) fmt = fmaxf(fmaxf(fmt, fabsf(w.f0)), fabsf(w.f1));
            }
            const unsigned packed = ((unsigned)(w.row + 16384) << 16) | (unsigned)(w.col + 16384);
            rc[u] = (kMaskInside && !valid) ? 0u : packed;
            fa[u] = w.a;
            fb[u] = w.b;
            if (WANT_DT) {
                fdt[u] = (kMaskInside && !valid) ? 0.f : w.dt;
                // run key of the flow-gradient reduction: packed (row, col[, bin]) -- unique per cell, decoded by shifts
                fsrc[u] = (int)e.key;
            }
            if (!KNOWN) {
                mnp = pk_min_u16(mnp, packed);
                mxp = pk_max_u16(mxp, packed);
            }
        }
        if (!kMaskInside && !wave_full) {  // wave-uniform: the one wave of a segment that holds its end (and wave 0 of an odd start)
#pragma unroll
            for (int u = 0; u < L::kEPT; ++u) {
                const bool valid = (unsigned)(local_index(u) - odd) < (unsigned)cnt;
                rc[u] = valid ? rc[u] : 0u;
                if (WANT_DT) fdt[u] = valid ? fdt[u] : 0.f;
            }
        }
    }
    if (KNOWN) {
        // K3: the few threads whose 1/64th of the segment holds an event K1 moved to another cell fetch the offsets and apply them.
        // The fractions follow: x' is the same number, a = x' - cell.  (No fp64, no second look at the flow: K1 decided.)
        if (kExact && win.border && wave_live) {  // workgroup-uniform && wave-uniform
            auto apply = [&](int u, unsigned nib) {
                const int sr = (int)(nib << 30) >> 30, sc = (int)(nib << 28) >> 30;
                rc[u] += (unsigned)((sr << 16) + sc);  // (no borrow between the fields: row + 16384 and col + 16384 stay positive)
                fa[u] -= (float)sr;
                fb[u] -= (float)sc;
            };
            if (STRIDED) {
#pragma unroll
                for (int j = 0; j < L::kEPT / 2; ++j) {
                    const int l = local_index(2 * j);
                    if (((win.bmask >> (l >> L::kBlkShift)) & 1ull) == 0ull) continue;
                    const unsigned nb = (shifts[l >> 3] >> ((l & 7) * 4)) & 0xFFu;
                    if (nb & 0xFu) apply(2 * j, nb & 0xFu);
                    if (nb >> 4) apply(2 * j + 1, nb >> 4);
                }
            } else {
                // a thread's kEPT consecutive slots lie in one word of eight nibbles, or (six events per thread) straddle two; likewise
                // they lie in one or two of the segment's 64ths
                const int l0 = local_index(0), l1 = l0 + L::kEPT - 1;
                // (a word is valid only where ITS OWN 64th is flagged: K1 clears the words of flagged blocks only, ADVICE r4)
                const bool blk0 = ((win.bmask >> (l0 >> L::kBlkShift)) & 1ull) != 0ull, blk1 = ((win.bmask >> (l1 >> L::kBlkShift)) & 1ull) != 0ull;
                if (blk0 || blk1) {
                    unsigned long long nb = blk0 ? shifts[l0 >> 3] : 0u;
                    if ((l1 >> 3) != (l0 >> 3) && blk1) nb |= (unsigned long long)shifts[l1 >> 3] << 32;
                    nb >>= (l0 & 7) * 4;
                    if (L::kEPT < 16 && (nb & ((1ull << (4 * L::kEPT)) - 1ull)) != 0ull) {
#pragma unroll
                        for (int u = 0; u < L::kEPT; ++u) {
                            const unsigned nib = (unsigned)(nb >> (4 * u)) & 0xFu;
                            if (nib) apply(u, nib);
                        }
                    }
                }
            }
        }
        return win;
    }
    if (!WANT_DT) CMAX_STAMP_AFTER(0, 1, rc[L::kEPT - 1]);  // (K1: events and flows have arrived, the warp arithmetic is done)
    bool thread_exact = false;  // this thread moved one of its events to another cell than the fp32 arithmetic found
    if (kExact) {
        const float mthr = kFlow ? exact_margin<FRAC>(mcoef, fmt) : mt;  // at least as wide as the margin of each of this thread's events
        const bool border = amin < mthr || amax > 1.f - 1e-6f - mthr;
        if (border) {  // rare (about one wave in a hundred): see warp_exact
            // Which slots?  From registers alone: every load below is a round trip to memory in front of the workgroup's next barrier.
            const float mhi = 1.f - 1e-6f - mthr;
            unsigned cand = 0u;
#pragma unroll
            for (int u = 0; u < L::kEPT; ++u)
                if (rc[u] != 0u && (fa[u] < mthr || fa[u] > mhi || fb[u] < mthr || fb[u] > mhi)) cand |= 1u << u;
            // ONE copy of the re-warp, a rolled loop over the candidate slots (typically one): unrolled per slot it was kEPT copies of
            // ~150 instructions between the warp loop and the box reduction, and K1 paid for their mere presence (20M events: 39 -> 44 us
            // with the branch never taken, profiles/r04_ablation.txt).  The slot's registers are picked and put back with selects.
#pragma nounroll
            while (cand != 0u) {
                const int u = __builtin_ctz(cand);
                cand &= cand - 1u;
                unsigned rcu = rc[0];
                float fau = fa[0], fbu = fb[0];
#pragma unroll
                for (int k = 1; k < L::kEPT; ++k) {
                    rcu = u == k ? rc[k] : rcu;
                    fau = u == k ? fa[k] : fau;
                    fbu = u == k ? fb[k] : fbu;
                }
                // the packed event again (eight events per thread: loaded again -- keeping them in registers for this rare path would cost
                // every thread 16 VGPRs and the kernel a wave per SIMD) and its time beyond fp32: the residual in the packed word's top byte,
                // or (binned handles: that byte is the voxel bin) the fp64 array, both loads in flight together
                const int l = STRIDED ? 2 * ((u >> 1) * L::kThr + (int)threadIdx.x) + (u & 1) : L::kEPT * (int)threadIdx.x + u;
                uint2 e;
                if (L::kEPT <= 4 && !(L::kBig && el.compact)) {  // four events per thread: the packed events stay in registers (8 VGPRs these kernels have to spare) --
                    // one round trip less in front of the barrier, and at one round of workgroups per launch the slowest workgroup IS the kernel
                    e = make_uint2(raw[0].x, raw[0].y);
#pragma unroll
                    for (int k = 1; k < L::kEPT; ++k) {
                        const uint2 ek = (k & 1) ? make_uint2(raw[k >> 1].z, raw[k >> 1].w) : make_uint2(raw[k >> 1].x, raw[k >> 1].y);
                        e.x = u == k ? ek.x : e.x;
                        e.y = u == k ? ek.y : e.y;
                    }
                } else {
                    e = seg_ev[l];
                }
                const unsigned ex = e.x;
                double tau;
                if (ev.tau64) tau = ev.tau64[first + l];  // launch-uniform
                else tau = tau_refined(e);
                double m0 = thd0, m1 = thd1;
                if (kFlow) {  // the flow at the source pixel again (cached), as the device holds it; the event's own margin
                    const int ix = (int)(ex & 0xFFFu), iy = (int)((ex >> 12) & 0xFFFu), hw = wp.H * wp.W;
                    const int64_t src = (int64_t)ix * wp.W + iy + (MODEL == CMAX_MODEL_VOXEL ? (int64_t)(ex >> 24) * 2 * hw : (int64_t)0);
                    const float f0 = wp.motion[src], f1 = wp.motion[src + hw];
                    const float me = exact_margin<FRAC>(mcoef, fmaxf(fabsf(f0), fabsf(f1))), ehi = 1.f - 1e-6f - me;
                    m0 = (double)f0;
                    m1 = (double)f1;
                    if (!(fau < me || fau > ehi || fbu < me || fbu > ehi)) continue;
                    if constexpr (F64FLOW) {  // the caller's fp64 flow: f0 / f1 are its high parts, the low plane lies behind the field (k_split_motion)
                        const int64_t lo = src + (int64_t)(MODEL == CMAX_MODEL_VOXEL ? wp.T : 1) * 2 * hw;
                        m0 += (double)wp.motion[lo];
                        m1 += (double)wp.motion[lo + hw];
                    }
                }
                const Warped w = warp_exact<MODEL, FRAC>(ev, ex, first + l, tau, period, wp, m0, m1);
                const unsigned packed = ((unsigned)(w.row + 16384) << 16) | (unsigned)(w.col + 16384);
                // the cell's offset from the one the fp32 arithmetic found (-1, 0, 1 per axis), for K3
                const int sr = (int)(packed >> 16) - (int)(rcu >> 16), sc = (int)(packed & 0xFFFFu) - (int)(rcu & 0xFFFFu);
                nibbles |= ((unsigned)(sr & 3) | ((unsigned)(sc & 3) << 2)) << (4 * u);
#pragma unroll
                for (int k = 0; k < L::kEPT; ++k) {
                    rc[k] = u == k ? packed : rc[k];
                    fa[k] = u == k ? w.a : fa[k];
                    fb[k] = u == k ? w.b : fb[k];
                }
                mnp = pk_min_u16(mnp, packed);  // the box may grow by the cell the event moved to (it never needs to shrink)
                mxp = pk_max_u16(mxp, packed);
            }
            thread_exact = nibbles != 0u;
        }
    }
    // wave reduction on the VALU: 4 row shifts, then lane 15 of each row to the next row, lane 31 to rows 2-3;
    // lane 63 ends up with the wave's box
    mnq = ~mnp;
#define CMAX_BOX_STEP(CTRL)                  \
    mnq = pk_max_u16(mnq, dpp_u0<CTRL>(mnq)); \
    mxp = pk_max_u16(mxp, dpp_u0<CTRL>(mxp));
    CMAX_BOX_STEP(kDppRowShr1)
    CMAX_BOX_STEP(kDppRowShr2)
    CMAX_BOX_STEP(kDppRowShr4)
    CMAX_BOX_STEP(kDppRowShr8)
    CMAX_BOX_STEP(kDppRowBcast15)
    CMAX_BOX_STEP(kDppRowBcast31)
#undef CMAX_BOX_STEP
    // which 1/64ths of the segment's slots hold an event that moved (scalar loop over the lanes that moved one: rare)
    unsigned long long wave_mask = 0ull;
    if (kExact) {
        unsigned long long bal = __builtin_amdgcn_ballot_w64(thread_exact);
        const int wave_first = (int)(threadIdx.x & ~(kWave - 1));
        while (bal != 0ull) {  // wave-uniform
            const int ln = __builtin_ctzll(bal);
            bal &= bal - 1ull;
            wave_mask |= 1ull << ((L::kEPT * (wave_first + ln)) >> L::kBlkShift);
            wave_mask |= 1ull << ((L::kEPT * (wave_first + ln) + L::kEPT - 1) >> L::kBlkShift);  // (six events per thread can straddle two 64ths)
        }
    }
    if ((threadIdx.x & (kWave - 1)) == kWave - 1) s_box[threadIdx.x / kWave] = make_uint4(mnq, mxp, (unsigned)wave_mask, (unsigned)(wave_mask >> 32));
    if (!WANT_DT) CMAX_STAMP(0, 2);
    __syncthreads();
    const uint2 *s_b2 = reinterpret_cast<const uint2 *>(s_box);
    uint2 bx = s_b2[0];
#pragma unroll
    for (int wv = 1; wv < L::kNW; ++wv) {
        const uint2 o = s_b2[2 * wv];
        bx.x = pk_max_u16(bx.x, o.x);
        bx.y = pk_max_u16(bx.y, o.y);
    }
    unsigned bmn = ~bx.x, bmx = bx.y;  // back to the minima (0xFFFF per field when no slot is valid)
    bmn = (unsigned)__builtin_amdgcn_readfirstlane((int)bmn);
    bmx = (unsigned)__builtin_amdgcn_readfirstlane((int)bmx);
    // The masks are for whoever publishes the window: WAVE 0 ONLY adds them up (the other waves' Window::bmask / border are not valid) --
    // 2 kNW more instructions per thread are what this costs every thread of a workgroup that holds four events per thread
    win.bmask = 0ull;
    if (kExact && threadIdx.x < kWave) {  // wave-uniform
        unsigned mz = 0u, mw = 0u;
#pragma unroll
        for (int wv = 0; wv < L::kNW; ++wv) {
            mz |= s_box[wv].z;
            mw |= s_box[wv].w;
        }
        win.bmask = (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)mz) | ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)mw) << 32);
    }
    win.border = win.bmask != 0ull;
    const int bmnr = (int)(bmn >> 16) - 16384, bmnc = (int)(bmn & 0xFFFFu) - 16384;
    const int bmxr = (int)(bmx >> 16) - 16384, bmxc = (int)(bmx & 0xFFFFu) - 16384;
    // Fast window: the whole 2x2 footprint of every event, NOT clipped to the image -> no per-vote tests
    // (cells outside the image are skipped by the flush / read as zero by the gather).
    {
        const bool any = bmx != 0u;
        const int h = any ? bmxr - bmnr + 2 : 0, w = any ? bmxc - bmnc + 2 : 0;
        const int stride = window_stride(w);
        if (w <= kWinMaxW && h * stride <= L::kWinCap) {
            win.r0 = any ? bmnr : 0;
            win.c0 = any ? bmnc : 0;
            win.h = h;
            win.w = w;
            win.stride = stride;
            win.clipped = false;
            init(win);
            return win;
        }
    }
    // Rare (very large displacements): window = centre of the box clipped to the image; votes / reads that
    // fall outside it but inside the image go to global memory, every corner is tested.
    int r0 = max(bmnr, 0), r1 = min(bmxr + 2, wp.Hp);
    int c0 = max(bmnc, 0), c1 = min(bmxc + 2, wp.Wp);
    int h = max(r1 - r0, 0), w = max(c1 - c0, 0);
    if (w > kWinMaxW) {
        c0 += (w - kWinMaxW) / 2;
        w = kWinMaxW;
    }
    const int stride = window_stride(w);
    const int hmax = L::kWinCap / stride;
    if (h > hmax) {
        r0 += (h - hmax) / 2;
        h = hmax;
    }
    win.clipped = true;
    win.stride = stride;
    win.r0 = r0;
    win.c0 = c0;
    win.h = h;
    win.w = w;
    init(win);
    return win;
}

// (the kernels without a WarpHead)
template <class L, int MODEL, bool FRAC, bool WANT_DT, bool STRIDED = false, bool KNOWN = false, bool F64FLOW = false, typename Init>
__device__ __forceinline__ Window phase_warp(const EvView &ev, const WarpParams &wp, int4 sg, EventLoads<L> &el, unsigned (&rc)[L::kEPT],
                                              float (&fa)[L::kEPT], float (&fb)[L::kEPT], float (&fdt)[L::kEPT], int (&fsrc)[L::kEPT],
                                              uint4 *s_box, const int4 *known, const unsigned *__restrict__ shifts, Init init, bool &wave_live,
                                              unsigned &nibbles) {
    return phase_warp<L, MODEL, FRAC, WANT_DT, STRIDED, KNOWN, F64FLOW>(ev, wp, sg, el, rc, fa, fb, fdt, fsrc, s_box, known, shifts, init, wave_live, nibbles, NoHead{});
}

// Local word index of an event's top-left corner in the fast window, origin = (r0 + 16384) * stride + c0 + 16384
// (one v_mad_u32_u24: both factors are below 2^24).
// An empty slot (rc == 0) gives 0 - origin, a huge unsigned, and is sent to `scratch` = kWinCap + lane: a per-lane
// word behind the window (64 lanes on ONE LDS address would serialise the atomic).
// Round 6: (rc >> 16) * stride - origin is ONE v_mad_u32_u16 (high half selected by op_sel; `neg_origin` = 0 - origin in a VGPR, the
// instruction's one scalar operand being the stride), the column joins through an SDWA add of rc's low half: two instructions + the
// min, where shift, mask, multiply-add, subtract and min were five.
__device__ __forceinline__ int fast_index(unsigned rc, unsigned neg_origin, int stride, unsigned scratch) {
    return (int)min(add_lo16_u(mad_hi16_u(rc, (unsigned)stride, neg_origin), rc), scratch);
}

// ---------------------------------------------------------------------------------------------
// K1: warp + bilinear vote.  LDS window in signed 12.20 fixed point (ds_add_u32), coalesced flush.
// ---------------------------------------------------------------------------------------------
// MU: also accumulate RefArgs::musum (blurred variance with a gradient) -- its own instantiation, so that the kernel every
// other objective runs carries none of it
// Kernel parameters: what the head dereferences first.  The first 14 argument dwords arrive in SGPRs (-amdgpu-kernarg-preload-count,
// build.py: 16 user SGPRs, two of them the argument block's own address), and they hold every pointer the head reads through: the work
// list, the events, theta and the batch's time extremes (K3: K1's windows as well).  As compiled, the head is then TWO dependent round
// trips -- { segment, theta, extremes, [window,] the argument block's words } under one scalar wait, then the events under one vector
// wait in front of the first warp instruction (profiles/head_loads_isa.txt).  Until that listing was taken the head was described
// as "arguments -> segment -> events"; the compiled kernels had four to five dependent trips: the events were waited for inside
// issue_event_loads (K1), the argument block was read behind them, and the time extremes and theta -- through pointers out of the
// argument block -- behind that.
// (second launch bound = waves per SIMD the register allocation has to leave room for: the 512 x 8 kernel of the big segments sat at 68
// VGPRs -- seven waves -- once the border tracking joined its warp loop; scheduled for 64 it keeps eight: K1 of 20M events 46.2 -> see
// profiles/r04_ablation.txt)
// WEIGHTED (cmax_set_event_weights): an event votes round(w / wmax * K) instead of K, split over its four cells from the row totals as
// before (the four integers add up to it exactly); wmax is folded back in by the flush.  The window, the cells and the offsets
// published for K3 do not depend on w.
// EXACT = called with an ExactFlow behind ra (dense / voxel, cmax_objective_t::motion_dtype == CMAX_F64): phase_warp's F64FLOW -- instantiations
// of their own, the ones without the argument are untouched.
template <class L, int MODEL, bool FRAC, bool MU = false, bool WEIGHTED = false, class... EXACT>
__global__ void __launch_bounds__(L::kThr, L::kVoteWaves)
k_vote(const int4 *__restrict__ segs, int nseg, int z_motion, const uint2 *__restrict__ evp, const char *__restrict__ cev, const float *__restrict__ motion,
       const double *__restrict__ tmm, int head_flags, EvView ev, WarpParams wp, RefArgs ra, EXACT...) {
    constexpr bool F64FLOW = sizeof...(EXACT) > 0;
    static_assert(sizeof...(EXACT) <= 1 && (std::is_same_v<EXACT, ExactFlow> && ...), "k_vote: an ExactFlow or nothing");
    __shared__ int s_win[L::kWinCap + kScratch];
    __shared__ uint4 s_box[L::kNW];
    CMAX_STAMP(0, 0);
    // first thing: this workgroup's segment, and with it everything else the head reads from memory -- the batch period and theta
    // (load_head_words; standard segments).  All leading parameters arrive in SGPRs: none of these loads waits for the argument block.
    const int sidx = segment_of_block(nseg);
    if (sidx >= nseg) return;
    const int4 sg = segs[sidx];
    motion += (int64_t)blockIdx.z * z_motion;  // blockIdx.z = candidate motion (cmax_objective_batch; one candidate otherwise)
    ev.ev = evp;
    wp.motion = motion;
    wp.d = ra.d[blockIdx.y];  // blockIdx.y = reference time
    HeadWords headw = {};
    if constexpr (L::kEntryHead) {
        headw = load_head_words<MODEL>(motion, tmm, head_flags);
        // ... and the words of the argument block the warp needs: ONE batch of scalar loads, issued before the first wait.  (Left to
        // the compiler they followed the wait for the events, in two dependent groups: profiles/head_loads_isa.txt.)
        asm volatile("" ::"s"(sg.x), "s"(sg.y), CMAX_HEAD_PIN_WORDS(headw), "s"(wp.d), "s"(wp.H), "s"(wp.W), "s"(wp.ph), "s"(wp.pw));
    }
    EventLoads<L> el;
    issue_event_loads<L, false>(evp, cev, sidx, sg, el);
    std::conditional_t<L::kEntryHead, WarpHead, NoHead> head;  // (mid / big segments: phase_warp reads period and theta itself)
    if constexpr (L::kEntryHead) head = decode_head_words(headw, head_flags);
    static_assert(!(MU && WEIGHTED), "the vote sums of the blurred variance count events: weighted handles take the unfused image path");
    float fw[L::kEPT];
    float wscale = 0.f, inv_fix = L::kInvFixNS;  // K / wmax; 1 / K, weighted: wmax / K
    if constexpr (WEIGHTED) {  // (the slot weights themselves are loaded behind the warp, below)
        wscale = ra.wnorm[0] * L::kFixNS;
        inv_fix = ra.wnorm[1] * L::kInvFixNS;
    }
    wp.d_lo = ra.d_lo[blockIdx.y];  // (read by warp_exact only: the compiler sinks this scalar load into that rare path)
    const int zy = (int)(blockIdx.z * gridDim.y + blockIdx.y);  // (candidate, reference time): index of this launch's windows / offsets
    float *__restrict__ iwe = ra.img[blockIdx.y] + blockIdx.z * ra.z_img;
    long long *__restrict__ iwe64 = ra.img64[blockIdx.y];  // deterministic mode: integer image instead (launch-uniform)
    // kernel arguments that are first used between the two barriers: fetched here, with the others -- left to the compiler they were
    // three scalar loads with a wait each at their points of use, on the critical path of every workgroup
    int4 *const win_base = ra.win;
    unsigned *const shifts_base = ra.shifts;
    const int windows_only = ra.windows_only;
    asm volatile("" ::"s"(win_base), "s"(shifts_base), "s"(windows_only));
    unsigned rc[L::kEPT];
    float fa[L::kEPT], fb[L::kEPT], fdt[L::kEPT];
    int fsrc[L::kEPT];
    bool live;  // this wave holds events (wave-uniform)
    unsigned nibbles;  // cell offsets of the events this thread decided in fp64 (phase_warp)
    const Window win = phase_warp<L, MODEL, FRAC, false, false, false, F64FLOW>(ev, wp, sg, el, rc, fa, fb, fdt, fsrc, s_box, nullptr, nullptr, [&](const Window &w) {
        const int wn = w.h * w.stride;
        for (int i = threadIdx.x; i < wn; i += L::kThr) s_win[i] = 0;
    }, live, nibbles, head);
    CMAX_STAMP(0, 3);
    // the weights of this thread's slots: loaded HERE, not with the events -- live through the warp they are kEPT more registers at the
    // kernel's peak, and the b512 instantiations (eight events per thread under the 64-VGPR bound of kVoteWaves) spilled them to scratch;
    // first used behind the barrier below, which hides the load
    if constexpr (WEIGHTED) load_slot_weights<L, false>(ra.wgt, sg, fw);
    if (ra.grad_zero && blockIdx.y == 0 && blockIdx.z == 0) {  // launch-uniform: this workgroup's slice of the gradient buffer K3 will add into (write-through)
        const int64_t chunk4 = (ra.n_grad_zero4 + nseg - 1) / nseg, q1 = min(ra.n_grad_zero4, (int64_t)(sidx + 1) * chunk4);
        for (int64_t q = (int64_t)sidx * chunk4 + threadIdx.x; q < q1; q += L::kThr) store_zero4_sc1(reinterpret_cast<float *>(ra.grad_zero + q));
    }
    if (blockIdx.x == 0) {  // (behind the event loads: their pointers come out of the argument block, and a wait for it at the head of the
        // kernel stood in front of every workgroup's first load)
        double *__restrict__ stat_zero = ra.stat[blockIdx.y] ? ra.stat[blockIdx.y] + blockIdx.z * ra.z_raw : nullptr;
        // the statistics accumulators of the image being filled are reset here (K2 follows in stream order)
        // (8 doubles on each of the kStatSub lines: the statistics use two of them, the raw sums of the deferred 2-DoF K3 six)
        if (stat_zero && threadIdx.x < 8 * kStatSub) stat_zero[(threadIdx.x >> 3) * kSubStride + (threadIdx.x & 7)] = 0.0;
        // ... and the lines the 2-DoF K3 of this evaluation adds its gradient sums to (objectives that also keep statistics)
        if (ra.raw_zero && threadIdx.x < 8 * kStatSub)
            ra.raw_zero[(int64_t)blockIdx.y * kRawStride + (threadIdx.x >> 3) * kSubStride + (threadIdx.x & 7)] = 0.0;
    }
    // for K3 of the same evaluation: the window, and -- rare -- the cell offsets of the events that were decided in fp64.  The words of
    // the 1/64ths of the segment that Window::bmask names are cleared here and filled behind the barrier below (the others are never read)
    unsigned *__restrict__ shifts = (MODEL >= 0 && shifts_base) ? shifts_base + ((int64_t)zy * nseg + sidx) * L::kShiftWords : nullptr;
    if (win_base && threadIdx.x == 0) win_base[(int64_t)zy * nseg + sidx] = pack_window(win);  // (wave 0: its Window::bmask is the valid one)
    if (MODEL >= 0 && shifts && win.border) {  // wave 0 only (wave-uniform), rare
        for (int t = threadIdx.x; t < L::kShiftWords; t += kWave)
            if ((win.bmask >> (t >> (L::kBlkShift - 3))) & 1ull) /* a word holds 8 slots */ __hip_atomic_store(&shifts[t], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // Blurred variance (RefArgs::musum, see k_blur_stats_adj_var): sum_p I[p] b(row) b(col) over the votes.  b = 1 except within two
    // pixels of the border and an event's four weights add up to 1, so the sum is the NUMBER OF EVENTS (which the host knows)
    // plus a correction from the workgroups whose window touches that band or leaves the image -- only those do anything here
    // (macc: this thread's share of the correction).
    double *__restrict__ musum = MU ? ra.musum[blockIdx.y] : nullptr;
    const bool band = MU && (win.clipped || win.r0 < 2 || win.r0 + win.h > wp.Hp - 2 || win.c0 < 2 || win.c0 + win.w > wp.Wp - 2);
    float macc = 0.f;
    auto band_weight = [&](int r, int c) -> float {
        const float br = (r < 2 || r >= wp.Hp - 2) ? ((r == 0 || r == wp.Hp - 1) ? ra.band_b0 : ra.band_b1) : 1.f;
        const float bc = (c < 2 || c >= wp.Wp - 2) ? ((c == 0 || c == wp.Wp - 1) ? ra.band_b0 : ra.band_b1) : 1.f;
        return br * bc;
    };
    __syncthreads();
    if (MODEL >= 0 && shifts && nibbles != 0u) {  // this thread's kEPT slots share one word of 8 nibbles, or (six per thread) straddle two
        const int l0 = L::kEPT * (int)threadIdx.x;
        const unsigned long long nb = (unsigned long long)nibbles << ((l0 & 7) * 4);
        if ((unsigned)nb) atomicOr(&shifts[l0 >> 3], (unsigned)nb);
        if ((unsigned)(nb >> 32)) atomicOr(&shifts[(l0 >> 3) + 1], (unsigned)(nb >> 32));
    }
    CMAX_STAMP(0, 4);
    if (windows_only) return;  // launch-uniform: the windows and offsets for a K3 whose vote this was not
    if (!live) {
        // a wave without events votes nothing
    } else if (!win.clipped) {
        // phase B, fast window: 4 votes per event, no tests.  w_pos0..3 of event_image_converter.py:365-368 as
        // 12.20 fixed point: (na K) nb etc. equal (na nb) K exactly (K is a power of two)
        unsigned neg_origin = 0u - ((unsigned)(win.r0 + 16384) * (unsigned)win.stride + (unsigned)(win.c0 + 16384));
        asm volatile("" : "+v"(neg_origin));  // (a VGPR: v_mad_u32_u16's one scalar operand is the stride)
        const int stride = win.stride;
        const unsigned scratch = L::kWinCap + (threadIdx.x & (kWave - 1));
        // Consecutive events of a thread that fall into the same cell are summed in registers first (fixed point: exact).
        // On a sharp image -- what the optimiser converges to -- hundreds of votes land on a few LDS words and the LDS
        // atomic unit serialises equal addresses; neighbouring sorted events mostly share their cell then.  Uniform events:
        // +0.15 us (nothing to merge); 1M events of 2500 dots at their true motion: K1 8.5 -> 7.0 us, cfg3 24.5 -> 21.6 us.
        {  // (a second copy of this loop for full waves -- no min in the index -- measured: 14 VALU instructions per wave less, the same time)
            int cur = -1, w0 = 0, w1 = 0, w2 = 0, w3 = 0;
#pragma unroll
            for (int u = 0; u < L::kEPT; ++u) {
                const float a = fa[u], b = fb[u];
                float kf = L::kFixNS;
                int ktot = (int)L::kFixNS;
                if constexpr (WEIGHTED) {  // the event's whole vote, rounded once; its four shares below add up to it exactly
                    ktot = cvt_rpi(fw[u] * wscale);
                    kf = (float)ktot;
                }
                const float ak = a * kf, nak = kf - ak;
                const int idx = fast_index(rc[u], neg_origin, win.stride, scratch);
                // Round 6: the two weights of a ROW from the row's total -- r0 = rpi((1 - a) K), v1 = rpi((1 - a) b K), v0 = r0 - v1; the lower
                // row from K - r0 -- three conversions and three integer subtractions where four products and four conversions were: the four
                // weights of an event now add up to K EXACTLY (each within one unit, 2^-19 / 2^-20 of a vote, of its separately rounded value)
                const int r0 = cvt_rpi(nak), r1 = ktot - r0;
                const int v1 = cvt_rpi(nak * b), v0 = r0 - v1, v3 = cvt_rpi(ak * b), v2 = r1 - v3;
                if (idx != cur) {
                    if (cur >= 0) {
                        atomicAdd(&s_win[cur], w0);
                        atomicAdd(&s_win[cur + 1], w1);
                        atomicAdd(&s_win[cur + stride], w2);
                        atomicAdd(&s_win[cur + stride + 1], w3);
                    }
                    cur = idx;
                    w0 = v0;
                    w1 = v1;
                    w2 = v2;
                    w3 = v3;
                } else {
                    w0 += v0;
                    w1 += v1;
                    w2 += v2;
                    w3 += v3;
                }
            }
            atomicAdd(&s_win[cur], w0);
            atomicAdd(&s_win[cur + 1], w1);
            atomicAdd(&s_win[cur + stride], w2);
            atomicAdd(&s_win[cur + stride + 1], w3);
        }
        // workgroup-uniform, windows that reach outside the image only: the share of each event's unit vote that leaves it
        // (the flush skips those cells)
        if (band && (win.r0 < 0 || win.r0 + win.h > wp.Hp || win.c0 < 0 || win.c0 + win.w > wp.Wp)) {
#pragma unroll
            for (int u = 0; u < L::kEPT; ++u) {
                const int row = (int)(rc[u] >> 16) - 16384, col = (int)(rc[u] & 0xFFFFu) - 16384;
                const float a = fa[u], b = fb[u];
                const float wr = ((unsigned)row < (unsigned)wp.Hp ? 1.f - a : 0.f) + ((unsigned)(row + 1) < (unsigned)wp.Hp ? a : 0.f);
                const float wc = ((unsigned)col < (unsigned)wp.Wp ? 1.f - b : 0.f) + ((unsigned)(col + 1) < (unsigned)wp.Wp ? b : 0.f);
                if (rc[u] != 0u) macc -= 1.f - wr * wc;
            }
        }
    } else {
        // workgroup-uniform, rare: every corner tested; a vote outside the window adds 0 to a per-lane scratch
        // word, and goes to the image with a global atomic if it is inside the image
        const int dummy = L::kDummy + (int)(threadIdx.x & (kWave - 1));
#pragma unroll
        for (int u = 0; u < L::kEPT; ++u) {
            const int row = (int)(rc[u] >> 16) - 16384, col = (int)(rc[u] & 0xFFFFu) - 16384;  // empty slot: (-16384, -16384)
            const float a = fa[u], b = fb[u], na = 1.f - a, nb = 1.f - b;
            const int lr = row - win.r0, lc = col - win.c0;
            const bool r_in0 = (unsigned)lr < (unsigned)win.h, r_in1 = (unsigned)(lr + 1) < (unsigned)win.h;
            const bool c_in0 = (unsigned)lc < (unsigned)win.w, c_in1 = (unsigned)(lc + 1) < (unsigned)win.w;
            const int base = lr * win.stride + lc;
            const int stride = win.stride;
            float kq = L::kFixNS, wq = 1.f;  // the event's vote in the window's fixed point / in the image's unit
            if constexpr (WEIGHTED) {
                kq = fw[u] * wscale;
                wq = fw[u];
            }
            atomicAdd(&s_win[(r_in0 && c_in0) ? base : dummy], (r_in0 && c_in0) ? __float2int_rn(na * nb * kq) : 0);
            atomicAdd(&s_win[(r_in1 && c_in0) ? base + stride : dummy], (r_in1 && c_in0) ? __float2int_rn(a * nb * kq) : 0);
            atomicAdd(&s_win[(r_in0 && c_in1) ? base + 1 : dummy], (r_in0 && c_in1) ? __float2int_rn(na * b * kq) : 0);
            atomicAdd(&s_win[(r_in1 && c_in1) ? base + stride + 1 : dummy], (r_in1 && c_in1) ? __float2int_rn(a * b * kq) : 0);
            if (rc[u] == 0u) continue;
            float wv[4] = {na * nb, a * nb, na * b, a * b};
            if constexpr (WEIGHTED) {
#pragma unroll
                for (int q = 0; q < 4; ++q) wv[q] *= wq;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = row + (q & 1), c = col + (q >> 1);
                const bool in_win = (unsigned)(r - win.r0) < (unsigned)win.h && (unsigned)(c - win.c0) < (unsigned)win.w;
                if (!in_win && (unsigned)r < (unsigned)wp.Hp && (unsigned)c < (unsigned)wp.Wp) {
                    if (iwe64) atomic_add_i64(&iwe64[(int64_t)r * wp.Wp + c], (long long)__float2int_rn(wv[q] * L::kFixNS));
                    else atomic_add(&iwe[(int64_t)r * wp.Wp + c], wv[q]);
                    if (band) macc += wv[q] * (band_weight(r, c) - 1.f);  // (a clipped window is a band window, and lies inside the image)
                } else if (band && !in_win) {
                    macc -= wv[q];  // a vote that leaves the image
                }
            }
        }
    }
    CMAX_STAMP(0, 5);
    __syncthreads();
    CMAX_STAMP(0, 6);
    // flush: one coalesced global atomic per touched window pixel inside the image (a wave per window row)
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (band) {
        // workgroup-uniform.  Before the flush (a global atomic issued last would put its round trip at the end of the kernel:
        // K1 of cfg4 +0.6 us), and only over the cells that count: with val = the votes of a cell,
        //   sum_p I[p] b b = (number of events) - (votes that left the image: counted per event above)
        //                    + sum over the BAND cells of the image of val (b b - 1),
        // the cells of this window in columns 0, 1, Wp - 2, Wp - 1 (rows outside the band rows), then in rows 0, 1, Hp - 2, Hp - 1:
        // one cell per thread and part, no loop-carried LDS latency.
        for (int t = threadIdx.x; t < 4 * win.h; t += L::kThr) {
            const int r = t >> 2, q = t & 3, R = win.r0 + r;
            const int C = q < 2 ? q : wp.Wp - 4 + q, c = C - win.c0;
            if ((unsigned)c < (unsigned)win.w && R >= 2 && R < wp.Hp - 2) macc += (float)s_win[r * win.stride + c] * L::kInvFixNS * (band_weight(R, C) - 1.f);
        }
        for (int q = 0; q < 4; ++q) {
            const int R = q < 2 ? q : wp.Hp - 4 + q, r = R - win.r0;
            if ((unsigned)r >= (unsigned)win.h) continue;  // workgroup-uniform
            for (int c = threadIdx.x; c < win.w; c += L::kThr) {
                const int C = win.c0 + c;
                if ((unsigned)C < (unsigned)wp.Wp) macc += (float)s_win[r * win.stride + c] * L::kInvFixNS * (band_weight(R, C) - 1.f);
            }
        }
        float m = macc;  // fp32 over the wave, fp64 across waves and workgroups
        m += dpp_f<kDppRowShr1>(m);
        m += dpp_f<kDppRowShr2>(m);
        m += dpp_f<kDppRowShr4>(m);
        m += dpp_f<kDppRowShr8>(m);
        m += dpp_f<kDppRowBcast15>(m);
        m += dpp_f<kDppRowBcast31>(m);
        // no reduction across the waves: every wave that found anything sends its own sum, ahead of its share of the flush
        if (lane == kWave - 1 && m != 0.f) atomic_add(&musum[((sidx * L::kNW + wave) % kMuLines) * kSubStride], (double)m);
    }
    if (iwe64) {
        // deterministic mode: the window's integers go to a 64-bit integer image as they are (exact, any order);
        // k_fixed_to_image rounds the finished sums to fp32 once
        for (int r = wave; r < win.h; r += L::kNW) {
            if ((unsigned)(win.r0 + r) >= (unsigned)wp.Hp) continue;
            long long *dst = iwe64 + (pix_index(win.r0 + r, 0, wp.Wp) + win.c0);
            for (int c = lane; c < win.w; c += kWave) {
                const int v = s_win[r * win.stride + c];
                if (v != 0 && (unsigned)(win.c0 + c) < (unsigned)wp.Wp) atomic_add_i64(&dst[c], (long long)v);
            }
        }
    } else if (L::kBig) {
        // Big segments: FLAT walk over the window's LDS words (see K3's window staging; the padding column holds 0).  Measured: K1 of
        // 20M events 38.3 -> 37.6 us, 64M 127.3 -> 126.7; with standard segments it is the row form that wins (cfg5 shard 12.95 vs 13.4).
        // row = i / stride = (i * ceil(2^21 / stride)) >> 21, exact for i < 2^13, stride < 2^8; both products are 24-bit multiplies
        const unsigned ustride = (unsigned)win.stride, magic = ((1u << 21) + ustride - 1u) / ustride;
        const int wn = win.h * win.stride;
        if (win.r0 >= 0 && win.c0 >= 0 && win.r0 + win.h <= wp.Hp && win.c0 + win.w <= wp.Wp && win.stride <= wp.Wp) {
            // workgroup-uniform (round 6): the window lies inside the image -- most do -- so no cell needs a test (the padding column holds
            // 0), and word i = r stride + c goes to pixel (r0 + r) Wp + c0 + c = [r0 Wp + c0] + r (Wp - stride) + i: the row by the magic
            // multiply, one multiply-add, the conversion and the scale -- 6 VALU instructions per non-zero word where the tested form has 14
            float *__restrict__ base = iwe + pix_index(win.r0, win.c0, wp.Wp);
            const unsigned pitch_diff = (unsigned)wp.Wp - ustride;  // (>= 0: tested above; a window as wide as the image may have stride = Wp + 1)
            for (int i = threadIdx.x; i < wn; i += L::kThr) {
                const int v = s_win[i];
                if (v == 0) continue;
                const unsigned r = mul24_u((unsigned)i, magic) >> 21;
                atomic_add(&base[mad24_u(r, pitch_diff, (unsigned)i)], (float)v * inv_fix);
            }
        } else {
            for (int i = threadIdx.x; i < wn; i += L::kThr) {
                const int v = s_win[i];
                if (v == 0) continue;
                const unsigned r = mul24_u((unsigned)i, magic) >> 21, c = (unsigned)i - mul24_u(r, ustride);
                const int R = win.r0 + (int)r, C = win.c0 + (int)c;
                if ((unsigned)R < (unsigned)wp.Hp && (unsigned)C < (unsigned)wp.Wp) atomic_add(&iwe[pix_index(R, C, wp.Wp)], (float)v * inv_fix);
            }
        }
    } else if (win.w > 32) {
        for (int r = wave; r < win.h; r += L::kNW) {
            if ((unsigned)(win.r0 + r) >= (unsigned)wp.Hp) continue;
            float *dst = iwe + (pix_index(win.r0 + r, 0, wp.Wp) + win.c0);
            for (int c = lane; c < win.w; c += kWave) {
                const int v = s_win[r * win.stride + c];
                if (v != 0 && (unsigned)(win.c0 + c) < (unsigned)wp.Wp) atomic_add(&dst[c], (float)v * inv_fix);
            }
        }
    } else {  // narrow window: two rows per wave
        const int half = lane >> 5, c = lane & 31;
        for (int r = 2 * wave + half; r < win.h; r += 2 * L::kNW) {
            if (c < win.w && (unsigned)(win.r0 + r) < (unsigned)wp.Hp && (unsigned)(win.c0 + c) < (unsigned)wp.Wp) {
                const int v = s_win[r * win.stride + c];
                if (v != 0) atomic_add(&iwe[pix_index(win.r0 + r, win.c0 + c, wp.Wp)], (float)v * inv_fix);
            }
        }
    }
    CMAX_STAMP(0, 7);
}

// ---------------------------------------------------------------------------------------------
// K1T (2-DoF): warp + vote of the image AND of its two tangent images, so that loss and gradient of a 2-DoF objective
// follow in image space without a second pass over the events (and, across GPUs, from ONE all-reduce).
//   x' = x + dt theta0 moves the row fraction a, y' the column fraction b; with the cell held fixed
//     dI/dtheta0 = sum_e dt [ -(1-b) d(r,c) - b d(r,c+1) + (1-b) d(r+1,c) + b d(r+1,c+1) ]
//   = (E0 shifted one row down) - E0,   E0[r,c] += dt (1-b), E0[r,c+1] += dt b      -- TWO votes instead of four,
//     dI/dtheta1 = (F1 shifted one column right) - F1,   F1[r,c] += dt (1-a), F1[r+1,c] += dt a,
//   and  dL/dtheta0 = <G, dI/dtheta0> = sum_q E0[q] (G~[q + (1,0)] - G~[q])  with G~ = dL/dIWE, zero outside the image
//   (a vote outside the image is dropped by the reference, so its G is zero): row -1 of E0 and column -1 of F1 still
//   matter (their lower / right neighbour is inside), hence E0 is [Hp + 1, Wp] with row offset 1, F1 [Hp, Wp + 1].
// LDS: three planes of kTanCap words in the window's coordinates, 12.20 fixed point for I and 14.18 for the tangent planes
// (|dt| <= 2 for the "before" / "after" reference times: 2040 x 2 x 2^18 = 2^30).  dt is the NORMALISED one here; the
// image-space kernel multiplies by the batch period when normalize_t is off.
// ---------------------------------------------------------------------------------------------
template <class L, bool FRAC>
__global__ void __launch_bounds__(L::kThr) k_vote_tan2(const int4 *__restrict__ segs, int nseg, EvView ev, WarpParams wp, RefArgs ra) {
    __shared__ int s_win[3 * L::kTanCap + kScratch];
    __shared__ uint4 s_box[L::kNW];
    wp.d = ra.d[blockIdx.y];  // blockIdx.y = reference time
    wp.d_lo = ra.d_lo[blockIdx.y];
    float *__restrict__ iwe = ra.img[blockIdx.y];                      // [Hp, Wp]
    float *__restrict__ e0g = iwe + (int64_t)wp.Hp * wp.Wp;            // [Hp + 1, Wp], row -1 first
    float *__restrict__ f1g = e0g + (int64_t)(wp.Hp + 1) * wp.Wp;      // [Hp, Wp + 1], column -1 first
    const float ts = time_scale(wp), inv_ts = ts > 0.f ? 1.f / ts : 0.f;  // fdt is in the warp's time unit; the votes carry dt / period
    const int sidx = segment_of_block(nseg);
    if (sidx >= nseg) return;
    const int4 sg = segs[sidx];
    EventLoads<L> el;
    issue_event_loads<L, false>(ev.ev, nullptr, 0, sg, el);
    unsigned rc[L::kEPT];
    float fa[L::kEPT], fb[L::kEPT], fdt[L::kEPT];
    int fsrc[L::kEPT];
    bool live;
    unsigned nib_unused;
    const Window win = phase_warp<L, CMAX_MODEL_2DOF, FRAC, true>(ev, wp, sg, el, rc, fa, fb, fdt, fsrc, s_box, nullptr, nullptr, [&](const Window &w) {
        const int wn = w.h * w.stride;
        if (wn <= L::kTanCap)
            for (int i = threadIdx.x; i < wn; i += L::kThr) {
                s_win[i] = 0;
                s_win[L::kTanCap + i] = 0;
                s_win[2 * L::kTanCap + i] = 0;
            }
    }, live, nib_unused);
    const int wn = win.h * win.stride;
    const bool fits = !win.clipped && wn <= L::kTanCap;  // workgroup-uniform
    __syncthreads();
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (fits) {
        if (live) {
            const unsigned origin = (unsigned)(win.r0 + 16384) * (unsigned)win.stride + (unsigned)(win.c0 + 16384);
            const int stride = win.stride;
#pragma unroll
            for (int u = 0; u < L::kEPT; ++u) {
                if (rc[u] == 0u) continue;
                const float a = fa[u], b = fb[u], dt = fdt[u] * inv_ts;
                const float ak = a * L::kFixNS, nak = L::kFixNS - ak, nb = 1.f - b;
                const int idx = (int)(__umul24(rc[u] >> 16, (unsigned)win.stride) + (rc[u] & 0xFFFFu) - origin);  // inside the window by construction
                // the image plane gets the SAME integers as k_vote (weights from row totals): both paths then sum identical votes
                const int r0 = cvt_rpi(nak), r1 = (int)L::kFixNS - r0, v1 = cvt_rpi(nak * b), v3 = cvt_rpi(ak * b);
                atomicAdd(&s_win[idx], r0 - v1);
                atomicAdd(&s_win[idx + 1], v1);
                atomicAdd(&s_win[idx + stride], r1 - v3);
                atomicAdd(&s_win[idx + stride + 1], v3);
                const float dk = dt * L::kTanFix;
                atomicAdd(&s_win[L::kTanCap + idx], cvt_rpi(dk * nb));
                atomicAdd(&s_win[L::kTanCap + idx + 1], cvt_rpi(dk * b));
                atomicAdd(&s_win[2 * L::kTanCap + idx], cvt_rpi(dk * (1.f - a)));
                atomicAdd(&s_win[2 * L::kTanCap + idx + stride], cvt_rpi(dk * a));
            }
        }
        __syncthreads();
        // flush: a wave per window row and plane
        for (int r = wave; r < win.h; r += L::kNW) {
            const int R = win.r0 + r;
            for (int c = lane; c < win.w; c += kWave) {
                const int C = win.c0 + c, q = r * win.stride + c;
                const int v = s_win[q], e = s_win[L::kTanCap + q], f = s_win[2 * L::kTanCap + q];
                const bool rin = (unsigned)R < (unsigned)wp.Hp, cin = (unsigned)C < (unsigned)wp.Wp;
                if (v != 0 && rin && cin) atomic_add(&iwe[(int64_t)R * wp.Wp + C], (float)v * L::kInvFixNS);
                if (e != 0 && cin && (unsigned)(R + 1) <= (unsigned)wp.Hp) atomic_add(&e0g[(int64_t)(R + 1) * wp.Wp + C], (float)e * L::kTanInvFix);
                if (f != 0 && rin && (unsigned)(C + 1) <= (unsigned)wp.Wp) atomic_add(&f1g[(int64_t)R * (wp.Wp + 1) + C + 1], (float)f * L::kTanInvFix);
            }
        }
    } else if (live) {
        // window too large for three planes (very large displacements): straight to memory, every vote tested
#pragma unroll
        for (int u = 0; u < L::kEPT; ++u) {
            if (rc[u] == 0u) continue;
            const int row = (int)(rc[u] >> 16) - 16384, col = (int)(rc[u] & 0xFFFFu) - 16384;
            const float a = fa[u], b = fb[u], dt = fdt[u] * inv_ts, na = 1.f - a, nb = 1.f - b;
            auto vote_i = [&](int r, int c, float w) {
                if ((unsigned)r < (unsigned)wp.Hp && (unsigned)c < (unsigned)wp.Wp) atomic_add(&iwe[(int64_t)r * wp.Wp + c], w);
            };
            vote_i(row, col, na * nb);
            vote_i(row, col + 1, na * b);
            vote_i(row + 1, col, a * nb);
            vote_i(row + 1, col + 1, a * b);
            auto vote_e = [&](int r, int c, float w) {
                if ((unsigned)(r + 1) <= (unsigned)wp.Hp && (unsigned)c < (unsigned)wp.Wp) atomic_add(&e0g[(int64_t)(r + 1) * wp.Wp + c], w);
            };
            vote_e(row, col, dt * nb);
            vote_e(row, col + 1, dt * b);
            auto vote_f = [&](int r, int c, float w) {
                if ((unsigned)r < (unsigned)wp.Hp && (unsigned)(c + 1) <= (unsigned)wp.Wp) atomic_add(&f1g[(int64_t)r * (wp.Wp + 1) + c + 1], w);
            };
            vote_f(row, col, dt * na);
            vote_f(row + 1, col, dt * a);
        }
    }
}

// kFoldStatsInside: the K2 of a plain variance as the leading workgroups of the K3 launch (k_stats<VARIANCE> with the layout's
// workgroup size).  They finish long before the gathering workgroups do, so the ticket that finds the last of them -- four
// dependent fabric round trips -- costs the evaluation nothing; that one writes the loss.
template <class L>
__device__ __forceinline__ void stats_inside_role(const float *__restrict__ img, float *__restrict__ zero_img, int H, int W, const ObjParams &op,
                                                  double *__restrict__ stat_slot, const RefArgs &ra, double *__restrict__ result, double *smem) {
    const int nblk = ra.stat_blocks;
    const unsigned npix = (unsigned)H * (unsigned)W, stride = (unsigned)nblk * L::kThr;
    const int i0 = op.omit ? 1 : 0;
    double v[2] = {0.0, 0.0};
    for (unsigned base = blockIdx.x * L::kThr + threadIdx.x; base < npix; base += 4u * stride) {
        float x[4];
        bool in[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {  // 4 independent loads in flight per thread
            const unsigned p = base + (unsigned)u * stride;
            const unsigned r = p / (unsigned)W, c = p - r * (unsigned)W;
            in[u] = p < npix && (int)r >= i0 && (int)r < H - i0 && (int)c >= i0 && (int)c < W - i0;
            x[u] = img[p < npix ? p : npix - 1u];  // unconditional: see pin()
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) pin(x[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = in[u] ? x[u] : 0.f;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double xd = (double)x[u];
            v[0] += xd;
            v[1] += xd * xd;
        }
    }
    // behind the loads (see k_stats): the vote image of the next evaluation, and the other buffer of the vote sums
    zero_fill_sc1(zero_img, (int64_t)npix, (int64_t)blockIdx.x * L::kThr + threadIdx.x, (int64_t)nblk * L::kThr);
    if (blockIdx.x == 0 && threadIdx.x < kMuLines)
        __hip_atomic_store(&ra.musum_next[threadIdx.x * kSubStride], 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    block_sum<2>(v, smem);
    if (threadIdx.x == 0) {
        double *a = stat_slot + kSubStride * (blockIdx.x % op.nsub);
        atomic_add(&a[0], v[0]);
        atomic_add(&a[1], v[1]);
        if (arrive_last(ra.ticket, (int)blockIdx.x, nblk)) write_result_variance_agent(op, stat_slot, result);
    }
}

// ---------------------------------------------------------------------------------------------
// K3: per-event gradient, one workgroup per segment (same work list and window as K1).
//     The dL/dIWE window is staged in LDS; per event
//        dL/dx' = (1-b)(G10-G00) + b(G11-G01),  dL/dy' = (1-a)(G01-G00) + a(G11-G10)
//     2-DoF : per-workgroup fp64 partial of sum dt*(gx, gy) -> gpart[block] (summed by k_finish)
//     dense : -dt*g reduced over runs of equal source pixel inside the wave (events are sorted by
//             pixel), one fp32 atomic per run and channel
//     FOLD  : where dL/dIWE comes from -- a finished G image (kFoldNone), one that still lacks its chain factor (kFoldScale:
//             normalised costs), or the raw vote image itself (kFoldStats / kFoldStatsInside / kFoldDeferred: plain variance,
//             G = c2 (IWE - mu) 1_Omega is never materialised; c2 and mu enter after the gather)
// ---------------------------------------------------------------------------------------------
//     VARIANT (dense / voxel): how the per-event terms -dt*g reach the flow gradient
//        kGradRuns    dense: runs reduced serially per thread + one segmented scan, one atomic per run; voxel: LDS accumulators,
//                     atomic flush of the non-zero cells
//        kGradStrided dense, short runs: one segmented scan per slot pair over lanes holding consecutive events
//        kGradDet     deterministic mode (any model): each event's term is converted to 64-bit fixed point on its own (scale
//                     from max |image|, identical in every workgroup) and only integers are added from there on -- per
//                     thread, per workgroup, and with 64-bit global atomics for the flow gradient (one pair per event:
//                     slow, exact, independent of the order of events, workgroups and atomics)
//        kGradOwned   the work list gives every group (source tile, or (tile, time bin)) to exactly ONE segment and the
//                     objective has one reference time: LDS accumulators, and the flush STORES every cell of the segment's
//                     groups (zeros included), coalesced 64-byte rows -- no atomics, and nobody has to clear the gradient
//                     buffer first
// ---------------------------------------------------------------------------------------------
//     WEIGHTED (cmax_set_event_weights): dt <- w dt per event -- every sum below is linear in dt, so the 2-DoF wave sums, the dense run
//             reduction, the LDS accumulators and the block-scaled fixed point of the owned path (its scale is the workgroup's largest
//             WEIGHTED term) all follow
template <class L, int MODEL, bool FRAC, int FOLD, int VARIANT, bool WEIGHTED = false>
__global__ void __launch_bounds__(L::kThr)
k_grad(const int4 *__restrict__ segs, int nseg, int head_word, const uint2 *__restrict__ evp, const char *__restrict__ cev, const int4 *__restrict__ win_base,
       const float *__restrict__ motion, const double *__restrict__ tmm, EvView ev, WarpParams wp, RefArgs ra, ObjParams op,
       const double *__restrict__ stat, double *__restrict__ gpart_base, float *__restrict__ gflow, double *__restrict__ result) {
    // head_word (the 14 preloaded dwords hold six pointers, nseg and this): bits 0-1 = the head's flags (load_head_words), bits 2-4 =
    // the launch's reference times (gridDim.y: read from the argument block it was a dependent load in front of the window's); above
    // them what else the head of this MODEL needs -- 2-DoF: floats between the candidates' thetas (cmax_objective_batch: blockIdx.z),
    // flow models (one candidate per launch): RefArgs::stat_blocks, the leading workgroups that run the statistics (kFoldStatsInside)
    const int head_flags = head_word & 3, n_ref_grid = (head_word >> 2) & 7;
    const int stat_blocks = MODEL == CMAX_MODEL_2DOF ? 0 : head_word >> 5;
    constexpr bool STRIDED = VARIANT == kGradStrided;
    constexpr bool kOwned = VARIANT == kGradOwned || VARIANT == kGradOwnedSmall;
    constexpr bool kDet = VARIANT == kGradDet;  // deterministic mode: every per-event term is added as a 64-bit integer
    static_assert(!kDet || FOLD == kFoldNone || FOLD == kFoldStats, "deterministic mode runs the unfused image path");
    constexpr bool kInside = FOLD == kFoldStatsInside;                // the statistics run as the leading workgroups of this launch
    constexpr bool kStatsFold = FOLD == kFoldStats || kInside;        // the window holds the masked raw image
    static_assert(!kInside || MODEL != CMAX_MODEL_2DOF, "statistics inside K3: flow-gradient models, one reference time");
    static_assert(!kOwned || MODEL == CMAX_MODEL_DENSE || MODEL == CMAX_MODEL_VOXEL, "owned groups: flow-gradient models only");
    if (kInside && (int)blockIdx.x < stat_blocks) {  // workgroup-uniform: this workgroup is one of K2's (first thing: nothing else is live)
        __shared__ double s_stat[2 * L::kNW];
        stats_inside_role<L>(ra.img[0], ra.zero[0], wp.Hp, wp.Wp, op, const_cast<double *>(stat), ra, result, s_stat);
        return;
    }
    CMAX_STAMP(1, 0);
    // first thing: this workgroup's segment, the window K1 used for it, the batch period and theta (load_head_words) -- the fourteen
    // leading argument dwords arrive in SGPRs, so none of these loads waits for the argument block and all come back under one wait
    const int sidx = segment_of_block(nseg, kInside ? blockIdx.x - (unsigned)stat_blocks : blockIdx.x);
    if (sidx >= nseg) return;
    const int4 sg = segs[sidx];
    // (mid / big segments, which keep the head they had, also keep its statements and their order: the 512 x 8 kernels sit at their
    // register lines, profiles/head_loads_resources.txt)
    const int zy = (int)(blockIdx.z * (L::kEntryHead ? (unsigned)n_ref_grid : gridDim.y) + blockIdx.y);  // (candidate of cmax_objective_batch, reference time)
    const int4 *known = win_base + (int64_t)zy * nseg + sidx;
    int4 known_win = make_int4(0, 0, 0, 0);
    ev.ev = evp;
    EventLoads<L> el;
    std::conditional_t<L::kEntryHead, WarpHead, NoHead> head;  // (mid / big segments: phase_warp reads period and theta itself)
    float fw[L::kEPT];
    static_assert(!WEIGHTED || (!kDet && !kInside && FOLD != kFoldDeferred), "weighted handles: the general K1 -> statistics -> K3 path");
    int k;
    const float *__restrict__ img;
    int64_t z_img;
    if constexpr (L::kEntryHead) {
        if (MODEL == CMAX_MODEL_2DOF) motion += (int64_t)blockIdx.z * (head_word >> 5);
        else motion += (int64_t)blockIdx.z * ra.z_motion;  // (a flow is first read behind the events)
        known_win = *known;
        known = &known_win;
        const HeadWords headw = load_head_words<MODEL>(motion, tmm, head_flags);
        wp.motion = motion;
        wp.d = ra.d[blockIdx.y];  // blockIdx.y = reference time of this workgroup
        // ... and the words of the argument block that the warp, the window's staging and the wave that writes the loss need: ONE batch of
        // scalar loads, issued before the first wait (as in k_vote) -- the window's pixel loads then follow the segment's wait directly.
        // Only values AS LOADED are pinned: arithmetic on one of them in front of the pin is a use, and the compiler puts a wait there
        // and the loads it has not issued yet behind it.
        const float *const img_y = ra.img[blockIdx.y];
        z_img = ra.z_img;
        const int k0 = ra.k0;
        const int64_t z_raw = ra.z_raw;              // (the address of the raw sums and the image to clear: used in front of the window's
        float *const zero_y = ra.zero[blockIdx.y];  // pixel loads, where they were a scalar wait of their own)
        asm volatile("" ::"s"(sg.x), "s"(sg.y), "s"(known_win.x), "s"(known_win.y), "s"(known_win.z), "s"(known_win.w), CMAX_HEAD_PIN_WORDS(headw), "s"(wp.d), "s"(wp.H),
                     "s"(wp.W), "s"(wp.ph), "s"(wp.pw), "s"(wp.Hp), "s"(wp.Wp), "s"(img_y), "s"(z_img), "s"(op.omit), "s"(k0), "s"(gpart_base), "s"(result), "s"(z_raw),
                     "s"(zero_y));
        k = k0 + (int)blockIdx.y;
        img = img_y + blockIdx.z * z_img;
        issue_event_loads<L, VARIANT == kGradStrided>(evp, cev, sidx, sg, el);
        head = decode_head_words(headw, head_flags);
        if constexpr (WEIGHTED) load_slot_weights<L, VARIANT == kGradStrided>(ra.wgt, sg, fw);
    } else {
        wp.motion += (int64_t)blockIdx.z * ra.z_motion;
        issue_event_loads<L, VARIANT == kGradStrided>(evp, cev, sidx, sg, el);
        if constexpr (WEIGHTED) load_slot_weights<L, VARIANT == kGradStrided>(ra.wgt, sg, fw);
        wp.d = ra.d[blockIdx.y];  // blockIdx.y = reference time of this workgroup
        k = ra.k0 + (int)blockIdx.y;
        z_img = ra.z_img;
        img = ra.img[blockIdx.y] + blockIdx.z * ra.z_img;
    }
    float *__restrict__ zero_img = ra.zero[blockIdx.y] ? ra.zero[blockIdx.y] + blockIdx.z * z_img : nullptr;
    // 2-DoF: the RAW SUMS of reference time k -- kRawLines accumulators, one 128-byte line each, of two doubles (sum dt g) or, with
    // deferred statistics, six (k_finish_lines / k_finish_raw / cmax_finalize_raw_host fold them)
    double *__restrict__ gpart = gpart_base ? gpart_base + blockIdx.z * ra.z_raw + (int64_t)k * kRawStride : nullptr;
    static_assert(FOLD != kFoldDeferred || MODEL == CMAX_MODEL_2DOF, "deferred statistics: 2-DoF only");
    static_assert(!STRIDED || MODEL == CMAX_MODEL_DENSE, "the strided slot layout exists for the dense scan only");
    __shared__ float s_win[L::kWinCap + kScratch];
    __shared__ double s_red[6 * L::kNW];
    // flow-gradient accumulators (x | y) in LDS: voxel only.  Measured on MI355X (cfg3 / cfg5): the dense model is
    // faster with a segmented scan + one global atomic per run (25 vs 34 us) -- its runs are long (16 events per
    // pixel) -- while voxel runs are ~2 events and the accumulators win (cfg4 K3 37 -> 26 us in fixed point)
    constexpr bool kLdsAcc = (MODEL == CMAX_MODEL_VOXEL && !kDet) || kOwned;
    // dense (owned) segments span <= 3 source tiles; voxel ones kAccCells / 256 (tile, bin) groups.  The smaller array keeps
    // four 512-thread workgroups per CU for the dense model (33 KB window + 6 KB instead of + 24 KB)
    // (kGradOwnedSmall: a voxel work list cut into segments of <= 3 (tile, bin) groups, see build_segments)
    static_assert(VARIANT != kGradOwnedSmall || (MODEL == CMAX_MODEL_VOXEL && L::kSlots <= 3072), "small accumulators: voxel, standard / mid segments");
    constexpr int kAcc = (MODEL == CMAX_MODEL_DENSE ? L::kAccDense : (VARIANT == kGradOwnedSmall ? L::kAccSmall : kAccCells));
    __shared__ int s_acc[kLdsAcc ? 2 * kAcc : 1];
    __shared__ float s_max[L::kNW];
    // The loss: all statistics are complete when this kernel starts (K2 ran).  Written by the last wave of the FIRST workgroup
    // -- at the tail of the kernel (the last segment's workgroup, one thread walking the accumulators' cache lines) it cost
    // K3 ~0.5 us with 8 lines per image and 3 us with 32.
    if (!kInside && result && k == 0 && sidx == 0 && threadIdx.x >= L::kThr - kWave) write_result<true>(op, stat, result);
    // Segments of a sparse batch (the solver's 30k events: ~100 events per segment, cut by the 12-group span) skip the
    // LDS accumulators: zeroing and flushing 2 x 3072 cells plus the block-wide scale reduction cost more than the two
    // global atomics per event they save (voxel K3 of the YAML objective, 3 reference times: 21.4 -> see profiles).
    const bool sparse_seg = kLdsAcc && !kOwned && sg.y < kSparseSegment;  // (an owned segment stores all its cells anyway)
    if (kLdsAcc && !sparse_seg) {
        for (int i = threadIdx.x; i < 2 * kAcc; i += L::kThr) s_acc[i] = 0;  // made visible by the barriers of phase_warp
    }
    const int i0 = op.omit ? 1 : 0;
    // What the LDS window holds at an in-image pixel.  The chain factor (kFoldStats / kFoldScale) and the mean (kFoldStats) are
    // NOT applied here: the gather only takes differences inside a 2 x 2 footprint -- the mean cancels wherever the mask
    // 1_Omega is constant -- and the chain factor multiplies the per-event result.  Both come from the image statistics, and a
    // gather of the statistics' cache lines by every wave at the head of the kernel was what K3 waited for (16 waves x 1100
    // workgroups on 8 lines: cfg4's K3 14.6 us with a finished G image, 17.7 us with the same image unscaled); now wave 0
    // fetches them while the events load, and everybody reads them from LDS behind the barrier that follows the window load.
    auto g_at = [&](int r, int c) -> float {
        const float x = img[pix_index(r, c, wp.Wp)];
        if (FOLD == kFoldNone || FOLD == kFoldScale) return x;  // a G image (kFoldScale: stored without its chain factor)
        const bool in = (r >= i0) && (r < wp.Hp - i0) && (c >= i0) && (c < wp.Wp - i0);
        return in ? x : 0.f;  // masked raw image (kFoldStats, kFoldStatsInside, kFoldDeferred)
    };
    // deferred statistics (K2's work, see k_finish_deferred): no pass over the image.  The image is the sum of the events' bilinear
    // votes, so over the region Omega
    //     sum_p I[p]^2 = sum_e sum_{c in corners(e)} w_ec I[c] 1_Omega(c),     sum_p I[p] = sum_e sum_c w_ec 1_Omega(c),
    // and the gather below already holds an event's four (masked) corner values and its fractions: one bilinear interpolation per event.
    __shared__ float s_chain[2];  // chain factor and mean of this reference time
    float c2 = 1.f, mu = 0.f;
    // A normalised cost's chain factor depends on the variances, and kFoldStats needs the mean (for the windows that reach
    // outside Omega): the LAST wave (segments rarely fill their 2048 slots, so it is the one with the fewest events, often
    // none) fetches the statistics ahead of its event loads.  Otherwise the factor is a constant of the objective.
    const bool chain_from_stats = FOLD == kFoldStats || (FOLD == kFoldScale && op.normalized);  // launch-uniform
    if (chain_from_stats && (kDet || threadIdx.x >= L::kThr - kWave)) {
        double mud = 0.0;
        const double coef = chain_coef<true>(op, stat, k, &mud);  // whole converged waves
        c2 = FOLD == kFoldStats ? (float)(coef * 2.0 / (region_pixels(op.H, op.W, op.omit) - 1.0)) : (float)coef;
        mu = (float)mud;
        if (threadIdx.x == L::kThr - 1) {
            s_chain[0] = c2;
            s_chain[1] = mu;
        }
    } else if (kStatsFold || FOLD == kFoldScale) {
        const double coef = (op.negate ? -1.0 : 1.0) * op.mult[k] * (op.minimize ? -1.0 : 1.0);  // chain_coef without the statistics
        c2 = kStatsFold ? (float)(coef * 2.0 / (region_pixels(op.H, op.W, op.omit) - 1.0)) : (float)coef;
    }
    if (kInside && threadIdx.x >= L::kThr - kWave) {  // the mean from K1's vote sums: (events + corrections) / |Omega|
        const int ln = (int)threadIdx.x - (L::kThr - kWave);
        double m = ln < kMuLines ? ra.musum[blockIdx.y][ln * kSubStride] : 0.0;
        m = wave_sum_lane63(m);
        if (threadIdx.x == L::kThr - 1) s_chain[1] = (float)(((double)ra.n_events + m) / region_pixels(op.H, op.W, op.omit));
    }
    // deterministic mode: fixed-point scale of this reference time (2-DoF) / of the whole launch (flow gradient), from
    // bounds that every workgroup evaluates identically: |term| <= |dt|max * 2 max|G|, max|G| from max|image|
    double det_s = 1.0;
    if (kDet) {
        auto term_bound = [&](int kk) -> double {
            double mud = 0.0;
            const double coef = fabs(chain_coef<true>(op, stat, kk, &mud));
            const double imx = (double)__uint_as_float(ra.imax[kk]);
            const double npx = region_pixels(op.H, op.W, op.omit);
            // (a focus loss: coef (2/n) A max|I|, A = sum_s c_s |S_s|_1^2 of its stencils -- 1 mean square, 64 Laplacian, 34 Hessian)
            const double gb = op.cost == CMAX_COST_VARIANCE ? coef * 2.0 / (npx - 1.0) * (imx + fabs(mud))
                                                            : coef * 2.0 * (op.cost == CMAX_COST_LAPLACIAN ? 64.0 : (op.cost == CMAX_COST_HESSIAN ? 34.0 : 1.0)) * imx / npx;
            const double dk = (double)ra.d[kk - ra.k0];
            return 4.0 * fmax(fabs(dk), fabs(1.0 - dk)) * (double)time_scale(wp) * 2.0 * gb;  // x4: fp32 rounding of G and of the term
        };
        double bound = 0.0;
        if (MODEL == CMAX_MODEL_2DOF) bound = term_bound(k);
        else
            for (int kk = 0; kk < op.n_ref; ++kk) bound = fmax(bound, term_bound(kk));
        det_s = det_scale(bound, ra.n_events);
        if (sidx == 0 && threadIdx.x == 0 && (MODEL == CMAX_MODEL_2DOF || k == 0)) ra.det_inv_scale[MODEL == CMAX_MODEL_2DOF ? k : 0] = 1.0 / det_s;
    }
    unsigned rc[L::kEPT];
    float fa[L::kEPT], fb[L::kEPT], fdt[L::kEPT];
    int fsrc[L::kEPT];
    const int lane = threadIdx.x & (kWave - 1);
    // stage dL/dIWE of the window in LDS, zero outside the image (masked vote)
    auto load_window = [&](const Window &w) {
        // (Round 3: batching these loads -- four unconditional loads per thread in flight, selects afterwards -- was measured too.  The
        // compiler does wait for every load of these loops in place, but at 8 waves per SIMD that latency is hidden, and the batched
        // form needs ~40 more SGPRs (validity masks, uniform row counts): above 80, i.e. 7 waves per SIMD.  cfg3 K3 17.6 -> 16.8 us,
        // but cfg2 6.8 -> 7.5, cfg4 14.4 -> 19.6 (one 1024-thread workgroup per CU), cfg5 17.3 -> 18.4: profiles/r03_ablation.txt.)
        // (a second, test-free copy of these loops for windows that lie inside the image was measured: the extra scalar
        // state costs more than the tests -- dense K3 of cfg5 17.3 -> 19.5 us, profiles/r02_ablation.txt)
        // (Round 3: LDS-direct loads -- global_load_lds_dword, a wave per window row, every row of a wave in flight at once, no
        // select and no ds_write -- were measured for windows inside the image: cfg3 K3 17.65 -> 17.1 us, but cfg2 6.8 -> 7.3, cfg4
        // 14.3 -> 15.5, cfg5 17.05 -> 18.1, hbm 174 -> 180: profiles/r03_ablation.txt.)
        auto g_win = [&](int r, int c) -> float {
            const int R = w.r0 + r, C = w.c0 + c;
            return ((unsigned)R < (unsigned)wp.Hp && (unsigned)C < (unsigned)wp.Wp) ? g_at(R, C) : 0.f;
        };
        // Dense / voxel: FLAT walk over the window's LDS words (row pitch = stride; the padding column is written as 0): consecutive
        // lanes write consecutive words and every iteration uses all 64 lanes -- the wave-per-row form below runs a 68-cell row as
        // 64 + 4 lanes.  row = i / stride through one v_mul_hi_u32 (exact: i < 2^13, stride < 2^8).  Measured (profiles/r03_ablation.txt
        // 13): K3 of cfg3 17.6 -> 17.15 us, cfg4 12.75 -> 12.4, cfg5 shard 17.0 -> 16.4, 20M events 52.1 -> 49.7, 64M 156 -> 151;
        // the 2-DoF K3 (cfg2: narrow windows, a third of the cells) keeps the row form (6.8 vs 6.9 us).  The same walk with four loads
        // per thread in flight (unconditional at a clamped pixel, pin(), selects) was slower again: cfg3 18.7, 20M events 61.
        if (MODEL != CMAX_MODEL_2DOF) {
            const unsigned ustride = (unsigned)w.stride, magic = ((1u << 21) + ustride - 1u) / ustride;  // (see K1's flat flush)
            const int wn = w.h * w.stride;
            // Round 6 (big segments): a window whose rows -- padding column included -- lie inside the image and inside Omega needs no test and no
            // mask per word (workgroup-uniform; most windows): word i = r stride + c is pixel [r0 Wp + c0] + r (Wp - stride) + i, four VALU
            // instructions per word where the tested form has ~20 -- at nine words per thread a fifth of this kernel's VALU instructions.
            // (The padding column then holds the pixel right of the window instead of 0: no footprint reads it.)
            if (L::kBig && w.r0 >= i0 && w.c0 >= i0 && w.r0 + w.h <= wp.Hp - i0 && w.c0 + w.stride <= wp.Wp - i0) {
                const float *__restrict__ base = img + pix_index(w.r0, w.c0, wp.Wp);
                const unsigned pitch_diff = (unsigned)wp.Wp - ustride;
                for (int i = threadIdx.x; i < wn; i += L::kThr) {
                    const unsigned r = mul24_u((unsigned)i, magic) >> 21;
                    s_win[i] = base[mad24_u(r, pitch_diff, (unsigned)i)];
                }
            } else {
                for (int i = threadIdx.x; i < wn; i += L::kThr) {
                    const unsigned r = mul24_u((unsigned)i, magic) >> 21, c = (unsigned)i - mul24_u(r, ustride);
                    s_win[i] = (int)c < w.w ? g_win((int)r, (int)c) : 0.f;
                }
            }
        } else if (w.w > 32) {  // a wave per window row: coalesced, no integer division
            for (int r = threadIdx.x / kWave; r < w.h; r += L::kNW)
                for (int c = lane; c < w.w; c += kWave) s_win[r * w.stride + c] = g_win(r, c);
        } else {  // narrow window: two rows per wave
            const int half = lane >> 5, c = lane & 31;
            for (int r = 2 * (threadIdx.x / kWave) + half; r < w.h; r += 2 * L::kNW)
                if (c < w.w) s_win[r * w.stride + c] = g_win(r, c);
        }
    };
    // the window K1 used for this segment, and the cell offsets of the events K1 decided in fp64 (the host runs K1 first, always)
    const unsigned *__restrict__ shifts = ra.shifts + ((int64_t)zy * nseg + sidx) * L::kShiftWords;
    bool live;  // this wave holds events (wave-uniform)
    unsigned nib_unused;
    const Window win = phase_warp<L, MODEL, FRAC, true, STRIDED, true>(ev, wp, sg, el, rc, fa, fb, fdt, fsrc, nullptr, known, shifts, load_window, live, nib_unused, head);
    CMAX_STAMP_AFTER(1, 1, rc[L::kEPT - 1]);
    if (threadIdx.x < kScratch) s_win[L::kWinCap + threadIdx.x] = 0.f;  // empty slots / masked corners read 0 from here
    __syncthreads();
    CMAX_STAMP(1, 2);
    // per event: dt <- c2 dt (every sum below is linear in dt), and -- kFoldStats, windows that reach outside Omega only -- the mean's
    // share mu * bilinear-difference(1_Omega) of the gathered difference (zero wherever the four corners lie on one side of the mask)
    bool edge_mu = false;
    if constexpr (WEIGHTED) {
#pragma unroll
        for (int j = 0; j < L::kEPT; ++j) fdt[j] *= fw[j];
    }
    if (kStatsFold || FOLD == kFoldScale) {
        if (chain_from_stats && !kDet) {
            c2 = s_chain[0];
            mu = s_chain[1];
        }
        if (kInside) mu = s_chain[1];
#pragma unroll
        for (int j = 0; j < L::kEPT; ++j) fdt[j] *= c2;
    }
    if (kStatsFold)  // workgroup-uniform
        edge_mu = win.clipped || win.r0 < i0 || win.r0 + win.h > wp.Hp - i0 || win.c0 < i0 || win.c0 + win.w > wp.Wp - i0;
    const int hw = wp.H * wp.W;
    const int dummy = L::kDummy + lane;
    const int stride = win.stride;
    unsigned neg_origin = 0u - ((unsigned)(win.r0 + 16384) * (unsigned)win.stride + (unsigned)(win.c0 + 16384));
    asm volatile("" : "+v"(neg_origin));  // (a VGPR: see fast_index)
    const unsigned scratch = L::kWinCap + lane;
    // per event: dL/dx' = (1-b)(G10-G00) + b(G11-G01), dL/dy' = (1-a)(G01-G00) + a(G11-G10)
    // (deferred statistics: also g_bil = the masked image interpolated at the event, sum_c w_ec I[c] 1_Omega(c), for sum I^2)
    float g_bil = 0.f;
    auto gather = [&](int j, float &gx, float &gy) {
        // g[0] = G00 (row, col), g[1] = G10 (row+1, col), g[2] = G01 (row, col+1), g[3] = G11
        float g[4];
        if (!win.clipped) {  // fast window: the footprint is inside by construction
            const int idx = fast_index(rc[j], neg_origin, win.stride, scratch);
            g[0] = s_win[idx];
            g[2] = s_win[idx + 1];
            g[1] = s_win[idx + stride];
            g[3] = s_win[idx + stride + 1];
        } else {  // workgroup-uniform, rare: a corner outside the window reads the zero scratch word, or global memory if it is inside the image
            const int row = (int)(rc[j] >> 16) - 16384, col = (int)(rc[j] & 0xFFFFu) - 16384;  // empty slot: far outside
            const int lr = row - win.r0, lc = col - win.c0;
            const bool r_in0 = (unsigned)lr < (unsigned)win.h, r_in1 = (unsigned)(lr + 1) < (unsigned)win.h;
            const bool c_in0 = (unsigned)lc < (unsigned)win.w, c_in1 = (unsigned)(lc + 1) < (unsigned)win.w;
            const int base = lr * win.stride + lc;
            g[0] = s_win[(r_in0 && c_in0) ? base : dummy];
            g[1] = s_win[(r_in1 && c_in0) ? base + stride : dummy];
            g[2] = s_win[(r_in0 && c_in1) ? base + 1 : dummy];
            g[3] = s_win[(r_in1 && c_in1) ? base + stride + 1 : dummy];
            if (rc[j] != 0u) {
#pragma unroll 1
                for (int q = 0; q < 4; ++q) {  // rolled: ONE copy of the global fetch per slot -- this path is rare and slow anyway, and unrolled it cost the
                                               // kernels that never take it ~1 % (profiles/r03_ablation.txt 24, 25)
                    const int r = row + (q & 1), c = col + (q >> 1);
                    const bool in_win = (unsigned)(r - win.r0) < (unsigned)win.h && (unsigned)(c - win.c0) < (unsigned)win.w;
                    if (!in_win && (unsigned)r < (unsigned)wp.Hp && (unsigned)c < (unsigned)wp.Wp) {
                        const float v = g_at(r, c);
                        g[0] = q == 0 ? v : g[0];
                        g[1] = q == 1 ? v : g[1];
                        g[2] = q == 2 ? v : g[2];
                        g[3] = q == 3 ? v : g[3];
                    }
                }
            }
        }
        const float a = fa[j], b = fb[j];
        gx = (1.f - b) * (g[1] - g[0]) + b * (g[3] - g[2]);
        gy = (1.f - a) * (g[2] - g[0]) + a * (g[3] - g[1]);
        if (FOLD == kFoldDeferred) {  // (1-b)((1-a) G00 + a G10) + b((1-a) G01 + a G11) on the row differences gx already has
            const float t0 = fmaf(a, g[1] - g[0], g[0]), t1 = fmaf(a, g[3] - g[2], g[2]);
            g_bil = fmaf(b, t1 - t0, t0);
        }
        if (kStatsFold && edge_mu) {  // workgroup-uniform: the mean's share mu * bilinear-difference(1_Omega) (nothing is kept per event:
            // two more registers per slot put the 512-thread owned kernel at 66 VGPRs, i.e. 7 waves per SIMD instead of 8)
            const int hi = wp.Hp - 2 * i0, wi = wp.Wp - 2 * i0;
            const int row = (int)(rc[j] >> 16) - 16384, col = (int)(rc[j] & 0xFFFFu) - 16384;  // empty slot: far outside, all masks 0
            const float mr0 = (unsigned)(row - i0) < (unsigned)hi ? 1.f : 0.f, mr1 = (unsigned)(row + 1 - i0) < (unsigned)hi ? 1.f : 0.f;
            const float mc0 = (unsigned)(col - i0) < (unsigned)wi ? 1.f : 0.f, mc1 = (unsigned)(col + 1 - i0) < (unsigned)wi ? 1.f : 0.f;
            gx -= mu * (mr1 - mr0) * ((1.f - b) * mc0 + b * mc1);
            gy -= mu * (mc1 - mc0) * ((1.f - a) * mr0 + a * mr1);
        }
    };
    // decode a run key (source pixel, time bin) into its flow-gradient element
    auto flow_index = [&](unsigned key) -> int64_t {
        const int ix = (int)(key & 0xFFFu), iy = (int)((key >> 12) & 0xFFFu), bin = (int)(key >> 24);
        return (MODEL == CMAX_MODEL_VOXEL ? (int64_t)bin * 2 * hw : (int64_t)0) + pix_index(ix, iy, wp.W);
    };
    // accumulator cell: [group - first group of the segment][pixel in tile], group = tile * T + bin (the sort
    // order of a binned handle, see resort_key)
    // Dense flows (owned segments: whole tiles of ONE tile row, sg.w of them from tile column tcol0 on) keep their cells as the 16 pixel
    // rows of that strip, [row in tile][column - 16 tcol0], row pitch 16 sg.w: four instructions per event instead of eight, and the
    // flush writes whole rows of the strip.
    const int Tg = MODEL == CMAX_MODEL_VOXEL ? wp.T : 1;  // groups per source tile
    const int strip_tile0 = sg.z / Tg, strip_trow = strip_tile0 / wp.ntc, strip_tcol0 = strip_tile0 - strip_trow * wp.ntc;  // (workgroup-uniform)
    const unsigned strip_w = (unsigned)sg.w << 4, strip_y0 = (unsigned)strip_tcol0 << 4;
    auto acc_cell = [&](unsigned key) -> int {
        if (MODEL == CMAX_MODEL_DENSE) return (int)(mad24_u(key & 15u, strip_w, (key >> 12) & 0xFFFu) - strip_y0);
        const int ix = (int)(key & 0xFFFu), iy = (int)((key >> 12) & 0xFFFu), bin = (int)(key >> 24);
        const unsigned tile = __umul24((unsigned)(ix >> 4), (unsigned)wp.ntc & 0xFFFFFFu) + (unsigned)(iy >> 4);  // (the mask lets the
        const int group = MODEL == CMAX_MODEL_VOXEL ? (int)__umul24(tile, (unsigned)Tg & 0xFFFFFFu) + bin : (int)tile;  // compiler keep the 24-bit multiply)
        return ((group - sg.z) << 8) + ((ix & 15) << 4) + (iy & 15);
    };
    float accx = 0.f, accy = 0.f, s2x = 0.f, s2y = 0.f;
    float sum_i = 0.f, sum_ii = 0.f;  // deferred statistics: this thread's share of sum I and sum I^2 over Omega (see above)
    if (kDet) {
        __shared__ long long s_acc64[2];
        if (MODEL == CMAX_MODEL_2DOF) {
            if (threadIdx.x < 2) s_acc64[threadIdx.x] = 0;
            __syncthreads();
        }
        long long ax64 = 0, ay64 = 0;
        if (live) {
            // flow gradient: the events of a thread are consecutive in the sort order, i.e. mostly of ONE source pixel (cell of the
            // gradient) -- their integer terms are summed in registers and leave with one pair of 64-bit atomics per run instead
            // of per event.  Integer addition is exact and associative: any grouping gives the same bits (round 3; cfg3 423 us with
            // one pair per event).
            unsigned kcur = 0xFFFFFFFFu;
#pragma unroll
            for (int j = 0; j < L::kEPT; ++j) {
                float gx, gy;
                gather(j, gx, gy);
                const float sgn = MODEL == CMAX_MODEL_2DOF ? 1.f : -1.f;
                // the product is rounded to fp32 once (a deterministic function of the event), then becomes an integer
                const long long qx = det_fixed((double)(sgn * fdt[j] * gx), det_s), qy = det_fixed((double)(sgn * fdt[j] * gy), det_s);
                if (MODEL == CMAX_MODEL_2DOF) {
                    ax64 += qx;
                    ay64 += qy;
                } else if (rc[j] != 0u) {
                    const unsigned key = (unsigned)fsrc[j];
                    if (key != kcur) {
                        if (kcur != 0xFFFFFFFFu) {
                            const int64_t g = flow_index(kcur);
                            atomic_add_i64(&ra.g64[g], ax64);
                            atomic_add_i64(&ra.g64[g + hw], ay64);
                        }
                        kcur = key;
                        ax64 = 0;
                        ay64 = 0;
                    }
                    ax64 += qx;
                    ay64 += qy;
                }
            }
            if (MODEL != CMAX_MODEL_2DOF && kcur != 0xFFFFFFFFu) {
                const int64_t g = flow_index(kcur);
                atomic_add_i64(&ra.g64[g], ax64);
                atomic_add_i64(&ra.g64[g + hw], ay64);
            }
        }
        if (MODEL == CMAX_MODEL_2DOF) {
            if (live) {
                atomic_add_i64(&s_acc64[0], ax64);  // 64-bit LDS integer atomics: exact in any order
                atomic_add_i64(&s_acc64[1], ay64);
            }
            __syncthreads();
            if (threadIdx.x < 2) ra.g64[((int64_t)k * nseg + sidx) * 2 + threadIdx.x] = s_acc64[threadIdx.x];
        }
        return;
    }
    if (MODEL == CMAX_MODEL_2DOF) {
        if (live) {
#pragma unroll
        for (int j = 0; j < L::kEPT; ++j) {
            float gx, gy;
            gather(j, gx, gy);
            accx = fmaf(fdt[j], gx, accx);  // dt = 0 for an empty slot; <= kEPT terms in fp32, then fp64 across the workgroup
            accy = fmaf(fdt[j], gy, accy);
            if (FOLD == kFoldDeferred) sum_ii += g_bil;  // an empty slot gathers zeros; <= kEPT terms in fp32, as above
        }
        if (FOLD == kFoldDeferred) {
            // the mean enters only where a footprint straddles the edge of the region Omega the variance is taken
            // over: with m = 1_Omega, S2 = sum dt * bilinear-difference(m), and an event's share of sum I is the
            // bilinear interpolation of m (the mask is a rectangle: a product of a row and a column factor).
            // Workgroup-uniform test: most windows lie inside Omega, where S2 is exactly 0 and every event counts 1
            // (K1's four integer weights add up to K exactly), and skip this.
            const int hi = wp.Hp - 2 * i0, wi = wp.Wp - 2 * i0;
            const bool edge = win.clipped || win.r0 < i0 || win.r0 + win.h > wp.Hp - i0 || win.c0 < i0 || win.c0 + win.w > wp.Wp - i0;
            if (edge) {
#pragma unroll
                for (int j = 0; j < L::kEPT; ++j) {
                    const int row = (int)(rc[j] >> 16) - 16384, col = (int)(rc[j] & 0xFFFFu) - 16384;  // empty slot: far outside, all masks 0
                    const float mr0 = (unsigned)(row - i0) < (unsigned)hi ? 1.f : 0.f, mr1 = (unsigned)(row + 1 - i0) < (unsigned)hi ? 1.f : 0.f;
                    const float mc0 = (unsigned)(col - i0) < (unsigned)wi ? 1.f : 0.f, mc1 = (unsigned)(col + 1 - i0) < (unsigned)wi ? 1.f : 0.f;
                    const float a = fa[j], b = fb[j];
                    const float wr = (1.f - a) * mr0 + a * mr1, wc = (1.f - b) * mc0 + b * mc1;
                    s2x = fmaf(fdt[j], (mr1 - mr0) * wc, s2x);
                    s2y = fmaf(fdt[j], (mc1 - mc0) * wr, s2y);
                    sum_i = fmaf(wr, wc, sum_i);
                }
            } else {
#pragma unroll
                for (int j = 0; j < L::kEPT; ++j) sum_i += rc[j] != 0u ? 1.f : 0.f;
            }
        }
        }  // live
    } else if (!kLdsAcc) {
        // Dense: sum -dt*g over runs of equal source pixel (the events are pixel-sorted) and issue one global atomic
        // per run and channel.  A thread reduces a CHUNK of consecutive slots serially in registers (runs that begin
        // and end inside the chunk are emitted on the spot), then ONE head-flag segmented scan over the wave joins the
        // trailing run of a lane with the lanes that continue it.
        //   long runs  (consecutive layout): chunk = all kEPT slots of the thread -> one scan per thread;
        //   short runs (strided layout)    : chunks = the slot pairs (2j, 2j+1), for which neighbouring lanes hold
        //                                    neighbouring events -> their atomics fall on neighbouring pixels.
        constexpr unsigned kNoKey = 0xFF000000u;  // empty slot: never equal to a real key (dense keys have bin 0)
        auto emit = [&](unsigned key, float sx, float sy) {
            if (key >= kNoKey) return;
            const int64_t g = flow_index(key);
            atomic_add(&gflow[g], sx);
            atomic_add(&gflow[g + hw], sy);
        };
        auto reduce_chunk = [&](int base, auto chunk) {
            constexpr int kChunk = decltype(chunk)::value;
            float gx, gy;
            gather(base, gx, gy);
            const unsigned k_first = rc[base] != 0u ? (unsigned)fsrc[base] : kNoKey;
            unsigned kcur = k_first;
            float ax = -fdt[base] * gx, ay = -fdt[base] * gy;  // sum of the current run
            float lx = 0.f, ly = 0.f;                          // sum of the leading run once it is complete
            bool uniform = true;                               // all slots so far share k_first
#pragma unroll
            for (int j = base + 1; j < base + kChunk; ++j) {
                gather(j, gx, gy);
                const unsigned key = rc[j] != 0u ? (unsigned)fsrc[j] : kNoKey;
                const float vx = -fdt[j] * gx, vy = -fdt[j] * gy;
                if (key == kcur) {
                    ax += vx;
                    ay += vy;
                } else {
                    if (uniform) {  // the leading run ends here; it may continue a run of the previous lane
                        lx = ax;
                        ly = ay;
                        uniform = false;
                    } else {
                        emit(kcur, ax, ay);  // a run that begins and ends inside this chunk
                    }
                    kcur = key;
                    ax = vx;
                    ay = vy;
                }
            }
            // cross-lane: (ax, ay) = trailing run of this lane's chunk (the whole chunk if uniform)
            const unsigned kprev_last = (unsigned)dpp_i<kDppWaveShr1>((int)~k_first, (int)kcur);  // lane 0 sees ~k_first: no predecessor
            const bool joins = kprev_last == k_first && k_first < kNoKey;
            const int head = (uniform && joins) ? 0 : 1;
            const unsigned knext_first = (unsigned)dpp_i<kDppWaveShl1>((int)~kcur, (int)k_first);  // lane 63 sees ~kcur: always a tail
            seg_scan64(head, ax, ay, lane);
            // what the previous lane passes on: its inclusive value
            const float cx = dpp_f<kDppWaveShr1>(ax), cy = dpp_f<kDppWaveShr1>(ay);
            if (!uniform) emit(k_first, lx + (joins ? cx : 0.f), ly + (joins ? cy : 0.f));
            if (knext_first != kcur) emit(kcur, ax, ay);
        };
        if (!live) {
            // a wave without events has no run to reduce
        } else if (STRIDED) {
#pragma unroll
            for (int j = 0; j < L::kEPT; j += 2) reduce_chunk(j, std::integral_constant<int, 2>{});
        } else {
            reduce_chunk(0, std::integral_constant<int, L::kEPT>{});
        }
    } else {
        // LDS accumulators in block-scaled fixed point.  ds_add_f32 runs at 1/12 of the ds_add_u32 rate on gfx950
        // (profiles/r01_microbench.txt) and voxel runs are ~2 events long, so every event adds its two terms as
        // integers: scale = 2^(19 - e) with 2^e > max |term| of the workgroup; <= kSegMax terms per cell stay
        // below 2^30.  Rounding: 2^-20 of the workgroup's largest term per addition.
        float vx[L::kEPT], vy[L::kEPT], vmax = 0.f;
#pragma unroll
        for (int j = 0; j < L::kEPT; ++j) {
            float gx = 0.f, gy = 0.f;
            if (live) gather(j, gx, gy);
            vx[j] = -fdt[j] * gx;
            vy[j] = -fdt[j] * gy;
            vmax = fmaxf(vmax, fmaxf(fabsf(vx[j]), fabsf(vy[j])));
        }
        if (sparse_seg) {  // workgroup-uniform
#pragma unroll
            for (int j = 0; j < L::kEPT; ++j) {
                if (rc[j] == 0u) continue;
                const int64_t g = flow_index((unsigned)fsrc[j]);
                atomic_add(&gflow[g], vx[j]);
                atomic_add(&gflow[g + hw], vy[j]);
            }
                return;
        }
#define CMAX_MAX_STEP(CTRL) vmax = fmaxf(vmax, dpp_f<CTRL>(vmax));
        CMAX_MAX_STEP(kDppRowShr1)
        CMAX_MAX_STEP(kDppRowShr2)
        CMAX_MAX_STEP(kDppRowShr4)
        CMAX_MAX_STEP(kDppRowShr8)
        CMAX_MAX_STEP(kDppRowBcast15)
        CMAX_MAX_STEP(kDppRowBcast31)
#undef CMAX_MAX_STEP
        if (lane == kWave - 1) s_max[threadIdx.x / kWave] = vmax;
        __syncthreads();
        vmax = s_max[0];
#pragma unroll
        for (int wv = 1; wv < L::kNW; ++wv) vmax = fmaxf(vmax, s_max[wv]);
        int e = 0;
        (void)frexpf(vmax, &e);  // vmax = f * 2^e, f in [0.5, 1)
        const float scale = ldexpf(1.f, L::kAccExp - e), inv_scale = ldexpf(1.f, e - L::kAccExp);
        if (kOwned) {
            // events ordered by pixel (dense: inside the tile; voxel: inside the (tile, bin) group), consecutive ones per
            // thread: equal cells are summed in registers first (exact in fixed point) -- fewer LDS atomics and no
            // same-address serialisation inside a lane's run
            if (live && vmax > 0.f && vmax < 3.0e38f) {
                int cur = -1, sx = 0, sy = 0;
#pragma unroll
                for (int j = 0; j < L::kEPT; ++j) {
                    const int cell = rc[j] != 0u ? acc_cell((unsigned)fsrc[j]) : -1;
                    const int qx = cvt_rpi(vx[j] * scale), qy = cvt_rpi(vy[j] * scale);  // 0 for an empty slot (dt = 0)
                    if (cell != cur) {
                        if (cur >= 0) {
                            atomicAdd(&s_acc[cur], sx);
                            atomicAdd(&s_acc[kAcc + cur], sy);
                        }
                        cur = cell;
                        sx = qx;
                        sy = qy;
                    } else {
                        sx += qx;
                        sy += qy;
                    }
                }
                if (cur >= 0) {
                    atomicAdd(&s_acc[cur], sx);
                    atomicAdd(&s_acc[kAcc + cur], sy);
                }
            }
        } else if (vmax > 0.f && vmax < 3.0e38f) {
#pragma unroll
            for (int j = 0; j < L::kEPT; ++j) {
                if (rc[j] == 0u) continue;
                const unsigned key = (unsigned)fsrc[j];
                const int cell = acc_cell(key);
                if (kOwned || (unsigned)cell < (unsigned)kAcc) {  // owned: the host keeps a segment inside kAcc
                    atomicAdd(&s_acc[cell], cvt_rpi(vx[j] * scale));
                    atomicAdd(&s_acc[kAcc + cell], cvt_rpi(vy[j] * scale));
                } else {  // accumulator too small for this segment (very many time bins): straight to memory
                    const int64_t g = flow_index(key);
                    atomic_add(&gflow[g], vx[j]);
                    atomic_add(&gflow[g + hw], vy[j]);
                }
            }
        }
        // flush: 64 lanes = 4 rows x 16 pixels of one source tile -> one global atomic per non-zero cell; owned groups:
        // one plain store per cell (this segment is the only writer of its groups' pixels, zeros included)
        CMAX_STAMP(1, 3);
        __syncthreads();
        CMAX_STAMP(1, 4);
        int ncell = sg.w << 8;
        if (ncell > kAcc) ncell = kAcc;
        // A segment's groups are consecutive groups of ONE tile row: its first group is decoded once (workgroup-uniform integer
        // divisions), a cell then needs a shift and -- voxel -- one multiply by the magic reciprocal of T.  (Three integer
        // divisions by run-time values PER CELL were ~120 VALU instructions each time: a quarter of the owned dense K3's budget.)
        const int tile0 = strip_tile0, bin0 = sg.z - tile0 * Tg;
        const int trow = strip_trow, tcol0 = strip_tcol0;
        const unsigned magic = ((1u << 20) + (unsigned)Tg - 1u) / (unsigned)Tg;  // (b * magic) >> 20 = b / T for b < 2^12, T < 2^8
        const unsigned strip_magic = ((1u << 20) + strip_w - 1u) / (strip_w > 0u ? strip_w : 1u);  // cell / strip_w for cell < 2^11, strip_w <= 96
        for (int cell = threadIdx.x; cell < ncell; cell += L::kThr) {
            const int ax = s_acc[cell], ay = s_acc[kAcc + cell];
            if (!kOwned && ax == 0 && ay == 0) continue;
            int tcol = tcol0 + (cell >> 8), bin = 0;
            if (MODEL == CMAX_MODEL_VOXEL) {
                const unsigned b = (unsigned)(bin0 + (cell >> 8)), q = __umul24(b, magic) >> 20;
                tcol = tcol0 + (int)q;
                bin = (int)(b - __umul24(q, (unsigned)Tg));
            }
            int ix = (trow << 4) + ((cell >> 4) & 15), iy = (tcol << 4) + (cell & 15);
            if (MODEL == CMAX_MODEL_DENSE) {  // strip layout (acc_cell)
                const unsigned lr = mul24_u((unsigned)cell, strip_magic) >> 20;
                ix = (trow << 4) + (int)lr;
                iy = (int)(strip_y0 + (unsigned)cell - mul24_u(lr, strip_w));
            }
            const int64_t g = (MODEL == CMAX_MODEL_VOXEL ? (int64_t)bin * 2 * hw : (int64_t)0) + pix_index(ix, iy, wp.W);
            if (kOwned) {
                if (ix < wp.H && iy < wp.W) {  // tiles on the last tile row / column reach past the sensor
                    gflow[g] = (float)ax * inv_scale;
                    gflow[g + hw] = (float)ay * inv_scale;
                }
            } else {
                atomic_add(&gflow[g], (float)ax * inv_scale);
                atomic_add(&gflow[g + hw], (float)ay * inv_scale);
            }
        }
    }
    CMAX_STAMP(1, 5);
    if (MODEL == CMAX_MODEL_2DOF && FOLD != kFoldDeferred) {  // fp32 over the wave, fp64 across waves (see the deferred tail)
        float *s_f = reinterpret_cast<float *>(s_red);
        float w2[2] = {accx, accy};
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            float v = w2[q];
            v += dpp_f<kDppRowShr1>(v);
            v += dpp_f<kDppRowShr2>(v);
            v += dpp_f<kDppRowShr4>(v);
            v += dpp_f<kDppRowShr8>(v);
            v += dpp_f<kDppRowBcast15>(v);
            v += dpp_f<kDppRowBcast31>(v);
            if (lane == kWave - 1) s_f[q * L::kNW + threadIdx.x / kWave] = v;
        }
        __syncthreads();
        if (threadIdx.x < 2) {  // two fp64 atomics per workgroup into accumulator line (segment mod kRawLines), as in the deferred tail
            double a = 0.0;
            for (int w = 0; w < L::kNW; ++w) a += (double)s_f[threadIdx.x * L::kNW + w];
            atomic_add(&gpart[(sidx & (kRawLines - 1)) * kSubStride + threadIdx.x], a);
        }
    }
    if (FOLD == kFoldDeferred) {
        // Workgroup sums.  A block_sum of six doubles (36 dependent v_add_f64 behind 72 DPP moves per wave, two
        // barriers) cost 2 of this kernel's 8.7 us.  All six sums are reduced over the wave in fp32 -- each of their
        // <= 512 terms already carries fp32 rounding, a 6-level tree adds less than the terms bring (sum I inside
        // Omega is a count below 2^24: exact) -- and in fp64 across waves and workgroups.
        float *s_f = reinterpret_cast<float *>(s_red);  // [6][kNW] floats
        float w6[6] = {accx, accy, s2x, s2y, sum_i, sum_ii};
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            float v = w6[q];
            v += dpp_f<kDppRowShr1>(v);
            v += dpp_f<kDppRowShr2>(v);
            v += dpp_f<kDppRowShr4>(v);
            v += dpp_f<kDppRowShr8>(v);
            v += dpp_f<kDppRowBcast15>(v);
            v += dpp_f<kDppRowBcast31>(v);
            if (lane == kWave - 1) s_f[q * L::kNW + threadIdx.x / kWave] = v;
        }
        if (FOLD == kFoldDeferred && zero_img) {
            // Issued here, behind the event and window loads (vmcnt retires in issue order: stores issued first sit
            // on the critical path of every load behind them).
            // This workgroup's slice of the next evaluation's vote image is cleared with WRITE-THROUGH stores (sc1): a
            // plain store leaves the line in this XCD's L2, and the device-scope atomics of the next K1 then pay for
            // getting it out again (K1 in the pipeline 8.2 us vs 6.1 us back to back; with sc1 zeroing 7.6).
            const int npix = wp.Hp * wp.Wp;
            if ((npix & 3) == 0 && (reinterpret_cast<uintptr_t>(zero_img) & 15u) == 0) {
                const int n4 = npix >> 2, chunk4 = ra.zero_chunk4;  // (from the host: the division was ~80 scalar instructions in every wave)
                const int q1 = min(n4, (sidx + 1) * chunk4);
                for (int q = sidx * chunk4 + (int)threadIdx.x; q < q1; q += L::kThr) store_zero4_sc1(zero_img + 4 * (int64_t)q);
            } else {
                const int chunk = ra.zero_chunk, p1 = min(npix, (sidx + 1) * chunk);
                for (int p = sidx * chunk + (int)threadIdx.x; p < p1; p += L::kThr)
                    __hip_atomic_store(&zero_img[p], 0.f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __syncthreads();
        // Six fp64 atomics per workgroup into accumulator line (segment mod kRawLines): no per-segment partials, no ticket, no
        // fence -- whoever consumes the evaluation folds kRawLines x 6 doubles (k_finish_raw: one wave; cmax_finalize_raw_host:
        // the host, behind the copy it makes anyway).  ~22 workgroups share a line over the whole duration of the kernel.
        CMAX_STAMP(1, 6);
        if (threadIdx.x < 6) {
            double a = 0.0;
            for (int w = 0; w < L::kNW; ++w) a += (double)s_f[threadIdx.x * L::kNW + w];
            atomic_add(&gpart[(sidx & (kRawLines - 1)) * kSubStride + threadIdx.x], a);
        }
        return;
    }
}

// ---------------------------------------------------------------------------------------------
// K3w: dL/dw per event (cmax_objective_weight_grad), one workgroup per segment -- K3's segment, window and published-offset
//     machinery (the window K1 used, the cells K1 decided), consecutive slots, a FINISHED G = dL/dIWE image per reference time:
//        dL/dw_e = (1-a)(1-b) G00 + a(1-b) G10 + (1-a) b G01 + a b G11
//     NOT multiplied by w (an event of weight 0 has a derivative).  Slot l of the segment stores gw[plane y][first + l] -- the index
//     load_slot_weights reads a weight from -- coalesced, no atomics; empty slots store nothing (their index belongs to a neighbouring
//     segment; the host clears the planes).  MODEL = -1: the un-warped events against dL/dI_orig (normalised costs).
//     A kernel of its own rather than one more flag of k_grad: no existing instantiation changes (profiles/weight_grad_resources.txt).
// ---------------------------------------------------------------------------------------------
template <class L, int MODEL, bool FRAC>
__global__ void __launch_bounds__(L::kThr)
k_weight_gather(const int4 *__restrict__ segs, int nseg, const uint2 *__restrict__ evp, const char *__restrict__ cev, const int4 *__restrict__ win_base, EvView ev,
                WarpParams wp, RefArgs ra, float *__restrict__ gw, int64_t plane) {
    const int sidx = segment_of_block(nseg);
    if (sidx >= nseg) return;
    const int4 sg = segs[sidx];
    const int4 *known = win_base + (int64_t)blockIdx.y * nseg + sidx;
    ev.ev = evp;
    EventLoads<L> el;
    issue_event_loads<L, false>(evp, cev, sidx, sg, el);
    wp.d = ra.d[blockIdx.y];  // blockIdx.y = reference time of this workgroup
    const float *__restrict__ img = ra.img[blockIdx.y];
    __shared__ float s_win[L::kWinCap + kScratch];
    unsigned rc[L::kEPT];
    float fa[L::kEPT], fb[L::kEPT], fdt[L::kEPT];
    int fsrc[L::kEPT];
    const int lane = threadIdx.x & (kWave - 1);
    auto g_at = [&](int r, int c) -> float { return img[pix_index(r, c, wp.Wp)]; };
    auto load_window = [&](const Window &w) {  // G of the window, zero outside the image (flat walk, see k_grad)
        const unsigned ustride = (unsigned)w.stride, magic = ((1u << 21) + ustride - 1u) / ustride;
        const int wn = w.h * w.stride;
        for (int i = threadIdx.x; i < wn; i += L::kThr) {
            const unsigned r = mul24_u((unsigned)i, magic) >> 21, c = (unsigned)i - mul24_u(r, ustride);
            const int R = w.r0 + (int)r, C = w.c0 + (int)c;
            s_win[i] = ((int)c < w.w && (unsigned)R < (unsigned)wp.Hp && (unsigned)C < (unsigned)wp.Wp) ? g_at(R, C) : 0.f;
        }
    };
    const unsigned *__restrict__ shifts = ra.shifts + ((int64_t)blockIdx.y * nseg + sidx) * L::kShiftWords;
    bool live;
    unsigned nib_unused;
    const Window win = phase_warp<L, MODEL, FRAC, true, false, true>(ev, wp, sg, el, rc, fa, fb, fdt, fsrc, nullptr, known, shifts, load_window, live, nib_unused);
    if (threadIdx.x < kScratch) s_win[L::kWinCap + threadIdx.x] = 0.f;  // empty slots / masked corners read 0 from here
    __syncthreads();
    if (!live) return;  // (wave-uniform, behind the last barrier)
    const int dummy = L::kDummy + lane;
    const int stride = win.stride;
    unsigned neg_origin = 0u - ((unsigned)(win.r0 + 16384) * (unsigned)win.stride + (unsigned)(win.c0 + 16384));
    asm volatile("" : "+v"(neg_origin));  // (a VGPR: see fast_index)
    const unsigned scratch = L::kWinCap + lane;
    const int odd = sg.x & 1;
    float *__restrict__ out = gw + (int64_t)blockIdx.y * plane + ((int64_t)sg.x - odd);
#pragma unroll
    for (int j = 0; j < L::kEPT; ++j) {
        float g[4];  // g[0] = G00 (row, col), g[1] = G10 (row+1, col), g[2] = G01 (row, col+1), g[3] = G11
        if (!win.clipped) {  // fast window: the footprint is inside by construction
            const int idx = fast_index(rc[j], neg_origin, win.stride, scratch);
            g[0] = s_win[idx];
            g[2] = s_win[idx + 1];
            g[1] = s_win[idx + stride];
            g[3] = s_win[idx + stride + 1];
        } else {  // workgroup-uniform, rare: a corner outside the window reads global memory if it is inside the image (see k_grad)
            const int row = (int)(rc[j] >> 16) - 16384, col = (int)(rc[j] & 0xFFFFu) - 16384;  // empty slot: far outside
            const int lr = row - win.r0, lc = col - win.c0;
            const bool r_in0 = (unsigned)lr < (unsigned)win.h, r_in1 = (unsigned)(lr + 1) < (unsigned)win.h;
            const bool c_in0 = (unsigned)lc < (unsigned)win.w, c_in1 = (unsigned)(lc + 1) < (unsigned)win.w;
            const int base = lr * win.stride + lc;
            g[0] = s_win[(r_in0 && c_in0) ? base : dummy];
            g[1] = s_win[(r_in1 && c_in0) ? base + stride : dummy];
            g[2] = s_win[(r_in0 && c_in1) ? base + 1 : dummy];
            g[3] = s_win[(r_in1 && c_in1) ? base + stride + 1 : dummy];
            if (rc[j] != 0u) {
#pragma unroll 1
                for (int q = 0; q < 4; ++q) {
                    const int r = row + (q & 1), c = col + (q >> 1);
                    const bool in_win = (unsigned)(r - win.r0) < (unsigned)win.h && (unsigned)(c - win.c0) < (unsigned)win.w;
                    if (!in_win && (unsigned)r < (unsigned)wp.Hp && (unsigned)c < (unsigned)wp.Wp) {
                        const float v = g_at(r, c);
                        g[0] = q == 0 ? v : g[0];
                        g[1] = q == 1 ? v : g[1];
                        g[2] = q == 2 ? v : g[2];
                        g[3] = q == 3 ? v : g[3];
                    }
                }
            }
        }
        const float a = fa[j], b = fb[j];
        const float t0 = fmaf(a, g[1] - g[0], g[0]), t1 = fmaf(a, g[3] - g[2], g[2]);
        const int l = L::kEPT * (int)threadIdx.x + j;
        if ((unsigned)(l - odd) < (unsigned)sg.y) out[l] = fmaf(b, t1 - t0, t0);
    }
}

// ---------------------------------------------------------------------------------------------
// K3e: dL/d(event) per event (cmax_objective_event_grad), one workgroup per segment -- K3w's twin with the bilinear DIFFERENCES
//     where K3w has the interpolation (the same window, the same published cells, consecutive slots, a FINISHED G image per
//     reference time):
//        gx = w [(1-b)(G10-G00) + b(G11-G01)],  gy = w [(1-a)(G01-G00) + a(G11-G10)]      (what cmax_vote_bwd returns per image)
//        c  = dL/d(dt) = gx th0 + gy th1 (2-DoF: x' = x + dt theta)  |  -(gx f0 + gy f1) (dense / voxel: x' = x - dt f[src]),
//     dt the time offset as the warp uses it; source pixel and bin are piecewise constant.  Slot l of the segment stores
//     ge[plane 3 y + {0, 1, 2}][first + l] = (gx, gy, c), coalesced, no atomics; empty slots store nothing (the host clears the
//     planes).  MODEL = -1: the un-warped events against dL/dI_orig -- the x and y planes only.  WEIGHTED: w = the slot's weight
//     (load_slot_weights), else 1.  A kernel of its own: no existing instantiation changes (profiles/event_grad_resources.txt).
// ---------------------------------------------------------------------------------------------
template <class L, int MODEL, bool FRAC, bool WEIGHTED>
__global__ void __launch_bounds__(L::kThr)
k_event_grad_gather(const int4 *__restrict__ segs, int nseg, const uint2 *__restrict__ evp, const char *__restrict__ cev, const int4 *__restrict__ win_base, EvView ev,
                    WarpParams wp, RefArgs ra, float *__restrict__ ge, int64_t plane) {
    constexpr bool kFlow = MODEL == CMAX_MODEL_DENSE || MODEL == CMAX_MODEL_VOXEL;
    const int sidx = segment_of_block(nseg);
    if (sidx >= nseg) return;
    const int4 sg = segs[sidx];
    const int4 *known = win_base + (int64_t)blockIdx.y * nseg + sidx;
    ev.ev = evp;
    EventLoads<L> el;
    issue_event_loads<L, false>(evp, cev, sidx, sg, el);
    wp.d = ra.d[blockIdx.y];  // blockIdx.y = reference time of this workgroup
    const float *__restrict__ img = ra.img[blockIdx.y];
    __shared__ float s_win[L::kWinCap + kScratch];
    unsigned rc[L::kEPT];
    float fa[L::kEPT], fb[L::kEPT], fdt[L::kEPT];
    int fsrc[L::kEPT];
    const int lane = threadIdx.x & (kWave - 1);
    auto g_at = [&](int r, int c) -> float { return img[pix_index(r, c, wp.Wp)]; };
    auto load_window = [&](const Window &w) {  // G of the window, zero outside the image (flat walk, see k_grad)
        const unsigned ustride = (unsigned)w.stride, magic = ((1u << 21) + ustride - 1u) / ustride;
        const int wn = w.h * w.stride;
        for (int i = threadIdx.x; i < wn; i += L::kThr) {
            const unsigned r = mul24_u((unsigned)i, magic) >> 21, c = (unsigned)i - mul24_u(r, ustride);
            const int R = w.r0 + (int)r, C = w.c0 + (int)c;
            s_win[i] = ((int)c < w.w && (unsigned)R < (unsigned)wp.Hp && (unsigned)C < (unsigned)wp.Wp) ? g_at(R, C) : 0.f;
        }
    };
    const unsigned *__restrict__ shifts = ra.shifts + ((int64_t)blockIdx.y * nseg + sidx) * L::kShiftWords;
    bool live;
    unsigned nib_unused;
    const Window win = phase_warp<L, MODEL, FRAC, true, false, true>(ev, wp, sg, el, rc, fa, fb, fdt, fsrc, nullptr, known, shifts, load_window, live, nib_unused);
    float fw[L::kEPT];  // (behind the warp, as in K1: not live through it)
    if constexpr (WEIGHTED) load_slot_weights<L, false>(ra.wgt, sg, fw);
    float th0 = 0.f, th1 = 0.f;
    if (MODEL == CMAX_MODEL_2DOF) {  // theta as phase_warp reads it
        if (wp.motion_f64) {
            const int *mw = reinterpret_cast<const int *>(wp.motion);
            th0 = (float)__hiloint2double(mw[1], mw[0]);
            th1 = (float)__hiloint2double(mw[3], mw[2]);
        } else {
            th0 = wp.motion[0];
            th1 = wp.motion[1];
        }
    }
    if (threadIdx.x < kScratch) s_win[L::kWinCap + threadIdx.x] = 0.f;  // empty slots / masked corners read 0 from here
    __syncthreads();
    if (!live) return;  // (wave-uniform, behind the last barrier)
    const int dummy = L::kDummy + lane;
    const int stride = win.stride;
    unsigned neg_origin = 0u - ((unsigned)(win.r0 + 16384) * (unsigned)win.stride + (unsigned)(win.c0 + 16384));
    asm volatile("" : "+v"(neg_origin));  // (a VGPR: see fast_index)
    const unsigned scratch = L::kWinCap + lane;
    const int odd = sg.x & 1;
    const int hw = wp.H * wp.W;
    float *__restrict__ outx = ge + (int64_t)blockIdx.y * 3 * plane + ((int64_t)sg.x - odd);
    float *__restrict__ outy = outx + plane;
    float *__restrict__ outc = outy + plane;
#pragma unroll
    for (int j = 0; j < L::kEPT; ++j) {
        float g[4];  // g[0] = G00 (row, col), g[1] = G10 (row+1, col), g[2] = G01 (row, col+1), g[3] = G11
        if (!win.clipped) {  // fast window: the footprint is inside by construction
            const int idx = fast_index(rc[j], neg_origin, win.stride, scratch);
            g[0] = s_win[idx];
            g[2] = s_win[idx + 1];
            g[1] = s_win[idx + stride];
            g[3] = s_win[idx + stride + 1];
        } else {  // workgroup-uniform, rare: a corner outside the window reads global memory if it is inside the image (see k_grad)
            const int row = (int)(rc[j] >> 16) - 16384, col = (int)(rc[j] & 0xFFFFu) - 16384;  // empty slot: far outside
            const int lr = row - win.r0, lc = col - win.c0;
            const bool r_in0 = (unsigned)lr < (unsigned)win.h, r_in1 = (unsigned)(lr + 1) < (unsigned)win.h;
            const bool c_in0 = (unsigned)lc < (unsigned)win.w, c_in1 = (unsigned)(lc + 1) < (unsigned)win.w;
            const int base = lr * win.stride + lc;
            g[0] = s_win[(r_in0 && c_in0) ? base : dummy];
            g[1] = s_win[(r_in1 && c_in0) ? base + stride : dummy];
            g[2] = s_win[(r_in0 && c_in1) ? base + 1 : dummy];
            g[3] = s_win[(r_in1 && c_in1) ? base + stride + 1 : dummy];
            if (rc[j] != 0u) {
#pragma unroll 1
                for (int q = 0; q < 4; ++q) {
                    const int r = row + (q & 1), c = col + (q >> 1);
                    const bool in_win = (unsigned)(r - win.r0) < (unsigned)win.h && (unsigned)(c - win.c0) < (unsigned)win.w;
                    if (!in_win && (unsigned)r < (unsigned)wp.Hp && (unsigned)c < (unsigned)wp.Wp) {
                        const float v = g_at(r, c);
                        g[0] = q == 0 ? v : g[0];
                        g[1] = q == 1 ? v : g[1];
                        g[2] = q == 2 ? v : g[2];
                        g[3] = q == 3 ? v : g[3];
                    }
                }
            }
        }
        const float a = fa[j], b = fb[j];
        float gx = (1.f - b) * (g[1] - g[0]) + b * (g[3] - g[2]);
        float gy = (1.f - a) * (g[2] - g[0]) + a * (g[3] - g[1]);
        if constexpr (WEIGHTED) {
            gx *= fw[j];
            gy *= fw[j];
        }
        const int l = L::kEPT * (int)threadIdx.x + j;
        if ((unsigned)(l - odd) < (unsigned)sg.y) {
            outx[l] = gx;
            outy[l] = gy;
            if (MODEL == CMAX_MODEL_2DOF) {
                outc[l] = fmaf(gx, th0, gy * th1);
            } else if (kFlow) {  // the flow at the event's source pixel (and bin), as the warp read it
                const unsigned key = (unsigned)fsrc[j];
                const int ix = (int)(key & 0xFFFu), iy = (int)((key >> 12) & 0xFFFu), bin = (int)(key >> 24);
                const int64_t fi = (MODEL == CMAX_MODEL_VOXEL ? (int64_t)bin * 2 * hw : (int64_t)0) + pix_index(ix, iy, wp.W);
                outc[l] = -fmaf(gx, wp.motion[fi], gy * wp.motion[fi + hw]);
            }
        }
    }
}

// trailing kernel arguments of the WEIGHTED instantiations (a parameter pack: the unweighted kernels keep their argument block)
__device__ __forceinline__ const float *pack_ptr(int) { return nullptr; }
__device__ __forceinline__ const float *pack_ptr(int, ExactFlow) { return nullptr; }  // (the tag of an fp64 flow ends the pack)
template <class... R>
__device__ __forceinline__ const float *pack_ptr(int i, const float *a, R... r) { return i == 0 ? a : pack_ptr(i - 1, r...); }

// dimg64 (deterministic mode): the window's integers (and the overflow of a clipped window, rounded at the same scale) go to a
// 64-bit integer image with integer atomics -- exact in any order; k_fixed_to_image rounds the finished sums once
// WEIGHTED = called with (w_packed, d_wnorm) behind dimg64 (cmax_iwes_jvp on a weighted handle; default mode only): the event's four
// derivative votes are multiplied by w / wmax before they are rounded, the flush carries wmax -- (1 / wmax, wmax) from d_wnorm as in K1,
// the slot weights loaded behind the warp as in K1 (profiles/weights_resources.txt).  The overflow of a clipped window is not rounded: w d.
template <class L, int MODEL, bool FRAC, class... WGT>
__global__ void __launch_bounds__(L::kThr) k_vote_tan(EvView ev, WarpParams wp, TanParams tp, const int4 *__restrict__ segs, int nseg,
                                                  float *__restrict__ dimg, double *__restrict__ stat_zero, long long *__restrict__ dimg64, WGT... wargs) {
    constexpr bool F64FLOW = (std::is_same_v<WGT, ExactFlow> || ...);  // an ExactFlow ends the arguments: phase_warp's F64FLOW, as in k_vote
    constexpr int kWgtArgs = (int)sizeof...(WGT) - (F64FLOW ? 1 : 0);
    constexpr bool WEIGHTED = kWgtArgs > 0;
    static_assert(kWgtArgs == 0 || kWgtArgs == 2, "k_vote_tan: (w_packed, d_wnorm) or nothing");
    __shared__ int s_win[L::kWinCap + kScratch];
    __shared__ uint4 s_box[L::kNW];
    wp.d = tp.d[blockIdx.y];  // blockIdx.y = reference time
    wp.d_lo = tp.d_lo[blockIdx.y];
    // (the by-value parameter block is only read: writing to it would move it to scratch memory for the indexing)
    const float wn0 = WEIGHTED ? pack_ptr(1, wargs...)[0] : 1.f, wn1 = WEIGHTED ? pack_ptr(1, wargs...)[1] : 1.f;
    // weighted: an event's votes are round(w d fix / wmax), the flush multiplies by wmax / fix
    const float fix = WEIGHTED ? tp.fixk[blockIdx.y] * wn0 : tp.fixk[blockIdx.y], inv_fix = WEIGHTED ? wn1 / tp.fixk[blockIdx.y] : 1.f / fix;
    dimg += blockIdx.y * tp.bs;
    if (dimg64) dimg64 += blockIdx.y * tp.bs;
    stat_zero += blockIdx.y * kStatStride;
    if (stat_zero && blockIdx.x == 0 && threadIdx.x < 2 * kStatSub) stat_zero[(threadIdx.x >> 1) * kSubStride + (threadIdx.x & 1)] = 0.0;
    const int sidx = segment_of_block(nseg);
    if (sidx >= nseg) return;
    const int4 sg = segs[sidx];
    EventLoads<L> el;
    issue_event_loads<L, false>(ev.ev, nullptr, 0, sg, el);
    unsigned rc[L::kEPT];
    float fa[L::kEPT], fb[L::kEPT], fdt[L::kEPT];
    int fsrc[L::kEPT];
    bool live;
    unsigned nib_unused;
    const Window win = phase_warp<L, MODEL, FRAC, true, false, false, F64FLOW>(ev, wp, sg, el, rc, fa, fb, fdt, fsrc, s_box, nullptr, nullptr, [&](const Window &w) {
        const int wn = w.h * w.stride;
        for (int i = threadIdx.x; i < wn; i += L::kThr) s_win[i] = 0;
    }, live, nib_unused);
    float u0 = 0.f, u1 = 0.f;
    if (MODEL == CMAX_MODEL_2DOF) {
        u0 = tp.u[0];
        u1 = tp.u[1];
    }
    float fw[L::kEPT];  // (behind the warp, as in K1: not live through it)
    if constexpr (WEIGHTED) load_slot_weights<L, false>(pack_ptr(0, wargs...), sg, fw);
    __syncthreads();
    const int dummy = L::kDummy + (int)(threadIdx.x & (kWave - 1));
#pragma unroll
    for (int u = 0; u < L::kEPT; ++u) {
        const bool valid = rc[u] != 0u;
        const int row = (int)(rc[u] >> 16) - 16384, col = (int)(rc[u] & 0xFFFFu) - 16384;
        const float a = fa[u], b = fb[u], na = 1.f - a, nb = 1.f - b;
        float da = 0.f, db = 0.f;
        if (valid) tangent_delta<MODEL>(wp, tp, fdt[u], (unsigned)fsrc[u], u0, u1, da, db);
        if constexpr (WEIGHTED) {  // the four votes are linear in (da, db): w scales the VOTES, here through their common factors
            const float w = valid ? fw[u] : 0.f;  // (an empty slot's weight is padding)
            da *= w;
            db *= w;
        }
        // derivatives of w00 = na nb, w10 = a nb, w01 = na b, w11 = a b along (da, db)
        const float d00 = -nb * da - na * db, d10 = nb * da - a * db, d01 = -b * da + na * db, d11 = b * da + a * db;
        const int lr = row - win.r0, lc = col - win.c0;
        const bool r_in0 = (unsigned)lr < (unsigned)win.h, r_in1 = (unsigned)(lr + 1) < (unsigned)win.h;
        const bool c_in0 = (unsigned)lc < (unsigned)win.w, c_in1 = (unsigned)(lc + 1) < (unsigned)win.w;
        const int base = lr * win.stride + lc, stride = win.stride;
        atomicAdd(&s_win[(r_in0 && c_in0) ? base : dummy], (r_in0 && c_in0) ? __float2int_rn(d00 * fix) : 0);
        atomicAdd(&s_win[(r_in1 && c_in0) ? base + stride : dummy], (r_in1 && c_in0) ? __float2int_rn(d10 * fix) : 0);
        atomicAdd(&s_win[(r_in0 && c_in1) ? base + 1 : dummy], (r_in0 && c_in1) ? __float2int_rn(d01 * fix) : 0);
        atomicAdd(&s_win[(r_in1 && c_in1) ? base + stride + 1 : dummy], (r_in1 && c_in1) ? __float2int_rn(d11 * fix) : 0);
        if (win.clipped && valid) {
            const float dv[4] = {d00, d10, d01, d11};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = row + (q & 1), c = col + (q >> 1);
                const bool in_win = (unsigned)(r - win.r0) < (unsigned)win.h && (unsigned)(c - win.c0) < (unsigned)win.w;
                if (!in_win && (unsigned)r < (unsigned)wp.Hp && (unsigned)c < (unsigned)wp.Wp) {
                    if (dimg64) atomic_add_i64(&dimg64[(int64_t)r * wp.Wp + c], (long long)__float2int_rn(dv[q] * fix));
                    else atomic_add(&dimg[(int64_t)r * wp.Wp + c], dv[q]);
                }
            }
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    for (int r = wave; r < win.h; r += L::kNW) {
        if ((unsigned)(win.r0 + r) >= (unsigned)wp.Hp) continue;  // the fast window is not clipped to the image
        float *dst = dimg + (int64_t)(win.r0 + r) * wp.Wp + win.c0;
        long long *dst64 = dimg64 ? dimg64 + (int64_t)(win.r0 + r) * wp.Wp + win.c0 : nullptr;
        for (int c = lane; c < win.w; c += kWave) {
            const int v = s_win[r * win.stride + c];
            if (v != 0 && (unsigned)(win.c0 + c) < (unsigned)wp.Wp) {
                if (dst64) atomic_add_i64(&dst64[c], (long long)v);
                else atomic_add(&dst[c], (float)v * inv_fix);
            }
        }
    }
}

// T3: per-event second-order gather.  G = dL/dIWE (current), Gp = its tangent.
// WEIGHTED = called with w_packed behind det (cmax_iwes_vjp / cmax_iwes_vjp_tan on a weighted handle; default mode only): the factor w goes
// on the final dt (hx, hy) product only -- tangent_delta is the displacement dt u of the warped POINT, which the weight does not move.
template <class L, int MODEL, bool FRAC, class... WGT>
__global__ void __launch_bounds__(L::kThr)
k_grad_hvp(EvView ev, WarpParams wp, TanParams tp, const int4 *__restrict__ segs, int nseg, const float *__restrict__ G,
           const float *__restrict__ Gp, double *__restrict__ gpart, float *__restrict__ hflow, HvpDet det, WGT... wargs) {
    constexpr bool F64FLOW = (std::is_same_v<WGT, ExactFlow> || ...);  // an ExactFlow ends the arguments, as in k_vote_tan
    constexpr int kWgtArgs = (int)sizeof...(WGT) - (F64FLOW ? 1 : 0);
    constexpr bool WEIGHTED = kWgtArgs > 0;
    static_assert(kWgtArgs <= 1, "k_grad_hvp: w_packed or nothing");
    wp.d = tp.d[blockIdx.y];  // blockIdx.y = reference time
    wp.d_lo = tp.d_lo[blockIdx.y];
    G += blockIdx.y * tp.bs;
    Gp += blockIdx.y * tp.bs;
    if (gpart) gpart += (int64_t)blockIdx.y * nseg * 2;
    __shared__ float s_g[L::kWinCap + kWave];
    __shared__ float s_p[L::kWinCap + kWave];
    __shared__ uint4 s_box[L::kNW];
    __shared__ double s_red[2 * L::kNW];
    const int sidx = segment_of_block(nseg);
    if (sidx >= nseg) return;
    const int4 sg = segs[sidx];
    EventLoads<L> el;
    issue_event_loads<L, false>(ev.ev, nullptr, 0, sg, el);
    unsigned rc[L::kEPT];
    float fa[L::kEPT], fb[L::kEPT], fdt[L::kEPT];
    int fsrc[L::kEPT];
    const int lane = threadIdx.x & (kWave - 1);
    bool live;
    unsigned nib_unused;
    const Window win = phase_warp<L, MODEL, FRAC, true, false, false, F64FLOW>(ev, wp, sg, el, rc, fa, fb, fdt, fsrc, s_box, nullptr, nullptr, [&](const Window &w) {
        for (int r = threadIdx.x / kWave; r < w.h; r += L::kNW)
            for (int c = lane; c < w.w; c += kWave) {
                const int64_t q = (int64_t)(w.r0 + r) * wp.Wp + w.c0 + c;
                const bool in = (unsigned)(w.r0 + r) < (unsigned)wp.Hp && (unsigned)(w.c0 + c) < (unsigned)wp.Wp;
                s_g[r * w.stride + c] = in ? G[q] : 0.f;  // the fast window is not clipped to the image
                s_p[r * w.stride + c] = in ? Gp[q] : 0.f;
            }
    }, live, nib_unused);
    float u0 = 0.f, u1 = 0.f;
    if (MODEL == CMAX_MODEL_2DOF) {
        u0 = tp.u[0];
        u1 = tp.u[1];
    }
    if (threadIdx.x < kWave) {
        s_g[L::kDummy + threadIdx.x] = 0.f;
        s_p[L::kDummy + threadIdx.x] = 0.f;
    }
    float fw[L::kEPT];  // (behind the warp, as in K1: not live through it)
    if constexpr (WEIGHTED) load_slot_weights<L, false>(pack_ptr(0, wargs...), sg, fw);
    __syncthreads();
    const int hw = wp.H * wp.W;
    const int dummy = L::kDummy + lane, stride = win.stride;
    float accx = 0.f, accy = 0.f;
    // deterministic mode (det.g64 != null): every term becomes a 64-bit integer at a scale all workgroups derive identically from
    // max |G| and max |G'| of this reference time (|hx| <= 4 max|G| dtmax + 2 max|G'|, |term| <= dtmax |hx|; x4 for the fp32 roundings)
    // and only integers are added from there on -- per thread, then 64-bit LDS atomics (2-DoF) or global ones per run of one
    // source pixel (flow models): exact in any order, like the deterministic K3
    const bool kdet = det.g64 != nullptr;
    double det_s = 1.0;
    long long ax64 = 0, ay64 = 0;
    unsigned kcur = 0xFFFFFFFFu;
    __shared__ long long s_acc64[2];
    if (kdet) {
        auto bound_of = [&](int kk) -> double {
            const double gmx = (double)__uint_as_float(det.imax[kk]), gpmx = (double)__uint_as_float(det.imax[4 + kk]);
            const double dk = (double)tp.d[kk], dtm = fmax(fabs(dk), fabs(1.0 - dk)) * (double)time_scale(wp);
            return 4.0 * dtm * (4.0 * gmx * dtm + 2.0 * gpmx);
        };
        double bound = 0.0;
        if (MODEL == CMAX_MODEL_2DOF) bound = bound_of((int)blockIdx.y);
        else
            for (int kk = 0; kk < det.n_ref; ++kk) bound = fmax(bound, bound_of(kk));
        det_s = det_scale(bound, det.n_events);
        if (sidx == 0 && threadIdx.x == 0 && (MODEL == CMAX_MODEL_2DOF || blockIdx.y == 0)) det.inv_scale[MODEL == CMAX_MODEL_2DOF ? blockIdx.y : 0] = 1.0 / det_s;
        if (MODEL == CMAX_MODEL_2DOF) {
            if (threadIdx.x < 2) s_acc64[threadIdx.x] = 0;
            __syncthreads();
        }
    }
#pragma unroll
    for (int j = 0; j < L::kEPT; ++j) {
        const bool valid = rc[j] != 0u;
        const int row = (int)(rc[j] >> 16) - 16384, col = (int)(rc[j] & 0xFFFFu) - 16384;
        const int lr = row - win.r0, lc = col - win.c0;
        const bool r_in0 = (unsigned)lr < (unsigned)win.h, r_in1 = (unsigned)(lr + 1) < (unsigned)win.h;
        const bool c_in0 = (unsigned)lc < (unsigned)win.w, c_in1 = (unsigned)(lc + 1) < (unsigned)win.w;
        const int base = lr * win.stride + lc;
        const int i00 = (r_in0 && c_in0) ? base : dummy, i10 = (r_in1 && c_in0) ? base + stride : dummy;
        const int i01 = (r_in0 && c_in1) ? base + 1 : dummy, i11 = (r_in1 && c_in1) ? base + stride + 1 : dummy;
        float g[4] = {s_g[i00], s_g[i10], s_g[i01], s_g[i11]};
        float q[4] = {s_p[i00], s_p[i10], s_p[i01], s_p[i11]};
        if (win.clipped && valid) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int r = row + (t & 1), c = col + (t >> 1);
                const bool in_win = (unsigned)(r - win.r0) < (unsigned)win.h && (unsigned)(c - win.c0) < (unsigned)win.w;
                if (!in_win && (unsigned)r < (unsigned)wp.Hp && (unsigned)c < (unsigned)wp.Wp) {
                    g[t] = G[(int64_t)r * wp.Wp + c];
                    q[t] = Gp[(int64_t)r * wp.Wp + c];
                }
            }
        }
        const float a = fa[j], b = fb[j];
        float dt = fdt[j];
        float da = 0.f, db = 0.f;
        if (valid) tangent_delta<MODEL>(wp, tp, dt, (unsigned)fsrc[j], u0, u1, da, db);
        const float mixed = (g[3] - g[2]) - (g[1] - g[0]);  // d gx / d b = d gy / d a
        const float hx = mixed * db + (1.f - b) * (q[1] - q[0]) + b * (q[3] - q[2]);
        const float hy = mixed * da + (1.f - a) * (q[2] - q[0]) + a * (q[3] - q[1]);
        if constexpr (WEIGHTED) dt = valid ? dt * fw[j] : 0.f;  // from here on dt only multiplies (hx, hy); an empty slot's weight is padding
        if (kdet) {
            const float sgn = MODEL == CMAX_MODEL_2DOF ? 1.f : -1.f;
            const long long qx = det_fixed((double)(sgn * dt * hx), det_s), qy = det_fixed((double)(sgn * dt * hy), det_s);
            if (MODEL == CMAX_MODEL_2DOF) {
                if (valid) {
                    ax64 += qx;
                    ay64 += qy;
                }
            } else if (valid) {
                const unsigned key = (unsigned)fsrc[j];
                if (key != kcur) {
                    if (kcur != 0xFFFFFFFFu) {
                        const int64_t o = (int64_t)(kcur >> 24) * 2 * hw + (int64_t)(kcur & 0xFFFu) * wp.W + (int)((kcur >> 12) & 0xFFFu);
                        atomic_add_i64(&det.g64[o], ax64);
                        atomic_add_i64(&det.g64[o + hw], ay64);
                    }
                    kcur = key;
                    ax64 = 0;
                    ay64 = 0;
                }
                ax64 += qx;
                ay64 += qy;
            }
        } else if (MODEL == CMAX_MODEL_2DOF) {
            accx = fmaf(dt, hx, accx);
            accy = fmaf(dt, hy, accy);
        } else if (valid) {
            const unsigned key = (unsigned)fsrc[j];
            const int ix = (int)(key & 0xFFFu), iy = (int)((key >> 12) & 0xFFFu), bin = (int)(key >> 24);
            const int64_t o = (int64_t)bin * 2 * hw + (int64_t)ix * wp.W + iy;
            atomic_add(&hflow[o], -dt * hx);  // the HVP runs once per CG step: plain per-event atomics are enough
            atomic_add(&hflow[o + hw], -dt * hy);
        }
    }
    if (kdet) {
        if (MODEL == CMAX_MODEL_2DOF) {
            atomic_add_i64(&s_acc64[0], ax64);
            atomic_add_i64(&s_acc64[1], ay64);
            __syncthreads();
            if (threadIdx.x < 2) det.g64[((int64_t)blockIdx.y * nseg + sidx) * 2 + threadIdx.x] = s_acc64[threadIdx.x];
        } else if (kcur != 0xFFFFFFFFu) {
            const int64_t o = (int64_t)(kcur >> 24) * 2 * hw + (int64_t)(kcur & 0xFFFu) * wp.W + (int)((kcur >> 12) & 0xFFFu);
            atomic_add_i64(&det.g64[o], ax64);
            atomic_add_i64(&det.g64[o + hw], ay64);
        }
        return;
    }
    if (MODEL == CMAX_MODEL_2DOF) {
        double acc[2] = {(double)accx, (double)accy};
        block_sum<2>(acc, s_red);
        if (threadIdx.x == 0) {
            gpart[2 * sidx] = acc[0];
            gpart[2 * sidx + 1] = acc[1];
        }
    }
}

