// Fused contrast-maximization objective for MI355X (gfx950): the per-event kernels and their launch layer.
//
//   K1  k_vote      one workgroup per SEGMENT (<= 2040 consecutive sorted events = a few neighbouring
//                   source tiles): warp, bounding box of the targets, votes accumulated in an LDS
//                   window as 12.20 fixed point with ds_add_u32 (fp32 LDS atomics run at 1/12 of the
//                   integer rate on gfx950, profiles/r01_microbench.txt), one coalesced global
//                   atomicAdd per touched window pixel; publishes its windows for K3
//   K3  k_grad      per event: re-warp, gather G at the 4 corners -> dL/d(x',y') -> motion gradient
//                   (2-DoF: per-segment partials, for the plain variance together with the image
//                   statistics so that K2 is not launched at all; dense: runs of equal source pixel
//                   reduced in registers + one segmented scan, one atomic per run; voxel: LDS
//                   accumulators in block-scaled fixed point)
//   (K2, the image kernels between them, and k_finish* behind them: cmax_fused.hip)
// Every launch covers all reference times of the objective (blockIdx.y).  The event kernels live in
// cmax_event_kernels.inc, templates over the segment layout (EventLayout: t256 / t512 / t1024 for segments of
// up to 2040 events, m512 for mid and b512 / b1024 for big segments).  The layout of a launch is chosen in one
// function per kernel family: vote_layout (K1: 512 threads above 512 segments), grad_layout (K3: the same, 1024
// for the voxel K3 above 1024 segments) and plain_layout (deterministic K3 and the tangent kernels).
// Almost all kernel instantiations of the library are compiled here; the launchers (launch_vote, launch_grad, launch_vote_tan,
// launch_vote_tan2, launch_grad_hvp, the per-event gathers) are this unit's interface, declared in cmax_fused_internal.h.
//
// fp32 per event with the integer source pixel split from the fp32 displacement (keeps the
// bilinear fractions accurate to ulp(displacement) instead of ulp(coordinate)); fp64 reductions.
#include "cmax_fused_device.h"

namespace cmax {

// ---------------------------------------------------------------------------------------------
// per-event warp shared by K1 and K3
// ---------------------------------------------------------------------------------------------
// The normalised time of an UN-BINNED handle's packed event with the residual byte the sort left above the source pixel
// (tau_residual8, cmax_sort_kernels.h): tau = (double)tau32 + q * ulp(tau32) / 256
__device__ __forceinline__ double tau_refined(uint2 e) {
    const uint32_t eb = e.y & 0x7F800000u;
    const int q = (int)e.x >> 24;  // sign-extended
    const double hi = (double)__uint_as_float(e.y);
    return eb < (32u << 23) ? hi : hi + (double)q * (double)__uint_as_float(eb - (31u << 23));
}


// v_cvt_flr_i32_f32: (int)floor(x) in one instruction, saturating
__device__ __forceinline__ int cvt_flr(float x) {
    int r;
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}

struct Warped {
    int row, col;  // top-left corner in the padded image
    float a, b;    // row / column fractions
    float dt;
    int src;       // source pixel linear index (un-padded), + bin * 2HW for voxel
    float f0, f1;  // dense / voxel: the flow at the source pixel (phase_warp bounds the rounding of dt * f with it)
};

// One event as the warp sees it, whichever way it was stored (plain 8-byte event: absolute coordinates, zero bases; compact event of a
// big segment: coordinates relative to the segment's tile strip, bases from the region's header -- cmax_event_kernels.inc).
struct EvDec {
    unsigned ixr, iyr;  // source row / column minus EvBase::row / col
    unsigned top;       // top byte of the plain packed word (voxel: the time bin)
    unsigned key;       // (row | col << 12 [| bin << 24]) absolute: the run key of the flow-gradient reduction (K3)
    float tmd;          // tau - d: calculate_dt before the time scale, rounded once
};
struct EvBase {  // workgroup-uniform
    unsigned row, col;  // what ixr / iyr are relative to (0 for plain events)
    unsigned src;       // row * W + col
};

// MODEL: -1 none (orig_iwe), 0 2-DoF, 1 dense, 2 voxel
template <int MODEL, bool FRAC>
__device__ __forceinline__ Warped warp_one(const EvView &ev, const EvDec &e, const EvBase &eb, int64_t i, bool valid, const WarpParams &wp, float tscale, float th0,
                                           float th1) {
    Warped w;
    const int ix = (int)e.ixr, iy = (int)e.iyr;
    w.dt = e.tmd * tscale;  // calculate_dt, src/warp.py:254-259
    float dx = 0.f, dy = 0.f;
    if (FRAC && valid) {  // `valid` false: an empty slot of the caller (zero event), i may be outside the arrays
        dx = ev.rx[i];
        dy = ev.ry[i];
    }
    w.src = (int)(__umul24((unsigned)ix, (unsigned)wp.W & 0xFFFFFFu) + (unsigned)iy + eb.src);  // 12-bit x 13-bit: v_mul_u32_u24 (full rate; v_mul_lo_u32 runs at a quarter)
    if (MODEL == CMAX_MODEL_2DOF) {
        dx = fmaf(w.dt, th0, dx);  // x' = x + dt*theta0, src/warp.py:506-515
        dy = fmaf(w.dt, th1, dy);
    } else if (MODEL == CMAX_MODEL_DENSE || MODEL == CMAX_MODEL_VOXEL) {
        const int hw = wp.H * wp.W;
        if (MODEL == CMAX_MODEL_VOXEL) w.src += (int)e.top * 2 * hw;  // (2 HW can exceed 24 bits: a full 32-bit multiply)
        // uniform base + unsigned 32-bit BYTE offset: one address instruction per event and a `global_load_dword v, voff, s[base]`
        // per channel, instead of 64-bit per-lane pointer arithmetic (the field is < 4 GiB: checked by the host)
        const unsigned off = (unsigned)w.src * 4u;
        const char *m0 = reinterpret_cast<const char *>(wp.motion), *m1 = reinterpret_cast<const char *>(wp.motion + hw);
        w.f0 = *reinterpret_cast<const float *>(m0 + off);
        w.f1 = *reinterpret_cast<const float *>(m1 + off);
        dx = fmaf(-w.dt, w.f0, dx);  // x' = x - dt*F[0,ix,iy], src/warp.py:305-306
        dy = fmaf(-w.dt, w.f1, dy);
    }
    // floor(x' + 1e-6) = ix + floor(dx + 1e-6) exactly because ix is an integer
    // (bilinear_vote_tensor, src/event_image_converter.py:340-345)
    // Round 6 (VALU diet): v_floor_f32 + v_cvt_i32_f32 per coordinate; the v_med3_f32 between them (a clamp to +-8192) is gone:
    // a displacement beyond +-8192 px (a diverged or non-finite motion) now lands on whatever cell the saturated conversion names --
    // (v_cvt_i32_f32 saturates) -- its packed (row, col) word may wrap, but every consumer derives box, window and indices from the SAME word, so such an event
    // is either outside every window of the fast path's 8192 words (-> the clipped path, whose every corner is tested against window
    // and image) or votes in bounds; it was never defined where.
    const float fx = floorf(dx + 1e-6f), fy = floorf(dy + 1e-6f);
    const int fxi = (int)fx, fyi = (int)fy;  // (v_cvt_i32_f32 saturates; through inline asm v_cvt_flr_i32_f32 + v_cvt_f32_i32 are two instructions as well, but
    w.a = dx - fx;                           // the asm operands cost the 512 x 8 K3 eleven VGPRs, i.e. a wave per SIMD)
    w.b = dy - fy;
    w.row = ix + fxi + (int)(eb.row + (unsigned)wp.ph);
    w.col = iy + fyi + (int)(eb.col + (unsigned)wp.pw);
    return w;
}

// EXACT CELLS (round 3: 2-DoF; round 4: every model).  The image is continuous across a cell border, the gradient is not (it takes
// its differences of dL/dIWE from the event's own cell): an event whose displacement lies within fp32 rounding of a border falls
// on the other side in any fp32 evaluation, and its term of the gradient then comes from the wrong side of the kink -- ~70 of a
// million events moved the 2-DoF gradient (ONE sum over all events) by 6e-4 relative against the reference's fp64 value (the
// reference's own fp32 path: 1.3e-3, tests/golden/cfg2_fp32_reference.npz), and a flow gradient by more than 1e-4 in the pixels
// such events come from (2-5 of 0.6-1.8M entries at the BASELINE sizes).  The fp32 displacement of warp_one is off by at most
// 7 * 2^-24 |motion| max(period, 1) max(1, |d|, |1 - d|) (rounding of tau, of tau - d, of the time scale, of the product, of the
// + 1e-6); an event whose fraction a or b comes closer than exact_margin to 0 or 1 is warped again here BY K1, with the arithmetic of
// src/warp.py:304-307 / 506-515 + src/event_image_converter.py:340 in fp64: the fp64 normalised time (EvView::tau64, a load only
// these events make), the caller's fp64 theta (2-DoF), the flow as the device holds it (fp32 values, fp64 arithmetic) -- 1e-5 ..
// 1e-4 of the events -- and K1 publishes the cell's offset from the fp32 one for K3 (phase_warp).
template <int MODEL, bool FRAC>
__device__ __forceinline__ Warped warp_exact(const EvView &ev, unsigned ex, int64_t i, double tau, double period, const WarpParams &wp, double m0, double m1) {
    Warped w;
    const int ix = (int)(ex & 0xFFFu), iy = (int)((ex >> 12) & 0xFFFu);
    const double dtd = (tau - ((double)wp.d + (double)wp.d_lo)) * period;
    const double sgn = MODEL == CMAX_MODEL_2DOF ? 1.0 : -1.0;  // x' = x + dt theta (warp.py:514)  |  x' = x - dt F (warp.py:305)
    double srx = 0.0, sry = 0.0;  // the source coordinate's residual as the reference's fp64 arithmetic sees it
    if (FRAC) {
        const float2 lo = ev.rl[i];
        srx = (double)ev.rx[i] + (double)lo.x;
        sry = (double)ev.ry[i] + (double)lo.y;
    }
    const double ddx = fma(sgn * dtd, m0, srx), ddy = fma(sgn * dtd, m1, sry);
    const double fxd = fmin(fmax(floor(ddx + 1e-6), -8192.0), 8192.0), fyd = fmin(fmax(floor(ddy + 1e-6), -8192.0), 8192.0);
    w.a = (float)(ddx - fxd);
    w.b = (float)(ddy - fyd);
    w.row = ix + (int)fxd + wp.ph;
    w.col = iy + (int)fyd + wp.pw;
    w.dt = 0.f;
    w.src = 0;
    w.f0 = 0.f;
    w.f1 = 0.f;
    return w;
}
// The margin m of an event: it is a candidate for warp_exact when a + 1e-6 or b + 1e-6 lies in [0, m) or (1 - m, 1).  With eps = 2^-24
// the fp32 displacement dx = fl(rx -/+ dt32 f), dt32 = fl(fl(tau32 - d32) period32), is off by at most
//   eps (3.5 |dt f| + kappa |f|),   kappa = 0 for the reference time "first" (d = 0: the rounding of tau is then relative to dt itself),
//                                   else (1 + |d| / 2) period (roundings of tau and d: absolute in dt, so they scale with |f| alone)
// -- 3.5: the subtraction, the period, the product, the fma and the `+ 1e-6` at eps / 2 each, tau at eps (d = 0), theta at eps / 2
// (2-DoF) -- and |dt| <= period max(|d|, |1 - d|).  m = 1.5 eps (4 period max(|d|, |1 - d|) + kappa) fm with fm = max |motion component|
// of the event (a function of the EVENT alone, so that nothing depends on how threads and events are matched).  Fractional sources add
// the rounding of rx and the fma's on a sum of magnitude up to 1.  Everything else is RELATIVE to the motion: a zero motion -- the
// optimiser's usual starting point, where every event sits ON a border -- has no candidates.
// An fp64 flow / voxel (WarpParams::motion_f64): the bulk warp reads hi = fl(f), off from the caller's f by at most eps / 2 |f|, so
// dx gains eps / 2 |dt f| against the fp64 arithmetic on f itself -- the term listed for theta above, which the flow models had
// no use for while the flow was the device's own fp32.  The count is the 2-DoF model's, 3.5 |dt f| (4 with d = 0 counted in full)
// against the 6 |dt f| the coefficient grants, and fm = max |hi| is |f| to within 1 + eps: the coefficient stands, and an fp32 call
// selects the candidates it selected before.
__device__ __forceinline__ float exact_margin_coef(float d, float tscale) {
    const float kappa = d == 0.f ? 0.f : (1.f + 0.5f * fabsf(d)) * tscale;
    return 0x1.8p-24f * (4.f * tscale * fmaxf(fabsf(d), fabsf(1.f - d)) + kappa);
}
template <bool FRAC>
__device__ __forceinline__ float exact_margin(float coef, float fm) { return fmaf(coef, fm, FRAC ? 0x1p-21f : 0.f); }

__device__ __forceinline__ float time_scale(const WarpParams &wp) {
    return wp.normalize ? 1.0f : (float)(wp.tmm[1] - wp.tmm[0]);
}

// Workgroup -> segment, XCD-aware: the dispatcher places block b on XCD b % 8, so giving XCD x the
// contiguous range [x * per, (x+1) * per) keeps neighbouring tiles (shared halo rows of the IWE / G
// windows, neighbouring flow pixels) in one XCD's L2.  Placement only affects speed.
__device__ __forceinline__ int segment_of_block(int nseg, unsigned bx = blockIdx.x) {
    const int per = (nseg + 7) >> 3;
    return (int)(bx & 7u) * per + (int)(bx >> 3);
}

// Row stride of an LDS window of width w.  With a power-of-two stride (the first version: a shift per index) the bank of a
// cell is its COLUMN modulo 32 whatever its row -- a 20-pixel-wide window used 20 of the 32 banks, and the two rows of a
// 2 x 2 footprint always collided (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.55-0.70 in K1 and K3, profiles/r02_sq_*).  An odd
// stride walks the banks row by row; the index costs one v_mad_u32_u24 instead of a shift + add.
__host__ __device__ inline int window_stride(int w) { return (w < 15 ? 15 : w) | 1; }

struct Window {
    int r0, c0, h, w;  // top-left corner in the padded image, extent (clipped to the image and to LDS)
    int stride;        // LDS row stride in words: odd (window_stride), so that the rows of a window start in different banks
    bool clipped;      // the bounding box did not fit: votes / reads outside the window but inside the image exist
    bool border;       // the segment holds an event within fp32 rounding of a cell border (K1's verdict, re-used by K3)
    unsigned long long bmask;  // ... and where: bit q = such an event among the segment's slots [q * kSlots / 64, (q + 1) * kSlots / 64)
};
// A window as K1 publishes it for K3 of the same evaluation (RefArgs::win): position | geometry + flags | the 64 bits of bmask
// (the LDS row stride follows from the width)
__device__ __forceinline__ int4 pack_window(const Window &w) {
    return make_int4((int)(((unsigned)(w.r0 + 16384) << 16) | (unsigned)(w.c0 + 16384)),
                     w.h | (w.w << 12) | (w.clipped ? (1 << 28) : 0) | (w.border ? (1 << 29) : 0),
                     (int)(unsigned)w.bmask, (int)(unsigned)(w.bmask >> 32));
}
__device__ __forceinline__ Window unpack_window(int4 kw) {
    Window w;
    w.r0 = (int)((unsigned)kw.x >> 16) - 16384;
    w.c0 = (int)((unsigned)kw.x & 0xFFFFu) - 16384;
    w.h = kw.y & 0xFFF;
    w.w = (kw.y >> 12) & 0xFF;
    w.stride = window_stride(w.w);
    w.clipped = ((kw.y >> 28) & 1) != 0;
    w.border = ((kw.y >> 29) & 1) != 0;
    w.bmask = (unsigned long long)(unsigned)kw.z | ((unsigned long long)(unsigned)kw.w << 32);
    return w;
}
// Linear index of pixel (r, c) of an image that is W wide, r >= 0: one full-rate v_mad_u32_u24 (rows and widths are < 2^13;
// a 64-bit r * W + c is a quarter-rate v_mad_u64_u32, a 32-bit one a quarter-rate v_mul_lo_u32 -- and the event kernels are
// VALU-bound on the large configurations: SQ_ACTIVE_INST_VALU x 8 waves ~ 0.8 of the SIMD cycles in K1 / K3 of cfg3).
__device__ __forceinline__ int pix_index(int r, int c, int W) { return (int)__umul24((unsigned)r, (unsigned)W & 0xFFFFFFu) + c; }

constexpr int kScratch = 200;       // scratch words behind the window; the fast path sends the 2x2 footprint of an
                                    // empty slot to kWinCap + lane + {0, 1, stride, stride + 1}, stride <= 128
static_assert(kScratch >= 64 + kWinMaxW + 2, "scratch must hold a per-lane 2x2 footprint at the widest stride");

// v_cvt_rpi_i32_f32: floor(x + 0.5) in one instruction (rndne + cvt are two)
__device__ __forceinline__ int cvt_rpi(float x) {
    int r;
    asm("v_cvt_rpi_i32_f32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}
// v_mad_u32_u16 with the HIGH half of `packed` as first factor: (packed >> 16) * factor + addend in one instruction (`factor` wave-uniform,
// below 2^16), and v_add_u32 with the LOW half of `packed` through SDWA: the LDS word of a packed (row, col) in two instructions where
// shift, mask, multiply-add and add were four
__device__ __forceinline__ unsigned mad_hi16_u(unsigned packed, unsigned factor, unsigned addend) {
    unsigned r;
    asm("v_mad_u32_u16 %0, %1, %2, %3 op_sel:[1,0,0,0]" : "=v"(r) : "v"(packed), "s"(factor), "v"(addend));
    return r;
}
__device__ __forceinline__ unsigned add_lo16_u(unsigned a, unsigned packed) {
    unsigned r;
    asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0" : "=v"(r) : "v"(a), "v"(packed));
    return r;
}
// 24-bit multiplies with a UNIFORM second factor, spelled out: the compiler takes v_mul_lo_u32 / v_mul_hi_u32 whenever it cannot
// prove both factors below 2^24 (a run-time window stride: K1's vote index, one per event).  `b` must be wave-uniform.
__device__ __forceinline__ unsigned mul24_u(unsigned a, unsigned b) {
    unsigned r;
    asm("v_mul_u32_u24 %0, %1, %2" : "=v"(r) : "s"(b), "v"(a));
    return r;
}
__device__ __forceinline__ unsigned mad24_u(unsigned a, unsigned b, unsigned c) {
    unsigned r;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(b), "v"(c));
    return r;
}
typedef unsigned short ushort2_v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pk_min_u16(unsigned a, unsigned b) {  // v_pk_min_u16: both 16-bit halves at once
    return __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_bit_cast(ushort2_v, a), __builtin_bit_cast(ushort2_v, b)));
}
__device__ __forceinline__ unsigned pk_max_u16(unsigned a, unsigned b) {
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(ushort2_v, a), __builtin_bit_cast(ushort2_v, b)));
}

// ---- wave64 segmented inclusive scan without LDS traffic -------------------------------------------
// ds_bpermute-based __shfl_up costs ~16 cycles per wave instruction on gfx950 and the 6-step scan of
// (x, y, flag) was 60 % of the dense K3 (profiles/r01_ablation.txt).  DPP row shifts run on the VALU:
// 4 steps inside each 16-lane row, then three v_readlane carries across the rows.
// head: 1 on the first lane of every run.  On return (vx, vy) of the LAST lane of a run hold the run's sums.
__device__ __forceinline__ void seg_scan64(int head, float &vx, float &vy, int lane) {
    int f = head;  // "a run starts between my row's first lane and me"
#define CMAX_SEG_STEP(CTRL)                                   \
    {                                                         \
        const float x2 = dpp_f<CTRL>(vx), y2 = dpp_f<CTRL>(vy); \
        const int f2 = dpp_i<CTRL>(0, f);                     \
        if (!f) {                                             \
            vx += x2;                                         \
            vy += y2;                                         \
            f |= f2;                                          \
        }                                                     \
    }
    CMAX_SEG_STEP(kDppRowShr1)
    CMAX_SEG_STEP(kDppRowShr2)
    CMAX_SEG_STEP(kDppRowShr4)
    CMAX_SEG_STEP(kDppRowShr8)
#undef CMAX_SEG_STEP
    // carry the run that crosses a row boundary: lanes of row r without a head before them continue
    // the run ending at the last lane of row r-1 (whose value already contains earlier carries)
#pragma unroll
    for (int r = 1; r < 4; ++r) {
        const float cx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(vx), 16 * r - 1));
        const float cy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(vy), 16 * r - 1));
        if ((lane >> 4) == r && !f) {
            vx += cx;
            vy += cy;
        }
    }
}  // 64 scratch words behind the window: target of masked lanes (branch-free phase B)

// Arrival ticket of a group of workgroups inside one launch: called by ONE thread of workgroup `wg` of `total` after its
// device-scope atomics; true for exactly one caller, the last to arrive, and every other workgroup's atomics have been
// performed by then (the caller waits for its own acknowledgements first).  The counters are left at zero.  Same-line atomics
// serialise, hence kTicketSubs lines + one.  Four dependent fabric round trips (~5 us, profiles/r02_ablation.txt): only for work
// that is NOT at the end of its kernel.
__device__ __forceinline__ bool arrive_last(int *ticket, int wg, int total) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int nsub = total < kTicketSubs ? total : kTicketSubs;
    const int sub = wg % kTicketSubs, per = (total - sub + kTicketSubs - 1) / kTicketSubs;
    int *line = ticket + sub * kTicketLineInts;
    if (__hip_atomic_fetch_add(line, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != per - 1) return false;
    __hip_atomic_store(line, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // nobody else arrives on this line any more
    int *master = ticket + kTicketSubs * kTicketLineInts;
    if (__hip_atomic_fetch_add(master, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != nsub - 1) return false;
    __hip_atomic_store(master, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return true;
}

// loss of a plain variance objective with ONE reference time from accumulators that other workgroups of the same launch
// filled with device-scope atomics: device-scope loads (a plain load may be served from this XCD's L2)
__device__ __forceinline__ void write_result_variance_agent(const ObjParams &op, const double *stat, double *__restrict__ result) {
    double acc[2] = {0.0, 0.0};
    for (int u = 0; u < op.nsub; ++u) {
        acc[0] += __hip_atomic_load(&stat[kSubStride * u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        acc[1] += __hip_atomic_load(&stat[kSubStride * u + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const double v = contrast_value(CMAX_COST_VARIANCE, acc, region_pixels(op.H, op.W, op.omit), nullptr);
    const double loss = op.mult[0] * (op.minimize ? -v : v);
    result[0] = op.negate ? -loss : loss;
    result[1] = v;
    result[5] = 0.0;
}

// (da, db) of cached event slot: d(x', y')/d(motion) . u
template <int MODEL>
__device__ __forceinline__ void tangent_delta(const WarpParams &wp, const TanParams &tp, float dt, unsigned key, float u0, float u1,
                                              float &da, float &db) {
    if (MODEL == CMAX_MODEL_2DOF) {
        da = dt * u0;  // x' = x + dt * theta0
        db = dt * u1;
    } else {
        const int hw = wp.H * wp.W;
        const int ix = (int)(key & 0xFFFu), iy = (int)((key >> 12) & 0xFFFu), bin = (int)(key >> 24);
        const int src = bin * 2 * hw + ix * wp.W + iy;
        da = -dt * tp.u[src];  // x' = x - dt * F[0, ix, iy]
        db = -dt * tp.u[src + hw];
    }
}

// the event kernels
#include "cmax_event_kernels.inc"

__global__ void k_empty(const int4 *) {}  // cmax_debug_launch_floor

// The layout of the event kernels, chosen ONCE per kernel family (each family is instantiated for the layouts its function returns).
// A work list of big / mid segments (up to 4088 / 3064 events) can only be run by the big / mid layouts.
// K1: 512 threads (4 events per thread) once the work list exceeds what the chip holds at once -- as for K3: cfg2 (704 half-tile
// segments) K1 6.35 -> 5.97 us, evaluation 18.06 -> 17.38
static Layout vote_layout(const cmax_handle_s *h) {
    if (h->big) return Layout::b512;
    if (h->mid) return Layout::m512;
    return h->nseg > 512 ? Layout::t512 : Layout::t256;
}
// K3 (not deterministic): as K1, with the voxel K3 at 1024 threads on big segments and above 1024 segments (cfg4: 22.1 us with 512
// threads -> 19.3 us), and at 512 threads with the small accumulator array on owned groups of <= 3 groups per segment (build_segments)
Layout grad_layout(const cmax_handle_s *h, int model, bool owned) {
    const bool voxel = model == CMAX_MODEL_VOXEL;
    if (h->big) return voxel ? Layout::b1024 : Layout::b512;
    if (h->mid) return Layout::m512;
    if (voxel && owned && h->small_acc) return Layout::t512;
    if (voxel && h->nseg > 1024) return Layout::t1024;
    return h->nseg > 512 ? Layout::t512 : Layout::t256;  // K3 hides its latencies better with 8 waves per workgroup (cfg2: 7.5 -> 7.1 us)
}
// deterministic K3, the tangent votes (k_vote_tan, k_vote_tan2) and the second-order gather (k_grad_hvp)
static Layout plain_layout(const cmax_handle_s *h) {
    if (h->big) return Layout::b512;
    if (h->mid) return Layout::m512;
    return Layout::t256;
}

// f(L{}) for the layout L among Ls whose id is `id`
template <class... Ls, class F>
static void with_layout(Layout id, F &&f) {
    const bool found = ((Ls::kId == id ? (f(Ls{}), true) : false) || ...);
    if (!found) std::abort();  // (a choice function returned a layout its family is not instantiated for)
}
// f(std::true_type{}) or f(std::false_type{}): a run-time flag as a template argument
template <class F>
static void with_bool(bool b, F &&f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}
// grid.x of a kernel that finds its segment with segment_of_block: one workgroup per segment, the same number on each of the 8 XCDs
static int seg_blocks(int nseg) { return 8 * ((nseg + 7) / 8); }
// the 6-byte events of the work list from segment seg0 on (one region per segment), or nullptr where the kernels read the 8-byte ones
template <int MODEL>
static const char *compact_events(const cmax_handle_s *h, int seg0 = 0) {
    return (h->compact && h->big && MODEL != CMAX_MODEL_VOXEL) ? h->cev + (int64_t)seg0 * b512::kCompactStride : nullptr;
}
int layout_threads(Layout id) {
    int thr = 0;
    with_layout<t256, t512, t1024, m512, b512, b1024>(id, [&](auto l) { thr = decltype(l)::kThr; });
    return thr;
}

// the arguments every vote and gather of a weighted handle carries (cmax_set_event_weights): objective, cmax_iwe, the un-warped image
static RefArgs weighted_args(const cmax_handle_s *h, const RefArgs &ra_in) {
    RefArgs ra = ra_in;
    if (h->weighted) {
        ra.wgt = h->w_packed;
        ra.wnorm = h->d_wnorm;
    }
    return ra;
}

// WarpParams::normalize / motion_f64 as K1 and K3 take them among their leading parameters (load_head_words)
static int head_flags(const WarpParams &wp) { return (wp.normalize ? kHeadNormalize : 0) | (wp.motion_f64 ? kHeadMotionF64 : 0); }

template <int MODEL>
void launch_vote(cmax_handle_s *h, const EvView &ev, const WarpParams &wp, const RefArgs &ra_in, int n_ref, hipStream_t s, int nz) {
    const dim3 grid(seg_blocks(h->nseg), n_ref, nz);  // z: candidate motions of cmax_objective_batch
    const RefArgs ra = weighted_args(h, ra_in);
    ProfScope prof(h, kProfVote, s);
    const char *cev = compact_events<MODEL>(h);
    auto launch = [&](auto... exact) {  // (an ExactFlow or nothing)
        for (int rep = 0; rep < h->prof_repeat; ++rep)
            with_layout<b512, m512, t512, t256>(vote_layout(h), [&](auto l) {
                using L = decltype(l);
                with_bool(h->has_frac, [&](auto frac) {
                    if (ra.wgt) {  // weighted handle (never with the vote sums: eval_plan)
                        hipLaunchKernelGGL((k_vote<L, MODEL, frac.value, false, true, decltype(exact)...>), grid, dim3(L::kThr), 0, s, h->d_segs, h->nseg, ra.z_motion, ev.ev,
                                           cev, wp.motion, wp.tmm, head_flags(wp), ev, wp, ra, exact...);
                        return;
                    }
                    with_bool(ra.musum[0] != nullptr, [&](auto mu) {
                        hipLaunchKernelGGL((k_vote<L, MODEL, frac.value, mu.value, false, decltype(exact)...>), grid, dim3(L::kThr), 0, s, h->d_segs, h->nseg, ra.z_motion,
                                           ev.ev, cev, wp.motion, wp.tmm, head_flags(wp), ev, wp, ra, exact...);
                    });
                });
            });
    };
    if constexpr (MODEL == CMAX_MODEL_DENSE || MODEL == CMAX_MODEL_VOXEL) {
        if (wp.motion_f64) {  // the caller's fp64 flow, split: the instantiation whose border branch reads the low plane
            launch(ExactFlow{1});
            return;
        }
    }
    launch();
}

// seg0 / seg_n: sub-range of the work list (a band of tile rows, see cmax_comm_set_c2_bands); seg_n < 0 = the whole list.  The
// kernels only see a shifted list (RefArgs::win is shifted by the caller).
// A weighted handle (cmax_set_event_weights) runs the same layouts and variants in their WEIGHTED instantiations, and only the folds of
// the general path (eval_plan sends it through K1 -> statistics -> K3; deterministic mode is refused): the other combinations are
// not instantiated.
template <int MODEL>
void launch_grad(cmax_handle_s *h, const EvView &ev, const WarpParams &wp, const RefArgs &ra_in, int n_ref, int fold,
                 const ObjParams &op, double *gpart, float *gflow, double *result, bool owned, hipStream_t s, int seg0,
                 int seg_n, int nz) {
    if (h->weighted && (fold == kFoldDeferred || fold == kFoldStatsInside || h->deterministic)) std::abort();  // (eval_plan never asks for these)
    const int4 *segs = h->d_segs + seg0;
    const int nseg = seg_n < 0 ? h->nseg : seg_n;
    const dim3 grid(seg_blocks(nseg) + (fold == kFoldStatsInside ? ra_in.stat_blocks : 0), n_ref, nz);
    ProfScope prof(h, kProfGrad, s);
    RefArgs ra = weighted_args(h, ra_in);
    // deferred statistics: the slice of the next evaluation's vote image each workgroup clears, known here once per launch
    const int npix = wp.Hp * wp.Wp;
    ra.zero_chunk = nseg > 0 ? (npix + nseg - 1) / nseg : 0;
    ra.zero_chunk4 = nseg > 0 ? (npix / 4 + nseg - 1) / nseg : 0;
    const char *cev = compact_events<MODEL>(h, seg0);
    // k_grad's head word: the head's flags, the grid's reference times, and above them the candidates' stride (2-DoF) or the statistics
    // workgroups (flow models)
    const int head_payload = MODEL == CMAX_MODEL_2DOF ? ra.z_motion : (fold == kFoldStatsInside ? ra.stat_blocks : 0);
    if (n_ref < 1 || n_ref > 4 || head_payload < 0 || head_payload >= (1 << 26)) std::abort();  // (three bits, 26 bits: what the word has room for)
    const int head_word = head_flags(wp) | n_ref << 2 | head_payload << 5;
    auto launch = [&](auto l, auto frac, auto fold_c, auto variant, auto weighted) {
        using L = decltype(l);
        hipLaunchKernelGGL((k_grad<L, MODEL, frac.value, fold_c.value, variant.value, weighted.value>), grid, dim3(L::kThr), 0, s, segs, nseg, head_word, ev.ev, cev,
                           (const int4 *)ra.win, wp.motion, wp.tmm, ev, wp, ra, op, h->d_stat, gpart, gflow, result);
    };
    if (h->deterministic) {  // one workgroup size, two ways of obtaining dL/dIWE (objective_finish runs the unfused image path)
        with_layout<b512, m512, t256>(plain_layout(h), [&](auto l) {
            with_bool(h->has_frac, [&](auto frac) {
                if (fold == kFoldStats) launch(l, frac, int_c<kFoldStats>{}, int_c<kGradDet>{}, std::false_type{});
                else launch(l, frac, int_c<kFoldNone>{}, int_c<kGradDet>{}, std::false_type{});
            });
        });
        return;
    }
    // dense model: runs of equal source pixel are reduced serially per thread when they are long (pixel-sorted
    // handle, >= 8 events per active pixel), else with a segmented scan per slot over lanes holding consecutive events;
    // owned groups (dense / voxel, one reference time, group-aligned work list): LDS accumulators + plain stores
    const bool strided = MODEL == CMAX_MODEL_DENSE && !(h->long_runs && h->n_time_bin == 0);
    // voxel, owned groups of <= 3 groups per segment: the small accumulator array (grad_layout: 512 threads x 4 events, or mid segments)
    const bool small = MODEL == CMAX_MODEL_VOXEL && owned && h->small_acc && !h->big;
    auto body = [&](auto l) {
        using L = decltype(l);
        with_bool(h->weighted, [&](auto weighted) {
            constexpr bool kWeighted = decltype(weighted)::value;
            auto with_variant = [&](auto frac, auto fold_c) {
                if constexpr (MODEL == CMAX_MODEL_DENSE) {
                    if (owned) launch(l, frac, fold_c, int_c<kGradOwned>{}, weighted);
                    else if (strided) launch(l, frac, fold_c, int_c<kGradStrided>{}, weighted);
                    else launch(l, frac, fold_c, int_c<kGradRuns>{}, weighted);
                } else if constexpr (MODEL == CMAX_MODEL_VOXEL) {
                    if (owned && small) {
                        if constexpr (L::kThr == 512 && L::kSlots <= 3072) launch(l, frac, fold_c, int_c<kGradOwnedSmall>{}, weighted);
                    } else if (owned) {
                        launch(l, frac, fold_c, int_c<kGradOwned>{}, weighted);
                    } else {
                        launch(l, frac, fold_c, int_c<kGradRuns>{}, weighted);
                    }
                } else {
                    launch(l, frac, fold_c, int_c<kGradRuns>{}, weighted);
                }
            };
            with_bool(h->has_frac, [&](auto frac) {
                if (fold == kFoldDeferred) {
                    if constexpr (MODEL == CMAX_MODEL_2DOF && !kWeighted) with_variant(frac, int_c<kFoldDeferred>{});
                } else if (fold == kFoldStatsInside) {
                    if constexpr (MODEL != CMAX_MODEL_2DOF && !kWeighted) with_variant(frac, int_c<kFoldStatsInside>{});
                } else if (fold == kFoldStats) {
                    with_variant(frac, int_c<kFoldStats>{});
                } else if (fold == kFoldScale) {
                    with_variant(frac, int_c<kFoldScale>{});
                } else {
                    with_variant(frac, int_c<kFoldNone>{});
                }
            });
        });
    };
    for (int rep = 0; rep < h->prof_repeat; ++rep) {
        if constexpr (MODEL == CMAX_MODEL_VOXEL) with_layout<b1024, m512, t512, t1024, t256>(grad_layout(h, MODEL, owned), body);
        else with_layout<b512, m512, t512, t256>(grad_layout(h, MODEL, owned), body);
    }
}

// The launch form of the per-event gathers (K3w, K3e) over n_img images: K1's grid, events and layout (launch_vote), whose windows
// they read.  f(L{}, frac, grid, cev) launches the kernel.
template <int MODEL, class F>
static void launch_gather(cmax_handle_s *h, int n_img, F &&f) {
    const dim3 grid(seg_blocks(h->nseg), n_img);
    const char *cev = compact_events<MODEL>(h);
    with_layout<b512, m512, t512, t256>(vote_layout(h), [&](auto l) { with_bool(h->has_frac, [&](auto frac) { f(l, frac, grid, cev); }); });
}

// K3w of n_img images (MODEL >= 0: the reference times of the objective; -1: the un-warped events) into planes plane0 ..
template <int MODEL>
void launch_weight_gather(cmax_handle_s *h, const EvView &ev, const WarpParams &wp, const RefArgs &ra, int n_img, int plane0, hipStream_t s) {
    launch_gather<MODEL>(h, n_img, [&](auto l, auto frac, dim3 grid, const char *cev) {
        using L = decltype(l);
        hipLaunchKernelGGL((k_weight_gather<L, MODEL, frac.value>), grid, dim3(L::kThr), 0, s, h->d_segs, h->nseg, ev.ev, cev, (const int4 *)ra.win, ev, wp, ra,
                           h->gw_packed + (int64_t)plane0 * h->gw_plane, h->gw_plane);
    });
}

// K3e of n_img images (MODEL >= 0: the reference times of the objective; -1: the un-warped events) into planes plane0 ..
template <int MODEL>
void launch_event_gather(cmax_handle_s *h, const EvView &ev, const WarpParams &wp, const RefArgs &ra_in, int n_img, int plane0, hipStream_t s) {
    RefArgs ra = ra_in;
    if (h->weighted) ra.wgt = h->w_packed;
    launch_gather<MODEL>(h, n_img, [&](auto l, auto frac, dim3 grid, const char *cev) {
        using L = decltype(l);
        with_bool(h->weighted, [&](auto wgt) {
            hipLaunchKernelGGL((k_event_grad_gather<L, MODEL, frac.value, wgt.value>), grid, dim3(L::kThr), 0, s, h->d_segs, h->nseg, ev.ev, cev, (const int4 *)ra.win, ev,
                               wp, ra, h->ge_packed + (int64_t)plane0 * h->ge_plane, h->ge_plane);
        });
    });
}

// tangent votes of every reference time (blockIdx.y) into draw + k * tp.bs (zeroed by the caller); draw64: the integer images of
// deterministic mode.  A weighted handle passes its weights behind them (a weighted deterministic handle is refused at every entry).
template <int MODEL>
void launch_vote_tan(cmax_handle_s *h, const EvView &ev, const WarpParams &wp, const TanParams &tp, int n_ref, float *draw, hipStream_t s,
                     long long *draw64) {
    if (h->weighted && draw64) std::abort();
    const dim3 grid(seg_blocks(h->nseg), n_ref);
    auto launch = [&](auto... exact) {  // (an ExactFlow or nothing, as in launch_vote)
        with_layout<b512, m512, t256>(plain_layout(h), [&](auto l) {
            using L = decltype(l);
            with_bool(h->has_frac, [&](auto frac) {
                if (h->weighted)
                    hipLaunchKernelGGL((k_vote_tan<L, MODEL, frac.value, const float *, const float *, decltype(exact)...>), grid, dim3(L::kThr), 0, s, ev, wp, tp, h->d_segs,
                                       h->nseg, draw, h->d_stat_tan, draw64, (const float *)h->w_packed, (const float *)h->d_wnorm, exact...);
                else
                    hipLaunchKernelGGL((k_vote_tan<L, MODEL, frac.value, decltype(exact)...>), grid, dim3(L::kThr), 0, s, ev, wp, tp, h->d_segs, h->nseg, draw, h->d_stat_tan,
                                       draw64, exact...);
            });
        });
    };
    if constexpr (MODEL == CMAX_MODEL_DENSE || MODEL == CMAX_MODEL_VOXEL) {
        if (wp.motion_f64) {
            launch(ExactFlow{1});
            return;
        }
    }
    launch();
}

// det: the integer accumulators of deterministic mode (HvpDet{} otherwise); weights as launch_vote_tan
template <int MODEL>
void launch_grad_hvp(cmax_handle_s *h, const EvView &ev, const WarpParams &wp, const TanParams &tp, int n_ref, const float *G,
                     const float *Gp, double *gpart, float *hflow, hipStream_t s, const HvpDet &det) {
    if (h->weighted && h->deterministic) std::abort();
    const dim3 grid(seg_blocks(h->nseg), n_ref);
    auto launch = [&](auto... exact) {  // (an ExactFlow or nothing, as in launch_vote)
        with_layout<b512, m512, t256>(plain_layout(h), [&](auto l) {
            using L = decltype(l);
            with_bool(h->has_frac, [&](auto frac) {
                if (h->weighted)
                    hipLaunchKernelGGL((k_grad_hvp<L, MODEL, frac.value, const float *, decltype(exact)...>), grid, dim3(L::kThr), 0, s, ev, wp, tp, h->d_segs, h->nseg, G, Gp, gpart,
                                       hflow, det, (const float *)h->w_packed, exact...);
                else
                    hipLaunchKernelGGL((k_grad_hvp<L, MODEL, frac.value, decltype(exact)...>), grid, dim3(L::kThr), 0, s, ev, wp, tp, h->d_segs, h->nseg, G, Gp, gpart, hflow, det,
                                       exact...);
            });
        });
    };
    if constexpr (MODEL == CMAX_MODEL_DENSE || MODEL == CMAX_MODEL_VOXEL) {
        if (wp.motion_f64) {
            launch(ExactFlow{1});
            return;
        }
    }
    launch();
}

// 2-DoF tangent images of every reference time (blockIdx.y) into ra.img[k] (I | E0 | F1 planes, zeroed by the caller)
void launch_vote_tan2(cmax_handle_s *h, const EvView &ev, const WarpParams &wp, const RefArgs &ra, int n_ref, hipStream_t s) {
    const dim3 grid(seg_blocks(h->nseg), n_ref);
    ProfScope prof(h, kProfVote, s);
    for (int rep = 0; rep < h->prof_repeat; ++rep) {
        with_layout<b512, m512, t256>(plain_layout(h), [&](auto l) {
            using L = decltype(l);
            with_bool(h->has_frac, [&](auto frac) {
                hipLaunchKernelGGL((k_vote_tan2<L, frac.value>), grid, dim3(L::kThr), 0, s, h->d_segs, h->nseg, ev, wp, ra);
            });
        });
    }
}

// the compact copy of the sorted events, one region per segment of the current work list (build_segments, cmax_batch.hip)
int pack_compact_events(cmax_handle_s *h, hipStream_t s) {
    int rc = h->cev.reserve(&h->bytes, (int64_t)h->nseg * b512::kCompactStride, s);
    if (rc) return rc;
    hipLaunchKernelGGL((k_pack_compact<b512>), dim3(h->nseg), dim3(b512::kThr), 0, s, (const int4 *)h->d_segs, h->nseg, (const uint2 *)h->evp, h->ntc,
                       h->cev, h->d_flags + 3);
    CMAX_CHECK_HIP(hipGetLastError());
    return 0;
}
int64_t compact_region_bytes() { return b512::kCompactStride; }

// The models today's call sites use: every launcher for the three motion models, the vote and the per-event gathers for the
// un-warped image (MODEL = -1) as well.
#define CMAX_INSTANTIATE_LAUNCHERS(MODEL)                                                                                                     \
    template void launch_vote<MODEL>(cmax_handle_s *, const EvView &, const WarpParams &, const RefArgs &, int, hipStream_t, int);           \
    template void launch_weight_gather<MODEL>(cmax_handle_s *, const EvView &, const WarpParams &, const RefArgs &, int, int, hipStream_t);  \
    template void launch_event_gather<MODEL>(cmax_handle_s *, const EvView &, const WarpParams &, const RefArgs &, int, int, hipStream_t);
#define CMAX_INSTANTIATE_MODEL_LAUNCHERS(MODEL)                                                                                               \
    CMAX_INSTANTIATE_LAUNCHERS(MODEL)                                                                                                         \
    template void launch_grad<MODEL>(cmax_handle_s *, const EvView &, const WarpParams &, const RefArgs &, int, int, const ObjParams &, double *, float *, double *, bool, \
                                     hipStream_t, int, int, int);                                                                             \
    template void launch_vote_tan<MODEL>(cmax_handle_s *, const EvView &, const WarpParams &, const TanParams &, int, float *, hipStream_t, long long *); \
    template void launch_grad_hvp<MODEL>(cmax_handle_s *, const EvView &, const WarpParams &, const TanParams &, int, const float *, const float *, double *, float *, \
                                         hipStream_t, const HvpDet &);
CMAX_INSTANTIATE_LAUNCHERS(-1)
CMAX_INSTANTIATE_MODEL_LAUNCHERS(CMAX_MODEL_2DOF)
CMAX_INSTANTIATE_MODEL_LAUNCHERS(CMAX_MODEL_DENSE)
CMAX_INSTANTIATE_MODEL_LAUNCHERS(CMAX_MODEL_VOXEL)
#undef CMAX_INSTANTIATE_MODEL_LAUNCHERS
#undef CMAX_INSTANTIATE_LAUNCHERS

}  // namespace cmax

using namespace cmax;

extern "C" {

// tools/timeline.py: where the event kernels record their phase stamps (device buffer of 2 x 4096 x 8 u64; NULL: off).  Only
// libraries built with -DCMAX_TIMELINE record anything; the others return CMAX_ESTATE.
int cmax_debug_timeline(void *device_buffer) {
#ifdef CMAX_TIMELINE
    unsigned long long *p = static_cast<unsigned long long *>(device_buffer);
    const int rc = timeline_set(p);  // K1 / K3
    return rc ? rc : image_timeline_set(p);  // ... and the fused image kernel between them (cmax_fused.hip)
#else
    (void)device_buffer;
    set_error("debug_timeline: this library was built without -DCMAX_TIMELINE");
    return CMAX_ESTATE;
#endif
}

// Launch floor of the current work list: `pairs` times two dependent EMPTY launches with the grids of K1 and K3 of a single-reference
// objective on this batch (the launch structure of the headline evaluation).  bench.py brackets it with events: what the evaluation
// would cost if its kernels did nothing (profiles/r03_launch_floor.txt measured the same with tools/microbench_launch.hip).
int cmax_debug_launch_floor(cmax_handle_t h, int pairs, cmax_stream_t stream) {
    CMAX_REQUIRE(h != nullptr && pairs > 0, "debug_launch_floor");
    CMAX_REQUIRE(h->n > 0 && h->nseg > 0, "debug_launch_floor: no events set");
    const dim3 grid(seg_blocks(h->nseg));
    const int k1 = layout_threads(vote_layout(h)), k3 = layout_threads(grad_layout(h, CMAX_MODEL_2DOF, false));
    for (int i = 0; i < pairs; ++i) {
        hipLaunchKernelGGL(k_empty, grid, dim3(k1), 0, (hipStream_t)stream, h->d_segs);
        hipLaunchKernelGGL(k_empty, grid, dim3(k3), 0, (hipStream_t)stream, h->d_segs);
    }
    CMAX_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
