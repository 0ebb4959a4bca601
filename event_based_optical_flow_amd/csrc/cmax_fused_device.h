// Device helpers of the fused objective that BOTH the event kernels (cmax_event_launch.hip) and the image-side kernels
// (cmax_fused.hip) use: templates and inline device functions only -- no kernel lives here (every kernel is compiled in one unit).
#pragma once

#include "cmax_fused_internal.h"

namespace cmax {

// Phase timeline of the event kernels (builds with -DCMAX_TIMELINE only, tools/timeline.py): thread 0 of the first 4096 workgroups of
// reference time 0 stamps the 100 MHz wall clock at the phase boundaries of K1 (kernel 0) and K3 (kernel 1) into
// g_timeline[kernel][workgroup][8] (round 6: kernel 2 = the fused image kernel between them); a stamp that is to follow the arrival of
// loaded data is handed a value computed from it.  A __device__ variable belongs to the unit whose kernels write it: each of the two
// units holds its own copy of the pointer, and cmax_debug_timeline (cmax_event_launch.hip) sets both.
#ifdef CMAX_TIMELINE
static __device__ unsigned long long *g_timeline = nullptr;
static inline int timeline_set(unsigned long long *buffer) {  // this unit's copy
    CMAX_CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_timeline), &buffer, sizeof(buffer)));
    return 0;
}
__device__ __forceinline__ void timeline_stamp(int kernel, int idx) {
    if (g_timeline && threadIdx.x == 0 && blockIdx.y == 0 && blockIdx.x < 4096u) g_timeline[((size_t)kernel * 4096 + blockIdx.x) * 8 + idx] = wall_clock64();
}
template <typename T>
__device__ __forceinline__ void timeline_stamp_after(int kernel, int idx, T dep) {
    asm volatile("" ::"v"(dep));
    timeline_stamp(kernel, idx);
}
#define CMAX_STAMP(K, I) cmax::timeline_stamp(K, I)
#define CMAX_STAMP_AFTER(K, I, DEP) cmax::timeline_stamp_after(K, I, DEP)
#else
#define CMAX_STAMP(K, I) do { } while (0)
#define CMAX_STAMP_AFTER(K, I, DEP) do { } while (0)
#endif

// Compiler barrier on a loaded value.  `x = cond ? p[i] : 0` -- and even an unconditional load whose only use is such a
// select -- is compiled into an exec-masked block that holds the load AND its s_waitcnt: a thread that wants four loads in flight
// gets four dependent round trips to memory (found in round 3 in the ISA of K1 / K3 / k_stats: profiles/r03_ablation.txt).  Load
// unconditionally (clamped index), pin() every value, select afterwards: the loads are then issued back to back.
__device__ __forceinline__ void pin(float &v) { asm volatile("" : "+v"(v)); }

// 16 bytes of zeros, written through the L2 (sc1): see the deferred-statistics K3
typedef float float4_v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store_zero4_sc1(float *p) {
    const float4_v z = {0.f, 0.f, 0.f, 0.f};
    asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(z) : "memory");
}

// Clears n floats at `base`, the launch's threads striding over it (tid of nthreads), with write-through stores:
// buffers that the NEXT kernels fill with device-scope atomics (vote images, the flow gradient) must not stay
// parked in an XCD's L2.  16-byte stores when the buffer allows it.
__device__ __forceinline__ void zero_fill_sc1(float *base, int64_t n, int64_t tid, int64_t nthreads) {
    if (!base) return;
    if ((n & 3) == 0 && (reinterpret_cast<uintptr_t>(base) & 15u) == 0) {
        for (int64_t q = tid; q < (n >> 2); q += nthreads) store_zero4_sc1(base + 4 * q);
    } else {
        for (int64_t q = tid; q < n; q += nthreads) __hip_atomic_store(&base[q], 0.f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// DPP row shifts and broadcasts: cross-lane moves on the VALU (ds_bpermute-based shuffles cost ~16 cycles per wave instruction on gfx950)
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {  // lanes whose source is outside the row / wave read 0
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
template <int CTRL>
__device__ __forceinline__ int dpp_i(int old, int v) {
    return __builtin_amdgcn_update_dpp(old, v, CTRL, 0xF, 0xF, false);
}
template <int CTRL>
__device__ __forceinline__ unsigned dpp_u0(unsigned v) {  // lanes without a source read 0 (bound_ctrl: no move of the identity first)
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}
constexpr int kDppRowShr1 = 0x111, kDppRowShr2 = 0x112, kDppRowShr4 = 0x114, kDppRowShr8 = 0x118;
constexpr int kDppWaveShl1 = 0x130, kDppWaveShr1 = 0x138, kDppRowBcast15 = 0x142, kDppRowBcast31 = 0x143;

// raw contrast from the summed accumulators (variance: unbiased like torch.var, image_variance.py:55)
__device__ __forceinline__ double contrast_value(int cost, const double *acc, double npix, double *mu_out) {
    if (cost == CMAX_COST_VARIANCE) {
        const double mu = acc[0] / npix;
        if (mu_out) *mu_out = mu;
        return (acc[1] - acc[0] * mu) / (npix - 1.0);
    }
    return acc[0] / npix;
}

__device__ __forceinline__ double region_pixels(int H, int W, int omit) {
    const int i0 = omit ? 1 : 0;
    return (double)(H - 2 * i0) * (double)(W - 2 * i0);
}

// sum of the sub-accumulators of one slot.  WAVE: called by a whole converged wave -- lane u loads accumulator u,
// DPP reduction, broadcast from lane 63 (a serial walk over up to 32 addresses costs the event kernels 2-4 us of
// dependent scalar-load latency at the head of every workgroup).
template <bool WAVE = false>
__device__ __forceinline__ void stat_sum(const double *__restrict__ stat, int slot, int nsub, double (&acc)[2]) {
    if (WAVE) {
        const int lane = threadIdx.x & (kWave - 1);
        double a0 = 0.0, a1 = 0.0;
        if (lane < nsub) {
            a0 = stat[slot * kStatStride + kSubStride * lane];
            a1 = stat[slot * kStatStride + kSubStride * lane + 1];
        }
        a0 = wave_sum_lane63(a0);
        a1 = wave_sum_lane63(a1);
        acc[0] = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(a0), kWave - 1), __builtin_amdgcn_readlane(__double2loint(a0), kWave - 1));
        acc[1] = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(a1), kWave - 1), __builtin_amdgcn_readlane(__double2loint(a1), kWave - 1));
        return;
    }
    acc[0] = 0.0;
    acc[1] = 0.0;
    for (int u = 0; u < nsub; ++u) {
        acc[0] += stat[slot * kStatStride + kSubStride * u];
        acc[1] += stat[slot * kStatStride + kSubStride * u + 1];
    }
}

template <bool WAVE = false>
__device__ __forceinline__ double orig_value(const ObjParams &op, const double *stat) {
    // orig_iwe is NOT boundary-cropped for the variance (normalized_image_variance.py:40-41)
    const int omit_o = op.cost == CMAX_COST_VARIANCE ? 0 : op.omit;
    double acc[2];
    stat_sum<WAVE>(stat, 4, op.nsub, acc);
    return contrast_value(op.cost, acc, region_pixels(op.H, op.W, omit_o), nullptr);
}

// dL/dv_k: chain factor of reference time k, and the mean of its image (variance)
template <bool WAVE = false>
__device__ __forceinline__ double chain_coef(const ObjParams &op, const double *stat, int k, double *mu_out) {
    const double npix = region_pixels(op.H, op.W, op.omit);
    if (!op.normalized && op.cost != CMAX_COST_VARIANCE) {  // constant factor, no mean: the statistics are not needed
        const double c = op.mult[k] * (op.minimize ? -1.0 : 1.0);
        return op.negate ? -c : c;
    }
    double acc[2];
    stat_sum<WAVE>(stat, k, op.nsub, acc);
    const double v = contrast_value(op.cost, acc, npix, mu_out);
    double coef;
    if (!op.normalized) coef = op.mult[k] * (op.minimize ? -1.0 : 1.0);
    else {
        const double v_orig = orig_value<WAVE>(op, stat);
        coef = op.mult[k] * (op.minimize ? -v_orig / (v * v) : 1.0 / v_orig);
    }
    return op.negate ? -coef : coef;
}

// loss and per-reference-time contrasts -> result[0..5].  WAVE: called by a whole converged wave (the accumulators of a slot
// are gathered in ONE round trip instead of a serial walk over their cache lines); its first lane writes.
template <bool WAVE = false>
__device__ __forceinline__ void write_result(const ObjParams &op, const double *stat, double *__restrict__ result) {
    const double npix = region_pixels(op.H, op.W, op.omit);
    const double v_orig = op.normalized ? orig_value<WAVE>(op, stat) : 0.0;
    const bool writer = !WAVE || (threadIdx.x & (kWave - 1)) == 0;
    double loss = 0.0;
    for (int k = 0; k < op.n_ref; ++k) {
        double acc[2];
        stat_sum<WAVE>(stat, k, op.nsub, acc);
        const double v = contrast_value(op.cost, acc, npix, nullptr);
        if (writer) result[1 + k] = v;
        if (!op.normalized) loss += op.mult[k] * (op.minimize ? -v : v);
        else loss += op.mult[k] * (op.minimize ? v_orig / v : v / v_orig);
    }
    if (writer) {
        result[0] = op.negate ? -loss : loss;
        result[5] = v_orig;
    }
}

// ---------------------------------------------------------------------------------------------
// deterministic mode: fixed-point conversions
// ---------------------------------------------------------------------------------------------
// power-of-two scale s with  bound * n * s < 2^61: n terms of magnitude <= bound fit a 64-bit accumulator
// (n counted as at least 2048: a single term then stays below 2^50 and det_fixed's conversion is exact)
__device__ __forceinline__ double det_scale(double bound, long long n) {
    int e = 0;
    (void)frexp(bound * (double)(n > 2048 ? n : 2048), &e);  // bound n = f 2^e, f in [0.5, 1); 0 -> e = 0
    if (!(bound >= 0.0) || e > 1000) e = 1000;         // NaN / inf: any finite scale
    return ldexp(1.0, 60 - e);
}
// rint(x * s) as a 64-bit integer for |x s| < 2^51: x s + 1.5 2^52 carries the rounded integer in its low mantissa bits (one fma
// + a 64-bit subtraction; __double2ll_rn is a ~25-instruction sequence on gfx950, twice per event in the deterministic K3)
__device__ __forceinline__ long long det_fixed(double x, double s) {
    const double magic = 6755399441055744.0;  // 1.5 * 2^52
    return __double_as_longlong(fma(x, s, magic)) - __double_as_longlong(magic);
}
__device__ __forceinline__ void atomic_add_i64(long long *p, long long v) {
    atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);  // two's complement: wrap-around add
}

}  // namespace cmax
