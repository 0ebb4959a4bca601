// Patch grid -> dense flow and its adjoint, shared by the leaf operator (cmax_flow.hip) and the patch-objective
// plan (cmax_solver.hip).
#pragma once
#include "cmax_common.h"

namespace cmax {

// ---------------------------------------------------------------------------------------------
// Patch grid -> dense flow and its adjoint (interpolate_dense_flow_from_patch_tensor,
// src/solver/patch_contrast_base.py:462-506): negate, replicate-pad by (pad_h, pad_w), bilinear x
// (sw_h, sw_w) with align_corners=False, centre-crop to [H, W].
// patch.filter_type "nearest" (lines 494-495, template argument F = CMAX_FILTER_NEAREST): the resize takes, for pixel (r, c) of
// the up-sampled array, padded cell (r / sw_h, c / sw_w) -- the index rule of nearest-neighbour resizing by an integer factor.
// The forward is a negated copy (exact in both dtypes); in the adjoint a cell owns ONE clipped rectangle of the output.
// F = CMAX_FILTER_BILINEAR compiles to the code these kernels had before the argument existed.
// ---------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void bilin_tap(int dst, int scale, int n_in, int &i0, int &i1, T &lam) {
    T src = ((T)dst + (T)0.5) / (T)scale - (T)0.5;
    if (src < (T)0) src = (T)0;
    int a = (int)floor_t<T>(src);
    if (a > n_in - 1) a = n_in - 1;
    i0 = a;
    i1 = a + 1 < n_in ? a + 1 : n_in - 1;
    lam = src - (T)a;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// value of the dense flow at flat index p of [2,H,W]
template <typename T, int F = CMAX_FILTER_BILINEAR>
__device__ __forceinline__ T patch_interp(const T *__restrict__ motion, int ph, int pw, int pad_h, int pad_w, int sw_h, int sw_w, int H, int W,
                                          int64_t p) {
    const int c = (int)(p / ((int64_t)H * W));
    const int64_t q = p % ((int64_t)H * W);
    const int i = (int)(q / W), j = (int)(q % W);
    const int gh = ph + 2 * pad_h, gw = pw + 2 * pad_w;
    const int h1 = (gh * sw_h) / 2 - H / 2, w1 = (gw * sw_w) / 2 - W / 2;  // lines 501-505
    if constexpr (F == CMAX_FILTER_NEAREST) {
        // padded cell of the pixel, then the replicate padding: the clamp onto the grid
        const int R = clampi((i + h1) / sw_h, 0, gh - 1), C = clampi((j + w1) / sw_w, 0, gw - 1);
        return -motion[(int64_t)c * ph * pw + (int64_t)clampi(R - pad_h, 0, ph - 1) * pw + clampi(C - pad_w, 0, pw - 1)];
    }
    int r0, r1, c0, c1;
    T lr, lc;
    bilin_tap<T>(i + h1, sw_h, gh, r0, r1, lr);
    bilin_tap<T>(j + w1, sw_w, gw, c0, c1, lc);
    const T *m = motion + (int64_t)c * ph * pw;
    auto PM = [&](int R, int C) { return -m[(int64_t)clampi(R - pad_h, 0, ph - 1) * pw + clampi(C - pad_w, 0, pw - 1)]; };
    return ((T)1 - lr) * (((T)1 - lc) * PM(r0, c0) + lc * PM(r0, c1)) + lr * (((T)1 - lc) * PM(r1, c0) + lc * PM(r1, c1));
}

// TOut / scale: the plan writes the fp32 motion of the fused objective (flow * t_scale) straight from the fp64 patch grid
template <typename T, typename TOut = T, int F = CMAX_FILTER_BILINEAR>
__global__ void __launch_bounds__(256)
k_patch_to_dense(const T *__restrict__ motion, int ph, int pw, int pad_h, int pad_w, int sw_h, int sw_w, int H, int W,
                 TOut *__restrict__ flow, T scale = (T)1) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= 2 * (int64_t)H * W) return;
    const T v = patch_interp<T, F>(motion, ph, pw, pad_h, pad_w, sw_h, sw_w, H, W, p);
    flow[p] = (TOut)(v * scale);
}

// adjoint, gather form: one workgroup per patch cell sums the contributions of every output pixel
// whose taps touch the cell (no atomics: the motion gradient has only 2*ph*pw entries).
// Nearest filter: the cell's pixels are the rows [Rlo sw_h, (Rhi + 1) sw_h) x columns [Clo sw_w, (Chi + 1) sw_w) of the up-sampled
// array (a border cell takes the replicate padding's share along), cropped to the sensor; each thread adds its pixels in index order
// and block_sum adds the threads in a fixed order, so two runs agree bit for bit.
template <typename T, int F = CMAX_FILTER_BILINEAR>
__global__ void __launch_bounds__(256)
k_patch_to_dense_adj(const T *__restrict__ gflow, int ph, int pw, int pad_h, int pad_w, int sw_h, int sw_w, int H, int W,
                     T *__restrict__ gmotion) {
    __shared__ double smem[4];
    const int cell = blockIdx.x;  // c * ph * pw + pr * pw + pc
    const int c = cell / (ph * pw), pr = (cell / pw) % ph, pc = cell % pw;
    const int gh = ph + 2 * pad_h, gw = pw + 2 * pad_w;
    const int h1 = (gh * sw_h) / 2 - H / 2, w1 = (gw * sw_w) / 2 - W / 2;
    // padded rows that map to patch row pr: [Rlo, Rhi]; output rows with a tap on them lie in a band around
    const int Rlo = pr == 0 ? 0 : pr + pad_h, Rhi = pr == ph - 1 ? gh - 1 : pr + pad_h;
    const int Clo = pc == 0 ? 0 : pc + pad_w, Chi = pc == pw - 1 ? gw - 1 : pc + pad_w;
    if constexpr (F == CMAX_FILTER_NEAREST) {
        const int i_lo = max(Rlo * sw_h - h1, 0), i_hi = min((Rhi + 1) * sw_h - h1, H);
        const int j_lo = max(Clo * sw_w - w1, 0), j_hi = min((Chi + 1) * sw_w - w1, W);
        // a cell off the sensor on either axis: an empty rectangle, never a negative extent (see the bilinear band below)
        const int bw = max(j_hi - j_lo, 0), bh = max(i_hi - i_lo, 0);
        double acc[1] = {0.0};
        for (int t = threadIdx.x; t < bw * bh; t += blockDim.x)
            acc[0] -= (double)gflow[(int64_t)c * H * W + (int64_t)(i_lo + t / bw) * W + (j_lo + t % bw)];
        block_sum<1>(acc, smem);
        if (threadIdx.x == 0) gmotion[cell] = (T)acc[0];
        return;
    }
    const int i_lo = max((Rlo - 1) * sw_h - h1 - 1, 0), i_hi = min((Rhi + 2) * sw_h - h1 + 1, H);
    const int j_lo = max((Clo - 1) * sw_w - w1 - 1, 0), j_hi = min((Chi + 2) * sw_w - w1 + 1, W);
    // a cell of a grid that reaches far beyond the sensor has no pixel on one axis or on both: an empty band, not a negative one
    // (the product of two negative extents would walk rows and columns outside the image)
    const int bw = max(j_hi - j_lo, 0), bh = max(i_hi - i_lo, 0);
    double acc[1] = {0.0};
    for (int t = threadIdx.x; t < bw * bh; t += blockDim.x) {
        const int i = i_lo + t / bw, j = j_lo + t % bw;
        int r0, r1, c0, c1;
        T lr, lc;
        bilin_tap<T>(i + h1, sw_h, gh, r0, r1, lr);
        bilin_tap<T>(j + w1, sw_w, gw, c0, c1, lc);
        const T wr = (clampi(r0 - pad_h, 0, ph - 1) == pr ? (T)1 - lr : (T)0) + (clampi(r1 - pad_h, 0, ph - 1) == pr ? lr : (T)0);
        const T wc = (clampi(c0 - pad_w, 0, pw - 1) == pc ? (T)1 - lc : (T)0) + (clampi(c1 - pad_w, 0, pw - 1) == pc ? lc : (T)0);
        acc[0] += (double)(-gflow[(int64_t)c * H * W + (int64_t)i * W + j] * wr * wc);
    }
    block_sum<1>(acc, smem);
    if (threadIdx.x == 0) gmotion[cell] = (T)acc[0];
}


// ---------------------------------------------------------------------------------------------
// Signed maximum of a field (`scale = dense_flow.max()` of the scale_later map, patch_contrast_pyramid.py:489-490).
// A double as an unsigned key whose order is the order of the values: negative numbers have all bits flipped, the
// others the sign bit set (k_absmax of cmax_solver.hip compares raw bit patterns, which orders non-negative values only).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long ordered_key(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double ordered_value(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}

// Maximum over the calling workgroup (256 threads), valid in every thread
__device__ __forceinline__ double block_max(double m) {
    __shared__ double s_m[256 / kWave];
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, kWave));
    if ((threadIdx.x & (kWave - 1)) == 0) s_m[threadIdx.x / kWave] = m;
    __syncthreads();
    return fmax(fmax(s_m[0], s_m[1]), fmax(s_m[2], s_m[3]));
}

// Maximum of a field whose workgroups hold `m` each, one atomic per workgroup (few workgroups: equal-address atomics
// serialise); returns true in thread 0 of the LAST workgroup of the grid to arrive, which then holds the maximum of the whole
// field in `field_max` and has reset *key and *arrived to 0 for the next launch (both start as 0: below the key of every value).
__device__ __forceinline__ bool grid_max_last(double m, unsigned long long *key, unsigned int *arrived, double &field_max) {
    m = block_max(m);
    if (threadIdx.x != 0) return false;
    atomicMax(key, ordered_key(m));
    __threadfence();
    if (atomicAdd(arrived, 1u) != gridDim.x - 1) return false;
    __threadfence();
    field_max = ordered_value(atomicExch(key, 0ull));
    atomicExch(arrived, 0u);
    return true;
}

}  // namespace cmax
