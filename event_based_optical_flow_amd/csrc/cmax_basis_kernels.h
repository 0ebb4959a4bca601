// Flow basis -> dense flow and its adjoint: D = sum_k theta_k B_k with B [K][2][H][W], the map of every motion model that is LINEAR
// in its parameters (similarity, affine, the rotational motion field of a calibrated camera, a polynomial / PCA / learned basis).
// Shared by the leaf operator cmax_basis_to_dense and the basis plan (cmax_basis_plan_create), both in cmax_solver.hip.
//
// The reference has NO counterpart: its motion models are the 2-DoF translation, the per-pixel flow and the patch grid.  What the
// model composes with is the reference's dense-flow warp rule, x' = x - dt * D[src] (src/warp.py:263-313) -- the basis only says where
// D comes from, as the patch interpolation (cmax_patch_kernels.h) does for the patch grid.
#pragma once
#include "cmax_common.h"

namespace cmax {

constexpr int kBasisMaxK = CMAX_BASIS_MAX_K;
constexpr int kBasisAdjChunk = CMAX_BASIS_ADJ_CHUNK;  // elements of [2,H,W] one workgroup of k_basis_adj owns
constexpr int kBasisAdjPerThread = kBasisAdjChunk / 256;
constexpr int kBasisAdjTile = 4;  // basis fields reduced per pass over the workgroup's chunk
static_assert(kBasisAdjChunk % 256 == 0, "a chunk is a whole number of elements per thread");

// fp64 sum over k = 0 .. K-1, in that order, of theta_k B_k[e] (theta is wave-uniform; for each k the loads are coalesced in e)
template <typename TB>
__device__ __forceinline__ double basis_sum(const double *__restrict__ theta, const TB *__restrict__ basis, int K, int64_t n, int64_t e) {
    double acc = 0.0;
    int k = 0;
    for (; k + 4 <= K; k += 4) {  // four independent loads in flight, added in index order
        const double b0 = (double)basis[(int64_t)k * n + e], b1 = (double)basis[(int64_t)(k + 1) * n + e];
        const double b2 = (double)basis[(int64_t)(k + 2) * n + e], b3 = (double)basis[(int64_t)(k + 3) * n + e];
        acc += theta[k] * b0;
        acc += theta[k + 1] * b1;
        acc += theta[k + 2] * b2;
        acc += theta[k + 3] * b3;
    }
    for (; k < K; ++k) acc += theta[k] * (double)basis[(int64_t)k * n + e];
    return acc;
}

// out[e] = scale [* *scale_dev] * sum_k theta_k B_k[e], e < n = 2 H W; rounded to TO once.  theta: fp64 in device memory (the plan's
// x64: the descent's iterate is read in place); scale_dev as in k_convert_scale (a scalar that changes between replays of a graph).
template <typename TB, typename TO>
__global__ void __launch_bounds__(256)
k_basis_to_dense(const double *__restrict__ theta, const TB *__restrict__ basis, int K, int64_t n, double scale, const double *__restrict__ scale_dev,
                 TO *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const double sc = scale_dev ? scale * scale_dev[0] : scale;
    out[e] = (TO)(basis_sum<TB>(theta, basis, K, n, e) * sc);
}

// ... for an exact plan (motion_dtype == CMAX_F64): both planes of the scaled flow, as k_patch_to_dense_split writes them
template <typename TB>
__global__ void __launch_bounds__(256)
k_basis_to_dense_split(const double *__restrict__ theta, const TB *__restrict__ basis, int K, int64_t n, double scale, const double *__restrict__ scale_dev,
                       float *__restrict__ hi, float *__restrict__ lo) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const double sc = scale_dev ? scale * scale_dev[0] : scale;
    split_f64(basis_sum<TB>(theta, basis, K, n, e) * sc, hi[e], lo[e]);
}

// Adjoint, g_k = sum_e B_k[e] g[e].  Workgroup c owns the elements [c * kBasisAdjChunk, (c + 1) * kBasisAdjChunk) (clipped to n): it
// reads its share of g ONCE into registers (coalesced: thread t holds the elements t, t + 256, ...) and walks k in tiles of
// kBasisAdjTile -- a thread never holds more than kBasisAdjTile accumulators, whatever K is.  Every sum is fp64 in a fixed order (a
// thread's elements in index order, then block_sum's tree): partial[c][k] is a function of the inputs alone.  No atomics.
template <typename TB, typename TG>
__global__ void __launch_bounds__(256)
k_basis_adj(const TG *__restrict__ g, const TB *__restrict__ basis, int K, int64_t n, double *__restrict__ partial) {
    __shared__ double smem[kBasisAdjTile * (256 / kWave)];
    const int64_t base = (int64_t)blockIdx.x * kBasisAdjChunk + threadIdx.x;
    double gv[kBasisAdjPerThread];
#pragma unroll
    for (int j = 0; j < kBasisAdjPerThread; ++j) {
        const int64_t e = base + (int64_t)j * 256;
        gv[j] = e < n ? (double)g[e] : 0.0;
    }
    for (int k0 = 0; k0 < K; k0 += kBasisAdjTile) {
        double acc[kBasisAdjTile];
#pragma unroll
        for (int t = 0; t < kBasisAdjTile; ++t) {
            acc[t] = 0.0;
            if (k0 + t < K) {  // (block-uniform)
                const TB *__restrict__ b = basis + (int64_t)(k0 + t) * n;
#pragma unroll
                for (int j = 0; j < kBasisAdjPerThread; ++j) {
                    const int64_t e = base + (int64_t)j * 256;
                    if (e < n) acc[t] += (double)b[e] * gv[j];
                }
            }
        }
        block_sum<kBasisAdjTile>(acc, smem);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int t = 0; t < kBasisAdjTile; ++t)
                if (k0 + t < K) partial[(int64_t)blockIdx.x * K + k0 + t] = acc[t];
        }
    }
}

// ... and the fold: out[k] = sum over the chunks, in index order, of partial[c][k].  One workgroup: its 256 threads bring kBasisFoldTile
// chunks at a time into LDS (contiguous, every load of a tile in flight at once -- a thread that walked the chunks alone would pay a memory
// round trip every few of them), then thread k < K adds its column in index order.
constexpr int kBasisFoldTile = 32;
__global__ void __launch_bounds__(256) k_basis_fold(const double *__restrict__ partial, int n_chunks, int K, double *__restrict__ out) {
    __shared__ double s_p[kBasisFoldTile * kBasisMaxK];
    double acc = 0.0;
    for (int c0 = 0; c0 < n_chunks; c0 += kBasisFoldTile) {
        const int rows = n_chunks - c0 < kBasisFoldTile ? n_chunks - c0 : kBasisFoldTile;  // rows * K <= kBasisFoldTile * kBasisMaxK
        for (int i = threadIdx.x; i < rows * K; i += blockDim.x) s_p[i] = partial[(int64_t)c0 * K + i];
        __syncthreads();
        if ((int)threadIdx.x < K)
            for (int c = 0; c < rows; ++c) acc += s_p[c * K + threadIdx.x];
        __syncthreads();
    }
    if ((int)threadIdx.x < K) out[threadIdx.x] = acc;
}

// bmax[k] = max_e |B_k[e]| (one workgroup per k; plan creation: the bound sum_k |v_k| bmax_k >= |B v|_inf scales the tangent of a product)
template <typename TB>
__global__ void __launch_bounds__(256) k_basis_absmax(const TB *__restrict__ basis, int64_t n, double *__restrict__ bmax) {
    __shared__ double s_m[256 / kWave];
    const TB *__restrict__ b = basis + (int64_t)blockIdx.x * n;
    double m = 0.0;
    for (int64_t e = threadIdx.x; e < n; e += blockDim.x) m = fmax(m, fabs((double)b[e]));
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, kWave));
    if ((threadIdx.x & (kWave - 1)) == 0) s_m[threadIdx.x / kWave] = m;
    __syncthreads();
    if (threadIdx.x == 0) bmax[blockIdx.x] = fmax(fmax(s_m[0], s_m[1]), fmax(s_m[2], s_m[3]));
}

static inline int basis_adj_chunks(int64_t n) { return div_up(n, kBasisAdjChunk); }

// launchers (no allocation, no synchronisation: capturable)
template <typename TB, typename TO>
static inline void launch_basis_to_dense(const double *theta, const void *basis, int K, int64_t n, double scale, const double *scale_dev, TO *out, hipStream_t s) {
    hipLaunchKernelGGL((k_basis_to_dense<TB, TO>), dim3(div_up(n, 256)), dim3(256), 0, s, theta, (const TB *)basis, K, n, scale, scale_dev, out);
}
template <typename TB>
static inline void launch_basis_to_dense_split(const double *theta, const void *basis, int K, int64_t n, double scale, const double *scale_dev, float *hi,
                                               float *lo, hipStream_t s) {
    hipLaunchKernelGGL(k_basis_to_dense_split<TB>, dim3(div_up(n, 256)), dim3(256), 0, s, theta, (const TB *)basis, K, n, scale, scale_dev, hi, lo);
}
// partial: basis_adj_chunks(n) * K doubles of scratch
template <typename TB, typename TG>
static inline void launch_basis_adj(const TG *g, const void *basis, int K, int64_t n, double *partial, double *out, hipStream_t s) {
    const int chunks = basis_adj_chunks(n);
    hipLaunchKernelGGL((k_basis_adj<TB, TG>), dim3(chunks), dim3(256), 0, s, g, (const TB *)basis, K, n, partial);
    hipLaunchKernelGGL(k_basis_fold, dim3(1), dim3(256), 0, s, (const double *)partial, chunks, K, out);
}

}  // namespace cmax
