// Motion field over a grid of inverse depth -> dense flow, its tangent, its adjoint and its second-order adjoint:
//   rho = Q s,   U = sum_k a_k A_k,   R = sum_j b_j B_j,   D[c,e] = rho[e] U[c,e] + R[c,e]
// with A [Ka][2][H][W] (the translational field per unit inverse depth), B [Kb][2][H][W] (whatever does not depend on depth: the
// rotational field) and Q the bilinear interpolation of cmax_patch_kernels.h on ONE plane, without the negation the patch map carries.
// The map is a product of two unknowns (a and s): its derivative depends on the point, so besides the adjoint J(x)^T g there is the
// second-order adjoint J(x)^T dg + (dJ[u])^T g that an exact Hessian-vector product needs.  The gauge (a, s) -> (lambda a, s / lambda)
// leaves D unchanged.  Shared by the leaf operators cmax_depth_to_dense* and the depth plan (cmax_depth_plan_create), cmax_solver.hip.
//
// The reference has NO counterpart (its models: 2-DoF translation, per-pixel flow, patch grid); D is warped by its dense-flow rule
// x' = x - dt * D[src] (src/warp.py:263-313) like the flow of every plan.
#pragma once
#include "cmax_basis_kernels.h"
#include "cmax_common.h"
#include "cmax_patch_kernels.h"

namespace cmax {

constexpr int kDepthAdjChunk = CMAX_DEPTH_ADJ_CHUNK;  // consecutive PIXELS one workgroup of k_depth_adj owns
constexpr int kDepthAdjPerThread = kDepthAdjChunk / 256;
constexpr int kDepthAdjTile = 4;  // fields reduced per pass over the workgroup's chunk
static_assert(kDepthAdjChunk % 256 == 0, "a chunk is a whole number of pixels per thread");

struct DepthGeom {
    int ph, pw, pad_h, pad_w, sw_h, sw_w, H, W;
};

// (Q s)(i, j): the four taps of patch_interp<double> on one plane, positive sign
__device__ __forceinline__ double depth_interp(const double *__restrict__ s, const DepthGeom &g, int i, int j) {
    const int gh = g.ph + 2 * g.pad_h, gw = g.pw + 2 * g.pad_w;
    const int h1 = (gh * g.sw_h) / 2 - g.H / 2, w1 = (gw * g.sw_w) / 2 - g.W / 2;
    int r0, r1, c0, c1;
    double lr, lc;
    bilin_tap<double>(i + h1, g.sw_h, gh, r0, r1, lr);
    bilin_tap<double>(j + w1, g.sw_w, gw, c0, c1, lc);
    auto S = [&](int R, int C) { return s[(int64_t)clampi(R - g.pad_h, 0, g.ph - 1) * g.pw + clampi(C - g.pad_w, 0, g.pw - 1)]; };
    return (1.0 - lr) * ((1.0 - lc) * S(r0, c0) + lc * S(r0, c1)) + lr * ((1.0 - lc) * S(r1, c0) + lc * S(r1, c1));
}

// both components of D at pixel e (one thread per pixel: rho is interpolated once); n = 2 H W, the stride between fields
template <typename TB>
__device__ __forceinline__ void depth_flow(const double *__restrict__ a, const double *__restrict__ b, const double *__restrict__ s, const TB *__restrict__ A,
                                           const TB *__restrict__ B, int Ka, int Kb, const DepthGeom &g, int64_t e, double &d0, double &d1) {
    const int64_t hw = (int64_t)g.H * g.W, n = 2 * hw;
    const double rho = depth_interp(s, g, (int)(e / g.W), (int)(e % g.W));
    d0 = rho * basis_sum<TB>(a, A, Ka, n, e) + basis_sum<TB>(b, B, Kb, n, e);
    d1 = rho * basis_sum<TB>(a, A, Ka, n, hw + e) + basis_sum<TB>(b, B, Kb, n, hw + e);
}

// out[c][e] = scale [* *scale_dev] * D[c][e], rounded to TO once (scale / scale_dev as in k_basis_to_dense)
template <typename TB, typename TO>
__global__ void __launch_bounds__(256)
k_depth_to_dense(const double *__restrict__ a, const double *__restrict__ b, const double *__restrict__ s, const TB *__restrict__ A, const TB *__restrict__ B,
                 int Ka, int Kb, DepthGeom g, double scale, const double *__restrict__ scale_dev, TO *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, hw = (int64_t)g.H * g.W;
    if (e >= hw) return;
    const double sc = scale_dev ? scale * scale_dev[0] : scale;
    double d0, d1;
    depth_flow<TB>(a, b, s, A, B, Ka, Kb, g, e, d0, d1);
    out[e] = (TO)(d0 * sc);
    out[hw + e] = (TO)(d1 * sc);
}

// ... for an exact plan (motion_dtype == CMAX_F64): both planes of the scaled flow, as k_basis_to_dense_split writes them
template <typename TB>
__global__ void __launch_bounds__(256)
k_depth_to_dense_split(const double *__restrict__ a, const double *__restrict__ b, const double *__restrict__ s, const TB *__restrict__ A,
                       const TB *__restrict__ B, int Ka, int Kb, DepthGeom g, double scale, const double *__restrict__ scale_dev, float *__restrict__ hi,
                       float *__restrict__ lo) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, hw = (int64_t)g.H * g.W;
    if (e >= hw) return;
    const double sc = scale_dev ? scale * scale_dev[0] : scale;
    double d0, d1;
    depth_flow<TB>(a, b, s, A, B, Ka, Kb, g, e, d0, d1);
    split_f64(d0 * sc, hi[e], lo[e]);
    split_f64(d1 * sc, hi[hw + e], lo[hw + e]);
}

// Tangent along u = (da, db, ds):  dD = (Q ds) U + rho (A da) + B db, times scale
template <typename TB, typename TO>
__global__ void __launch_bounds__(256)
k_depth_to_dense_tan(const double *__restrict__ a, const double *__restrict__ s, const double *__restrict__ da, const double *__restrict__ db,
                     const double *__restrict__ ds, const TB *__restrict__ A, const TB *__restrict__ B, int Ka, int Kb, DepthGeom g, double scale,
                     TO *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, hw = (int64_t)g.H * g.W, n = 2 * hw;
    if (e >= hw) return;
    const int i = (int)(e / g.W), j = (int)(e % g.W);
    const double rho = depth_interp(s, g, i, j), drho = depth_interp(ds, g, i, j);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int64_t ec = c * hw + e;
        const double v = drho * basis_sum<TB>(a, A, Ka, n, ec) + rho * basis_sum<TB>(da, A, Ka, n, ec) + basis_sum<TB>(db, B, Kb, n, ec);
        out[ec] = (TO)(v * scale);
    }
}

// Adjoint (SECOND = false) for a cotangent g [2,H,W]:
//   partial[c][k]      = sum over the chunk of rho A_k . g           (k < Ka)
//   partial[c][Ka + j] = sum over the chunk of B_j . g
//   q[e]               = U[.,e] . g[.,e]                              (k_grid_adj turns the plane into g_s = Q^T q)
// Second-order adjoint (SECOND = true), out = J(x)^T dg + (dJ[u])^T g for u = (da, db, ds):
//   partial[c][k]      = sum of A_k . (rho dg + (Q ds) g),   partial[c][Ka + j] = sum of B_j . dg,   q[e] = U . dg + (A da) . g
// Workgroup c owns the pixels [c * kDepthAdjChunk, (c + 1) * kDepthAdjChunk) (clipped to H W).  It reads g (and dg) ONCE into registers
// (coalesced: thread t holds the pixels t, t + 256, ...), recomputes rho and Q ds from the grid, and walks the Ka + Kb fields in tiles of
// kDepthAdjTile: a thread never holds more than kDepthAdjTile accumulators, whatever Ka + Kb is, and every field is read once.  Every sum
// is fp64 in a fixed order (a thread's pixels in index order, component 0 before 1, then block_sum's tree).  No atomics.
template <typename TB, typename TG, bool SECOND>
__global__ void __launch_bounds__(256)
k_depth_adj(const TG *__restrict__ g, const TG *__restrict__ dg, const double *__restrict__ a, const double *__restrict__ s, const double *__restrict__ da,
            const double *__restrict__ ds, const TB *__restrict__ A, const TB *__restrict__ B, int Ka, int Kb, DepthGeom geo, double *__restrict__ partial,
            double *__restrict__ q) {
    __shared__ double smem[kDepthAdjTile * (256 / kWave)];
    const int64_t hw = (int64_t)geo.H * geo.W, n = 2 * hw;
    const int64_t base = (int64_t)blockIdx.x * kDepthAdjChunk + threadIdx.x;
    const int K = Ka + Kb;
    // wa: what a field of A is summed against, wb: a field of B; gq / hq: what U and (A da) are multiplied by for the plane q
    double wa[kDepthAdjPerThread][2], wb[kDepthAdjPerThread][2], hq[kDepthAdjPerThread][2], qv[kDepthAdjPerThread];
#pragma unroll
    for (int j = 0; j < kDepthAdjPerThread; ++j) {
        const int64_t e = base + (int64_t)j * 256;
        qv[j] = 0.0;
        if (e < hw) {
            const int pi = (int)(e / geo.W), pj = (int)(e % geo.W);
            const double rho = depth_interp(s, geo, pi, pj);
            const double g0 = (double)g[e], g1 = (double)g[hw + e];
            if constexpr (SECOND) {
                const double drho = depth_interp(ds, geo, pi, pj);
                const double h0 = (double)dg[e], h1 = (double)dg[hw + e];
                wa[j][0] = rho * h0 + drho * g0;
                wa[j][1] = rho * h1 + drho * g1;
                wb[j][0] = h0;
                wb[j][1] = h1;
                hq[j][0] = g0;
                hq[j][1] = g1;
            } else {
                wa[j][0] = rho * g0;
                wa[j][1] = rho * g1;
                wb[j][0] = g0;
                wb[j][1] = g1;
                hq[j][0] = hq[j][1] = 0.0;
            }
        } else {
            wa[j][0] = wa[j][1] = wb[j][0] = wb[j][1] = hq[j][0] = hq[j][1] = 0.0;
        }
    }
    for (int k0 = 0; k0 < K; k0 += kDepthAdjTile) {
        double acc[kDepthAdjTile];
#pragma unroll
        for (int t = 0; t < kDepthAdjTile; ++t) {
            acc[t] = 0.0;
            const int k = k0 + t;
            if (k >= K) continue;  // (block-uniform, like the two branches below)
            if (k < Ka) {
                const TB *__restrict__ f = A + (int64_t)k * n;
                const double ak = a[k], dak = SECOND ? da[k] : 0.0;
#pragma unroll
                for (int j = 0; j < kDepthAdjPerThread; ++j) {
                    const int64_t e = base + (int64_t)j * 256;
                    if (e < hw) {
                        const double f0 = (double)f[e], f1 = (double)f[hw + e];
                        acc[t] += f0 * wa[j][0];
                        acc[t] += f1 * wa[j][1];
                        // U . (g or dg) and, second order, (A da) . g
                        qv[j] += ak * (f0 * wb[j][0] + f1 * wb[j][1]);
                        if constexpr (SECOND) qv[j] += dak * (f0 * hq[j][0] + f1 * hq[j][1]);
                    }
                }
            } else {
                const TB *__restrict__ f = B + (int64_t)(k - Ka) * n;
#pragma unroll
                for (int j = 0; j < kDepthAdjPerThread; ++j) {
                    const int64_t e = base + (int64_t)j * 256;
                    if (e < hw) {
                        acc[t] += (double)f[e] * wb[j][0];
                        acc[t] += (double)f[hw + e] * wb[j][1];
                    }
                }
            }
        }
        block_sum<kDepthAdjTile>(acc, smem);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int t = 0; t < kDepthAdjTile; ++t)
                if (k0 + t < K) partial[(int64_t)blockIdx.x * K + k0 + t] = acc[t];
        }
    }
#pragma unroll
    for (int j = 0; j < kDepthAdjPerThread; ++j) {
        const int64_t e = base + (int64_t)j * 256;
        if (e < hw) q[e] = qv[j];
    }
}

// g_s = Q^T q: one workgroup per cell of the grid over its clipped band of pixels -- the band arithmetic of k_patch_to_dense_adj for one
// plane, with positive sign.  A cell with no pixel on one axis or on both has an empty band (never a negative extent) and receives 0.
__global__ void __launch_bounds__(256) k_grid_adj(const double *__restrict__ q, DepthGeom g, double *__restrict__ gs) {
    __shared__ double smem[4];
    const int cell = blockIdx.x, pr = cell / g.pw, pc = cell % g.pw;
    const int ph = g.ph, pw = g.pw, pad_h = g.pad_h, pad_w = g.pad_w, sw_h = g.sw_h, sw_w = g.sw_w, H = g.H, W = g.W;
    const int gh = ph + 2 * pad_h, gw = pw + 2 * pad_w;
    const int h1 = (gh * sw_h) / 2 - H / 2, w1 = (gw * sw_w) / 2 - W / 2;
    const int Rlo = pr == 0 ? 0 : pr + pad_h, Rhi = pr == ph - 1 ? gh - 1 : pr + pad_h;
    const int Clo = pc == 0 ? 0 : pc + pad_w, Chi = pc == pw - 1 ? gw - 1 : pc + pad_w;
    const int i_lo = max((Rlo - 1) * sw_h - h1 - 1, 0), i_hi = min((Rhi + 2) * sw_h - h1 + 1, H);
    const int j_lo = max((Clo - 1) * sw_w - w1 - 1, 0), j_hi = min((Chi + 2) * sw_w - w1 + 1, W);
    const int bw = max(j_hi - j_lo, 0), bh = max(i_hi - i_lo, 0);
    double acc[1] = {0.0};
    for (int t = threadIdx.x; t < bw * bh; t += blockDim.x) {
        const int i = i_lo + t / bw, j = j_lo + t % bw;
        int r0, r1, c0, c1;
        double lr, lc;
        bilin_tap<double>(i + h1, sw_h, gh, r0, r1, lr);
        bilin_tap<double>(j + w1, sw_w, gw, c0, c1, lc);
        const double wr = (clampi(r0 - pad_h, 0, ph - 1) == pr ? 1.0 - lr : 0.0) + (clampi(r1 - pad_h, 0, ph - 1) == pr ? lr : 0.0);
        const double wc = (clampi(c0 - pad_w, 0, pw - 1) == pc ? 1.0 - lc : 0.0) + (clampi(c1 - pad_w, 0, pw - 1) == pc ? lc : 0.0);
        acc[0] += q[(int64_t)i * W + j] * wr * wc;
    }
    block_sum<1>(acc, smem);
    if (threadIdx.x == 0) gs[cell] = acc[0];
}

static inline int depth_adj_chunks(int64_t hw) { return div_up(hw, kDepthAdjChunk); }

// launchers (no allocation, no synchronisation: capturable)
template <typename TB, typename TO>
static inline void launch_depth_to_dense(const double *a, const double *b, const double *s_, const void *A, const void *B, int Ka, int Kb, const DepthGeom &g,
                                         double scale, const double *scale_dev, TO *out, hipStream_t s) {
    hipLaunchKernelGGL((k_depth_to_dense<TB, TO>), dim3(div_up((int64_t)g.H * g.W, 256)), dim3(256), 0, s, a, b, s_, (const TB *)A, (const TB *)B, Ka, Kb, g,
                       scale, scale_dev, out);
}
template <typename TB>
static inline void launch_depth_to_dense_split(const double *a, const double *b, const double *s_, const void *A, const void *B, int Ka, int Kb,
                                               const DepthGeom &g, double scale, const double *scale_dev, float *hi, float *lo, hipStream_t s) {
    hipLaunchKernelGGL(k_depth_to_dense_split<TB>, dim3(div_up((int64_t)g.H * g.W, 256)), dim3(256), 0, s, a, b, s_, (const TB *)A, (const TB *)B, Ka, Kb, g,
                       scale, scale_dev, hi, lo);
}
template <typename TB, typename TO>
static inline void launch_depth_to_dense_tan(const double *a, const double *s_, const double *da, const double *db, const double *ds, const void *A,
                                             const void *B, int Ka, int Kb, const DepthGeom &g, double scale, TO *out, hipStream_t s) {
    hipLaunchKernelGGL((k_depth_to_dense_tan<TB, TO>), dim3(div_up((int64_t)g.H * g.W, 256)), dim3(256), 0, s, a, s_, da, db, ds, (const TB *)A,
                       (const TB *)B, Ka, Kb, g, scale, out);
}
// partial: depth_adj_chunks(H W) * (Ka + Kb) doubles, q: H W doubles of scratch; out_ab [Ka + Kb] (a then b), out_s [ph pw].
// dg / da / ds: the second-order adjoint's (SECOND), else unused.
template <typename TB, typename TG, bool SECOND>
static inline void launch_depth_adj(const TG *g, const TG *dg, const double *a, const double *s_, const double *da, const double *ds, const void *A,
                                    const void *B, int Ka, int Kb, const DepthGeom &geo, double *partial, double *q, double *out_ab, double *out_s,
                                    hipStream_t s) {
    const int chunks = depth_adj_chunks((int64_t)geo.H * geo.W);
    hipLaunchKernelGGL((k_depth_adj<TB, TG, SECOND>), dim3(chunks), dim3(256), 0, s, g, dg, a, s_, da, ds, (const TB *)A, (const TB *)B, Ka, Kb, geo, partial,
                       q);
    hipLaunchKernelGGL(k_basis_fold, dim3(1), dim3(256), 0, s, (const double *)partial, chunks, Ka + Kb, out_ab);
    hipLaunchKernelGGL(k_grid_adj, dim3(geo.ph * geo.pw), dim3(256), 0, s, (const double *)q, geo, out_s);
}

}  // namespace cmax
