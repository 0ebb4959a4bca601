// Event-collapse regularisers on a dense displacement field F [2,H,W] (F[0] along rows, F[1] along columns): the divergence of the
// flow and the change of area under the warp x' = x - s F (Shiba, Aoki, Gallego, "Event Collapse in Contrast Maximization
// Frameworks", Sensors 2022, on the flow field instead of per event).  Compiled in cmax_solver.hip only: the leaf operators
// cmax_flow_regularizer[_tan] and the plan's extra term (cmax_patch_plan_set_flow_regularizer).
//
// The reference has NO counterpart; include/cmax_hip.h states the formulas.  With Omega the interior 1 <= r <= H-2, 1 <= c <= W-2,
// n = (H-2)(W-2), central differences a = dF0/dr, b = dF0/dc, c = dF1/dr, d = dF1/dc on Omega and psi(u) = sqrt(u^2 + eps^2) - eps:
//   divergence  R = (1/n)  sum_Omega psi(a + d)
//   area        R = (1/2n) sum_Omega [psi(A(+s) - 1) + psi(A(-s) - 1)],  A(sigma) = 1 - sigma (a + d) + sigma^2 (a d - b c)
// Gradient: the transposed central difference of p = dR/d(a,b,c,d) (zero outside Omega).  Product: the same transpose of the
// directional derivative of p along dF.  All arithmetic is fp64 whatever the field's dtype is.
#pragma once
#include "cmax_common.h"

namespace cmax {

constexpr int kFrTileH = 8, kFrTileW = 32;  // one pixel per thread of a 256-thread workgroup
constexpr int kFrFH = kFrTileH + 4, kFrFW = kFrTileW + 4;  // field tile: halo of 2
constexpr int kFrPH = kFrTileH + 2, kFrPW = kFrTileW + 2;  // p = dR/d(a,b,c,d): the tile and a ring of one

struct FlowRegArgs {
    int H, W;
    double eps, s;
    double inv_n;  // 1 / n (divergence), 1 / 2n (area)
};

static inline int flowreg_tiles(int H, int W) { return div_up(H, kFrTileH) * div_up(W, kFrTileW); }

// psi and psi' / psi' and psi''.  eps = 0: |u|, sign(u) with psi'(0) = 0, psi'' = 0.  (sqrt(u^2 + eps^2) - eps is taken as
// u^2 / (sqrt(u^2 + eps^2) + eps): no cancellation where |u| << eps)
__device__ __forceinline__ void flowreg_psi(double u, double eps, double &v, double &d1) {
    const double den = sqrt(u * u + eps * eps);
    v = den > 0.0 ? u * u / (den + eps) : 0.0;
    d1 = den > 0.0 ? u / den : 0.0;
}
__device__ __forceinline__ void flowreg_dpsi(double u, double eps, double &d1, double &d2) {
    const double den = sqrt(u * u + eps * eps);
    d1 = den > 0.0 ? u / den : 0.0;
    d2 = den > 0.0 ? eps * eps / (den * den * den) : 0.0;
}

// What a kind contributes at one pixel of Omega from the derivatives q = (a, b, c, d): kPlanes planes of p are kept in LDS (the
// divergence has p_a = p_d and p_b = p_c = 0: one plane).
template <int KIND>
struct FlowRegTerm;

template <>
struct FlowRegTerm<CMAX_FLOWREG_DIVERGENCE> {
    static constexpr int kPlanes = 1;
    static __device__ __forceinline__ double grad(const double (&q)[4], const FlowRegArgs &ra, double (&p)[1]) {
        double v;
        flowreg_psi(q[0] + q[3], ra.eps, v, p[0]);
        return v;
    }
    static __device__ __forceinline__ void tan(const double (&q)[4], const double (&dq)[4], const FlowRegArgs &ra, double (&dp)[1]) {
        double d1, d2;
        flowreg_dpsi(q[0] + q[3], ra.eps, d1, d2);
        dp[0] = d2 * (dq[0] + dq[3]);
    }
    // planes of p that the transposed differences read: rows (d/dr) and columns (d/dc) of each component
    static __device__ __forceinline__ int row_plane(int comp) { return comp == 0 ? 0 : -1; }
    static __device__ __forceinline__ int col_plane(int comp) { return comp == 0 ? -1 : 0; }
};

template <>
struct FlowRegTerm<CMAX_FLOWREG_AREA> {
    static constexpr int kPlanes = 4;
    static __device__ __forceinline__ double grad(const double (&q)[4], const FlowRegArgs &ra, double (&p)[4]) {
        const double tr = q[0] + q[3], det = q[0] * q[3] - q[1] * q[2];
        double e = 0.0;
        p[0] = p[1] = p[2] = p[3] = 0.0;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const double sg = k == 0 ? ra.s : -ra.s, s2 = sg * sg;
            double v, d1;
            flowreg_psi(-sg * tr + s2 * det, ra.eps, v, d1);  // A(sigma) - 1
            e += v;
            p[0] += d1 * (-sg + s2 * q[3]);
            p[1] += d1 * (-s2 * q[2]);
            p[2] += d1 * (-s2 * q[1]);
            p[3] += d1 * (-sg + s2 * q[0]);
        }
        return e;
    }
    // psi'' acts on the directional derivative of u, psi' on the constant Hessian of A (d2A/da dd = sigma^2, d2A/db dc = -sigma^2)
    static __device__ __forceinline__ void tan(const double (&q)[4], const double (&dq)[4], const FlowRegArgs &ra, double (&dp)[4]) {
        const double tr = q[0] + q[3], det = q[0] * q[3] - q[1] * q[2];
        dp[0] = dp[1] = dp[2] = dp[3] = 0.0;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const double sg = k == 0 ? ra.s : -ra.s, s2 = sg * sg;
            double d1, d2;
            flowreg_dpsi(-sg * tr + s2 * det, ra.eps, d1, d2);
            const double ua = -sg + s2 * q[3], ub = -s2 * q[2], uc = -s2 * q[1], ud = -sg + s2 * q[0];
            const double du = d2 * (ua * dq[0] + ub * dq[1] + uc * dq[2] + ud * dq[3]);
            dp[0] += du * ua + d1 * s2 * dq[3];
            dp[1] += du * ub - d1 * s2 * dq[2];
            dp[2] += du * uc - d1 * s2 * dq[1];
            dp[3] += du * ud + d1 * s2 * dq[0];
        }
    }
    static __device__ __forceinline__ int row_plane(int comp) { return comp == 0 ? 0 : 2; }
    static __device__ __forceinline__ int col_plane(int comp) { return comp == 0 ? 1 : 3; }
};

// Both components of `scale * F` with a halo of 2 around the workgroup's tile, zero outside the image (a pixel of Omega never reads
// those), as fp64 whatever T is
template <typename T>
__device__ __forceinline__ void flowreg_stage(double (&t)[2][kFrFH][kFrFW], const T *__restrict__ F, double scale, int r0, int c0, int H, int W) {
    for (int q = threadIdx.x; q < 2 * kFrFH * kFrFW; q += 256) {
        const int comp = q / (kFrFH * kFrFW), rem = q - comp * (kFrFH * kFrFW), y = rem / kFrFW, x = rem - y * kFrFW;
        const int r = r0 - 2 + y, c = c0 - 2 + x;
        t[comp][y][x] = (unsigned)r < (unsigned)H && (unsigned)c < (unsigned)W ? scale * (double)F[((int64_t)comp * H + r) * W + c] : 0.0;
    }
}

// central differences (a, b, c, d) at the pixel whose field-tile coordinates are (y, x)
__device__ __forceinline__ void flowreg_diff(const double (&t)[2][kFrFH][kFrFW], int y, int x, double (&q)[4]) {
    q[0] = 0.5 * (t[0][y + 1][x] - t[0][y - 1][x]);
    q[1] = 0.5 * (t[0][y][x + 1] - t[0][y][x - 1]);
    q[2] = 0.5 * (t[1][y + 1][x] - t[1][y - 1][x]);
    q[3] = 0.5 * (t[1][y][x + 1] - t[1][y][x - 1]);
}

// Transposed central differences of the planes of p at the thread's pixel (la, lb) of the tile, then "store" (out is T [2,H,W]) or
// "add w * g" (out is an fp64 [2,H,W] accumulator)
template <int KIND, typename T, int NP>
__device__ __forceinline__ void flowreg_transpose_out(const double (&p)[NP][kFrPH][kFrPW], double inv_n, int r0, int c0, int H, int W, void *__restrict__ out,
                                                      int add, double w) {
    using K = FlowRegTerm<KIND>;
    const int la = threadIdx.x / kFrTileW, lb = threadIdx.x - la * kFrTileW;
    const int i = r0 + la, j = c0 + lb;
    if (i >= H || j >= W) return;
#pragma unroll
    for (int comp = 0; comp < 2; ++comp) {
        const int pr = K::row_plane(comp), pc = K::col_plane(comp);
        double g = 0.0;
        if (pr >= 0) g += p[pr][la][lb + 1] - p[pr][la + 2][lb + 1];  // pixel (i - 1, j) reads F(i, j) with +1/2, pixel (i + 1, j) with -1/2
        if (pc >= 0) g += p[pc][la + 1][lb] - p[pc][la + 1][lb + 2];
        g *= 0.5 * inv_n;
        const int64_t o = ((int64_t)comp * H + i) * W + j;
        if (add) reinterpret_cast<double *>(out)[o] += w * g;
        else reinterpret_cast<T *>(out)[o] = (T)g;
    }
}

// Value and gradient of R(scale * F) in one launch, after the shape of k_stats_gimage_st: one 8 x 32 tile per workgroup; the field with a
// halo of 2 in LDS; p for the tile and a ring of one, ZERO outside Omega, once per pixel; the transpose as plain differences on those;
// the energy of the tile's own pixels in fp64 through block_sum's fixed tree into partial[workgroup] (plain store: k_flowreg_fold adds
// them in index order, no atomics -- the same field gives the same bits).  out == nullptr: value only.
// LDS: every access is a ds_read_b64 / ds_write_b64 (bank = dword address mod 64, conflicts within a 32-lane half only).  A half-wave
// reads 32 consecutive doubles of one row, conflict-free at any pitch, and the staging loops write consecutive q, conflict-free when a
// row's pitch equals its width: no padding.  The loop over p reads the field tile at the pitch of a wider row, so a half-wave that
// straddles a row end pays one 2-way conflict.
template <int KIND, typename T>
__global__ void __launch_bounds__(256)
k_flowreg(const T *__restrict__ F, double scale, FlowRegArgs ra, double *__restrict__ partial, void *__restrict__ out, int add, double w) {
    using K = FlowRegTerm<KIND>;
    constexpr int NP = K::kPlanes;
    __shared__ double smem[256 / kWave];
    __shared__ double t_f[2][kFrFH][kFrFW];
    __shared__ double t_p[NP][kFrPH][kFrPW];
    const int H = ra.H, W = ra.W;
    const int tiles_w = (W + kFrTileW - 1) / kFrTileW;
    const int tr = blockIdx.x / tiles_w, tc = blockIdx.x - tr * tiles_w;
    const int r0 = tr * kFrTileH, c0 = tc * kFrTileW;  // top-left pixel of the tile
    flowreg_stage<T>(t_f, F, scale, r0, c0, H, W);
    __syncthreads();
    double v[1] = {0.0};
    for (int q = threadIdx.x; q < kFrPH * kFrPW; q += 256) {
        const int y = q / kFrPW, x = q - y * kFrPW;  // pixel (r0 - 1 + y, c0 - 1 + x)
        const int qi = r0 - 1 + y, qj = c0 - 1 + x;
        const bool in_om = qi >= 1 && qi < H - 1 && qj >= 1 && qj < W - 1;
        double d[4], p[NP];
        flowreg_diff(t_f, y + 1, x + 1, d);
        const double e = K::grad(d, ra, p);
#pragma unroll
        for (int k = 0; k < NP; ++k) t_p[k][y][x] = in_om ? p[k] : 0.0;
        if (in_om && y >= 1 && y <= kFrTileH && x >= 1 && x <= kFrTileW) v[0] += e;  // (a pixel of the ring belongs to a neighbour's sum)
    }
    block_sum<1>(v, smem);  // (its barriers also publish t_p)
    if (threadIdx.x == 0) partial[blockIdx.x] = v[0];
    if (out) flowreg_transpose_out<KIND, T, NP>(t_p, ra.inv_n, r0, c0, H, W, out, add, w);
}

// value[0] = inv_n * sum of the tiles' energies, in index order per thread and block_sum's tree across them: a function of the
// partials alone.  One workgroup.
__global__ void __launch_bounds__(256) k_flowreg_fold(const double *__restrict__ partial, int n_tiles, double inv_n, double *__restrict__ value) {
    __shared__ double smem[256 / kWave];
    double v[1] = {0.0};
    for (int i = threadIdx.x; i < n_tiles; i += 256) v[0] += partial[i];
    block_sum<1>(v, smem);
    if (threadIdx.x == 0) value[0] = inv_n * v[0];
}

// (grad^2 R)[dF] at scale * F along dscale [* *dscale_dev] * dF: the same structure, p exchanged for its directional derivative
template <int KIND, typename T>
__global__ void __launch_bounds__(256)
k_flowreg_tan(const T *__restrict__ F, const T *__restrict__ dF, double scale, double dscale, const double *__restrict__ dscale_dev, FlowRegArgs ra,
              void *__restrict__ out, int add, double w) {
    using K = FlowRegTerm<KIND>;
    constexpr int NP = K::kPlanes;
    __shared__ double t_f[2][kFrFH][kFrFW], t_df[2][kFrFH][kFrFW];
    __shared__ double t_p[NP][kFrPH][kFrPW];
    const int H = ra.H, W = ra.W;
    const int tiles_w = (W + kFrTileW - 1) / kFrTileW;
    const int tr = blockIdx.x / tiles_w, tc = blockIdx.x - tr * tiles_w;
    const int r0 = tr * kFrTileH, c0 = tc * kFrTileW;
    if (dscale_dev) dscale *= dscale_dev[0];
    flowreg_stage<T>(t_f, F, scale, r0, c0, H, W);
    flowreg_stage<T>(t_df, dF, dscale, r0, c0, H, W);
    __syncthreads();
    for (int q = threadIdx.x; q < kFrPH * kFrPW; q += 256) {
        const int y = q / kFrPW, x = q - y * kFrPW;
        const int qi = r0 - 1 + y, qj = c0 - 1 + x;
        const bool in_om = qi >= 1 && qi < H - 1 && qj >= 1 && qj < W - 1;
        double d[4], dd[4], dp[NP];
        flowreg_diff(t_f, y + 1, x + 1, d);
        flowreg_diff(t_df, y + 1, x + 1, dd);
        K::tan(d, dd, ra, dp);
#pragma unroll
        for (int k = 0; k < NP; ++k) t_p[k][y][x] = in_om ? dp[k] : 0.0;
    }
    __syncthreads();
    flowreg_transpose_out<KIND, T, NP>(t_p, ra.inv_n, r0, c0, H, W, out, add, w);
}

// launchers (no allocation, no synchronisation: capturable).  partial: flowreg_tiles(H, W) doubles of scratch.
static inline FlowRegArgs flowreg_args(const cmax_flow_regularizer_t &r, int H, int W) {
    const double n = (double)(H - 2) * (double)(W - 2);
    return FlowRegArgs{H, W, r.eps, r.s, r.kind == CMAX_FLOWREG_AREA ? 0.5 / n : 1.0 / n};
}
template <typename T>
static inline void launch_flowreg(const cmax_flow_regularizer_t &r, const T *F, double scale, int H, int W, double *partial, double *value, void *out,
                                  int add, double w, hipStream_t s) {
    const FlowRegArgs ra = flowreg_args(r, H, W);
    const int tiles = flowreg_tiles(H, W);
    if (r.kind == CMAX_FLOWREG_AREA) hipLaunchKernelGGL((k_flowreg<CMAX_FLOWREG_AREA, T>), dim3(tiles), dim3(256), 0, s, F, scale, ra, partial, out, add, w);
    else hipLaunchKernelGGL((k_flowreg<CMAX_FLOWREG_DIVERGENCE, T>), dim3(tiles), dim3(256), 0, s, F, scale, ra, partial, out, add, w);
    hipLaunchKernelGGL(k_flowreg_fold, dim3(1), dim3(256), 0, s, (const double *)partial, tiles, ra.inv_n, value);
}
template <typename T>
static inline void launch_flowreg_tan(const cmax_flow_regularizer_t &r, const T *F, const T *dF, double scale, double dscale, const double *dscale_dev, int H,
                                      int W, void *out, int add, double w, hipStream_t s) {
    const FlowRegArgs ra = flowreg_args(r, H, W);
    const int tiles = flowreg_tiles(H, W);
    if (r.kind == CMAX_FLOWREG_AREA)
        hipLaunchKernelGGL((k_flowreg_tan<CMAX_FLOWREG_AREA, T>), dim3(tiles), dim3(256), 0, s, F, dF, scale, dscale, dscale_dev, ra, out, add, w);
    else hipLaunchKernelGGL((k_flowreg_tan<CMAX_FLOWREG_DIVERGENCE, T>), dim3(tiles), dim3(256), 0, s, F, dF, scale, dscale, dscale_dev, ra, out, add, w);
}

// the descriptor's parameters (weight aside): kind 1 / 2, eps >= 0, s > 0, all finite
static inline bool flowreg_desc_ok(const cmax_flow_regularizer_t &r) {
    return (r.kind == CMAX_FLOWREG_DIVERGENCE || r.kind == CMAX_FLOWREG_AREA) && r.eps >= 0.0 && r.eps <= 1.7e308 && r.s > 0.0 && r.s <= 1.7e308;
}

}  // namespace cmax
