// Fused contrast-maximization objective for MI355X (gfx950).
//
// One evaluation = what PatchContrastMaximization.get_arg_for_cost + cost.calculate +
// torch.autograd.grad compute in the reference (src/solver/patch_contrast_base.py:273-352,
// src/solver/scipy_autograd/torch_wrapper.py:30-49), without ever materialising warped events:
//
//   set_events (once per batch)  pack to 8 B/event (12-bit row | 12-bit col | 8-bit time bin, fp32
//                                normalised time) and counting-sort by source-pixel tile (binned handles:
//                                by (tile, time bin)); the host cuts the sorted stream into segments
//   K1  k_vote      one workgroup per SEGMENT (<= 2040 consecutive sorted events = a few neighbouring
//                   source tiles): warp, bounding box of the targets, votes accumulated in an LDS
//                   window as 12.20 fixed point with ds_add_u32 (fp32 LDS atomics run at 1/12 of the
//                   integer rate on gfx950, profiles/r01_microbench.txt), one coalesced global
//                   atomicAdd per touched window pixel; publishes its windows for K3
//   K2  image kernels: k_stats (fp64 sums of the contrast function into `nsub` sub-accumulators per
//                   image: same-address fp64 atomics serialise at ~12 ns), or fused with what follows --
//                   k_blur_stats_adj_var (variance with blur and a gradient: ONE kernel, the mean comes from K1's vote sums;
//                   value-only / multi-GPU: k_blur_stats_var + k_gimage_blur_adj_var),
//                   k_stats_gimage_gm / k_blur_stats_gimage_gm (gradient magnitude: statistics + the
//                   G = dL/dIWE, blurs included), k_stats_gimage_st<COST> (the focus losses: statistics + G over
//                   FocusStencil, between k_blur3 and k_blur3_adj when the cost blurs).  They also clear the OTHER vote buffer for
//                   the next evaluation (double buffering: no memset in the steady state) and the
//                   flow-gradient buffer, with write-through stores.  Plain variance needs no G image:
//                   K3 gathers the raw image (the mean cancels in the gather's differences except at the
//                   edge of the region); on owned groups its K2 even runs INSIDE the K3 launch (kFoldStatsInside)
//   K3  k_grad      per event: re-warp, gather G at the 4 corners -> dL/d(x',y') -> motion gradient
//                   (2-DoF: per-segment partials, for the plain variance together with the image
//                   statistics so that K2 is not launched at all; dense: runs of equal source pixel
//                   reduced in registers + one segmented scan, one atomic per run; voxel: LDS
//                   accumulators in block-scaled fixed point)
//   k_finish / k_finish_deferred   sum the per-segment partials (2-DoF), write loss + gradient
// Every launch covers all reference times of the objective (blockIdx.y).  The event kernels (K1, K3, the tangent and per-event
// gathers: cmax_event_kernels.inc) and their launch layer are a translation unit of their own, cmax_event_launch.hip; so are the
// handle's lifetime and everything done once per batch (set_events above), cmax_batch.hip.  This unit holds what is done PER
// EVALUATION -- the image-side kernels and the orchestration -- and reaches the event kernels through the launchers declared in
// cmax_fused_internal.h (launch_vote, launch_grad, ...) alone.
//
// fp32 per event with the integer source pixel split from the fp32 displacement (keeps the
// bilinear fractions accurate to ulp(displacement) instead of ulp(coordinate)); fp64 reductions.
#include <algorithm>
#include <atomic>

#include "cmax_descent.h"
#include "cmax_lbfgs.h"
#include "cmax_fused_device.h"
#include "cmax_image_kernels.h"
#include "cmax_search_kernels.h"

// Environment knobs this unit reads (tuning experiments and A/B tests only; none changes results beyond rounding; the per-batch ones
// are listed in cmax_batch.hip):
//   CMAX_NO_STATS_INSIDE=1   plain variance on owned groups: k_stats as a launch of its own instead of inside K3's
//   CMAX_STAT_SWEEPS=n       statistics inside K3's launch: 4-pixel sweeps per statistics workgroup (fewer, longer workgroups)
//   CMAX_NO_FUSED_BLURVAR=1  blurred variance: k_blur_stats_var + k_gimage_blur_adj_var instead of k_blur_stats_adj_var
//   CMAX_NO_FUSED_FOCUS=1    focus losses: k_stats + k_gimage as launches of their own instead of k_stats_gimage_st
//   CMAX_NSUB=n          statistics sub-accumulators (cache lines) per image
//   CMAX_TAN2=0 | 1      2-DoF tangent-image path: never / also without a communicator
//   CMAX_PLAN_GRAPHS=1   replay the patch plan from captured hipGraphs (cmax_solver.hip)
namespace cmax {

// An fp64 flow / voxel at the boundary: out[i] = hi = (float)v[i] -- the value an fp32 caller passes, read by every kernel -- and
// out[count + i] = lo = (float)(v[i] - hi), read only where K1 decides a cell in fp64 (hi + lo = v to 2^-48 relative, what the source
// residual rx + rxl has); lo = 0 where hi is not finite (split_f64, cmax_common.h).  Streaming: 2 x 16-byte loads, 2 x 16-byte stores per thread and step
// (`vec`: count is a multiple of 4 and v is 16-byte aligned), one value per thread otherwise.
__global__ void __launch_bounds__(256) k_split_motion(const double *__restrict__ v, int64_t count, int vec, float *__restrict__ out) {
    const int64_t step = (int64_t)gridDim.x * blockDim.x, t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (vec) {
        const double2 *v2 = reinterpret_cast<const double2 *>(v);
        float4 *hi4 = reinterpret_cast<float4 *>(out), *lo4 = reinterpret_cast<float4 *>(out + count);
        for (int64_t i = t; i < count / 4; i += step) {
            const double2 a = v2[2 * i], b = v2[2 * i + 1];
            float4 hi, lo;
            split_f64(a.x, hi.x, lo.x);
            split_f64(a.y, hi.y, lo.y);
            split_f64(b.x, hi.z, lo.z);
            split_f64(b.y, hi.w, lo.w);
            hi4[i] = hi;
            lo4[i] = lo;
        }
    } else {
        for (int64_t i = t; i < count; i += step) split_f64(v[i], out[i], out[count + i]);
    }
}

// Stage the ROWS x COLS window of `img` whose top-left pixel is (r0, c0) into an LDS tile of row pitch LD floats, zero outside
// the image.  All of a thread's loads are issued before its first LDS store (see pin(): `in ? img[..] : 0` per iteration is one
// memory round trip per iteration).  256 threads.
template <int ROWS, int COLS, int LD>
__device__ __forceinline__ void stage_tile(float (*tile)[LD], const float *__restrict__ img, int r0, int c0, int H, int W) {
    constexpr int kN = ROWS * COLS, kIt = (kN + 255) / 256;
    float x[kIt];
#pragma unroll
    for (int u = 0; u < kIt; ++u) {
        const int q = threadIdx.x + 256 * u, a = q / COLS, b = q - a * COLS;
        const int r = min(max(r0 + a, 0), H - 1), c = min(max(c0 + b, 0), W - 1);
        x[u] = img[(int64_t)r * W + c];
    }
#pragma unroll
    for (int u = 0; u < kIt; ++u) pin(x[u]);
#pragma unroll
    for (int u = 0; u < kIt; ++u) {
        const int q = threadIdx.x + 256 * u, a = q / COLS, b = q - a * COLS;
        const int r = r0 + a, c = c0 + b;
        if (q < kN) tile[a][b] = ((unsigned)r < (unsigned)H && (unsigned)c < (unsigned)W) ? x[u] : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------
// K2: contrast statistics of one image (+ zeroing of the NEXT evaluation's vote image).
//     Workgroup b adds its fp64 partials to sub-accumulator b % 32 of its slot:
//     stat[slot][sub][0] = sum x (variance) or sum gx^2+gy^2 (grad-mag), [1] = sum x^2.
//     Same-address fp64 atomics serialise at ~12 ns each (they cost 47 us in the first version), so
//     they are spread over 32 addresses and consumers add the 32 values.  The accumulators are zeroed
//     by workgroup 0 of the K1 launch that fills the image (stream order), so no memset node exists.
// ---------------------------------------------------------------------------------------------

// THR: 256, or 1024 in deterministic mode (kStatSub workgroups, one per accumulator: they have to be large)
template <int COST, int THR = 256>
__global__ void __launch_bounds__(THR)
k_stats(const float *__restrict__ img, int H, int W, int omit, int nsub, double *__restrict__ stat_slot, float *__restrict__ zero_img,
        float4 *__restrict__ zero_extra, int64_t n_extra4, int64_t bs = 0) {
    __shared__ double smem[2 * (THR / 64)];
    img += blockIdx.y * bs;  // blockIdx.y: image of a batch (element stride bs)
    stat_slot += blockIdx.y * kStatStride;
    if (zero_img) zero_img += blockIdx.y * bs;
    // the flow-gradient buffer K3 accumulates into is cleared here (a hipMemsetAsync node costs 4-5 us)
    const int64_t gtid = (int64_t)blockIdx.x * THR + threadIdx.x, gthreads = (int64_t)gridDim.x * THR;
    const unsigned npix = (unsigned)H * (unsigned)W;
    const int i0 = omit ? 1 : 0;
    const unsigned stride = gridDim.x * (unsigned)THR;
    double v[2] = {0.0, 0.0};
    for (unsigned base = blockIdx.x * (unsigned)THR + threadIdx.x; base < npix; base += 4u * stride) {
        float x[4];
        bool in[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {  // 4 independent loads in flight per thread
            const unsigned p = base + (unsigned)u * stride;
            const unsigned r = p / (unsigned)W, c = p - r * (unsigned)W;
            in[u] = p < npix && (int)r >= i0 && (int)r < H - i0 && (int)c >= i0 && (int)c < W - i0;
            x[u] = 0.f;
            if (COST == CMAX_COST_VARIANCE) x[u] = img[p < npix ? p : npix - 1u];  // unconditional: see pin()
        }
        if (COST == CMAX_COST_VARIANCE) {
#pragma unroll
            for (int u = 0; u < 4; ++u) pin(x[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u) x[u] = in[u] ? x[u] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (COST == CMAX_COST_VARIANCE) {
                const double xd = (double)x[u];
                v[0] += xd;
                v[1] += xd * xd;
            } else if (in[u]) {
                const unsigned p = base + (unsigned)u * stride;
                const int r = (int)(p / (unsigned)W), c = (int)(p - (unsigned)r * (unsigned)W);
                if constexpr (COST == CMAX_COST_GRADMAG) {
                    float gx, gy;
                    sobel8_f32(img, H, W, r, c, gx, gy);
                    v[0] += (double)(gx * gx + gy * gy);
                } else if constexpr (COST != CMAX_COST_VARIANCE) {  // a focus loss: the energy of its responses (FocusStencil, cmax_image_kernels.h)
                    float n[3][3];
                    focus_load<1, float>(img, H, W, r, c, n);
                    v[0] += (double)focus_energy<COST, float>(n);
                }
            }
        }
    }
    // The clearing stores go out AFTER the image loads have been consumed: vmcnt retires in issue order, so a
    // write-through store issued first sits on the critical path of every load behind it (k_stats 6.2 -> see profiles)
    if (blockIdx.y == 0) zero_fill_sc1((float *)zero_extra, 4 * n_extra4, gtid, gthreads);
    zero_fill_sc1(zero_img, (int64_t)H * W, gtid, gthreads);
    block_sum<2>(v, smem);
    if (threadIdx.x == 0) {
        double *a = stat_slot + kSubStride * (blockIdx.x % nsub);
        atomic_add(&a[0], v[0]);
        if (COST == CMAX_COST_VARIANCE) atomic_add(&a[1], v[1]);
    }
}

// K2 + K2b in one pass for the gradient-magnitude cost: statistics as k_stats<GRADMAG>, and the UNSCALED
// G' = (2 / n) / 8 * Sobel^T (gx, gy) 1_Omega  -- the chain factor of the objective (which needs the statistics of
// every image) is applied by K3 when it loads its window (kFoldScale), and commutes with the blur transpose.
// Blurred variance cost in two image kernels instead of four (every dependent launch costs ~4.5 us):
//   k_blur_stats_var      Ib = blur3(I) (written: K3 / cmax_copy_iwe read it), sum Ib, sum Ib^2 over Omega, zeroing
//   k_gimage_blur_adj_var G = blur3^T [ c (Ib - mu) 1_Omega ]  with c, mu from the finished statistics
__global__ void __launch_bounds__(256)
k_blur_stats_var(const float *__restrict__ in0, int64_t in_stride, int H, int W, ImgArgs ia, float k0, float k1, int omit, int nsub, double *__restrict__ stat_base,
                 float4 *__restrict__ zero_extra, int64_t n_extra4) {
    __shared__ double smem[2 * 4];
    const float *__restrict__ img = in0 + blockIdx.y * in_stride;  // (leading, preloaded arguments: the tile loads leave without waiting for the argument block)
    float *__restrict__ blurred = ia.blurred[blockIdx.y];
    float *__restrict__ zero_img = ia.zero[blockIdx.y];
    double *__restrict__ stat_slot = stat_base + blockIdx.y * kStatStride;
    const int64_t gtid = (int64_t)blockIdx.x * 256 + threadIdx.x, gthreads = (int64_t)gridDim.x * 256;
    const unsigned npix = (unsigned)H * (unsigned)W;
    const int i0 = omit ? 1 : 0;
    double v[2] = {0.0, 0.0};
    for (unsigned p = blockIdx.x * 256u + threadIdx.x; p < npix; p += gridDim.x * 256u) {
        const int i = (int)(p / (unsigned)W), j = (int)(p - (unsigned)i * (unsigned)W);
        const int im = refl101(i - 1, H), ip = refl101(i + 1, H), jm = refl101(j - 1, W), jp = refl101(j + 1, W);
        auto row = [&](int r) { return k1 * img[(int64_t)r * W + jm] + k0 * img[(int64_t)r * W + j] + k1 * img[(int64_t)r * W + jp]; };
        const float b = k1 * row(im) + k0 * row(i) + k1 * row(ip);  // same arithmetic as k_blur3
        blurred[p] = b;
        if (i >= i0 && i < H - i0 && j >= i0 && j < W - i0) {
            v[0] += (double)b;
            v[1] += (double)b * (double)b;
        }
    }
    if (blockIdx.y == 0) zero_fill_sc1((float *)zero_extra, 4 * n_extra4, gtid, gthreads);  // behind the loads (see k_stats)
    zero_fill_sc1(zero_img, (int64_t)H * W, gtid, gthreads);
    block_sum<2>(v, smem);
    if (threadIdx.x == 0) {
        double *a = stat_slot + kSubStride * (blockIdx.x % nsub);
        atomic_add(&a[0], v[0]);
        atomic_add(&a[1], v[1]);
    }
}

constexpr int kGmTileH = 8, kGmTileW = 32;  // pixels per workgroup of k_stats_gimage_gm (256 threads, one pixel each)
__global__ void __launch_bounds__(256)
k_stats_gimage_gm(const float *__restrict__ in0, int64_t in_stride, int H, int W, ImgArgs ia, int omit, int nsub, double *__restrict__ stat_base, float4 *__restrict__ zero_extra,
                  int64_t n_extra4) {
    __shared__ double smem[2 * 4];
    __shared__ float tile[kGmTileH + 4][kGmTileW + 4 + 1];  // image tile with a halo of 2 (zero outside the image)
    const float *__restrict__ img = in0 + blockIdx.y * in_stride;  // (leading, preloaded arguments: the tile loads leave without waiting for the argument block)
    float *__restrict__ zero_img = ia.zero[blockIdx.y];
    float *__restrict__ G = ia.G[blockIdx.y];
    double *__restrict__ stat_slot = stat_base + blockIdx.y * kStatStride;
    const int64_t gtid = (int64_t)blockIdx.x * 256 + threadIdx.x, gthreads = (int64_t)gridDim.x * 256;
    const int tiles_w = (W + kGmTileW - 1) / kGmTileW;
    const int tr = blockIdx.x / tiles_w, tc = blockIdx.x - tr * tiles_w;
    const int r0 = tr * kGmTileH - 2, c0 = tc * kGmTileW - 2;
    CMAX_STAMP(2, 0);
    stage_tile<kGmTileH + 4, kGmTileW + 4>(tile, img, r0, c0, H, W);
    CMAX_STAMP_AFTER(2, 1, tile[0][0]);
    __syncthreads();
    CMAX_STAMP(2, 2);
    if (blockIdx.y == 0) zero_fill_sc1((float *)zero_extra, 4 * n_extra4, gtid, gthreads);  // behind the loads (see k_stats)
    zero_fill_sc1(zero_img, (int64_t)H * W, gtid, gthreads);
    CMAX_STAMP(2, 3);
    const int i0 = omit ? 1 : 0;
    const float gscale = (float)((2.0 / region_pixels(H, W, omit)) / 8.0) * ia.chain[blockIdx.y];
    const int la = threadIdx.x / kGmTileW, lb = threadIdx.x - la * kGmTileW;  // pixel of this thread inside the tile
    const int i = r0 + 2 + la, j = c0 + 2 + lb;
    double v[2] = {0.0, 0.0};
    // A tile whose pixels all have their 3 x 3 neighbourhood inside Omega (every tile but those along the border): the
    // transpose of the Sobel pair applied to its own responses is ONE 5 x 5 stencil on the image,
    //   Sobel^T Sobel = A(dr) W(dc) + W(dr) A(dc),  A = autocorrelation of (-1, 0, 1) = (-1, 0, 2, 0, -1),  W = that of (1, 2, 1) = (1, 4, 6, 4, 1)
    // -- 25 LDS reads per pixel instead of the 108 of the 18 responses below (workgroup-uniform branch; k_stats_gimage_gm of
    // cfg3 5.7 -> see profiles/r02_ablation.txt).
    const int ri = (int)blockIdx.x / tiles_w * kGmTileH, ci = tc * kGmTileW;
    const bool interior = ri >= i0 + 1 && ri + kGmTileH - 1 <= H - i0 - 2 && ci >= i0 + 1 && ci + kGmTileW - 1 <= W - i0 - 2;
    if (interior) {
        float t5[5][5];
#pragma unroll
        for (int a = 0; a < 5; ++a)
#pragma unroll
            for (int b = 0; b < 5; ++b) t5[a][b] = tile[la + a][lb + b];
        const float gxc = ((t5[3][1] + 2.f * t5[3][2] + t5[3][3]) - (t5[1][1] + 2.f * t5[1][2] + t5[1][3])) * 0.125f;
        const float gyc = ((t5[1][3] + 2.f * t5[2][3] + t5[3][3]) - (t5[1][1] + 2.f * t5[2][1] + t5[3][1])) * 0.125f;
        const float r_outer = -2.f * (t5[0][0] + t5[0][4] + t5[4][0] + t5[4][4]) - 4.f * (t5[0][1] + t5[0][2] + t5[0][3] + t5[4][1] + t5[4][2] + t5[4][3]);
        const float r_mid = -4.f * (t5[1][0] + t5[1][4] + t5[3][0] + t5[3][4]) + 8.f * (t5[1][2] + t5[3][2]);
        const float r_centre = -4.f * (t5[2][0] + t5[2][4]) + 8.f * (t5[2][1] + t5[2][3]) + 24.f * t5[2][2];
        G[(int64_t)i * W + j] = gscale * 0.125f * (r_outer + r_mid + r_centre);
        v[0] = (double)(gxc * gxc + gyc * gyc);
    } else {
        // Tiles along the border (workgroup-uniform; round 6).  They were the kernel's span: every thread computed the 18 Sobel responses of its
        // 3 x 3 neighbourhood (108 LDS reads) and added them under per-tap tests of Omega.  Now in two steps on LDS tiles: the responses of the
        // tile's pixels and a ring of one around them, ZERO outside Omega, once per pixel (12 reads); then the transpose as a plain 3 x 3
        // correlation (18 reads, no tests) -- the same products in the same order, the skipped ones now zeros.
        __shared__ float t_gx[kGmTileH + 2][kGmTileW + 2 + 1], t_gy[kGmTileH + 2][kGmTileW + 2 + 1];
        for (int q = threadIdx.x; q < (kGmTileH + 2) * (kGmTileW + 2); q += 256) {
            const int y = q / (kGmTileW + 2), x = q - y * (kGmTileW + 2);  // response of pixel (r0 + 1 + y, c0 + 1 + x): 3 x 3 window with top-left tile[y][x]
            const float(*t)[kGmTileW + 4 + 1] = tile;
            const int qi = r0 + 1 + y, qj = c0 + 1 + x;
            const bool in_om = qi >= i0 && qi < H - i0 && qj >= i0 && qj < W - i0;
            const float rx = ((t[y + 2][x] + 2.f * t[y + 2][x + 1] + t[y + 2][x + 2]) - (t[y][x] + 2.f * t[y][x + 1] + t[y][x + 2])) * 0.125f;
            const float ry = ((t[y][x + 2] + 2.f * t[y + 1][x + 2] + t[y + 2][x + 2]) - (t[y][x] + 2.f * t[y + 1][x] + t[y + 2][x])) * 0.125f;
            t_gx[y][x] = in_om ? rx : 0.f;
            t_gy[y][x] = in_om ? ry : 0.f;
        }
        __syncthreads();
        // transpose: output pixel q = (i - a, j - b) reads this pixel with tap (a, b); q outside Omega holds zeros
        float s = 0.f;
#pragma unroll
        for (int a = -1; a <= 1; ++a)
#pragma unroll
            for (int b = -1; b <= 1; ++b) {
                const float sx = (float)a * (b == 0 ? 2.f : 1.f);  // SX[a+1][b+1] = a * (2 - |b|)
                const float sy = (float)b * (a == 0 ? 2.f : 1.f);  // SY[a+1][b+1] = b * (2 - |a|)
                s += t_gx[la + 1 - a][lb + 1 - b] * sx + t_gy[la + 1 - a][lb + 1 - b] * sy;
            }
        if (i < H && j < W) G[(int64_t)i * W + j] = gscale * s;
        const float gxc = t_gx[la + 1][lb + 1], gyc = t_gy[la + 1][lb + 1];  // (zero outside Omega, the image included)
        v[0] = (double)(gxc * gxc + gyc * gyc);
    }
    CMAX_STAMP(2, 5);
    block_sum<2>(v, smem);
    CMAX_STAMP(2, 6);
    if (threadIdx.x == 0) atomic_add(&stat_slot[kSubStride * (blockIdx.x % nsub)], v[0]);
    CMAX_STAMP(2, 7);
}

// K2 + K2b in one pass for a focus loss (FocusStencil<COST>, cmax_image_kernels.h), after the border form of k_stats_gimage_gm: the
// image tile with a halo of 2 in LDS; the responses of the tile's pixels and a ring of one around them, ZERO outside Omega, once
// per pixel; the transpose as a plain 3 x 3 correlation on those (no tests of Omega); the energy of the thread's own pixel in fp64
// into the `nsub` accumulators.  G' = (2 / n) sum_s c_s S_s^T (r_s 1_Omega) leaves with the constant chain factor of a plain cost
// (ia.chain) and without one for the normalised forms (kFoldScale: K3 applies it).
// LDS pitch: every access is a ds_read_b32 / ds_write_b32 (bank = dword address mod 32, conflicts within a 32-lane half only).  A
// half-wave reads 32 consecutive floats of one row -- conflict-free at any pitch -- and the staging loops write consecutive q, which
// is conflict-free exactly when a row's pitch equals its width: the response tiles carry no padding.  (The image tile keeps the pitch
// of stage_tile's other user.)
template <int COST>
__global__ void __launch_bounds__(256)
k_stats_gimage_st(const float *__restrict__ in0, int64_t in_stride, int H, int W, ImgArgs ia, int omit, int nsub, double *__restrict__ stat_base, float4 *__restrict__ zero_extra,
                  int64_t n_extra4) {
    using S = FocusStencil<COST>;
    constexpr int kRH = kGmTileH + 2, kRW = kGmTileW + 2;  // responses: the tile and a ring of one
    __shared__ double smem[2 * 4];
    __shared__ float tile[kGmTileH + 4][kGmTileW + 4 + 1];  // image tile with a halo of 2 (zero outside the image)
    __shared__ float t_r[S::kResp][kRH][kRW];
    const float *__restrict__ img = in0 + blockIdx.y * in_stride;  // (leading, preloaded arguments: the tile loads leave without waiting for the argument block)
    float *__restrict__ zero_img = ia.zero[blockIdx.y];
    float *__restrict__ G = ia.G[blockIdx.y];
    double *__restrict__ stat_slot = stat_base + blockIdx.y * kStatStride;
    const int64_t gtid = (int64_t)blockIdx.x * 256 + threadIdx.x, gthreads = (int64_t)gridDim.x * 256;
    const int tiles_w = (W + kGmTileW - 1) / kGmTileW;
    const int tr = blockIdx.x / tiles_w, tc = blockIdx.x - tr * tiles_w;
    const int r0 = tr * kGmTileH - 2, c0 = tc * kGmTileW - 2;
    stage_tile<kGmTileH + 4, kGmTileW + 4>(tile, img, r0, c0, H, W);
    __syncthreads();
    if (blockIdx.y == 0) zero_fill_sc1((float *)zero_extra, 4 * n_extra4, gtid, gthreads);  // behind the loads (see k_stats)
    zero_fill_sc1(zero_img, (int64_t)H * W, gtid, gthreads);
    const int i0 = omit ? 1 : 0;
    const float gscale = (float)(2.0 / region_pixels(H, W, omit)) * ia.chain[blockIdx.y];
    for (int q = threadIdx.x; q < kRH * kRW; q += 256) {
        const int y = q / kRW, x = q - y * kRW;  // response of pixel (r0 + 1 + y, c0 + 1 + x): 3 x 3 window with top-left tile[y][x]
        const int qi = r0 + 1 + y, qj = c0 + 1 + x;
        const bool in_om = qi >= i0 && qi < H - i0 && qj >= i0 && qj < W - i0;
        float n[3][3], r[S::kResp];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) n[a][b] = tile[y + a][x + b];
        S::resp(n, r);
#pragma unroll
        for (int s = 0; s < S::kResp; ++s) t_r[s][y][x] = in_om ? r[s] : 0.f;
    }
    __syncthreads();
    const int la = threadIdx.x / kGmTileW, lb = threadIdx.x - la * kGmTileW;  // pixel of this thread inside the tile
    const int i = r0 + 2 + la, j = c0 + 2 + lb;
    // transpose: output pixel q = (i - a, j - b) reads this pixel with tap (a, b); q outside Omega holds zeros
    float g = 0.f, e = 0.f;
#pragma unroll
    for (int a = -1; a <= 1; ++a)
#pragma unroll
        for (int b = -1; b <= 1; ++b) {
            float r[S::kResp];
#pragma unroll
            for (int s = 0; s < S::kResp; ++s) r[s] = S::tap(s, a, b) != 0.f ? t_r[s][la + 1 - a][lb + 1 - b] : 0.f;
            g += focus_tap_sum<COST, float>(r, a, b);
        }
#pragma unroll
    for (int s = 0; s < S::kResp; ++s) {
        const float rc = t_r[s][la + 1][lb + 1];  // (zero outside Omega, the image included)
        e += S::weight(s) * rc * rc;
    }
    if (i < H && j < W) G[(int64_t)i * W + j] = gscale * g;
    double v[2] = {(double)e, 0.0};
    block_sum<2>(v, smem);
    if (threadIdx.x == 0) atomic_add(&stat_slot[kSubStride * (blockIdx.x % nsub)], v[0]);
}

// Blurred gradient-magnitude cost (the shipped YAML cost), whole image side of one reference time in ONE kernel:
//   Ib = blur3(I)  ->  statistics sum (gx^2 + gy^2) over Omega  ->  G' = (2/n)/8 Sobel^T(gx, gy) 1_Omega  ->  G = blur3^T G'
// (k_blur3 + k_stats_gimage_gm + k_blur3_adj = three dependent launches of ~4.5 us each on a 260 x 346 image).
// One 8 x 32 output tile per workgroup; the stages shrink a halo of 4 -> 3 -> 2 -> 1 -> 0 in LDS.  Arithmetic
// order as in the separate kernels.  G leaves without its chain factor (kFoldScale).
__global__ void __launch_bounds__(256)
k_blur_stats_gimage_gm(const float *__restrict__ in0, int64_t in_stride, int H, int W, ImgArgs ia, float k0, float k1, int omit, int nsub, double *__restrict__ stat_base,
                       float4 *__restrict__ zero_extra, int64_t n_extra4) {
    constexpr int TH = kGmTileH, TW = kGmTileW;
    const float *__restrict__ img = in0 + blockIdx.y * in_stride;  // (leading, preloaded arguments: the tile loads leave without waiting for the argument block)
    float *__restrict__ blurred = ia.blurred[blockIdx.y];
    float *__restrict__ zero_img = ia.zero[blockIdx.y];
    float *__restrict__ G = ia.G[blockIdx.y];
    double *__restrict__ stat_slot = stat_base + blockIdx.y * kStatStride;
    if (blockIdx.y > 0) n_extra4 = 0;  // the flow-gradient buffer is cleared once
    __shared__ double smem[2 * 4];
    __shared__ float t_i[TH + 8][TW + 8 + 1];   // raw image, halo 4 (only in-image cells are read)
    __shared__ float t_b[TH + 6][TW + 6 + 1];   // blurred image, halo 3, zero outside the image (Sobel zero padding)
    __shared__ float t_gx[TH + 4][TW + 4 + 1];  // Sobel/8 responses, halo 2
    __shared__ float t_gy[TH + 4][TW + 4 + 1];
    __shared__ float t_g[TH + 2][TW + 2 + 1];   // G', halo 1, zero outside the image
    const int64_t gtid = (int64_t)blockIdx.x * 256 + threadIdx.x, gthreads = (int64_t)gridDim.x * 256;
    const int tiles_w = (W + TW - 1) / TW;
    const int tr = blockIdx.x / tiles_w, tc = blockIdx.x - tr * tiles_w;
    const int R0 = tr * TH, C0 = tc * TW;  // top-left output pixel
    const int i0 = omit ? 1 : 0;
    auto in_img = [&](int r, int c) { return (unsigned)r < (unsigned)H && (unsigned)c < (unsigned)W; };
    stage_tile<TH + 8, TW + 8>(t_i, img, R0 - 4, C0 - 4, H, W);
    __syncthreads();
    zero_fill_sc1((float *)zero_extra, 4 * n_extra4, gtid, gthreads);  // behind the loads (see k_stats)
    zero_fill_sc1(zero_img, (int64_t)H * W, gtid, gthreads);
    for (int q = threadIdx.x; q < (TH + 6) * (TW + 6); q += 256) {
        const int a = q / (TW + 6), b = q - a * (TW + 6), r = R0 - 3 + a, c = C0 - 3 + b;
        float v = 0.f;
        if (in_img(r, c)) {  // reflect-101 neighbours are at most one pixel away: inside the halo-4 tile
            const int rm = refl101(r - 1, H) - (R0 - 4), rr = r - (R0 - 4), rp = refl101(r + 1, H) - (R0 - 4);
            const int cm = refl101(c - 1, W) - (C0 - 4), cc = c - (C0 - 4), cp = refl101(c + 1, W) - (C0 - 4);
            auto row = [&](int y) { return k1 * t_i[y][cm] + k0 * t_i[y][cc] + k1 * t_i[y][cp]; };
            v = k1 * row(rm) + k0 * row(rr) + k1 * row(rp);
        }
        t_b[a][b] = v;
    }
    __syncthreads();
    for (int q = threadIdx.x; q < (TH + 4) * (TW + 4); q += 256) {
        const int a = q / (TW + 4), b = q - a * (TW + 4);  // response at (R0 - 2 + a, C0 - 2 + b): t_b window rows a..a+2, cols b..b+2
        t_gx[a][b] = ((t_b[a + 2][b] + 2.f * t_b[a + 2][b + 1] + t_b[a + 2][b + 2]) - (t_b[a][b] + 2.f * t_b[a][b + 1] + t_b[a][b + 2])) * 0.125f;
        t_gy[a][b] = ((t_b[a][b + 2] + 2.f * t_b[a + 1][b + 2] + t_b[a + 2][b + 2]) - (t_b[a][b] + 2.f * t_b[a + 1][b] + t_b[a + 2][b])) * 0.125f;
    }
    __syncthreads();
    const float gscale = (float)((2.0 / region_pixels(H, W, omit)) / 8.0) * ia.chain[blockIdx.y];
    for (int q = threadIdx.x; q < (TH + 2) * (TW + 2); q += 256) {
        const int a = q / (TW + 2), b = q - a * (TW + 2), r = R0 - 1 + a, c = C0 - 1 + b;
        float sum = 0.f;
        if (in_img(r, c)) {
#pragma unroll
            for (int da = -1; da <= 1; ++da)
#pragma unroll
                for (int db = -1; db <= 1; ++db) {
                    const int qi = r - da, qj = c - db;  // output pixel of the Sobel that reads (r, c) with tap (da, db)
                    if (qi < i0 || qi >= H - i0 || qj < i0 || qj >= W - i0) continue;
                    const float sx = (float)da * (db == 0 ? 2.f : 1.f), sy = (float)db * (da == 0 ? 2.f : 1.f);
                    sum += t_gx[a + 1 - da][b + 1 - db] * sx + t_gy[a + 1 - da][b + 1 - db] * sy;  // (qi, qj) in halo-2 coordinates
                }
        }
        t_g[a][b] = gscale * sum;
    }
    __syncthreads();
    const int la = threadIdx.x / TW, lb = threadIdx.x - la * TW;
    const int i = R0 + la, j = C0 + lb;
    double v[2] = {0.0, 0.0};
    if (i < H && j < W) {
        const int64_t p = (int64_t)i * W + j;
        blurred[p] = t_b[la + 3][lb + 3];
        G[p] = blur_adj_1d<float>(i, H, k0, k1, [&](int r) {
            return blur_adj_1d<float>(j, W, k0, k1, [&](int c) { return t_g[r - (R0 - 1)][c - (C0 - 1)]; });
        });
        if (i >= i0 && i < H - i0 && j >= i0 && j < W - i0) {
            const float gx = t_gx[la + 2][lb + 2], gy = t_gy[la + 2][lb + 2];
            v[0] = (double)(gx * gx + gy * gy);
        }
    }
    block_sum<2>(v, smem);
    if (threadIdx.x == 0) atomic_add(&stat_slot[kSubStride * (blockIdx.x % nsub)], v[0]);
}

// Blurred variance cost with a gradient, whole image side of one reference time in ONE kernel (k_blur_stats_var +
// k_gimage_blur_adj_var are two dependent launches of ~4.7 + 5.0 us on a 260 x 346 image):
//   G = c blur3^T [ (Ib - mu) 1_Omega ],  c = coef 2 / (n - 1)
// needs the mean of the blurred image before the transpose can start.  The blur is linear: sum_Omega Ib = sum_p I[p] B[p] with
// B = blur3^T 1_Omega = b(r) b(c), b = 1 except within two pixels of the border (border_weight) -- a sum over the VOTES: the number
// of events, plus what K1's workgroups along the border add up (RefArgs::musum).  The mean only matters where B or the mask
// 1_Omega vary (everywhere else the gather's differences cancel it), so the 2^-20 rounding of the fixed-point weights inside
// "four weights add up to 1" is immaterial.  So this kernel reads mu, blurs, sums (for the loss) and writes
// G' = 2 / (n - 1) blur3^T [ (Ib - mu) 1_Omega ]; K3 (kFoldScale) multiplies by coef once the statistics are complete.
// One 8 x 32 output tile per workgroup, halo 2 -> 1 -> 0 in LDS; arithmetic of the blur as in k_blur3.
__global__ void __launch_bounds__(256)
k_blur_stats_adj_var(const float *__restrict__ in0, int64_t in_stride, int H, int W, ImgArgs ia, float k0, float k1, int omit, int nsub, double *__restrict__ stat_base,
                     float4 *__restrict__ zero_extra, int64_t n_extra4, const double *__restrict__ musum, double *__restrict__ musum_next,
                     int64_t n_events) {
    constexpr int TH = 8, TW = 32;
    __shared__ float s_mu;
    if (threadIdx.x < kWave) {  // issued first: the latency hides behind the tile loads
        double m = threadIdx.x < kMuLines ? musum[blockIdx.y * kMuStride + threadIdx.x * kSubStride] : 0.0;
        m = wave_sum_lane63(m);
        if (threadIdx.x == kWave - 1) s_mu = (float)(((double)n_events + m) / region_pixels(H, W, omit));
        // the accumulators of the NEXT evaluation (the other buffer: nobody reads or adds to it during this one), written through
        if (blockIdx.x == 0 && threadIdx.x < kMuLines)
            __hip_atomic_store(&musum_next[blockIdx.y * kMuStride + threadIdx.x * kSubStride], 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const float *__restrict__ img = in0 + blockIdx.y * in_stride;  // (leading, preloaded arguments: the tile loads leave without waiting for the argument block)
    float *__restrict__ blurred = ia.blurred[blockIdx.y];
    float *__restrict__ zero_img = ia.zero[blockIdx.y];
    float *__restrict__ G = ia.G[blockIdx.y];
    double *__restrict__ stat_slot = stat_base + blockIdx.y * kStatStride;
    if (blockIdx.y > 0) n_extra4 = 0;  // the flow-gradient buffer is cleared once
    __shared__ double smem[2 * 4];
    __shared__ float t_i[TH + 4][TW + 4 + 1];  // raw image, halo 2 (only in-image cells are read)
    __shared__ float t_b[TH + 2][TW + 2 + 1];  // blurred image, halo 1
    const int64_t gtid = (int64_t)blockIdx.x * 256 + threadIdx.x, gthreads = (int64_t)gridDim.x * 256;
    const int tiles_w = (W + TW - 1) / TW;
    const int tr = blockIdx.x / tiles_w, tc = blockIdx.x - tr * tiles_w;
    const int R0 = tr * TH, C0 = tc * TW;  // top-left output pixel
    const int i0 = omit ? 1 : 0;
    auto in_img = [&](int r, int c) { return (unsigned)r < (unsigned)H && (unsigned)c < (unsigned)W; };
    CMAX_STAMP(2, 0);
    // Round 6: BRANCH-FREE STENCILS.  tools/timeline.py had the two stencil phases of this kernel at 1.0 + 1.5 us of its workgroups' 4.8
    // (predicated taps: reflection, image and Omega tests per tap, each an LDS round trip behind a branch), and the tiles along the border
    // -- the slowest workgroups ARE the kernel's span -- at the same cost as everybody else.  Now the border is resolved where the tiles
    // are filled: the raw tile is staged WITH its reflect-101 halo (in-image reads only), the forward blur is a plain 3 x 3 stencil, the
    // masked, centred image d = (Ib - mu) 1_Omega gets a tile of its own, and blur^T is a 3 x 3 stencil on d whose per-axis tap weights
    // (k1, k0, k1; 0 beyond the image; 2 k1 for the reflected taps folded back onto rows / columns 1 and n - 2) are set up once per thread.
    {
        constexpr int kN = (TH + 4) * (TW + 4), kIt = (kN + 255) / 256;
        float x[kIt];
#pragma unroll
        for (int u = 0; u < kIt; ++u) {
            const int q = min((int)threadIdx.x + 256 * u, kN - 1), a = q / (TW + 4), b = q - a * (TW + 4);
            const int r = refl101(min(max(R0 - 2 + a, -2), H + 1), H), c = refl101(min(max(C0 - 2 + b, -2), W + 1), W);  // (H, W >= 4: the host's condition for this kernel)
            x[u] = img[(int64_t)r * W + c];
        }
#pragma unroll
        for (int u = 0; u < kIt; ++u) pin(x[u]);  // all loads in flight before the first LDS store (see pin())
#pragma unroll
        for (int u = 0; u < kIt; ++u) {
            const int q = threadIdx.x + 256 * u, a = q / (TW + 4), b = q - a * (TW + 4);
            if (q < kN) t_i[a][b] = x[u];
        }
    }
    CMAX_STAMP_AFTER(2, 1, t_i[0][0]);
    __syncthreads();
    CMAX_STAMP(2, 2);
    zero_fill_sc1((float *)zero_extra, 4 * n_extra4, gtid, gthreads);  // behind the loads (see k_stats)
    zero_fill_sc1(zero_img, (int64_t)H * W, gtid, gthreads);
    __shared__ float t_d[TH + 2][TW + 2 + 1];  // (Ib - mu) 1_Omega, halo 1
    {
        const float mu = s_mu;  // (published by the barrier above)
        for (int q = threadIdx.x; q < (TH + 2) * (TW + 2); q += 256) {
            const int a = q / (TW + 2), b = q - a * (TW + 2), r = R0 - 1 + a, c = C0 - 1 + b;  // t_b[a][b] = pixel (r, c) = t_i[a + 1][b + 1]
            auto row = [&](int y) { return k1 * t_i[y][b] + k0 * t_i[y][b + 1] + k1 * t_i[y][b + 2]; };
            const float vb = k1 * row(a) + k0 * row(a + 1) + k1 * row(a + 2);  // (the products and their order are k_blur3's)
            const bool in_om = r >= i0 && r < H - i0 && c >= i0 && c < W - i0;
            t_b[a][b] = in_img(r, c) ? vb : 0.f;
            t_d[a][b] = in_om ? vb - mu : 0.f;
        }
    }
    CMAX_STAMP(2, 3);
    __syncthreads();
    CMAX_STAMP(2, 4);
    const float gscale = (float)(2.0 / (region_pixels(H, W, omit) - 1.0)) * ia.chain[blockIdx.y];
    const int la = threadIdx.x / TW, lb = threadIdx.x - la * TW;
    const int i = R0 + la, j = C0 + lb;
    double v[2] = {0.0, 0.0};
    if (i < H && j < W) {
        const int64_t p = (int64_t)i * W + j;
        const float b = t_b[la + 1][lb + 1];
        blurred[p] = b;
        // blur^T along one axis of length n at index q: weight of d[q - 1] and of d[q + 1] (blur_adj_1d: a tap beyond the image does not exist;
        // rows / columns 1 and n - 2 also receive the reflected tap of their outer neighbour)
        const float rm = i >= 1 ? (i == 1 ? 2.f * k1 : k1) : 0.f, rp = i + 1 < H ? (i == H - 2 ? 2.f * k1 : k1) : 0.f;
        const float cm = j >= 1 ? (j == 1 ? 2.f * k1 : k1) : 0.f, cp = j + 1 < W ? (j == W - 2 ? 2.f * k1 : k1) : 0.f;
        auto rowadj = [&](int y) { return k0 * t_d[y][lb + 1] + cm * t_d[y][lb] + cp * t_d[y][lb + 2]; };
        G[p] = gscale * (k0 * rowadj(la + 1) + rm * rowadj(la) + rp * rowadj(la + 2));
        if (i >= i0 && i < H - i0 && j >= i0 && j < W - i0) {
            v[0] = (double)b;
            v[1] = (double)b * (double)b;
        }
    }
    CMAX_STAMP(2, 5);
    block_sum<2>(v, smem);
    CMAX_STAMP(2, 6);
    if (threadIdx.x == 0) {
        double *a = stat_slot + kSubStride * (blockIdx.x % nsub);
        atomic_add(&a[0], v[0]);
        atomic_add(&a[1], v[1]);
    }
    CMAX_STAMP(2, 7);
}

// b(p) of B = blur3^T 1_Omega along one axis of length n >= 4 (Omega = [i0, n - i0)): b(0) = b(n - 1), b(1) = b(n - 2), 1 elsewhere
static float border_weight(int p, int n, int i0, float k0, float k1) {
    auto one = [&](int r) { return (r >= i0 && r < n - i0) ? 1.f : 0.f; };
    float s = k0 * one(p);
    if (p - 1 >= 0) s += k1 * one(p - 1);
    if (p + 1 < n) s += k1 * one(p + 1);
    if (p == 1) s += k1 * one(0);      // the reflected taps of blur_adj_1d
    if (p == n - 2) s += k1 * one(n - 1);
    return s;
}

// 2-DoF, plain variance, tangent images (k_vote_tan2): everything the loss and the gradient need, in image space.
//   With m = 1_Omega (zero outside the image) and G = c (I - mu) m:
//     dL/dtheta0 = sum_q E0[q] (G~[q + (1,0)] - G~[q]) = c (S1x - mu S2x),
//       S1x = sum_q E0[q] (m I)[q + (1,0)] - (m I)[q],   S2x = sum_q E0[q] (m[q + (1,0)] - m[q]),   likewise S1y, S2y with F1
//   -- the six sums k_finish_deferred turns into loss, chain factors and gradient (the same quantities the deferred K3
//   gathers per event).  grid (kTanBlocks, n_ref); per-block partials [k][block][6]; clears the planes of the next evaluation.
constexpr int kTanBlocks = 128;
__global__ void __launch_bounds__(256)
k_tan_stats_var(const float *__restrict__ T, float *__restrict__ Tnext, int64_t tstride, int Hp, int Wp, int omit, int normalize,
                const double *__restrict__ tmm, double *__restrict__ part) {
    __shared__ double smem[6 * 4];
    const int k = blockIdx.y;
    const float *__restrict__ I = T + k * tstride;
    const float *__restrict__ E0 = I + (int64_t)Hp * Wp;        // row r of the image is stored row r + 1
    const float *__restrict__ F1 = E0 + (int64_t)(Hp + 1) * Wp;  // column c is stored column c + 1, row stride Wp + 1
    const float ts = normalize ? 1.f : (float)(tmm[1] - tmm[0]);  // the votes carry dt / period
    const int i0 = omit ? 1 : 0;
    const int npix = Hp * Wp;
    auto mask = [&](int r, int c) -> bool { return r >= i0 && r < Hp - i0 && c >= i0 && c < Wp - i0; };
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int p = blockIdx.x * 256 + threadIdx.x; p < npix; p += gridDim.x * 256) {
        const int r = p / Wp, c = p - r * Wp;
        const bool m = mask(r, c), md = r + 1 < Hp && mask(r + 1, c), mr = c + 1 < Wp && mask(r, c + 1);
        const float x = m ? I[p] : 0.f, xd = md ? I[p + Wp] : 0.f, xr = mr ? I[p + 1] : 0.f;
        const float e = E0[(int64_t)(r + 1) * Wp + c] * ts, f = F1[(int64_t)r * (Wp + 1) + c + 1] * ts;
        v[0] += (double)(e * (xd - x));
        v[1] += (double)(f * (xr - x));
        v[2] += (double)(e * ((md ? 1.f : 0.f) - (m ? 1.f : 0.f)));
        v[3] += (double)(f * ((mr ? 1.f : 0.f) - (m ? 1.f : 0.f)));
        if (r == 0) {  // votes whose upper corner lies one row above the image
            const float eu = E0[c] * ts;
            v[0] += (double)(eu * x);
            v[2] += (double)(eu * (m ? 1.f : 0.f));
        }
        if (c == 0) {  // ... one column left of it
            const float fl = F1[(int64_t)r * (Wp + 1)] * ts;
            v[1] += (double)(fl * x);
            v[3] += (double)(fl * (m ? 1.f : 0.f));
        }
        v[4] += (double)x;
        v[5] += (double)x * (double)x;
    }
    if (Tnext) zero_fill_sc1(Tnext + k * tstride, tstride, (int64_t)blockIdx.x * 256 + threadIdx.x, (int64_t)gridDim.x * 256);
    // the four gradient sums go over the wave in fp32 (DPP adds; their terms carry fp32 rounding already) and in fp64 across
    // waves and workgroups -- as in the deferred K3 -- while the two image sums, summed pixel by pixel here, stay fp64 throughout (a
    // block_sum of six doubles is 36 dependent v_add_f64 behind 72 DPP moves)
    float *s_f = reinterpret_cast<float *>(smem + 2 * 4);  // [4][4] floats behind the doubles of block_sum<2>
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float w = (float)v[q];
        w += dpp_f<kDppRowShr1>(w);
        w += dpp_f<kDppRowShr2>(w);
        w += dpp_f<kDppRowShr4>(w);
        w += dpp_f<kDppRowShr8>(w);
        w += dpp_f<kDppRowBcast15>(w);
        w += dpp_f<kDppRowBcast31>(w);
        if (lane == kWave - 1) s_f[q * 4 + wave] = w;
    }
    double im[2] = {v[4], v[5]};
    block_sum<2>(im, smem);  // (its barriers also publish s_f)
    if (threadIdx.x == 0) {
        double *o = part + ((int64_t)k * gridDim.x + blockIdx.x) * 6;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = (double)s_f[q * 4] + (double)s_f[q * 4 + 1] + (double)s_f[q * 4 + 2] + (double)s_f[q * 4 + 3];
        o[4] = im[0];
        o[5] = im[1];
    }
}

__global__ void k_finalize(ObjParams op, const double *__restrict__ stat, double *__restrict__ result) {
    if (threadIdx.x == 0 && blockIdx.x == 0) write_result(op, stat, result);
}

// K2b: G[p] = dL/dv_k * dv_k/dI[p]   (needed when a blur transpose follows or for the grad-mag cost;
//      the plain-variance gradient is folded into K3 instead)
template <int COST>
__global__ void __launch_bounds__(256)
k_gimage(const float *__restrict__ img, ObjParams op, int k, const double *__restrict__ stat, float *__restrict__ G, int64_t bs = 0) {
    k += blockIdx.y;  // blockIdx.y: reference time of a batch (element stride bs)
    img += blockIdx.y * bs;
    G += blockIdx.y * bs;
    const int H = op.H, W = op.W;
    const int i0 = op.omit ? 1 : 0;
    const double npix = region_pixels(H, W, op.omit);
    double mu = 0.0;
    const double coef = chain_coef<true>(op, stat, k, &mu);  // every wave is converged here
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (int64_t)H * W) return;
    const int i = (int)(p / W), j = (int)(p % W);
    if (COST == CMAX_COST_VARIANCE) {
        const bool in = (i >= i0) && (i < H - i0) && (j >= i0) && (j < W - i0);
        G[p] = in ? (float)(coef * 2.0 * ((double)img[p] - mu) / (npix - 1.0)) : 0.f;
    } else if constexpr (COST == CMAX_COST_GRADMAG) {
        G[p] = (float)(coef * (2.0 / npix) / 8.0) * sobel8_adj_f32(img, H, W, i0, i, j);
    } else if constexpr (COST != CMAX_COST_VARIANCE) {  // a focus loss (FocusStencil, cmax_image_kernels.h)
        float v5[5][5];
        focus_load<2, float>(img, H, W, i, j, v5);
        G[p] = (float)(coef * (2.0 / npix)) * focus_adj<COST, float>(v5, H, W, i0, i, j);
    }
}

__global__ void __launch_bounds__(256)
k_gimage_blur_adj_var(ImgArgs ia, ObjParams op, const double *__restrict__ stat, float k0, float k1) {
    const int k = blockIdx.y;
    const float *__restrict__ blurred = ia.in[k];
    float *__restrict__ G = ia.G[k];
    const int H = op.H, W = op.W, i0 = op.omit ? 1 : 0;
    double mud = 0.0;
    const double coef = chain_coef<true>(op, stat, k, &mud);  // every wave is converged here
    const float c2 = (float)(coef * 2.0 / (region_pixels(H, W, op.omit) - 1.0)), mu = (float)mud;
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (int64_t)H * W) return;
    const int i = (int)(p / W), j = (int)(p % W);
    auto g = [&](int r, int c) -> float {  // dL/d(blurred image): what k_gimage<VARIANCE> writes
        const bool in = (r >= i0) && (r < H - i0) && (c >= i0) && (c < W - i0);
        return in ? c2 * (blurred[(int64_t)r * W + c] - mu) : 0.f;
    };
    G[p] = blur_adj_1d<float>(i, H, k0, k1, [&](int r) { return blur_adj_1d<float>(j, W, k0, k1, [&](int c) { return g(r, c); }); });
}

// T2a: st[0] += sum_Omega dI (variance) or sum_Omega (gx dgx + gy dgy) (grad-mag); st[1] += sum_Omega I dI
template <int COST>
__global__ void __launch_bounds__(256)
k_stats_tan(const float *__restrict__ img, const float *__restrict__ dimg, int H, int W, int omit, int nsub, double *__restrict__ st,
            int64_t bs) {
    __shared__ double smem[2 * 4];
    img += blockIdx.y * bs;
    dimg += blockIdx.y * bs;
    st += blockIdx.y * kStatStride;
    const unsigned npix = (unsigned)H * (unsigned)W;
    const int i0 = omit ? 1 : 0;
    double v[2] = {0.0, 0.0};
    for (unsigned p = blockIdx.x * 256u + threadIdx.x; p < npix; p += gridDim.x * 256u) {
        const int r = (int)(p / (unsigned)W), c = (int)(p - (unsigned)r * (unsigned)W);
        if (r < i0 || r >= H - i0 || c < i0 || c >= W - i0) continue;
        if (COST == CMAX_COST_VARIANCE) {
            const double d = (double)dimg[p];
            v[0] += d;
            v[1] += d * (double)img[p];
        } else if constexpr (COST == CMAX_COST_GRADMAG) {
            float gx, gy, hx, hy;
            sobel8_f32(img, H, W, r, c, gx, gy);
            sobel8_f32(dimg, H, W, r, c, hx, hy);
            v[0] += (double)(gx * hx + gy * hy);
        } else if constexpr (COST != CMAX_COST_VARIANCE) {  // a focus loss: sum_s c_s r_s(I) r_s(dI)
            float n[3][3], m[3][3];
            focus_load<1, float>(img, H, W, r, c, n);
            focus_load<1, float>(dimg, H, W, r, c, m);
            v[0] += (double)focus_dot<COST, float>(n, m);
        }
    }
    block_sum<2>(v, smem);
    if (threadIdx.x == 0) {
        double *a = st + kSubStride * (blockIdx.x % nsub);
        atomic_add(&a[0], v[0]);
        if (COST == CMAX_COST_VARIANCE) atomic_add(&a[1], v[1]);
    }
}

// T2b: G'[p] = phi' * dG0[dI] + phi'' * dv * G0[I]   (stat: sums of I; st: tangent sums, slot-local pointer)
template <int COST>
__global__ void __launch_bounds__(256)
k_gimage_tan(const float *__restrict__ img, const float *__restrict__ dimg, ObjParams op, int k, const double *__restrict__ stat,
             const double *__restrict__ st, float *__restrict__ Gp, int64_t bs) {
    k += blockIdx.y;
    img += blockIdx.y * bs;
    dimg += blockIdx.y * bs;
    Gp += blockIdx.y * bs;
    st += blockIdx.y * kStatStride;
    const int H = op.H, W = op.W, i0 = op.omit ? 1 : 0;
    const double npix = region_pixels(H, W, op.omit);
    double acc[2], tacc[2] = {0.0, 0.0};
    stat_sum(stat, k, op.nsub, acc);
    for (int u = 0; u < op.nsub; ++u) {
        tacc[0] += st[kSubStride * u];
        tacc[1] += st[kSubStride * u + 1];
    }
    double mu = 0.0;
    const double v = contrast_value(COST, acc, npix, &mu);
    // phi(v): loss contribution of this reference time; phi' = chain factor, phi'' its derivative
    double p1, p2 = 0.0;
    if (!op.normalized) p1 = op.mult[k] * (op.minimize ? -1.0 : 1.0);
    else {
        const double v_orig = orig_value(op, stat);
        if (op.minimize) {
            p1 = -op.mult[k] * v_orig / (v * v);
            p2 = 2.0 * op.mult[k] * v_orig / (v * v * v);
        } else p1 = op.mult[k] / v_orig;
    }
    if (op.negate) {
        p1 = -p1;
        p2 = -p2;
    }
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (int64_t)H * W) return;
    const int i = (int)(p / W), j = (int)(p % W);
    if (COST == CMAX_COST_VARIANCE) {
        const double dmean = tacc[0] / npix;
        const double dv = 2.0 / (npix - 1.0) * (tacc[1] - mu * tacc[0]);  // <G0, dI>
        const bool in = (i >= i0) && (i < H - i0) && (j >= i0) && (j < W - i0);
        Gp[p] = in ? (float)((p1 * 2.0 * ((double)dimg[p] - dmean) + p2 * dv * 2.0 * ((double)img[p] - mu)) / (npix - 1.0)) : 0.f;
    } else if constexpr (COST == CMAX_COST_GRADMAG) {
        const double dv = 2.0 / npix * tacc[0];
        const double c = (2.0 / npix) / 8.0;
        Gp[p] = (float)(p1 * c) * sobel8_adj_f32(dimg, H, W, i0, i, j) + (float)(p2 * dv * c) * sobel8_adj_f32(img, H, W, i0, i, j);
    } else if constexpr (COST != CMAX_COST_VARIANCE) {  // a focus loss is quadratic: the same operator on the tangent image, plus the p2 term of the normalised forms
        const double dv = 2.0 / npix * tacc[0];
        const double c = 2.0 / npix;
        float v5[5][5];
        focus_load<2, float>(dimg, H, W, i, j, v5);
        float g = (float)(p1 * c) * focus_adj<COST, float>(v5, H, W, i0, i, j);
        if (p2 != 0.0) {
            focus_load<2, float>(img, H, W, i, j, v5);
            g += (float)(p2 * dv * c) * focus_adj<COST, float>(v5, H, W, i0, i, j);
        }
        Gp[p] = g;
    }
}

// fixed-point vote images -> fp32 images (blockIdx.y = image), the integer image is left zero for the next evaluation
__global__ void __launch_bounds__(256) k_fixed_to_image(FixedArgs fa, int64_t npix) {
    long long *__restrict__ src = fa.src[blockIdx.y];
    float *__restrict__ dst = fa.dst[blockIdx.y];
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < npix; p += (int64_t)gridDim.x * 256) {
        const long long v = src[p];
        dst[p] = (float)((double)v * (fa.inv_fixk[blockIdx.y] != 0.0 ? fa.inv_fixk[blockIdx.y] : fa.inv_fix));  // one rounding, of the exact sum
        if (v != 0) src[p] = 0;
    }
}

// max |image| of one statistics slot (order-free: integer max of the magnitude bits); imax[slot] zeroed by the caller
__global__ void __launch_bounds__(256) k_image_absmax(ImgArgs ia, int64_t npix, int slot0, unsigned *__restrict__ imax) {
    // one atomicMax per WORKGROUP on the image's word, and at most 256 workgroups per image: same-address atomics serialise at
    // ~12 ns each -- one per wave of a 1200-workgroup grid was 56 of the deterministic cfg3 evaluation's 225 us
    __shared__ unsigned s_m[4];
    const float *__restrict__ img = ia.in[blockIdx.y];
    unsigned m = 0u;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < npix; p += (int64_t)gridDim.x * 256)
        m = max(m, __float_as_uint(img[p]) & 0x7FFFFFFFu);
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, kWave));
    if ((threadIdx.x & (kWave - 1)) == 0) s_m[threadIdx.x / kWave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = max(max(s_m[0], s_m[1]), max(s_m[2], s_m[3]));
        if (m) atomicMax(&imax[slot0 + blockIdx.y], m);
    }
}
__global__ void __launch_bounds__(256) k_fixed_to_grad(long long *__restrict__ g64, float *__restrict__ grad, int64_t n, const double *__restrict__ inv_scale) {
    const double is = inv_scale[0];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const long long v = g64[i];
        grad[i] = (float)((double)v * is);
        if (v != 0) g64[i] = 0;
    }
}

// 2-DoF: gradient = sum over reference times and segments of the fixed-point partials (integer sums: any order)
__global__ void __launch_bounds__(256) k_finish_det(long long *__restrict__ gpart64, int nseg, int n_ref, const double *__restrict__ inv_scale,
                                                    double *__restrict__ gtheta) {
    __shared__ long long s_acc[2];
    double g0 = 0.0, g1 = 0.0;
    for (int k = 0; k < n_ref; ++k) {
        if (threadIdx.x < 2) s_acc[threadIdx.x] = 0;
        __syncthreads();
        long long a0 = 0, a1 = 0;
        long long *gp = gpart64 + (int64_t)k * nseg * 2;
        for (int i = threadIdx.x; i < nseg; i += blockDim.x) {
            a0 += gp[2 * i];
            a1 += gp[2 * i + 1];
        }
        atomic_add_i64(&s_acc[0], a0);
        atomic_add_i64(&s_acc[1], a1);
        __syncthreads();
        if (threadIdx.x == 0) {
            g0 += (double)s_acc[0] * inv_scale[k];  // reference times in fixed order
            g1 += (double)s_acc[1] * inv_scale[k];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        gtheta[0] = g0;
        gtheta[1] = g1;
    }
}

// 2-DoF objectives that keep statistics (everything but the deferred plain variance): K3 left sum dt g in doubles 0, 1 of kRawLines
// lines per reference time; gradient = their sum over lines and reference times.  One wave.  result_src -> result_dst / flag / seq:
// cmax_objective_host -- copy the result K3's first workgroup wrote to the device into pinned host memory beside the gradient and
// publish a run counter behind both.
__global__ void __launch_bounds__(64)
k_finish_lines(const double *__restrict__ raw, int n_ref, double *__restrict__ gtheta, const double *__restrict__ result_src,
               double *__restrict__ result_dst, volatile unsigned long long *flag, unsigned long long seq) {
    const int lane = threadIdx.x;
    double g0 = 0.0, g1 = 0.0;
    typedef double double2_v __attribute__((ext_vector_type(2)));
    const int line = lane < kRawLines ? lane : kRawLines - 1;  // unconditional 16-byte loads, masked afterwards (see k_finish_raw)
    double2_v a[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        a[k] = double2_v{0.0, 0.0};
        if (k < n_ref) a[k] = *reinterpret_cast<const double2_v *>(raw + (int64_t)k * kRawStride + line * kSubStride);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        g0 += lane < kRawLines ? a[k].x : 0.0;
        g1 += lane < kRawLines ? a[k].y : 0.0;
    }
    g0 = wave_sum_lane63(g0);
    g1 = wave_sum_lane63(g1);
    if (result_dst && lane < 8) result_dst[lane] = result_src[lane];
    if (lane == kWave - 1) {
        gtheta[0] = g0;
        gtheta[1] = g1;
    }
    if (flag) {  // (ONE wave: every lane's stores above have left it when the fence returns, so lane 63 may publish for all of them)
        __threadfence_system();
        if (lane == kWave - 1) *flag = seq;
    }
}

// 2-DoF only: gradient = sum of the per-segment partials of every K3 launch (one workgroup).
__global__ void __launch_bounds__(256)
k_finish(const double *__restrict__ gpart, int n_gpart, double *__restrict__ gtheta) {
    __shared__ double s_red[2 * 4];
    double acc[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < n_gpart; i += blockDim.x) {
        acc[0] += gpart[2 * i];
        acc[1] += gpart[2 * i + 1];
    }
    block_sum<2>(acc, s_red);
    if (threadIdx.x == 0) {
        gtheta[0] = acc[0];
        gtheta[1] = acc[1];
    }
}

// 2-DoF, plain variance, deferred statistics: K3 left (S1x, S1y, S2x, S2y, sum I, sum I^2) per reference time with
//   S1 = sum_e dt * bilinear-difference(1_Omega I),  S2 = the same of 1_Omega.  With G = c (I - mu) 1_Omega,
//   c = 2 coef / (n - 1):  dL/dtheta = sum_k c_k (S1_k - mu_k S2_k);  loss and coef_k from the image sums.
// One function for the device (k_finish_deferred, k_finish_raw) and the host (cmax_finalize_raw_host).
__host__ __device__ inline void finalize_deferred(const ObjParams &op, const double (*S)[6], double v_orig, double *result, double *gtheta) {
    const int i0 = op.omit ? 1 : 0;
    const double npix = (double)(op.H - 2 * i0) * (double)(op.W - 2 * i0);
    double loss = 0.0, g0 = 0.0, g1 = 0.0;
    for (int k = 0; k < op.n_ref; ++k) {
        const double mu = S[k][4] / npix;
        const double v = (S[k][5] - S[k][4] * mu) / (npix - 1.0);  // unbiased like torch.var, image_variance.py:55
        result[1 + k] = v;
        double coef;
        if (!op.normalized) {
            loss += op.mult[k] * (op.minimize ? -v : v);
            coef = op.mult[k] * (op.minimize ? -1.0 : 1.0);
        } else {
            loss += op.mult[k] * (op.minimize ? v_orig / v : v / v_orig);
            coef = op.mult[k] * (op.minimize ? -v_orig / (v * v) : 1.0 / v_orig);
        }
        if (op.negate) coef = -coef;
        const double c = coef * 2.0 / (npix - 1.0);
        g0 += c * (S[k][0] - mu * S[k][2]);
        g1 += c * (S[k][1] - mu * S[k][3]);
    }
    result[0] = op.negate ? -loss : loss;
    result[5] = v_orig;
    if (gtheta) {
        gtheta[0] = g0;
        gtheta[1] = g1;
    }
}

// per-block partials [n_ref][nseg][6] -> loss + gradient (the tangent-image path: k_tan_stats_var leaves kTanBlocks partials)
__global__ void __launch_bounds__(256)
k_finish_deferred(ObjParams op, const double *__restrict__ stat, const double *__restrict__ gpart, int nseg,
                  double *__restrict__ result, double *__restrict__ gtheta) {
    __shared__ double s_red[6 * 4];
    __shared__ double s_sum[4][6];
    for (int k = 0; k < op.n_ref; ++k) {
        double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const double *gp = gpart + (int64_t)k * nseg * 6;
        for (int i = threadIdx.x; i < nseg; i += blockDim.x) {
#pragma unroll
            for (int q = 0; q < 6; ++q) acc[q] += gp[6 * i + q];
        }
        block_sum<6>(acc, s_red);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int q = 0; q < 6; ++q) s_sum[k][q] = acc[q];
        }
    }
    if (threadIdx.x != 0) return;
    finalize_deferred(op, s_sum, op.normalized ? orig_value(op, stat) : 0.0, result, gtheta);
}

// The raw sums of the deferred K3 (kRawLines lines of six doubles per reference time) -> loss + gradient: ONE wave, lane l
// loads line l (all loads of all reference times in flight together), DPP sums, lane 63 finishes.  This launch exists only
// for callers that want the result ON THE DEVICE (cmax_objective); cmax_objective_raw / cmax_objective_host fold on the host.
// flag / seq (cmax_objective_host): result and gtheta are PINNED HOST memory; after they are visible system-wide the kernel writes
// the run counter `seq` behind them, which the host polls -- no copy engine, no hipStreamQuery.
__global__ void __launch_bounds__(64)
k_finish_raw(const double *__restrict__ raw, int n_ref, ObjParams op, const double *__restrict__ stat, double *__restrict__ result, double *__restrict__ gtheta,
             volatile unsigned long long *flag = nullptr, unsigned long long seq = 0) {
    // (raw and n_ref lead the parameter list: they arrive in SGPRs -- kernel-argument preload -- and the loads below leave at once, while
    // everything finalize_deferred needs is fetched from the argument block beside them: one round trip less in a one-wave kernel)
    // blockIdx.x = candidate motion of cmax_objective_batch (one workgroup otherwise)
    raw += (int64_t)blockIdx.x * n_ref * kRawStride;
    const int lane = threadIdx.x;
    double v[4][6];
    // every lane loads ITS line's six doubles as three 16-byte loads, all issued before the first use (lanes >= kRawLines re-read
    // the last line and are zeroed by a select: `lane < 32 ? raw[..] : 0` put each of the 6 x n_ref loads into an exec-masked
    // block with its own s_waitcnt -- six dependent round trips in a kernel that has only this one wave).  Likewise the reference
    // times: `if (k < n_ref)` around the loads of time k was a scalar branch per k whose block merged the loaded registers with the
    // zeros and WAITED for them there, in front of the next k's loads and of the fetch of `op` (profiles/head_loads_isa.txt) -- a time
    // the launch does not have re-reads the last one it has, and is never looked at.
    typedef double double2_v __attribute__((ext_vector_type(2)));
    const int line = lane < kRawLines ? lane : kRawLines - 1;
    double2_v ld[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int kk = k < n_ref ? k : max(n_ref - 1, 0);
        const double2_v *src = reinterpret_cast<const double2_v *>(raw + (int64_t)kk * kRawStride + line * kSubStride);
#pragma unroll
        for (int q = 0; q < 3; ++q) ld[k][q] = src[q];
    }
    // what finalize_deferred reads of the argument block, fetched while the lines are on their way (the barrier keeps the loads above in front)
    __builtin_amdgcn_sched_barrier(0);
    // (values as loaded only, and no use of the argument block above the barrier: a use is a wait, and it landed in front of the line loads)
    asm volatile("" ::"s"(op.n_ref), "s"(op.normalized), "s"(op.minimize), "s"(op.negate), "s"(op.omit), "s"(op.H), "s"(op.W), "s"(result), "s"(gtheta));
    result += 8 * blockIdx.x;
    if (gtheta) gtheta += 2 * blockIdx.x;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int q = 0; q < 6; ++q) v[k][q] = lane < kRawLines ? ((q & 1) ? ld[k][q >> 1].y : ld[k][q >> 1].x) : 0.0;
    const double v_orig = op.normalized ? orig_value<true>(op, stat) : 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k >= op.n_ref) break;  // (uniform: 18 VALU instructions per sum, and there is only this one wave)
#pragma unroll
        for (int q = 0; q < 6; ++q) v[k][q] = wave_sum_lane63(v[k][q]);
    }
    if (lane == kWave - 1) {
        // (n_ref as a constant per branch, as in finish_raw_step_wave: finalize_deferred's loop unrolls and v[][] stays in registers --
        // indexed by a run-time k it was 208 bytes of scratch per lane, written behind the loads and read back here)
        ObjParams on = op;
        double res[8], g[2];
        switch (op.n_ref) {
            case 1: on.n_ref = 1; finalize_deferred(on, v, v_orig, res, g); break;
            case 2: on.n_ref = 2; finalize_deferred(on, v, v_orig, res, g); break;
            case 3: on.n_ref = 3; finalize_deferred(on, v, v_orig, res, g); break;
            default: on.n_ref = 4; finalize_deferred(on, v, v_orig, res, g); break;
        }
        result[0] = res[0];
        result[5] = res[5];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < op.n_ref) result[1 + k] = res[1 + k];
        if (gtheta) {
            gtheta[0] = g[0];
            gtheta[1] = g[1];
        }
        if (flag) {
            __threadfence_system();
            *flag = seq;
        }
    }
}

// k_finish_raw for an iteration of the device-resident descent (cmax_objective_descend, src/solver/base.py:840-881): the same wave, the
// same three 16-byte loads per lane in flight, the same DPP sums and finalize_deferred -- and lane 63 then applies the optimiser's step to
// theta in place (cmax_descent.h, nx = 2), so that an iteration stays at K1 -> K3 -> ONE finishing launch.  result / gtheta: device memory.
// (one body for the single-start launch and its batched sibling below: the wave of one candidate)
// (its loads keep the `if (k < n_ref)` form k_finish_raw had: changing them is a change to the descent's kernels, which no listing or
// measurement of profiles/head_loads_* covers -- left for a change of its own)
__device__ __forceinline__ void finish_raw_step_wave(const double *__restrict__ raw, int n_ref, const ObjParams &op, const double *__restrict__ stat,
                                                     double *__restrict__ result, double *__restrict__ gtheta, const DescentArgs &step) {
    const int lane = threadIdx.x;
    double v[4][6];
    typedef double double2_v __attribute__((ext_vector_type(2)));
    const int line = lane < kRawLines ? lane : kRawLines - 1;  // unconditional loads, masked afterwards (see k_finish_raw)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int q = 0; q < 6; ++q) v[k][q] = 0.0;
        if (k < n_ref) {  // uniform
            const double2_v *src = reinterpret_cast<const double2_v *>(raw + (int64_t)k * kRawStride + line * kSubStride);
            const double2_v a = src[0], b = src[1], c = src[2];
            v[k][0] = a.x;
            v[k][1] = a.y;
            v[k][2] = b.x;
            v[k][3] = b.y;
            v[k][4] = c.x;
            v[k][5] = c.y;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int q = 0; q < 6; ++q) v[k][q] = lane < kRawLines ? v[k][q] : 0.0;
    const double v_orig = op.normalized ? orig_value<true>(op, stat) : 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k >= op.n_ref) break;  // (uniform)
#pragma unroll
        for (int q = 0; q < 6; ++q) v[k][q] = wave_sum_lane63(v[k][q]);
    }
    if (lane == kWave - 1) {
        // (n_ref as a constant per branch: finalize_deferred's loop over the reference times unrolls and v[][] stays in registers -- indexed
        // by a run-time k it is 208 bytes of scratch per lane)
        ObjParams on = op;
        double res[8], g[2];
        switch (op.n_ref) {
            case 1: on.n_ref = 1; finalize_deferred(on, v, v_orig, res, g); break;
            case 2: on.n_ref = 2; finalize_deferred(on, v, v_orig, res, g); break;
            case 3: on.n_ref = 3; finalize_deferred(on, v, v_orig, res, g); break;
            default: on.n_ref = 4; finalize_deferred(on, v, v_orig, res, g); break;
        }
        result[0] = res[0];
        result[5] = res[5];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < op.n_ref) result[1 + k] = res[1 + k];
        gtheta[0] = g[0];
        gtheta[1] = g[1];
        const double L = res[0], g0 = g[0], g1 = g[1];
        const DescentDecision d = descent_decide(step, L, !(isfinite(L) && isfinite(g0) && isfinite(g1)));
        descent_element(step, d, 0, g0);
        descent_element(step, d, 1, g1);
        descent_publish(step, d, L);
        if (step.it == step.n_iter - 1 && step.flag) {
            __threadfence_system();
            *step.flag = step.seq;
        }
    }
}

__global__ void __launch_bounds__(64)
k_finish_raw_step(const double *__restrict__ raw, int n_ref, ObjParams op, const double *__restrict__ stat, double *__restrict__ result, double *__restrict__ gtheta,
                  DescentArgs step) {
    finish_raw_step_wave(raw, n_ref, op, stat, result, gtheta, step);
}

// The same for the K candidates of cmax_objective_descend_batch: blockIdx.x = candidate, one wave each, on that candidate's raw lines (as
// k_finish_raw indexes them), result block, gradient, theta (the double[K][2] the batched K1 / K3 read through RefArgs::z_motion) and
// descent state (st_stride doubles apart).  Every candidate decides, steps and stops on its own control block; nothing is published to
// the host from here (step.res_pinned and step.flag are null: the call copies the states out behind the last launch).
__global__ void __launch_bounds__(64)
k_finish_raw_step_batch(const double *__restrict__ raw, int n_ref, ObjParams op, const double *__restrict__ stat, double *__restrict__ result,
                        double *__restrict__ gtheta, DescentArgs step, int64_t st_stride) {
    const int64_t z = blockIdx.x;
    step.x += 2 * z;
    step.st += z * st_stride;
    finish_raw_step_wave(raw + z * n_ref * kRawStride, n_ref, op, stat, result + 8 * z, gtheta + 2 * z, step);
}

// ---------------------------------------------------------------------------------------------
// host-side orchestration
// ---------------------------------------------------------------------------------------------
static float ref_fraction(int ref_mode, double frac) {
    if (ref_mode == CMAX_REF_FIRST) return 0.f;
    if (ref_mode == CMAX_REF_LAST) return 1.f;
    return (float)frac;
}
// ... and what fp32 lost of it (zero for the named directions and every dyadic fraction)
static float ref_fraction_lo(int ref_mode, double frac) {
    if (ref_mode == CMAX_REF_FIRST || ref_mode == CMAX_REF_LAST) return 0.f;
    return (float)(frac - (double)(float)frac);
}
// the reference times of a launch (RefArgs::d / d_lo)
static void fill_ref_times(RefArgs &ra, int n_ref, const int *ref_mode, const double *ref_frac) {
    for (int k = 0; k < n_ref; ++k) {
        ra.d[k] = ref_fraction(ref_mode[k], ref_frac[k]);
        ra.d_lo[k] = ref_fraction_lo(ref_mode[k], ref_frac[k]);
    }
}

// f(int_c<MODEL>{}) for the motion model of an objective (check_objective_args: one of the three)
template <class F>
static void with_model(int model, F &&f) {
    if (model == CMAX_MODEL_2DOF) f(int_c<CMAX_MODEL_2DOF>{});
    else if (model == CMAX_MODEL_DENSE) f(int_c<CMAX_MODEL_DENSE>{});
    else f(int_c<CMAX_MODEL_VOXEL>{});
}
// f(int_c<COST>{}) for the contrast of an objective (check_objective_args: one of the five)
template <class F>
static void with_cost(int cost, F &&f) {
    switch (cost) {
    case CMAX_COST_VARIANCE: f(int_c<CMAX_COST_VARIANCE>{}); break;
    case CMAX_COST_GRADMAG: f(int_c<CMAX_COST_GRADMAG>{}); break;
    case CMAX_COST_MEAN_SQUARE: f(int_c<CMAX_COST_MEAN_SQUARE>{}); break;
    case CMAX_COST_LAPLACIAN: f(int_c<CMAX_COST_LAPLACIAN>{}); break;
    case CMAX_COST_HESSIAN: f(int_c<CMAX_COST_HESSIAN>{}); break;
    default: break;  // (refused by cost_known at every entry)
    }
}
// the focus losses (FocusStencil, cmax_image_kernels.h): the general path K1 -> image kernel(s) -> K3, none of the variance shortcuts
static bool cost_is_focus(int cost) { return cost == CMAX_COST_MEAN_SQUARE || cost == CMAX_COST_LAPLACIAN || cost == CMAX_COST_HESSIAN; }
static bool cost_known(int cost) { return cost == CMAX_COST_VARIANCE || cost == CMAX_COST_GRADMAG || cost_is_focus(cost); }
template <class F>
static void with_focus_cost(int cost, F &&f) {
    if (cost == CMAX_COST_MEAN_SQUARE) f(int_c<CMAX_COST_MEAN_SQUARE>{});
    else if (cost == CMAX_COST_LAPLACIAN) f(int_c<CMAX_COST_LAPLACIAN>{});
    else if (cost == CMAX_COST_HESSIAN) f(int_c<CMAX_COST_HESSIAN>{});
}

static EvView ev_view(const cmax_handle_s *h) {
    EvView ev;
    ev.ev = h->evp;
    ev.rx = h->rx;
    ev.ry = h->ry;
    ev.rl = h->rl;
    ev.tau64 = h->n_time_bin > 0 ? h->tau64 : nullptr;
    return ev;
}

static WarpParams warp_params(const cmax_handle_s *h, const float *motion, int T, int ref_mode, double frac, int normalize, int motion_f64 = 0) {
    // wp.d is what the single-reference kernels (tangent / HVP) read; the batched kernels take it from RefArgs
    WarpParams wp;
    wp.H = h->H;
    wp.W = h->W;
    wp.Hp = h->Hp;
    wp.Wp = h->Wp;
    wp.ph = h->ph;
    wp.pw = h->pw;
    wp.T = T;
    wp.ntc = h->ntc;
    wp.d = ref_fraction(ref_mode, frac);
    wp.d_lo = ref_fraction_lo(ref_mode, frac);
    wp.normalize = normalize;
    wp.motion_f64 = motion_f64;
    wp.tmm = h->d_tmm;  // ALWAYS the handle's own pair (the base of its per-batch allocation: 16-byte aligned, never null once events are set):
                        // K1 / K3 load it unconditionally, as one 16-byte scalar load, whatever normalize_t and the model (load_head_words)
    wp.motion = motion;
    return wp;
}

// What a K1 launch does besides voting -- decided by eval_plan for the K1 of a whole evaluation; nothing for a plain vote (cmax_iwe, the
// un-warped image, the second-order product)
struct VoteJobs {
    bool publish_windows = false;  // K3 of the same evaluation re-uses the LDS windows (see finish_grad_args)
    bool sums = false;             // also accumulate sum_p I[p] B[p] (RefArgs::musum) into d_musum[mu_buf]; never deterministic, never without events
    float band_b0 = 0.f, band_b1 = 0.f;  // ... b(0) and b(1) of B's border_weight
    // 2-DoF objectives: K1 clears the raw sums its K3 adds into -- through its statistics slot when the objective keeps none
    // (deferred: raw_reset), through RefArgs::raw_zero otherwise (raw_lines)
    double *raw_reset = nullptr, *raw_lines = nullptr;
    float4 *grad_zero = nullptr;   // flow-gradient buffer to clear (RefArgs::grad_zero), or null
    int64_t n_grad_zero4 = 0;
};

// raw votes of n_ref reference times (one launch) into imgs[k] (cleared here unless bit k of zero_mask says it is
// zero already); stat_slot0 >= 0: the statistics accumulators of slots stat_slot0 + k are reset by the launch
static int vote_images(cmax_handle_s *h, int model, const float *motion, int T, int n_ref, const int *ref_mode, const double *ref_frac,
                       int normalize, float *const *imgs, unsigned zero_mask, int stat_slot0, hipStream_t s, const VoteJobs &jobs = {},
                       int motion_f64 = 0) {
    const int64_t npix = (int64_t)h->Hp * h->Wp;
    RefArgs ra = {};
    ra.raw_zero = jobs.raw_lines;
    ra.grad_zero = jobs.grad_zero;
    ra.n_grad_zero4 = jobs.n_grad_zero4;
    fill_ref_times(ra, n_ref, ref_mode, ref_frac);
    if (jobs.publish_windows && h->n > 0) {
        ra.win = h->d_win;
        ra.shifts = h->d_shifts;
        h->win_motion = motion;
        h->win_model = model;
        h->win_nref = n_ref;
        h->win_T = T;
        h->win_normalize = normalize;
        for (int k = 0; k < n_ref; ++k) h->win_d[k] = ra.d[k];
        h->win_generation = h->generation;
    }
    const bool det = h->deterministic && h->n > 0;  // votes go to the integer images, imgs[k] are written by the conversion below
    for (int k = 0; k < n_ref; ++k) {
        if (!det && !((zero_mask >> k) & 1u)) CMAX_CHECK_HIP(hipMemsetAsync(imgs[k], 0, npix * sizeof(float), s));
        if (det) ra.img64[k] = h->img64 + (int64_t)k * npix;
        // accumulators K1's first workgroup resets: the statistics of slot stat_slot0 + k, or (deferred 2-DoF objective: no
        // statistics kernel runs) the raw sums K3 of the same evaluation adds into
        double *stat_zero = jobs.raw_reset ? jobs.raw_reset + (int64_t)k * kRawStride : (stat_slot0 >= 0 ? h->d_stat + (stat_slot0 + k) * kStatStride : nullptr);
        if (h->n == 0 && stat_zero)  // no K1 launch on this rank: reset the accumulators explicitly
            CMAX_CHECK_HIP(hipMemsetAsync(stat_zero, 0, kStatStride * sizeof(double), s));
        ra.img[k] = imgs[k];
        ra.stat[k] = stat_zero;
        if (jobs.sums) ra.musum[k] = h->d_musum + ((int64_t)h->mu_buf * 4 + k) * kMuStride;
    }
    ra.band_b0 = jobs.band_b0;
    ra.band_b1 = jobs.band_b1;
    if (h->n == 0) return 0;
    const EvView ev = ev_view(h);
    const WarpParams wp = warp_params(h, motion, T, ref_mode[0], ref_frac[0], normalize, motion_f64);
    if (model < 0) launch_vote<-1>(h, ev, wp, ra, n_ref, s);  // the un-warped image
    else with_model(model, [&](auto m) { launch_vote<m.value>(h, ev, wp, ra, n_ref, s); });
    CMAX_CHECK_LAUNCH();
    if (det) {  // exact integer sums -> fp32 images, one rounding each; the integer images are zero again afterwards
        FixedArgs fa = {};
        fa.inv_fix = (h->big || h->mid) ? 1.0 / 524288.0 : 1.0 / 1048576.0;
        for (int k = 0; k < n_ref; ++k) {
            fa.src[k] = ra.img64[k];
            fa.dst[k] = imgs[k];
        }
        hipLaunchKernelGGL(k_fixed_to_image, dim3(stream_grid(npix, 256), n_ref), dim3(256), 0, s, fa, npix);
        CMAX_CHECK_LAUNCH();
    }
    return 0;
}

// one reference time
static int vote_image(cmax_handle_s *h, int model, const float *motion, int T, int ref_mode, double frac, int normalize,
                      float *raw, bool already_zero, int stat_slot, hipStream_t s) {
    float *imgs[1] = {raw};
    return vote_images(h, model, motion, T, 1, &ref_mode, &frac, normalize, imgs, already_zero ? 1u : 0u, stat_slot, s);
}

// the image the contrast is evaluated on: `raw`, or its blurred copy in `blur` when sigma > 0
static int blur_image(cmax_handle_s *h, double sigma, const float *raw, float *blur, const float **out, hipStream_t s) {
    *out = raw;
    if (sigma > 0) {
        const int64_t npix = (int64_t)h->Hp * h->Wp;
        double k0, k1;
        blur_taps(sigma, k0, k1);
        hipLaunchKernelGGL(k_blur3<float>, dim3(div_up(npix, 256)), dim3(256), 0, s, raw, h->Hp, h->Wp, (float)k0, (float)k1, blur);
        CMAX_CHECK_LAUNCH();
        *out = blur;
    }
    return 0;
}

static int stat_blocks(const cmax_handle_s *h) {
    // deterministic mode: one workgroup per sub-accumulator, so every accumulator receives exactly one addition
    if (h->deterministic) return kStatSub;
    // ~4 pixels per thread, at most kStatBlocksMax workgroups
    int64_t b = ((int64_t)h->Hp * h->Wp + 1023) / 1024;
    if (b < 1) b = 1;
    if (b > kStatBlocksMax) b = kStatBlocksMax;
    return (int)b;
}

// statistics of `img` -> stat[slot] (accumulators zeroed by the K1 launch); optionally zero `zero_img`
static int stat_subs(const cmax_handle_s *h) {
    if (h->deterministic) return kStatSub;
    // one 128-byte line per sub-accumulator (same-line atomics serialise).  Their readers are ONE wave per K3 workgroup (and
    // only for a normalised cost) and the wave that writes the loss, each with one load per lane -- when every wave of K3
    // gathered them at its head, more than 8 lines cost K3 more than they saved K2 (cfg3 K3 18.7 -> 21.1 us with 25 lines).
    // 16 lines: cfg3's image kernel (1200 workgroups) 6.0 -> 5.65 us, cfg4's (363) 6.5 -> 5.95.
    int n = stat_blocks(h) / 6;
    static const int forced = getenv("CMAX_NSUB") ? atoi(getenv("CMAX_NSUB")) : 0;  // tuning only
    if (forced > 0) return forced < kStatSub ? forced : kStatSub;
    return n < 4 ? 4 : (n > 16 ? 16 : n);
}

// zero_extra: optional buffer of n_extra floats (16-byte aligned, n_extra % 4 == 0) cleared by the same launch
static int launch_stats(cmax_handle_s *h, int cost, const float *img, int omit, int slot, float *zero_img, hipStream_t s,
                        float *zero_extra = nullptr, int64_t n_extra = 0) {
    const int grid = stat_blocks(h);
    const int nsub = stat_subs(h);
    double *stat_slot = h->d_stat + slot * kStatStride;
    ProfScope prof(h, kProfStats, s);
    for (int rep = 0; rep < h->prof_repeat; ++rep) {
        with_cost(cost, [&](auto c) {
            if (h->deterministic)  // kStatSub workgroups of 1024 threads: every accumulator is written once, the summation order is fixed
                hipLaunchKernelGGL((k_stats<c.value, 1024>), dim3(grid), dim3(1024), 0, s, img, h->Hp, h->Wp, omit, nsub, stat_slot, zero_img, (float4 *)zero_extra, n_extra / 4);
            else
                hipLaunchKernelGGL(k_stats<c.value>, dim3(grid), dim3(256), 0, s, img, h->Hp, h->Wp, omit, nsub, stat_slot, zero_img, (float4 *)zero_extra, n_extra / 4);
        });
    }
    CMAX_CHECK_LAUNCH();
    return 0;
}

bool handle_is_deterministic(cmax_handle_t h) { return h && h->deterministic; }

void handle_get_eval_state(cmax_handle_t h, HandleEvalState *out) {
    out->cur_buf = h->cur_buf;
    out->zero_mask[0] = h->zero_mask[0];
    out->zero_mask[1] = h->zero_mask[1];
    out->orig_valid = h->orig_valid ? 1 : 0;
    out->orig_cost = h->orig_cost;
    out->orig_omit = h->orig_omit;
    out->orig_sigma = h->orig_sigma;
    for (int k = 0; k < 4; ++k) out->last_iwe[k] = h->last_iwe[k];
    out->generation = h->generation;
    out->profiling = h->profiling ? 1 : 0;
    out->deterministic = h->deterministic ? 1 : 0;
    out->mu_buf = h->mu_buf;
}

uint64_t handle_state_key(const HandleEvalState &st, int kind) {
    uint64_t sb;
    std::memcpy(&sb, &st.orig_sigma, sizeof(sb));
    uint64_t k = (uint64_t)kind;
    k = k * 1000003u + (uint64_t)st.cur_buf;
    k = k * 1000003u + st.zero_mask[0];
    k = k * 1000003u + st.zero_mask[1];
    k = k * 1000003u + (uint64_t)st.orig_valid;
    k = k * 1000003u + (uint64_t)st.deterministic;
    k = k * 1000003u + (uint64_t)st.mu_buf;
    k = k * 1000003u + (uint64_t)(st.orig_cost + 7);
    k = k * 1000003u + (uint64_t)(st.orig_omit + 7);
    k = k * 1000003u + sb;
    return k;
}

void handle_set_eval_state(cmax_handle_t h, const HandleEvalState *in) {
    h->cur_buf = in->cur_buf;
    h->zero_mask[0] = in->zero_mask[0];
    h->zero_mask[1] = in->zero_mask[1];
    h->orig_valid = in->orig_valid != 0;
    h->orig_cost = in->orig_cost;
    h->orig_omit = in->orig_omit;
    h->orig_sigma = in->orig_sigma;
    for (int k = 0; k < 4; ++k) h->last_iwe[k] = in->last_iwe[k];
    h->mu_buf = in->mu_buf;
}

}  // namespace cmax

using namespace cmax;

extern "C" {

int cmax_iwe(cmax_handle_t h, int model, const float *motion, int T, int ref_mode, double ref_frac, int normalize_t,
             double sigma, float *iwe_out, cmax_stream_t stream) {
    CMAX_REQUIRE(h != nullptr && iwe_out != nullptr, "iwe: handle / output");
    CMAX_REQUIRE(model < 0 || motion != nullptr, "iwe: motion");
    CMAX_REQUIRE(model <= CMAX_MODEL_VOXEL, "iwe: model");
    CMAX_REQUIRE(model != CMAX_MODEL_VOXEL || (T > 0 && T == h->n_time_bin), "iwe: voxel T must match the handle's time bins");
    CMAX_REQUIRE(model != CMAX_MODEL_VOXEL || !h->slab_major, "iwe: a voxel motion needs time BINS (cmax_set_time_bins), this handle is in slab order");
    CMAX_REQUIRE(model <= CMAX_MODEL_2DOF || h->n_outside == 0, "iwe: the batch holds events off the sensor (cmax_set_keep_outside): 2-DoF / un-warped only");
    hipStream_t s = (hipStream_t)stream;
    float *raw = sigma > 0 ? h->G : iwe_out;  // G is scratch outside cmax_objective
    int rc = vote_image(h, model, motion, T, ref_mode, ref_frac, normalize_t, raw, false, -1, s);
    if (rc) return rc;
    const float *img = nullptr;
    return blur_image(h, sigma, raw, iwe_out, &img, s);
}

// the objective descriptor as the kernels see it
static ObjParams obj_params(const cmax_handle_s *h, const cmax_objective_t *d) {
    ObjParams op;
    op.cost = d->cost;
    op.normalized = d->normalized;
    op.minimize = d->minimize;
    op.negate = d->negate;
    op.omit = d->omit_boundary;
    op.n_ref = d->n_ref;
    for (int k = 0; k < 4; ++k) op.mult[k] = d->mult[k];
    op.H = h->Hp;
    op.W = h->Wp;
    op.nsub = stat_subs(h);
    return op;
}

static int check_objective_args(cmax_handle_t h, const cmax_objective_t *d, const float *motion) {
    CMAX_REQUIRE(h && d && motion, "objective: null pointer");
    CMAX_REQUIRE(d->model >= CMAX_MODEL_2DOF && d->model <= CMAX_MODEL_VOXEL, "objective: model");
    CMAX_REQUIRE(cost_known(d->cost), "objective: cost");
    CMAX_REQUIRE(d->n_ref >= 1 && d->n_ref <= 4, "objective: n_ref");
    CMAX_REQUIRE(d->motion_dtype == CMAX_F32 || d->motion_dtype == CMAX_F64, "objective: motion_dtype must be CMAX_F32 or CMAX_F64");
    CMAX_REQUIRE(d->model != CMAX_MODEL_VOXEL || (d->T > 0 && d->T == h->n_time_bin), "objective: voxel T must match the handle's time bins");
    CMAX_REQUIRE(d->model != CMAX_MODEL_VOXEL || !h->slab_major, "objective: a voxel motion needs time BINS (cmax_set_time_bins), this handle is in slab order");
    CMAX_REQUIRE(d->model == CMAX_MODEL_2DOF || h->n_outside == 0,
                 "objective: the batch holds events off the sensor: only the 2-DoF model is defined for them -- a flow has no value there (cmax_set_keep_outside(h, 0) before cmax_set_events drops them)");
    CMAX_REQUIRE(!d->omit_boundary || (h->Hp > 2 && h->Wp > 2), "objective: image too small for omit_boundary");
    CMAX_REQUIRE((int64_t)(d->model == CMAX_MODEL_VOXEL ? d->T : 1) * 2 * h->H * h->W * 4 < ((int64_t)1 << 32),
                 "objective: the motion field must be smaller than 4 GiB (32-bit byte offsets in the event kernels)");
    return 0;
}

static bool orig_cache_hit(const cmax_handle_s *h, const cmax_objective_t *d) {
    return h->orig_valid && h->orig_sigma == d->sigma && h->orig_cost == d->cost && h->orig_omit == d->omit_boundary;
}

// K1 without its votes: the LDS windows and the fp64 cell decisions (RefArgs::win / shifts) of this warp, for a K3 that follows
static int publish_windows(cmax_handle_s *h, const cmax_objective_t *d, const float *motion, hipStream_t s) {
    RefArgs ra = {};
    ra.win = h->d_win;
    ra.shifts = h->d_shifts;
    ra.windows_only = 1;
    fill_ref_times(ra, d->n_ref, d->ref_mode, d->ref_frac);
    const EvView ev = ev_view(h);
    const WarpParams wp = warp_params(h, motion, d->T, d->ref_mode[0], d->ref_frac[0], d->normalize_t, d->motion_dtype == CMAX_F64);
    with_model(d->model, [&](auto m) { launch_vote<m.value>(h, ev, wp, ra, d->n_ref, s); });
    CMAX_CHECK_LAUNCH();
    h->win_motion = nullptr;  // (nobody may take these windows for those of a vote)
    return 0;
}

// 2-DoF + plain variance with a gradient: K3 gathers the image statistics itself and k_finish_raw applies
// the chain factors -- no K2 launch (unless a workgroup's slice of the image would get long)
static bool deferred_applies(const cmax_handle_s *h, const cmax_objective_t *d, const void *grad) {
    // (a weighted handle takes the general K1 -> statistics -> K3 path: the raw sums' indicator image and sum I are not carried)
    return !h->deterministic && !h->weighted && !h->general_only && grad && d->model == CMAX_MODEL_2DOF && d->cost == CMAX_COST_VARIANCE && !(d->sigma > 0) && h->n > 0 &&
           (int64_t)h->Hp * h->Wp <= (int64_t)h->nseg * 8192;
}

// every 2-DoF objective of the default mode leaves its gradient as sums in kRawLines lines (deferred: six sums, loss included)
static bool two_dof_lines(const cmax_handle_s *h, const cmax_objective_t *d, const void *grad) {
    return !h->deterministic && grad && d->model == CMAX_MODEL_2DOF && h->n > 0;
}

// the motion gradient of an objective: elements, bytes, element type of its exchange
struct GradExtent {
    int64_t count;
    size_t bytes;
    CommType type;
};
static GradExtent grad_extent(const cmax_handle_s *h, const cmax_objective_t *d) {
    if (d->model == CMAX_MODEL_2DOF) return {2, 2 * sizeof(double), kCommF64};
    const int64_t count = (int64_t)(d->model == CMAX_MODEL_VOXEL ? d->T : 1) * 2 * h->H * h->W;
    return {count, (size_t)count * sizeof(float), kCommF32};
}

// The motion as the kernels read it (behind check_objective_args).  fp32, or the 2-DoF model's double theta[2]: the caller's pointer.
// An fp64 flow / voxel: the high plane of its split in the handle's scratch, the low plane behind it (k_split_motion) -- one launch
// on the caller's stream in front of the evaluation; everything but K1's fp64 cell decisions then runs what an fp32 call on
// (float)flow runs.  The scratch grows on first use (with a synchronisation: not inside a stream capture).
static int kernel_motion(cmax_handle_s *h, const cmax_objective_t *d, const void *motion_v, hipStream_t s, const float **motion) {
    *motion = static_cast<const float *>(motion_v);
    if (d->motion_dtype != CMAX_F64 || d->model == CMAX_MODEL_2DOF) return 0;
    const int64_t count = grad_extent(h, d).count;
    if (2 * count > h->m64.capacity() && h->win_motion == h->m64) h->win_motion = nullptr;  // (windows of a vote on planes that go away)
    int rc = h->m64.reserve(&h->bytes, 2 * count, s);
    if (rc) return rc;
    const int vec = (count % 4 == 0 && (reinterpret_cast<uintptr_t>(motion_v) & 15u) == 0) ? 1 : 0;
    const int64_t items = vec ? count / 4 : count;
    hipLaunchKernelGGL(k_split_motion, dim3(stream_grid(items, 256)), dim3(256), 0, s, static_cast<const double *>(motion_v), count, vec, h->m64);
    CMAX_CHECK_LAUNCH();
    h->m64_src = motion_v;
    *motion = h->m64;
    return 0;
}

// C2 in row bands (cmax_comm_set_c2_bands).  WHETHER the gradient is exchanged in bands, and in which, must not depend on anything a
// rank knows about its own slice (a rank without events, or whose work list is not group-aligned, issued ONE all-reduce
// while its peers issued `bands` grouped ones -- different collective sequences, i.e. a hang): the bands follow from the sensor's tile
// rows and the setting alone, every rank issues the same `bands` grouped all-reduces on its second stream, and only HOW its K3 runs
// in front of them is local -- band by band where the work list allows it (overlap), in one launch or not at all otherwise (eval_plan: bands).
static int c2_prepare_bands(cmax_handle_s *h, int bands) {
    if (!h->comm_stream) CMAX_CHECK_HIP(hipStreamCreateWithFlags(&h->comm_stream, hipStreamNonBlocking));
    while ((int)h->band_ev.size() < bands + 1) {
        hipEvent_t e = nullptr;
        CMAX_CHECK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        h->band_ev.push_back(e);
    }
    return 0;
}
// RANK-CONSISTENT SCALARS (round 6).  After C1 every rank evaluates the contrast on the same reduced image, but with
// fp64 atomics in its own order: result[8] (loss and statistics) agrees across ranks to ~1e-16 relative, not bit for bit -- and every
// rank runs its own copy of the optimiser (src/solver/scipy_autograd/scipy_minimize.py:100-117), where ONE differing Wolfe / Armijo
// comparison means different call sequences, mismatched collectives, a hang.  The gradient is identical by construction (it is
// all-reduced); the scalars are made so by the same exchange: every rank but 0 zeroes its result[8] behind its last writer and the
// eight doubles ride in the gradient's (grouped) all-reduce -- x + 0 + ... + 0 is exact, so all ranks leave with rank 0's bits.  A
// value-only evaluation gets the 64-byte exchange on its own.  A 1-rank communicator runs the same sequence.
static int result_zero_unless_rank0(cmax::Comm *comm, double *result, hipStream_t s) {
    if (comm && result && comm_rank(comm) != 0) CMAX_CHECK_HIP(hipMemsetAsync(result, 0, 8 * sizeof(double), s));
    return 0;
}
static int result_exchange_alone(cmax::Comm *comm, double *result, hipStream_t s) {
    int rc = result_zero_unless_rank0(comm, result, s);
    return rc ? rc : comm_allreduce(comm, result, 8, kCommF64, kCommSum, s);
}
// the gradient's all-reduce with result[8] riding along (one grouped RCCL call)
static int grad_and_result_exchange(cmax::Comm *comm, void *grad, size_t gcount, CommType gtype, double *result, hipStream_t s) {
    int rc = result_zero_unless_rank0(comm, result, s);
    if (rc) return rc;
    void *bufs[2] = {grad, result};
    const size_t counts[2] = {gcount, 8};
    const CommType types[2] = {gtype, kCommF64};
    return comm_allreduce_group(comm, bufs, counts, types, result ? 2 : 1, kCommSum, s);
}

// band b's rows of both channels, all-reduced on the second stream once `s` has passed this point (band 0 carries result[8], see above)
static int c2_exchange_band(cmax_handle_s *h, cmax::Comm *c2_comm, float *grad, int b, int bands, hipStream_t s, double *result = nullptr) {
    const int tr0 = (int)((int64_t)h->ntr * b / bands), tr1 = (int)((int64_t)h->ntr * (b + 1) / bands);
    const int64_t hw = (int64_t)h->H * h->W;
    if (b == 0 && result) {
        int rc = result_zero_unless_rank0(c2_comm, result, s);
        if (rc) return rc;
    }
    CMAX_CHECK_HIP(hipEventRecord(h->band_ev[b], s));
    CMAX_CHECK_HIP(hipStreamWaitEvent(h->comm_stream, h->band_ev[b], 0));
    const int r0 = tr0 * kTile, r1 = std::min(tr1 * kTile, h->H);
    void *bufs[3] = {grad + (int64_t)r0 * h->W, grad + hw + (int64_t)r0 * h->W, result};
    const size_t counts[3] = {(size_t)(r1 - r0) * h->W, (size_t)(r1 - r0) * h->W, 8};
    const CommType types[3] = {kCommF32, kCommF32, kCommF64};
    return comm_allreduce_group(c2_comm, bufs, counts, types, (b == 0 && result) ? 3 : 2, kCommSum, h->comm_stream);
}
// the reduced gradient back to the caller's stream
static int c2_join_bands(cmax_handle_s *h, int bands, hipStream_t s) {
    CMAX_CHECK_HIP(hipEventRecord(h->band_ev[bands], h->comm_stream));
    CMAX_CHECK_HIP(hipStreamWaitEvent(s, h->band_ev[bands], 0));
    return 0;
}
// every band behind a gradient that is already complete on this rank
static int c2_exchange_all_bands(cmax_handle_s *h, cmax::Comm *c2_comm, float *grad, int bands, hipStream_t s, double *result) {
    int rc = c2_prepare_bands(h, bands);
    for (int b = 0; b < bands && !rc; ++b) rc = c2_exchange_band(h, c2_comm, grad, b, bands, s, result);
    return rc ? rc : c2_join_bands(h, bands, s);
}

// 2-DoF, plain variance: K1T (image + two tangent images) -> [ONE all-reduce] -> k_tan_stats_var -> k_finish_deferred.
// No pass over the events for the gradient, and across GPUs no second exchange: after the all-reduce every rank holds
// the whole batch's three images and finishes loss and gradient on its own.
// force: CMAX_TAN2 (1 = also on one GPU, 0 = never, -1 = unset)
static bool tan2_applicable(const cmax_handle_s *h, const cmax_objective_t *d, const void *grad, bool dist, int force) {
    if (force == 0 || h->deterministic || h->weighted || h->general_only || !grad) return false;
    if (d->model != CMAX_MODEL_2DOF || d->cost != CMAX_COST_VARIANCE || d->sigma > 0) return false;
    // Rank-consistent scalars: behind the single exchange every rank finishes loss AND gradient on its own -- from the reduced planes in a
    // fixed order (per-workgroup partials, one folding wave: bit-identical on every rank), but a NORMALISED variance also reads the
    // un-warped image's cached statistics, which each rank summed with atomics in its own order.  Across real ranks that objective
    // takes the two-exchange path, whose gradient is all-reduced and whose scalars ride along.
    if (d->normalized && h->comm && comm_nranks(h->comm) > 1) return false;
    if (d->normalized && !orig_cache_hit(h, d)) return false;  // the first evaluation of a batch builds the un-warped image's statistics on the standard path
    return dist || force == 1;
}

// How one evaluation runs: every path decision, taken ONCE by eval_plan before anything is enqueued.  objective_eval, objective_vote /
// vote_images and objective_finish read the plan; none of them derives a decision again.
struct EvalPlan {
    // ---- the form of the call
    // whole: K1 of this very call voted the images (objective_eval), so `motion` still holds the values of the vote that published
    // h->d_win and K3 re-uses the windows.  The stand-alone cmax_objective_finish cannot know -- a caching allocator hands the same
    // address to a different motion -- and lets K3 derive its windows again; every decision that needs a job done by K1 is false for it.
    bool whole;
    bool tan2;                // the tangent-image path instead (objective_eval_tan2): nothing below applies
    bool empty;               // empty batch and no communicator: loss 0, zero gradient, no launch
    cmax::Comm *c2_comm;      // the gradient (result[8] riding along) is all-reduced: in `bands` row bands by objective_finish, in one call behind it when bands == 1
    bool result_alone;        // value-only evaluation under a communicator: result[8] is exchanged on its own
    double *raw;              // lines: the accumulators of the 2-DoF K3 -- the caller's (cmax_objective_raw) or the handle's own
    bool raw_only;            // stop at those sums: the caller folds them itself (cmax_objective_raw), no finishing launch
    volatile unsigned long long *host_flag;  // cmax_objective_host: `result` and `grad` are pinned host memory, the finishing kernel writes the
    unsigned long long host_seq;             // run counter behind them
    GradExtent g;
    const DescentArgs *step;  // cmax_objective_descend on the deferred path: the finishing launch is k_finish_raw_step, which also applies this step
    // ---- the path
    bool deferred;  // deferred_applies: no K2, K3 gathers the statistics, k_finish_raw applies the chain factors
    bool lines;     // two_dof_lines (includes the deferred case)
    bool fused_gm;  // gradient magnitude with a gradient: K2 and K2b (and the blurs) are one kernel: statistics + G image without its chain factor
    bool fused_st;  // a focus loss with a gradient: [k_blur3 ->] k_stats_gimage_st (statistics + G image, chain factor as for fused_gm) [-> k_blur3_adj]
    bool plain_st;  // ... with CMAX_NO_FUSED_FOCUS=1: k_stats in front, k_gimage with the full chain factor behind it (kFoldNone)
    bool blur_var;  // blurred variance: blur + statistics in one kernel
    bool fused_bv;  // ... with a gradient on one GPU: K1 also sums the votes against blur^T 1_Omega, so that ONE image kernel can blur, sum and
                    // write the un-centred, unscaled A' = 2 / (n - 1) blur^T [Ib 1_Omega] (k_blur_stats_adj_var); K3 applies the chain factor
                    // (kFoldScale) and, along the image border, the mean.  Across GPUs the sum would need its own exchange: two image kernels.
    bool owned;     // owned groups: K3 stores every element of the flow gradient itself -- nothing to clear
    bool stats_inside;  // plain variance, not normalised, K1 of this call summed its votes: the statistics run inside the K3 launch (kFoldStatsInside)
    int stat_blocks;    // ... in this many leading workgroups (RefArgs::stat_blocks)
    int fold;           // kFold* of K3
    // who clears the flow gradient K3 adds into (no one on owned groups): K1 (vote.grad_zero), the statistics / fused image kernel, or a memset
    float4 *stats_clear4;
    int64_t n_stats_clear4;
    bool memset_grad;
    float tap0, tap1;   // blur taps (sigma > 0)
    int bands;          // row bands the gradient is exchanged in: the same on every rank
    bool k3_in_bands;   // ... and this rank's work list allows K3 band by band, each band's rows exchanged behind it
    VoteJobs vote;      // what K1 does for the launches behind it
};

// The form of an evaluation as its entry asks for it; an entry names the fields it sets, eval_plan alone reads them.
struct EvalForm {
    cmax::Comm *comm = nullptr;  // time-sliced batch: the images are all-reduced, and (not skip_c2) the gradient or result[8] behind them
    bool skip_c2 = false;        // ... the gradient stays this rank's share (objective_dist_local_grad)
    double *raw_out = nullptr;   // stop at the raw sums of the 2-DoF K3, written here (cmax_objective_raw; `grad` is then only a non-null marker)
    volatile unsigned long long *host_flag = nullptr;  // `result` and `grad` are pinned host memory: the finishing kernel writes the run
    unsigned long long host_seq = 0;                   // counter host_seq behind them (cmax_objective_host)
    const DescentArgs *step = nullptr;  // a descent's step, to ride on the finishing launch where the path has one that can apply it
    bool *stepped = nullptr;            // ... out: it does (otherwise the caller launches the step behind the evaluation)
};

static EvalPlan eval_plan(const cmax_handle_s *h, const cmax_objective_t *d, const void *grad, bool whole, const EvalForm &form = {}) {
    cmax::Comm *const comm = form.comm;
    const bool skip_c2 = form.skip_c2;
    double *const raw_out = form.raw_out;
    volatile unsigned long long *const host_flag = form.host_flag;
    static const int tan2_env = getenv("CMAX_TAN2") ? atoi(getenv("CMAX_TAN2")) : -1;
    static const bool no_fused_bv = getenv("CMAX_NO_FUSED_BLURVAR") != nullptr;
    static const bool no_stats_inside = getenv("CMAX_NO_STATS_INSIDE") != nullptr;
    static const bool no_fused_focus = getenv("CMAX_NO_FUSED_FOCUS") != nullptr;
    static const int sweeps_env = getenv("CMAX_STAT_SWEEPS") ? std::max(1, atoi(getenv("CMAX_STAT_SWEEPS"))) : 0;
    EvalPlan p = {};
    const bool dist = comm != nullptr;  // also a 1-rank communicator: the same enqueue sequence, RCCL included
    const int64_t npix = (int64_t)h->Hp * h->Wp;
    p.whole = whole;
    // (never with a host flag: the tangent-image path ends in kernels that know nothing of it -- ADVICE r3)
    p.tan2 = whole && !raw_out && !host_flag && !skip_c2 && (h->n > 0 || dist) && tan2_applicable(h, d, grad, dist, tan2_env);
    // empty batch: loss 0, zero gradient (patch_contrast_base.py:253-255).  A time slice may be empty while the batch is not.
    p.empty = whole && h->n == 0 && !dist;
    p.c2_comm = (dist && grad && !raw_out && !skip_c2) ? comm : nullptr;
    p.result_alone = dist && !grad && !raw_out && !skip_c2;
    p.raw_only = raw_out != nullptr;
    p.host_flag = host_flag;
    p.host_seq = form.host_seq;
    p.g = grad_extent(h, d);
    const bool det = h->deterministic, two_dof = d->model == CMAX_MODEL_2DOF;
    const bool fold_var = d->cost == CMAX_COST_VARIANCE && !(d->sigma > 0);
    // (the deferred K3 takes sum I and sum I^2 from its own events' gather: the image must be what THIS handle's events voted in this
    // call -- an image the caller hands to cmax_objective_finish, or one that was all-reduced, keeps its statistics launch)
    p.deferred = deferred_applies(h, d, grad) && whole && !dist;
    // (a descent's step rides on the deferred path's finishing launch; on every other path the caller launches it behind the evaluation)
    p.step = (p.deferred && !p.tan2 && !p.empty) ? form.step : nullptr;
    if (form.stepped) *form.stepped = p.step != nullptr;
    p.lines = two_dof_lines(h, d, grad);
    p.raw = p.lines ? (raw_out ? raw_out : h->d_raw) : nullptr;
    p.fused_gm = !det && grad && d->cost == CMAX_COST_GRADMAG && h->n > 0;
    p.fused_st = !det && grad && cost_is_focus(d->cost) && h->n > 0 && !no_fused_focus;
    p.plain_st = !det && grad && cost_is_focus(d->cost) && h->n > 0 && no_fused_focus;
    p.blur_var = !det && d->cost == CMAX_COST_VARIANCE && d->sigma > 0;
    // K1 can sum its votes for the kernels behind it (not on a weighted handle: the sum counts events)
    const bool k1_sums_ok = whole && !dist && !h->weighted && !h->general_only && h->Hp >= 4 && h->Wp >= 4;
    p.fused_bv = k1_sums_ok && p.blur_var && grad && h->n > 0 && !no_fused_bv;
    // K3 stores every element of the flow gradient itself (one writer per pixel): needs the group-aligned work list, ONE reference
    // time (several would add into the same pixels) and the sort order that matches the model (dense: tiles; voxel: (tile, bin) of
    // the same T)
    p.owned = !det && grad && h->owned && h->n > 0 && d->n_ref == 1 &&
              ((d->model == CMAX_MODEL_DENSE && h->n_time_bin == 0) || (d->model == CMAX_MODEL_VOXEL && h->n_time_bin == d->T));
    // plain variance (no blur, not normalised) on owned groups: nothing in the gradient needs the finished statistics once the
    // mean comes from the votes, so K2 runs inside the K3 launch (kFoldStatsInside)
    // ... and on work lists that are not group-aligned (K3 adds its gradient with atomics) once K1 clears the gradient buffer -- the
    // other job of the separate statistics launch (round 4: 20M events 88.5 -> see profiles/r04_ablation.txt 16)
    const bool inside_ok = k1_sums_ok && !no_stats_inside && fold_var && !d->normalized;
    // a launch in front of K3 can clear the flow gradient with its 16-byte stores
    const bool clearable = grad && !two_dof && !p.owned && !det && h->n > 0 && p.g.count % 4 == 0 && ((uintptr_t)grad & 15u) == 0;
    const bool cleared_by_vote = inside_ok && clearable && d->n_ref == 1;
    p.stats_inside = inside_ok && (p.owned || cleared_by_vote);
    if (clearable && !cleared_by_vote) {
        p.stats_clear4 = (float4 *)grad;
        p.n_stats_clear4 = p.g.count / 4;
    }
    p.memset_grad = grad && !two_dof && !p.owned && !det && !clearable;
    p.fold = p.deferred ? kFoldDeferred
                        : (p.stats_inside ? kFoldStatsInside
                                          : (fold_var ? kFoldStats : (((p.fused_gm || p.fused_st || p.fused_bv) && d->normalized) ? kFoldScale : kFoldNone)));
    if (p.stats_inside) {
        // Sweeps of 4 pixels per thread and statistics workgroup: two (round 3, standard segments: K3 of cfg5 with 1 / 2 / 4 / 8 sweeps 18.8 /
        // 17.9 / 18.3 / 18.3 us) -- unless the gathering workgroups fit the chip in ONE round and the statistics workgroups are what
        // spills into a second: then four, if that makes the launch fit (round 4, mid segments: cfg5's shard is 900 gathering workgroups;
        // with 232 statistics workgroups 1132 > 1024 resident, with 120 it fits -- K3 16.1 -> 14.8 us, the evaluation 28.8 -> 27.4 us;
        // 3 / 4 / 6 / 8 / 16 sweeps: 28.8 / 27.4 / 27.6 / 27.8 / 31.3 us, profiles/r04_ablation.txt 15).  CMAX_STAT_SWEEPS overrides.
        // (h->owned, as before: the launch's grad_layout takes this call's `owned`, which can be false where h->owned is not)
        const int gthreads = layout_threads(grad_layout(h, d->model, h->owned));
        auto blocks_for = [&](int sweeps) {
            const int64_t per_block = 4 * (int64_t)gthreads * sweeps;
            return (int)std::min<int64_t>(8 * div_up(div_up(npix, per_block), 8), 8 * (kStatBlocksMax / 8));
        };
        int sweeps = sweeps_env ? sweeps_env : 2;
        if (!sweeps_env) {
            const int resident = 256 * (2048 / gthreads), gather = 8 * div_up(h->nseg, 8) * d->n_ref;  // workgroups the chip holds at once
            if (gather <= resident && gather + blocks_for(2) * d->n_ref > resident && gather + blocks_for(4) * d->n_ref <= resident) sweeps = 4;
        }
        p.stat_blocks = blocks_for(sweeps);
    }
    double k0 = 0, k1 = 0;
    if (d->sigma > 0) blur_taps(d->sigma, k0, k1);
    p.tap0 = (float)k0;
    p.tap1 = (float)k1;
    p.bands = (p.c2_comm && d->model == CMAX_MODEL_DENSE && h->c2_bands > 1) ? std::min(h->c2_bands, h->ntr) : 1;  // (the same on every rank, see c2_prepare_bands)
    p.k3_in_bands = p.bands > 1 && p.owned && (int)h->row_seg_start.size() == h->ntr + 1;
    if (!whole) return p;  // (no K1 in this call)
    p.vote.publish_windows = true;
    p.vote.sums = p.fused_bv || p.stats_inside;
    if (p.vote.sums) {  // B = blur^T 1_Omega = b(r) b(c); no blur: B = 1_Omega
        const float b0 = d->sigma > 0 ? p.tap0 : 1.f, b1 = d->sigma > 0 ? p.tap1 : 0.f;
        p.vote.band_b0 = border_weight(0, h->Hp, d->omit_boundary ? 1 : 0, b0, b1);
        p.vote.band_b1 = border_weight(1, h->Hp, d->omit_boundary ? 1 : 0, b0, b1);
    }
    if (p.deferred) p.vote.raw_reset = p.raw;
    else p.vote.raw_lines = p.raw;
    if (cleared_by_vote) {
        p.vote.grad_zero = (float4 *)grad;
        p.vote.n_grad_zero4 = p.g.count / 4;
    }
    return p;
}

// votes of every reference time (+ the un-warped image when needed) into images[0 .. n_images);
// zero_mask bit k: images[k] is already zero (the handle's double-buffered images)
static int objective_vote(cmax_handle_t h, const cmax_objective_t *d, const float *motion, float *images, unsigned zero_mask, int *n_images_out, hipStream_t s, const VoteJobs &jobs) {
    const int64_t npix = (int64_t)h->Hp * h->Wp;
    float *imgs[4];
    for (int k = 0; k < d->n_ref; ++k) imgs[k] = images + k * npix;
    int rc = vote_images(h, d->model, motion, d->T, d->n_ref, d->ref_mode, d->ref_frac, d->normalize_t, imgs, zero_mask, 0, s, jobs, d->motion_dtype == CMAX_F64);
    if (rc) return rc;
    int n_images = d->n_ref;
    if (d->normalized && !orig_cache_hit(h, d)) {  // un-warped image, once per batch (patch_contrast_base.py:295-301)
        rc = vote_image(h, -1, nullptr, 0, CMAX_REF_FIRST, 0.0, 1, images + (int64_t)d->n_ref * npix, (zero_mask >> d->n_ref) & 1u, 4, s);
        if (rc) return rc;
        ++n_images;
    }
    *n_images_out = n_images;
    return 0;
}

int cmax_objective_vote(cmax_handle_t h, const cmax_objective_t *d, const void *motion_v, float *images, int *n_images_host,
                        cmax_stream_t stream) {
    CMAX_REFUSE_WEIGHTED(h, "objective_vote");
    const float *motion = static_cast<const float *>(motion_v);  // double theta[2] when d->motion_dtype == CMAX_F64
    int rc = check_objective_args(h, d, motion);
    if (rc) return rc;
    CMAX_REQUIRE(images && n_images_host, "objective_vote: images / n_images_host");
    rc = kernel_motion(h, d, motion_v, (hipStream_t)stream, &motion);
    if (rc) return rc;
    VoteJobs jobs;
    jobs.publish_windows = true;
    return objective_vote(h, d, motion, images, 0u, n_images_host, (hipStream_t)stream, jobs);
}

// ---- the stages of objective_finish, in the order they enqueue
// blur (when the cost blurs) and statistics of the un-warped image `raw` into slot 4, cached per batch under the key orig_cache_hit compares
static int orig_image_stats(cmax_handle_s *h, const cmax_objective_t *d, const float *raw, float *blur, float *zero_img, hipStream_t s) {
    const float *img = nullptr;
    int rc = blur_image(h, d->sigma, raw, blur, &img, s);
    if (rc) return rc;
    // orig_iwe is NOT boundary-cropped for the variance (normalized_image_variance.py:40-41)
    const int omit_o = d->cost == CMAX_COST_VARIANCE ? 0 : d->omit_boundary;
    rc = launch_stats(h, d->cost, img, omit_o, 4, zero_img, s);
    if (rc) return rc;
    h->orig_valid = true;
    h->orig_sigma = d->sigma;
    h->orig_cost = d->cost;
    h->orig_omit = d->omit_boundary;
    return 0;
}

static dim3 gm_grid(const cmax_handle_s *h, const cmax_objective_t *d) {  // one 8 x 32 pixel tile per workgroup
    return dim3(div_up(h->Hp, kGmTileH) * div_up(h->Wp, kGmTileW), d->n_ref);
}

// contrast statistics: one fused blur + statistics kernel (blurred variance), or blur + k_stats per reference time -- or nothing
// where K3 / the fused image kernel of finish_gimage produce them
static int finish_contrast_stats(cmax_handle_s *h, const cmax_objective_t *d, const EvalPlan &p, const ObjParams &op, const ImgArgs &ia, hipStream_t s) {
    const int Hp = h->Hp, Wp = h->Wp;
    const int64_t npix = (int64_t)Hp * Wp;
    if (p.fused_bv) {
        ProfScope prof(h, kProfStats, s);
        for (int rep = 0; rep < h->prof_repeat; ++rep)
            hipLaunchKernelGGL(k_blur_stats_adj_var, gm_grid(h, d), dim3(256), 0, s, ia.in[0], npix, Hp, Wp, ia, p.tap0, p.tap1, d->omit_boundary, op.nsub,
                               h->d_stat, p.stats_clear4, p.n_stats_clear4, h->d_musum + (int64_t)h->mu_buf * 4 * kMuStride,
                               h->d_musum + (int64_t)(h->mu_buf ^ 1) * 4 * kMuStride, h->n);
        CMAX_CHECK_LAUNCH();
        h->mu_buf ^= 1;  // the next evaluation adds into the buffer this launch cleared
    } else if (p.blur_var) {
        ProfScope prof(h, kProfStats, s);
        for (int rep = 0; rep < h->prof_repeat; ++rep)
            hipLaunchKernelGGL(k_blur_stats_var, dim3(stat_blocks(h), d->n_ref), dim3(256), 0, s, ia.in[0], npix, Hp, Wp, ia, p.tap0, p.tap1, d->omit_boundary,
                               op.nsub, h->d_stat, p.stats_clear4, p.n_stats_clear4);
        CMAX_CHECK_LAUNCH();
    } else if (!(p.deferred || p.fused_gm || p.fused_st || p.stats_inside)) {  // those get their statistics from K3 / from the fused image kernel
        for (int k = 0; k < d->n_ref; ++k) {
            const float *img = nullptr;
            int rc = blur_image(h, d->sigma, ia.in[k], h->iweb[k], &img, s);
            if (rc) return rc;
            rc = launch_stats(h, d->cost, img, d->omit_boundary, k, ia.zero[k], s, k == 0 ? (float *)p.stats_clear4 : nullptr, k == 0 ? 4 * p.n_stats_clear4 : 0);
            if (rc) return rc;
        }
    }
    return 0;
}

// value only, or a rank without events: the loss by its own tiny launch (k_finalize); a zero gradient that still takes part in every band's exchange
static int finish_without_gather(cmax_handle_s *h, const EvalPlan &p, const ObjParams &op, double *result, void *grad, hipStream_t s) {
    {
        ProfScope prof(h, kProfFinish, s);
        hipLaunchKernelGGL(k_finalize, dim3(1), dim3(64), 0, s, op, h->d_stat, result);
        CMAX_CHECK_LAUNCH();
    }
    if (!grad) return 0;
    CMAX_CHECK_HIP(hipMemsetAsync(grad, 0, p.g.bytes, s));  // this rank holds no events of the batch
    return p.bands > 1 ? c2_exchange_all_bands(h, p.c2_comm, (float *)grad, p.bands, s, result) : 0;
}

// room for `count` fixed-point gradient accumulators (deterministic flow gradients; zero between evaluations)
static int reserve_g64(cmax_handle_s *h, int64_t count, hipStream_t s) {
    bool fresh = false;
    int rc = h->g64.reserve(&h->bytes, count, s, &fresh);
    if (rc) return rc;
    if (fresh) CMAX_CHECK_HIP(hipMemsetAsync(h->g64, 0, (size_t)count * sizeof(long long), s));
    return 0;
}

// deterministic mode: the fixed-point sums of the gather -> the gradient (2-DoF: per-segment partials in d_gpart; flow: g64)
static int launch_finish_det(cmax_handle_s *h, const cmax_objective_t *d, void *out, hipStream_t s) {
    const int64_t gcount = grad_extent(h, d).count;
    if (d->model == CMAX_MODEL_2DOF)
        hipLaunchKernelGGL(k_finish_det, dim3(1), dim3(256), 0, s, reinterpret_cast<long long *>(h->d_gpart.get()), h->nseg, d->n_ref, h->d_det_inv_scale, (double *)out);
    else
        hipLaunchKernelGGL(k_fixed_to_grad, dim3(stream_grid(gcount, 256)), dim3(256), 0, s, h->g64, (float *)out, gcount, h->d_det_inv_scale);
    CMAX_CHECK_LAUNCH();
    return 0;
}

// dL/dIWE with its chain factor from the finished statistics: k_gimage on the (blurred) image, then the blur transpose (the unfused image
// path: deterministic mode, and the focus losses under CMAX_NO_FUSED_FOCUS)
static int launch_gimage_unfused(cmax_handle_s *h, const cmax_objective_t *d, const EvalPlan &p, const ObjParams &op, hipStream_t s) {
    const int Hp = h->Hp, Wp = h->Wp;
    const int64_t npix = (int64_t)Hp * Wp;
    if (d->sigma > 0) {
        int rc = h->Gt_det.reserve(&h->bytes, 4 * npix, s);
        if (rc) return rc;
    }
    float *gdst = d->sigma > 0 ? h->Gt_det : h->G;
    const dim3 igrid(div_up(npix, 256), d->n_ref);
    // the n_ref images are not contiguous (last_iwe[k] = blurred copies or the caller's buffer): one launch each
    with_cost(d->cost, [&](auto c) {
        for (int k = 0; k < d->n_ref; ++k)
            hipLaunchKernelGGL(k_gimage<c.value>, dim3(igrid.x), dim3(256), 0, s, h->last_iwe[k], op, k, h->d_stat, gdst + k * npix, (int64_t)0);
    });
    if (d->sigma > 0) hipLaunchKernelGGL(k_blur3_adj<float>, igrid, dim3(256), 0, s, h->Gt_det, Hp, Wp, p.tap0, p.tap1, h->G, npix);
    CMAX_CHECK_LAUNCH();
    return 0;
}

// backward, image space: the clearing memset of the flow gradient where no launch does it, then dL/dIWE as a G image per reference time
// (folded into K3 for the plain variance) -- deterministic: absmax pre-pass + the unfused k_gimage [+ blur transpose]
static int finish_gimage(cmax_handle_s *h, const cmax_objective_t *d, const EvalPlan &p, const ObjParams &op, const ImgArgs &ia, void *grad, hipStream_t s) {
    const int Hp = h->Hp, Wp = h->Wp;
    const int64_t npix = (int64_t)Hp * Wp;
    if (p.memset_grad) CMAX_CHECK_HIP(hipMemsetAsync(grad, 0, p.g.bytes, s));
    if (h->deterministic) {  // the unfused image path (k_blur3, k_stats with one workgroup per accumulator, k_gimage, k_blur3_adj: every sum in a fixed order)
        // bound of the per-event terms: max |image the contrast is evaluated on| per reference time (integer max: order-free)
        CMAX_CHECK_HIP(hipMemsetAsync(h->d_imax, 0, kStatSlots * sizeof(unsigned), s));
        ImgArgs im = {};
        for (int k = 0; k < d->n_ref; ++k) im.in[k] = h->last_iwe[k];
        hipLaunchKernelGGL(k_image_absmax, dim3(std::min(stream_grid(npix, 1024), 256), d->n_ref), dim3(256), 0, s, im, npix, 0, h->d_imax);
        CMAX_CHECK_LAUNCH();
        if (p.fold == kFoldNone) {
            int rc = launch_gimage_unfused(h, d, p, op, s);
            if (rc) return rc;
        }
        return d->model == CMAX_MODEL_2DOF ? 0 : reserve_g64(h, p.g.count, s);
    }
    if (p.plain_st) {  // CMAX_NO_FUSED_FOCUS: the statistics are finished (finish_contrast_stats), G with its chain factor by k_gimage
        ProfScope prof(h, kProfGimage, s);
        return launch_gimage_unfused(h, d, p, op, s);
    }
    if (p.fused_st) {
        ProfScope prof(h, kProfStats, s);
        for (int rep = 0; rep < h->prof_repeat; ++rep) {
            if (!(d->sigma > 0)) {  // the votes are contiguous: every reference time in one launch
                with_focus_cost(d->cost, [&](auto c) {
                    hipLaunchKernelGGL(k_stats_gimage_st<c.value>, gm_grid(h, d), dim3(256), 0, s, ia.in[0], npix, Hp, Wp, ia, d->omit_boundary, op.nsub, h->d_stat,
                                       p.stats_clear4, p.n_stats_clear4);
                });
                continue;
            }
            // sigma > 0: k_blur3 -> the fused kernel on the blurred copy, G' into the scratch -> k_blur3_adj (the copies are buffers of
            // their own: one launch per reference time)
            int rc = h->Gt_det.reserve(&h->bytes, 4 * npix, s);
            if (rc) return rc;
            for (int k = 0; k < d->n_ref; ++k) {
                const float *img = nullptr;
                rc = blur_image(h, d->sigma, ia.in[k], h->iweb[k], &img, s);
                if (rc) return rc;
                ImgArgs ik = {};
                ik.zero[0] = ia.zero[k];
                ik.G[0] = h->Gt_det + k * npix;
                ik.chain[0] = ia.chain[k];
                with_focus_cost(d->cost, [&](auto c) {
                    hipLaunchKernelGGL(k_stats_gimage_st<c.value>, dim3(gm_grid(h, d).x), dim3(256), 0, s, img, (int64_t)0, Hp, Wp, ik, d->omit_boundary, op.nsub,
                                       h->d_stat + k * kStatStride, k == 0 ? p.stats_clear4 : nullptr, k == 0 ? p.n_stats_clear4 : (int64_t)0);
                });
            }
            hipLaunchKernelGGL(k_blur3_adj<float>, dim3(div_up(npix, 256), d->n_ref), dim3(256), 0, s, h->Gt_det, Hp, Wp, p.tap0, p.tap1, h->G, npix);
        }
        CMAX_CHECK_LAUNCH();
        return 0;
    }
    if (p.fused_bv) {
        // dL/dIWE was written (without mean and chain factor) by the statistics kernel
    } else if (p.blur_var) {
        ImgArgs ib = ia;
        for (int k = 0; k < d->n_ref; ++k) ib.in[k] = h->iweb[k];
        ProfScope prof(h, kProfGimage, s);
        for (int rep = 0; rep < h->prof_repeat; ++rep)
            hipLaunchKernelGGL(k_gimage_blur_adj_var, dim3(div_up(npix, 256), d->n_ref), dim3(256), 0, s, ib, op, h->d_stat, p.tap0, p.tap1);
        CMAX_CHECK_LAUNCH();
    } else if (p.fused_gm) {
        ProfScope prof(h, kProfStats, s);
        for (int rep = 0; rep < h->prof_repeat; ++rep) {
            if (d->sigma > 0)  // raw votes -> blurred image, statistics and the finished G (blur transpose included)
                hipLaunchKernelGGL(k_blur_stats_gimage_gm, gm_grid(h, d), dim3(256), 0, s, ia.in[0], npix, Hp, Wp, ia, p.tap0, p.tap1, d->omit_boundary, op.nsub,
                                   h->d_stat, p.stats_clear4, p.n_stats_clear4);
            else
                hipLaunchKernelGGL(k_stats_gimage_gm, gm_grid(h, d), dim3(256), 0, s, ia.in[0], npix, Hp, Wp, ia, d->omit_boundary, op.nsub, h->d_stat, p.stats_clear4, p.n_stats_clear4);
        }
        CMAX_CHECK_LAUNCH();
    }
    return 0;
}

// the arguments of K3 (all reference times in one launch); enqueues the windows-only K1 where the handle's windows are not this warp's
static int finish_grad_args(cmax_handle_s *h, const cmax_objective_t *d, const EvalPlan &p, const float *motion, const ImgArgs &ia, RefArgs &ra, hipStream_t s) {
    const int64_t npix = (int64_t)h->Hp * h->Wp;
    fill_ref_times(ra, d->n_ref, d->ref_mode, d->ref_frac);
    bool same_vote = p.whole && h->win_generation == h->generation && h->win_motion == motion && h->win_model == d->model &&
                     h->win_nref == d->n_ref && h->win_T == d->T && h->win_normalize == d->normalize_t;
    for (int k = 0; k < d->n_ref; ++k) {
        ra.img[k] = (p.fold == kFoldNone || p.fold == kFoldScale) ? h->G + k * npix : const_cast<float *>(h->last_iwe[k]);
        ra.zero[k] = (p.deferred || p.stats_inside) ? ia.zero[k] : nullptr;
        same_vote = same_vote && h->win_d[k] == ra.d[k];
    }
    // K3 follows the windows -- and the fp64 cell decisions -- of a K1 launch with exactly this warp: that of the same evaluation, or
    // (the stand-alone cmax_objective_finish, whose vote the handle cannot vouch for) a K1 launch that only publishes them
    if (!same_vote) {
        int rc = publish_windows(h, d, motion, s);
        if (rc) return rc;
    }
    ra.win = h->d_win;
    ra.shifts = h->d_shifts;
    ra.n_events = h->n;
    if (p.stats_inside) {
        ra.stat_blocks = p.stat_blocks;
        ra.ticket = h->d_ticket;
        ra.musum[0] = h->d_musum + (int64_t)h->mu_buf * 4 * kMuStride;
        ra.musum_next = h->d_musum + (int64_t)(h->mu_buf ^ 1) * 4 * kMuStride;
        h->mu_buf ^= 1;  // the next evaluation adds into the buffer this launch clears
    }
    if (h->deterministic) {  // the integer-accumulating K3
        ra.imax = h->d_imax;
        ra.g64 = d->model == CMAX_MODEL_2DOF ? reinterpret_cast<long long *>(h->d_gpart.get()) : h->g64;  // (d_gpart: [4][nseg][6] doubles, 2 used per segment)
        ra.det_inv_scale = h->d_det_inv_scale;
    }
    return 0;
}

// C2 in row bands (cmax_comm_set_c2_bands): dense objective on an owned work list under a communicator.  The owned K3 STORES
// every gradient element of its segments' tiles, so after the launch that covers tile rows [a, b) the pixel rows [16 a, 16 b)
// of both channels are final on this rank: they are all-reduced on the handle's second stream while the caller's stream
// already runs the next band's K3.  One event per band hands the rows over, one event hands the reduced gradient back.
static int finish_grad_in_bands(cmax_handle_s *h, const cmax_objective_t *d, const EvalPlan &p, const EvView &ev, const WarpParams &wp, const RefArgs &ra,
                                const ObjParams &op, double *res, double *result, float *grad, hipStream_t s) {
    int rc = c2_prepare_bands(h, p.bands);
    if (rc) return rc;
    for (int b = 0; b < p.bands; ++b) {
        const int tr0 = (int)((int64_t)h->ntr * b / p.bands), tr1 = (int)((int64_t)h->ntr * (b + 1) / p.bands);
        const int s0 = h->row_seg_start[tr0], s1 = h->row_seg_start[tr1];
        RefArgs rb = ra;
        rb.win += s0;  // (one reference time: the windows of segment i sit at win[i])
        rb.shifts += (int64_t)s0 * (h->big ? 512 : (h->mid ? 384 : 256));
        if (s1 > s0) launch_grad<CMAX_MODEL_DENSE>(h, ev, wp, rb, d->n_ref, p.fold, op, nullptr, grad, b == 0 ? res : nullptr, p.owned, s, s0, s1 - s0);
        CMAX_CHECK_LAUNCH();
        rc = c2_exchange_band(h, p.c2_comm, grad, b, p.bands, s, result);
        if (rc) return rc;
    }
    return c2_join_bands(h, p.bands, s);
}

// 2-DoF, default mode: the one-wave kernel that folds the raw sums into (loss and) gradient -- unless the caller does that itself (raw_only)
static int finish_two_dof(cmax_handle_s *h, const cmax_objective_t *d, const EvalPlan &p, const ObjParams &op, double *result, void *grad, hipStream_t s) {
    if (!p.lines || p.raw_only) return 0;
    ProfScope prof(h, kProfFinish, s);
    if (p.deferred && p.step)
        hipLaunchKernelGGL(k_finish_raw_step, dim3(1), dim3(64), 0, s, (const double *)p.raw, op.n_ref, op, h->d_stat, result, (double *)grad, *p.step);
    else if (p.deferred)
        hipLaunchKernelGGL(k_finish_raw, dim3(1), dim3(64), 0, s, (const double *)p.raw, op.n_ref, op, h->d_stat, result, (double *)grad, p.host_flag, p.host_seq);
    else  // (host_flag: K3's first workgroup wrote the loss into the pinned `result`)
        hipLaunchKernelGGL(k_finish_lines, dim3(1), dim3(64), 0, s, p.raw, d->n_ref, (double *)grad, (const double *)nullptr, (double *)nullptr, p.host_flag, p.host_seq);
    CMAX_CHECK_LAUNCH();
    return 0;
}

static int objective_finish(cmax_handle_t h, const cmax_objective_t *d, const EvalPlan &p, const float *motion, const float *images, int n_images, float *zero_next, double *result,
                            void *grad, hipStream_t s) {
    const int64_t npix = (int64_t)h->Hp * h->Wp;
    const ObjParams op = obj_params(h, d);
    int rc = 0;
    if (d->normalized) {  // statistics of the un-warped image (slot 4) are cached per batch
        if (n_images == d->n_ref + 1) {
            rc = orig_image_stats(h, d, images + (int64_t)d->n_ref * npix, h->iweb[4], zero_next ? zero_next + (int64_t)d->n_ref * npix : nullptr, s);
            if (rc) return rc;
        } else if (!orig_cache_hit(h, d)) {
            set_error("objective_finish: normalised cost needs the un-warped image (n_images == n_ref + 1)");
            return CMAX_ESTATE;
        }
    }
    if (p.lines && !p.whole) CMAX_CHECK_HIP(hipMemsetAsync(p.raw, 0, (size_t)d->n_ref * kRawStride * sizeof(double), s));  // (whole: K1 cleared them)
    // per-reference-time pointers of the image kernels (every kernel class covers all reference times in one launch)
    // zero_next: base of the image buffer of the NEXT evaluation (the statistics of image k zero zero_next[k]) or nullptr
    ImgArgs ia = {};
    for (int k = 0; k < d->n_ref; ++k) {
        ia.in[k] = images + k * npix;
        ia.blurred[k] = h->iweb[k];
        ia.zero[k] = zero_next ? zero_next + k * npix : nullptr;
        ia.G[k] = h->G + k * npix;
        // not normalised: the chain factor of chain_coef is a constant -- the fused image kernels fold it into G and K3 reads a finished image
        ia.chain[k] = op.normalized ? 1.f : (float)((op.negate ? -1.0 : 1.0) * op.mult[k] * (op.minimize ? -1.0 : 1.0));
        h->last_iwe[k] = d->sigma > 0 ? h->iweb[k] : images + k * npix;  // the image the contrast is evaluated on
    }
    rc = finish_contrast_stats(h, d, p, op, ia, s);
    if (rc) return rc;
    if (!grad || h->n == 0) return finish_without_gather(h, p, op, result, grad, s);
    rc = finish_gimage(h, d, p, op, ia, grad, s);
    if (rc) return rc;
    RefArgs ra = {};
    rc = finish_grad_args(h, d, p, motion, ia, ra, s);
    if (rc) return rc;
    const EvView ev = ev_view(h);
    const WarpParams wp = warp_params(h, motion, d->T, d->ref_mode[0], d->ref_frac[0], d->normalize_t, d->motion_dtype == CMAX_F64);
    // the first workgroup writes the loss (deferred: the finishing step does).  Raw form of an objective with statistics: into doubles
    // 8..15 of the first line of the raw buffer (the sums use doubles 0, 1 of every line)
    double *res = p.deferred ? nullptr : (p.raw_only ? p.raw + 8 : result);
    if (p.k3_in_bands) return finish_grad_in_bands(h, d, p, ev, wp, ra, op, res, result, (float *)grad, s);
    // K3 in one launch
    const bool two_dof = d->model == CMAX_MODEL_2DOF;
    double *gpart = two_dof ? (p.lines ? p.raw : h->d_gpart) : nullptr;
    float *gflow = two_dof ? nullptr : (float *)grad;
    with_model(d->model, [&](auto m) { launch_grad<m.value>(h, ev, wp, ra, d->n_ref, p.fold, op, gpart, gflow, res, p.owned, s); });
    CMAX_CHECK_LAUNCH();
    if (h->deterministic) {
        ProfScope prof(h, kProfFinish, s);
        rc = launch_finish_det(h, d, grad, s);
        if (rc) return rc;
    }
    // this rank's work list does not allow K3 in bands (or the mode is deterministic): the same exchanges behind one launch
    if (p.bands > 1) return c2_exchange_all_bands(h, p.c2_comm, (float *)grad, p.bands, s, result);
    return finish_two_dof(h, d, p, op, result, grad, s);
}

int cmax_objective_finish(cmax_handle_t h, const cmax_objective_t *d, const void *motion_v, const float *images, int n_images,
                          double *result, void *grad, cmax_stream_t stream) {
    CMAX_REFUSE_WEIGHTED(h, "objective_finish");
    const float *motion = static_cast<const float *>(motion_v);  // double theta[2] when d->motion_dtype == CMAX_F64
    int rc = check_objective_args(h, d, motion);
    if (rc) return rc;
    CMAX_REQUIRE(images && result, "objective_finish: images / result");
    CMAX_REQUIRE(n_images == d->n_ref || n_images == d->n_ref + 1, "objective_finish: n_images");
    // (an fp64 flow is split into the scratch every vote's split went to: the handle's windows are this motion's only if that vote's was)
    if (h->m64 && h->win_motion == h->m64 && h->m64_src != motion_v) h->win_motion = nullptr;
    rc = kernel_motion(h, d, motion_v, (hipStream_t)stream, &motion);
    if (rc) return rc;
    return objective_finish(h, d, eval_plan(h, d, grad, false), motion, images, n_images, nullptr, result, grad, (hipStream_t)stream);
}

static int objective_eval_tan2(cmax_handle_t h, const cmax_objective_t *d, const float *motion, double *result, void *grad, hipStream_t s,
                               cmax::Comm *comm) {
    const int Hp = h->Hp, Wp = h->Wp, nr = d->n_ref;
    const int64_t tsize = (int64_t)3 * Hp * Wp + Hp + Wp;
    const int64_t tstride = (tsize + 3) & ~(int64_t)3;  // 16-byte aligned planes: the clearing stores are 16 bytes wide
    int rc = 0;
    bool fresh = false;
    rc = h->tan.reserve(&h->bytes, 2 * 4 * tstride, s, &fresh);
    if (!rc) rc = h->d_tanpart.reserve(&h->bytes, 4 * kTanBlocks * 6, s);
    if (rc) return rc;
    if (fresh) h->tan_zero_mask[0] = h->tan_zero_mask[1] = 0u;
    float *cur = h->tan + (int64_t)h->tan_cur * 4 * tstride, *nxt = h->tan + (int64_t)(h->tan_cur ^ 1) * 4 * tstride;
    RefArgs ra = {};
    fill_ref_times(ra, nr, d->ref_mode, d->ref_frac);
    for (int k = 0; k < nr; ++k) {
        if (!((h->tan_zero_mask[h->tan_cur] >> k) & 1u)) CMAX_CHECK_HIP(hipMemsetAsync(cur + k * tstride, 0, (size_t)tstride * sizeof(float), s));
        ra.img[k] = cur + k * tstride;
    }
    const unsigned used = (1u << nr) - 1u;
    h->tan_zero_mask[h->tan_cur] &= ~used;
    const WarpParams wp = warp_params(h, motion, 0, d->ref_mode[0], d->ref_frac[0], d->normalize_t, d->motion_dtype == CMAX_F64);
    if (h->n > 0) {
        launch_vote_tan2(h, ev_view(h), wp, ra, nr, s);
        CMAX_CHECK_LAUNCH();
    }
    if (comm) {  // the ONE exchange of a 2-DoF evaluation: all planes of all reference times are contiguous
        ProfScope prof(h, kProfComm, s);
        rc = comm_allreduce(comm, cur, (size_t)nr * tstride, kCommF32, kCommSum, s);
        if (rc) return rc;
    }
    for (int k = 0; k < nr; ++k) h->last_iwe[k] = cur + k * tstride;  // the raw image is the first plane
    {
        ProfScope prof(h, kProfStats, s);
        for (int rep = 0; rep < h->prof_repeat; ++rep)
            hipLaunchKernelGGL(k_tan_stats_var, dim3(kTanBlocks, nr), dim3(256), 0, s, cur, nxt, tstride, Hp, Wp, d->omit_boundary, d->normalize_t,
                               h->d_tmm, h->d_tanpart);
        CMAX_CHECK_LAUNCH();
    }
    h->tan_zero_mask[h->tan_cur ^ 1] |= used;
    h->tan_cur ^= 1;
    const ObjParams op = obj_params(h, d);
    {
        ProfScope prof(h, kProfFinish, s);
        hipLaunchKernelGGL(k_finish_deferred, dim3(1), dim3(256), 0, s, op, h->d_stat, h->d_tanpart, kTanBlocks, result, (double *)grad);
        CMAX_CHECK_LAUNCH();
    }
    return 0;
}

// vote -> [all-reduce of the images] -> finish -> [all-reduce of the gradient], all on the handle's double-buffered images
static int objective_eval(cmax_handle_t h, const cmax_objective_t *d, const float *motion, double *result, void *grad, hipStream_t s,
                          const EvalForm &form = {}) {
    const EvalPlan p = eval_plan(h, d, grad, true, form);
    cmax::Comm *const comm = form.comm;
    if (p.tan2) return objective_eval_tan2(h, d, motion, result, grad, s, comm);
    if (p.raw_only && !p.lines) {
        set_error("objective_raw: this objective has no raw form (2-DoF, a non-empty batch, not deterministic)");
        return CMAX_EINVAL;
    }
    if (p.empty) {
        CMAX_CHECK_HIP(hipMemsetAsync(result, 0, 8 * sizeof(double), s));
        if (grad) CMAX_CHECK_HIP(hipMemsetAsync(grad, 0, p.g.bytes, s));
        return 0;
    }
    const int64_t npix = (int64_t)h->Hp * h->Wp;
    float *cur = h->imgs + (int64_t)h->cur_buf * 5 * npix;
    float *nxt = h->imgs + (int64_t)(h->cur_buf ^ 1) * 5 * npix;
    int n_images = 0;
    const int mu_buf = h->mu_buf;
    int rc = objective_vote(h, d, motion, cur, h->zero_mask[h->cur_buf], &n_images, s, p.vote);
    if (rc) return rc;
    const unsigned used = (1u << n_images) - 1u;
    h->zero_mask[h->cur_buf] &= ~used;  // now holds votes
    if (comm) {  // C1: every reference time (+ the un-warped image) in one call; the images are contiguous
        ProfScope prof(h, kProfComm, s);
        rc = comm_allreduce(comm, cur, (size_t)n_images * npix, kCommF32, kCommSum, s);
        if (rc) return rc;
    }
    rc = objective_finish(h, d, p, motion, cur, n_images, nxt, result, grad, s);
    if (rc) {
        // K1 summed its votes and the error came before the launch that reads them (it clears the other buffer and flips mu_buf): the
        // next evaluation must find clean accumulators
        if (p.vote.sums && h->mu_buf == mu_buf) (void)hipMemsetAsync(h->d_musum + (int64_t)mu_buf * 4 * kMuStride, 0, (size_t)4 * kMuStride * sizeof(double), s);
        return rc;
    }
    h->zero_mask[h->cur_buf ^ 1] |= used;  // zeroed by this evaluation's k_stats launches
    h->cur_buf ^= 1;
    if (p.c2_comm && p.bands == 1) {  // C2, result[8] riding along (rank-consistent scalars); bands > 1: exchanged behind K3 already
        ProfScope prof(h, kProfComm, s);
        rc = grad_and_result_exchange(comm, grad, (size_t)p.g.count, p.g.type, result, s);
        if (rc) return rc;
    } else if (p.result_alone) {  // value only: the 64 bytes on their own
        ProfScope prof(h, kProfComm, s);
        rc = result_exchange_alone(comm, result, s);
        if (rc) return rc;
    }
    return 0;
}

int cmax_objective(cmax_handle_t h, const cmax_objective_t *d, const void *motion_v, double *result, void *grad,
                   cmax_stream_t stream) {
    const float *motion = static_cast<const float *>(motion_v);  // double theta[2] when d->motion_dtype == CMAX_F64
    int rc = check_objective_args(h, d, motion);
    if (rc) return rc;
    CMAX_REQUIRE(result, "objective: result");
    rc = kernel_motion(h, d, motion_v, (hipStream_t)stream, &motion);
    if (rc) return rc;
    return objective_eval(h, d, motion, result, grad, (hipStream_t)stream);
}

}  // extern "C"

// ---- dL/dw of the fused objective (cmax_objective_weight_grad) ---------------------------------------------------------------
namespace cmax {
// dL/dI_orig of a normalised cost: the un-warped image is a (weighted) vote too, so v_orig depends on the weights.
//   L = +- sum_k m_k v_orig / v_k (minimize) | +- sum_k m_k v_k / v_orig   ->   dL/dv_orig = +- sum_k m_k / v_k | -+ sum_k m_k v_k / v_orig^2
// from the fp64 statistics on the device (slots 0 .. n_ref - 1 and 4); dv_orig/dI as k_gimage, with the region orig_value uses.
template <int COST>
__global__ void __launch_bounds__(256) k_gimage_orig(const float *__restrict__ img, ObjParams op, const double *__restrict__ stat, float *__restrict__ G) {
    const int H = op.H, W = op.W;
    const int omit_o = COST == CMAX_COST_VARIANCE ? 0 : op.omit;  // orig_iwe is NOT boundary-cropped for the variance
    const int i0 = omit_o ? 1 : 0;
    const double npix = region_pixels(H, W, omit_o), npix_k = region_pixels(H, W, op.omit);
    double acc[2], mu = 0.0;
    stat_sum<true>(stat, 4, op.nsub, acc);  // every wave is converged here
    const double v_orig = contrast_value(COST, acc, npix, &mu);
    double coef = 0.0;
    for (int k = 0; k < op.n_ref; ++k) {
        double ak[2];
        stat_sum<true>(stat, k, op.nsub, ak);
        const double v = contrast_value(COST, ak, npix_k, nullptr);
        coef += op.mult[k] * (op.minimize ? 1.0 / v : -v / (v_orig * v_orig));
    }
    if (op.negate) coef = -coef;
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (int64_t)H * W) return;
    const int i = (int)(p / W), j = (int)(p % W);
    if (COST == CMAX_COST_VARIANCE) {
        const bool in = (i >= i0) && (i < H - i0) && (j >= i0) && (j < W - i0);
        G[p] = in ? (float)(coef * 2.0 * ((double)img[p] - mu) / (npix - 1.0)) : 0.f;
    } else if constexpr (COST == CMAX_COST_GRADMAG) {
        G[p] = (float)(coef * (2.0 / npix) / 8.0) * sobel8_adj_f32(img, H, W, i0, i, j);
    } else if constexpr (COST != CMAX_COST_VARIANCE) {  // a focus loss (FocusStencil, cmax_image_kernels.h)
        float v5[5][5];
        focus_load<2, float>(img, H, W, i, j, v5);
        G[p] = (float)(coef * (2.0 / npix)) * focus_adj<COST, float>(v5, H, W, i0, i, j);
    }
}

// grad_w[src[i]] = sum over the planes, in index order, of gw_packed[plane][i] (behind a zero fill of grad_w: events that were not packed keep 0)
__global__ void __launch_bounds__(256) k_weight_grad_scatter(const float *__restrict__ gw, int64_t plane, int n_planes, const int *__restrict__ src, int64_t n,
                                                            float *__restrict__ grad_w) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float a = gw[i];
    for (int q = 1; q < n_planes; ++q) a += gw[(int64_t)q * plane + i];
    grad_w[src[i]] = a;
}

// cmax_objective_event_grad: grad_events[src[i]] = (sum_k gx, sum_k gy, sum_k c) over the planes of ge_packed in index order (+ the un-warped image's
// x and y planes), behind a zero fill of grad_events.  csum[k] = sum_i c_{i,k} in fp64 without atomics: a fixed tree per workgroup into
// part[k][block], folded by k_event_csum_finish in a fixed order -- the same bits on every run.
constexpr int kEventGradPlanes = 14;  // three per reference time (at most four) + two for the un-warped image
__device__ __forceinline__ double block_sum_256(double v, double *s_red) {  // every thread of a 256-thread workgroup; the sum in thread 0
    __syncthreads();
    s_red[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s_red[threadIdx.x] += s_red[threadIdx.x + w];
        __syncthreads();
    }
    return s_red[0];
}
__global__ void __launch_bounds__(256) k_event_grad_scatter(const float *__restrict__ ge, int64_t plane, int n_ref, int has_orig, const int *__restrict__ src, int64_t n,
                                                           float *__restrict__ grad_events, double *__restrict__ part, int64_t n_blocks) {
    __shared__ double s_red[256];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < n;
    float gx = 0.f, gy = 0.f, c = 0.f;
    for (int k = 0; k < n_ref; ++k) {
        const float *p = ge + (int64_t)(3 * k) * plane;
        const float ck = valid ? p[2 * plane + i] : 0.f;
        if (valid) {
            gx += p[i];
            gy += p[plane + i];
            c += ck;
        }
        const double tot = block_sum_256((double)ck, s_red);
        if (threadIdx.x == 0) part[(int64_t)k * n_blocks + blockIdx.x] = tot;
    }
    if (!valid) return;
    if (has_orig) {
        const float *p = ge + (int64_t)(3 * n_ref) * plane;
        gx += p[i];
        gy += p[plane + i];
    }
    float *out = grad_events + 3 * (int64_t)src[i];
    out[0] = gx;
    out[1] = gy;
    out[2] = c;
}
// csum[k] (blockIdx.x = k < 4): thread t adds part[k][t], part[k][t + 256], ... in that order, then the tree; entries k >= n_ref are zero
__global__ void __launch_bounds__(256) k_event_csum_finish(const double *__restrict__ part, int64_t n_blocks, int n_ref, double *__restrict__ csum) {
    __shared__ double s_red[256];
    const int k = blockIdx.x;
    double a = 0.0;
    if (k < n_ref)
        for (int64_t b = threadIdx.x; b < n_blocks; b += 256) a += part[(int64_t)k * n_blocks + b];
    const double tot = block_sum_256(a, s_red);
    if (threadIdx.x == 0) csum[k] = tot;
}

// the first n_planes of a packed per-event buffer (gw_packed: 5 planes, ge_packed: kEventGradPlanes), zeroed; a plane is sized like w_packed
static int reserve_packed_planes(cmax_handle_s *h, DevBuf<float> &packed, int64_t *plane_len, int capacity, int n_planes, hipStream_t s) {
    if (h->n > *plane_len) {  // (the plane's length is the layout of the buffer too: kept beside it)
        *plane_len = 0;
        const int64_t plane = (h->n + kWeightPad + 3) & ~(int64_t)3;
        int rc = packed.reserve(&h->bytes, capacity * plane, s);
        if (rc) return rc;
        *plane_len = plane;
    }
    CMAX_CHECK_HIP(hipMemsetAsync(packed, 0, (size_t)n_planes * *plane_len * sizeof(float), s));
    return 0;
}

// One more plane: the un-warped events against G_orig, behind a K1 launch that only publishes their windows.  gather(ev, wp, ra) launches
// K3w / K3e of that one image into its plane.
template <class Gather>
static int gather_unwarped(cmax_handle_s *h, const float *G_orig, hipStream_t s, Gather &&gather) {
    const EvView ev = ev_view(h);
    RefArgs ra = {};
    const int ref_mode = CMAX_REF_FIRST;
    const double frac = 0.0;
    fill_ref_times(ra, 1, &ref_mode, &frac);
    ra.win = h->d_win;
    ra.shifts = h->d_shifts;
    ra.windows_only = 1;
    const WarpParams wp = warp_params(h, nullptr, 0, CMAX_REF_FIRST, 0.0, 1);
    launch_vote<-1>(h, ev, wp, ra, 1, s);
    CMAX_CHECK_LAUNCH();
    h->win_motion = nullptr;  // (the handle's windows are no evaluation's any more)
    h->win_generation = ~(uint64_t)0;
    ra.windows_only = 0;
    ra.img[0] = const_cast<float *>(G_orig);  // (read only by the gather)
    gather(ev, wp, ra);
    CMAX_CHECK_LAUNCH();
    return 0;
}

// behind objective_eval of the same call: its images, statistics, windows and cell offsets are the handle's current ones.
// grad_events == nullptr: dL/dw into grad_w (one plane per image); else dL/d(event) into grad_events [n][3] and csum[4] (three planes
// per reference time, two for the un-warped image)
static int per_event_finish(cmax_handle_s *h, const cmax_objective_t *d, const float *motion, const float *orig_raw, float *grad_w, float *grad_events, double *csum,
                            hipStream_t s) {
    const int Hp = h->Hp, Wp = h->Wp, nr = d->n_ref;
    const int64_t npix = (int64_t)Hp * Wp;
    const bool events = grad_events != nullptr;
    const int n_planes = events ? 3 * nr + (d->normalized ? 2 : 0) : nr + (d->normalized ? 1 : 0);
    int rc = h->gw_G.reserve(&h->bytes, 5 * npix, s);
    if (!rc) rc = h->gw_Gt.reserve(&h->bytes, 5 * npix, s);
    if (rc) return rc;
    rc = events ? reserve_packed_planes(h, h->ge_packed, &h->ge_plane, kEventGradPlanes, n_planes, s) : reserve_packed_planes(h, h->gw_packed, &h->gw_plane, 5, n_planes, s);
    if (rc) return rc;
    if (events) {  // per-workgroup partial sums of the scatter (csum), [4][blocks]
        rc = h->ge_part.reserve(&h->bytes, (int64_t)4 * div_up(h->n, 256), s);
        if (rc) return rc;
    }
    const ObjParams op = obj_params(h, d);
    double k0 = 0, k1 = 0;
    if (d->sigma > 0) blur_taps(d->sigma, k0, k1);
    // G_k = dL/dIWE_k with its chain factor (multi-focal multipliers included), the blur transpose applied
    float *gdst = d->sigma > 0 ? h->gw_Gt : h->gw_G;
    const dim3 igrid(div_up(npix, 256));
    with_cost(d->cost, [&](auto c) {
        for (int k = 0; k < nr; ++k) hipLaunchKernelGGL(k_gimage<c.value>, igrid, dim3(256), 0, s, h->last_iwe[k], op, k, h->d_stat, gdst + k * npix, (int64_t)0);
        if (d->normalized) {  // slot 4: G_orig on the (blurred) un-warped image
            const float *img = d->sigma > 0 ? h->iweb[4] : orig_raw;
            hipLaunchKernelGGL(k_gimage_orig<c.value>, igrid, dim3(256), 0, s, img, op, h->d_stat, gdst + 4 * npix);
        }
    });
    if (d->sigma > 0) {
        hipLaunchKernelGGL(k_blur3_adj<float>, dim3(igrid.x, nr), dim3(256), 0, s, h->gw_Gt, Hp, Wp, (float)k0, (float)k1, h->gw_G, npix);
        if (d->normalized)
            hipLaunchKernelGGL(k_blur3_adj<float>, igrid, dim3(256), 0, s, h->gw_Gt + 4 * npix, Hp, Wp, (float)k0, (float)k1, h->gw_G + 4 * npix, (int64_t)0);
    }
    CMAX_CHECK_LAUNCH();
    const EvView ev = ev_view(h);
    {  // one plane per reference time: the windows and cells K1 of this evaluation published
        RefArgs ra = {};
        fill_ref_times(ra, nr, d->ref_mode, d->ref_frac);
        for (int k = 0; k < nr; ++k) ra.img[k] = h->gw_G + k * npix;
        ra.win = h->d_win;
        ra.shifts = h->d_shifts;
        const WarpParams wp = warp_params(h, motion, d->T, d->ref_mode[0], d->ref_frac[0], d->normalize_t, d->motion_dtype == CMAX_F64);
        with_model(d->model, [&](auto m) {
            if (events) launch_event_gather<m.value>(h, ev, wp, ra, nr, 0, s);
            else launch_weight_gather<m.value>(h, ev, wp, ra, nr, 0, s);
        });
        CMAX_CHECK_LAUNCH();
    }
    if (d->normalized) {
        rc = gather_unwarped(h, h->gw_G + 4 * npix, s, [&](const EvView &ev, const WarpParams &wp, const RefArgs &ra) {
            if (events) launch_event_gather<-1>(h, ev, wp, ra, 1, 3 * nr, s);
            else launch_weight_gather<-1>(h, ev, wp, ra, 1, nr, s);
        });
        if (rc) return rc;
    }
    if (events) {
        const int64_t blocks = div_up(h->n, 256);
        hipLaunchKernelGGL(k_event_grad_scatter, dim3(blocks), dim3(256), 0, s, (const float *)h->ge_packed, h->ge_plane, nr, d->normalized ? 1 : 0, (const int *)h->src, h->n,
                           grad_events, h->ge_part, blocks);
        hipLaunchKernelGGL(k_event_csum_finish, dim3(4), dim3(256), 0, s, (const double *)h->ge_part, blocks, nr, csum);
    } else {
        hipLaunchKernelGGL(k_weight_grad_scatter, dim3(div_up(h->n, 256)), dim3(256), 0, s, (const float *)h->gw_packed, h->gw_plane, n_planes, (const int *)h->src, h->n, grad_w);
    }
    CMAX_CHECK_LAUNCH();
    return 0;
}
}  // namespace cmax

extern "C" {

// the per-event derivatives and the IWE layer are not built for these two kinds of handle (`what`: the entry that was called)
static int refuse_det_or_comm(const cmax_handle_s *h, const char *what) {
    if (h->deterministic) {
        set_error("%s: not built for deterministic mode (cmax_set_deterministic)", what);
        return CMAX_EUNSUPPORTED;
    }
    if (h->comm) {
        set_error("%s: not built for a handle with a communicator (cmax_comm_init)", what);
        return CMAX_EUNSUPPORTED;
    }
    return 0;
}

// what cmax_objective_weight_grad and _event_grad check alike (`what`: the entry that was called)
static int per_event_check(cmax_handle_t h, const cmax_objective_t *d, const float *motion, int64_t n, const char *what) {
    int rc = check_objective_args(h, d, motion);
    if (rc) return rc;
    if (n != h->n_in) {
        set_error("%s:%d bad argument: %s: n must equal the n of the last cmax_set_events (one row of the result per event, in the caller's order)", __FILE__, __LINE__, what);
        return CMAX_EINVAL;
    }
    return refuse_det_or_comm(h, what);
}

// The evaluation in front of per_event_finish: the general path (K1 -> statistics / image kernel -> K3) on any handle, and the un-warped
// image voted again into *orig_raw: G_orig needs the image itself, the per-batch cache keeps its statistics only
static int per_event_eval(cmax_handle_t h, const cmax_objective_t *d, const float *motion, double *result, void *grad, hipStream_t s, const float **orig_raw) {
    const int64_t npix = (int64_t)h->Hp * h->Wp;
    *orig_raw = h->imgs + (int64_t)h->cur_buf * 5 * npix + (int64_t)d->n_ref * npix;
    h->general_only = true;
    if (d->normalized) h->orig_valid = false;
    const int rc = objective_eval(h, d, motion, result, grad, s);
    h->general_only = false;
    return rc;
}

int cmax_objective_weight_grad(cmax_handle_t h, const cmax_objective_t *d, const void *motion_v, double *result, void *grad, float *grad_w,
                               int64_t n, cmax_stream_t stream) {
    const float *motion = static_cast<const float *>(motion_v);  // double theta[2] when d->motion_dtype == CMAX_F64
    CMAX_REQUIRE(result && (grad_w || n == 0), "objective_weight_grad: result / grad_w (grad_w may be NULL only for n == 0)");
    int rc = per_event_check(h, d, motion, n, "objective_weight_grad");
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    rc = kernel_motion(h, d, motion_v, s, &motion);
    if (rc) return rc;
    if (n > 0) CMAX_CHECK_HIP(hipMemsetAsync(grad_w, 0, (size_t)n * sizeof(float), s));
    const float *orig_raw = nullptr;
    rc = per_event_eval(h, d, motion, result, grad, s, &orig_raw);
    if (rc || h->n == 0) return rc;
    return per_event_finish(h, d, motion, orig_raw, grad_w, nullptr, nullptr, s);
}

int cmax_objective_event_grad(cmax_handle_t h, const cmax_objective_t *d, const void *motion_v, double *result, void *grad, float *grad_events,
                              int64_t n, double *csum, cmax_stream_t stream) {
    const float *motion = static_cast<const float *>(motion_v);  // double theta[2] when d->motion_dtype == CMAX_F64
    CMAX_REQUIRE(result && csum && (grad_events || n == 0), "objective_event_grad: result / csum / grad_events (grad_events may be NULL only for n == 0)");
    int rc = per_event_check(h, d, motion, n, "objective_event_grad");
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    rc = kernel_motion(h, d, motion_v, s, &motion);
    if (rc) return rc;
    if (n > 0) CMAX_CHECK_HIP(hipMemsetAsync(grad_events, 0, (size_t)n * 3 * sizeof(float), s));
    CMAX_CHECK_HIP(hipMemsetAsync(csum, 0, 4 * sizeof(double), s));
    const float *orig_raw = nullptr;
    rc = per_event_eval(h, d, motion, result, grad, s, &orig_raw);
    if (rc || h->n == 0) return rc;
    return per_event_finish(h, d, motion, orig_raw, nullptr, grad_events, csum, s);
}

int cmax_objective_dist(cmax_handle_t h, const cmax_objective_t *d, const void *motion_v, double *result, void *grad,
                        cmax_stream_t stream) {
    CMAX_REFUSE_WEIGHTED(h, "objective_dist");
    const float *motion = static_cast<const float *>(motion_v);  // double theta[2] when d->motion_dtype == CMAX_F64
    int rc = check_objective_args(h, d, motion);
    if (rc) return rc;
    CMAX_REQUIRE(result, "objective_dist: result");
    rc = kernel_motion(h, d, motion_v, (hipStream_t)stream, &motion);
    if (rc) return rc;
    EvalForm form;
    form.comm = h->comm;
    return objective_eval(h, d, motion, result, grad, (hipStream_t)stream, form);
}

// when K candidates share the launches of one (cmax_objective_batch, cmax_objective_descend_batch): the headline objective on one GPU
static bool batch_fast_applies(const cmax_handle_s *h, const cmax_objective_t *d, int K, const void *grads) {
    return K > 1 && grads && deferred_applies(h, d, grads) && !d->normalized && !h->comm && !h->profiling;
}

// The fast path of cmax_objective_batch, enqueued: K1 and K3 with blockIdx.z = candidate on the batch workspace (grown here), then ONE
// finishing launch of K waves -- k_finish_raw into results / grads (step == nullptr), or k_finish_raw_step_batch, which also applies
// iteration step->it of cmax_objective_descend_batch to every candidate (step->x = motions as double[K][2], step->st the first
// candidate's state, st_stride doubles between candidates) -- and the double-buffer bookkeeping of one evaluation.
static int batch_enqueue(cmax_handle_t h, const cmax_objective_t *d, const float *motions, int K, int64_t mfloats, double *results, double *grads,
                         const DescentArgs *step, int64_t st_stride, hipStream_t s) {
    int rc = 0;
    const int64_t npix = (int64_t)h->Hp * h->Wp;
    const int nr = d->n_ref;
    if (K > h->batch_cap || h->nseg > h->batch_seg_cap) {
        // the four buffers share one layout (batch_cap candidates, batch_seg_cap segments): all of them go, whichever grew
        const int cap = std::max(K, h->batch_cap), scap = std::max(h->nseg, h->batch_seg_cap);
        h->batch_cap = h->batch_seg_cap = 0;  // (a failed allocation below must not leave a later call believing the workspace is there)
        rc = release_all(s, h->bimg, h->braw, h->bwin, h->bshifts);
        if (!rc) rc = h->bimg.reserve(&h->bytes, (int64_t)2 * cap * 4 * npix, s);
        if (!rc) rc = h->braw.reserve(&h->bytes, (int64_t)cap * 4 * kRawStride, s);
        if (!rc) rc = h->bwin.reserve(&h->bytes, (int64_t)cap * 4 * scap, s);
        if (!rc) rc = h->bshifts.reserve(&h->bytes, (int64_t)cap * 4 * scap * kShiftWordsMax, s);
        if (rc) return rc;
        CMAX_CHECK_HIP(hipMemsetAsync(h->bshifts, 0, (size_t)cap * 4 * scap * kShiftWordsMax * sizeof(unsigned), s));
        h->batch_cap = cap;
        h->batch_seg_cap = scap;
        h->batch_zero[0] = h->batch_zero[1] = 0;
    }
    // candidate z, reference time k: image at bimg[buffer][(z * nr + k) * npix]; the launch's images are contiguous
    float *cur = h->bimg + (int64_t)h->batch_cur * h->batch_cap * 4 * npix;
    float *nxt = h->bimg + (int64_t)(h->batch_cur ^ 1) * h->batch_cap * 4 * npix;
    if (h->batch_zero[h->batch_cur] < K * nr) CMAX_CHECK_HIP(hipMemsetAsync(cur, 0, (size_t)K * nr * npix * sizeof(float), s));
    const ObjParams op = obj_params(h, d);
    const EvView ev = ev_view(h);
    const WarpParams wp = warp_params(h, motions, 0, d->ref_mode[0], d->ref_frac[0], d->normalize_t, d->motion_dtype == CMAX_F64);
    RefArgs ra = {};
    ra.win = h->bwin;
    ra.shifts = h->bshifts;
    ra.z_img = (int64_t)nr * npix;
    ra.z_raw = (int64_t)nr * kRawStride;
    ra.z_motion = (int)mfloats;
    fill_ref_times(ra, nr, d->ref_mode, d->ref_frac);
    for (int k = 0; k < nr; ++k) {
        ra.img[k] = cur + k * npix;
        ra.stat[k] = h->braw + (int64_t)k * kRawStride;  // K1's first workgroup of every (candidate, reference time) resets its lines
        ra.zero[k] = nxt + k * npix;                      // K3 clears the other buffer's image of the same (candidate, reference time)
    }
    ra.n_events = h->n;
    launch_vote<CMAX_MODEL_2DOF>(h, ev, wp, ra, nr, s, K);
    CMAX_CHECK_LAUNCH();
    launch_grad<CMAX_MODEL_2DOF>(h, ev, wp, ra, nr, kFoldDeferred, op, h->braw, nullptr, nullptr, false, s, 0, -1, K);
    CMAX_CHECK_LAUNCH();
    if (step)
        hipLaunchKernelGGL(k_finish_raw_step_batch, dim3(K), dim3(64), 0, s, (const double *)h->braw, nr, op, h->d_stat, results, grads, *step, st_stride);
    else
        hipLaunchKernelGGL(k_finish_raw, dim3(K), dim3(64), 0, s, (const double *)h->braw, nr, op, h->d_stat, results, grads,
                           (volatile unsigned long long *)nullptr, 0ull);
    CMAX_CHECK_LAUNCH();
    h->batch_zero[h->batch_cur] = 0;           // holds votes now
    h->batch_zero[h->batch_cur ^ 1] = K * nr;  // K3 cleared the first K * nr images of the other buffer (a larger batch clears it itself)
    h->batch_cur ^= 1;
    return 0;
}

// K candidate motions in ONE launch pair.  The reference's gradient-free paths evaluate the objective for batches of sampled motions
// (src/solver/base.py:738-758 run_optuna; src/solver/patch_contrast_pyramid.py:363-415), and a line search asks for several steps
// along one direction: each evaluation of such a batch alone is two dependent launches and a finishing one, and at cfg2's size those
// launches' floor is 40 % of it (roofline.launch_floor_us).  Here blockIdx.z of K1 / K3 is the candidate -- every candidate its own
// vote image, raw-sum lines and windows -- and the finishing kernel runs one wave per candidate.
// Fast path: 2-DoF, plain image variance (sigma 0, not normalised), default mode, one GPU -- the headline objective.  Everything
// else is evaluated candidate by candidate inside this call (same results, no speed-up).
int cmax_objective_batch(cmax_handle_t h, const cmax_objective_t *d, const void *motions_v, int K, double *results, void *grads,
                         cmax_stream_t stream) {
    const float *motions = static_cast<const float *>(motions_v);
    int rc = check_objective_args(h, d, motions);
    if (rc) return rc;
    CMAX_REQUIRE(results != nullptr && K >= 1 && K <= 64, "objective_batch: results / 1 <= K <= 64");
    hipStream_t s = (hipStream_t)stream;
    const bool two_dof = d->model == CMAX_MODEL_2DOF;
    const GradExtent g = grad_extent(h, d);
    const int64_t mfloats = (two_dof ? 2 : g.count) * (d->motion_dtype == CMAX_F64 ? 2 : 1);  // floats per candidate motion
    if (!batch_fast_applies(h, d, K, grads)) {
        for (int z = 0; z < K; ++z) {
            const float *motion = nullptr;  // (an fp64 flow: every candidate is split in front of its evaluation, stream-ordered in the one scratch)
            rc = kernel_motion(h, d, motions + z * mfloats, s, &motion);
            if (!rc) rc = objective_eval(h, d, motion, results + 8 * z, grads ? (char *)grads + (size_t)z * g.bytes : nullptr, s);
            if (rc) return rc;
        }
        return 0;
    }
    return batch_enqueue(h, d, motions, K, mfloats, results, (double *)grads, nullptr, 0, s);
}

int cmax_objective_has_raw(cmax_handle_t h, const cmax_objective_t *d) {
    if (!h || !d || h->weighted) return 0;  // (the raw form is not carried for per-event weights)
    if (cost_is_focus(d->cost)) return 0;   // (nor offered for the focus losses)
    if (!two_dof_lines(h, d, (const void *)h)) return 0;
    // (a NORMALISED plain variance runs the deferred K3, whose fold needs the un-warped image's statistics from the device)
    return deferred_applies(h, d, (const void *)h) && d->normalized ? 0 : 1;
}

int cmax_objective_raw(cmax_handle_t h, const cmax_objective_t *d, const void *motion_v, double *raw, cmax_stream_t stream) {
    CMAX_REFUSE_WEIGHTED(h, "objective_raw");
    const float *motion = static_cast<const float *>(motion_v);
    int rc = check_objective_args(h, d, motion);
    if (rc) return rc;
    CMAX_REQUIRE(raw, "objective_raw: raw");
    CMAX_REQUIRE(cmax_objective_has_raw(h, d), "objective_raw: this objective has no raw form (see cmax_objective_has_raw)");
    EvalForm form;
    form.raw_out = raw;
    return objective_eval(h, d, motion, nullptr, (void *)raw, (hipStream_t)stream, form);
}

int cmax_finalize_raw_host(cmax_handle_t h, const cmax_objective_t *d, const double *raw_host, double *result_host, double *grad_host) {
    CMAX_REQUIRE(h && d && raw_host && result_host, "finalize_raw_host: null pointer");
    CMAX_REQUIRE(d->n_ref >= 1 && d->n_ref <= 4 && d->model == CMAX_MODEL_2DOF, "finalize_raw_host: descriptor");
    for (int k = 0; k < 8; ++k) result_host[k] = 0.0;
    if (!deferred_applies(h, d, (const void *)h)) {
        // objectives that keep statistics: K3's first workgroup wrote result[8] into doubles 8..15 of the first line, every
        // workgroup added sum dt g into doubles 0, 1 of a line
        for (int k = 0; k < 8; ++k) result_host[k] = raw_host[8 + k];
        if (grad_host) {
            double g0 = 0.0, g1 = 0.0;
            for (int k = 0; k < d->n_ref; ++k)
                for (int l = 0; l < kRawLines; ++l) {
                    g0 += raw_host[(int64_t)k * kRawStride + l * kSubStride];
                    g1 += raw_host[(int64_t)k * kRawStride + l * kSubStride + 1];
                }
            grad_host[0] = g0;
            grad_host[1] = g1;
        }
        return 0;
    }
    CMAX_REQUIRE(!d->normalized, "finalize_raw_host: a normalised plain variance needs the un-warped image's statistics (use cmax_objective_host)");
    const ObjParams op = obj_params(h, d);
    double S[4][6];
    for (int k = 0; k < d->n_ref; ++k)
        for (int q = 0; q < 6; ++q) {
            double a = 0.0;
            for (int l = 0; l < kRawLines; ++l) a += raw_host[(int64_t)k * kRawStride + l * kSubStride + q];
            S[k][q] = a;
        }
    finalize_deferred(op, S, 0.0, result_host, grad_host);
    return 0;
}

// busy-wait for the stream: hipStreamSynchronize sleeps in the driver and wakes up ~10 us late (profiles/r02_solver_objective.txt)
static int spin_until_done(hipStream_t s) {
    hipError_t e;
    while ((e = hipStreamQuery(s)) == hipErrorNotReady) {
    }
    if (e != hipSuccess) {
        set_error("stream error while waiting for the evaluation: %s", hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}

// The wait of the entries whose last kernel stores run counter `seq` into the head of h->hp_out: polled for tens of ms at most, then the
// runtime is asked.  who: the entry and the kernel that should have reported.
static int wait_host_seq(cmax_handle_t h, unsigned long long seq, hipStream_t s, const char *who) {
    unsigned long long seen = 0;
    const int rc = wait_run_counter(cmax_handle_s::hp_counter(h->hp_out), seq, 20000000L, s, &seen);
    if (!rc && seen != seq) {
        set_error("%s did not report (stream finished without its run counter)", who);
        return CMAX_ESTATE;
    }
    return rc;
}

int cmax_objective_host(cmax_handle_t h, const cmax_objective_t *d, const void *motion_v, double *result_host, void *grad_host,
                        cmax_stream_t stream) {
    const float *motion = static_cast<const float *>(motion_v);
    int rc = check_objective_args(h, d, motion);
    if (rc) return rc;
    CMAX_REQUIRE(result_host, "objective_host: result_host");
    hipStream_t s = (hipStream_t)stream;
    rc = kernel_motion(h, d, motion_v, s, &motion);
    if (rc) return rc;
    if (grad_host && two_dof_lines(h, d, grad_host)) {
        // 2-DoF objectives: K1 [-> image kernel] -> K3 -> the one-wave finishing kernel, which writes (loss and) gradient STRAIGHT INTO PINNED HOST
        // MEMORY and then a run counter behind them; the host polls that word.  No copy engine and no driver call between the
        // last kernel and the caller (a 4 KB device-to-host copy of the raw sums + hipStreamQuery polling was 5-6 us slower per
        // evaluation, profiles/r03_ablation.txt 10).
        rc = h->hp_out.reserve(cmax_handle_s::kHpPayload);
        if (rc) return rc;
        double *const hp = h->hp_out, *const hp_dev = h->hp_out.dev();
        EvalForm form;
        form.host_flag = cmax_handle_s::hp_counter(hp_dev);
        form.host_seq = ++h->host_seq;
        for (int k = 0; k < 8; ++k) hp[cmax_handle_s::kHpResult + k] = 0.0;  // (the kernel writes the entries the descriptor uses)
        rc = objective_eval(h, d, motion, hp_dev + cmax_handle_s::kHpResult, hp_dev + cmax_handle_s::kHpStaged, s, form);
        if (!rc) rc = wait_host_seq(h, form.host_seq, s, "objective_host: the finishing kernel");
        if (rc) return rc;
        std::memcpy(result_host, hp + cmax_handle_s::kHpResult, 8 * sizeof(double));
        std::memcpy(grad_host, hp + cmax_handle_s::kHpStaged, 2 * sizeof(double));
        return 0;
    }
    const int64_t gbytes = grad_host ? (int64_t)grad_extent(h, d).bytes : 0;
    rc = h->d_host_grad.reserve(&h->bytes, gbytes, s);
    if (!rc) rc = h->hp_out.reserve(cmax_handle_s::kHpPayload + (gbytes + 7) / 8);
    if (rc) return rc;
    rc = objective_eval(h, d, motion, h->d_host_result, grad_host ? h->d_host_grad.get() : nullptr, s);
    if (rc) return rc;
    double *const hp_result = h->hp_out + cmax_handle_s::kHpResult, *const hp_grad = h->hp_out + cmax_handle_s::kHpPayload;
    CMAX_CHECK_HIP(hipMemcpyAsync(hp_result, h->d_host_result, 8 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (grad_host) CMAX_CHECK_HIP(hipMemcpyAsync(hp_grad, h->d_host_grad, (size_t)gbytes, hipMemcpyDeviceToHost, s));
    rc = spin_until_done(s);
    if (rc) return rc;
    std::memcpy(result_host, hp_result, 8 * sizeof(double));
    if (grad_host) std::memcpy(grad_host, hp_grad, (size_t)gbytes);
    return 0;
}

// The n_iter iterations of ONE trajectory, enqueued: what cmax_objective runs from the device-resident theta, the step riding on the deferred
// path's finishing launch or launched behind the evaluation.  hp_dev (may be null): the device view of the pinned block that receives the
// result and, behind it, the run counter `seq` from the last iteration.
static int descend_one(cmax_handle_t h, const cmax_objective_t *d, const cmax_descent_t *o, double *theta, double *grad, double *result, double *st, bool trace,
                       double *hp_dev, unsigned long long seq, hipStream_t s) {
    static const bool no_fused_step = getenv("CMAX_DESCENT_NO_FUSED_STEP") != nullptr;  // (tools/probe_descent.py: the separate finish + step)
    for (int it = 0; it < o->n_iter; ++it) {
        DescentArgs a = descent_args(*o, it, 2, trace, theta, st);
        if (it == o->n_iter - 1 && hp_dev) {
            a.res_pinned = hp_dev + cmax_handle_s::kHpResult;
            a.flag = cmax_handle_s::hp_counter(hp_dev);
            a.seq = seq;
        }
        bool stepped = false;
        EvalForm form;
        form.step = no_fused_step ? nullptr : &a;
        form.stepped = &stepped;
        int rc = objective_eval(h, d, reinterpret_cast<const float *>(theta), result, grad, s, form);
        if (!rc && !stepped) rc = launch_descent_step(a, result, grad, s);
        if (rc) return rc;
    }
    return 0;
}

// SolverBase.run_torch (src/solver/base.py:840-881) on a 2-DoF fused objective: theta0 once, n_iter x (what cmax_objective runs from the
// device-resident theta -> the step) eagerly on the caller's stream, ONE wait behind the last iteration's run counter, the copies out.
int cmax_objective_descend(cmax_handle_t h, const cmax_objective_t *d, const double *theta0_host, const cmax_descent_t *o, cmax_descent_result_t *res_host,
                           double *x_last_host, double *x_best_host, double *loss_history_host, double *x_trace_host, cmax_stream_t stream) {
    int rc = descent_entry_check("objective_descend", o, h && d && theta0_host && res_host && x_last_host && x_best_host && loss_history_host, d, h && h->comm);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int nx = 2, n_iter = o->n_iter;
    const bool trace = x_trace_host != nullptr;
    constexpr int kHead = 16;  // theta[2] | grad[2] | pad[4] | result[8]
    rc = h->descent.reserve(&h->bytes, kHead + descent_state_doubles(nx, n_iter, trace), s);
    if (!rc) rc = h->hp_out.reserve(cmax_handle_s::kHpPayload);
    if (rc) return rc;
    double *theta = h->descent, *grad = theta + 2, *result = theta + 8, *st = theta + kHead;
    rc = check_objective_args(h, d, reinterpret_cast<const float *>(theta));
    if (rc) return rc;
    const unsigned long long seq = ++h->host_seq;
    double *const theta0_pinned = h->hp_out + cmax_handle_s::kHpStaged;
    theta0_pinned[0] = theta0_host[0];
    theta0_pinned[1] = theta0_host[1];
    CMAX_CHECK_HIP(hipMemcpyAsync(theta, theta0_pinned, 2 * sizeof(double), hipMemcpyHostToDevice, s));
    rc = descend_one(h, d, o, theta, grad, result, st, trace, h->hp_out.dev(), seq, s);
    if (!rc) rc = wait_host_seq(h, seq, s, "objective_descend: the last step");
    if (rc) return rc;
    descent_result(h->hp_out + cmax_handle_s::kHpResult, res_host);
    rc = descent_copy_out(st, true, nx, n_iter, x_best_host, x_last_host, loss_history_host, x_trace_host, s);
    if (rc) return rc;
    CMAX_CHECK_HIP(hipStreamSynchronize(s));
    return 0;
}

// L-BFGS on a 2-DoF fused objective (the rules: include/cmax_hip.h): theta0 once, n_eval x (what cmax_objective runs from the device-resident
// theta, the general sequence -> k_lbfgs_step) eagerly on the caller's stream, ONE wait behind the last step's run counter, the copies out.
// h->lbfgs: theta[2] | grad[2] | pad[4] | result[8] | the L-BFGS state (cmax_lbfgs.h, nx = 2).
int cmax_objective_lbfgs(cmax_handle_t h, const cmax_objective_t *d, const double *theta0_host, const cmax_lbfgs_t *o, cmax_lbfgs_result_t *res_host,
                         double *x_host, double *loss_history_host, double *alpha_host, int32_t *code_host, double *x_trace_host, cmax_stream_t stream) {
    int rc = lbfgs_entry_check("objective_lbfgs", o, h && d && theta0_host && res_host && x_host && loss_history_host && alpha_host && code_host, d, h && h->comm);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int nx = 2, n_eval = o->n_eval, m = o->history;
    const bool trace = x_trace_host != nullptr;
    constexpr int kHead = 16;  // theta[2] | grad[2] | pad[4] | result[8]
    rc = h->lbfgs.reserve(&h->bytes, kHead + lbfgs_state_doubles(nx, m, n_eval, trace), s);
    if (!rc) rc = h->hp_out.reserve(cmax_handle_s::kHpPayload);
    if (rc) return rc;
    double *theta = h->lbfgs, *grad = theta + 2, *result = theta + 8, *st = theta + kHead;
    rc = check_objective_args(h, d, reinterpret_cast<const float *>(theta));
    if (rc) return rc;
    const unsigned long long seq = ++h->host_seq;
    double *const theta0_pinned = h->hp_out + cmax_handle_s::kHpStaged;
    theta0_pinned[0] = theta0_host[0];
    theta0_pinned[1] = theta0_host[1];
    CMAX_CHECK_HIP(hipMemcpyAsync(theta, theta0_pinned, 2 * sizeof(double), hipMemcpyHostToDevice, s));
    for (int e = 0; e < n_eval; ++e) {
        LbfgsArgs a = lbfgs_args(*o, e, nx, trace, theta, st);
        if (e == n_eval - 1) {
            a.res_pinned = h->hp_out.dev() + cmax_handle_s::kHpResult;
            a.flag = cmax_handle_s::hp_counter(h->hp_out.dev());
            a.seq = seq;
        }
        rc = objective_eval(h, d, reinterpret_cast<const float *>(theta), result, grad, s, EvalForm());
        if (!rc) rc = launch_lbfgs_step(a, result, grad, s);
        if (rc) return rc;
    }
    rc = wait_host_seq(h, seq, s, "objective_lbfgs: the last step");
    if (rc) return rc;
    lbfgs_result(h->hp_out + cmax_handle_s::kHpResult, res_host);
    rc = lbfgs_copy_out(st, nx, m, n_eval, x_host, loss_history_host, alpha_host, code_host, x_trace_host, s);
    if (rc) return rc;
    CMAX_CHECK_HIP(hipStreamSynchronize(s));
    return 0;
}

// K independent trajectories of cmax_objective_descend in one call (multi-start: the 2-DoF objective is not convex, and the reference's
// "global-best" grid, src/solver/patch_contrast_base.py:164-187, is correct only to its spacing).  Where cmax_objective_batch's fast path
// applies, an iteration of ALL K candidates is K1 -> K3 (blockIdx.z = candidate) -> one finishing launch of K waves that also steps every
// candidate on its own state; everything else, and K = 1, runs candidate by candidate as cmax_objective_descend does.  ONE wait: the copy of
// all states to pinned memory behind the last launch.
// h->descent_batch: theta[K][2] | grad[K][2] | pad[K][4] | result[K][8] | K descent states (cmax_descent.h, nx = 2).
int cmax_objective_descend_batch(cmax_handle_t h, const cmax_objective_t *d, const double *theta0_host, int K, const cmax_descent_t *o,
                                 cmax_descent_result_t *res_host, double *x_last_host, double *x_best_host, double *loss_history_host,
                                 double *x_trace_host, cmax_stream_t stream) {
    CMAX_REQUIRE(K >= 1 && K <= CMAX_DESCENT_MAX_STARTS, "objective_descend_batch: 1 <= K <= 64 starts per call");
    int rc = descent_entry_check("objective_descend_batch", o, h && d && theta0_host && res_host && x_last_host && x_best_host && loss_history_host, d, h && h->comm);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int nx = 2, n_iter = o->n_iter;
    const bool trace = x_trace_host != nullptr;
    constexpr int kHead = 16;  // per candidate: theta[2], grad[2], pad[4], result[8]
    const int64_t S = descent_state_doubles(nx, n_iter, trace);
    rc = h->descent_batch.reserve(&h->bytes, (int64_t)K * (kHead + S), s);
    if (!rc) rc = h->hp_out.reserve(cmax_handle_s::kHpPayload + (int64_t)K * S);
    if (rc) return rc;
    double *theta = h->descent_batch, *grad = theta + 2 * K, *result = theta + 8 * K, *st = theta + (int64_t)kHead * K;
    rc = check_objective_args(h, d, reinterpret_cast<const float *>(theta));
    if (rc) return rc;
    double *const staged = h->hp_out + cmax_handle_s::kHpPayload;  // (theta0[K] goes out of it, the K states come back into it)
    std::memcpy(staged, theta0_host, (size_t)K * 2 * sizeof(double));
    CMAX_CHECK_HIP(hipMemcpyAsync(theta, staged, (size_t)K * 2 * sizeof(double), hipMemcpyHostToDevice, s));
    if (batch_fast_applies(h, d, K, grad)) {
        for (int it = 0; it < n_iter; ++it) {
            const DescentArgs a = descent_args(*o, it, nx, trace, theta, st);
            rc = batch_enqueue(h, d, reinterpret_cast<const float *>(theta), K, 4, result, grad, &a, S, s);
            if (rc) return rc;
        }
    } else {
        for (int z = 0; z < K; ++z) {
            rc = descend_one(h, d, o, theta + 2 * z, grad + 2 * z, result + 8 * z, st + z * S, trace, nullptr, 0, s);
            if (rc) return rc;
        }
    }
    CMAX_CHECK_HIP(hipMemcpyAsync(staged, st, (size_t)(K * S) * sizeof(double), hipMemcpyDeviceToHost, s));
    CMAX_CHECK_HIP(hipStreamSynchronize(s));
    for (int z = 0; z < K; ++z) {
        descent_result_of_state(staged + z * S, &res_host[z]);
        (void)descent_copy_out(staged + z * S, false, nx, n_iter, x_best_host + (int64_t)z * nx, x_last_host + (int64_t)z * nx, loss_history_host + (int64_t)z * n_iter,
                               trace ? x_trace_host + (int64_t)z * (n_iter + 1) * nx : nullptr, s);
    }
    return 0;
}

int cmax_set_deterministic(cmax_handle_t h, int enable) {
    CMAX_REQUIRE(h != nullptr, "set_deterministic: handle");
    if (enable) CMAX_REFUSE_WEIGHTED(h, "set_deterministic");
    if (enable) {  // each buffer on its own: a failed allocation must not leave a later call believing everything is there
        const int64_t npix = (int64_t)h->Hp * h->Wp;
        bool fresh = false;
        int rc = h->img64.reserve(&h->bytes, 5 * npix, nullptr, &fresh);
        if (rc) return rc;
        if (fresh && hipMemset(h->img64, 0, (size_t)5 * npix * sizeof(long long)) != hipSuccess) {
            h->img64.release();
            set_error("set_deterministic: clearing the integer images failed");
            return CMAX_ENOMEM;
        }
        rc = h->d_imax.reserve(&h->bytes, 8, nullptr);  // [0..4]: images of the objective; HVP: [0..3] max |G_k|, [4..7] max |G'_k|
        if (!rc) rc = h->d_det_inv_scale.reserve(&h->bytes, 4, nullptr);
        if (rc) return rc;
    }
    h->deterministic = enable != 0;
    h->win_generation = ~(uint64_t)0;  // windows published by the other mode's K1 stay valid, but keep the state simple
    return 0;
}

int cmax_get_deterministic(cmax_handle_t h, int *enabled) {
    CMAX_REQUIRE(h != nullptr && enabled != nullptr, "get_deterministic");
    *enabled = h->deterministic ? 1 : 0;
    return 0;
}

int cmax_comm_set_c2_bands(cmax_handle_t h, int bands) {
    CMAX_REQUIRE(h != nullptr && bands >= 1 && bands <= 64, "comm_set_c2_bands: bands must be in 1..64");
    h->c2_bands = bands;
    return 0;
}

int cmax_comm_available(char *path_host, int path_capacity) { return comm_available(path_host, path_capacity); }

int cmax_comm_unique_id(void *id_host) {
    CMAX_REQUIRE(id_host != nullptr, "comm_unique_id: id_host");
    return comm_unique_id(id_host);
}

int cmax_comm_init(cmax_handle_t h, const void *id_host, int nranks, int rank) {
    CMAX_REFUSE_WEIGHTED(h, "comm_init");
    CMAX_REQUIRE(h != nullptr, "comm_init: handle");
    CMAX_REQUIRE(nranks >= 1 && rank >= 0 && rank < nranks, "comm_init: need 0 <= rank < nranks");
    if (h->comm) {
        comm_destroy(h->comm);
        h->comm = nullptr;
    }
    if (nranks == 1 && !id_host) return 0;  // a single slice is the whole batch: no communicator, RCCL is never loaded
    CMAX_REQUIRE(id_host != nullptr, "comm_init: id_host");
    int dev = -1;
    CMAX_CHECK_HIP(hipGetDevice(&dev));
    if (dev != h->device) {
        set_error("comm_init: the current HIP device is %d but the handle lives on device %d", dev, h->device);
        return CMAX_ESTATE;
    }
    return comm_create(id_host, nranks, rank, &h->comm);
}

int cmax_comm_destroy(cmax_handle_t h) {
    CMAX_REQUIRE(h != nullptr, "comm_destroy: handle");
    comm_destroy(h->comm);
    h->comm = nullptr;
    return 0;
}

int cmax_comm_info(cmax_handle_t h, int *nranks, int *rank, int *rccl_version) {
    CMAX_REQUIRE(h != nullptr, "comm_info: handle");
    if (nranks) *nranks = comm_nranks(h->comm);
    if (rank) *rank = comm_rank(h->comm);
    if (rccl_version) *rccl_version = h->comm ? comm_version() : 0;
    return 0;
}

int cmax_comm_allreduce(cmax_handle_t h, void *buf, int64_t count, int dtype, int op, cmax_stream_t stream) {
    CMAX_REQUIRE(h != nullptr && (buf != nullptr || count == 0) && count >= 0, "comm_allreduce: handle / buffer");
    CMAX_REQUIRE(dtype == CMAX_F32 || dtype == CMAX_F64, "comm_allreduce: dtype");
    CMAX_REQUIRE(op >= 0 && op <= 2, "comm_allreduce: op must be 0 (sum), 1 (min) or 2 (max)");
    ProfScope prof(h, kProfComm, (hipStream_t)stream);
    return comm_allreduce(h->comm, buf, (size_t)count, dtype == CMAX_F64 ? kCommF64 : kCommF32,
                          op == 1 ? kCommMin : (op == 2 ? kCommMax : kCommSum), (hipStream_t)stream);
}

}  // extern "C"

namespace cmax {

// scratch of the second-order path and of the IWE layer: [6][4] images, the tangent statistics (k_vote_tan's first workgroup clears them) and Gt
static int tangent_scratch(cmax_handle_s *h, hipStream_t s) {
    const int64_t npix = (int64_t)h->Hp * h->Wp;
    int rc = h->hvp_img.reserve(&h->bytes, 6 * 4 * npix, s);
    if (!rc) rc = h->d_stat_tan.reserve(&h->bytes, 4 * kStatStride, s);
    if (!rc) rc = h->Gt.reserve(&h->bytes, 4 * npix, s);  // (cmax_create's holds one image)
    return rc;
}

// derivative votes are bounded by 2 |dt|_max (the tangent has unit max-norm): fixed-point scale per reference time
static TanParams tangent_params(const cmax_handle_s *h, const cmax_objective_t *d, const float *tangent) {
    const double period = d->normalize_t ? 1.0 : (h->tmax_host - h->tmin_host);
    TanParams tp = {};
    tp.u = tangent;
    tp.bs = (int64_t)h->Hp * h->Wp;
    for (int k = 0; k < d->n_ref; ++k) {
        const double dref = ref_fraction(d->ref_mode[k], d->ref_frac[k]);
        double dtmax = fabs(dref) > fabs(1.0 - dref) ? fabs(dref) : fabs(1.0 - dref);
        dtmax *= period > 0 ? period : 1.0;
        if (dtmax < 1e-30) dtmax = 1e-30;
        tp.d[k] = (float)dref;
        tp.d_lo[k] = ref_fraction_lo(d->ref_mode[k], d->ref_frac[k]);
        tp.fixk[k] = (float)(1073741824.0 / ((double)h->seg_max * 2.0 * dtmax));  // 2^30 / (events * max |derivative vote|)
    }
    tp.fix = tp.fixk[0];
    tp.inv_fix = 1.f / tp.fix;
    return tp;
}

}  // namespace cmax

extern "C" {

// T3 against the images G (current) and Gp (tangent) into `out` (zeroed by the caller): 2-DoF partials folded by k_finish, flow models
// added per event; in deterministic mode both accumulate the integers of `det` and launch_finish_det rounds them once
static int second_order_gather(cmax_handle_s *h, const cmax_objective_t *d, const EvView &ev, const WarpParams &wp, const TanParams &tp, const float *G,
                               const float *Gp, void *out, const HvpDet &det, hipStream_t s) {
    const bool two_dof = d->model == CMAX_MODEL_2DOF;
    with_model(d->model, [&](auto m) { launch_grad_hvp<m.value>(h, ev, wp, tp, d->n_ref, G, Gp, two_dof ? h->d_gpart : nullptr, two_dof ? nullptr : (float *)out, s, det); });
    CMAX_CHECK_LAUNCH();
    if (h->deterministic) return launch_finish_det(h, d, out, s);
    if (two_dof) {
        hipLaunchKernelGGL(k_finish, dim3(1), dim3(256), 0, s, h->d_gpart, d->n_ref * h->nseg, (double *)out);
        CMAX_CHECK_LAUNCH();
    }
    return 0;
}

// comm: the handle holds a time slice of the batch -- the images and the tangent images are all-reduced (ONE grouped call: both are
// sums over events), everything in image space runs redundantly on every rank, the second-order gather covers this rank's events;
// reduce_hv: ... and the product is all-reduced too (cmax_objective_hvp_dist); the patch plan reduces its 2 n_patch numbers instead
static int objective_hvp_impl(cmax_handle_t h, const cmax_objective_t *d, const float *motion, const float *tangent, void *hv, hipStream_t s,
                              cmax::Comm *comm, bool reduce_hv) {
    int rc = 0;
    const bool dist = comm != nullptr;
    const int Hp = h->Hp, Wp = h->Wp;
    const int64_t npix = (int64_t)Hp * Wp;
    const bool two_dof = d->model == CMAX_MODEL_2DOF;
    const GradExtent g = grad_extent(h, d);
    CMAX_CHECK_HIP(hipMemsetAsync(hv, 0, g.bytes, s));
    if (h->n == 0 && !dist) return 0;
    rc = tangent_scratch(h, s);
    if (rc) return rc;
    // [6 kinds][4 reference times][npix]: every kernel of the chain covers all reference times in one launch
    // (blockIdx.y, element stride npix)
    const int64_t bs = npix;
    float *I = h->hvp_img, *Ib = I + 4 * npix, *dI = I + 8 * npix, *dIb = I + 12 * npix, *Gp = I + 16 * npix, *Gpt = I + 20 * npix;
    const int nr = d->n_ref;

    const ObjParams op = obj_params(h, d);
    const int nsub = op.nsub;

    // statistics of the un-warped image (slot 4), cached per batch like in cmax_objective
    if (d->normalized && !orig_cache_hit(h, d)) {
        rc = vote_image(h, -1, nullptr, 0, CMAX_REF_FIRST, 0.0, 1, I, false, 4, s);
        if (rc) return rc;
        if (dist) {
            ProfScope prof(h, kProfComm, s);
            rc = comm_allreduce(comm, I, (size_t)npix, kCommF32, kCommSum, s);
            if (rc) return rc;
        }
        rc = orig_image_stats(h, d, I, Ib, nullptr, s);
        if (rc) return rc;
    }

    const EvView ev = ev_view(h);
    double k0 = 0, k1 = 0;
    if (d->sigma > 0) blur_taps(d->sigma, k0, k1);
    const dim3 igrid(div_up(npix, 256), nr), sgrid(stat_blocks(h), nr);
    const TanParams tp = tangent_params(h, d, tangent);
    const WarpParams wp = warp_params(h, motion, d->T, d->ref_mode[0], d->ref_frac[0], d->normalize_t, d->motion_dtype == CMAX_F64);
    // images, their blur and statistics (slots 0 .. nr-1)
    CMAX_CHECK_HIP(hipMemsetAsync(I, 0, (size_t)nr * npix * sizeof(float), s));
    {
        float *imgs[4];
        for (int k = 0; k < nr; ++k) imgs[k] = I + k * npix;
        rc = vote_images(h, d->model, motion, d->T, nr, d->ref_mode, d->ref_frac, d->normalize_t, imgs, 0xFu, 0, s);
        if (rc) return rc;
    }
    // T1: tangent images (their blur follows below)
    CMAX_CHECK_HIP(hipMemsetAsync(dI, 0, (size_t)nr * npix * sizeof(float), s));
    // deterministic mode (round 3): the tangent votes go to the integer images (all zero between uses) and are rounded to fp32
    // once; the second-order gather below accumulates integers -- the product is then bit-identical from run to run like the
    // loss and the gradient
    const bool det = h->deterministic;
    long long *dI64 = det ? h->img64 : nullptr;
    if (h->n > 0) with_model(d->model, [&](auto m) { launch_vote_tan<m.value>(h, ev, wp, tp, nr, dI, s, dI64); });
    CMAX_CHECK_LAUNCH();
    if (det && h->n > 0) {
        FixedArgs fa = {};
        for (int k = 0; k < nr; ++k) {
            fa.src[k] = h->img64 + (int64_t)k * npix;
            fa.dst[k] = dI + k * npix;
            fa.inv_fixk[k] = 1.0 / (double)tp.fixk[k];
        }
        hipLaunchKernelGGL(k_fixed_to_image, dim3(stream_grid(npix, 256), nr), dim3(256), 0, s, fa, npix);
        CMAX_CHECK_LAUNCH();
    }
    if (dist) {  // C1 of the product: images and tangent images of all reference times, one grouped call
        ProfScope prof(h, kProfComm, s);
        void *bufs[2] = {I, dI};
        const size_t counts[2] = {(size_t)nr * npix, (size_t)nr * npix};
        const CommType types[2] = {kCommF32, kCommF32};
        rc = comm_allreduce_group(comm, bufs, counts, types, 2, kCommSum, s);
        if (rc) return rc;
    }
    if (h->n == 0) {  // this rank holds no events of the batch: nothing to gather, but it takes part in every exchange
        if (dist && reduce_hv) {
            ProfScope prof(h, kProfComm, s);
            rc = comm_allreduce(comm, hv, (size_t)g.count, g.type, kCommSum, s);
        }
        return rc;
    }
    const float *img = I, *dimg = dI;
    if (d->sigma > 0) {
        hipLaunchKernelGGL(k_blur3<float>, igrid, dim3(256), 0, s, I, Hp, Wp, (float)k0, (float)k1, Ib, bs);
        img = Ib;
    }
    with_cost(d->cost, [&](auto c) {
        hipLaunchKernelGGL(k_stats<c.value>, sgrid, dim3(256), 0, s, img, Hp, Wp, d->omit_boundary, nsub, h->d_stat, (float *)nullptr, (float4 *)nullptr, (int64_t)0, bs);
    });
    CMAX_CHECK_LAUNCH();
    // (the tangent images were voted above, next to the images)
    if (d->sigma > 0) {
        hipLaunchKernelGGL(k_blur3<float>, igrid, dim3(256), 0, s, dI, Hp, Wp, (float)k0, (float)k1, dIb, bs);
        dimg = dIb;
    }
    // T2: tangent statistics, G (current) and G' (tangent), blur transposes
    float *Gk = d->sigma > 0 ? h->Gt : h->G, *Gpk = d->sigma > 0 ? Gpt : Gp;
    with_cost(d->cost, [&](auto c) {
        hipLaunchKernelGGL(k_stats_tan<c.value>, sgrid, dim3(256), 0, s, img, dimg, Hp, Wp, d->omit_boundary, nsub, h->d_stat_tan, bs);
        hipLaunchKernelGGL(k_gimage<c.value>, igrid, dim3(256), 0, s, img, op, 0, h->d_stat, Gk, bs);
        hipLaunchKernelGGL(k_gimage_tan<c.value>, igrid, dim3(256), 0, s, img, dimg, op, 0, h->d_stat, h->d_stat_tan, Gpk, bs);
    });
    if (d->sigma > 0) {
        hipLaunchKernelGGL(k_blur3_adj<float>, igrid, dim3(256), 0, s, h->Gt, Hp, Wp, (float)k0, (float)k1, h->G, bs);
        hipLaunchKernelGGL(k_blur3_adj<float>, igrid, dim3(256), 0, s, Gpt, Hp, Wp, (float)k0, (float)k1, Gp, bs);
    }
    CMAX_CHECK_LAUNCH();
    // T3
    HvpDet hd = {};
    if (det) {
        // the bounds the fixed-point scale is derived from: max |G_k| and max |G'_k| (integer maxima: order-free)
        CMAX_CHECK_HIP(hipMemsetAsync(h->d_imax, 0, 8 * sizeof(unsigned), s));
        ImgArgs ig = {}, ip = {};
        for (int k = 0; k < nr; ++k) {
            ig.in[k] = h->G + k * npix;
            ip.in[k] = Gp + k * npix;
        }
        const dim3 mgrid(std::min(stream_grid(npix, 1024), 256), nr);
        hipLaunchKernelGGL(k_image_absmax, mgrid, dim3(256), 0, s, ig, npix, 0, h->d_imax);
        hipLaunchKernelGGL(k_image_absmax, mgrid, dim3(256), 0, s, ip, npix, 4, h->d_imax);
        CMAX_CHECK_LAUNCH();
        if (!two_dof) {
            rc = reserve_g64(h, g.count, s);
            if (rc) return rc;
        }
        hd.g64 = two_dof ? reinterpret_cast<long long *>(h->d_gpart.get()) : h->g64;  // (d_gpart: [4][nseg][2] doubles = as many 64-bit integers)
        hd.imax = h->d_imax;
        hd.inv_scale = h->d_det_inv_scale;
        hd.n_events = h->n;
        hd.n_ref = nr;
    }
    rc = second_order_gather(h, d, ev, wp, tp, h->G, Gp, hv, hd, s);
    if (rc) return rc;
    if (dist && reduce_hv) {
        ProfScope prof(h, kProfComm, s);
        rc = comm_allreduce(comm, hv, (size_t)g.count, g.type, kCommSum, s);
        if (rc) return rc;
    }
    return 0;
}

int cmax_objective_hvp(cmax_handle_t h, const cmax_objective_t *d, const void *motion_v, const float *tangent, void *hv,
                       cmax_stream_t stream) {
    CMAX_REFUSE_WEIGHTED(h, "objective_hvp");
    const float *motion = static_cast<const float *>(motion_v);  // double theta[2] when d->motion_dtype == CMAX_F64
    int rc = check_objective_args(h, d, motion);
    if (rc) return rc;
    CMAX_REQUIRE(tangent && hv, "objective_hvp: tangent / hv");
    rc = kernel_motion(h, d, motion_v, (hipStream_t)stream, &motion);
    if (rc) return rc;
    return objective_hvp_impl(h, d, motion, tangent, hv, (hipStream_t)stream, nullptr, false);
}

int cmax_objective_hvp_dist(cmax_handle_t h, const cmax_objective_t *d, const void *motion_v, const float *tangent, void *hv,
                            cmax_stream_t stream) {
    CMAX_REFUSE_WEIGHTED(h, "objective_hvp_dist");
    const float *motion = static_cast<const float *>(motion_v);
    int rc = check_objective_args(h, d, motion);
    if (rc) return rc;
    CMAX_REQUIRE(tangent && hv, "objective_hvp_dist: tangent / hv");
    rc = kernel_motion(h, d, motion_v, (hipStream_t)stream, &motion);
    if (rc) return rc;
    return objective_hvp_impl(h, d, motion, tangent, hv, (hipStream_t)stream, h->comm, true);
}

}  // extern "C"

// ---- the image of warped events as a differentiable layer (cmax_iwes, _vjp, _jvp, _vjp_tan) --------------------------------------------
namespace cmax {

// the part of an objective descriptor the event side reads (argument checks, warp parameters, windows)
static cmax_objective_t iwes_as_objective(const cmax_iwes_t *d) {
    cmax_objective_t o = {};
    o.model = d->model;
    o.cost = CMAX_COST_VARIANCE;
    o.normalize_t = d->normalize_t;
    o.n_ref = d->n_ref;
    for (int k = 0; k < 4; ++k) {
        o.ref_mode[k] = d->ref_mode[k];
        o.ref_frac[k] = d->ref_frac[k];
        o.mult[k] = 1.0;
    }
    o.sigma = d->sigma;
    o.T = d->T;
    o.motion_dtype = d->motion_dtype;
    return o;
}

static int iwes_check(cmax_handle_t h, const cmax_iwes_t *d, const void *motion, const char *what, cmax_objective_t *o) {
    CMAX_REQUIRE(h && d && motion, "iwes: null pointer");
    CMAX_REQUIRE(d->n_ref >= 1 && d->n_ref <= 4, "iwes: n_ref");
    *o = iwes_as_objective(d);
    int rc = check_objective_args(h, o, static_cast<const float *>(motion));
    if (rc) return rc;
    return refuse_det_or_comm(h, what);
}

// the caller's n planes as the event kernels read them: the planes themselves, or their blur transpose in `stage`
static int iwes_stage(cmax_handle_s *h, double sigma, const float *planes, int n, float *stage, const float **out, hipStream_t s) {
    *out = planes;
    if (!(sigma > 0)) return 0;
    const int64_t npix = (int64_t)h->Hp * h->Wp;
    double k0 = 0, k1 = 0;
    blur_taps(sigma, k0, k1);
    hipLaunchKernelGGL(k_blur3_adj<float>, dim3(div_up(npix, 256), n), dim3(256), 0, s, planes, h->Hp, h->Wp, (float)k0, (float)k1, stage, npix);
    CMAX_CHECK_LAUNCH();
    *out = stage;
    return 0;
}

// T3 with the caller's images (out zeroed by the caller)
static int iwes_gather(cmax_handle_s *h, const cmax_objective_t *d, const float *motion, const float *tangent, const float *G, const float *Gp, void *out,
                       hipStream_t s) {
    const WarpParams wp = warp_params(h, motion, d->T, d->ref_mode[0], d->ref_frac[0], d->normalize_t, d->motion_dtype == CMAX_F64);
    return second_order_gather(h, d, ev_view(h), wp, tangent_params(h, d, tangent), G, Gp, out, HvpDet{}, s);
}

// grad_w (zeroed by the caller) from finished planes G[0 .. n_ref) (+ G[n_ref] at the un-warped positions): per_event_finish's gather and
// scatter, behind windows published for THIS motion
static int iwes_weight_grad(cmax_handle_s *h, const cmax_objective_t *d, const float *motion, const float *G, bool with_orig, float *grad_w, hipStream_t s) {
    const int64_t npix = (int64_t)h->Hp * h->Wp;
    const int nr = d->n_ref, n_planes = nr + (with_orig ? 1 : 0);
    int rc = reserve_packed_planes(h, h->gw_packed, &h->gw_plane, 5, n_planes, s);
    if (rc) return rc;
    const EvView ev = ev_view(h);
    rc = publish_windows(h, d, motion, s);
    if (rc) return rc;
    h->win_generation = ~(uint64_t)0;
    {
        RefArgs ra = {};
        fill_ref_times(ra, nr, d->ref_mode, d->ref_frac);
        for (int k = 0; k < nr; ++k) ra.img[k] = const_cast<float *>(G) + k * npix;  // (read only by the gather)
        ra.win = h->d_win;
        ra.shifts = h->d_shifts;
        const WarpParams wp = warp_params(h, motion, d->T, d->ref_mode[0], d->ref_frac[0], d->normalize_t, d->motion_dtype == CMAX_F64);
        with_model(d->model, [&](auto m) { launch_weight_gather<m.value>(h, ev, wp, ra, nr, 0, s); });
        CMAX_CHECK_LAUNCH();
    }
    if (with_orig) {
        rc = gather_unwarped(h, G + nr * npix, s,
                             [&](const EvView &ev, const WarpParams &wp, const RefArgs &ra) { launch_weight_gather<-1>(h, ev, wp, ra, 1, nr, s); });
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_weight_grad_scatter, dim3(div_up(h->n, 256)), dim3(256), 0, s, (const float *)h->gw_packed, h->gw_plane, n_planes, (const int *)h->src, h->n, grad_w);
    CMAX_CHECK_LAUNCH();
    return 0;
}

}  // namespace cmax

extern "C" {

int cmax_sizeof_iwes(void) { return (int)sizeof(cmax_iwes_t); }

int cmax_iwes(cmax_handle_t h, const cmax_iwes_t *d, const void *motion_v, float *images, cmax_stream_t stream) {
    cmax_objective_t o;
    int rc = iwes_check(h, d, motion_v, "iwes", &o);
    if (rc) return rc;
    CMAX_REQUIRE(images != nullptr, "iwes: images");
    hipStream_t s = (hipStream_t)stream;
    const float *motion = nullptr;
    rc = kernel_motion(h, &o, motion_v, s, &motion);
    if (rc) return rc;
    const int64_t npix = (int64_t)h->Hp * h->Wp;
    const int nr = o.n_ref, n_img = nr + (d->with_orig ? 1 : 0);
    if (h->n == 0) {
        CMAX_CHECK_HIP(hipMemsetAsync(images, 0, (size_t)n_img * npix * sizeof(float), s));
        return 0;
    }
    float *raw = images;
    if (o.sigma > 0) {  // votes into the scratch (five consecutive images), the blur writes the caller's buffer
        rc = tangent_scratch(h, s);
        if (rc) return rc;
        raw = h->hvp_img;
    }
    float *imgs[4];
    for (int k = 0; k < nr; ++k) imgs[k] = raw + k * npix;
    rc = vote_images(h, o.model, motion, o.T, nr, o.ref_mode, o.ref_frac, o.normalize_t, imgs, 0u, -1, s, {}, o.motion_dtype == CMAX_F64);
    if (rc) return rc;
    if (d->with_orig) {
        rc = vote_image(h, -1, nullptr, 0, CMAX_REF_FIRST, 0.0, 1, raw + nr * npix, false, -1, s);
        if (rc) return rc;
    }
    if (o.sigma > 0) {
        double k0 = 0, k1 = 0;
        blur_taps(o.sigma, k0, k1);
        hipLaunchKernelGGL(k_blur3<float>, dim3(div_up(npix, 256), n_img), dim3(256), 0, s, (const float *)raw, h->Hp, h->Wp, (float)k0, (float)k1, images, npix);
        CMAX_CHECK_LAUNCH();
    }
    return 0;
}

int cmax_iwes_vjp(cmax_handle_t h, const cmax_iwes_t *d, const void *motion_v, const float *gimages, void *grad_motion, float *grad_w, int64_t n,
                  cmax_stream_t stream) {
    cmax_objective_t o;
    int rc = iwes_check(h, d, motion_v, "iwes_vjp", &o);
    if (rc) return rc;
    CMAX_REQUIRE(gimages && grad_motion, "iwes_vjp: gimages / grad_motion");
    CMAX_REQUIRE(!grad_w || n == h->n_in, "iwes_vjp: n must equal the n of the last cmax_set_events (one derivative per event, in the caller's order)");
    hipStream_t s = (hipStream_t)stream;
    const float *motion = nullptr;
    rc = kernel_motion(h, &o, motion_v, s, &motion);
    if (rc) return rc;
    const int64_t npix = (int64_t)h->Hp * h->Wp;
    const GradExtent g = grad_extent(h, &o);
    CMAX_CHECK_HIP(hipMemsetAsync(grad_motion, 0, g.bytes, s));
    if (grad_w && n > 0) CMAX_CHECK_HIP(hipMemsetAsync(grad_w, 0, (size_t)n * sizeof(float), s));
    if (h->n == 0) return 0;
    rc = tangent_scratch(h, s);
    if (rc) return rc;
    bool fresh = false;  // the zero tangent (once per motion size)
    rc = h->iw_zero.reserve(&h->bytes, g.count, s, &fresh);
    if (rc) return rc;
    if (fresh) CMAX_CHECK_HIP(hipMemset(h->iw_zero, 0, (size_t)g.count * sizeof(float)));
    const int n_planes = o.n_ref + ((d->with_orig && grad_w) ? 1 : 0);
    const float *G = nullptr;
    rc = iwes_stage(h, o.sigma, gimages, n_planes, h->hvp_img + 16 * npix, &G, s);
    if (rc) return rc;
    // J^T G = T3 with u = 0 (no mixed term) and G' = G
    rc = iwes_gather(h, &o, motion, h->iw_zero, G, G, grad_motion, s);
    if (rc || !grad_w) return rc;
    return iwes_weight_grad(h, &o, motion, G, d->with_orig != 0, grad_w, s);
}

int cmax_iwes_jvp(cmax_handle_t h, const cmax_iwes_t *d, const void *motion_v, const float *tangent, float *dimages, cmax_stream_t stream) {
    cmax_objective_t o;
    int rc = iwes_check(h, d, motion_v, "iwes_jvp", &o);
    if (rc) return rc;
    CMAX_REQUIRE(tangent && dimages, "iwes_jvp: tangent / dimages");
    hipStream_t s = (hipStream_t)stream;
    const float *motion = nullptr;
    rc = kernel_motion(h, &o, motion_v, s, &motion);
    if (rc) return rc;
    const int64_t npix = (int64_t)h->Hp * h->Wp;
    const int nr = o.n_ref;
    if (h->n == 0) {
        CMAX_CHECK_HIP(hipMemsetAsync(dimages, 0, (size_t)nr * npix * sizeof(float), s));
        return 0;
    }
    rc = tangent_scratch(h, s);
    if (rc) return rc;
    float *draw = o.sigma > 0 ? h->hvp_img + 8 * npix : dimages;
    CMAX_CHECK_HIP(hipMemsetAsync(draw, 0, (size_t)nr * npix * sizeof(float), s));
    const EvView ev = ev_view(h);
    const TanParams tp = tangent_params(h, &o, tangent);
    const WarpParams wp = warp_params(h, motion, o.T, o.ref_mode[0], o.ref_frac[0], o.normalize_t, o.motion_dtype == CMAX_F64);
    with_model(o.model, [&](auto m) { launch_vote_tan<m.value>(h, ev, wp, tp, nr, draw, s); });
    CMAX_CHECK_LAUNCH();
    if (o.sigma > 0) {
        double k0 = 0, k1 = 0;
        blur_taps(o.sigma, k0, k1);
        hipLaunchKernelGGL(k_blur3<float>, dim3(div_up(npix, 256), nr), dim3(256), 0, s, (const float *)draw, h->Hp, h->Wp, (float)k0, (float)k1, dimages, npix);
        CMAX_CHECK_LAUNCH();
    }
    return 0;
}

int cmax_iwes_vjp_tan(cmax_handle_t h, const cmax_iwes_t *d, const void *motion_v, const float *tangent, const float *gimages, const float *gimages_tan,
                      void *out, cmax_stream_t stream) {
    cmax_objective_t o;
    int rc = iwes_check(h, d, motion_v, "iwes_vjp_tan", &o);
    if (rc) return rc;
    CMAX_REQUIRE(tangent && gimages && gimages_tan && out, "iwes_vjp_tan: tangent / gimages / gimages_tan / out");
    hipStream_t s = (hipStream_t)stream;
    const float *motion = nullptr;
    rc = kernel_motion(h, &o, motion_v, s, &motion);
    if (rc) return rc;
    const int64_t npix = (int64_t)h->Hp * h->Wp;
    const GradExtent g = grad_extent(h, &o);
    CMAX_CHECK_HIP(hipMemsetAsync(out, 0, g.bytes, s));
    if (h->n == 0) return 0;
    rc = tangent_scratch(h, s);
    if (rc) return rc;
    const float *G = nullptr, *Gp = nullptr;
    rc = iwes_stage(h, o.sigma, gimages, o.n_ref, h->hvp_img, &G, s);
    if (!rc) rc = iwes_stage(h, o.sigma, gimages_tan, o.n_ref, h->hvp_img + 4 * npix, &Gp, s);
    if (rc) return rc;
    return iwes_gather(h, &o, motion, tangent, G, Gp, out, s);
}

}  // extern "C"

// library-internal (cmax_solver.hip): the evaluation / the product of a time-sliced batch with the motion gradient LEFT AS THIS
// RANK'S SHARE -- the patch plan carries it through the (linear) adjoints of the voxel chain and of the patch interpolation and
// all-reduces 2 n_patch numbers instead of 2 H W [T]
namespace cmax {
#ifdef CMAX_TIMELINE
int image_timeline_set(unsigned long long *buffer) { return timeline_set(buffer); }
#endif
bool handle_has_comm(cmax_handle_t h) { return h && h->comm != nullptr; }
int objective_dist_local_grad(cmax_handle_t h, const cmax_objective_t *d, const float *motion, double *result, void *grad, hipStream_t s) {
    CMAX_REFUSE_WEIGHTED(h, "patch plan evaluation");
    int rc = check_objective_args(h, d, motion);
    if (rc) return rc;
    EvalForm form;
    form.comm = h->comm;
    form.skip_c2 = true;
    return objective_eval(h, d, motion, result, grad, s, form);
}
int objective_hvp_dist_local(cmax_handle_t h, const cmax_objective_t *d, const float *motion, const float *tangent, void *hv, hipStream_t s) {
    CMAX_REFUSE_WEIGHTED(h, "patch plan product");
    int rc = check_objective_args(h, d, motion);
    if (rc) return rc;
    return objective_hvp_impl(h, d, motion, tangent, hv, s, h->comm, false);
}
int objective_presplit(cmax_handle_t h, const cmax_objective_t *d, const float *motion, double *result, void *grad, hipStream_t s) {
    int rc = check_objective_args(h, d, motion);
    if (rc) return rc;
    return objective_eval(h, d, motion, result, grad, s);
}
int objective_hvp_presplit(cmax_handle_t h, const cmax_objective_t *d, const float *motion, const float *tangent, void *hv, hipStream_t s) {
    CMAX_REFUSE_WEIGHTED(h, "patch plan product");
    int rc = check_objective_args(h, d, motion);
    if (rc) return rc;
    return objective_hvp_impl(h, d, motion, tangent, hv, s, nullptr, false);
}
int handle_allreduce_sum(cmax_handle_t h, void *buf, size_t count, bool f64, hipStream_t s) {
    if (!h || !h->comm) return 0;
    ProfScope prof(h, kProfComm, s);
    return comm_allreduce(h->comm, buf, count, f64 ? kCommF64 : kCommF32, kCommSum, s);
}
// ... with `n_scalars` doubles that every rank computed redundantly (the per-term result[8] of the patch plan) made RANK 0'S on every
// rank by the same grouped call (rank-consistent scalars, see result_zero_unless_rank0); buf may be null (value-only evaluation)
int handle_allreduce_sum_with_scalars(cmax_handle_t h, void *buf, size_t count, bool f64, double *scalars, int n_scalars, hipStream_t s) {
    if (!h || !h->comm) return 0;
    ProfScope prof(h, kProfComm, s);
    if (comm_rank(h->comm) != 0) CMAX_CHECK_HIP(hipMemsetAsync(scalars, 0, (size_t)n_scalars * sizeof(double), s));
    void *bufs[2] = {scalars, buf};
    const size_t counts[2] = {(size_t)n_scalars, count};
    const CommType types[2] = {kCommF64, f64 ? kCommF64 : kCommF32};
    return comm_allreduce_group(h->comm, bufs, counts, types, (buf && count) ? 2 : 1, kCommSum, s);
}
}  // namespace cmax

extern "C" {

int cmax_sizeof_objective(void) { return (int)sizeof(cmax_objective_t); }

static void prof_clear(cmax_handle_s *h) {
    for (int c = 0; c < CMAX_PROF_CLASSES; ++c) {
        for (hipEvent_t e : h->prof_ev[c]) (void)hipEventDestroy(e);
        h->prof_ev[c].clear();
    }
}

int cmax_set_profiling(cmax_handle_t h, int enable) {
    CMAX_REQUIRE(h != nullptr, "set_profiling");
    CMAX_REQUIRE(enable >= 0 && enable <= 64, "set_profiling: 0 (off), 1 (bracket every launch) or 2..64 (repeat count)");
    prof_clear(h);
    h->profiling = enable != 0;
    h->prof_repeat = enable > 1 ? enable : 1;
    return 0;
}

int cmax_read_profile_all(cmax_handle_t h, double *total_ms_host, int64_t *count_host) {
    CMAX_REQUIRE(h && total_ms_host && count_host, "read_profile");
    for (int c = 0; c < CMAX_PROF_CLASSES; ++c) {
        double tot = 0.0;
        const size_t np = h->prof_ev[c].size() / 2;
        for (size_t i = 0; i < np; ++i) {
            CMAX_CHECK_HIP(hipEventSynchronize(h->prof_ev[c][2 * i + 1]));
            float ms = 0.f;
            CMAX_CHECK_HIP(hipEventElapsedTime(&ms, h->prof_ev[c][2 * i], h->prof_ev[c][2 * i + 1]));
            tot += (double)ms;
        }
        total_ms_host[c] = tot;
        count_host[c] = (int64_t)np * (c <= kProfGrad ? h->prof_repeat : 1);  // only the four hot classes are repeated
    }
    prof_clear(h);
    return 0;
}

int cmax_read_profile(cmax_handle_t h, double *total_ms_host, int64_t *count_host) {
    CMAX_REQUIRE(h && total_ms_host && count_host, "read_profile");
    double ms[CMAX_PROF_CLASSES];
    int64_t cnt[CMAX_PROF_CLASSES];
    const int rc = cmax_read_profile_all(h, ms, cnt);
    if (rc) return rc;
    for (int c = 0; c < 4; ++c) {
        total_ms_host[c] = ms[c];
        count_host[c] = cnt[c];
    }
    return 0;
}

int cmax_copy_iwe(cmax_handle_t h, int k, float *iwe_out, cmax_stream_t stream) {
    CMAX_REQUIRE(h && iwe_out && k >= 0 && k < 4, "copy_iwe");
    if (!h->last_iwe[k]) {
        set_error("copy_iwe: no objective evaluated yet for slot %d", k);
        return CMAX_ESTATE;
    }
    CMAX_CHECK_HIP(hipMemcpyAsync(iwe_out, h->last_iwe[k], (size_t)h->Hp * h->Wp * sizeof(float), hipMemcpyDeviceToDevice,
                                  (hipStream_t)stream));
    return 0;
}

int cmax_patch_search(cmax_handle_t h, int n_patch, const int *boxes, int img_h, int img_w, int n_cand, const float *cand,
                      double sigma, float *gm_out, int *count_out, cmax_stream_t stream) {
    CMAX_REFUSE_WEIGHTED(h, "patch_search");
    CMAX_REQUIRE(h && boxes && gm_out && count_out, "patch_search: null argument");
    CMAX_REQUIRE(n_patch > 0 && n_cand >= 0 && (n_cand == 0 || cand), "patch_search: n_patch > 0, n_cand >= 0");
    CMAX_REQUIRE(img_h > 0 && img_w > 0 && sigma >= 0.0, "patch_search: patch image size / sigma");
    CMAX_REQUIRE(n_cand < 65535, "patch_search: at most 65534 candidates per patch");
    const size_t lds = (size_t)2 * img_h * img_w * sizeof(float);
    if (lds > 64 * 1024 - 256) {
        set_error("patch_search: a %d x %d patch image does not fit the 64 KB workgroup LDS budget", img_h, img_w);
        return CMAX_EINVAL;
    }
    if (h->n == 0) {
        set_error("patch_search: no events set");
        return CMAX_ESTATE;
    }
    hipStream_t s = (hipStream_t)stream;
    {
        int rc = h->search_range.reserve(&h->bytes, n_patch, s);
        if (rc) return rc;
    }
    CMAX_REQUIRE(h->n_outside == 0, "patch_search: the batch holds events off the sensor (cmax_set_keep_outside)");
    SearchArgs a;
    a.evp = h->evp;
    a.rx = h->rx;
    a.ry = h->ry;
    a.tile_start = h->d_tile_start;
    a.groups_per_tile = h->n_time_bin > 0 ? h->n_time_bin : 1;
    a.ntr = h->ntr;
    a.ntc = h->ntc;
    a.has_frac = h->has_frac ? 1 : 0;
    a.slab_major = h->slab_major && h->n_time_bin > 0 ? 1 : 0;
    a.boxes = (const int4 *)boxes;
    a.img_h = img_h;
    a.img_w = img_w;
    hipLaunchKernelGGL(k_search_range, dim3(n_patch), dim3(kSearchThreads), 0, s, a, h->search_range, count_out);
    CMAX_CHECK_LAUNCH();
    const int radius = sigma > 0.0 ? (int)(4.0 * sigma + 0.5) : 0;  // scipy.ndimage.gaussian_filter, truncate = 4
    hipLaunchKernelGGL(k_patch_search, dim3(n_patch, n_cand + 1), dim3(kSearchThreads), lds, s, a, h->search_range, n_cand,
                       (const float2 *)cand, (float)(h->tmax_host - h->tmin_host), (float)sigma, radius, gm_out);
    CMAX_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
