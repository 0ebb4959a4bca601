// The optimiser's objective for patch-based flow in ONE library call: x[2 * n_patch] (host, fp64) ->
// loss, gradient (host, fp64), every stage on the device, one stream synchronisation per call.
//
// Equivalent of PyramidalPatchContrastMaximization.objective_scipy + motion_to_dense_flow
// (src/solver/patch_contrast_pyramid.py:430-516) under TorchWrapper.get_value_and_grad / get_hvp
// (src/solver/scipy_autograd/torch_wrapper.py:30-73):
//   patch motion -> dense flow (cmax_patch_to_dense) -> x t_scale [-> Burgers / upwind voxel] -> fp32
//   -> sum_i w_i * fused contrast objective_i (cmax_objective)  [+ w_tv * total_variation(patch motion)]
// and back through the hand-written adjoints.  The stages are the library's own C entry points (the same
// kernels the autograd wrappers of functional.py chain one Python call at a time); what this file adds is
// the plan that owns the intermediate buffers and the pinned staging, so that an evaluation costs one
// ctypes call instead of ~40 Python-level operations, and replays its launch sequence from a captured hipGraph
// (measured on the cfg1-shaped objective: 0.40 ms -> 0.09 ms per value + gradient).
// Pre/post stages run in fp64 like the reference's solver (patch_contrast_pyramid.py:186); the event
// path is fp32 per event with fp64 reductions as everywhere in cmax_fused.hip.
// A plan made by cmax_basis_plan_create is the same plan with the patch interpolation exchanged for a flow basis, D = sum_k x_k B_k
// (cmax_basis_kernels.h): a motion model linear in its parameters.  The reference has no counterpart for that map; D is warped by its
// dense-flow rule x' = x - dt * D[src] (src/warp.py:263-313).
// A plan made by cmax_depth_plan_create maps x = [a | b | s] to D = (Q s) (sum_k a_k A_k) + sum_j b_j B_j (cmax_depth_kernels.h): the motion
// field of a static scene over a grid of inverse depth.  That map is NOT linear, so its product has a sequence of its own (enqueue_hvp_depth).
#include <cstring>
#include <new>
#include <atomic>
#include <vector>

#include "cmax_basis_kernels.h"
#include "cmax_buffers.h"
#include "cmax_common.h"
#include "cmax_depth_kernels.h"
#include "cmax_descent.h"
#include "cmax_lbfgs.h"
#include "cmax_flowreg_kernels.h"
#include "cmax_image_kernels.h"
#include "cmax_patch_kernels.h"

namespace cmax {

// out = in * scale [* *scale_dev]: scalars that change from call to call (the tangent's norm) live in device memory so
// that a captured graph can be replayed with new values
template <typename TO, typename TI>
__global__ void __launch_bounds__(256)
k_convert_scale(const TI *__restrict__ in, int64_t n, double scale, const double *__restrict__ scale_dev, TO *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const double sc = scale_dev ? scale * scale_dev[0] : scale;
    if (i < n) out[i] = (TO)((double)in[i] * sc);
}

// ... for a plan whose terms take the fp64 motion (cmax_objective_t::motion_dtype == CMAX_F64): hi = what k_convert_scale<float, double>
// writes, lo = what fp32 lost of the scaled value (split_f64), in the same launch
__global__ void __launch_bounds__(256)
k_convert_split(const double *__restrict__ in, int64_t n, double scale, const double *__restrict__ scale_dev, float *__restrict__ hi, float *__restrict__ lo) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const double sc = scale_dev ? scale * scale_dev[0] : scale;
    if (i < n) split_f64(in[i] * sc, hi[i], lo[i]);
}
// ... and of k_patch_to_dense<double, float>: the patch grid -> both planes of flow * scale
template <int F = CMAX_FILTER_BILINEAR>
__global__ void __launch_bounds__(256)
k_patch_to_dense_split(const double *__restrict__ motion, int ph, int pw, int pad_h, int pad_w, int sw_h, int sw_w, int H, int W, float *__restrict__ hi,
                       float *__restrict__ lo, double scale) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= 2 * (int64_t)H * W) return;
    split_f64(patch_interp<double, F>(motion, ph, pw, pad_h, pad_w, sw_h, sw_w, H, W, p) * scale, hi[p], lo[p]);
}

// acc (=, +=) w [* *w_dev] * g
__global__ void __launch_bounds__(256)
k_accumulate(const float *__restrict__ g, int64_t n, double w, int first, double *__restrict__ acc, const double *__restrict__ w_dev = nullptr) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w_dev) w *= w_dev[0];
    if (i < n) acc[i] = (first ? 0.0 : acc[i]) + w * (double)g[i];
}

// max |x| as the bit pattern of a non-negative double (order-preserving under unsigned compare); *bits zeroed by the caller
__global__ void __launch_bounds__(256) k_absmax(const double *__restrict__ x, int64_t n, unsigned long long *__restrict__ bits) {
    __shared__ double s_m[256 / kWave];
    double m = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + 3 * stride < n; i += 4 * stride) {  // four independent loads in flight per thread
        const double a = x[i], b = x[i + stride], c = x[i + 2 * stride], d = x[i + 3 * stride];
        m = fmax(fmax(m, fmax(fabs(a), fabs(b))), fmax(fabs(c), fabs(d)));
    }
    for (; i < n; i += stride) m = fmax(m, fabs(x[i]));
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, kWave));
    if ((threadIdx.x & (kWave - 1)) == 0) s_m[threadIdx.x / kWave] = m;
    __syncthreads();
    // one atomic per workgroup (and few workgroups): equal-address atomics serialise at ~12 ns each
    if (threadIdx.x == 0) atomicMax(bits, (unsigned long long)__double_as_longlong(fmax(fmax(s_m[0], s_m[1]), fmax(s_m[2], s_m[3]))));
}

// scal[0] = max (1 if the field is all zero), scal[1] = 1 / scal[0]
__global__ void k_absmax_finish(const unsigned long long *__restrict__ bits, double *__restrict__ scal) {
    const double m = __longlong_as_double((long long)bits[0]);
    scal[0] = m > 0.0 ? m : 1.0;
    scal[1] = 1.0 / scal[0];
}

// ---------------------------------------------------------------------------------------------
// solver.scale_later (src/solver/patch_contrast_pyramid.py:489-515, src/solver/base.py:219-224): with D = P x [2,H,W] the dense
// flow, t = t_scale and C the Burgers / upwind voxel chain,
//   s = max D (ONE signed scalar over both components),  u = t D / s,  V = C(u),  motion M = s V.
// torch's full-reduction max back-propagates evenly over the n elements equal to the maximum: kappa = ds/dD = 1/n there.
// With g_M = dL/dM and h = J(u)^T g_M (the adjoint sweep, unscaled seed):   g_D = t h + kappa (<g_M, V> - <h, u>).
// Along a tangent Dd:  sd = <kappa, Dd>,  ud = (t Dd - u sd) / s,  W = J ud,  Md = sd V + s W,  gd_M = H_MM Md,
//   hd = J^T gd_M + (dJ[ud])^T g_M (the dual sweep, seeds (g_M, gd_M)),  gd_D = t hd + kappa (<gd_M, V> + <g_M, W> - <hd, u> - <h, ud>).
// s, the tie count and every inner product stay in device memory (the sequence is capturable).  Reductions: kSlBlocks
// workgroups leave one partial sum each (plain stores), and every workgroup of the consuming kernel adds them up in the
// same fixed order -- no floating-point atomics, bit-identical from run to run.
// ---------------------------------------------------------------------------------------------
constexpr int kSlBlocks = 256;  // = the consumers' workgroup size: one partial per thread
// partial[slot][kSlBlocks]: 0..2 inner products taken before the adjoint sweep, 3..4 after it, 5 tie count, 6 sum of Dd over the ties,
// 7 maxima of D
constexpr int kSlSlots = 8, kSlPost = 3, kSlCount = 5, kSlTangent = 6, kSlMax = 7;
// scalars: [0] s (1 when the maximum is 0 or not finite: the event kernels must see a finite motion), [1] 1 if s is usable, else 0
// (the tail then writes NaN, the reference's 0/0), [2] sd
constexpr int kSlScalars = 4;
static inline int sl_grid(int64_t n) { const int g = div_up(n, 256); return g < kSlBlocks ? g : kSlBlocks; }

// D = P x and, per workgroup, its signed maximum (no atomics: ~700 same-address atomics would cost more than the pass itself)
template <int F = CMAX_FILTER_BILINEAR>
__global__ void __launch_bounds__(256)
k_patch_to_dense_max(const double *__restrict__ motion, int ph, int pw, int pad_h, int pad_w, int sw_h, int sw_w, int H, int W,
                     double *__restrict__ D, double *__restrict__ partial) {
    double m = -INFINITY;
    const int64_t n = 2 * (int64_t)H * W;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const double v = D[p] = patch_interp<double, F>(motion, ph, pw, pad_h, pad_w, sw_h, sw_w, H, W, p);
        m = fmax(m, v);
    }
    m = block_max(m);
    if (threadIdx.x == 0) partial[kSlMax * kSlBlocks + blockIdx.x] = m;
}

// s = max D from the workgroups' maxima; u = t D / s; per workgroup: number of pixels with D == s and (Hessian-vector
// products) the sum of the tangent Dd over them.  Workgroup 0 publishes s and whether it is usable.
__global__ void __launch_bounds__(256)
k_sl_scale(const double *__restrict__ D, const double *__restrict__ Dd, int64_t n, double t, int n_partial, double *__restrict__ sl,
           double *__restrict__ u, double *__restrict__ partial) {
    __shared__ double smem[2 * 256 / kWave];
    const double fm = block_max((int)threadIdx.x < n_partial ? partial[kSlMax * kSlBlocks + threadIdx.x] : -INFINITY);
    const bool ok = isfinite(fm) && fm != 0.0;
    const double s = ok ? fm : 1.0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        sl[0] = s;
        sl[1] = ok ? 1.0 : 0.0;
    }
    double v[2] = {0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double d = D[i];
        double q = d * t / s;  // the reference's order: dense_flow * t_scale / scale
        if (!ok && !isfinite(q)) q = 0.0;
        u[i] = q;
        if (ok && d == s) {
            v[0] += 1.0;
            if (Dd) v[1] += Dd[i];
        }
    }
    block_sum<2>(v, smem);
    if (threadIdx.x == 0) {
        partial[kSlCount * kSlBlocks + blockIdx.x] = v[0];
        partial[kSlTangent * kSlBlocks + blockIdx.x] = v[1];
    }
}

// ud = (t Dd - u sd) / s in place of Dd, with sd = <kappa, Dd>; Dd arrives un-normalised (times *dd_scale)
__global__ void __launch_bounds__(256)
k_sl_tangent(const double *__restrict__ u, double *__restrict__ Dd, int64_t n, double t, const double *__restrict__ dd_scale,
             double *__restrict__ sl, const double *__restrict__ partial, int n_partial) {
    __shared__ double smem[2 * 256 / kWave];
    __shared__ double s_sd;
    double v[2] = {0.0, 0.0};
    if ((int)threadIdx.x < n_partial) {
        v[0] = partial[kSlCount * kSlBlocks + threadIdx.x];
        v[1] = partial[kSlTangent * kSlBlocks + threadIdx.x];
    }
    block_sum<2>(v, smem);
    if (threadIdx.x == 0) s_sd = v[0] > 0.0 ? dd_scale[0] * v[1] / v[0] : 0.0;
    __syncthreads();
    const double sd = s_sd, s = sl[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) sl[2] = sd;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) Dd[i] = (t * (Dd[i] * dd_scale[0]) - u[i] * sd) / s;
}

// Md = sd V + s W (fp64, its max-norm is taken next) and the fp32 motion s V in one pass
__global__ void __launch_bounds__(256)
k_sl_motion_tangent(const double *__restrict__ V, const double *__restrict__ Wt, int64_t n, const double *__restrict__ sl,
                    double *__restrict__ Md, float *__restrict__ motion32) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double s = sl[0], sd = sl[2], v = V[i];
    Md[i] = sd * v + s * Wt[i];
    motion32[i] = (float)(s * v);
}
// ... of a plan whose terms take the fp64 motion: both planes of s V (k_convert_split)
__global__ void __launch_bounds__(256)
k_sl_motion_tangent_split(const double *__restrict__ V, const double *__restrict__ Wt, int64_t n, const double *__restrict__ sl,
                          double *__restrict__ Md, float *__restrict__ hi, float *__restrict__ lo) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double s = sl[0], sd = sl[2], v = V[i];
    Md[i] = sd * v + s * Wt[i];
    split_f64(s * v, hi[i], lo[i]);
}

struct DotJobs {
    const double *a[3], *b[3];
    int n_dots;
};
// partial[slot0 + k][workgroup] = this workgroup's share of <a_k, b_k>, k < n_dots
__global__ void __launch_bounds__(256) k_sl_dots(DotJobs jobs, int64_t n, int slot0, double *__restrict__ partial) {
    __shared__ double smem[3 * 256 / kWave];
    double v[3] = {0.0, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (k < jobs.n_dots) v[k] += jobs.a[k][i] * jobs.b[k][i];
    }
    block_sum<3>(v, smem);
    if (threadIdx.x == 0)
        for (int k = 0; k < jobs.n_dots; ++k) partial[(slot0 + k) * kSlBlocks + blockIdx.x] = v[k];
}

struct SlCoef {
    double c[kSlCount];  // weight of inner product `slot` in g_s (0: slot not used by this call)
    int n_pre, n_post, n_count;  // partials per slot: before the sweep, after it, of the tie count
};
// g_D = t h + g_s kappa: the scatter of g_s over the ties rides on the pass that scales the sweep's result
__global__ void __launch_bounds__(256)
k_sl_grad_dense(const double *__restrict__ h, const double *__restrict__ D, int64_t n, double t, const double *__restrict__ sl,
                const double *__restrict__ partial, SlCoef cf, double *__restrict__ gD) {
    __shared__ double smem[2 * 256 / kWave];
    __shared__ double s_gk;
    double v[2] = {0.0, 0.0};
    for (int k = 0; k < kSlCount; ++k)
        if (cf.c[k] != 0.0 && (int)threadIdx.x < (k < kSlPost ? cf.n_pre : cf.n_post)) v[0] += cf.c[k] * partial[k * kSlBlocks + threadIdx.x];
    if ((int)threadIdx.x < cf.n_count) v[1] = partial[kSlCount * kSlBlocks + threadIdx.x];
    block_sum<2>(v, smem);
    if (threadIdx.x == 0) s_gk = v[1] > 0.0 ? v[0] / v[1] : 0.0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) gD[i] = t * h[i] + (D[i] == sl[0] ? s_gk : 0.0);
}

// ---- the reduction as a leaf operator (the autograd-chained path): out[0] = max, out[1] = number of elements equal to it
template <typename T>
__global__ void __launch_bounds__(256) k_field_max(const T *__restrict__ x, int64_t n, double *__restrict__ out) {
    double m = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) m = fmax(m, (double)x[i]);
    double fm;
    if (grid_max_last(m, reinterpret_cast<unsigned long long *>(out + 2), reinterpret_cast<unsigned int *>(out + 3), fm)) out[0] = fm;
}
template <typename T>
__global__ void __launch_bounds__(256) k_field_count(const T *__restrict__ x, int64_t n, double *__restrict__ out) {
    __shared__ double smem[256 / kWave];
    const double m = out[0];
    double v[1] = {0.0};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) v[0] += (double)x[i] == m ? 1.0 : 0.0;
    block_sum<1>(v, smem);
    if (threadIdx.x == 0 && v[0] > 0.0) atomic_add(out + 1, v[0]);  // (whole numbers: exact in any order)
}
// adjoint: gx = gout / count on the elements equal to the maximum, 0 elsewhere
template <typename T>
__global__ void __launch_bounds__(256)
k_field_max_adj(const T *__restrict__ x, int64_t n, const double *__restrict__ out, const double *__restrict__ gout, T *__restrict__ gx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) gx[i] = (double)x[i] == out[0] ? (T)(gout[0] / out[1]) : (T)0;
}

enum { kMapPatch = 0, kMapBasis = 1, kMapDepth = 2 };  // cmax_patch_plan_s::map_kind

struct FinalParams {
    int n_terms, with_tv, nx;  // nx = 0: value only
    int flag_slot;             // index (in doubles) of the run counter in the output: 1 + the plan's nx, whatever this call's nx is
    int ph, pw, tv_crop;       // patch grid of the total-variation term
    double weight[4], tv_weight, gscale;
    double reg_weight = 0.0;  // flow regulariser (cmax_flowreg_kernels.h): its value is results[8 * 4]; 0 = no such term
};

// Tail of an evaluation in ONE workgroup (every dependent launch costs ~4.5 us on this chip and the operands are a
// few hundred numbers): total variation of the patch motion x [2,ph,pw] -- mean |Sobel/8| over 4 channels,
// TotalVariation.calculate_torch, src/costs/total_variation.py:60-75, 110-126 -- and its sub-gradient, the weighted
// sum of the contrast terms, and the chain through t_scale:
//   out[0] = sum_i w_i result_i + w_tv TV(x) [+ w_reg R(F), the flow regulariser's value in the fifth result slot],   out[1 + j] = gscale * gx[j] + w_tv dTV/dx[j]
// gx comes as fp64 (gx64) or fp32 (gx32); gscale_dev multiplies gscale (Hessian-vector products).  `out` may be
// pinned host memory.  ok_dev (scale_later plans): *ok_dev == 0 -> loss and gradient are NaN.
constexpr int kTailLds = 4096;  // patch-grid values staged in LDS by k_patch_tail (2 x 45 x 45 patches)
__global__ void __launch_bounds__(256)
k_patch_tail(FinalParams fp, const double *__restrict__ results, const double *__restrict__ x, const double *__restrict__ gx64,
             const float *__restrict__ gx32, const double *__restrict__ gscale_dev, double *__restrict__ out,
             unsigned long long *__restrict__ seq_dev, const double *__restrict__ ok_dev = nullptr) {
    __shared__ double smem[4];
    __shared__ double s_tv;
    __shared__ double s_x[kTailLds];
    __shared__ signed char s_sx[kTailLds], s_sy[kTailLds];  // sign of the Sobel responses on Omega, 0 elsewhere
    const int h = fp.ph, w = fp.pw, hw = h * w;
    const int i0 = fp.tv_crop ? 1 : 0, hh = h - 2 * i0, ww = w - 2 * i0;
    const double ntv = 4.0 * (double)hh * (double)ww;
    const bool lds = 2 * hw <= kTailLds;
    const double *xs = x;
    if (fp.with_tv) {
        if (lds) {
            for (int p = threadIdx.x; p < 2 * hw; p += blockDim.x) s_x[p] = x[p];
            __syncthreads();
            xs = s_x;
        }
        double v[1] = {0.0};
        for (int p = threadIdx.x; p < 2 * hw; p += blockDim.x) {
            const int c = p / hw, r = p - c * hw, i = r / w, j = r - i * w;
            signed char gx = 0, gy = 0;
            if (i >= i0 && i < h - i0 && j >= i0 && j < w - i0) {
                double sx, sy;
                sobel8<double>(xs + c * hw, h, w, i, j, sx, sy);
                v[0] += fabs(sx) + fabs(sy);
                gx = (signed char)((sx > 0) - (sx < 0));
                gy = (signed char)((sy > 0) - (sy < 0));
            }
            if (lds) {
                s_sx[p] = gx;
                s_sy[p] = gy;
            }
        }
        block_sum<1>(v, smem);  // its barriers also publish s_sx / s_sy
        if (threadIdx.x == 0) s_tv = v[0] / ntv;
        __syncthreads();
    }
    double gscale = fp.gscale;
    if (gscale_dev) gscale *= gscale_dev[0];
    const bool undefined = ok_dev && ok_dev[0] == 0.0;  // scale_later with max D = 0 (or not finite): the reference divides 0 by 0
    if (threadIdx.x == 0) {
        double loss = 0.0;
        for (int i = 0; i < fp.n_terms; ++i) loss += fp.weight[i] * results[8 * i];
        if (fp.with_tv) loss += fp.tv_weight * s_tv;
        if (fp.reg_weight != 0.0) loss += fp.reg_weight * results[8 * 4];
        out[0] = undefined ? (double)NAN : loss;
    }
    for (int p = threadIdx.x; p < fp.nx; p += blockDim.x) {
        double g = gscale * (gx64 ? gx64[p] : (double)gx32[p]);
        if (fp.with_tv) {
            const int c = p / hw, r = p - c * hw, i = r / w, j = r - i * w;
            double sgn = 0.0;
            for (int a = -1; a <= 1; ++a)
                for (int b = -1; b <= 1; ++b) {
                    const int qi = i - a, qj = j - b;  // output pixel that reads (i, j) with tap (a, b)
                    if (qi < i0 || qi >= h - i0 || qj < i0 || qj >= w - i0) continue;
                    double gsx, gsy;
                    if (lds) {
                        gsx = (double)s_sx[c * hw + qi * w + qj];
                        gsy = (double)s_sy[c * hw + qi * w + qj];
                    } else {
                        double sx, sy;
                        sobel8<double>(x + c * hw, h, w, qi, qj, sx, sy);
                        gsx = (double)((sx > 0) - (sx < 0));
                        gsy = (double)((sy > 0) - (sy < 0));
                    }
                    // SX[a+1][b+1] = a * (2 - |b|), SY[a+1][b+1] = b * (2 - |a|)
                    sgn += gsx * (double)(a * (2 - (b < 0 ? -b : b))) + gsy * (double)(b * (2 - (a < 0 ? -a : a)));
                }
            g += fp.tv_weight * sgn / 8.0 / ntv;
        }
        out[1 + p] = undefined ? (double)NAN : g;
    }
    // completion flag for a host that polls the (pinned) output instead of sleeping in hipStreamSynchronize: a run
    // counter, written after every result of this launch is visible system-wide
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long v = seq_dev[0] + 1ull;
        seq_dev[0] = v;
        reinterpret_cast<volatile unsigned long long *>(out + fp.flag_slot)[0] = v;
    }
}

// One iteration of the device-resident descent (cmax_descent.h; src/solver/base.py:840-881): loss and gradient are read where the
// tail / the 2-DoF objective left them in device memory, the non-finite test covers ALL of g before any store, then m, v, x, x_best,
// history and trace are updated grid-stride in fp64.  ONE workgroup: nx is 2 .. 8192 and every step depends on the last.  The last
// iteration publishes the result block and, behind a system-wide fence, the run counter to pinned memory, as k_patch_tail does.
__global__ void __launch_bounds__(256) k_descent_step(DescentArgs a, const double *__restrict__ loss, const double *__restrict__ grad) {
    const double L = loss[0];
    int bad = isfinite(L) ? 0 : 1;
    for (int p = threadIdx.x; p < a.nx; p += blockDim.x) bad |= isfinite(grad[p]) ? 0 : 1;
    bad = __syncthreads_or(bad);
    const DescentDecision d = descent_decide(a, L, bad != 0);
    for (int p = threadIdx.x; p < a.nx; p += blockDim.x) descent_element(a, d, p, grad[p]);
    __syncthreads();  // (every thread has read the control block)
    if (threadIdx.x == 0) descent_publish(a, d, L);
    if (a.it == a.n_iter - 1 && a.flag) {
        __threadfence_system();
        __syncthreads();
        if (threadIdx.x == 0) *a.flag = a.seq_src ? a.seq_src[0] : a.seq;
    }
}

int launch_descent_step(const DescentArgs &a, const double *loss, const double *grad, hipStream_t s) {
    hipLaunchKernelGGL(k_descent_step, dim3(1), dim3(256), 0, s, a, loss, grad);
    CMAX_CHECK_LAUNCH();
    return 0;
}

// ---- device-resident L-BFGS (cmax_lbfgs.h; the rules: include/cmax_hip.h) ----------------------------------------------------------------
// exact in any order; every lane receives the result
__device__ __forceinline__ double wave_max_all(double v) {
    for (int o = kWave / 2; o; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double wave_min_all(double v) {
    for (int o = kWave / 2; o; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ bool lbfgs_held(int slot, int head, int k, int m) { return slot < m && (slot - head + m) % m < k; }
__device__ __forceinline__ double lbfgs_trial(double xa, double alpha, double d, double x0, double max_move) {
    return fmin(fmax(xa + alpha * d, x0 - max_move), x0 + max_move);
}

// The textbook two-loop recursion on the vectors themselves (LbfgsArgs::two_loop; x_a, g_a and the pairs are stored): q lives in v.d, every
// inner product is a block reduction that waits for the last.  s^T y of a pair comes from the Gram diagonal.  -> g_a^T d in every thread.
__device__ double lbfgs_two_loop_direction(const LbfgsView &v, int nx, int m, int k, int head, double *s_red, double *s_a, double *s_bc) {
    constexpr int M = CMAX_LBFGS_MAX_HISTORY, NB = kLbBasis;
    const int tid = threadIdx.x;
    for (int p = tid; p < nx; p += blockDim.x) v.d[p] = v.ga[p];
    for (int i = k - 1; i >= 0; --i) {
        const int c = (head + i) % m;
        const double *S = v.S + (int64_t)c * nx, *Y = v.Y + (int64_t)c * nx;
        double dot[1] = {0.0};
        for (int p = tid; p < nx; p += blockDim.x) dot[0] += S[p] * v.d[p];
        block_sum<1>(dot, s_red);
        if (tid == 0) s_a[c] = dot[0] / v.gram[c * NB + M + c];
        __syncthreads();
        const double ai = s_a[c];
        for (int p = tid; p < nx; p += blockDim.x) v.d[p] -= ai * Y[p];
    }
    const int cn = (head + k - 1) % m;
    const double gamma = v.gram[cn * NB + M + cn] / v.gram[(M + cn) * NB + M + cn];
    for (int p = tid; p < nx; p += blockDim.x) v.d[p] *= gamma;
    for (int i = 0; i < k; ++i) {
        const int c = (head + i) % m;
        const double *S = v.S + (int64_t)c * nx, *Y = v.Y + (int64_t)c * nx;
        double dot[1] = {0.0};
        for (int p = tid; p < nx; p += blockDim.x) dot[0] += Y[p] * v.d[p];
        block_sum<1>(dot, s_red);
        if (tid == 0) s_bc[0] = s_a[c] - dot[0] / v.gram[c * NB + M + c];
        __syncthreads();
        const double t = s_bc[0];
        for (int p = tid; p < nx; p += blockDim.x) v.d[p] += t * S[p];
    }
    double dot[1] = {0.0};
    for (int p = tid; p < nx; p += blockDim.x) {
        const double dp = -v.d[p];
        v.d[p] = dp;
        dot[0] += v.ga[p] * dp;
    }
    block_sum<1>(dot, s_red);
    if (tid == 0) s_bc[1] = dot[0];
    __syncthreads();
    return s_bc[1];
}

// One evaluation's decision of the device-resident L-BFGS: loss and gradient are read where the tail / the 2-DoF objective left them, as in
// k_descent_step; ONE workgroup (nx is 2 .. 8192, m <= 16, every step depends on the last).  The non-finite test covers ALL of g before
// any store.  An evaluation that passes the Armijo test costs ONE reduction pass behind one barrier: the threads stride over x for the
// products among the new s, y and g (wave tree, then the four waves in order), and every wave takes eight rows of {S, Y}, four at a time,
// for their products with s, y and g.  Wave 0 then brings the Gram matrix (LDS copy and state) up to date and runs the two-loop recursion
// on the COEFFICIENTS of d in the basis {s_i, y_i, g}: lane j keeps u_j = <current vector, basis_j>, so a step of the recursion is one
// cross-lane read and one multiply-add, with no reduction.  A last pass forms d as one linear combination, stores the new pair, x_a and
// g_a, and reduces the box's limit on alpha; the trial point is written in place of x.  No atomics: the result depends on nothing but
// the inputs.  The last evaluation publishes the result block and, behind a system-wide fence, the run counter, as k_descent_step does.
__global__ void __launch_bounds__(256) k_lbfgs_step(LbfgsArgs a, const double *__restrict__ loss, const double *__restrict__ grad) {
    constexpr int M = CMAX_LBFGS_MAX_HISTORY, NB = kLbBasis, G = kLbG;
    __shared__ double s_gram[NB * NB];
    __shared__ double s_prod[2 * M][3];  // <row, s>, <row, y>, <row, g>: rows 0 .. 15 the S slots, 16 .. 31 the Y slots
    __shared__ double s_part[4][8];      // per wave: ss, sy, yy, gs, gy, gg, |g|_1, |g|_inf
    __shared__ double s_coef[NB];
    __shared__ double s_gd;
    __shared__ double s_min[4];
    __shared__ double s_a[M], s_bc[2];  // (two_loop only)
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave, nx = a.nx, m = a.m;
    const LbfgsView v = lbfgs_view(a.st, nx, m, a.n_eval);
    const bool first = a.e == 0, last = a.e == a.n_eval - 1;
    const double L = loss[0];
    // the control block (every thread reads it; the writer waits behind a barrier).  Evaluation 0 reads none of the state.
    const bool done_prev = !first && v.ctrl[kLbDone] != 0.0;
    int status = first ? CMAX_LBFGS_BUDGET : (int)v.ctrl[kLbStatus];
    double L_a = first ? 0.0 : v.ctrl[kLbLa];
    const double alpha_e = first ? 0.0 : v.ctrl[kLbAlpha];  // the alpha of the point evaluated here
    double alpha = alpha_e, gd = first ? 0.0 : v.ctrl[kLbGd];
    int n_ls = first ? 0 : (int)v.ctrl[kLbNls], n_iter = first ? 0 : (int)v.ctrl[kLbNiter], used = first ? 0 : (int)v.ctrl[kLbUsed];
    int k = first ? 0 : (int)v.ctrl[kLbK], head = first ? 0 : (int)v.ctrl[kLbHead];
    double ginf_a = first ? 0.0 : v.ctrl[kLbGinf], g1_a = first ? 0.0 : v.ctrl[kLbG1], gg_a = first ? 0.0 : v.ctrl[kLbGg];
    double last_alpha = first ? 0.0 : v.ctrl[kLbLastAlpha];
    if (a.has_trace)
        for (int p = tid; p < nx; p += blockDim.x) v.trace[(int64_t)a.e * nx + p] = a.x[p];

    int code = CMAX_LBFGS_CODE_IDLE;
    bool done = done_prev;
    if (!done_prev) {
        const bool armijo = first || (isfinite(L) && L <= L_a + a.c1 * alpha * gd);
        bool ok = false;
        double ss = 0.0, sy = 0.0, yy = 0.0, gs = 0.0, gy = 0.0, gg = 0.0, g1 = 0.0, ginf = 0.0;
        if (armijo) {  // (uniform) the one reduction pass
            if (k > 0 && !a.two_loop)
                for (int i = tid; i < NB * NB; i += blockDim.x) s_gram[i] = v.gram[i];
            int bad = isfinite(L) ? 0 : 1;
            double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, mx = 0.0;
            for (int p = tid; p < nx; p += blockDim.x) {
                const double g = grad[p];
                bad |= isfinite(g) ? 0 : 1;
                const double sp = first ? 0.0 : a.x[p] - v.xa[p], yp = first ? 0.0 : g - v.ga[p];
                acc[0] += sp * sp;
                acc[1] += sp * yp;
                acc[2] += yp * yp;
                acc[3] += g * sp;
                acc[4] += g * yp;
                acc[5] += g * g;
                acc[6] += fabs(g);
                mx = fmax(mx, fabs(g));
            }
#pragma unroll
            for (int q = 0; q < 7; ++q) acc[q] = wave_sum_lane63(acc[q]);
            mx = wave_max_all(mx);
            if (lane == kWave - 1) {
#pragma unroll
                for (int q = 0; q < 7; ++q) s_part[wid][q] = acc[q];
                s_part[wid][7] = mx;
            }
            if (k > 0 && !a.two_loop) {
                for (int grp = 0; grp < 2; ++grp) {
                    const double *row[4];
                    bool held[4], any = false;
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int r = wid + 4 * (4 * grp + t), slot = r & (M - 1);
                        held[t] = lbfgs_held(slot, head, k, m);
                        any |= held[t];
                        row[t] = held[t] ? (r < M ? v.S : v.Y) + (int64_t)slot * nx : v.d;  // (a row that is not held: any readable line, result unused)
                    }
                    if (!any) continue;
                    double pr[4][3] = {};
                    for (int p = lane; p < nx; p += kWave) {
                        const double g = grad[p], sp = a.x[p] - v.xa[p], yp = g - v.ga[p];
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            const double b = row[t][p];
                            pr[t][0] += b * sp;
                            pr[t][1] += b * yp;
                            pr[t][2] += b * g;
                        }
                    }
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) pr[t][c] = wave_sum_lane63(pr[t][c]);
                        if (lane == kWave - 1 && held[t]) {
                            const int r = wid + 4 * (4 * grp + t);
                            s_prod[r][0] = pr[t][0];
                            s_prod[r][1] = pr[t][1];
                            s_prod[r][2] = pr[t][2];
                        }
                    }
                }
            }
            bad = __syncthreads_or(bad);
            ok = bad == 0;
            ss = s_part[0][0] + s_part[1][0] + s_part[2][0] + s_part[3][0];
            sy = s_part[0][1] + s_part[1][1] + s_part[2][1] + s_part[3][1];
            yy = s_part[0][2] + s_part[1][2] + s_part[2][2] + s_part[3][2];
            gs = s_part[0][3] + s_part[1][3] + s_part[2][3] + s_part[3][3];
            gy = s_part[0][4] + s_part[1][4] + s_part[2][4] + s_part[3][4];
            gg = s_part[0][5] + s_part[1][5] + s_part[2][5] + s_part[3][5];
            g1 = s_part[0][6] + s_part[1][6] + s_part[2][6] + s_part[3][6];
            ginf = fmax(fmax(s_part[0][7], s_part[1][7]), fmax(s_part[2][7], s_part[3][7]));
        }

        // what the next trial is formed from: the accepted point's gradient, whether the new point is stored, the direction's kind
        bool choose = false, accept = false, push = false, steep = true, stored = false;
        int nslot = -1;
        double alpha0 = 0.0;
        if (ok) {
            accept = true;
            code = first ? CMAX_LBFGS_CODE_START : CMAX_LBFGS_CODE_ACCEPTED;
            push = !first && yy > 0.0 && sy > a.curv_eps * yy;
            const int k_old = k, head_old = head;
            if (push) {
                if (k < m) {
                    nslot = (head + k) % m;
                    k += 1;
                } else {
                    nslot = head;
                    head = (head + 1) % m;
                }
            }
            if (!first) {
                n_iter += 1;
                last_alpha = alpha;
            }
            n_ls = 0;
            L_a = L;
            ginf_a = ginf;
            g1_a = g1;
            gg_a = gg;
            if (ginf <= a.gtol) {
                status = CMAX_LBFGS_CONVERGED;
                done = true;
            } else {
                choose = true;
                if (k > 0 && a.two_loop) {
                    for (int p = tid; p < nx; p += blockDim.x) {
                        const double g = grad[p], xt = a.x[p];
                        if (push) {
                            v.S[(int64_t)nslot * nx + p] = xt - v.xa[p];
                            v.Y[(int64_t)nslot * nx + p] = g - v.ga[p];
                        }
                        v.xa[p] = xt;
                        v.ga[p] = g;
                    }
                    if (tid == 0 && push) {
                        v.gram[nslot * NB + M + nslot] = sy;
                        v.gram[(M + nslot) * NB + M + nslot] = yy;
                    }
                    stored = true;
                    __syncthreads();
                    const double gdn = lbfgs_two_loop_direction(v, nx, m, k, head, s_min, s_a, s_bc);
                    if (gdn < 0.0) {
                        steep = false;
                        gd = gdn;
                        alpha0 = 1.0;
                    } else {
                        k = 0;
                        head = 0;
                    }
                } else if (k > 0) {
                    if (wid == 0 && lane < NB) {  // the Gram matrix: the rows of the new s and y, the row of the new g
                        const int j = lane;
                        const bool hj = j < G && lbfgs_held(j & (M - 1), head_old, k_old, m);
                        double ps = j == G ? gs : (hj ? s_prod[j & (2 * M - 1)][0] : 0.0);
                        double py = j == G ? gy : (hj ? s_prod[j & (2 * M - 1)][1] : 0.0);
                        double pg = j == G ? gg : (hj ? s_prod[j & (2 * M - 1)][2] : 0.0);
                        if (push) {
                            if (j == nslot) ps = ss, py = sy, pg = gs;
                            if (j == M + nslot) ps = sy, py = yy, pg = gy;
                            s_gram[nslot * NB + j] = s_gram[j * NB + nslot] = ps;
                            s_gram[(M + nslot) * NB + j] = s_gram[j * NB + M + nslot] = py;
                            v.gram[nslot * NB + j] = v.gram[j * NB + nslot] = ps;
                            v.gram[(M + nslot) * NB + j] = v.gram[j * NB + M + nslot] = py;
                        }
                        s_gram[G * NB + j] = s_gram[j * NB + G] = pg;
                        v.gram[G * NB + j] = v.gram[j * NB + G] = pg;
                    }
                    __syncthreads();
                    if (wid == 0) {  // the two-loop recursion on coefficients: u = <vector, basis_j> per lane
                        const int j = lane;
                        const bool hj = j == G || (j < G && lbfgs_held(j & (M - 1), head, k, m));
                        double u = j < NB ? s_gram[G * NB + j] : 0.0, coef = j == G ? 1.0 : 0.0, a_mine = 0.0;
                        for (int i = k - 1; i >= 0; --i) {
                            const int c = (head + i) % m;
                            const double ai = __shfl(u, c) / s_gram[c * NB + M + c];
                            if (j == c) a_mine = ai;
                            if (j == M + c) coef -= ai;
                            if (j < NB) u -= ai * s_gram[(M + c) * NB + j];
                        }
                        const int cn = (head + k - 1) % m;
                        const double gamma = s_gram[cn * NB + M + cn] / s_gram[(M + cn) * NB + M + cn];
                        u *= gamma;
                        coef *= gamma;
                        for (int i = 0; i < k; ++i) {
                            const int c = (head + i) % m;
                            const double t = __shfl(a_mine, c) - __shfl(u, M + c) / s_gram[c * NB + M + c];
                            if (j == c) coef += t;
                            if (j < NB) u += t * s_gram[c * NB + j];
                        }
                        const double gdn = -__shfl(u, G);
                        if (j < NB) s_coef[j] = hj ? coef : 0.0;
                        if (j == 0) s_gd = gdn;
                    }
                    __syncthreads();
                    const double gdn = s_gd;
                    if (gdn < 0.0) {
                        steep = false;
                        gd = gdn;
                        alpha0 = 1.0;
                    } else {  // not a descent direction: the history goes
                        k = 0;
                        head = 0;
                    }
                }
            }
        } else if (first) {
            status = CMAX_LBFGS_NONFINITE_START;
            done = true;
            code = CMAX_LBFGS_CODE_START;
            L_a = L;
            ginf_a = (double)NAN;
            for (int p = tid; p < nx; p += blockDim.x) v.xa[p] = a.x[p];
        } else {
            n_ls += 1;
            code = CMAX_LBFGS_CODE_REJECTED;
            if (n_ls > a.max_ls && k == 0) {
                status = CMAX_LBFGS_LINESEARCH;
                done = true;
                for (int p = tid; p < nx; p += blockDim.x) a.x[p] = v.xa[p];
            } else if (n_ls > a.max_ls) {
                code = CMAX_LBFGS_CODE_RESET;
                k = 0;
                head = 0;
                n_ls = 0;
                choose = true;
            } else {
                alpha *= a.shrink;
                for (int p = tid; p < nx; p += blockDim.x) a.x[p] = lbfgs_trial(v.xa[p], alpha, v.d[p], v.x0[p], a.max_move);
            }
        }
        if (accept && !choose) {  // converged: the accepted point is stored, nothing else
            for (int p = tid; p < nx; p += blockDim.x) {
                v.xa[p] = a.x[p];
                v.ga[p] = grad[p];
            }
        }
        if (choose) {
            if (steep) {
                gd = -gg_a;
                alpha0 = fmin(1.0, a.step0 / g1_a);
            }
            double tmin = (double)INFINITY;
            for (int p = tid; p < nx; p += blockDim.x) {
                double g, xa, x0, sp = 0.0, yp = 0.0;
                if (accept && !stored) {
                    g = grad[p];
                    xa = a.x[p];
                    x0 = first ? xa : v.x0[p];
                    if (!first) {
                        sp = xa - v.xa[p];
                        yp = g - v.ga[p];
                    }
                    if (push) {
                        v.S[(int64_t)nslot * nx + p] = sp;
                        v.Y[(int64_t)nslot * nx + p] = yp;
                    }
                    v.xa[p] = xa;
                    v.ga[p] = g;
                    if (first) v.x0[p] = xa;
                } else {
                    g = v.ga[p];
                    xa = v.xa[p];
                    x0 = v.x0[p];
                }
                double dp = -g;
                if (!steep && a.two_loop) {
                    dp = v.d[p];
                } else if (!steep) {
                    double r = 0.0;
                    for (int i = 0; i < k; ++i) {  // oldest to newest, then g: one fixed order
                        const int c = (head + i) % m;
                        const double sv = c == nslot ? sp : v.S[(int64_t)c * nx + p], yv = c == nslot ? yp : v.Y[(int64_t)c * nx + p];
                        r += s_coef[c] * sv + s_coef[M + c] * yv;
                    }
                    dp = -(r + s_coef[G] * g);
                }
                v.d[p] = dp;
                const double lim = dp > 0.0 ? (x0 + a.max_move - xa) / dp : (dp < 0.0 ? (x0 - a.max_move - xa) / dp : (double)INFINITY);
                tmin = fmin(tmin, lim);
            }
            tmin = wave_min_all(tmin);
            if (lane == 0) s_min[wid] = tmin;
            __syncthreads();
            alpha = fmin(alpha0, fmin(fmin(s_min[0], s_min[1]), fmin(s_min[2], s_min[3])));
            if (alpha > 0.0) {
                for (int p = tid; p < nx; p += blockDim.x) a.x[p] = lbfgs_trial(v.xa[p], alpha, v.d[p], v.x0[p], a.max_move);
            } else {
                status = CMAX_LBFGS_BOX;
                done = true;
                for (int p = tid; p < nx; p += blockDim.x) a.x[p] = v.xa[p];
            }
        }
        if (done) used = a.e + 1;
    }
    if (last && a.has_trace)
        for (int p = tid; p < nx; p += blockDim.x) v.trace[(int64_t)a.n_eval * nx + p] = v.xa[p];
    __syncthreads();  // (every thread has read the control block)
    if (tid == 0) {
        v.loss[a.e] = done_prev ? (double)NAN : L;
        v.alpha[a.e] = done_prev ? 0.0 : alpha_e;
        v.code[a.e] = code;
        if (!done_prev) {
            v.ctrl[kLbDone] = done ? 1.0 : 0.0;
            v.ctrl[kLbStatus] = (double)status;
            v.ctrl[kLbLa] = L_a;
            v.ctrl[kLbAlpha] = alpha;
            v.ctrl[kLbGd] = gd;
            v.ctrl[kLbNls] = (double)n_ls;
            v.ctrl[kLbNiter] = (double)n_iter;
            v.ctrl[kLbUsed] = (double)used;
            v.ctrl[kLbK] = (double)k;
            v.ctrl[kLbHead] = (double)head;
            v.ctrl[kLbGinf] = ginf_a;
            v.ctrl[kLbG1] = g1_a;
            v.ctrl[kLbGg] = gg_a;
            v.ctrl[kLbLastAlpha] = last_alpha;
        }
        if (last && a.res_pinned) {
            a.res_pinned[0] = L_a;
            a.res_pinned[1] = ginf_a;
            a.res_pinned[2] = last_alpha;
            a.res_pinned[3] = (double)n_iter;
            a.res_pinned[4] = (double)(done ? used : a.n_eval);
            a.res_pinned[5] = (double)status;
        }
    }
    if (last && a.flag) {
        __threadfence_system();
        __syncthreads();
        if (tid == 0) *a.flag = a.seq_src ? a.seq_src[0] : a.seq;
    }
}

int launch_lbfgs_step(const LbfgsArgs &a_in, const double *loss, const double *grad, hipStream_t s) {
    static const bool two_loop = getenv("CMAX_LBFGS_TWO_LOOP") != nullptr;  // (tools/probe_lbfgs.py: the textbook recursion, for its cost)
    LbfgsArgs a = a_in;
    a.two_loop = two_loop ? 1 : 0;
    hipLaunchKernelGGL(k_lbfgs_step, dim3(1), dim3(256), 0, s, a, loss, grad);
    CMAX_CHECK_LAUNCH();
    return 0;
}

}  // namespace cmax

struct __attribute__((visibility("hidden"))) cmax_patch_plan_s {  // (hidden: its implicit destructor is no export)
    cmax_handle_t handle = nullptr;
    cmax_patch_objective_t d;
    int nx = 0;            // 2 * ph * pw (basis plan: K; depth plan: Ka + Kb + ph * pw)
    int64_t nflow = 0;     // 2 * H * W
    int64_t nmotion = 0;   // nflow or T * nflow
    cmax::DevBuf<double> x64, flow64, vox64, gacc64, gflow64, gx64, results;
    double *v64 = nullptr;  // (inside x64)
    // time-aware Hessian-vector product (allocated on first use): tangent flow / voxel, tangent of dL/dvoxel, scalars
    cmax::DevBuf<double> dflow64, dvox64, dgacc64, dgflow64, scal;
    cmax::DevBuf<float> motion32, grad32, tan32, gx32;
    // the terms carry motion_dtype == CMAX_F64: motion32 is [2][nmotion], the high plane (the fp32 motion of every other plan) and the low
    // plane of the fp64 flow / voxel the plan holds anyway, written by the same conversion launches and read by K1's fp64 cell decisions
    bool exact = false;
    // What maps x to the dense flow: the patch interpolation P (d.filter_type), or a flow basis B [K][2][H][W] (cmax_basis_plan_create: nx = K,
    // the plan's own copy of the basis in the caller's dtype, max |B_k| per field on the host, the chunk sums of the adjoint)
    int map_kind = cmax::kMapPatch;
    int basis_dtype = CMAX_F32;
    cmax::DevBuf<float> basis32;
    cmax::DevBuf<double> basis64, basis_partial;
    std::vector<double> bmax;
    // ... or the depth map (cmax_depth_plan_create: x = [a | b | s], nx = Ka + Kb + ph pw; the basis buffer holds A then B, basis_partial the
    // chunk sums of k_depth_adj, depth_q its plane q [H,W])
    int Ka = 0, Kb = 0;
    cmax::DevBuf<double> depth_q;
    // cmax_patch_plan_set_flow_regularizer: one more term on F = t (map x), kind CMAX_FLOWREG_NONE = none; the tiles' energies
    cmax_flow_regularizer_t reg = {};
    cmax::DevBuf<double> reg_partial;
    // scale_later: D = P x (flow64 then holds u = t D / s), the scalars and the partial sums of the reductions
    cmax::DevBuf<double> dense64, sl, sl_partial;
    cmax::PinnedBuf<double> h_in, h_out;       // pinned staging: x | v | 2 scalars, loss | grad | run counter (the tail kernel writes h_out through its dev())
    cmax::DevBuf<unsigned long long> seq_dev;  // device-side run counter of the tail kernel
    unsigned long long seq_seen = 0;           // its value after the last completed call
    // cmax_patch_plan_descend (reserved on first use): the tail's output in device memory (loss | grad | counter slot), the descent state
    cmax::DevBuf<double> d_out, descent;
    cmax::PinnedBuf<double> h_res;  // ... and the result block the last step writes (the run counter goes to h_out's slot, like every tail's)
    cmax::DevBuf<double> lbfgs;     // cmax_patch_plan_lbfgs (reserved on first use): the L-BFGS state (cmax_lbfgs.h); d_out and h_res are shared
    // Captured launch sequences (hipGraph), replayed on the plan's own stream: an evaluation is ~25 small launches,
    // host-bound when issued one by one.  Keyed by everything that changes the sequence: the kind of call and the
    // handle's host-side state (which vote buffer is current, which images are already zero, whether the
    // un-warped image is cached, the generation of the packed events).
    struct GraphEntry {
        uint64_t key;
        uint64_t generation;
        hipGraphExec_t exec;
        cmax::HandleEvalState post;  // handle state after the sequence
    };
    std::vector<GraphEntry> graphs;
    hipStream_t own_stream = nullptr;
    hipEvent_t ev_caller = nullptr;
    bool graphs_ok = false;  // hipGraph replay: opt-in (CMAX_PLAN_GRAPHS=1), see run_sequence
    int eager_calls = 0;  // the first calls run eagerly (lazy allocations, caches)
};

using namespace cmax;

namespace {

// Time-sliced batches (the handle holds a communicator, cmax_comm_init): the solver's objective is evaluated the way
// cmax_objective_dist evaluates a fused term -- K1 -> all-reduce(images) -> image kernels -> K3 on this rank's events -- but the
// flow gradient is NOT exchanged (2 H W [T] floats: 7.4 MB at 720p).  Every step from there to the optimiser's gradient is linear
// (weighted sum over the terms, adjoint sweep of the voxel chain, adjoint of the patch interpolation), so each rank carries its
// share through them and the ranks all-reduce 2 n_patch numbers (4 KB for a 16 x 16 grid) in front of the tail kernel.  Loss,
// total variation and everything derived from x are computed redundantly and identically on every rank.
int plan_objective(cmax_patch_plan_s *p, const cmax_objective_t *term, double *result, void *grad, hipStream_t s) {
    if (handle_has_comm(p->handle)) return objective_dist_local_grad(p->handle, term, p->motion32, result, grad, s);
    if (p->exact) return objective_presplit(p->handle, term, p->motion32, result, grad, s);  // (the planes are split already)
    return cmax_objective(p->handle, term, p->motion32, result, grad, s);
}
int plan_objective_hvp(cmax_patch_plan_s *p, const cmax_objective_t *term, void *hv, hipStream_t s) {
    if (handle_has_comm(p->handle)) return objective_hvp_dist_local(p->handle, term, p->motion32, p->tan32, hv, s);
    if (p->exact) return objective_hvp_presplit(p->handle, term, p->motion32, p->tan32, hv, s);
    return cmax_objective_hvp(p->handle, term, p->motion32, p->tan32, hv, s);
}
// C2 of the plan: the gradient (or product) w.r.t. the patch motion, summed over the ranks (a no-op without a communicator)
int plan_reduce_gx(cmax_patch_plan_s *p, const double *gx64, const float *gx32, hipStream_t s) {
    if (!handle_has_comm(p->handle)) return 0;
    if (gx64) return handle_allreduce_sum(p->handle, const_cast<double *>(gx64), (size_t)p->nx, true, s);
    return handle_allreduce_sum(p->handle, const_cast<float *>(gx32), (size_t)p->nx, false, s);
}
// ... of an EVALUATION: the terms' result[8] ride along and leave as rank 0's on every rank (each rank summed its statistics in its own
// order; replicated optimisers must see the same loss bit for bit).  Value-only evaluations exchange the scalars alone.
int plan_reduce_gx_and_results(cmax_patch_plan_s *p, const double *gx64, const float *gx32, hipStream_t s) {
    if (!handle_has_comm(p->handle)) return 0;
    const int n_scalars = 8 * p->d.n_terms;
    if (gx64) return handle_allreduce_sum_with_scalars(p->handle, const_cast<double *>(gx64), (size_t)p->nx, true, p->results, n_scalars, s);
    return handle_allreduce_sum_with_scalars(p->handle, const_cast<float *>(gx32), gx32 ? (size_t)p->nx : 0, false, p->results, n_scalars, s);
}

// D = P x with the plan's filter, and the workgroups' maxima (scale_later)
void launch_patch_to_dense_max(cmax_patch_plan_s *p, const double *src64, hipStream_t s) {
    const cmax_patch_objective_t &d = p->d;
    if (d.filter_type == CMAX_FILTER_NEAREST)
        hipLaunchKernelGGL(k_patch_to_dense_max<CMAX_FILTER_NEAREST>, dim3(sl_grid(p->nflow)), dim3(256), 0, s, src64, d.ph, d.pw, d.pad_h, d.pad_w, d.sw_h, d.sw_w, d.H, d.W,
                           p->dense64, p->sl_partial);
    else
        hipLaunchKernelGGL(k_patch_to_dense_max<CMAX_FILTER_BILINEAR>, dim3(sl_grid(p->nflow)), dim3(256), 0, s, src64, d.ph, d.pw, d.pad_h, d.pad_w, d.sw_h, d.sw_w, d.H, d.W,
                           p->dense64, p->sl_partial);
}

const void *plan_basis(const cmax_patch_plan_s *p) { return p->basis_dtype == CMAX_F64 ? (const void *)p->basis64.get() : (const void *)p->basis32.get(); }

// Basis plan: dst = scale [* *scale_dev] * B src64, as fp32 (both planes when `lo32`) or fp64
int basis_forward(cmax_patch_plan_s *p, const double *src64, double scale, const double *scale_dev, float *dst32, float *lo32, double *dst64, hipStream_t s) {
    const bool b64 = p->basis_dtype == CMAX_F64;
    const void *B = plan_basis(p);
    if (dst64) {
        if (b64) launch_basis_to_dense<double, double>(src64, B, p->nx, p->nflow, scale, scale_dev, dst64, s);
        else launch_basis_to_dense<float, double>(src64, B, p->nx, p->nflow, scale, scale_dev, dst64, s);
    } else if (lo32) {
        if (b64) launch_basis_to_dense_split<double>(src64, B, p->nx, p->nflow, scale, scale_dev, dst32, lo32, s);
        else launch_basis_to_dense_split<float>(src64, B, p->nx, p->nflow, scale, scale_dev, dst32, lo32, s);
    } else {
        if (b64) launch_basis_to_dense<double, float>(src64, B, p->nx, p->nflow, scale, scale_dev, dst32, s);
        else launch_basis_to_dense<float, float>(src64, B, p->nx, p->nflow, scale, scale_dev, dst32, s);
    }
    CMAX_CHECK_LAUNCH();
    return 0;
}

DepthGeom plan_depth_geom(const cmax_patch_plan_s *p) {
    const cmax_patch_objective_t &d = p->d;
    return DepthGeom{d.ph, d.pw, d.pad_h, d.pad_w, d.sw_h, d.sw_w, d.H, d.W};
}
// the plan's copy of A, and of B behind it, as typed by basis_dtype
const void *plan_depth_B(const cmax_patch_plan_s *p) {
    const int64_t off = (int64_t)p->Ka * p->nflow;
    return p->basis_dtype == CMAX_F64 ? (const void *)(p->basis64.get() + off) : (const void *)(p->basis32.get() + off);
}

// Depth plan: dst = scale [* *scale_dev] * D(src64), src64 = [a | b | s], as fp32 (both planes when `lo32`) or fp64
int depth_forward(cmax_patch_plan_s *p, const double *src64, double scale, const double *scale_dev, float *dst32, float *lo32, double *dst64, hipStream_t s) {
    const bool b64 = p->basis_dtype == CMAX_F64;
    const void *A = plan_basis(p), *B = plan_depth_B(p);
    const DepthGeom g = plan_depth_geom(p);
    const int Ka = p->Ka, Kb = p->Kb;
    const double *a = src64, *b = src64 + Ka, *sg = src64 + Ka + Kb;
    if (dst64) {
        if (b64) launch_depth_to_dense<double, double>(a, b, sg, A, B, Ka, Kb, g, scale, scale_dev, dst64, s);
        else launch_depth_to_dense<float, double>(a, b, sg, A, B, Ka, Kb, g, scale, scale_dev, dst64, s);
    } else if (lo32) {
        if (b64) launch_depth_to_dense_split<double>(a, b, sg, A, B, Ka, Kb, g, scale, scale_dev, dst32, lo32, s);
        else launch_depth_to_dense_split<float>(a, b, sg, A, B, Ka, Kb, g, scale, scale_dev, dst32, lo32, s);
    } else {
        if (b64) launch_depth_to_dense<double, float>(a, b, sg, A, B, Ka, Kb, g, scale, scale_dev, dst32, s);
        else launch_depth_to_dense<float, float>(a, b, sg, A, B, Ka, Kb, g, scale, scale_dev, dst32, s);
    }
    CMAX_CHECK_LAUNCH();
    return 0;
}

// ... its adjoint at x = x64 into gx64 [a | b | s] (SECOND: the second-order adjoint along v64 for the seeds (g, dg)); always fp64
template <typename TG, bool SECOND>
int depth_adjoint(cmax_patch_plan_s *p, const TG *g, const TG *dg, hipStream_t s) {
    const void *A = plan_basis(p), *B = plan_depth_B(p);
    const DepthGeom geo = plan_depth_geom(p);
    const int Ka = p->Ka, Kb = p->Kb;
    const double *x = p->x64, *v = p->v64;
    if (p->basis_dtype == CMAX_F64)
        launch_depth_adj<double, TG, SECOND>(g, dg, x, x + Ka + Kb, v, v + Ka + Kb, A, B, Ka, Kb, geo, p->basis_partial, p->depth_q, p->gx64, p->gx64 + Ka + Kb, s);
    else
        launch_depth_adj<float, TG, SECOND>(g, dg, x, x + Ka + Kb, v, v + Ka + Kb, A, B, Ka, Kb, geo, p->basis_partial, p->depth_q, p->gx64, p->gx64 + Ka + Kb, s);
    CMAX_CHECK_LAUNCH();
    return 0;
}

// The plan's map x -> dense flow, unscaled, in fp64 (the patch interpolation with the plan's filter, the basis, or the depth map)
int map_forward64(cmax_patch_plan_s *p, const double *src64, double *dst64, hipStream_t s) {
    const cmax_patch_objective_t &d = p->d;
    if (p->map_kind == kMapDepth) return depth_forward(p, src64, 1.0, nullptr, nullptr, nullptr, dst64, s);
    if (p->map_kind == kMapBasis) return basis_forward(p, src64, 1.0, nullptr, nullptr, nullptr, dst64, s);
    return cmax_patch_to_dense_filter(src64, CMAX_F64, d.ph, d.pw, d.pad_h, d.pad_w, d.sw_h, d.sw_w, d.H, d.W, d.filter_type, 0, dst64, s);
}

// ... and its adjoint on a flow gradient in fp32 or fp64: the result is returned through the pointer of its dtype (the patch adjoint
// answers in the dtype of its input, the basis adjoint and the depth adjoint -- taken at the x the plan holds in x64 -- always in fp64)
int map_adjoint(cmax_patch_plan_s *p, const float *g32, const double *g64, const double **gx64, const float **gx32, hipStream_t s) {
    const cmax_patch_objective_t &d = p->d;
    if (p->map_kind == kMapDepth) {
        int rc = g32 ? depth_adjoint<float, false>(p, g32, nullptr, s) : depth_adjoint<double, false>(p, g64, nullptr, s);
        if (!rc) *gx64 = p->gx64;
        return rc;
    }
    if (p->map_kind == kMapBasis) {
        const bool b64 = p->basis_dtype == CMAX_F64;
        const void *B = plan_basis(p);
        if (g32) {
            if (b64) launch_basis_adj<double, float>(g32, B, p->nx, p->nflow, p->basis_partial, p->gx64, s);
            else launch_basis_adj<float, float>(g32, B, p->nx, p->nflow, p->basis_partial, p->gx64, s);
        } else {
            if (b64) launch_basis_adj<double, double>(g64, B, p->nx, p->nflow, p->basis_partial, p->gx64, s);
            else launch_basis_adj<float, double>(g64, B, p->nx, p->nflow, p->basis_partial, p->gx64, s);
        }
        CMAX_CHECK_LAUNCH();
        *gx64 = p->gx64;
        return 0;
    }
    if (g32) {
        int rc = cmax_patch_to_dense_filter(g32, CMAX_F32, d.ph, d.pw, d.pad_h, d.pad_w, d.sw_h, d.sw_w, d.H, d.W, d.filter_type, 1, p->gx32, s);
        if (!rc) *gx32 = p->gx32;
        return rc;
    }
    int rc = cmax_patch_to_dense_filter(g64, CMAX_F64, d.ph, d.pw, d.pad_h, d.pad_w, d.sw_h, d.sw_w, d.H, d.W, d.filter_type, 1, p->gx64, s);
    if (!rc) *gx64 = p->gx64;
    return rc;
}

bool plan_has_reg(const cmax_patch_plan_s *p) { return p->reg.kind != CMAX_FLOWREG_NONE; }
int plan_refuse_reg_comm(const cmax_patch_plan_s *p, const char *who) {
    if (!plan_has_reg(p) || !handle_has_comm(p->handle)) return 0;
    set_error("%s: the plan's flow regulariser is not built for time-sliced batches (the handle holds a communicator): the term would be counted once per rank", who);
    return CMAX_EUNSUPPORTED;
}

// The flow regulariser on F = t (map x) in fp64, before any rounding: its value into the fifth result slot and, with `acc`, weight * dR/dF
// added into that fp64 [2,H,W] accumulator.  A time-aware plan holds F in flow64 already; any other plan maps x once more, unscaled, and
// the kernel scales as it stages.
int plan_flowreg(cmax_patch_plan_s *p, double *acc, hipStream_t s) {
    const cmax_patch_objective_t &d = p->d;
    double scale = 1.0;
    if (!d.time_aware) {
        int rc = map_forward64(p, p->x64, p->flow64, s);
        if (rc) return rc;
        scale = d.t_scale;
    }
    launch_flowreg<double>(p->reg, p->flow64, scale, d.H, d.W, p->reg_partial, p->results + 8 * 4, acc, 1, p->reg.weight, s);
    CMAX_CHECK_LAUNCH();
    return 0;
}

// x (host) -> fp32 motion of the fused objective: flow [2,H,W] or voxel [T,2,H,W] in pixel per normalised time.
// Leaves the fp64 flow (scaled) in flow64 and, when time-aware, the fp64 voxel in vox64.
int forward_motion(cmax_patch_plan_s *p, const double *src64, double scale, const double *scale_dev, float *dst32, hipStream_t s) {
    const cmax_patch_objective_t &d = p->d;
    const int grid = div_up(p->nflow, 256);
    const bool split = p->exact && dst32 == p->motion32;  // the motion of an exact plan (not its tangent): both planes, in the launches below
    const bool nearest = d.filter_type == CMAX_FILTER_NEAREST;
    float *lo32 = dst32 + p->nmotion;
    if (p->map_kind == kMapBasis || p->map_kind == kMapDepth) {  // these kernels scale (scale_dev included) and round in the launch that sums
        const bool depth = p->map_kind == kMapDepth;
        if (!d.time_aware)
            return depth ? depth_forward(p, src64, scale, scale_dev, dst32, split ? lo32 : nullptr, nullptr, s)
                         : basis_forward(p, src64, scale, scale_dev, dst32, split ? lo32 : nullptr, nullptr, s);
        int rc = depth ? depth_forward(p, src64, scale, scale_dev, nullptr, nullptr, p->flow64, s)
                       : basis_forward(p, src64, scale, scale_dev, nullptr, nullptr, p->flow64, s);
        if (rc) return rc;
        bool wrote32 = false;  // the voxel on the displacement field, as the patch plan's time-aware branch below
        rc = voxel_construct_f64_f32(p->flow64, d.T, d.t0, d.H, d.W, d.scheme, p->vox64, split ? nullptr : dst32, split ? nullptr : &wrote32, s);
        if (rc) return rc;
        if (split) hipLaunchKernelGGL(k_convert_split, dim3(div_up(p->nmotion, 256)), dim3(256), 0, s, p->vox64, p->nmotion, 1.0, (const double *)nullptr, dst32, lo32);
        else if (!wrote32) hipLaunchKernelGGL((k_convert_scale<float, double>), dim3(div_up(p->nmotion, 256)), dim3(256), 0, s, p->vox64, p->nmotion, 1.0, (const double *)nullptr, dst32);
        CMAX_CHECK_LAUNCH();
        return 0;
    }
    if (!d.time_aware && !scale_dev && split) {
        if (nearest) hipLaunchKernelGGL(k_patch_to_dense_split<CMAX_FILTER_NEAREST>, dim3(grid), dim3(256), 0, s, src64, d.ph, d.pw, d.pad_h, d.pad_w, d.sw_h, d.sw_w, d.H, d.W, dst32, lo32, scale);
        else hipLaunchKernelGGL(k_patch_to_dense_split<CMAX_FILTER_BILINEAR>, dim3(grid), dim3(256), 0, s, src64, d.ph, d.pw, d.pad_h, d.pad_w, d.sw_h, d.sw_w, d.H, d.W, dst32, lo32, scale);
        CMAX_CHECK_LAUNCH();
        return 0;
    }
    if (!d.time_aware && !scale_dev) {  // patch grid -> fp32 flow * scale in one kernel
        if (nearest) hipLaunchKernelGGL((k_patch_to_dense<double, float, CMAX_FILTER_NEAREST>), dim3(grid), dim3(256), 0, s, src64, d.ph, d.pw, d.pad_h, d.pad_w, d.sw_h, d.sw_w,
                                        d.H, d.W, dst32, scale);
        else hipLaunchKernelGGL((k_patch_to_dense<double, float, CMAX_FILTER_BILINEAR>), dim3(grid), dim3(256), 0, s, src64, d.ph, d.pw, d.pad_h, d.pad_w, d.sw_h, d.sw_w,
                                d.H, d.W, dst32, scale);
        CMAX_CHECK_LAUNCH();
        return 0;
    }
    if (d.time_aware && d.scale_later && !scale_dev) {
        // D = P x and s = max D; u = t D / s (tie count on the way); V = C(u); fp32 motion s V, s read from device memory
        launch_patch_to_dense_max(p, src64, s);
        hipLaunchKernelGGL(k_sl_scale, dim3(sl_grid(p->nflow)), dim3(256), 0, s, p->dense64, (const double *)nullptr, p->nflow, scale, sl_grid(p->nflow),
                           p->sl, p->flow64, p->sl_partial);
        CMAX_CHECK_LAUNCH();
        int rc = voxel_construct_f64_f32(p->flow64, d.T, d.t0, d.H, d.W, d.scheme, p->vox64, nullptr, nullptr, s);
        if (rc) return rc;
        if (split) hipLaunchKernelGGL(k_convert_split, dim3(div_up(p->nmotion, 256)), dim3(256), 0, s, p->vox64, p->nmotion, 1.0, (const double *)p->sl, dst32, lo32);
        else hipLaunchKernelGGL((k_convert_scale<float, double>), dim3(div_up(p->nmotion, 256)), dim3(256), 0, s, p->vox64, p->nmotion, 1.0, (const double *)p->sl, dst32);
        CMAX_CHECK_LAUNCH();
        return 0;
    }
    if (d.time_aware && !scale_dev) {
        // patch grid -> fp64 displacement field (x t_scale) in one kernel; the voxel is built on the displacement
        // field (patch_contrast_pyramid.py:452, 499-515) and leaves the chain kernel in fp64 and fp32 at once
        if (nearest) hipLaunchKernelGGL((k_patch_to_dense<double, double, CMAX_FILTER_NEAREST>), dim3(grid), dim3(256), 0, s, src64, d.ph, d.pw, d.pad_h, d.pad_w, d.sw_h, d.sw_w,
                                        d.H, d.W, p->flow64, scale);
        else hipLaunchKernelGGL((k_patch_to_dense<double, double, CMAX_FILTER_BILINEAR>), dim3(grid), dim3(256), 0, s, src64, d.ph, d.pw, d.pad_h, d.pad_w, d.sw_h, d.sw_w,
                                d.H, d.W, p->flow64, scale);
        CMAX_CHECK_LAUNCH();
        bool wrote32 = false;
        // (an exact plan: the chain kernel writes no low plane -- where it would have written the fp32 copy itself, the conversion is this plan's one launch more)
        int rc = voxel_construct_f64_f32(p->flow64, d.T, d.t0, d.H, d.W, d.scheme, p->vox64, split ? nullptr : dst32, split ? nullptr : &wrote32, s);
        if (rc) return rc;
        if (split) {
            hipLaunchKernelGGL(k_convert_split, dim3(div_up(p->nmotion, 256)), dim3(256), 0, s, p->vox64, p->nmotion, 1.0, (const double *)nullptr, dst32, lo32);
            CMAX_CHECK_LAUNCH();
        } else if (!wrote32) {
            hipLaunchKernelGGL((k_convert_scale<float, double>), dim3(div_up(p->nmotion, 256)), dim3(256), 0, s, p->vox64, p->nmotion, 1.0, (const double *)nullptr, dst32);
            CMAX_CHECK_LAUNCH();
        }
        return 0;
    }
    int rc = cmax_patch_to_dense_filter(src64, CMAX_F64, d.ph, d.pw, d.pad_h, d.pad_w, d.sw_h, d.sw_w, d.H, d.W, d.filter_type, 0, p->flow64, s);
    if (rc) return rc;
    if (!d.time_aware) {
        if (split) hipLaunchKernelGGL(k_convert_split, dim3(grid), dim3(256), 0, s, p->flow64, p->nflow, scale, scale_dev, dst32, lo32);
        else hipLaunchKernelGGL((k_convert_scale<float, double>), dim3(grid), dim3(256), 0, s, p->flow64, p->nflow, scale, scale_dev, dst32);
        CMAX_CHECK_LAUNCH();
        return 0;
    }
    hipLaunchKernelGGL((k_convert_scale<double, double>), dim3(grid), dim3(256), 0, s, p->flow64, p->nflow, scale, scale_dev, p->flow64);
    CMAX_CHECK_LAUNCH();
    rc = cmax_voxel_construct(p->flow64, CMAX_F64, d.T, d.t0, d.H, d.W, d.scheme, p->vox64, s);
    if (rc) return rc;
    if (split) hipLaunchKernelGGL(k_convert_split, dim3(div_up(p->nmotion, 256)), dim3(256), 0, s, p->vox64, p->nmotion, 1.0, (const double *)nullptr, dst32, lo32);
    else hipLaunchKernelGGL((k_convert_scale<float, double>), dim3(div_up(p->nmotion, 256)), dim3(256), 0, s, p->vox64, p->nmotion, 1.0, (const double *)nullptr, dst32);
    CMAX_CHECK_LAUNCH();
    return 0;
}

// gradient of the fused terms w.r.t. the patch motion (without t_scale): gx64 or gx32 (returned through the pointers)
int backward_motion(cmax_patch_plan_s *p, const double **gx64, const float **gx32, double *weight_scale, hipStream_t s) {
    const cmax_patch_objective_t &d = p->d;
    *gx64 = nullptr;
    *gx32 = nullptr;
    *weight_scale = 1.0;
    if (d.n_terms == 1 && !d.time_aware && !plan_has_reg(p)) {
        // one term on the dense flow: the adjoint of the interpolation reads the fp32 flow gradient as it is
        // (fp64 accumulation inside), the term's weight is applied by the tail
        int rc = map_adjoint(p, p->grad32, nullptr, gx64, gx32, s);
        if (rc) return rc;
        *weight_scale = d.weight[0];
        return 0;
    }
    const double *gflow = p->gacc64;
    if (d.time_aware && d.scale_later) {
        // g_D = t h + kappa (<g_M, V> - <h, u>), h = J^T g_M: the first product before the sweep clobbers g_M, the second after it
        DotJobs pre = {{p->gacc64}, {p->vox64}, 1};
        hipLaunchKernelGGL(k_sl_dots, dim3(sl_grid(p->nmotion)), dim3(256), 0, s, pre, p->nmotion, 0, p->sl_partial);
        CMAX_CHECK_LAUNCH();
        int rc = voxel_construct_adj_f64(p->vox64, d.T, d.t0, d.H, d.W, d.scheme, p->gacc64, s, handle_is_deterministic(p->handle));
        if (rc) return rc;
        const double *h = p->gacc64 + (int64_t)d.t0 * p->nflow;
        DotJobs post = {{h}, {p->flow64}, 1};
        hipLaunchKernelGGL(k_sl_dots, dim3(sl_grid(p->nflow)), dim3(256), 0, s, post, p->nflow, kSlPost, p->sl_partial);
        SlCoef cf = {{1.0, 0.0, 0.0, -1.0, 0.0}, sl_grid(p->nmotion), sl_grid(p->nflow), sl_grid(p->nflow)};
        hipLaunchKernelGGL(k_sl_grad_dense, dim3(div_up(p->nflow, 256)), dim3(256), 0, s, h, p->dense64, p->nflow, d.t_scale, p->sl, p->sl_partial, cf,
                           p->gflow64);
        CMAX_CHECK_LAUNCH();
        gflow = p->gflow64;  // (t is applied above: the tail gets gscale 1)
    } else if (d.time_aware) {  // the sweep leaves dL/dF in bin t0 of the gradient voxel: read it there
        int rc = voxel_construct_adj_f64(p->vox64, d.T, d.t0, d.H, d.W, d.scheme, p->gacc64, s, handle_is_deterministic(p->handle));
        if (rc) return rc;
        if (plan_has_reg(p)) {  // one more term on F: where the map's adjoint reads
            rc = plan_flowreg(p, p->gacc64 + (int64_t)d.t0 * p->nflow, s);
            if (rc) return rc;
        }
        gflow = p->gacc64 + (int64_t)d.t0 * p->nflow;
    }
    return map_adjoint(p, nullptr, gflow, gx64, gx32, s);
}

// Everything between the input and the output of one evaluation, enqueued on `s` (no synchronisation).  x_src: pinned host memory the
// leading copy brings x from (nullptr: x64 holds x already -- the descent's iterate); out: where the tail writes loss | gradient | run
// counter (the device view of the pinned output, or the descent's device buffer).
int enqueue_evaluate(cmax_patch_plan_s *p, bool tv, bool want_grad, hipStream_t s, const double *x_src, double *out) {
    const cmax_patch_objective_t &d = p->d;
    if (x_src) CMAX_CHECK_HIP(hipMemcpyAsync(p->x64, x_src, (size_t)p->nx * sizeof(double), hipMemcpyHostToDevice, s));
    int rc = forward_motion(p, p->x64, d.t_scale, nullptr, p->motion32, s);
    if (rc) return rc;
    const bool reg = plan_has_reg(p);
    const bool accumulate = want_grad && (reg || !(d.n_terms == 1 && !d.time_aware));  // (the regulariser adds into gacc64)
    for (int i = 0; i < d.n_terms; ++i) {
        rc = plan_objective(p, &d.term[i], p->results + 8 * i, want_grad ? p->grad32 : nullptr, s);
        if (rc) return rc;
        if (accumulate) {
            hipLaunchKernelGGL(k_accumulate, dim3(div_up(p->nmotion, 256)), dim3(256), 0, s, p->grad32, p->nmotion, d.weight[i], i == 0 ? 1 : 0, p->gacc64);
            CMAX_CHECK_LAUNCH();
        }
    }
    if (reg && !(d.time_aware && want_grad)) {  // (a time-aware gradient: behind the adjoint sweep, in backward_motion)
        rc = plan_flowreg(p, want_grad ? (double *)p->gacc64 : nullptr, s);
        if (rc) return rc;
    }
    const double *gx64 = nullptr;
    const float *gx32 = nullptr;
    double wscale = 1.0;
    if (want_grad) rc = backward_motion(p, &gx64, &gx32, &wscale, s);
    if (!rc && d.n_terms > 0) rc = plan_reduce_gx_and_results(p, gx64, gx32, s);
    else if (!rc && want_grad) rc = plan_reduce_gx(p, gx64, gx32, s);
    if (rc) return rc;
    FinalParams fp;
    fp.n_terms = d.n_terms;
    fp.flag_slot = 1 + (int)p->nx;
    fp.with_tv = tv ? 1 : 0;
    fp.nx = want_grad ? p->nx : 0;
    fp.ph = d.ph;
    fp.pw = d.pw;
    fp.tv_crop = d.tv_omit_boundary && d.ph > 2 && d.pw > 2;  // total_variation.py:123-125
    for (int i = 0; i < 4; ++i) fp.weight[i] = d.weight[i];
    fp.tv_weight = d.tv_weight;
    fp.gscale = d.t_scale * wscale;  // d(flow * t_scale) / d flow
    fp.reg_weight = reg ? p->reg.weight : 0.0;
    if (d.time_aware && d.scale_later) fp.gscale = 1.0;
    const double *ok_dev = d.time_aware && d.scale_later ? p->sl + 1 : nullptr;
    hipLaunchKernelGGL(k_patch_tail, dim3(1), dim3(256), 0, s, fp, p->results, p->x64, gx64, gx32, (const double *)nullptr, out, p->seq_dev, ok_dev);
    CMAX_CHECK_LAUNCH();
    return 0;
}

// Hessian-vector product: h_in = x | v | 1/|v|_inf | |v|_inf
// Time-aware objective: x -> F = t P x -> voxel V(F) -> L(V).  With g_V = dL/dV, H_VV the Hessian of the fused
// terms (cmax_objective_hvp) and J = dV/dF:
//   H_x v = t P^T [ J^T H_VV J (t P v) + (dJ[t P v])^T g_V ]
// J (t P v) is the tangent voxel of the dual-number sweep; the bracket is what its adjoint sweep returns for the
// seeds (g_V, H_VV dV).  The tangent handed to cmax_objective_hvp must have max-norm <= 1, hence the device-side
// max |dV| (the propagation can amplify the tangent).
int enqueue_hvp_time_aware(cmax_patch_plan_s *p, hipStream_t s) {
    const cmax_patch_objective_t &d = p->d;
    CMAX_CHECK_HIP(hipMemcpyAsync(p->x64, p->h_in, (2 * (size_t)p->nx + 2) * sizeof(double), hipMemcpyHostToDevice, s));
    const double *inv_vmax = p->x64 + 2 * p->nx, *vmax = inv_vmax + 1;
    const int fgrid = div_up(p->nflow, 256), mgrid = div_up(p->nmotion, 256);
    // F = t P x,  dF = t P v / |v|_inf
    int rc = map_forward64(p, p->x64, p->flow64, s);
    if (rc) return rc;
    rc = map_forward64(p, p->v64, p->dflow64, s);
    if (rc) return rc;
    hipLaunchKernelGGL((k_convert_scale<double, double>), dim3(fgrid), dim3(256), 0, s, p->flow64, p->nflow, d.t_scale, (const double *)nullptr, p->flow64);
    hipLaunchKernelGGL((k_convert_scale<double, double>), dim3(fgrid), dim3(256), 0, s, p->dflow64, p->nflow, d.t_scale, inv_vmax, p->dflow64);
    CMAX_CHECK_LAUNCH();
    rc = cmax_voxel_construct_tan(p->flow64, p->dflow64, CMAX_F64, d.T, d.t0, d.H, d.W, d.scheme, p->vox64, p->dvox64, s);
    if (rc) return rc;
    // fp32 motion and unit-norm fp32 tangent of the fused terms
    unsigned long long *bits = reinterpret_cast<unsigned long long *>(p->scal + 2);
    CMAX_CHECK_HIP(hipMemsetAsync(bits, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_absmax, dim3(mgrid < 256 ? mgrid : 256), dim3(256), 0, s, p->dvox64, p->nmotion, bits);
    hipLaunchKernelGGL(k_absmax_finish, dim3(1), dim3(1), 0, s, bits, p->scal);
    if (p->exact) hipLaunchKernelGGL(k_convert_split, dim3(mgrid), dim3(256), 0, s, p->vox64, p->nmotion, 1.0, (const double *)nullptr, p->motion32, p->motion32 + p->nmotion);
    else hipLaunchKernelGGL((k_convert_scale<float, double>), dim3(mgrid), dim3(256), 0, s, p->vox64, p->nmotion, 1.0, (const double *)nullptr, p->motion32);
    hipLaunchKernelGGL((k_convert_scale<float, double>), dim3(mgrid), dim3(256), 0, s, p->dvox64, p->nmotion, 1.0, p->scal + 1, p->tan32);
    CMAX_CHECK_LAUNCH();
    for (int i = 0; i < d.n_terms; ++i) {
        rc = plan_objective(p, &d.term[i], p->results + 8 * i, p->grad32, s);  // g_V (time-sliced batch: this rank's share, like everything below)
        if (rc) return rc;
        hipLaunchKernelGGL(k_accumulate, dim3(mgrid), dim3(256), 0, s, p->grad32, p->nmotion, d.weight[i], i == 0 ? 1 : 0, p->gacc64, (const double *)nullptr);
        CMAX_CHECK_LAUNCH();
        rc = plan_objective_hvp(p, &d.term[i], p->grad32, s);  // H_VV dV / max|dV|
        if (rc) return rc;
        hipLaunchKernelGGL(k_accumulate, dim3(mgrid), dim3(256), 0, s, p->grad32, p->nmotion, d.weight[i], i == 0 ? 1 : 0, p->dgacc64, (const double *)p->scal);
        CMAX_CHECK_LAUNCH();
    }
    // the sweep leaves d(dL/dF) in bin t0 of the tangent gradient voxel: the interpolation adjoint reads it there
    rc = voxel_construct_adj_tan_f64(p->vox64, p->dvox64, d.T, d.t0, d.H, d.W, d.scheme, p->gacc64, p->dgacc64, s, handle_is_deterministic(p->handle));
    if (rc) return rc;
    if (plan_has_reg(p)) {  // w (grad^2_F R)[dF] for the same tangent, where the map's adjoint reads
        launch_flowreg_tan<double>(p->reg, p->flow64, p->dflow64, 1.0, 1.0, nullptr, d.H, d.W, p->dgacc64 + (int64_t)d.t0 * p->nflow, 1, p->reg.weight, s);
        CMAX_CHECK_LAUNCH();
    }
    const double *gx64 = nullptr;
    const float *gx32 = nullptr;
    rc = map_adjoint(p, nullptr, p->dgacc64 + (int64_t)d.t0 * p->nflow, &gx64, &gx32, s);
    if (!rc) rc = plan_reduce_gx(p, p->gx64, nullptr, s);
    if (rc) return rc;
    FinalParams fp;
    fp.n_terms = 0;
    fp.flag_slot = 1 + (int)p->nx;
    fp.with_tv = 0;  // total_variation is piecewise linear: zero Hessian almost everywhere
    fp.nx = p->nx;
    fp.ph = d.ph;
    fp.pw = d.pw;
    fp.tv_crop = 0;
    for (int i = 0; i < 4; ++i) fp.weight[i] = 0.0;
    fp.tv_weight = 0.0;
    fp.gscale = d.t_scale;  // the outer t P^T; times |v|_inf from device memory
    hipLaunchKernelGGL(k_patch_tail, dim3(1), dim3(256), 0, s, fp, p->results, p->x64, p->gx64, (const float *)nullptr, vmax, p->h_out.dev(), p->seq_dev);
    CMAX_CHECK_LAUNCH();
    return 0;
}

// ... with scale_later: the map x -> M = s C(t P x / s) and its second-order adjoint as derived above k_patch_to_dense_max.
int enqueue_hvp_scale_later(cmax_patch_plan_s *p, hipStream_t s) {
    const cmax_patch_objective_t &d = p->d;
    CMAX_CHECK_HIP(hipMemcpyAsync(p->x64, p->h_in, (2 * (size_t)p->nx + 2) * sizeof(double), hipMemcpyHostToDevice, s));
    const double *inv_vmax = p->x64 + 2 * p->nx, *vmax = inv_vmax + 1;
    const int fgrid = div_up(p->nflow, 256), mgrid = div_up(p->nmotion, 256);
    // D = P x, s = max D;  Dd = P v;  u = t D / s (flow64);  ud = (t Dd / |v|_inf - u sd) / s (dflow64)
    launch_patch_to_dense_max(p, p->x64, s);
    CMAX_CHECK_LAUNCH();
    int rc = cmax_patch_to_dense_filter(p->v64, CMAX_F64, d.ph, d.pw, d.pad_h, d.pad_w, d.sw_h, d.sw_w, d.H, d.W, d.filter_type, 0, p->dflow64, s);
    if (rc) return rc;
    hipLaunchKernelGGL(k_sl_scale, dim3(sl_grid(p->nflow)), dim3(256), 0, s, p->dense64, (const double *)p->dflow64, p->nflow, d.t_scale, sl_grid(p->nflow),
                       p->sl, p->flow64, p->sl_partial);
    hipLaunchKernelGGL(k_sl_tangent, dim3(fgrid), dim3(256), 0, s, p->flow64, p->dflow64, p->nflow, d.t_scale, inv_vmax, p->sl, p->sl_partial, sl_grid(p->nflow));
    CMAX_CHECK_LAUNCH();
    // V = C(u), W = J ud
    rc = cmax_voxel_construct_tan(p->flow64, p->dflow64, CMAX_F64, d.T, d.t0, d.H, d.W, d.scheme, p->vox64, p->dvox64, s);
    if (rc) return rc;
    // fp32 motion s V; tangent Md = sd V + s W (staged in dgacc64, free until the first product lands there), scaled to unit max-norm
    if (p->exact)
        hipLaunchKernelGGL(k_sl_motion_tangent_split, dim3(mgrid), dim3(256), 0, s, p->vox64, p->dvox64, p->nmotion, p->sl, p->dgacc64, p->motion32,
                           p->motion32 + p->nmotion);
    else hipLaunchKernelGGL(k_sl_motion_tangent, dim3(mgrid), dim3(256), 0, s, p->vox64, p->dvox64, p->nmotion, p->sl, p->dgacc64, p->motion32);
    unsigned long long *bits = reinterpret_cast<unsigned long long *>(p->scal + 2);
    CMAX_CHECK_HIP(hipMemsetAsync(bits, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_absmax, dim3(mgrid < 256 ? mgrid : 256), dim3(256), 0, s, p->dgacc64, p->nmotion, bits);
    hipLaunchKernelGGL(k_absmax_finish, dim3(1), dim3(1), 0, s, bits, p->scal);
    hipLaunchKernelGGL((k_convert_scale<float, double>), dim3(mgrid), dim3(256), 0, s, p->dgacc64, p->nmotion, 1.0, p->scal + 1, p->tan32);
    CMAX_CHECK_LAUNCH();
    for (int i = 0; i < d.n_terms; ++i) {
        rc = plan_objective(p, &d.term[i], p->results + 8 * i, p->grad32, s);  // g_M
        if (rc) return rc;
        hipLaunchKernelGGL(k_accumulate, dim3(mgrid), dim3(256), 0, s, p->grad32, p->nmotion, d.weight[i], i == 0 ? 1 : 0, p->gacc64, (const double *)nullptr);
        CMAX_CHECK_LAUNCH();
        rc = plan_objective_hvp(p, &d.term[i], p->grad32, s);  // H_MM Md / max|Md|
        if (rc) return rc;
        hipLaunchKernelGGL(k_accumulate, dim3(mgrid), dim3(256), 0, s, p->grad32, p->nmotion, d.weight[i], i == 0 ? 1 : 0, p->dgacc64, (const double *)p->scal);
        CMAX_CHECK_LAUNCH();
    }
    // <gd_M, V> and <g_M, W> before the dual sweep clobbers its seeds, <hd, u> and <h, ud> after it
    DotJobs pre = {{p->dgacc64, p->gacc64}, {p->vox64, p->dvox64}, 2};
    hipLaunchKernelGGL(k_sl_dots, dim3(sl_grid(p->nmotion)), dim3(256), 0, s, pre, p->nmotion, 0, p->sl_partial);
    CMAX_CHECK_LAUNCH();
    rc = voxel_construct_adj_tan_f64(p->vox64, p->dvox64, d.T, d.t0, d.H, d.W, d.scheme, p->gacc64, p->dgacc64, s, handle_is_deterministic(p->handle));
    if (rc) return rc;
    const double *h = p->gacc64 + (int64_t)d.t0 * p->nflow, *hd = p->dgacc64 + (int64_t)d.t0 * p->nflow;
    DotJobs post = {{hd, h}, {p->flow64, p->dflow64}, 2};
    hipLaunchKernelGGL(k_sl_dots, dim3(sl_grid(p->nflow)), dim3(256), 0, s, post, p->nflow, kSlPost, p->sl_partial);
    SlCoef cf = {{1.0, 1.0, 0.0, -1.0, -1.0}, sl_grid(p->nmotion), sl_grid(p->nflow), sl_grid(p->nflow)};
    hipLaunchKernelGGL(k_sl_grad_dense, dim3(fgrid), dim3(256), 0, s, hd, p->dense64, p->nflow, d.t_scale, p->sl, p->sl_partial, cf, p->dgflow64);
    CMAX_CHECK_LAUNCH();
    rc = cmax_patch_to_dense_filter(p->dgflow64, CMAX_F64, d.ph, d.pw, d.pad_h, d.pad_w, d.sw_h, d.sw_w, d.H, d.W, d.filter_type, 1, p->gx64, s);
    if (rc) return rc;
    FinalParams fp;
    fp.n_terms = 0;
    fp.flag_slot = 1 + (int)p->nx;
    fp.with_tv = 0;
    fp.nx = p->nx;
    fp.ph = d.ph;
    fp.pw = d.pw;
    fp.tv_crop = 0;
    for (int i = 0; i < 4; ++i) fp.weight[i] = 0.0;
    fp.tv_weight = 0.0;
    fp.gscale = 1.0;  // t is in gd_D; times |v|_inf from device memory
    hipLaunchKernelGGL(k_patch_tail, dim3(1), dim3(256), 0, s, fp, p->results, p->x64, p->gx64, (const float *)nullptr, vmax, p->h_out.dev(), p->seq_dev,
                       (const double *)(p->sl + 1));
    CMAX_CHECK_LAUNCH();
    return 0;
}

// Depth plan (the map x -> D is a product of unknowns: its derivative J depends on x).  With F = t D(x), g_F = dL/dF and v the tangent:
//   H_x v = t [ J^T (H_FF t dD) + (dJ[v])^T g_F ],   dD = J v (k_depth_to_dense_tan)
// -- the second-order adjoint of k_depth_adj on the seeds (g_F, dg_F).  A time-aware plan puts the voxel chain between F and the fused
// terms exactly as enqueue_hvp_time_aware does.  The tangent handed to cmax_objective_hvp is scaled to unit max-norm from a maximum taken
// on the device: no host bound holds for the product (Q ds) (A a), and the scalars the host sends with x | v are not used.
int enqueue_hvp_depth(cmax_patch_plan_s *p, hipStream_t s) {
    const cmax_patch_objective_t &d = p->d;
    CMAX_CHECK_HIP(hipMemcpyAsync(p->x64, p->h_in, (2 * (size_t)p->nx + 2) * sizeof(double), hipMemcpyHostToDevice, s));
    const int mgrid = div_up(p->nmotion, 256);
    const int Ka = p->Ka, Kb = p->Kb;
    const int64_t off0 = d.time_aware ? (int64_t)d.t0 * p->nflow : 0;
    // F = t D(x) -> the fp32 motion (flow64 / vox64 as an evaluation leaves them);  dF = t J v in fp64
    const double *x = p->x64, *v = p->v64;
    if (p->basis_dtype == CMAX_F64)
        launch_depth_to_dense_tan<double, double>(x, x + Ka + Kb, v, v + Ka, v + Ka + Kb, plan_basis(p), plan_depth_B(p), Ka, Kb, plan_depth_geom(p), d.t_scale,
                                                  (double *)p->dflow64, s);
    else
        launch_depth_to_dense_tan<float, double>(x, x + Ka + Kb, v, v + Ka, v + Ka + Kb, plan_basis(p), plan_depth_B(p), Ka, Kb, plan_depth_geom(p), d.t_scale,
                                                 (double *)p->dflow64, s);
    CMAX_CHECK_LAUNCH();
    int rc = 0;
    const double *tan64 = p->dflow64;
    if (d.time_aware) {
        rc = depth_forward(p, p->x64, d.t_scale, nullptr, nullptr, nullptr, p->flow64, s);
        if (rc) return rc;
        rc = cmax_voxel_construct_tan(p->flow64, p->dflow64, CMAX_F64, d.T, d.t0, d.H, d.W, d.scheme, p->vox64, p->dvox64, s);
        if (rc) return rc;
        if (p->exact) hipLaunchKernelGGL(k_convert_split, dim3(mgrid), dim3(256), 0, s, p->vox64, p->nmotion, 1.0, (const double *)nullptr, p->motion32, p->motion32 + p->nmotion);
        else hipLaunchKernelGGL((k_convert_scale<float, double>), dim3(mgrid), dim3(256), 0, s, p->vox64, p->nmotion, 1.0, (const double *)nullptr, p->motion32);
        CMAX_CHECK_LAUNCH();
        tan64 = p->dvox64;
    } else {
        rc = forward_motion(p, p->x64, d.t_scale, nullptr, p->motion32, s);
        if (rc) return rc;
    }
    unsigned long long *bits = reinterpret_cast<unsigned long long *>(p->scal + 2);
    CMAX_CHECK_HIP(hipMemsetAsync(bits, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_absmax, dim3(mgrid < 256 ? mgrid : 256), dim3(256), 0, s, tan64, p->nmotion, bits);
    hipLaunchKernelGGL(k_absmax_finish, dim3(1), dim3(1), 0, s, bits, p->scal);
    hipLaunchKernelGGL((k_convert_scale<float, double>), dim3(mgrid), dim3(256), 0, s, tan64, p->nmotion, 1.0, p->scal + 1, p->tan32);
    CMAX_CHECK_LAUNCH();
    for (int i = 0; i < d.n_terms; ++i) {
        rc = plan_objective(p, &d.term[i], p->results + 8 * i, p->grad32, s);  // g of the motion
        if (rc) return rc;
        hipLaunchKernelGGL(k_accumulate, dim3(mgrid), dim3(256), 0, s, p->grad32, p->nmotion, d.weight[i], i == 0 ? 1 : 0, p->gacc64, (const double *)nullptr);
        CMAX_CHECK_LAUNCH();
        rc = plan_objective_hvp(p, &d.term[i], p->grad32, s);  // H (tangent / its max-norm)
        if (rc) return rc;
        hipLaunchKernelGGL(k_accumulate, dim3(mgrid), dim3(256), 0, s, p->grad32, p->nmotion, d.weight[i], i == 0 ? 1 : 0, p->dgacc64, (const double *)p->scal);
        CMAX_CHECK_LAUNCH();
    }
    if (d.time_aware) {  // the dual sweep leaves g_F and dg_F in bin t0 of the two gradient voxels
        rc = voxel_construct_adj_tan_f64(p->vox64, p->dvox64, d.T, d.t0, d.H, d.W, d.scheme, p->gacc64, p->dgacc64, s, handle_is_deterministic(p->handle));
        if (rc) return rc;
    }
    if (plan_has_reg(p)) {  // one more term on F: w dR/dF into g_F, w (grad^2_F R)[dF] into dg_F
        rc = plan_flowreg(p, p->gacc64 + off0, s);  // (a plan that is not time-aware: flow64 = D(x) unscaled from here on)
        if (rc) return rc;
        launch_flowreg_tan<double>(p->reg, p->flow64, p->dflow64, d.time_aware ? 1.0 : d.t_scale, 1.0, nullptr, d.H, d.W, p->dgacc64 + off0, 1, p->reg.weight, s);
        CMAX_CHECK_LAUNCH();
    }
    rc = depth_adjoint<double, true>(p, p->gacc64 + off0, p->dgacc64 + off0, s);
    if (rc) return rc;
    FinalParams fp;
    fp.n_terms = 0;
    fp.flag_slot = 1 + (int)p->nx;
    fp.with_tv = 0;
    fp.nx = p->nx;
    fp.ph = d.ph;
    fp.pw = d.pw;
    fp.tv_crop = 0;
    for (int i = 0; i < 4; ++i) fp.weight[i] = 0.0;
    fp.tv_weight = 0.0;
    fp.gscale = d.t_scale;  // the outer t J^T (the inner t is in dF)
    hipLaunchKernelGGL(k_patch_tail, dim3(1), dim3(256), 0, s, fp, p->results, p->x64, p->gx64, (const float *)nullptr, (const double *)nullptr, p->h_out.dev(), p->seq_dev);
    CMAX_CHECK_LAUNCH();
    return 0;
}

int enqueue_hvp(cmax_patch_plan_s *p, hipStream_t s) {
    const cmax_patch_objective_t &d = p->d;
    if (p->map_kind == kMapDepth) return enqueue_hvp_depth(p, s);
    if (d.time_aware && d.scale_later) return enqueue_hvp_scale_later(p, s);
    if (d.time_aware) return enqueue_hvp_time_aware(p, s);
    // x64 | v64 | scal64 are one allocation: a single copy brings x, v and the two scalars
    CMAX_CHECK_HIP(hipMemcpyAsync(p->x64, p->h_in, (2 * (size_t)p->nx + 2) * sizeof(double), hipMemcpyHostToDevice, s));
    const double *inv_vmax = p->x64 + 2 * p->nx, *vmax = inv_vmax + 1;
    int rc = forward_motion(p, p->x64, d.t_scale, nullptr, p->motion32, s);
    if (rc) return rc;
    // tangent of the flow, scaled to max-norm <= 1 (the interpolation is a negated convex combination, so
    // |P v|_inf <= |v|_inf): u = (t_scale * |v|_inf) * tan32, and H is linear in u
    rc = forward_motion(p, p->v64, 1.0, inv_vmax, p->tan32, s);
    if (rc) return rc;
    const bool reg = plan_has_reg(p);
    const bool accumulate = reg || !(d.n_terms == 1 && !d.time_aware);
    for (int i = 0; i < d.n_terms; ++i) {
        rc = plan_objective_hvp(p, &d.term[i], p->grad32, s);
        if (rc) return rc;
        if (accumulate) {
            hipLaunchKernelGGL(k_accumulate, dim3(div_up(p->nmotion, 256)), dim3(256), 0, s, p->grad32, p->nmotion, d.weight[i], i == 0 ? 1 : 0, p->gacc64);
            CMAX_CHECK_LAUNCH();
        }
    }
    if (reg) {  // w (grad^2_F R)[P v / |v|_inf] at F = t P x, in fp64: scaled by t^2 |v|_inf with the rest
        rc = map_forward64(p, p->x64, p->flow64, s);
        if (!rc) rc = map_forward64(p, p->v64, p->dflow64, s);
        if (rc) return rc;
        launch_flowreg_tan<double>(p->reg, p->flow64, p->dflow64, d.t_scale, 1.0, inv_vmax, d.H, d.W, p->gacc64, 1, p->reg.weight, s);
        CMAX_CHECK_LAUNCH();
    }
    const double *gx64 = nullptr;
    const float *gx32 = nullptr;
    double wscale = 1.0;
    rc = backward_motion(p, &gx64, &gx32, &wscale, s);
    if (!rc) rc = plan_reduce_gx(p, gx64, gx32, s);
    if (rc) return rc;
    FinalParams fp;
    fp.n_terms = 0;
    fp.flag_slot = 1 + (int)p->nx;
    fp.with_tv = 0;  // total_variation is piecewise linear: zero Hessian almost everywhere
    fp.nx = p->nx;
    fp.ph = d.ph;
    fp.pw = d.pw;
    fp.tv_crop = 0;
    for (int i = 0; i < 4; ++i) fp.weight[i] = 0.0;
    fp.tv_weight = 0.0;
    fp.gscale = d.t_scale * d.t_scale * wscale;  // H_x = t^2 P^T H_flow P (times |v|_inf, from device memory)
    hipLaunchKernelGGL(k_patch_tail, dim3(1), dim3(256), 0, s, fp, p->results, p->x64, gx64, gx32, vmax, p->h_out.dev(), p->seq_dev);
    CMAX_CHECK_LAUNCH();
    return 0;
}

uint64_t state_key(const HandleEvalState &st, int kind) { return handle_state_key(st, kind); }

void drop_graphs(cmax_patch_plan_s *p) {
    for (auto &g : p->graphs) (void)hipGraphExecDestroy(g.exec);
    p->graphs.clear();
}

// The tail kernel bumps a run counter in the pinned output after its results are visible: the slot behind loss | grad, in the host's
// view of h_out or the device's.
static volatile unsigned long long *plan_flag(const cmax_patch_plan_s *p, double *h_out) {
    return reinterpret_cast<volatile unsigned long long *>(h_out + 1 + p->nx);
}

// poll: a few ms at most, then sleep like everybody else.  Whatever the counter says once the stream is done is adopted.
static int wait_for_tail(cmax_patch_plan_s *p, hipStream_t s, bool poll, unsigned long long n_tails = 1ull) {
    const unsigned long long expected = p->seq_seen + n_tails;  // (a descent: one tail per iteration, the last step publishes the counter)
    return wait_run_counter(plan_flag(p, p->h_out), expected, poll ? 4000000L : 0L, s, &p->seq_seen);
}

// Runs `enqueue(stream)` and waits for its result.  Default: eager launches on the caller's stream -- the first kernel
// starts while the host is still enqueueing the rest, and that beats replaying the same sequence from a captured
// hipGraph (measured, 30k-event YAML objective: 0.063 vs 0.075 ms per value+gradient, 0.154 vs 0.165 ms time-aware; a graph
// launch costs ~12 us before its first node runs, the nodes are dependent either way).  CMAX_PLAN_GRAPHS=1 (read at plan
// creation) switches the replay on: eager for the first calls (and whenever the handle is being profiled or a capture
// failed), afterwards a captured hipGraph per (kind, handle state) replayed on the plan's stream.
template <typename F>
int run_sequence(cmax_patch_plan_s *p, int kind, hipStream_t caller, F enqueue) {
    HandleEvalState pre;
    handle_get_eval_state(p->handle, &pre);
    if (!p->graphs.empty() && p->graphs[0].generation != pre.generation) {
        drop_graphs(p);  // new events behind the handle: other device pointers, another work list
        p->eager_calls = 0;
    }
    const bool eager = !p->graphs_ok || pre.profiling || p->eager_calls < 3 || handle_has_comm(p->handle);  // (collectives are never captured)
    if (eager) {
        ++p->eager_calls;
        int rc = enqueue(caller);
        if (rc) return rc;
        return wait_for_tail(p, caller, p->eager_calls > 1);  // (the first call may compile / allocate: sleep)
    }
    const uint64_t key = state_key(pre, kind);
    cmax_patch_plan_s::GraphEntry *entry = nullptr;
    for (auto &g : p->graphs)
        if (g.key == key) entry = &g;
    if (!entry) {
        if (p->graphs.size() >= 32) drop_graphs(p);
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        bool ok = hipStreamBeginCapture(p->own_stream, hipStreamCaptureModeRelaxed) == hipSuccess;
        int rc = 0;
        if (ok) {
            rc = enqueue(p->own_stream);  // host-side bookkeeping of the handle runs as in an eager call
            ok = hipStreamEndCapture(p->own_stream, &graph) == hipSuccess && rc == 0 && graph != nullptr;
        }
        if (ok) ok = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess;
        if (graph) (void)hipGraphDestroy(graph);
        if (!ok) {  // never again: fall back to eager launches
            (void)hipGetLastError();
            p->graphs_ok = false;
            handle_set_eval_state(p->handle, &pre);
            rc = enqueue(caller);
            if (rc) return rc;
            return wait_for_tail(p, caller, false);
        }
        cmax_patch_plan_s::GraphEntry e;
        e.key = key;
        e.generation = pre.generation;
        e.exec = exec;
        handle_get_eval_state(p->handle, &e.post);
        p->graphs.push_back(e);
        entry = &p->graphs.back();
    } else {
        handle_set_eval_state(p->handle, &entry->post);
    }
    // order after whatever the caller has queued, run, wait
    CMAX_CHECK_HIP(hipEventRecord(p->ev_caller, caller));
    CMAX_CHECK_HIP(hipStreamWaitEvent(p->own_stream, p->ev_caller, 0));
    CMAX_CHECK_HIP(hipGraphLaunch(entry->exec, p->own_stream));
    return wait_for_tail(p, p->own_stream, true);
}

}  // namespace

extern "C" {

int cmax_sizeof_patch_objective(void) { return (int)sizeof(cmax_patch_objective_t); }

static int plan_allocate(cmax_handle_t h, const cmax_patch_objective_t &d, int nx, const char *who, cmax_patch_plan_t *out);

int cmax_patch_plan_create(cmax_handle_t h, const cmax_patch_objective_t *desc, cmax_patch_plan_t *out) {
    CMAX_REQUIRE(h && desc && out, "patch_plan_create: null pointer");
    if (handle_is_weighted(h)) {
        set_error("patch_plan_create: not built for a handle that holds per-event weights (cmax_set_event_weights); pass weights = NULL to clear them");
        return CMAX_EUNSUPPORTED;
    }
    const cmax_patch_objective_t &d = *desc;
    CMAX_REQUIRE(d.n_terms >= 1 && d.n_terms <= 4, "patch_plan_create: n_terms");
    CMAX_REQUIRE(d.H > 0 && d.W > 0 && d.ph > 0 && d.pw > 0 && d.sw_h > 0 && d.sw_w > 0 && d.pad_h >= 0 && d.pad_w >= 0, "patch_plan_create: sizes");
    CMAX_REQUIRE(!d.time_aware || (d.T > 0 && d.t0 >= 0 && d.t0 < d.T), "patch_plan_create: time bins");
    CMAX_REQUIRE(d.filter_type == CMAX_FILTER_BILINEAR || d.filter_type == CMAX_FILTER_NEAREST, "patch_plan_create: filter_type (CMAX_FILTER_BILINEAR or CMAX_FILTER_NEAREST)");
    for (int i = 0; i < d.n_terms; ++i) {
        CMAX_REQUIRE(d.term[i].model == (d.time_aware ? CMAX_MODEL_VOXEL : CMAX_MODEL_DENSE), "patch_plan_create: term model must match time_aware");
        CMAX_REQUIRE(!d.time_aware || d.term[i].T == d.T, "patch_plan_create: term T");
        CMAX_REQUIRE(d.term[i].motion_dtype == d.term[0].motion_dtype, "patch_plan_create: the terms must agree on motion_dtype");
    }
    if (d.time_aware && d.scale_later && handle_has_comm(h)) {
        set_error("patch_plan_create: scale_later is not built for time-sliced batches (the handle holds a communicator)");
        return CMAX_EINVAL;
    }
    return plan_allocate(h, d, 2 * d.ph * d.pw, "patch_plan_create", out);
}

// The plan's buffers for a checked descriptor and nx unknowns (`who` names the entry point in messages)
static int plan_allocate(cmax_handle_t h, const cmax_patch_objective_t &d, int nx, const char *who, cmax_patch_plan_t *out) {
    cmax_patch_plan_s *p = new (std::nothrow) cmax_patch_plan_s();
    if (!p) {
        set_error("%s: out of host memory", who);
        return CMAX_ENOMEM;
    }
    p->handle = h;
    p->d = d;
    p->nx = nx;
    if (const char *e = getenv("CMAX_PLAN_GRAPHS")) p->graphs_ok = atoi(e) != 0;
    p->nflow = 2 * (int64_t)d.H * d.W;
    p->nmotion = d.time_aware ? (int64_t)d.T * p->nflow : p->nflow;
    p->exact = d.term[0].motion_dtype == CMAX_F64;
    int rc = 0;
    if (!rc) rc = p->x64.reserve(nullptr, 2 * (int64_t)p->nx + 2, nullptr);  // x | v | 2 scalars, filled by one copy
    if (!rc) p->v64 = p->x64 + p->nx;
    if (!rc) rc = p->flow64.reserve(nullptr, p->nflow, nullptr);
    if (!rc && d.time_aware) rc = p->vox64.reserve(nullptr, p->nmotion, nullptr);
    if (!rc) rc = p->gacc64.reserve(nullptr, p->nmotion, nullptr);
    if (!rc && d.time_aware) rc = p->gflow64.reserve(nullptr, p->nflow, nullptr);
    if (!rc && d.time_aware && d.scale_later) {
        rc = p->dense64.reserve(nullptr, p->nflow, nullptr);
        if (!rc) rc = p->sl.reserve(nullptr, kSlScalars, nullptr);
        if (!rc) rc = p->sl_partial.reserve(nullptr, kSlSlots * kSlBlocks, nullptr);
    }
    if (!rc) rc = p->gx64.reserve(nullptr, p->nx, nullptr);
    if (!rc) rc = p->results.reserve(nullptr, 8 * 5, nullptr);  // four terms and the flow regulariser's value
    if (!rc) rc = p->motion32.reserve(nullptr, (p->exact ? 2 : 1) * p->nmotion, nullptr);
    if (!rc) rc = p->grad32.reserve(nullptr, p->nmotion, nullptr);
    if (!rc) rc = p->tan32.reserve(nullptr, p->nmotion, nullptr);
    if (!rc) rc = p->gx32.reserve(nullptr, p->nx, nullptr);
    if (!rc) rc = p->h_in.reserve(2 * (int64_t)p->nx + 2);
    if (!rc && hipStreamCreateWithFlags(&p->own_stream, hipStreamNonBlocking) != hipSuccess) rc = CMAX_ENOMEM;
    if (!rc && hipEventCreateWithFlags(&p->ev_caller, hipEventDisableTiming) != hipSuccess) rc = CMAX_ENOMEM;
    if (!rc) rc = p->h_out.reserve(2 + (int64_t)p->nx);  // (zero-filled: the run counter starts where seq_dev and seq_seen do)
    if (!rc) rc = p->seq_dev.reserve(nullptr, 1, nullptr);
    if (!rc && hipMemset(p->seq_dev, 0, sizeof(unsigned long long)) != hipSuccess) rc = CMAX_ENOMEM;
    if (rc) {
        if (rc == CMAX_ENOMEM) set_error("%s: allocation failed", who);
        cmax_patch_plan_destroy(p);
        return rc;
    }
    *out = p;
    return 0;
}

int cmax_sizeof_basis_objective(void) { return (int)sizeof(cmax_basis_objective_t); }

// A patch plan whose map x -> dense flow is D = sum_k x_k B_k (cmax_basis_kernels.h; no counterpart in the reference, whose dense-flow
// warp rule src/warp.py:263-313 the model composes with).  The descriptor becomes a cmax_patch_objective_t with a 1 x K "grid" that
// nothing interpolates (map_kind picks the basis wherever the filter is picked) and no total variation.
int cmax_basis_plan_create(cmax_handle_t h, const cmax_basis_objective_t *desc, const void *basis_dev, cmax_stream_t stream, cmax_patch_plan_t *out) {
    CMAX_REQUIRE(h && desc && basis_dev && out, "basis_plan_create: null pointer");
    if (handle_is_weighted(h)) {
        set_error("basis_plan_create: not built for a handle that holds per-event weights (cmax_set_event_weights); pass weights = NULL to clear them");
        return CMAX_EUNSUPPORTED;
    }
    if (handle_has_comm(h)) {
        set_error("basis_plan_create: not built for time-sliced batches (the handle holds a communicator)");
        return CMAX_EUNSUPPORTED;
    }
    const cmax_basis_objective_t &b = *desc;
    CMAX_REQUIRE(b.K >= 1 && b.K <= CMAX_BASIS_MAX_K, "basis_plan_create: K (1 .. CMAX_BASIS_MAX_K)");
    CMAX_REQUIRE(b.basis_dtype == CMAX_F32 || b.basis_dtype == CMAX_F64, "basis_plan_create: basis_dtype (CMAX_F32 or CMAX_F64)");
    CMAX_REQUIRE(b.scale_later == 0, "basis_plan_create: scale_later is not built for a flow basis");
    CMAX_REQUIRE(b.n_terms >= 1 && b.n_terms <= 4, "basis_plan_create: n_terms");
    CMAX_REQUIRE(b.H > 0 && b.W > 0, "basis_plan_create: sizes");
    CMAX_REQUIRE(!b.time_aware || (b.T > 0 && b.t0 >= 0 && b.t0 < b.T), "basis_plan_create: time bins");
    for (int i = 0; i < b.n_terms; ++i) {
        CMAX_REQUIRE(b.term[i].model == (b.time_aware ? CMAX_MODEL_VOXEL : CMAX_MODEL_DENSE), "basis_plan_create: term model must match time_aware");
        CMAX_REQUIRE(!b.time_aware || b.term[i].T == b.T, "basis_plan_create: term T");
        CMAX_REQUIRE(b.term[i].motion_dtype == b.term[0].motion_dtype, "basis_plan_create: the terms must agree on motion_dtype");
    }
    cmax_patch_objective_t d;
    std::memset(&d, 0, sizeof(d));
    d.n_terms = b.n_terms;
    d.time_aware = b.time_aware;
    d.T = b.T;
    d.scheme = b.scheme;
    d.t0 = b.t0;
    d.H = b.H;
    d.W = b.W;
    d.ph = 1;
    d.pw = b.K;
    d.sw_h = d.sw_w = 1;
    d.filter_type = CMAX_FILTER_BILINEAR;
    d.t_scale = b.t_scale;
    for (int i = 0; i < 4; ++i) d.weight[i] = b.weight[i];
    for (int i = 0; i < b.n_terms; ++i) d.term[i] = b.term[i];
    cmax_patch_plan_t p = nullptr;
    int rc = plan_allocate(h, d, b.K, "basis_plan_create", &p);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int64_t nb = (int64_t)b.K * p->nflow;
    p->map_kind = kMapBasis;
    p->basis_dtype = b.basis_dtype;
    const bool b64 = b.basis_dtype == CMAX_F64;
    rc = b64 ? p->basis64.reserve(nullptr, nb, nullptr) : p->basis32.reserve(nullptr, nb, nullptr);
    if (!rc) rc = p->basis_partial.reserve(nullptr, (int64_t)basis_adj_chunks(p->nflow) * b.K, nullptr);
    double bmax[CMAX_BASIS_MAX_K];
    if (!rc) {
        // the plan's copy, max |B_k| per field (into the chunk sums' buffer: K doubles fit and nothing else uses it yet), the read-back
        hipError_t e = hipMemcpyAsync(const_cast<void *>(plan_basis(p)), basis_dev, (size_t)nb * (b64 ? sizeof(double) : sizeof(float)), hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) {
            if (b64) hipLaunchKernelGGL(k_basis_absmax<double>, dim3(b.K), dim3(256), 0, s, (const double *)p->basis64, p->nflow, (double *)p->basis_partial);
            else hipLaunchKernelGGL(k_basis_absmax<float>, dim3(b.K), dim3(256), 0, s, (const float *)p->basis32, p->nflow, (double *)p->basis_partial);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(bmax, p->basis_partial, (size_t)b.K * sizeof(double), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            set_error("basis_plan_create: copying the basis failed: %s", hipGetErrorString(e));
            rc = (int)e;
        }
    }
    if (rc) {
        if (rc == CMAX_ENOMEM) set_error("basis_plan_create: allocation failed");
        cmax_patch_plan_destroy(p);
        return rc;
    }
    p->bmax.assign(bmax, bmax + b.K);
    *out = p;
    return 0;
}

int cmax_basis_to_dense(const void *theta_dev, const void *basis_dev, int dtype, int K, int H, int W, int adjoint, void *out, cmax_stream_t stream) {
    CMAX_REQUIRE(theta_dev && basis_dev && out && H > 0 && W > 0, "basis_to_dense");
    CMAX_REQUIRE(K >= 1 && K <= CMAX_BASIS_MAX_K, "basis_to_dense: K (1 .. CMAX_BASIS_MAX_K)");
    CMAX_REQUIRE(dtype == CMAX_F32 || dtype == CMAX_F64, "basis_to_dense: dtype");
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = 2 * (int64_t)H * W;
    if (!adjoint) {
        if (dtype == CMAX_F32) launch_basis_to_dense<float, float>((const double *)theta_dev, basis_dev, K, n, 1.0, nullptr, (float *)out, s);
        else launch_basis_to_dense<double, double>((const double *)theta_dev, basis_dev, K, n, 1.0, nullptr, (double *)out, s);
        CMAX_CHECK_LAUNCH();
        return 0;
    }
    // the chunk sums: a stream-ordered temporary keeps the operator stateless (as the accumulators of cmax_warp_events_bwd)
    double *partial = nullptr;
    CMAX_CHECK_HIP(hipMallocAsync((void **)&partial, (size_t)basis_adj_chunks(n) * K * sizeof(double), s));
    if (dtype == CMAX_F32) launch_basis_adj<float, float>((const float *)theta_dev, basis_dev, K, n, partial, (double *)out, s);
    else launch_basis_adj<double, double>((const double *)theta_dev, basis_dev, K, n, partial, (double *)out, s);
    const hipError_t e = hipGetLastError();
    CMAX_CHECK_HIP(hipFreeAsync(partial, s));
    CMAX_CHECK_HIP(e);
    return 0;
}

int cmax_sizeof_depth_objective(void) { return (int)sizeof(cmax_depth_objective_t); }

// A patch plan whose map is the depth map of cmax_depth_kernels.h: the descriptor becomes a cmax_patch_objective_t that carries the grid's
// geometry (the kernels read it there) and no total variation; map_kind picks the map wherever the filter is picked.
int cmax_depth_plan_create(cmax_handle_t h, const cmax_depth_objective_t *desc, const void *A_dev, const void *B_dev, cmax_stream_t stream,
                           cmax_patch_plan_t *out) {
    CMAX_REQUIRE(h && desc && A_dev && out, "depth_plan_create: null pointer");
    if (handle_is_weighted(h)) {
        set_error("depth_plan_create: not built for a handle that holds per-event weights (cmax_set_event_weights); pass weights = NULL to clear them");
        return CMAX_EUNSUPPORTED;
    }
    if (handle_has_comm(h)) {
        set_error("depth_plan_create: not built for time-sliced batches (the handle holds a communicator)");
        return CMAX_EUNSUPPORTED;
    }
    const cmax_depth_objective_t &b = *desc;
    CMAX_REQUIRE(b.Ka >= 1 && b.Kb >= 0 && b.Ka <= CMAX_BASIS_MAX_K && b.Kb <= CMAX_BASIS_MAX_K && b.Ka + b.Kb <= CMAX_BASIS_MAX_K,
                 "depth_plan_create: Ka, Kb (1 <= Ka, 0 <= Kb, Ka + Kb <= CMAX_BASIS_MAX_K)");
    CMAX_REQUIRE(b.Kb == 0 || B_dev, "depth_plan_create: null B with Kb > 0");
    CMAX_REQUIRE(b.basis_dtype == CMAX_F32 || b.basis_dtype == CMAX_F64, "depth_plan_create: basis_dtype (CMAX_F32 or CMAX_F64)");
    CMAX_REQUIRE(b.scale_later == 0, "depth_plan_create: scale_later is not built for the depth map");
    CMAX_REQUIRE(b.filter_type == CMAX_FILTER_BILINEAR, "depth_plan_create: filter_type: only CMAX_FILTER_BILINEAR is built for the depth map (nearest is refused)");
    CMAX_REQUIRE(b.tv_weight == 0.0, "depth_plan_create: tv_weight: total variation is not built for the depth grid (must be 0)");
    CMAX_REQUIRE(b.n_terms >= 1 && b.n_terms <= 4, "depth_plan_create: n_terms");
    CMAX_REQUIRE(b.H > 0 && b.W > 0 && b.ph > 0 && b.pw > 0 && b.sw_h > 0 && b.sw_w > 0 && b.pad_h >= 0 && b.pad_w >= 0, "depth_plan_create: sizes");
    CMAX_REQUIRE((int64_t)b.ph * b.pw <= (1 << 20), "depth_plan_create: sizes (ph pw)");
    CMAX_REQUIRE(!b.time_aware || (b.T > 0 && b.t0 >= 0 && b.t0 < b.T), "depth_plan_create: time bins");
    for (int i = 0; i < b.n_terms; ++i) {
        CMAX_REQUIRE(b.term[i].model == (b.time_aware ? CMAX_MODEL_VOXEL : CMAX_MODEL_DENSE), "depth_plan_create: term model must match time_aware");
        CMAX_REQUIRE(!b.time_aware || b.term[i].T == b.T, "depth_plan_create: term T");
        CMAX_REQUIRE(b.term[i].motion_dtype == b.term[0].motion_dtype, "depth_plan_create: the terms must agree on motion_dtype");
    }
    cmax_patch_objective_t d;
    std::memset(&d, 0, sizeof(d));
    d.n_terms = b.n_terms;
    d.time_aware = b.time_aware;
    d.T = b.T;
    d.scheme = b.scheme;
    d.t0 = b.t0;
    d.H = b.H;
    d.W = b.W;
    d.ph = b.ph;
    d.pw = b.pw;
    d.sw_h = b.sw_h;
    d.sw_w = b.sw_w;
    d.pad_h = b.pad_h;
    d.pad_w = b.pad_w;
    d.filter_type = CMAX_FILTER_BILINEAR;
    d.t_scale = b.t_scale;
    for (int i = 0; i < 4; ++i) d.weight[i] = b.weight[i];
    for (int i = 0; i < b.n_terms; ++i) d.term[i] = b.term[i];
    cmax_patch_plan_t p = nullptr;
    const int K = b.Ka + b.Kb;
    int rc = plan_allocate(h, d, K + b.ph * b.pw, "depth_plan_create", &p);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    p->map_kind = kMapDepth;
    p->Ka = b.Ka;
    p->Kb = b.Kb;
    p->basis_dtype = b.basis_dtype;
    const bool b64 = b.basis_dtype == CMAX_F64;
    const size_t esz = b64 ? sizeof(double) : sizeof(float);
    rc = b64 ? p->basis64.reserve(nullptr, (int64_t)K * p->nflow, nullptr) : p->basis32.reserve(nullptr, (int64_t)K * p->nflow, nullptr);
    if (!rc) rc = p->basis_partial.reserve(nullptr, (int64_t)depth_adj_chunks(p->nflow / 2) * K, nullptr);
    if (!rc) rc = p->depth_q.reserve(nullptr, p->nflow / 2, nullptr);
    if (!rc) {
        hipError_t e = hipMemcpyAsync(const_cast<void *>(plan_basis(p)), A_dev, (size_t)b.Ka * p->nflow * esz, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess && b.Kb > 0) e = hipMemcpyAsync(const_cast<void *>(plan_depth_B(p)), B_dev, (size_t)b.Kb * p->nflow * esz, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            set_error("depth_plan_create: copying the bases failed: %s", hipGetErrorString(e));
            rc = (int)e;
        }
    }
    if (rc) {
        if (rc == CMAX_ENOMEM) set_error("depth_plan_create: allocation failed");
        cmax_patch_plan_destroy(p);
        return rc;
    }
    *out = p;
    return 0;
}

// what every depth leaf checks before it launches
static int depth_leaf_check(const char *who, bool pointers, int dtype, int Ka, int Kb, const void *B, int ph, int pw, int pad_h, int pad_w, int sw_h, int sw_w,
                            int H, int W) {
    const bool ok = pointers && (Kb == 0 || B) && (dtype == CMAX_F32 || dtype == CMAX_F64) && Ka >= 1 && Kb >= 0 && Ka <= CMAX_BASIS_MAX_K &&
                    Kb <= CMAX_BASIS_MAX_K && Ka + Kb <= CMAX_BASIS_MAX_K && H > 0 && W > 0 && ph > 0 && pw > 0 && sw_h > 0 && sw_w > 0 && pad_h >= 0 &&
                    pad_w >= 0 && (int64_t)ph * pw <= (1 << 20);
    if (!ok) {
        set_error("%s: bad argument: null pointer, dtype, Ka / Kb (1 <= Ka, 0 <= Kb, Ka + Kb <= CMAX_BASIS_MAX_K) or sizes", who);
        return CMAX_EINVAL;
    }
    return 0;
}

int cmax_depth_to_dense(const void *a, const void *b, const void *s_, const void *A, const void *B, int dtype, int Ka, int Kb, int ph, int pw, int pad_h,
                        int pad_w, int sw_h, int sw_w, int H, int W, void *out, cmax_stream_t stream) {
    if (int rc = depth_leaf_check("depth_to_dense", a && s_ && A && out && (Kb == 0 || b), dtype, Ka, Kb, B, ph, pw, pad_h, pad_w, sw_h, sw_w, H, W)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const DepthGeom g{ph, pw, pad_h, pad_w, sw_h, sw_w, H, W};
    if (dtype == CMAX_F32) launch_depth_to_dense<float, float>((const double *)a, (const double *)b, (const double *)s_, A, B, Ka, Kb, g, 1.0, nullptr, (float *)out, s);
    else launch_depth_to_dense<double, double>((const double *)a, (const double *)b, (const double *)s_, A, B, Ka, Kb, g, 1.0, nullptr, (double *)out, s);
    CMAX_CHECK_LAUNCH();
    return 0;
}

int cmax_depth_to_dense_tan(const void *a, const void *s_, const void *da, const void *db, const void *ds, const void *A, const void *B, int dtype, int Ka,
                            int Kb, int ph, int pw, int pad_h, int pad_w, int sw_h, int sw_w, int H, int W, void *out, cmax_stream_t stream) {
    if (int rc = depth_leaf_check("depth_to_dense_tan", a && s_ && da && ds && A && out && (Kb == 0 || db), dtype, Ka, Kb, B, ph, pw, pad_h, pad_w, sw_h, sw_w, H, W))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    const DepthGeom g{ph, pw, pad_h, pad_w, sw_h, sw_w, H, W};
    if (dtype == CMAX_F32)
        launch_depth_to_dense_tan<float, float>((const double *)a, (const double *)s_, (const double *)da, (const double *)db, (const double *)ds, A, B, Ka, Kb, g, 1.0,
                                                (float *)out, s);
    else
        launch_depth_to_dense_tan<double, double>((const double *)a, (const double *)s_, (const double *)da, (const double *)db, (const double *)ds, A, B, Ka, Kb, g,
                                                  1.0, (double *)out, s);
    CMAX_CHECK_LAUNCH();
    return 0;
}

// both adjoints of the leaf: chunk sums, the folded [a | b] block and the plane q in ONE stream-ordered temporary
static int depth_leaf_adjoint(bool second, const void *a, const void *s_, const void *da, const void *ds, const void *g, const void *dg, const void *A,
                              const void *B, int dtype, int Ka, int Kb, const DepthGeom &geo, double *out_a, double *out_b, double *out_s, hipStream_t s) {
    const int64_t hw = (int64_t)geo.H * geo.W;
    const int K = Ka + Kb;
    const size_t n_partial = (size_t)depth_adj_chunks(hw) * K;
    double *tmp = nullptr;
    CMAX_CHECK_HIP(hipMallocAsync((void **)&tmp, (n_partial + K + (size_t)hw) * sizeof(double), s));
    double *ab = tmp + n_partial, *q = ab + K;
    const double *a_ = (const double *)a, *sg = (const double *)s_, *da_ = (const double *)da, *ds_ = (const double *)ds;
    if (dtype == CMAX_F32) {
        if (second) launch_depth_adj<float, float, true>((const float *)g, (const float *)dg, a_, sg, da_, ds_, A, B, Ka, Kb, geo, tmp, q, ab, out_s, s);
        else launch_depth_adj<float, float, false>((const float *)g, (const float *)nullptr, a_, sg, da_, ds_, A, B, Ka, Kb, geo, tmp, q, ab, out_s, s);
    } else {
        if (second) launch_depth_adj<double, double, true>((const double *)g, (const double *)dg, a_, sg, da_, ds_, A, B, Ka, Kb, geo, tmp, q, ab, out_s, s);
        else launch_depth_adj<double, double, false>((const double *)g, (const double *)nullptr, a_, sg, da_, ds_, A, B, Ka, Kb, geo, tmp, q, ab, out_s, s);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out_a, ab, (size_t)Ka * sizeof(double), hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && Kb > 0) e = hipMemcpyAsync(out_b, ab + Ka, (size_t)Kb * sizeof(double), hipMemcpyDeviceToDevice, s);
    CMAX_CHECK_HIP(hipFreeAsync(tmp, s));
    CMAX_CHECK_HIP(e);
    return 0;
}

int cmax_depth_to_dense_adj(const void *a, const void *s_, const void *g, const void *A, const void *B, int dtype, int Ka, int Kb, int ph, int pw, int pad_h,
                            int pad_w, int sw_h, int sw_w, int H, int W, double *g_a, double *g_b, double *g_s, cmax_stream_t stream) {
    if (int rc = depth_leaf_check("depth_to_dense_adj", a && s_ && g && A && g_a && g_s && (Kb == 0 || g_b), dtype, Ka, Kb, B, ph, pw, pad_h, pad_w, sw_h, sw_w, H, W))
        return rc;
    return depth_leaf_adjoint(false, a, s_, nullptr, nullptr, g, nullptr, A, B, dtype, Ka, Kb, DepthGeom{ph, pw, pad_h, pad_w, sw_h, sw_w, H, W}, g_a, g_b, g_s,
                              (hipStream_t)stream);
}

int cmax_depth_to_dense_adj2(const void *a, const void *s_, const void *da, const void *ds, const void *g, const void *dg, const void *A, const void *B, int dtype,
                             int Ka, int Kb, int ph, int pw, int pad_h, int pad_w, int sw_h, int sw_w, int H, int W, double *out_a, double *out_b, double *out_s,
                             cmax_stream_t stream) {
    if (int rc = depth_leaf_check("depth_to_dense_adj2", a && s_ && da && ds && g && dg && A && out_a && out_s && (Kb == 0 || out_b), dtype, Ka, Kb, B, ph, pw, pad_h,
                                  pad_w, sw_h, sw_w, H, W))
        return rc;
    return depth_leaf_adjoint(true, a, s_, da, ds, g, dg, A, B, dtype, Ka, Kb, DepthGeom{ph, pw, pad_h, pad_w, sw_h, sw_w, H, W}, out_a, out_b, out_s,
                              (hipStream_t)stream);
}

int cmax_patch_plan_set_t_scale(cmax_patch_plan_t p, double t_scale) {
    CMAX_REQUIRE(p != nullptr, "patch_plan_set_t_scale");
    if (p->d.t_scale != t_scale) {
        p->d.t_scale = t_scale;
        drop_graphs(p);  // the scale is baked into captured launches
        p->eager_calls = 0;
    }
    return 0;
}

int cmax_sizeof_flow_regularizer(void) { return (int)sizeof(cmax_flow_regularizer_t); }

int cmax_patch_plan_set_flow_regularizer(cmax_patch_plan_t p, const cmax_flow_regularizer_t *desc) {
    CMAX_REQUIRE(p != nullptr, "patch_plan_set_flow_regularizer: null plan");
    cmax_flow_regularizer_t r = {};
    if (desc && desc->kind != CMAX_FLOWREG_NONE) {
        r = *desc;
        CMAX_REQUIRE(flowreg_desc_ok(r), "patch_plan_set_flow_regularizer: kind (CMAX_FLOWREG_DIVERGENCE or _AREA), eps >= 0 and s > 0, all finite");
        CMAX_REQUIRE(r.weight >= -1.7e308 && r.weight <= 1.7e308, "patch_plan_set_flow_regularizer: weight must be finite");
        CMAX_REQUIRE(p->d.H >= 3 && p->d.W >= 3, "patch_plan_set_flow_regularizer: the sensor must be at least 3 x 3");
        if (p->d.time_aware && p->d.scale_later) {
            set_error("patch_plan_set_flow_regularizer: not built for a scale_later plan (its map is rescaled by a maximum: F is not t_scale * map x)");
            return CMAX_EINVAL;
        }
        if (handle_has_comm(p->handle)) {
            set_error("patch_plan_set_flow_regularizer: not built for time-sliced batches (the handle holds a communicator): the term would be counted once per rank");
            return CMAX_EUNSUPPORTED;
        }
        r.reserved = 0;
        int rc = p->reg_partial.reserve(nullptr, flowreg_tiles(p->d.H, p->d.W), nullptr);
        if (rc) {
            set_error("patch_plan_set_flow_regularizer: allocation failed");
            return rc;
        }
    }
    p->reg = r;
    drop_graphs(p);  // the term's launches and its parameters are baked into captured sequences
    p->eager_calls = 0;
    return 0;
}

int cmax_flow_regularizer(const void *F, int dtype, int H, int W, const cmax_flow_regularizer_t *desc, double *value_dev, void *grad, cmax_stream_t stream) {
    CMAX_REQUIRE(F && desc && value_dev, "flow_regularizer: null pointer");
    CMAX_REQUIRE(dtype == CMAX_F32 || dtype == CMAX_F64, "flow_regularizer: dtype");
    CMAX_REQUIRE(H >= 3 && W >= 3, "flow_regularizer: H and W must be at least 3");
    CMAX_REQUIRE(flowreg_desc_ok(*desc), "flow_regularizer: kind (CMAX_FLOWREG_DIVERGENCE or _AREA), eps >= 0 and s > 0, all finite");
    hipStream_t s = (hipStream_t)stream;
    // the tiles' energies: a stream-ordered temporary keeps the operator stateless (as the chunk sums of cmax_basis_to_dense)
    double *partial = nullptr;
    CMAX_CHECK_HIP(hipMallocAsync((void **)&partial, (size_t)flowreg_tiles(H, W) * sizeof(double), s));
    if (dtype == CMAX_F32) launch_flowreg<float>(*desc, (const float *)F, 1.0, H, W, partial, value_dev, grad, 0, 1.0, s);
    else launch_flowreg<double>(*desc, (const double *)F, 1.0, H, W, partial, value_dev, grad, 0, 1.0, s);
    const hipError_t e = hipGetLastError();
    CMAX_CHECK_HIP(hipFreeAsync(partial, s));
    CMAX_CHECK_HIP(e);
    return 0;
}

int cmax_flow_regularizer_tan(const void *F, const void *dF, int dtype, int H, int W, const cmax_flow_regularizer_t *desc, void *hv, cmax_stream_t stream) {
    CMAX_REQUIRE(F && dF && desc && hv, "flow_regularizer_tan: null pointer");
    CMAX_REQUIRE(dtype == CMAX_F32 || dtype == CMAX_F64, "flow_regularizer_tan: dtype");
    CMAX_REQUIRE(H >= 3 && W >= 3, "flow_regularizer_tan: H and W must be at least 3");
    CMAX_REQUIRE(flowreg_desc_ok(*desc), "flow_regularizer_tan: kind (CMAX_FLOWREG_DIVERGENCE or _AREA), eps >= 0 and s > 0, all finite");
    hipStream_t s = (hipStream_t)stream;
    if (dtype == CMAX_F32) launch_flowreg_tan<float>(*desc, (const float *)F, (const float *)dF, 1.0, 1.0, nullptr, H, W, hv, 0, 1.0, s);
    else launch_flowreg_tan<double>(*desc, (const double *)F, (const double *)dF, 1.0, 1.0, nullptr, H, W, hv, 0, 1.0, s);
    CMAX_CHECK_LAUNCH();
    return 0;
}

int cmax_patch_plan_info(cmax_patch_plan_t p, int *n_graphs, int *graph_replay_enabled) {
    CMAX_REQUIRE(p && n_graphs && graph_replay_enabled, "patch_plan_info");
    *n_graphs = (int)p->graphs.size();
    *graph_replay_enabled = p->graphs_ok ? 1 : 0;
    return 0;
}

int cmax_patch_plan_destroy(cmax_patch_plan_t p) {
    if (!p) return 0;
    drop_graphs(p);
    if (p->own_stream) (void)hipStreamDestroy(p->own_stream);
    if (p->ev_caller) (void)hipEventDestroy(p->ev_caller);
    delete p;  // (the buffers free themselves)
    return 0;
}

int cmax_patch_plan_evaluate(cmax_patch_plan_t p, const double *x_host, int with_tv, double *loss_host, double *grad_host,
                             cmax_stream_t stream) {
    CMAX_REQUIRE(p && x_host && loss_host, "patch_plan_evaluate: null pointer");
    if (handle_is_weighted(p->handle)) {  // (a plan made before the handle received weights: refused like cmax_patch_plan_create)
        set_error("patch_plan_evaluate: not built for a handle that holds per-event weights (cmax_set_event_weights); pass weights = NULL to clear them");
        return CMAX_EUNSUPPORTED;
    }
    if (int rc = plan_refuse_reg_comm(p, "patch_plan_evaluate")) return rc;
    const bool tv = with_tv && p->d.tv_weight != 0.0;
    std::memcpy(p->h_in, x_host, (size_t)p->nx * sizeof(double));
    const int kind = (tv ? 1 : 0) | (grad_host ? 2 : 0);
    int rc = run_sequence(p, kind, (hipStream_t)stream, [&](hipStream_t s) { return enqueue_evaluate(p, tv, grad_host != nullptr, s, p->h_in, p->h_out.dev()); });
    if (rc) return rc;
    *loss_host = p->h_out[0];
    if (grad_host) std::memcpy(grad_host, p->h_out + 1, (size_t)p->nx * sizeof(double));
    return 0;
}

int cmax_sizeof_descent(void) { return (int)sizeof(cmax_descent_t); }

// SolverBase.run_torch (src/solver/base.py:840-881) on the plan's objective: x0 once, n_iter x (evaluate from the device-resident x -> tail
// into a device buffer -> k_descent_step) eagerly on the caller's stream, ONE wait, the copies out.
int cmax_patch_plan_descend(cmax_patch_plan_t p, const double *x0_host, int with_tv, const cmax_descent_t *o, cmax_descent_result_t *res_host,
                            double *x_last_host, double *x_best_host, double *loss_history_host, double *x_trace_host, cmax_stream_t stream) {
    int rc = descent_entry_check("patch_plan_descend", o, p && x0_host && res_host && x_last_host && x_best_host && loss_history_host, nullptr,
                                 p && handle_has_comm(p->handle));
    if (rc) return rc;
    if (handle_is_weighted(p->handle)) {
        set_error("patch_plan_descend: not built for a handle that holds per-event weights (cmax_set_event_weights); pass weights = NULL to clear them");
        return CMAX_EUNSUPPORTED;
    }
    hipStream_t s = (hipStream_t)stream;
    const bool tv = with_tv && p->d.tv_weight != 0.0, trace = x_trace_host != nullptr;
    const int nx = p->nx, n_iter = o->n_iter;
    const int64_t n_state = descent_state_doubles(nx, n_iter, trace);
    rc = p->d_out.reserve(nullptr, 2 + (int64_t)nx, s);
    if (!rc) rc = p->descent.reserve(nullptr, n_state, s);
    if (!rc) rc = p->h_res.reserve(4);
    if (rc) return rc;
    std::memcpy(p->h_in, x0_host, (size_t)nx * sizeof(double));
    CMAX_CHECK_HIP(hipMemcpyAsync(p->x64, p->h_in, (size_t)nx * sizeof(double), hipMemcpyHostToDevice, s));
    for (int it = 0; it < n_iter; ++it) {
        rc = enqueue_evaluate(p, tv, true, s, nullptr, p->d_out);
        if (rc) return rc;
        DescentArgs a = descent_args(*o, it, nx, trace, p->x64, p->descent);
        if (it == n_iter - 1) {
            a.res_pinned = p->h_res.dev();
            a.flag = plan_flag(p, p->h_out.dev());
            a.seq_src = p->seq_dev;
        }
        rc = launch_descent_step(a, p->d_out, p->d_out + 1, s);
        if (rc) return rc;
    }
    ++p->eager_calls;
    rc = wait_for_tail(p, s, p->eager_calls > 1, (unsigned long long)n_iter);
    if (rc) return rc;
    descent_result(p->h_res, res_host);
    rc = descent_copy_out(p->descent, true, nx, n_iter, x_best_host, x_last_host, loss_history_host, x_trace_host, s);  // (behind the wait: the state is final)
    if (rc) return rc;
    CMAX_CHECK_HIP(hipStreamSynchronize(s));
    return 0;
}

int cmax_sizeof_lbfgs(void) { return (int)sizeof(cmax_lbfgs_t); }

// L-BFGS on the plan's objective (the rules: include/cmax_hip.h): x0 once, n_eval x (evaluate from the device-resident x -> tail into a
// device buffer -> k_lbfgs_step, which decides and writes the next point) eagerly on the caller's stream, ONE wait, the copies out.
int cmax_patch_plan_lbfgs(cmax_patch_plan_t p, const double *x0_host, int with_tv, const cmax_lbfgs_t *o, cmax_lbfgs_result_t *res_host, double *x_host,
                          double *loss_history_host, double *alpha_host, int32_t *code_host, double *x_trace_host, cmax_stream_t stream) {
    int rc = lbfgs_entry_check("patch_plan_lbfgs", o, p && x0_host && res_host && x_host && loss_history_host && alpha_host && code_host, nullptr,
                               p && handle_has_comm(p->handle));
    if (rc) return rc;
    if (handle_is_weighted(p->handle)) {
        set_error("patch_plan_lbfgs: not built for a handle that holds per-event weights (cmax_set_event_weights); pass weights = NULL to clear them");
        return CMAX_EUNSUPPORTED;
    }
    hipStream_t s = (hipStream_t)stream;
    const bool tv = with_tv && p->d.tv_weight != 0.0, trace = x_trace_host != nullptr;
    const int nx = p->nx, n_eval = o->n_eval, m = o->history;
    rc = p->d_out.reserve(nullptr, 2 + (int64_t)nx, s);
    if (!rc) rc = p->lbfgs.reserve(nullptr, lbfgs_state_doubles(nx, m, n_eval, trace), s);
    if (!rc) rc = p->h_res.reserve(8);
    if (rc) return rc;
    std::memcpy(p->h_in, x0_host, (size_t)nx * sizeof(double));
    CMAX_CHECK_HIP(hipMemcpyAsync(p->x64, p->h_in, (size_t)nx * sizeof(double), hipMemcpyHostToDevice, s));
    for (int e = 0; e < n_eval; ++e) {
        rc = enqueue_evaluate(p, tv, true, s, nullptr, p->d_out);
        if (rc) return rc;
        LbfgsArgs a = lbfgs_args(*o, e, nx, trace, p->x64, p->lbfgs);
        if (e == n_eval - 1) {
            a.res_pinned = p->h_res.dev();
            a.flag = plan_flag(p, p->h_out.dev());
            a.seq_src = p->seq_dev;
        }
        rc = launch_lbfgs_step(a, p->d_out, p->d_out + 1, s);
        if (rc) return rc;
    }
    ++p->eager_calls;
    rc = wait_for_tail(p, s, p->eager_calls > 1, (unsigned long long)n_eval);
    if (rc) return rc;
    lbfgs_result(p->h_res, res_host);
    rc = lbfgs_copy_out(p->lbfgs, nx, m, n_eval, x_host, loss_history_host, alpha_host, code_host, x_trace_host, s);  // (behind the wait: the state is final)
    if (rc) return rc;
    CMAX_CHECK_HIP(hipStreamSynchronize(s));
    return 0;
}

int cmax_patch_plan_hvp(cmax_patch_plan_t p, const double *x_host, const double *v_host, double *hv_host, cmax_stream_t stream) {
    CMAX_REQUIRE(p && x_host && v_host && hv_host, "patch_plan_hvp: null pointer");
    if (handle_is_weighted(p->handle)) {
        set_error("patch_plan_hvp: not built for a handle that holds per-event weights (cmax_set_event_weights); pass weights = NULL to clear them");
        return CMAX_EUNSUPPORTED;
    }
    if (int rc = plan_refuse_reg_comm(p, "patch_plan_hvp")) return rc;
    const cmax_patch_objective_t &d = p->d;
    if (plan_has_reg(p) && !d.time_aware) {  // the regulariser's fp64 tangent field, on first use
        int rc = p->dflow64.reserve(nullptr, p->nflow, (hipStream_t)stream);
        if (rc) return rc;
    }
    if (p->map_kind == kMapDepth && !d.time_aware) {  // the fp64 tangent field, the second seed and the device-side maximum, on first use
        hipStream_t s = (hipStream_t)stream;
        int rc = p->dflow64.reserve(nullptr, p->nflow, s);
        if (!rc) rc = p->dgacc64.reserve(nullptr, p->nmotion, s);
        if (!rc) rc = p->scal.reserve(nullptr, 4, s);
        if (rc) return rc;
    }
    if (d.time_aware) {  // second-order buffers of the voxel chain, on first use
        hipStream_t s = (hipStream_t)stream;
        int rc = p->dflow64.reserve(nullptr, p->nflow, s);
        if (!rc) rc = p->dvox64.reserve(nullptr, p->nmotion, s);
        if (!rc) rc = p->dgacc64.reserve(nullptr, p->nmotion, s);
        if (!rc) rc = p->dgflow64.reserve(nullptr, p->nflow, s);
        if (!rc) rc = p->scal.reserve(nullptr, 4, s);
        if (rc) return rc;
    }
    // |v|_inf bounds |P v|_inf (a negated convex combination); a basis can amplify: sum_k |v_k| max|B_k| bounds |B v|_inf.  A depth plan
    // takes its scale on the device (enqueue_hvp_depth): here |v|_inf only tells a zero tangent from any other
    double vmax = 0.0;
    if (p->map_kind == kMapBasis)
        for (int j = 0; j < p->nx; ++j) vmax += fabs(v_host[j]) * p->bmax[j];
    else
        for (int j = 0; j < p->nx; ++j) vmax = fabs(v_host[j]) > vmax ? fabs(v_host[j]) : vmax;
    if (!(vmax > 0.0)) {
        std::memset(hv_host, 0, (size_t)p->nx * sizeof(double));
        return 0;
    }
    std::memcpy(p->h_in, x_host, (size_t)p->nx * sizeof(double));
    std::memcpy(p->h_in + p->nx, v_host, (size_t)p->nx * sizeof(double));
    p->h_in[2 * p->nx] = 1.0 / vmax;  // the tangent of the flow is scaled to max-norm <= 1 ...
    p->h_in[2 * p->nx + 1] = vmax;    // ... and the product scaled back (H is linear in the tangent)
    int rc = run_sequence(p, 4, (hipStream_t)stream, [&](hipStream_t s) { return enqueue_hvp(p, s); });
    if (rc) return rc;
    std::memcpy(hv_host, p->h_out + 1, (size_t)p->nx * sizeof(double));
    return 0;
}

int cmax_field_max(const void *x, int dtype, int64_t n, double *out, cmax_stream_t stream) {
    CMAX_REQUIRE(x && out && n > 0, "field_max");
    CMAX_REQUIRE(dtype == CMAX_F32 || dtype == CMAX_F64, "field_max: dtype");
    hipStream_t s = (hipStream_t)stream;
    CMAX_CHECK_HIP(hipMemsetAsync(out, 0, 4 * sizeof(double), s));
    const int grid = sl_grid(n);
    if (dtype == CMAX_F32) {
        hipLaunchKernelGGL(k_field_max<float>, dim3(grid), dim3(256), 0, s, (const float *)x, n, out);
        hipLaunchKernelGGL(k_field_count<float>, dim3(grid), dim3(256), 0, s, (const float *)x, n, out);
    } else {
        hipLaunchKernelGGL(k_field_max<double>, dim3(grid), dim3(256), 0, s, (const double *)x, n, out);
        hipLaunchKernelGGL(k_field_count<double>, dim3(grid), dim3(256), 0, s, (const double *)x, n, out);
    }
    CMAX_CHECK_LAUNCH();
    return 0;
}

int cmax_field_max_adj(const void *x, int dtype, int64_t n, const double *out, const double *gout, void *gx, cmax_stream_t stream) {
    CMAX_REQUIRE(x && out && gout && gx && n > 0, "field_max_adj");
    CMAX_REQUIRE(dtype == CMAX_F32 || dtype == CMAX_F64, "field_max_adj: dtype");
    hipStream_t s = (hipStream_t)stream;
    if (dtype == CMAX_F32) hipLaunchKernelGGL(k_field_max_adj<float>, dim3(div_up(n, 256)), dim3(256), 0, s, (const float *)x, n, out, gout, (float *)gx);
    else hipLaunchKernelGGL(k_field_max_adj<double>, dim3(div_up(n, 256)), dim3(256), 0, s, (const double *)x, n, out, gout, (double *)gx);
    CMAX_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
