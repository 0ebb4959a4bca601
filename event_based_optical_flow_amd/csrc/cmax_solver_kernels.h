// The kernels of the solver unit (cmax_solver.hip includes this once; nothing else does): the conversions between the fp64 stages and the
// fp32 motion of the fused terms, the scale_later reductions, the tail of an evaluation, and the device-resident descent and L-BFGS steps.
#pragma once
#include "cmax_common.h"
#include "cmax_descent.h"
#include "cmax_lbfgs.h"
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
