// The optimiser's objective in ONE library call: x (host, fp64) -> loss, gradient or Hessian-vector product (host, fp64), every stage on
// the device, one stream synchronisation per call.  A plan (cmax_patch_plan_t) is a map, a chain, the fused terms, a tail:
//
//   x --map--> dense flow D [2,H,W] --x t_scale--> F [--chain--> voxel V [T,2,H,W]] --fp32--> sum_i w_i * fused contrast objective_i
//                                                                                              [+ w_reg R(F)] [+ w_tv * total_variation(x)]
//
// and back through the hand-written adjoints.
//  - The map (map_forward / map_tangent64 / map_adjoint) is the patch interpolation with a bilinear or nearest filter
//    (cmax_patch_plan_create), a flow basis D = sum_k x_k B_k (cmax_basis_plan_create, cmax_basis_kernels.h) or the depth / ego-motion
//    map D = (Q s) (sum_k a_k A_k) + sum_j b_j B_j with x = [a | b | s] (cmax_depth_plan_create, cmax_depth_kernels.h).  The first two
//    are linear in x; the depth map is not, so its product has a sequence of its own (enqueue_hvp_depth).  Nothing outside the three
//    functions and the *_plan_create entries looks at what the map is, except where a sequence is chosen (enqueue_hvp), its buffers are
//    reserved and the host bounds the tangent (cmax_patch_plan_hvp).
//  - The chain is the Burgers / upwind voxel propagation of a time-aware plan (cmax_flow.hip), with scale_later its normalisation by
//    max D in front (patch map only; the derivation stands above k_patch_to_dense_max in cmax_solver_kernels.h).
//  - The fused terms are the library's own entry points (cmax_objective, cmax_objective_hvp: cmax_fused.hip), fp32 per event with fp64
//    reductions; an exact plan (motion_dtype == CMAX_F64) hands them both planes of the fp64 motion.  The flow regulariser
//    (cmax_patch_plan_set_flow_regularizer) is one more term on F.
//  - The tail (k_patch_tail) is one workgroup: weighted sum, total variation, the chain through t_scale, the run counter the host waits on.
// forward_motion runs map, normalisation, chain and fp32 conversion in that order; backward_motion runs them in reverse.  The four product
// sequences (enqueue_hvp_dense / _time_aware / _scale_later / _depth) share their stages: copy_in_product, tangent_max / tangent_to_fp32 (unit_tangent: both),
// terms_grad_and_product, product_tail.
//
// Equivalent of PyramidalPatchContrastMaximization.objective_scipy + motion_to_dense_flow (src/solver/patch_contrast_pyramid.py:430-516)
// under TorchWrapper.get_value_and_grad / get_hvp (src/solver/scipy_autograd/torch_wrapper.py:30-73).  The stages are the same kernels
// the autograd wrappers of functional.py chain one Python call at a time; what the plan adds is that it owns the intermediate buffers and
// the pinned staging, so that an evaluation costs one ctypes call instead of ~40 Python-level operations (measured on the cfg1-shaped
// objective: 0.40 ms -> 0.09 ms per value + gradient), and can replay its launch sequence from a captured hipGraph.
// Pre/post stages run in fp64 like the reference's solver (patch_contrast_pyramid.py:186).  The reference has no counterpart for the basis
// and depth maps; their D is warped by its dense-flow rule x' = x - dt * D[src] (src/warp.py:263-313).
//
// This file: the plan struct, the map, the stages, the sequences, the C entries.  The unit's kernels are in cmax_solver_kernels.h.
#include <cstring>
#include <new>
#include <atomic>
#include <type_traits>
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
#include "cmax_solver_kernels.h"

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

// ---------------------------------------------------------------------------------------------
// The map x -> dense flow D [2,H,W]: the patch interpolation P x with the plan's filter, a flow basis sum_k x_k B_k, or the depth
// map (Q s) (A a) + B b.  map_forward, map_tangent64 and map_adjoint decide on map_kind; the stages and the sequences below call
// them and do not look behind.
// ---------------------------------------------------------------------------------------------
// Where a field goes: fp32 (`hi32`; with `lo32` also what fp32 lost of the fp64 value -- the two planes of an exact plan's motion) or
// fp64.  Exactly one of hi32 / f64 is set.
struct MapDst {
    float *hi32 = nullptr, *lo32 = nullptr;
    double *f64 = nullptr;
};
MapDst dst_f64(double *f64) { return MapDst{nullptr, nullptr, f64}; }
MapDst motion_dst(const cmax_patch_plan_s *p) { return MapDst{p->motion32, p->exact ? p->motion32 + p->nmotion : nullptr, nullptr}; }
// What an adjoint answered: the patch adjoint in the dtype of its input, the basis adjoint and the depth adjoint always in fp64.
// Exactly one pointer is set.
struct MapGrad {
    const double *g64 = nullptr;
    const float *g32 = nullptr;
};

// f(TB()) with TB the element type of the plan's copy of the basis; f(integral_constant<filter>) with the plan's patch filter
template <typename F>
void with_basis_type(const cmax_patch_plan_s *p, F f) {
    if (p->basis_dtype == CMAX_F64) f(double());
    else f(float());
}
template <typename F>
void with_filter(const cmax_patch_plan_s *p, F f) {
    if (p->d.filter_type == CMAX_FILTER_NEAREST) f(std::integral_constant<int, CMAX_FILTER_NEAREST>());
    else f(std::integral_constant<int, CMAX_FILTER_BILINEAR>());
}

const void *plan_basis(const cmax_patch_plan_s *p) { return p->basis_dtype == CMAX_F64 ? (const void *)p->basis64.get() : (const void *)p->basis32.get(); }
DepthGeom plan_depth_geom(const cmax_patch_plan_s *p) {
    const cmax_patch_objective_t &d = p->d;
    return DepthGeom{d.ph, d.pw, d.pad_h, d.pad_w, d.sw_h, d.sw_w, d.H, d.W};
}
// the depth plan's copy of A, and of B behind it, as typed by basis_dtype
const void *plan_depth_B(const cmax_patch_plan_s *p) {
    const int64_t off = (int64_t)p->Ka * p->nflow;
    return p->basis_dtype == CMAX_F64 ? (const void *)(p->basis64.get() + off) : (const void *)(p->basis32.get() + off);
}

// dst = src [n] * scale [* *scale_dev], an fp32 destination
int convert_to_fp32(const double *src, int64_t n, double scale, const double *scale_dev, MapDst dst, hipStream_t s) {
    if (dst.lo32) hipLaunchKernelGGL(k_convert_split, dim3(div_up(n, 256)), dim3(256), 0, s, src, n, scale, scale_dev, dst.hi32, dst.lo32);
    else hipLaunchKernelGGL((k_convert_scale<float, double>), dim3(div_up(n, 256)), dim3(256), 0, s, src, n, scale, scale_dev, dst.hi32);
    CMAX_CHECK_LAUNCH();
    return 0;
}

// dst = scale [* *scale_dev] * D(src64), src64 laid out like x.  The basis and the depth kernels scale (scale_dev included) and round in
// the launch that sums.  The patch interpolation does so for a host-side scale; with scale_dev (fp32 destinations only: the tangent of
// enqueue_hvp_dense) it goes through the leaf's fp64 field in flow64, which this CLOBBERS, and a conversion.
int map_forward(cmax_patch_plan_s *p, const double *src64, double scale, const double *scale_dev, MapDst dst, hipStream_t s) {
    const cmax_patch_objective_t &d = p->d;
    if (p->map_kind == kMapBasis) {
        with_basis_type(p, [&](auto tb) {
            using TB = decltype(tb);
            if (dst.f64) launch_basis_to_dense<TB, double>(src64, plan_basis(p), p->nx, p->nflow, scale, scale_dev, dst.f64, s);
            else if (dst.lo32) launch_basis_to_dense_split<TB>(src64, plan_basis(p), p->nx, p->nflow, scale, scale_dev, dst.hi32, dst.lo32, s);
            else launch_basis_to_dense<TB, float>(src64, plan_basis(p), p->nx, p->nflow, scale, scale_dev, dst.hi32, s);
        });
    } else if (p->map_kind == kMapDepth) {
        const void *A = plan_basis(p), *B = plan_depth_B(p);
        const DepthGeom g = plan_depth_geom(p);
        const int Ka = p->Ka, Kb = p->Kb;
        const double *a = src64, *b = src64 + Ka, *sg = src64 + Ka + Kb;
        with_basis_type(p, [&](auto tb) {
            using TB = decltype(tb);
            if (dst.f64) launch_depth_to_dense<TB, double>(a, b, sg, A, B, Ka, Kb, g, scale, scale_dev, dst.f64, s);
            else if (dst.lo32) launch_depth_to_dense_split<TB>(a, b, sg, A, B, Ka, Kb, g, scale, scale_dev, dst.hi32, dst.lo32, s);
            else launch_depth_to_dense<TB, float>(a, b, sg, A, B, Ka, Kb, g, scale, scale_dev, dst.hi32, s);
        });
    } else if (scale_dev) {
        int rc = cmax_patch_to_dense_filter(src64, CMAX_F64, d.ph, d.pw, d.pad_h, d.pad_w, d.sw_h, d.sw_w, d.H, d.W, d.filter_type, 0, p->flow64, s);
        if (rc) return rc;
        return convert_to_fp32(p->flow64, p->nflow, scale, scale_dev, dst, s);
    } else {
        const dim3 grid(div_up(p->nflow, 256)), block(256);
        with_filter(p, [&](auto filter) {
            constexpr int F = decltype(filter)::value;
            if (dst.f64)
                hipLaunchKernelGGL((k_patch_to_dense<double, double, F>), grid, block, 0, s, src64, d.ph, d.pw, d.pad_h, d.pad_w, d.sw_h, d.sw_w, d.H, d.W, dst.f64, scale);
            else if (dst.lo32)
                hipLaunchKernelGGL(k_patch_to_dense_split<F>, grid, block, 0, s, src64, d.ph, d.pw, d.pad_h, d.pad_w, d.sw_h, d.sw_w, d.H, d.W, dst.hi32, dst.lo32, scale);
            else
                hipLaunchKernelGGL((k_patch_to_dense<double, float, F>), grid, block, 0, s, src64, d.ph, d.pw, d.pad_h, d.pad_w, d.sw_h, d.sw_w, d.H, d.W, dst.hi32, scale);
        });
    }
    CMAX_CHECK_LAUNCH();
    return 0;
}

// dst64 = scale * J(x64) v64, the tangent of the map in fp64: the map of v64 where the map is linear, k_depth_to_dense_tan otherwise
int map_tangent64(cmax_patch_plan_s *p, double scale, double *dst64, hipStream_t s) {
    if (p->map_kind != kMapDepth) return map_forward(p, p->v64, scale, nullptr, dst_f64(dst64), s);
    const int Ka = p->Ka, Kb = p->Kb;
    const double *x = p->x64, *v = p->v64;
    with_basis_type(p, [&](auto tb) {
        launch_depth_to_dense_tan<decltype(tb), double>(x, x + Ka + Kb, v, v + Ka, v + Ka + Kb, plan_basis(p), plan_depth_B(p), Ka, Kb, plan_depth_geom(p), scale, dst64, s);
    });
    CMAX_CHECK_LAUNCH();
    return 0;
}

// The adjoint of the map on a flow gradient in fp32 (g32) or fp64 (g64), taken at the x the plan holds in x64.  With dg64 (depth plan
// only, where J depends on x): the second-order adjoint along v64 for the seeds (g64, dg64).
int map_adjoint(cmax_patch_plan_s *p, const float *g32, const double *g64, const double *dg64, MapGrad *out, hipStream_t s) {
    const cmax_patch_objective_t &d = p->d;
    *out = MapGrad();
    if (p->map_kind == kMapPatch) {
        int rc = g32 ? cmax_patch_to_dense_filter(g32, CMAX_F32, d.ph, d.pw, d.pad_h, d.pad_w, d.sw_h, d.sw_w, d.H, d.W, d.filter_type, 1, p->gx32, s)
                     : cmax_patch_to_dense_filter(g64, CMAX_F64, d.ph, d.pw, d.pad_h, d.pad_w, d.sw_h, d.sw_w, d.H, d.W, d.filter_type, 1, p->gx64, s);
        if (g32) out->g32 = p->gx32;
        else out->g64 = p->gx64;
        return rc;
    }
    if (p->map_kind == kMapBasis) {
        with_basis_type(p, [&](auto tb) {
            using TB = decltype(tb);
            if (g32) launch_basis_adj<TB, float>(g32, plan_basis(p), p->nx, p->nflow, p->basis_partial, p->gx64, s);
            else launch_basis_adj<TB, double>(g64, plan_basis(p), p->nx, p->nflow, p->basis_partial, p->gx64, s);
        });
    } else {
        const void *A = plan_basis(p), *B = plan_depth_B(p);
        const DepthGeom geo = plan_depth_geom(p);
        const int Ka = p->Ka, Kb = p->Kb;
        const double *x = p->x64, *v = p->v64;
        double *gx = p->gx64;
        with_basis_type(p, [&](auto tb) {
            using TB = decltype(tb);
            const float *no32 = nullptr;
            const double *no64 = nullptr;
            if (dg64) launch_depth_adj<TB, double, true>(g64, dg64, x, x + Ka + Kb, v, v + Ka + Kb, A, B, Ka, Kb, geo, p->basis_partial, p->depth_q, gx, gx + Ka + Kb, s);
            else if (g32) launch_depth_adj<TB, float, false>(g32, no32, x, x + Ka + Kb, v, v + Ka + Kb, A, B, Ka, Kb, geo, p->basis_partial, p->depth_q, gx, gx + Ka + Kb, s);
            else launch_depth_adj<TB, double, false>(g64, no64, x, x + Ka + Kb, v, v + Ka + Kb, A, B, Ka, Kb, geo, p->basis_partial, p->depth_q, gx, gx + Ka + Kb, s);
        });
    }
    CMAX_CHECK_LAUNCH();
    out->g64 = p->gx64;
    return 0;
}

// C2 of the plan: the gradient (or product) w.r.t. the unknowns, summed over the ranks (a no-op without a communicator)
int plan_reduce_gx(cmax_patch_plan_s *p, MapGrad gx, hipStream_t s) {
    if (!handle_has_comm(p->handle)) return 0;
    if (gx.g64) return handle_allreduce_sum(p->handle, const_cast<double *>(gx.g64), (size_t)p->nx, true, s);
    return handle_allreduce_sum(p->handle, const_cast<float *>(gx.g32), (size_t)p->nx, false, s);
}
// ... of an EVALUATION: the terms' result[8] ride along and leave as rank 0's on every rank (each rank summed its statistics in its own
// order; replicated optimisers must see the same loss bit for bit).  Value-only evaluations exchange the scalars alone.
int plan_reduce_gx_and_results(cmax_patch_plan_s *p, MapGrad gx, hipStream_t s) {
    if (!handle_has_comm(p->handle)) return 0;
    const int n_scalars = 8 * p->d.n_terms;
    if (gx.g64) return handle_allreduce_sum_with_scalars(p->handle, const_cast<double *>(gx.g64), (size_t)p->nx, true, p->results, n_scalars, s);
    return handle_allreduce_sum_with_scalars(p->handle, const_cast<float *>(gx.g32), gx.g32 ? (size_t)p->nx : 0, false, p->results, n_scalars, s);
}

bool plan_has_reg(const cmax_patch_plan_s *p) { return p->reg.kind != CMAX_FLOWREG_NONE; }
int plan_refuse_reg_comm(const cmax_patch_plan_s *p, const char *who) {
    if (!plan_has_reg(p) || !handle_has_comm(p->handle)) return 0;
    set_error("%s: the plan's flow regulariser is not built for time-sliced batches (the handle holds a communicator): the term would be counted once per rank", who);
    return CMAX_EUNSUPPORTED;
}
// (a plan made before the handle received weights is refused like a new one)
int plan_refuse_weights(cmax_handle_t h, const char *who) {
    if (!handle_is_weighted(h)) return 0;
    set_error("%s: not built for a handle that holds per-event weights (cmax_set_event_weights); pass weights = NULL to clear them", who);
    return CMAX_EUNSUPPORTED;
}

// The flow regulariser on F = t (map x) in fp64, before any rounding: its value into the fifth result slot and, with `acc`, weight * dR/dF
// added into that fp64 [2,H,W] accumulator.  A time-aware plan holds F in flow64 already; any other plan maps x once more, unscaled, and
// the kernel scales as it stages.
int plan_flowreg(cmax_patch_plan_s *p, double *acc, hipStream_t s) {
    const cmax_patch_objective_t &d = p->d;
    double scale = 1.0;
    if (!d.time_aware) {
        int rc = map_forward(p, p->x64, 1.0, nullptr, dst_f64(p->flow64), s);
        if (rc) return rc;
        scale = d.t_scale;
    }
    launch_flowreg<double>(p->reg, p->flow64, scale, d.H, d.W, p->reg_partial, p->results + 8 * 4, acc, 1, p->reg.weight, s);
    CMAX_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Forward: x64 -> the fp32 motion of the fused terms, flow [2,H,W] or voxel [T,2,H,W] in pixel per normalised time, in four stages:
// the map, the scale_later normalisation (if any), the voxel chain (if time-aware), the fp32 conversion.
// ---------------------------------------------------------------------------------------------
// scale_later, stages 1 and 2: D = P x (dense64) and s = max D; u = t D / s into flow64 (tie count on the way).  With the tangent:
// Dd = P v into dflow64, and its sum over the ties.
int scale_later_normalise(cmax_patch_plan_s *p, bool with_tangent, hipStream_t s) {
    const cmax_patch_objective_t &d = p->d;
    const dim3 grid(sl_grid(p->nflow)), block(256);
    with_filter(p, [&](auto filter) {
        hipLaunchKernelGGL(k_patch_to_dense_max<decltype(filter)::value>, grid, block, 0, s, (const double *)p->x64, d.ph, d.pw, d.pad_h, d.pad_w, d.sw_h, d.sw_w, d.H, d.W,
                           (double *)p->dense64, (double *)p->sl_partial);
    });
    CMAX_CHECK_LAUNCH();
    if (with_tangent) {
        int rc = cmax_patch_to_dense_filter(p->v64, CMAX_F64, d.ph, d.pw, d.pad_h, d.pad_w, d.sw_h, d.sw_w, d.H, d.W, d.filter_type, 0, p->dflow64, s);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_sl_scale, grid, block, 0, s, p->dense64, with_tangent ? (const double *)p->dflow64 : nullptr, p->nflow, d.t_scale, sl_grid(p->nflow), p->sl,
                       p->flow64, p->sl_partial);
    CMAX_CHECK_LAUNCH();
    return 0;
}

// stage 4 behind a chain: the fp64 voxel [* *scale_dev] -> the motion's fp32 plane(s)
int motion_from_voxel(cmax_patch_plan_s *p, const double *scale_dev, hipStream_t s) {
    return convert_to_fp32(p->vox64, p->nmotion, 1.0, scale_dev, motion_dst(p), s);
}

// stages 3 and 4: the voxel chain on the displacement field in flow64 (patch_contrast_pyramid.py:452, 499-515) -> vox64, then the fp32
// plane(s) unless the chain kernel wrote them: it leaves fp64 and fp32 at once where it can, but no low plane and no device-side scale
int chain_to_motion(cmax_patch_plan_s *p, const double *scale_dev, hipStream_t s) {
    const cmax_patch_objective_t &d = p->d;
    const bool may_fuse = !p->exact && !scale_dev;
    bool wrote32 = false;
    int rc = voxel_construct_f64_f32(p->flow64, d.T, d.t0, d.H, d.W, d.scheme, p->vox64, may_fuse ? (float *)p->motion32 : nullptr, may_fuse ? &wrote32 : nullptr, s);
    if (rc || wrote32) return rc;
    return motion_from_voxel(p, scale_dev, s);
}

// Leaves the fp64 flow (scaled) in flow64 when time-aware, and the fp64 voxel in vox64.
int forward_motion(cmax_patch_plan_s *p, hipStream_t s) {
    const cmax_patch_objective_t &d = p->d;
    if (!d.time_aware) return map_forward(p, p->x64, d.t_scale, nullptr, motion_dst(p), s);  // map, scale and rounding in one kernel
    if (d.scale_later) {  // V = C(u), motion s V with s read from device memory
        int rc = scale_later_normalise(p, false, s);
        return rc ? rc : chain_to_motion(p, p->sl, s);
    }
    int rc = map_forward(p, p->x64, d.t_scale, nullptr, dst_f64(p->flow64), s);
    return rc ? rc : chain_to_motion(p, nullptr, s);
}

// gradient of the fused terms w.r.t. the unknowns (without t_scale), and what the tail still has to multiply it by
int backward_motion(cmax_patch_plan_s *p, MapGrad *gx, double *weight_scale, hipStream_t s) {
    const cmax_patch_objective_t &d = p->d;
    *weight_scale = 1.0;
    if (d.n_terms == 1 && !d.time_aware && !plan_has_reg(p)) {
        // one term on the dense flow: the adjoint of the map reads the fp32 flow gradient as it is (fp64 accumulation inside), the
        // term's weight is applied by the tail
        *weight_scale = d.weight[0];
        return map_adjoint(p, p->grad32, nullptr, nullptr, gx, s);
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
    return map_adjoint(p, nullptr, gflow, nullptr, gx, s);
}

// The tail kernel: loss | gradient (or product) | run counter into `out` -- the device view of the pinned output, or the descent's device buffer
int launch_tail(cmax_patch_plan_s *p, FinalParams fp, MapGrad gx, const double *gscale_dev, const double *ok_dev, double *out, hipStream_t s) {
    fp.flag_slot = 1 + (int)p->nx;
    fp.ph = p->d.ph;
    fp.pw = p->d.pw;
    hipLaunchKernelGGL(k_patch_tail, dim3(1), dim3(256), 0, s, fp, p->results, p->x64, gx.g64, gx.g32, gscale_dev, out, p->seq_dev, ok_dev);
    CMAX_CHECK_LAUNCH();
    return 0;
}

// Everything between the input and the output of one evaluation, enqueued on `s` (no synchronisation).  x_src: pinned host memory the
// leading copy brings x from (nullptr: x64 holds x already -- the descent's iterate); out: where the tail writes.
int enqueue_evaluate(cmax_patch_plan_s *p, bool tv, bool want_grad, hipStream_t s, const double *x_src, double *out) {
    const cmax_patch_objective_t &d = p->d;
    if (x_src) CMAX_CHECK_HIP(hipMemcpyAsync(p->x64, x_src, (size_t)p->nx * sizeof(double), hipMemcpyHostToDevice, s));
    int rc = forward_motion(p, s);
    if (rc) return rc;
    const bool reg = plan_has_reg(p), sl = d.time_aware && d.scale_later;
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
    MapGrad gx;
    double wscale = 1.0;
    if (want_grad) rc = backward_motion(p, &gx, &wscale, s);
    if (!rc && d.n_terms > 0) rc = plan_reduce_gx_and_results(p, gx, s);
    else if (!rc && want_grad) rc = plan_reduce_gx(p, gx, s);
    if (rc) return rc;
    FinalParams fp = {};
    fp.n_terms = d.n_terms;
    fp.with_tv = tv ? 1 : 0;
    fp.nx = want_grad ? p->nx : 0;
    fp.tv_crop = d.tv_omit_boundary && d.ph > 2 && d.pw > 2;  // total_variation.py:123-125
    for (int i = 0; i < 4; ++i) fp.weight[i] = d.weight[i];
    fp.tv_weight = d.tv_weight;
    fp.gscale = sl ? 1.0 : d.t_scale * wscale;  // d(flow * t_scale) / d flow (scale_later: t is in g_D)
    fp.reg_weight = reg ? p->reg.weight : 0.0;
    return launch_tail(p, fp, gx, nullptr, sl ? p->sl + 1 : nullptr, out, s);
}

// ---------------------------------------------------------------------------------------------
// Hessian-vector products: h_in = x | v | 1/|v|_inf | |v|_inf.  The stages the four sequences share, then the sequences.
// ---------------------------------------------------------------------------------------------
// x64 | v64 | the two scalars are one allocation: a single copy brings them
int copy_in_product(cmax_patch_plan_s *p, hipStream_t s) {
    CMAX_CHECK_HIP(hipMemcpyAsync(p->x64, p->h_in, (2 * (size_t)p->nx + 2) * sizeof(double), hipMemcpyHostToDevice, s));
    return 0;
}

// The tangent handed to cmax_objective_hvp must have max-norm <= 1 (the chain and a non-linear map can amplify it, so no host bound
// holds): scal[0] = max |src64| over the motion (1 if it is all zero), scal[1] = 1 / scal[0], on the device ...
int tangent_max(cmax_patch_plan_s *p, const double *src64, hipStream_t s) {
    const int mgrid = div_up(p->nmotion, 256);
    unsigned long long *bits = reinterpret_cast<unsigned long long *>(p->scal + 2);
    CMAX_CHECK_HIP(hipMemsetAsync(bits, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_absmax, dim3(mgrid < 256 ? mgrid : 256), dim3(256), 0, s, src64, p->nmotion, bits);
    hipLaunchKernelGGL(k_absmax_finish, dim3(1), dim3(1), 0, s, bits, p->scal);
    CMAX_CHECK_LAUNCH();
    return 0;
}
// ... tan32 = src64 * scal[1] ...
int tangent_to_fp32(cmax_patch_plan_s *p, const double *src64, hipStream_t s) {
    hipLaunchKernelGGL((k_convert_scale<float, double>), dim3(div_up(p->nmotion, 256)), dim3(256), 0, s, src64, p->nmotion, 1.0, p->scal + 1, p->tan32);
    CMAX_CHECK_LAUNCH();
    return 0;
}
// ... and both
int unit_tangent(cmax_patch_plan_s *p, const double *src64, hipStream_t s) {
    int rc = tangent_max(p, src64, s);
    return rc ? rc : tangent_to_fp32(p, src64, s);
}

// Per term: g of the motion, summed into gacc64; H (tangent / its max-norm), summed into dgacc64 and scaled back by scal[0].  (A
// time-sliced batch: this rank's share, like everything behind it.)
int terms_grad_and_product(cmax_patch_plan_s *p, hipStream_t s) {
    const cmax_patch_objective_t &d = p->d;
    const int mgrid = div_up(p->nmotion, 256);
    for (int i = 0; i < d.n_terms; ++i) {
        int rc = plan_objective(p, &d.term[i], p->results + 8 * i, p->grad32, s);
        if (rc) return rc;
        hipLaunchKernelGGL(k_accumulate, dim3(mgrid), dim3(256), 0, s, p->grad32, p->nmotion, d.weight[i], i == 0 ? 1 : 0, p->gacc64, (const double *)nullptr);
        CMAX_CHECK_LAUNCH();
        rc = plan_objective_hvp(p, &d.term[i], p->grad32, s);
        if (rc) return rc;
        hipLaunchKernelGGL(k_accumulate, dim3(mgrid), dim3(256), 0, s, p->grad32, p->nmotion, d.weight[i], i == 0 ? 1 : 0, p->dgacc64, (const double *)p->scal);
        CMAX_CHECK_LAUNCH();
    }
    return 0;
}

// out = gscale [* *gscale_dev] * gx, no loss terms and no total variation (piecewise linear: zero Hessian almost everywhere)
int product_tail(cmax_patch_plan_s *p, double gscale, MapGrad gx, const double *gscale_dev, const double *ok_dev, hipStream_t s) {
    FinalParams fp = {};
    fp.nx = p->nx;
    fp.gscale = gscale;
    return launch_tail(p, fp, gx, gscale_dev, ok_dev, p->h_out.dev(), s);
}

// A linear map and no chain: H_x v = t^2 P^T H_flow P v.
int enqueue_hvp_dense(cmax_patch_plan_s *p, hipStream_t s) {
    const cmax_patch_objective_t &d = p->d;
    int rc = copy_in_product(p, s);
    if (rc) return rc;
    const double *inv_vmax = p->x64 + 2 * p->nx, *vmax = inv_vmax + 1;
    rc = forward_motion(p, s);
    if (rc) return rc;
    // tangent of the flow, scaled to max-norm <= 1 by the host's bound (the interpolation is a negated convex combination, so
    // |P v|_inf <= |v|_inf; a basis: cmax_patch_plan_hvp): u = (t_scale * |v|_inf) * tan32, and H is linear in u
    rc = map_forward(p, p->v64, 1.0, inv_vmax, MapDst{p->tan32, nullptr, nullptr}, s);
    if (rc) return rc;
    const bool reg = plan_has_reg(p);
    const bool accumulate = reg || d.n_terms != 1;
    for (int i = 0; i < d.n_terms; ++i) {
        rc = plan_objective_hvp(p, &d.term[i], p->grad32, s);
        if (rc) return rc;
        if (accumulate) {
            hipLaunchKernelGGL(k_accumulate, dim3(div_up(p->nmotion, 256)), dim3(256), 0, s, p->grad32, p->nmotion, d.weight[i], i == 0 ? 1 : 0, p->gacc64);
            CMAX_CHECK_LAUNCH();
        }
    }
    if (reg) {  // w (grad^2_F R)[P v / |v|_inf] at F = t P x, in fp64: scaled by t^2 |v|_inf with the rest
        rc = map_forward(p, p->x64, 1.0, nullptr, dst_f64(p->flow64), s);
        if (!rc) rc = map_tangent64(p, 1.0, p->dflow64, s);
        if (rc) return rc;
        launch_flowreg_tan<double>(p->reg, p->flow64, p->dflow64, d.t_scale, 1.0, inv_vmax, d.H, d.W, p->gacc64, 1, p->reg.weight, s);
        CMAX_CHECK_LAUNCH();
    }
    MapGrad gx;
    double wscale = 1.0;
    rc = backward_motion(p, &gx, &wscale, s);
    if (!rc) rc = plan_reduce_gx(p, gx, s);
    if (rc) return rc;
    return product_tail(p, d.t_scale * d.t_scale * wscale, gx, vmax, nullptr, s);  // (times |v|_inf, from device memory)
}

// Time-aware objective: x -> F = t P x -> voxel V(F) -> L(V).  With g_V = dL/dV, H_VV the Hessian of the fused
// terms (cmax_objective_hvp) and J = dV/dF:
//   H_x v = t P^T [ J^T H_VV J (t P v) + (dJ[t P v])^T g_V ]
// J (t P v) is the tangent voxel of the dual-number sweep; the bracket is what its adjoint sweep returns for the
// seeds (g_V, H_VV dV).  The tangent handed to cmax_objective_hvp must have max-norm <= 1, hence the device-side
// max |dV| (the propagation can amplify the tangent).
int enqueue_hvp_time_aware(cmax_patch_plan_s *p, hipStream_t s) {
    const cmax_patch_objective_t &d = p->d;
    int rc = copy_in_product(p, s);
    if (rc) return rc;
    const double *inv_vmax = p->x64 + 2 * p->nx, *vmax = inv_vmax + 1;
    const int fgrid = div_up(p->nflow, 256);
    const int64_t off0 = (int64_t)d.t0 * p->nflow;
    // F = t P x,  dF = t P v / |v|_inf
    rc = map_forward(p, p->x64, 1.0, nullptr, dst_f64(p->flow64), s);
    if (!rc) rc = map_tangent64(p, 1.0, p->dflow64, s);
    if (rc) return rc;
    hipLaunchKernelGGL((k_convert_scale<double, double>), dim3(fgrid), dim3(256), 0, s, p->flow64, p->nflow, d.t_scale, (const double *)nullptr, p->flow64);
    hipLaunchKernelGGL((k_convert_scale<double, double>), dim3(fgrid), dim3(256), 0, s, p->dflow64, p->nflow, d.t_scale, inv_vmax, p->dflow64);
    CMAX_CHECK_LAUNCH();
    rc = cmax_voxel_construct_tan(p->flow64, p->dflow64, CMAX_F64, d.T, d.t0, d.H, d.W, d.scheme, p->vox64, p->dvox64, s);
    if (rc) return rc;
    // fp32 motion and unit-norm fp32 tangent of the fused terms
    rc = tangent_max(p, p->dvox64, s);
    if (!rc) rc = motion_from_voxel(p, nullptr, s);
    if (!rc) rc = tangent_to_fp32(p, p->dvox64, s);
    if (!rc) rc = terms_grad_and_product(p, s);  // g_V, H_VV dV
    if (rc) return rc;
    // the sweep leaves d(dL/dF) in bin t0 of the tangent gradient voxel: the map's adjoint reads it there
    rc = voxel_construct_adj_tan_f64(p->vox64, p->dvox64, d.T, d.t0, d.H, d.W, d.scheme, p->gacc64, p->dgacc64, s, handle_is_deterministic(p->handle));
    if (rc) return rc;
    if (plan_has_reg(p)) {  // w (grad^2_F R)[dF] for the same tangent, where the map's adjoint reads
        launch_flowreg_tan<double>(p->reg, p->flow64, p->dflow64, 1.0, 1.0, nullptr, d.H, d.W, p->dgacc64 + off0, 1, p->reg.weight, s);
        CMAX_CHECK_LAUNCH();
    }
    MapGrad gx;
    rc = map_adjoint(p, nullptr, p->dgacc64 + off0, nullptr, &gx, s);
    if (!rc) rc = plan_reduce_gx(p, gx, s);
    if (rc) return rc;
    return product_tail(p, d.t_scale, gx, vmax, nullptr, s);  // the outer t P^T; times |v|_inf from device memory
}

// ... with scale_later: the map x -> M = s C(t P x / s) and its second-order adjoint as derived above k_patch_to_dense_max.
int enqueue_hvp_scale_later(cmax_patch_plan_s *p, hipStream_t s) {
    const cmax_patch_objective_t &d = p->d;
    int rc = copy_in_product(p, s);
    if (rc) return rc;
    const double *inv_vmax = p->x64 + 2 * p->nx, *vmax = inv_vmax + 1;
    const int fgrid = div_up(p->nflow, 256), mgrid = div_up(p->nmotion, 256);
    // D = P x, s = max D;  Dd = P v;  u = t D / s (flow64);  ud = (t Dd / |v|_inf - u sd) / s (dflow64)
    rc = scale_later_normalise(p, true, s);
    if (rc) return rc;
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
    rc = unit_tangent(p, p->dgacc64, s);
    if (!rc) rc = terms_grad_and_product(p, s);  // g_M, H_MM Md
    if (rc) return rc;
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
    MapGrad gx;
    rc = map_adjoint(p, nullptr, p->dgflow64, nullptr, &gx, s);
    if (rc) return rc;
    return product_tail(p, 1.0, gx, vmax, p->sl + 1, s);  // t is in gd_D; times |v|_inf from device memory
}

// Depth plan (the map x -> D is a product of unknowns: its derivative J depends on x).  With F = t D(x), g_F = dL/dF and v the tangent:
//   H_x v = t [ J^T (H_FF t dD) + (dJ[v])^T g_F ],   dD = J v (k_depth_to_dense_tan)
// -- the second-order adjoint of k_depth_adj on the seeds (g_F, dg_F).  A time-aware plan puts the voxel chain between F and the fused
// terms exactly as enqueue_hvp_time_aware does.  The tangent handed to cmax_objective_hvp is scaled to unit max-norm from a maximum taken
// on the device: no host bound holds for the product (Q ds) (A a), and the scalars the host sends with x | v are not used.
int enqueue_hvp_depth(cmax_patch_plan_s *p, hipStream_t s) {
    const cmax_patch_objective_t &d = p->d;
    int rc = copy_in_product(p, s);
    if (rc) return rc;
    const int64_t off0 = d.time_aware ? (int64_t)d.t0 * p->nflow : 0;
    // dF = t J v in fp64;  F = t D(x) -> the fp32 motion (flow64 / vox64 as an evaluation leaves them)
    rc = map_tangent64(p, d.t_scale, p->dflow64, s);
    if (rc) return rc;
    const double *tan64 = p->dflow64;
    if (d.time_aware) {
        rc = map_forward(p, p->x64, d.t_scale, nullptr, dst_f64(p->flow64), s);
        if (!rc) rc = cmax_voxel_construct_tan(p->flow64, p->dflow64, CMAX_F64, d.T, d.t0, d.H, d.W, d.scheme, p->vox64, p->dvox64, s);
        if (!rc) rc = motion_from_voxel(p, nullptr, s);
        tan64 = p->dvox64;
    } else {
        rc = forward_motion(p, s);
    }
    if (!rc) rc = unit_tangent(p, tan64, s);
    if (!rc) rc = terms_grad_and_product(p, s);
    if (rc) return rc;
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
    MapGrad gx;
    rc = map_adjoint(p, nullptr, p->gacc64 + off0, p->dgacc64 + off0, &gx, s);
    if (rc) return rc;
    return product_tail(p, d.t_scale, gx, nullptr, nullptr, s);  // the outer t J^T (the inner t is in dF)
}

int enqueue_hvp(cmax_patch_plan_s *p, hipStream_t s) {
    const cmax_patch_objective_t &d = p->d;
    if (p->map_kind == kMapDepth) return enqueue_hvp_depth(p, s);
    if (d.time_aware && d.scale_later) return enqueue_hvp_scale_later(p, s);
    if (d.time_aware) return enqueue_hvp_time_aware(p, s);
    return enqueue_hvp_dense(p, s);
}

// The second-order buffers, on first use: the fp64 tangent field (also what the regulariser's product reads), the tangent voxel, the second
// seed, the scale_later tangent gradient, the device-side maximum
int reserve_product_buffers(cmax_patch_plan_s *p, hipStream_t s) {
    const bool chain = p->d.time_aware, device_max = chain || p->map_kind == kMapDepth;
    int rc = 0;
    if (device_max || plan_has_reg(p)) rc = p->dflow64.reserve(nullptr, p->nflow, s);
    if (!rc && chain) rc = p->dvox64.reserve(nullptr, p->nmotion, s);
    if (!rc && device_max) rc = p->dgacc64.reserve(nullptr, p->nmotion, s);
    if (!rc && chain) rc = p->dgflow64.reserve(nullptr, p->nflow, s);
    if (!rc && device_max) rc = p->scal.reserve(nullptr, 4, s);
    return rc;
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

// cmax_patch_plan_descend / _lbfgs: x0 once, n x (evaluate from the device-resident x -> tail into a device buffer -> `step(i, last)`, the
// solver's own kernel) eagerly on the caller's stream, ONE wait.  The last step publishes `n_result` doubles and the run counter.
template <typename Step>
int run_device_solver(cmax_patch_plan_s *p, const double *x0_host, int with_tv, int n, int n_result, hipStream_t s, Step step) {
    const bool tv = with_tv && p->d.tv_weight != 0.0;
    int rc = p->d_out.reserve(nullptr, 2 + (int64_t)p->nx, s);
    if (!rc) rc = p->h_res.reserve(n_result);
    if (rc) return rc;
    std::memcpy(p->h_in, x0_host, (size_t)p->nx * sizeof(double));
    CMAX_CHECK_HIP(hipMemcpyAsync(p->x64, p->h_in, (size_t)p->nx * sizeof(double), hipMemcpyHostToDevice, s));
    for (int i = 0; i < n; ++i) {
        rc = enqueue_evaluate(p, tv, true, s, nullptr, p->d_out);
        if (!rc) rc = step(i, i == n - 1);
        if (rc) return rc;
    }
    ++p->eager_calls;
    return wait_for_tail(p, s, p->eager_calls > 1, (unsigned long long)n);
}
// the last step's result block, and the run counter into h_out's slot like every tail's
template <typename Args>
void publish_result_from(cmax_patch_plan_s *p, Args &a) {
    a.res_pinned = p->h_res.dev();
    a.flag = plan_flag(p, p->h_out.dev());
    a.seq_src = p->seq_dev;
}

// What the three descriptors share: the number of terms, the time bins, and terms that fit them and agree on motion_dtype
int check_plan_terms(const char *who, int n_terms, int time_aware, int T, int t0, const cmax_objective_t *term) {
    auto bad = [who](int line, const char *what) {
        set_error("%s:%d bad argument: %s: %s", __FILE__, line, who, what);
        return CMAX_EINVAL;
    };
    if (!(n_terms >= 1 && n_terms <= 4)) return bad(__LINE__, "n_terms");
    if (time_aware && !(T > 0 && t0 >= 0 && t0 < T)) return bad(__LINE__, "time bins");
    for (int i = 0; i < n_terms; ++i) {
        if (term[i].model != (time_aware ? CMAX_MODEL_VOXEL : CMAX_MODEL_DENSE)) return bad(__LINE__, "term model must match time_aware");
        if (time_aware && term[i].T != T) return bad(__LINE__, "term T");
        if (term[i].motion_dtype != term[0].motion_dtype) return bad(__LINE__, "the terms must agree on motion_dtype");
    }
    return 0;
}

// The fields a basis or a depth descriptor shares with cmax_patch_objective_t; the grid's geometry is the caller's, total variation stays 0
template <typename Desc>
cmax_patch_objective_t plan_descriptor_of(const Desc &b) {
    cmax_patch_objective_t d;
    std::memset(&d, 0, sizeof(d));
    d.n_terms = b.n_terms;
    d.time_aware = b.time_aware;
    d.T = b.T;
    d.scheme = b.scheme;
    d.t0 = b.t0;
    d.H = b.H;
    d.W = b.W;
    d.filter_type = CMAX_FILTER_BILINEAR;
    d.t_scale = b.t_scale;
    for (int i = 0; i < 4; ++i) d.weight[i] = b.weight[i];
    for (int i = 0; i < b.n_terms; ++i) d.term[i] = b.term[i];
    return d;
}

int plan_create_failed(cmax_patch_plan_t p, int rc, const char *who) {
    if (rc == CMAX_ENOMEM) set_error("%s: allocation failed", who);
    cmax_patch_plan_destroy(p);
    return rc;
}


}  // namespace

extern "C" {

int cmax_sizeof_patch_objective(void) { return (int)sizeof(cmax_patch_objective_t); }

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
    if (rc) return plan_create_failed(p, rc, who);
    *out = p;
    return 0;
}

// a basis or a depth plan's own copy of its fields: `n` elements of basis_dtype
static int plan_reserve_basis(cmax_patch_plan_t p, int basis_dtype, int64_t n) {
    p->basis_dtype = basis_dtype;
    return basis_dtype == CMAX_F64 ? p->basis64.reserve(nullptr, n, nullptr) : p->basis32.reserve(nullptr, n, nullptr);
}

int cmax_patch_plan_create(cmax_handle_t h, const cmax_patch_objective_t *desc, cmax_patch_plan_t *out) {
    CMAX_REQUIRE(h && desc && out, "patch_plan_create: null pointer");
    if (int rc = plan_refuse_weights(h, "patch_plan_create")) return rc;
    const cmax_patch_objective_t &d = *desc;
    CMAX_REQUIRE(d.H > 0 && d.W > 0 && d.ph > 0 && d.pw > 0 && d.sw_h > 0 && d.sw_w > 0 && d.pad_h >= 0 && d.pad_w >= 0, "patch_plan_create: sizes");
    CMAX_REQUIRE(d.filter_type == CMAX_FILTER_BILINEAR || d.filter_type == CMAX_FILTER_NEAREST, "patch_plan_create: filter_type (CMAX_FILTER_BILINEAR or CMAX_FILTER_NEAREST)");
    if (int rc = check_plan_terms("patch_plan_create", d.n_terms, d.time_aware, d.T, d.t0, d.term)) return rc;
    if (d.time_aware && d.scale_later && handle_has_comm(h)) {
        set_error("patch_plan_create: scale_later is not built for time-sliced batches (the handle holds a communicator)");
        return CMAX_EINVAL;
    }
    return plan_allocate(h, d, 2 * d.ph * d.pw, "patch_plan_create", out);
}

int cmax_sizeof_basis_objective(void) { return (int)sizeof(cmax_basis_objective_t); }

// A patch plan whose map x -> dense flow is D = sum_k x_k B_k (cmax_basis_kernels.h; no counterpart in the reference, whose dense-flow
// warp rule src/warp.py:263-313 the model composes with).  The descriptor becomes a cmax_patch_objective_t with a 1 x K "grid" that
// nothing interpolates (map_kind picks the basis wherever the filter is picked) and no total variation.
int cmax_basis_plan_create(cmax_handle_t h, const cmax_basis_objective_t *desc, const void *basis_dev, cmax_stream_t stream, cmax_patch_plan_t *out) {
    const char *who = "basis_plan_create";
    CMAX_REQUIRE(h && desc && basis_dev && out, "basis_plan_create: null pointer");
    if (int rc = plan_refuse_weights(h, who)) return rc;
    if (handle_has_comm(h)) {
        set_error("basis_plan_create: not built for time-sliced batches (the handle holds a communicator)");
        return CMAX_EUNSUPPORTED;
    }
    const cmax_basis_objective_t &b = *desc;
    CMAX_REQUIRE(b.K >= 1 && b.K <= CMAX_BASIS_MAX_K, "basis_plan_create: K (1 .. CMAX_BASIS_MAX_K)");
    CMAX_REQUIRE(b.basis_dtype == CMAX_F32 || b.basis_dtype == CMAX_F64, "basis_plan_create: basis_dtype (CMAX_F32 or CMAX_F64)");
    CMAX_REQUIRE(b.scale_later == 0, "basis_plan_create: scale_later is not built for a flow basis");
    CMAX_REQUIRE(b.H > 0 && b.W > 0, "basis_plan_create: sizes");
    if (int rc = check_plan_terms(who, b.n_terms, b.time_aware, b.T, b.t0, b.term)) return rc;
    cmax_patch_objective_t d = plan_descriptor_of(b);
    d.ph = 1;
    d.pw = b.K;
    d.sw_h = d.sw_w = 1;
    cmax_patch_plan_t p = nullptr;
    int rc = plan_allocate(h, d, b.K, who, &p);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int64_t nb = (int64_t)b.K * p->nflow;
    p->map_kind = kMapBasis;
    const bool b64 = b.basis_dtype == CMAX_F64;
    rc = plan_reserve_basis(p, b.basis_dtype, nb);
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
    if (rc) return plan_create_failed(p, rc, who);
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
    const char *who = "depth_plan_create";
    CMAX_REQUIRE(h && desc && A_dev && out, "depth_plan_create: null pointer");
    if (int rc = plan_refuse_weights(h, who)) return rc;
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
    CMAX_REQUIRE(b.H > 0 && b.W > 0 && b.ph > 0 && b.pw > 0 && b.sw_h > 0 && b.sw_w > 0 && b.pad_h >= 0 && b.pad_w >= 0, "depth_plan_create: sizes");
    CMAX_REQUIRE((int64_t)b.ph * b.pw <= (1 << 20), "depth_plan_create: sizes (ph pw)");
    if (int rc = check_plan_terms(who, b.n_terms, b.time_aware, b.T, b.t0, b.term)) return rc;
    cmax_patch_objective_t d = plan_descriptor_of(b);
    d.ph = b.ph;
    d.pw = b.pw;
    d.sw_h = b.sw_h;
    d.sw_w = b.sw_w;
    d.pad_h = b.pad_h;
    d.pad_w = b.pad_w;
    cmax_patch_plan_t p = nullptr;
    const int K = b.Ka + b.Kb;
    int rc = plan_allocate(h, d, K + b.ph * b.pw, who, &p);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    p->map_kind = kMapDepth;
    p->Ka = b.Ka;
    p->Kb = b.Kb;
    const size_t esz = b.basis_dtype == CMAX_F64 ? sizeof(double) : sizeof(float);
    rc = plan_reserve_basis(p, b.basis_dtype, (int64_t)K * p->nflow);
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
    if (rc) return plan_create_failed(p, rc, who);
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
    if (int rc = plan_refuse_weights(p->handle, "patch_plan_evaluate")) return rc;
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

// SolverBase.run_torch (src/solver/base.py:840-881) on the plan's objective: run_device_solver around k_descent_step, the copies out.
int cmax_patch_plan_descend(cmax_patch_plan_t p, const double *x0_host, int with_tv, const cmax_descent_t *o, cmax_descent_result_t *res_host,
                            double *x_last_host, double *x_best_host, double *loss_history_host, double *x_trace_host, cmax_stream_t stream) {
    int rc = descent_entry_check("patch_plan_descend", o, p && x0_host && res_host && x_last_host && x_best_host && loss_history_host, nullptr,
                                 p && handle_has_comm(p->handle));
    if (!rc) rc = plan_refuse_weights(p->handle, "patch_plan_descend");
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const bool trace = x_trace_host != nullptr;
    const int nx = p->nx, n_iter = o->n_iter;
    rc = p->descent.reserve(nullptr, descent_state_doubles(nx, n_iter, trace), s);
    if (!rc) rc = run_device_solver(p, x0_host, with_tv, n_iter, 4, s, [&](int it, bool last) {
        DescentArgs a = descent_args(*o, it, nx, trace, p->x64, p->descent);
        if (last) publish_result_from(p, a);
        return launch_descent_step(a, p->d_out, p->d_out + 1, s);
    });
    if (rc) return rc;
    descent_result(p->h_res, res_host);
    rc = descent_copy_out(p->descent, true, nx, n_iter, x_best_host, x_last_host, loss_history_host, x_trace_host, s);  // (behind the wait: the state is final)
    if (rc) return rc;
    CMAX_CHECK_HIP(hipStreamSynchronize(s));
    return 0;
}

int cmax_sizeof_lbfgs(void) { return (int)sizeof(cmax_lbfgs_t); }

// L-BFGS on the plan's objective (the rules: include/cmax_hip.h): run_device_solver around k_lbfgs_step, which decides and writes the
// next point; the copies out.
int cmax_patch_plan_lbfgs(cmax_patch_plan_t p, const double *x0_host, int with_tv, const cmax_lbfgs_t *o, cmax_lbfgs_result_t *res_host, double *x_host,
                          double *loss_history_host, double *alpha_host, int32_t *code_host, double *x_trace_host, cmax_stream_t stream) {
    int rc = lbfgs_entry_check("patch_plan_lbfgs", o, p && x0_host && res_host && x_host && loss_history_host && alpha_host && code_host, nullptr,
                               p && handle_has_comm(p->handle));
    if (!rc) rc = plan_refuse_weights(p->handle, "patch_plan_lbfgs");
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const bool trace = x_trace_host != nullptr;
    const int nx = p->nx, n_eval = o->n_eval, m = o->history;
    rc = p->lbfgs.reserve(nullptr, lbfgs_state_doubles(nx, m, n_eval, trace), s);
    if (!rc) rc = run_device_solver(p, x0_host, with_tv, n_eval, 8, s, [&](int e, bool last) {
        LbfgsArgs a = lbfgs_args(*o, e, nx, trace, p->x64, p->lbfgs);
        if (last) publish_result_from(p, a);
        return launch_lbfgs_step(a, p->d_out, p->d_out + 1, s);
    });
    if (rc) return rc;
    lbfgs_result(p->h_res, res_host);
    rc = lbfgs_copy_out(p->lbfgs, nx, m, n_eval, x_host, loss_history_host, alpha_host, code_host, x_trace_host, s);  // (behind the wait: the state is final)
    if (rc) return rc;
    CMAX_CHECK_HIP(hipStreamSynchronize(s));
    return 0;
}

int cmax_patch_plan_hvp(cmax_patch_plan_t p, const double *x_host, const double *v_host, double *hv_host, cmax_stream_t stream) {
    CMAX_REQUIRE(p && x_host && v_host && hv_host, "patch_plan_hvp: null pointer");
    if (int rc = plan_refuse_weights(p->handle, "patch_plan_hvp")) return rc;
    if (int rc = plan_refuse_reg_comm(p, "patch_plan_hvp")) return rc;
    if (int rc = reserve_product_buffers(p, (hipStream_t)stream)) return rc;
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
