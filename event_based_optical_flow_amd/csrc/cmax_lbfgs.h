// Device-resident L-BFGS with a backtracking line search (cmax_patch_plan_lbfgs, cmax_objective_lbfgs; the rules are pinned in
// include/cmax_hip.h): what the two entries share on the host -- the checks of descriptor and arguments (lbfgs_check, lbfgs_entry_check),
// the arguments of one step launch (lbfgs_args), the view of a final state's regions and the one routine that hands them to the caller
// (lbfgs_copy_out) -- and the layout of the state, which is written in this file only (k_lbfgs_step of cmax_solver.hip indexes it through
// the functions below).  The reference has no counterpart: its quasi-Newton methods are SciPy's, driven from the host.
#pragma once
#include <cmath>
#include <cstring>

#include "cmax_common.h"

namespace cmax {

// L-BFGS state in device memory (doubles):
//   ctrl[kLbCtrl] | gram[kLbBasis][kLbBasis] | pad -> kLbFixed | x0[nx] | x_a[nx] | g_a[nx] | d[nx] | S[m][nx] | Y[m][nx]
//   | loss_history[n_eval] | alpha[n_eval] | code[n_eval] as int32 (ceil(n_eval / 2) doubles) | x_trace[(n_eval + 1) nx]
// The pairs sit in a ring of m physical slots: logical pair i (0 = oldest) is slot (head + i) % m, k of them are held.  gram is the Gram
// matrix of the basis {s of slot j: index j;  y of slot j: index 16 + j;  g_a: index 32}, kept between steps: an accepted step reduces only
// the products with the new s, y and g.  Entries of slots that are not held are never read.  Evaluation 0 reads none of the state.
constexpr int kLbDone = 0, kLbStatus = 1, kLbLa = 2, kLbAlpha = 3, kLbGd = 4, kLbNls = 5, kLbNiter = 6, kLbUsed = 7, kLbK = 8, kLbHead = 9,
              kLbGinf = 10, kLbG1 = 11, kLbGg = 12, kLbLastAlpha = 13, kLbCtrl = 16;
constexpr int kLbBasis = 2 * CMAX_LBFGS_MAX_HISTORY + 1, kLbG = 2 * CMAX_LBFGS_MAX_HISTORY, kLbFixed = 1112;
static_assert(kLbCtrl + kLbBasis * kLbBasis <= kLbFixed && kLbFixed % 8 == 0, "the fixed head holds the control block and the Gram matrix");
static inline int64_t lbfgs_code_doubles(int n_eval) { return ((int64_t)n_eval + 1) / 2; }
static inline int64_t lbfgs_state_doubles(int nx, int m, int n_eval, bool trace) {
    return kLbFixed + (4 + 2 * (int64_t)m) * nx + 2 * (int64_t)n_eval + lbfgs_code_doubles(n_eval) + (trace ? ((int64_t)n_eval + 1) * nx : 0);
}

struct LbfgsArgs {
    int e, n_eval, nx, m, max_ls, has_trace;
    int two_loop;  // measurement aid (tools/probe_lbfgs.py, CMAX_LBFGS_TWO_LOOP): the textbook recursion, 2k + 1 dependent block reductions
    double c1, shrink, curv_eps, gtol, step0, max_move;
    double *x;   // the point the next evaluation reads, written in place
    double *st;  // the state above
    // the last evaluation: result block (final_loss, gnorm_inf, last_alpha, n_iter, n_eval_used, status as doubles) and, behind a system-wide
    // fence, the run counter -- *seq_src when given (the patch plan's tail counter), else seq -- both in pinned host memory
    double *res_pinned;
    volatile unsigned long long *flag;
    const unsigned long long *seq_src;
    unsigned long long seq;
};

// the regions of a state (device code and the copies out)
struct LbfgsView {
    double *ctrl, *gram, *x0, *xa, *ga, *d, *S, *Y, *loss, *alpha;
    int32_t *code;
    double *trace;
};
__host__ __device__ static inline LbfgsView lbfgs_view(double *st, int nx, int m, int n_eval) {
    LbfgsView v;
    v.ctrl = st;
    v.gram = st + kLbCtrl;
    v.x0 = st + kLbFixed;
    v.xa = v.x0 + nx;
    v.ga = v.xa + nx;
    v.d = v.ga + nx;
    v.S = v.d + nx;
    v.Y = v.S + (int64_t)m * nx;
    v.loss = v.Y + (int64_t)m * nx;
    v.alpha = v.loss + n_eval;
    v.code = reinterpret_cast<int32_t *>(v.alpha + n_eval);
    v.trace = v.alpha + n_eval + ((int64_t)n_eval + 1) / 2;
    return v;
}

// arguments of evaluation `e`
static inline LbfgsArgs lbfgs_args(const cmax_lbfgs_t &o, int e, int nx, bool trace, double *x, double *st) {
    LbfgsArgs a = {};
    a.e = e;
    a.n_eval = o.n_eval;
    a.nx = nx;
    a.m = o.history;
    a.max_ls = o.max_ls;
    a.has_trace = trace ? 1 : 0;
    a.c1 = o.c1;
    a.shrink = o.shrink;
    a.curv_eps = o.curv_eps;
    a.gtol = o.gtol;
    a.step0 = o.step0;
    a.max_move = o.max_move;
    a.x = x;
    a.st = st;
    return a;
}

// CMAX_EINVAL naming the field, before any launch
static inline int lbfgs_check(const cmax_lbfgs_t *o, const char *who) {
    const char *why = nullptr;
    if (!o) why = "null descriptor";
    else if (o->n_eval < 1 || o->n_eval > CMAX_DESCENT_MAX_ITER) why = "n_eval must be in 1 .. 4096";
    else if (o->history < 1 || o->history > CMAX_LBFGS_MAX_HISTORY) why = "history must be in 1 .. 16";
    else if (o->max_ls < 1) why = "max_ls must be at least 1";
    else if (!(o->c1 > 0.0 && o->c1 < 0.5)) why = "c1 must be in (0, 0.5)";
    else if (!(o->shrink > 0.0 && o->shrink < 1.0)) why = "shrink must be in (0, 1)";
    else if (!(std::isfinite(o->curv_eps) && o->curv_eps >= 0.0)) why = "curv_eps must be finite and not negative";
    else if (!(std::isfinite(o->gtol) && o->gtol >= 0.0)) why = "gtol must be finite and not negative";
    else if (!(std::isfinite(o->step0) && o->step0 > 0.0)) why = "step0 must be finite and positive";
    else if (!(std::isfinite(o->max_move) && o->max_move > 0.0)) why = "max_move must be finite and positive";
    if (!why) return 0;
    set_error("%s: bad lbfgs descriptor: %s", who, why);
    return CMAX_EINVAL;
}

// What the two entries ask of their caller before anything is reserved or enqueued, in descent_entry_check's order.  pointers: none of
// the entry's required pointers is null; d: the objective's descriptor (null for a patch plan); comm: the handle holds a communicator.
static inline int lbfgs_entry_check(const char *who, const cmax_lbfgs_t *o, bool pointers, const cmax_objective_t *d, bool comm) {
    const int rc = lbfgs_check(o, who);
    if (rc) return rc;
    const char *why = nullptr;
    if (!pointers) why = "null pointer";
    else if (d && d->model != CMAX_MODEL_2DOF) why = "2-DoF descriptors only (a dense flow / voxel is solved through a patch plan: cmax_patch_plan_lbfgs)";
    else if (d && d->motion_dtype != CMAX_F64) why = "the iterate is fp64 in device memory: desc->motion_dtype must be CMAX_F64";
    if (why) {
        set_error("bad argument: %s: %s", who, why);
        return CMAX_EINVAL;
    }
    if (comm) {
        set_error("%s: not built for time-sliced batches (the handle holds a communicator)", who);
        return CMAX_EUNSUPPORTED;
    }
    return 0;
}

// pinned result block -> the caller's struct
static inline void lbfgs_result(const double *res_pinned, cmax_lbfgs_result_t *out) {
    out->final_loss = res_pinned[0];
    out->gnorm_inf = res_pinned[1];
    out->last_alpha = res_pinned[2];
    out->n_iter = (int32_t)res_pinned[3];
    out->n_eval_used = (int32_t)res_pinned[4];
    out->status = (int32_t)res_pinned[5];
}

// x_a, the three logs and (x_trace_host non-null) the trace of the FINAL device state to the caller: one copy per region queued on s,
// the caller waits for the stream.
static inline int lbfgs_copy_out(double *st, int nx, int m, int n_eval, double *x_host, double *loss_history_host, double *alpha_host,
                                 int32_t *code_host, double *x_trace_host, hipStream_t s) {
    const LbfgsView v = lbfgs_view(st, nx, m, n_eval);
    CMAX_CHECK_HIP(hipMemcpyAsync(x_host, v.xa, (size_t)nx * sizeof(double), hipMemcpyDeviceToHost, s));
    CMAX_CHECK_HIP(hipMemcpyAsync(loss_history_host, v.loss, (size_t)n_eval * sizeof(double), hipMemcpyDeviceToHost, s));
    CMAX_CHECK_HIP(hipMemcpyAsync(alpha_host, v.alpha, (size_t)n_eval * sizeof(double), hipMemcpyDeviceToHost, s));
    CMAX_CHECK_HIP(hipMemcpyAsync(code_host, v.code, (size_t)n_eval * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (x_trace_host) CMAX_CHECK_HIP(hipMemcpyAsync(x_trace_host, v.trace, (size_t)((int64_t)n_eval + 1) * nx * sizeof(double), hipMemcpyDeviceToHost, s));
    return 0;
}

// cmax_solver.hip: one k_lbfgs_step launch; loss[1] and grad[nx] where the evaluation left them in device memory
__attribute__((visibility("hidden"))) int launch_lbfgs_step(const LbfgsArgs &a, const double *loss, const double *grad, hipStream_t s);

}  // namespace cmax
