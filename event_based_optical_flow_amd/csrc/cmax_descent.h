// Device-resident SGD / Adam (cmax_patch_plan_descend, cmax_objective_descend, cmax_objective_descend_batch; the rules are pinned in
// include/cmax_hip.h): the update of one iteration as the kernels that apply it share it -- k_descent_step (cmax_solver.hip: one workgroup,
// any nx), k_finish_raw_step (cmax_fused.hip: lane 63 of the one-wave finishing kernel, nx = 2) and its sibling k_finish_raw_step_batch
// (one such wave per candidate, every candidate its own state) -- and what the three entries share on the host: the checks of descriptor
// and arguments (descent_check, descent_entry_check), the view of a final state's regions (descent_view) and the one routine that hands
// them to the caller (descent_copy_out), from device memory or from a host copy of the state.  The state's layout is written in this file
// only: the device functions below and descent_view.
// SolverBase.run_torch, src/solver/base.py:840-881.
#pragma once
#include <cmath>
#include <cstring>

#include "cmax_common.h"

namespace cmax {

// Descent state in device memory (doubles): ctrl[kDcCtrl] | x_best[nx] | x_last[nx] | m[nx] | v[nx] | loss_history[n_iter] | x_trace[(n_iter + 1) nx]
// Iteration 0 reads none of it (best = +inf, m = v = 0 by rule): a call never sees what an earlier call left.
constexpr int kDcBest = 0, kDcBestIter = 1, kDcDone = 2, kDcStopped = 3, kDcLastLr = 4, kDcCtrl = 8;
static inline int64_t descent_state_doubles(int nx, int n_iter, bool trace) {
    return kDcCtrl + 4 * (int64_t)nx + n_iter + (trace ? ((int64_t)n_iter + 1) * nx : 0);
}

struct DescentArgs {
    int method, it, n_iter, nx, has_trace;
    double lr_it;             // lr * lr_decay^floor(it / lr_step)
    double momentum, beta1, beta2, eps;
    double bc1, bc2_sqrt;     // Adam: 1 - beta1^t, sqrt(1 - beta2^t), t = it + 1
    double *x;                // the iterate, stepped in place
    double *st;               // the state above
    // the last iteration: result block (best_loss, best_iter, n_done, last_lr as doubles) and, behind a system-wide fence, the run counter
    // -- *seq_src when given (the patch plan's tail counter), else seq -- both in pinned host memory
    double *res_pinned;
    volatile unsigned long long *flag;
    const unsigned long long *seq_src;
    unsigned long long seq;
};

// arguments of iteration `it`
static inline DescentArgs descent_args(const cmax_descent_t &o, int it, int nx, bool trace, double *x, double *st) {
    DescentArgs a = {};
    a.method = o.method;
    a.it = it;
    a.n_iter = o.n_iter;
    a.nx = nx;
    a.has_trace = trace ? 1 : 0;
    a.lr_it = o.lr * std::pow(o.lr_decay, (double)(it / o.lr_step));
    a.momentum = o.momentum;
    a.beta1 = o.beta1;
    a.beta2 = o.beta2;
    a.eps = o.eps;
    a.bc1 = 1.0 - std::pow(o.beta1, (double)(it + 1));
    a.bc2_sqrt = std::sqrt(1.0 - std::pow(o.beta2, (double)(it + 1)));
    a.x = x;
    a.st = st;
    return a;
}

// CMAX_EINVAL with the reason, before any launch
static inline int descent_check(const cmax_descent_t *o, const char *who) {
    const char *why = nullptr;
    if (!o) why = "null descriptor";
    else if (o->method != CMAX_OPT_SGD && o->method != CMAX_OPT_ADAM) why = "unknown method (CMAX_OPT_SGD or CMAX_OPT_ADAM)";
    else if (o->n_iter < 1 || o->n_iter > CMAX_DESCENT_MAX_ITER) why = "n_iter must be in 1 .. 4096";
    else if (!(std::isfinite(o->lr) && o->lr > 0.0)) why = "lr must be finite and positive";
    else if (!(std::isfinite(o->lr_decay) && o->lr_decay > 0.0)) why = "lr_decay must be finite and positive";
    else if (!(std::isfinite(o->eps) && o->eps > 0.0)) why = "eps must be finite and positive";
    else if (o->lr_step < 1) why = "lr_step must be at least 1";
    else if (!(o->momentum >= 0.0 && o->momentum < 1.0)) why = "momentum must be in [0, 1)";
    else if (!(o->beta1 >= 0.0 && o->beta1 < 1.0)) why = "beta1 must be in [0, 1)";
    else if (!(o->beta2 >= 0.0 && o->beta2 < 1.0)) why = "beta2 must be in [0, 1)";
    if (!why) return 0;
    set_error("%s: bad descent descriptor: %s", who, why);
    return CMAX_EINVAL;
}

// What the three entries ask of their caller before anything is reserved or enqueued.  pointers: none of the entry's required pointers is
// null; d: the objective's descriptor (null for a patch plan, whose terms were checked when it was made); comm: the handle holds a communicator.
static inline int descent_entry_check(const char *who, const cmax_descent_t *o, bool pointers, const cmax_objective_t *d, bool comm) {
    const int rc = descent_check(o, who);
    if (rc) return rc;
    const char *why = nullptr;
    if (!pointers) why = "null pointer";
    else if (d && d->model != CMAX_MODEL_2DOF) why = "2-DoF descriptors only (a dense flow / voxel descends through a patch plan: cmax_patch_plan_descend)";
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
static inline void descent_result(const double *res_pinned, cmax_descent_result_t *out) {
    out->best_loss = res_pinned[0];
    out->best_iter = (int32_t)res_pinned[1];
    out->n_done = (int32_t)res_pinned[2];
    out->last_lr = res_pinned[3];
}

// The regions of one state that a caller receives, from the layout above (host code's only reading of it; m and v stay the kernels')
struct DescentView {
    const double *ctrl, *x_best, *x_last, *history, *trace;
};
static inline DescentView descent_view(const double *st, int nx, int n_iter) {
    const double *xb = st + kDcCtrl, *hist = xb + 4 * (int64_t)nx;
    return {st, xb, xb + nx, hist, hist + n_iter};
}

// x_best, x_last, the history and (x_trace_host non-null) the trace of the FINAL state `st` to the caller.  on_device: st is device memory
// -- one copy per region queued on s, the caller waits for the stream; otherwise st is host memory that holds the state already.
static inline int descent_copy_out(const double *st, bool on_device, int nx, int n_iter, double *x_best_host, double *x_last_host,
                                   double *loss_history_host, double *x_trace_host, hipStream_t s) {
    const DescentView v = descent_view(st, nx, n_iter);
    const struct {
        double *dst;
        const double *src;
        int64_t n;
    } part[4] = {{x_best_host, v.x_best, nx}, {x_last_host, v.x_last, nx}, {loss_history_host, v.history, n_iter}, {x_trace_host, v.trace, ((int64_t)n_iter + 1) * nx}};
    for (const auto &c : part) {
        if (!c.dst) continue;
        if (on_device) CMAX_CHECK_HIP(hipMemcpyAsync(c.dst, c.src, (size_t)c.n * sizeof(double), hipMemcpyDeviceToHost, s));
        else std::memcpy(c.dst, c.src, (size_t)c.n * sizeof(double));
    }
    return 0;
}
// the control block of a final state in host memory -> the caller's struct
static inline void descent_result_of_state(const double *ctrl, cmax_descent_result_t *out) {
    out->best_loss = ctrl[kDcBest];
    out->best_iter = (int32_t)ctrl[kDcBestIter];
    out->n_done = (int32_t)ctrl[kDcDone];
    out->last_lr = ctrl[kDcLastLr];
}

// cmax_solver.hip: one k_descent_step launch; loss[1] and grad[nx] where the evaluation left them in device memory
__attribute__((visibility("hidden"))) int launch_descent_step(const DescentArgs &a, const double *loss, const double *grad, hipStream_t s);

#if defined(__HIPCC__)
struct DescentDecision {
    bool stopped_prev, stop, better;
    double best, best_iter, done, last_lr;  // the control block after this iteration
};
// Reads the control block (every thread that takes part in descent_element; the writer waits for them).  bad: L_it or an entry of g_it
// is not finite.
__device__ __forceinline__ DescentDecision descent_decide(const DescentArgs &a, double L, bool bad) {
    DescentDecision d;
    const bool first = a.it == 0;
    d.stopped_prev = !first && a.st[kDcStopped] != 0.0;
    d.stop = d.stopped_prev || bad;
    const double best = first ? (double)INFINITY : a.st[kDcBest];
    d.better = !d.stopped_prev && L < best;  // (strict; a NaN never wins)
    d.best = d.better ? L : best;
    d.best_iter = d.better ? (double)a.it : (first ? -1.0 : a.st[kDcBestIter]);
    d.done = d.stop ? (first ? 0.0 : a.st[kDcDone]) : (double)(a.it + 1);
    d.last_lr = d.stop ? (first ? 0.0 : a.st[kDcLastLr]) : a.lr_it;
    return d;
}
// entry p: trace, x_best, the optimiser's state, the step, and (last iteration) x_last
__device__ __forceinline__ void descent_element(const DescentArgs &a, const DescentDecision &d, int p, double g) {
    const int nx = a.nx;
    double *xb = a.st + kDcCtrl, *xl = xb + nx, *m = xl + nx, *v = m + nx, *trace = v + nx + a.n_iter;
    double x = a.x[p];
    if (a.has_trace) trace[(int64_t)a.it * nx + p] = x;
    if (d.better || a.it == 0) xb[p] = x;  // (iteration 0 without a finite loss: x_best = x0)
    if (!d.stop) {
        if (a.method == CMAX_OPT_SGD) {
            const double buf = a.it == 0 ? g : a.momentum * m[p] + g;
            m[p] = buf;
            x -= a.lr_it * buf;
        } else {
            const double mm = a.it == 0 ? (1.0 - a.beta1) * g : a.beta1 * m[p] + (1.0 - a.beta1) * g;
            const double vv = a.it == 0 ? (1.0 - a.beta2) * g * g : a.beta2 * v[p] + (1.0 - a.beta2) * g * g;
            m[p] = mm;
            v[p] = vv;
            x -= (a.lr_it / a.bc1) * mm / (sqrt(vv) / a.bc2_sqrt + a.eps);
        }
        a.x[p] = x;
    }
    if (a.it == a.n_iter - 1) {
        xl[p] = x;
        if (a.has_trace) trace[(int64_t)a.n_iter * nx + p] = x;
    }
}
// one thread, after every descent_decide of the launch has read the control block
__device__ __forceinline__ void descent_publish(const DescentArgs &a, const DescentDecision &d, double L) {
    double *hist = a.st + kDcCtrl + 4 * (int64_t)a.nx;
    hist[a.it] = d.stopped_prev ? (double)NAN : L;
    a.st[kDcBest] = d.best;
    a.st[kDcBestIter] = d.best_iter;
    a.st[kDcDone] = d.done;
    a.st[kDcStopped] = d.stop ? 1.0 : 0.0;
    a.st[kDcLastLr] = d.last_lr;
    if (a.it == a.n_iter - 1 && a.res_pinned) {
        a.res_pinned[0] = d.best;
        a.res_pinned[1] = d.best_iter;
        a.res_pinned[2] = d.done;
        a.res_pinned[3] = d.last_lr;
    }
}
#endif

}  // namespace cmax
