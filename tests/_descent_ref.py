"""TEST INFRASTRUCTURE ONLY: the update rule of the device-resident descent (cmax_patch_plan_descend / cmax_objective_descend, pinned in
include/cmax_hip.h) restated in plain numpy fp64 -- torch.optim.SGD / Adam under StepLR, as SolverBase.run_torch calls them
(src/solver/base.py:840-881).  tests/test_descent_reference.py holds it to torch's own optimisers; tests/test_gpu_descent.py holds the
kernels to it."""
import numpy as np


def options(method, lr=0.05, lr_step=1, lr_decay=0.1, momentum=0.0, beta1=0.9, beta2=0.999, eps=1e-8):
    return dict(method=method, lr=float(lr), lr_step=int(lr_step), lr_decay=float(lr_decay), momentum=float(momentum), beta1=float(beta1),
                beta2=float(beta2), eps=float(eps))


def learning_rate(it, opt):
    """StepLR: lr_it = lr * lr_decay^floor(it / lr_step)."""
    return opt["lr"] * opt["lr_decay"] ** (it // opt["lr_step"])


def step(state, x, g, it, opt):
    """Iteration `it` (0-based): the optimiser's state (a dict, empty before iteration 0) is updated in place from the gradient g at x;
    returns the next iterate."""
    x, g = np.asarray(x, dtype=np.float64), np.asarray(g, dtype=np.float64)
    lr = learning_rate(it, opt)
    if opt["method"] == "SGD":
        state["buf"] = g.copy() if it == 0 else opt["momentum"] * state["buf"] + g
        return x - lr * state["buf"]
    if opt["method"] == "Adam":
        b1, b2, t = opt["beta1"], opt["beta2"], it + 1
        state["m"] = b1 * state.get("m", 0.0) + (1.0 - b1) * g
        state["v"] = b2 * state.get("v", 0.0) + (1.0 - b2) * g * g
        return x - (lr / (1.0 - b1 ** t)) * state["m"] / (np.sqrt(state["v"]) / np.sqrt(1.0 - b2 ** t) + opt["eps"])
    raise KeyError(opt["method"])


def best_of(history):
    """(best_loss, best_iter) of the strict comparison `L_it < best_loss` from +inf: the first occurrence of the minimum; a NaN never
    wins; (inf, -1) when no entry is below +inf."""
    best, best_it = np.inf, -1
    for it, loss in enumerate(history):
        if loss < best:
            best, best_it = float(loss), it
    return best, best_it
