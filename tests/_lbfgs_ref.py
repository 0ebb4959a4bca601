"""The device-resident L-BFGS (cmax_patch_plan_lbfgs / cmax_objective_lbfgs) restated in numpy, as a state machine: the rules of
include/cmax_hip.h, one evaluation per `transition`.  The direction is the textbook two-loop recursion over the held pairs; the
kernel evaluates the same recursion on Gram coefficients.  `minimize` drives it from the host; the GPU tests drive it teacher-forced
(state["x"] is overwritten with the traced point before every transition, so the history is rebuilt from the TRACED accepted points).

    state = start(x0, desc);  loop:  L, g = f(state["x"]);  state, x_next = transition(state, L, g)
"""
import numpy as np

BUDGET, CONVERGED, LINESEARCH, BOX, NONFINITE_START = 0, 1, 2, 3, 4
STATUS_WORDS = {BUDGET: "BUDGET", CONVERGED: "CONVERGED", LINESEARCH: "LINESEARCH", BOX: "BOX", NONFINITE_START: "NONFINITE_START"}
START, ACCEPTED, REJECTED, RESET, IDLE = 0, 1, 2, 3, 4
# every branch of the rule; `transition` adds the ones it takes to state["branches"]
BRANCHES = ("reject", "reset", "linesearch", "skipped_pair", "nondescent_reset", "box", "converged_at_start", "nonfinite_trial",
            "nonfinite_start", "accept", "push", "drop_oldest", "converged", "clipped_alpha")


def descriptor(n_eval, history=8, max_ls=10, c1=1e-4, shrink=0.5, curv_eps=1e-10, gtol=1e-5, step0=1.0, max_move=1.0):
    return dict(n_eval=int(n_eval), history=int(history), max_ls=int(max_ls), c1=float(c1), shrink=float(shrink), curv_eps=float(curv_eps),
                gtol=float(gtol), step0=float(step0), max_move=float(max_move))


def two_loop(pairs, g):
    """-H g by the L-BFGS recursion, pairs oldest first, H0 = (s^T y / y^T y) I of the newest pair."""
    q, a = g.copy(), []
    for s, y in reversed(pairs):
        ai = (s @ q) / (s @ y)
        a.append(ai)
        q = q - ai * y
    s, y = pairs[-1]
    r = (s @ y) / (y @ y) * q
    for (s, y), ai in zip(pairs, reversed(a)):
        b = (y @ r) / (s @ y)
        r = r + (ai - b) * s
    return -r


def start(x0, desc):
    x0 = np.array(x0, dtype=np.float64).reshape(-1)
    return dict(desc=desc, e=0, x=x0.copy(), x0=x0.copy(), xa=None, La=None, ga=None, d=None, alpha=0.0, gd=0.0, n_ls=0, n_iter=0, pairs=[],
                done=False, status=BUDGET, used=0, last_alpha=0.0, ginf=0.0, branches=set(), margin=None)


def _trial(st):
    o = st["desc"]
    return np.minimum(np.maximum(st["xa"] + st["alpha"] * st["d"], st["x0"] - o["max_move"]), st["x0"] + o["max_move"])


def _choose(st):
    """Direction, first alpha and the box at the accepted point -> the next trial point (or BOX)."""
    o, g = st["desc"], st["ga"]
    d = None
    if st["pairs"]:
        d = two_loop(st["pairs"], g)
        if not g @ d < 0.0:
            st["pairs"], d = [], None
            st["branches"].add("nondescent_reset")
    if d is None:
        d, alpha = -g, min(1.0, o["step0"] / np.abs(g).sum())
    else:
        alpha = 1.0
    lo, hi = st["x0"] - o["max_move"], st["x0"] + o["max_move"]
    with np.errstate(divide="ignore", invalid="ignore"):
        lim = np.where(d > 0.0, (hi - st["xa"]) / d, np.where(d < 0.0, (lo - st["xa"]) / d, np.inf))
    if lim.min() < alpha:
        st["branches"].add("clipped_alpha")
    st["d"], st["gd"], st["alpha"] = d, float(g @ d), float(min(alpha, lim.min()))
    if not st["alpha"] > 0.0:
        st["status"], st["done"] = BOX, True
        st["branches"].add("box")
        return st["xa"].copy()
    return _trial(st)


def transition(st, L, g):
    """One evaluation: (L, g) at st["x"] -> (state, the next point to evaluate, None once the budget is spent).  The per-evaluation
    outputs are left in st["code"], st["alpha_e"], st["loss_e"]; st["margin"] is the Armijo margin of a decision (None without one)."""
    o, e = st["desc"], st["e"]
    L, g = float(L), np.asarray(g, dtype=np.float64).reshape(-1)
    st["margin"], st["alpha_e"], st["loss_e"] = None, 0.0, L
    finite = bool(np.isfinite(L) and np.isfinite(g).all())
    if st["done"]:
        st["code"], st["loss_e"], x_next = IDLE, np.nan, st["xa"].copy()
    elif e == 0:
        st["code"] = START
        if not finite:
            st["status"], st["done"], st["xa"], st["La"], st["ginf"] = NONFINITE_START, True, st["x"].copy(), L, np.nan
            st["branches"].add("nonfinite_start")
            x_next = st["xa"].copy()
        else:
            st["xa"], st["La"], st["ga"], st["ginf"] = st["x"].copy(), L, g.copy(), float(np.abs(g).max())
            if st["ginf"] <= o["gtol"]:
                st["status"], st["done"] = CONVERGED, True
                st["branches"].add("converged_at_start")
                x_next = st["xa"].copy()
            else:
                x_next = _choose(st)
    else:
        st["alpha_e"] = st["alpha"]
        bound = st["La"] + o["c1"] * st["alpha"] * st["gd"]
        if np.isfinite(L):
            st["margin"] = bound - L
        ok = finite and L <= bound
        if not ok:
            st["n_ls"] += 1
            st["code"] = REJECTED
            st["branches"].add("reject" if finite else "nonfinite_trial")
            if st["n_ls"] > o["max_ls"] and not st["pairs"]:
                st["status"], st["done"] = LINESEARCH, True
                st["branches"].add("linesearch")
                x_next = st["xa"].copy()
            elif st["n_ls"] > o["max_ls"]:
                st["code"], st["pairs"], st["n_ls"] = RESET, [], 0
                st["branches"].add("reset")
                x_next = _choose(st)
            else:
                st["alpha"] *= o["shrink"]
                x_next = _trial(st)
        else:
            st["code"] = ACCEPTED
            st["branches"].add("accept")
            s, y = st["x"] - st["xa"], g - st["ga"]
            if y @ y > 0.0 and s @ y > o["curv_eps"] * (y @ y):
                st["branches"].add("push")
                if len(st["pairs"]) == o["history"]:
                    st["pairs"].pop(0)
                    st["branches"].add("drop_oldest")
                st["pairs"].append((s, y))
            else:
                st["branches"].add("skipped_pair")
            st["xa"], st["La"], st["ga"], st["ginf"] = st["x"].copy(), L, g.copy(), float(np.abs(g).max())
            st["n_iter"] += 1
            st["n_ls"], st["last_alpha"] = 0, st["alpha"]
            if st["ginf"] <= o["gtol"]:
                st["status"], st["done"] = CONVERGED, True
                st["branches"].add("converged")
                x_next = st["xa"].copy()
            else:
                x_next = _choose(st)
    if st["done"] and st["used"] == 0:
        st["used"] = e + 1
    st["e"] = e + 1
    st["x"] = x_next
    return st, (x_next if st["e"] < o["n_eval"] else None)


def minimize(fun, x0, desc):
    """fun(x) -> (L, g), driven from the host: what one library call returns, as a dictionary (plus the branches taken and the Armijo
    margins of the decisions, relative to max(1, |L_a|))."""
    st = start(x0, desc)
    n = desc["n_eval"]
    trace, loss, alpha, code, margins = np.empty((n + 1, st["x0"].size)), np.empty(n), np.empty(n), np.empty(n, dtype=np.int32), []
    for e in range(n):
        trace[e] = st["x"]
        La = st["La"]
        st, _ = transition(st, *fun(st["x"]))
        loss[e], alpha[e], code[e] = st["loss_e"], st["alpha_e"], st["code"]
        if st["margin"] is not None:
            margins.append(abs(st["margin"]) / max(1.0, abs(La)))
    trace[n] = st["xa"]
    return dict(x=st["xa"].copy(), fun=st["La"], gnorm_inf=st["ginf"], status=st["status"], nit=st["n_iter"], nfev=st["used"] if st["done"] else n,
                last_alpha=st["last_alpha"], loss_history=loss, alpha=alpha, code=code, trace=trace, branches=st["branches"],
                margins=np.array(margins), state=st)
