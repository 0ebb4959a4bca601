"""Plans, starts and descriptors of the device-resident L-BFGS tests, shared by tests/test_gpu_lbfgs.py (the kernel) and
tests/test_lbfgs_reference.py (the same cases through tests/_lbfgs_ref.minimize over tests/_patch_ref.plan on the CPU: which branches
they take and that no Armijo decision is close).

The batches of tests/_patch_cases.py hold point features moving by (4, -3) pixels over the period.  A start drawn around 0.8 of that
motion lies where the contrast has curvature, so that pairs are pushed, dropped and sometimes skipped; the random starts of the descent
tests lie on the flat part, where every pair is skipped and the history stays empty."""
import numpy as np

import _patch_cases as C
import _patch_ref

BURGERS = dict(time_aware=True, T=10, scheme="burgers", t0="middle")
N_EVAL = 16
# the three geometries of tests/test_gpu_descent.py, chosen for nx: 2 (below a wave), 24, 4140 (a grid-stride remainder); every history
# {1, 3, 8} and every variant {plain, tv, burgers} at least once
RULE = {
    "1x1-m1-plain": dict(gid="1x1-pad0", size=(20, 28), history=1, variant="plain", seed=1, max_move=100.0),
    "3x4-m3-tv": dict(gid="3x4-odd", size=(27, 40), history=3, variant="tv", seed=1, max_move=100.0),
    "3x4-m8-burgers": dict(gid="3x4-odd", size=(27, 40), history=8, variant="burgers", seed=1, max_move=100.0),
    "46x45-m3-plain": dict(gid="46x45", size=(92, 90), history=3, variant="plain", seed=3, max_move=1000.0),
    "46x45-m8-tv": dict(gid="46x45", size=(92, 90), history=8, variant="tv", seed=3, max_move=1000.0),
}
# parameters picked by running tests/_lbfgs_ref.minimize over tests/_patch_ref.plan (tests/test_lbfgs_reference.py asserts what they
# take there): a first step of 1-norm 2000 on a plan whose gradient is large enough for step0 to bind; the same with max_ls = 1; a box
# a hundredth of the distance the free solve travels; max_ls = 1 with shrink 0.9 on starts that accept first, so that two rejects in a row
# meet a NON-EMPTY history: the reset branch, at nx 24 (twice, history 8) and at nx 4140
FORCED = {
    "reset-3x4-m8": dict(gid="3x4-odd", size=(27, 40), history=8, variant="burgers", seed=1, max_move=100.0, max_ls=1, shrink=0.9),
    "reset-46x45-m3": dict(gid="46x45", size=(92, 90), history=3, variant="plain", seed=3, max_move=1000.0, max_ls=1, shrink=0.9),
    "overshoot": dict(gid="3x4-odd", size=(27, 40), history=3, variant="plain", seed=1, max_move=1e4, step0=2000.0, weight=1e6),
    "max-ls-1": dict(gid="3x4-odd", size=(27, 40), history=3, variant="plain", seed=1, max_move=1e4, step0=2000.0, weight=1e6, max_ls=1),
    "small-box": dict(gid="3x4-odd", size=(27, 40), history=3, variant="plain", seed=1, max_move=0.25),
}


def start(gid, seed, frac=0.8, px=0.5):
    pis = C.GEOMETRY[gid]["patch_image_size"]
    base = np.stack([np.full(pis, 4.0 * frac), np.full(pis, -3.0 * frac)])
    m = base + np.random.default_rng(seed).normal(0, px, (2,) + tuple(pis))
    return (np.round(m / C.PERIOD * 1024.0) / 1024.0).reshape(-1)  # multiples of 2^-10, as tests/_patch_cases.patch_motion


def descriptor_kwargs(c, n_eval=N_EVAL):
    kw = dict(n_eval=n_eval, history=c["history"], gtol=1e-9, max_move=c["max_move"], step0=c.get("step0", 1.0), max_ls=c.get("max_ls", 10),
              shrink=c.get("shrink", 0.5))
    return kw


def inputs(c):
    """-> (events, spec, x0, with_tv)"""
    ev = C.batch(c["size"])
    kw = dict(BURGERS) if c["variant"] == "burgers" else {}
    if "weight" in c:  # the forced cases: the plans' gradients are ~1e-3 as they are, so a first step of min(1, step0 / |g|_1) is never too
        kw["terms"] = tuple((name, w * c["weight"]) for name, w in C.YAML_HYBRID)  # long on them; a hybrid weight scales loss and gradient
    spec = C.spec_of(c["gid"], c["size"], t_scale=float(ev[:, 2].max() - ev[:, 2].min()), **kw)
    return ev, spec, start(c["gid"], c["seed"]), c["variant"] == "tv"


def reference_fun(c):
    """x -> (L, g) of the case's plan in fp64 on the CPU (tests/_patch_ref.plan)."""
    ev, spec, _, tv = inputs(c)

    def fun(x):
        L, g, _ = _patch_ref.plan(x, ev, spec, with_tv=tv)
        return float(L), np.asarray(g, dtype=np.float64).reshape(-1)

    return fun
