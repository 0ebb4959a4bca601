"""TEST INFRASTRUCTURE ONLY: batches on which an fp64 dense flow / voxel and its fp32 rounding DISAGREE about cells, so that an evaluation
with `exact_flow=True` (cmax_objective_t::motion_dtype = CMAX_F64 for the flow models) is told apart from one that decided from
f32(flow).  Built on the helpers of tests/_cell_cases.py (imported, not restated).

Flows.  F = F32 + u ulp(F32), u uniform in (-0.49, 0.49): F32 is a smooth or a per-pixel random field of ~20 px per unit time as
_cell_cases draws them (fp32 values), so f32(F) = F32 and the residual r = F - f32(F) is what any fp64 field leaves behind its rounding.

Snapping.  x' = src - dt F[src] under the caller's flow and x'32 = x' + dt r under its rounding.  A selected event is placed, in fp64, so
that x' + 1e-6 lies at distance delta from an integer K on the side from which dt r pushes it ACROSS K:
    x' + 1e-6 = K + s delta,   s = -sign(dt r),   LOWER <= delta <= 0.6 |dt| |r|      (=> x'32 + 1e-6 = K - s (|dt r| - delta))
by solving for its time (integral sources) or its source fraction (fractional batches).  LOWER = _cell_cases.lower_bound, 16 x the
resolution of the packed time.  Only events with |dt| >= 0.4 and a non-empty interval are tried (|r| >= ulp / 4 at 20 px and |dt| = 0.5
leaves 7e-8 .. 1.4e-7 px; larger residuals and time offsets leave more), at most one per source pixel (and bin), never the first or the
last event, a voxel event stays in its bin; only events that two oracle warps (F, f32(F)) confirm to take different cells are kept.

tests/test_flow64_reference.py asserts per case, without a GPU: the flips, that the oracle's gradient at f32(F) misses the gate by 10 x
in the snapped events' source pixels, that the checkers below fail on it, and the numpy restatement of the device's split."""
import numpy as np

from oracle import oracle as orc

import _cell_cases as C
from _event_grad_ref import event_grad_objective

TOL = C.TOL  # the project's gate
BASE = C.BASE
DENSE, VOXEL = C.DENSE, C.VOXEL
MIN_DT = 0.4


def ulp32(x):
    """Spacing of fp32 at x on the side of zero (the smaller one at a power of two)."""
    x = np.abs(np.asarray(x, dtype=np.float32))
    return np.maximum((x - np.nextafter(x, np.float32(0))).astype(np.float64), 2.0 ** -149)


def flow64(kind, size, mag, seed, T=0):
    """fp64 flow [2, H, W] (T = 0) or voxel [T, 2, H, W], no entry representable in fp32, f32(F) = the _cell_cases field."""
    make = C.smooth_flow if kind == "smooth" else C.random_flow
    F32 = make(size, mag, seed) if T == 0 else np.stack([make(size, mag, seed + 17 * t) for t in range(T)])
    u = np.random.default_rng(seed + 5).uniform(-0.49, 0.49, F32.shape)
    u = np.where(np.abs(u) < 0.02, 0.02, u)
    F = F32 + u * ulp32(F32)
    assert (C.f32(F) == F32).all() and (F != F32).all()
    return F


def split_numpy(v):
    """The device's split (split_f64, csrc/cmax_common.h) in numpy: hi = (float)v, lo = (float)(v - hi), lo = 0 where hi is not finite."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(np.float32)
        lo = (v - hi.astype(np.float64)).astype(np.float32)
    return hi, np.where(np.isfinite(hi), lo, np.float32(0))


# ---------------------------------------------------------------------------------------------------------------------------------
# snapping
# ---------------------------------------------------------------------------------------------------------------------------------
def _flips(ev, F, model, size, direction, normalize_t, idx, axis):
    c64 = C.fp64_cells(ev, F, model, size, direction, normalize_t)
    c32 = C.fp64_cells(ev, C.f32(F), model, size, direction, normalize_t)
    return c64[axis][idx] != c32[axis][idx]


def _keeps_lower(ev, F, model, size, direction, normalize_t, idx, axis, low):
    warped, _ = orc.warp_event(ev, F, model, direction, size, normalize_t)
    xs = warped[idx, axis] + 1e-6
    return np.abs(xs - np.rint(xs)) >= low


def snap_flip_time(ev, F, model, size, idx, axis, direction="first", normalize_t=True, T=0, seed=0, near=None):
    """Moves ev[idx, 2] -> (events, the subset of idx whose cell on `axis` differs under F and f32(F)).  near: the new normalised time
    stays within `near` of the old one (large motions: the event keeps landing where it did)."""
    rng = np.random.default_rng(seed)
    ev = ev.copy()
    idx = np.asarray(idx, dtype=np.int64)
    idx = idx[(idx != 0) & (idx != ev.shape[0] - 1)]
    t = ev[:, 2].copy()
    t_lo, per = t.min(), t.max() - t.min()
    d, S, low = C.frac_of(direction), C._scale(ev, normalize_t), C.lower_bound(ev, F, normalize_t)
    c64 = C._coef(ev, F, model, size, T, axis)[idx]
    dc = c64 - C._coef(ev, C.f32(F), model, size, T, axis)[idx]  # x'(F) - x'(f32 F) = dt dc
    src = ev[idx, axis]
    if model == VOXEL:
        b = C._bins(ev, T)[idx]
        tau_lo, tau_hi = (b + 0.01) / T, (b + 0.99) / T
    else:
        tau_lo, tau_hi = np.full(len(idx), 0.002), np.full(len(idx), 0.998)
    if near is not None:
        tau_lo, tau_hi = np.maximum(tau_lo, C._tau(ev)[idx] - near), np.minimum(tau_hi, C._tau(ev)[idx] + near)
        idx, c64, dc, src, tau_lo, tau_hi = (a[tau_hi > tau_lo] for a in (idx, c64, dc, src, tau_lo, tau_hi))
    t_new, done = t[idx].copy(), np.zeros(len(idx), dtype=bool)
    for _ in range(8):
        u = rng.uniform(tau_lo, tau_hi)
        dt = (u - d) * S
        K = np.rint(src + dt * c64 + 1e-6)
        lo, hi = 1.05 * low, 0.6 * np.abs(dt * dc)
        delta = lo + rng.random(len(idx)) * np.maximum(hi - lo, 0.0)
        s = np.sign(dt * dc)  # = -sign(dt r): dc = -r
        with np.errstate(divide="ignore", invalid="ignore"):
            tau = d + (K + s * delta - 1e-6 - src) / (S * c64)
        ok = (hi > lo) & np.isfinite(tau) & (tau > tau_lo) & (tau < tau_hi) & (np.abs(tau - d) * S >= MIN_DT) & (np.abs(K - src) >= 1.0) & ~done
        ok &= (np.sign((tau - d) * dc) == np.sign(dt * dc)) & (delta <= 0.6 * np.abs((tau - d) * S * dc))  # (with the time it was solved for)
        t_new[ok] = t_lo + tau[ok] * per
        done |= ok
    ev[idx[done], 2] = t_new[done]
    idx = idx[done]
    good = _flips(ev, F, model, size, direction, normalize_t, idx, axis) & _keeps_lower(ev, F, model, size, direction, normalize_t, idx, axis, low)
    ev[idx[~good], 2] = t[idx[~good]]
    return ev, idx[good]


def snap_flip_source(ev, F, model, size, idx, axis, direction="first", normalize_t=True, T=0, seed=0, near=None):
    """Moves the source fraction ev[idx, axis] inside its pixel -> (events, the subset of idx that flips)."""
    rng = np.random.default_rng(seed)
    ev, orig = ev.copy(), ev
    idx = np.asarray(idx, dtype=np.int64)
    idx = idx[(idx != 0) & (idx != ev.shape[0] - 1)]
    d, S, low = C.frac_of(direction), C._scale(ev, normalize_t), C.lower_bound(ev, F, normalize_t)
    dt = ((C._tau(ev) - d) * S)[idx]
    c64 = C._coef(ev, F, model, size, T, axis)[idx]
    dc = c64 - C._coef(ev, C.f32(F), model, size, T, axis)[idx]
    disp, pix = dt * c64, np.floor(ev[idx, axis])
    lo, hi = 1.05 * low, 0.6 * np.abs(dt * dc)
    delta = lo + rng.random(len(idx)) * np.maximum(hi - lo, 0.0)
    s = np.sign(dt * dc)  # = -sign(dt r): dc = -r
    K = np.ceil(pix + disp + 0.002)
    new = K + s * delta - 1e-6 - disp
    ok = (hi > lo) & (np.abs(dt) >= MIN_DT) & (new > pix + 0.001) & (new < pix + 0.998) & (np.abs(disp) >= 1.0)
    ev[idx[ok], axis] = new[ok]
    idx = idx[ok]
    good = _flips(ev, F, model, size, direction, normalize_t, idx, axis) & _keeps_lower(ev, F, model, size, direction, normalize_t, idx, axis, low)
    ev[idx[~good], axis] = orig[idx[~good], axis]
    return ev, idx[good]


# ---------------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------------
def case(cid, model=DENSE, kind="random", n=4000, size=BASE, share=0.25, cost="image_variance", sigma=0, pad=0, warp_direction="first",
         frac=False, T=0, seed=0, mag=20.0, one=False, near=None):
    return dict(id=cid, model=model, kind=kind, n=n, size=size, share=share, cost=cost, sigma=sigma, pad=pad, warp_direction=warp_direction,
                normalize_t=True, frac=frac, T=T, seed=seed, mag=mag, one=one, near=near)


TABLE = [
    # motions on the base batch (40 x 56, 4000 events: t256)
    case("dense-smooth", kind="smooth", seed=1),
    case("dense-random", seed=2),
    case("voxel3", VOXEL, "random", T=3, seed=3),
    # reference times
    case("dense-middle", warp_direction="middle", seed=4),
    case("dense-last", warp_direction="last", seed=5),
    case("dense-third", warp_direction=1.0 / 3.0, seed=6),
    case("dense-multifocal", cost="multi_focal_normalized_image_variance", seed=7),
    # costs
    case("dense-var-blur", sigma=1, seed=8),
    case("dense-gm", cost="gradient_magnitude", seed=9),
    case("dense-gm-blur", cost="gradient_magnitude", sigma=1, seed=10),
    # sources
    case("dense-frac", frac=True, pad=3, seed=11),
    case("voxel3-frac", VOXEL, "random", T=3, frac=True, seed=12),
    # snapped share
    case("dense-all", share=1.0, seed=13),
    case("dense-one", one=True, seed=14),
    case("dense-none", share=0.0, seed=15),
    # the clipped window (150 px on 130 x 173) and sparse batches on a sensor with more than 512 / 1024 segments
    case("dense-clipped", kind="smooth", n=60_000, size=(130, 173), share=1.0, mag=150.0, seed=16, near=0.02),
    case("dense-t512", n=15_000, size=(720, 1280), share=1.0, seed=17),
    case("voxel10-t1024", VOXEL, "random", T=10, n=15_000, size=(720, 1280), share=1.0, seed=18),
]
# forced layouts, in child processes (tests/_flow64_worker.py)
WORKER = [
    case("mid-dense", n=600_000, size=(256, 256), share=0.02, seed=20),
    case("mid-voxel3", VOXEL, "random", T=3, n=600_000, size=(256, 256), share=0.02, seed=21),
    case("big-dense", n=30_000, share=0.1, seed=22),
]
BY_ID = {c["id"]: c for c in TABLE + WORKER}
SMALL = [c["id"] for c in TABLE if c["size"] == BASE]
_BUILT = {}


def _snap_set(ev, c, F, pool, direction, rng):
    """x-only and y-only halves of `pool` -> (events, snapped indices)"""
    snap = snap_flip_source if c["frac"] else snap_flip_time
    kept = []
    for axis, part in enumerate(np.array_split(np.asarray(pool, dtype=np.int64), 2)):
        ev, keep = snap(ev, F, c["model"], c["size"], part, axis, direction, c["normalize_t"], c["T"], seed=int(rng.integers(1 << 30)), near=c["near"])
        kept.append(keep)
    return ev, np.concatenate(kept)


def built(cid):
    """The case with its batch: ev, motion (fp64), motion32 = f32(motion) as fp64, snapped (indices that flip, confirmed on the final batch)."""
    if cid in _BUILT:
        return _BUILT[cid]
    c = dict(BY_ID[cid])
    model, size, T, n, seed = c["model"], c["size"], c["T"], c["n"], c["seed"]
    ev = C.batch(n, size, 100 + seed, c["frac"])
    F = flow64(c["kind"], size, c["mag"], 900 + seed, T)
    rng = np.random.default_rng(200 + seed)
    dirs = C.directions_of(c)
    pool = C.one_per_pixel(ev, size, T, n, 200 + seed)  # every event that is alone in its pixel (and bin) ...
    if c["mag"] > 100.0:  # large motions: only events that land on the sensor read a gradient
        land = np.ones(n, dtype=bool)
        for direction in dirs:
            xy, _ = orc.warp_event(ev, F, model, direction, size, c["normalize_t"])
            land &= (xy[:, 0] > 4) & (xy[:, 0] < size[0] - 5) & (xy[:, 1] > 4) & (xy[:, 1] < size[1] - 5)
        pool = pool[land[pool]]
    count = len(pool) if (c["one"] or c["share"] >= 1.0) else min(len(pool), int(round(c["share"] * n)))
    pool = rng.permutation(pool)[:count]  # ... or share x n of them are TRIED; the snapped events are those that can flip and verify
    snapped = []
    for di, part in enumerate(np.array_split(pool, len(dirs))):
        if len(part):
            ev, keep = _snap_set(ev, c, F, part, dirs[di], rng)
            snapped.append(keep)
    snapped = np.concatenate(snapped) if snapped else np.zeros(0, dtype=np.int64)
    if c["one"] and len(snapped) > 1:  # exactly one: the others go back to where they were
        orig = C.batch(n, size, 100 + seed, c["frac"])
        ev[snapped[1:]] = orig[snapped[1:]]
        snapped = snapped[:1]
    # on the final batch: which of them flip, at which reference time
    flip = np.zeros(len(snapped), dtype=bool)
    for direction in dirs:
        for axis in (0, 1):
            flip |= _flips(ev, F, model, size, direction, c["normalize_t"], snapped, axis)
    c.update(ev=ev, motion=F, motion32=C.f32(F), snapped=snapped[flip])
    _BUILT[cid] = c
    return c


def measured(cid):
    """built(cid) plus the fp64 references: c["full"] at the caller's flow, c["full32"] at its fp32 rounding (event_grad_objective: loss,
    grad, grad_events, iwes, image_grads), once per process."""
    c = built(cid)
    if "full" not in c:
        kw = C.ref_kwargs(c)
        c["full"] = event_grad_objective(c["ev"], c["motion"], c["model"], c["size"], 1.0, **kw)
        c["full32"] = event_grad_objective(c["ev"], c["motion32"], c["model"], c["size"], 1.0, **kw)
    return c


def snapped_rows(c, g):
    """[k, 2]: both channels of the motion gradient `g` at the snapped events' source pixels (and bins)."""
    ix, iy = C._pixel(c["ev"][c["snapped"]], c["size"])
    if c["model"] == VOXEL:
        b = C._bins(c["ev"], c["T"])[c["snapped"]]
        return np.stack([g[b, 0, ix, iy], g[b, 1, ix, iy]], axis=1)
    return np.stack([g[0, ix, iy], g[1, ix, iy]], axis=1)


def rounding_gap(c, per_event=False):
    """max over the snapped events' gradient rows of |grad(f32 F) - grad(F)|, relative to the largest gradient entry: what a result
    computed on the rounded flow misses the reference by (per_event: the figure of every snapped event)."""
    g64, g32 = c["full"]["grad"], c["full32"]["grad"]
    d = np.abs(snapped_rows(c, g32) - snapped_rows(c, g64)).max(axis=1) / np.abs(g64).max()
    return d if per_event else float(d.max(initial=0.0))


# ---------------------------------------------------------------------------------------------------------------------------------
# the checkers of tests/test_gpu_flow64.py
# ---------------------------------------------------------------------------------------------------------------------------------
def rel_max(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def check_field(tag, got, ref, what="grad"):
    """A motion gradient / Hessian-vector product / image / dL/dw at 1e-4 of its largest reference entry."""
    e = rel_max(got, ref)
    print(f"[flow64] {tag}: {what} rel err {e:.2e}")
    assert e <= TOL, (tag, what, e)
    return e


def check_loss(tag, got, ref):
    e = abs(float(got) - float(ref)) / abs(float(ref))
    print(f"[flow64] {tag}: loss rel err {e:.2e}")
    assert e <= TOL, (tag, "loss", e)
    return e


def check_per_event(tag, got, ref):
    return C.check_per_event(f"flow64 {tag}", got, ref)


# ---------------------------------------------------------------------------------------------------------------------------------
# K candidate flows on one batch, each with its own snapped third (objective_batch)
# ---------------------------------------------------------------------------------------------------------------------------------
def batch_case(K=3, n=4000, size=BASE, seed=60):
    if "batch" in _BUILT:
        return _BUILT["batch"]
    c = case("batch", seed=seed)
    ev = C.batch(n, size, seed)
    flows = np.stack([flow64("random", size, 20.0, seed + 31 * k) for k in range(K)])
    pool = C.one_per_pixel(ev, size, 0, n, seed)
    rng = np.random.default_rng(seed)
    snapped = []
    for k, part in enumerate(np.array_split(pool, K)):
        ev, keep = _snap_set(ev, c, flows[k], part, "first", rng)
        snapped.append(keep)
    for k in range(K):  # (on the final batch)
        flip = _flips(ev, flows[k], DENSE, size, "first", True, snapped[k], 0) | _flips(ev, flows[k], DENSE, size, "first", True, snapped[k], 1)
        snapped[k] = snapped[k][flip]
    _BUILT["batch"] = dict(ev=ev, flows=flows, snapped=snapped, size=size)
    return _BUILT["batch"]


# ---------------------------------------------------------------------------------------------------------------------------------
# the patch plan: 64 x 80 sensor, 4 x 5 patch grid; events snapped against the fp64 dense flow / voxel tests/_patch_ref.py computes from x
# ---------------------------------------------------------------------------------------------------------------------------------
PLAN_SIZE, PLAN_GRID, PLAN_SW = (64, 80), (4, 5), (16, 16)
PLAN_KINDS = {"dense": dict(time_aware=False, T=0, scale_later=False),
              "burgers3": dict(time_aware=True, T=3, scale_later=False),
              "scale-later": dict(time_aware=True, T=3, scale_later=True)}


def plan_case(kind, n=6000, seed=70):
    """-> dict(ev, x, v, spec (round32 False: the reference solver's own fp64 chain), spec32 (the fp32 rounding the default plan evaluates),
    motion (fp64 field of x), snapped, loss / grad / hv at either spec)."""
    key = "plan/" + kind
    if key in _BUILT:
        return _BUILT[key]
    import _patch_ref  # (torch: only the plan cases need it)

    kw = PLAN_KINDS[kind]
    model = VOXEL if kw["time_aware"] else DENSE
    ev = C.batch(n, PLAN_SIZE, seed)
    t_scale = float(ev[:, 2].max() - ev[:, 2].min())
    rng = np.random.default_rng(seed + 1)
    x = (rng.uniform(-20.0, 20.0, (2,) + PLAN_GRID) / t_scale).reshape(-1)  # ~20 px over the batch, nothing of it a multiple of 2^-10
    spec = dict(size=PLAN_SIZE, patch_image_size=PLAN_GRID, sw=PLAN_SW, pad=_patch_ref.patch_pad(PLAN_SW, PLAN_SW), t_scale=t_scale,
                terms=(("image_variance", 1.0),), sigma=1.0, tv_weight=0.01, tv_omit=True, omit=True, scheme="burgers", t0="middle",
                round32=False, **kw)
    F = _patch_ref.device_motion(x, spec)  # (round32 False: the fp64 field itself)
    assert (C.f32(F) != F).mean() > 0.99
    c = case(key, model=model, T=kw["T"], seed=seed)
    pool = rng.permutation(C.one_per_pixel(ev, PLAN_SIZE, kw["T"], n, seed))
    ev, snapped = _snap_set(ev, c, F, pool, "first", rng)
    flip = _flips(ev, F, model, PLAN_SIZE, "first", True, snapped, 0) | _flips(ev, F, model, PLAN_SIZE, "first", True, snapped, 1)
    v = rng.normal(0.0, 1.0, x.shape)
    out = dict(ev=ev, x=x, v=v, spec=spec, spec32=dict(spec, round32=True), motion=F, snapped=snapped[flip], model=model, kind=kind)
    out["loss"], out["grad"], out["hv"] = _patch_ref.plan(x, ev, spec, v=v)
    out["loss32"], out["grad32"], out["hv32"] = _patch_ref.plan(x, ev, out["spec32"], v=v)
    _BUILT[key] = out
    return out
