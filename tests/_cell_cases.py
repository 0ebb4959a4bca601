"""TEST INFRASTRUCTURE ONLY: batches whose events are SNAPPED onto cell borders, so that every kernel that decides a cell in fp64
(k_vote, k_vote_tan, k_vote_tan2, k_grad_hvp: exact_margin -> warp_exact) and every kernel that follows the published nibbles (k_grad,
k_weight_gather, k_event_grad_gather) is driven on purpose, and the per-event reading dL/d(x', y') shows every single decision.

Snapping.  `bilinear_vote` takes the cell floor(x' + 1e-6).  For a selected event the builder solves, linearly in fp64, for the event's
TIME (integral sources) or for its SOURCE FRACTION (fractional batches: the second axis of a corner is only reachable that way) so that
x' + 1e-6 -- as orc.warp_event computes it -- lies at a signed distance `delta` from an integer, verifies with one more orc.warp_event
call and keeps only the events that verify.  The first and the last event (sorted times: t_min, t_max) are never touched; a voxel event
stays inside its time bin; a dense / voxel case snaps at most one event per source pixel (and bin), so that every entry of the flow
gradient it touches is one event's reading.

|delta|: between LOWER = 16 * |motion|_max * 2^-32 (|motion| in pixels per normalised time: 16 x the resolution of the packed time, fp32
plus a residual byte) and 0.25 ulp of the event's fp32 displacement on that axis; the LADDER population instead takes
|delta| log-uniform from max(2^-28, LOWER) to 2^-12 px, both signs -- it asks whether exact_margin is wide enough wherever fp32 can still
flip, without restating it.  An exact tie is not defined and not built.

`fp32_cells` restates the device's split-base fp32 arithmetic (ix + floor(fl(rx +- dt32 f32) + 1e-6f), cmax_event_launch.hip warp_one) in numpy:
what a kernel WITHOUT exact cells computes.  tests/test_cell_reference.py asserts per case that it disagrees with the fp64 cell often
enough, that reading the wrong cell moves the per-event gradient by far more than the gate, and that the checker the GPU test uses
fails on a result composed from those cells."""
import numpy as np

from oracle import oracle as orc

import _hvp_ref
from _border import _event_grad
from _event_grad_ref import event_grad_objective
from _weighted_ref import weighted_objective

TOL = 1e-4  # the project's gate, per column of grad_events, relative to the column's largest reference entry
BASE = (40, 56)
_FRAC = {"first": 0.0, "middle": 0.5, "last": 1.0}
_MULTI = ("last", "first", "middle")  # (cmax._COST_TABLE's order)
_KEY_OF = {"last": "forward_iwe", "middle": "middle_iwe"}


def f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def frac_of(direction):
    return _FRAC[direction] if isinstance(direction, str) else float(direction)


def directions_of(c):
    return list(_MULTI) if c["cost"].startswith("multi_focal") else [c["warp_direction"]]


def _key_of(c, direction):
    return _KEY_OF[direction] if c["cost"].startswith("multi_focal") and direction in _KEY_OF else "iwe"


# ---------------------------------------------------------------------------------------------------------------------------------
# batches and motions (plain numpy: the anchor does not import the package)
# ---------------------------------------------------------------------------------------------------------------------------------
def batch(n, size, seed, frac=False, t_max=0.05):
    rng = np.random.default_rng(seed)
    ev = np.empty((n, 4))
    ev[:, 0] = rng.integers(0, size[0], n)
    ev[:, 1] = rng.integers(0, size[1], n)
    ev[:, 2] = np.sort(rng.uniform(0.0, t_max, n))
    ev[:, 3] = rng.integers(0, 2, n)
    if frac:
        ev[:, :2] += rng.uniform(0.001, 0.998, (n, 2))
    return ev


def smooth_flow(size, mag, seed):
    rng = np.random.default_rng(seed)
    r, c = np.meshgrid(np.linspace(0, 1, size[0]), np.linspace(0, 1, size[1]), indexing="ij")
    out = np.zeros((2,) + tuple(size))
    for ch in range(2):
        for _ in range(3):
            fr, fc, p = rng.uniform(0.3, 1.5, 2).tolist() + [rng.uniform(0, 2 * np.pi)]
            out[ch] += rng.uniform(0.4, 1.0) * np.sin(2 * np.pi * (fr * r + fc * c) + p)
        out[ch] *= mag / np.abs(out[ch]).max()
    return f32(out)


def random_flow(size, mag, seed):
    return f32(np.random.default_rng(seed).uniform(-mag, mag, (2,) + tuple(size)))


def _tau(ev):
    t = ev[:, 2]
    return (t - t.min()) / (t.max() - t.min())


def _pixel(ev, size, clip=False):
    ix, iy = np.floor(ev[:, 0]).astype(np.int64), np.floor(ev[:, 1]).astype(np.int64)
    if clip:  # kept off-sensor events: the nearest sensor pixel
        ix, iy = np.clip(ix, 0, size[0] - 1), np.clip(iy, 0, size[1] - 1)
    return ix, iy


def _bins(ev, T):
    return np.minimum((_tau(ev) * T).astype(np.int64), T - 1)


def _coef(ev, motion, model, size, T, axis):
    """x' = src + dt * coef on `axis`, per event (fp64 from the values the device holds)."""
    m = np.asarray(motion, dtype=np.float64)
    if model == "2d-translation":
        return np.full(ev.shape[0], m[axis])
    ix, iy = _pixel(ev, size)
    if model == "dense-flow":
        return -m[axis, ix, iy]
    return -m[_bins(ev, T), axis, ix, iy]


def _scale(ev, normalize_t):
    return 1.0 if normalize_t else float(ev[:, 2].max() - ev[:, 2].min())


def lower_bound(ev, motion, normalize_t=True):
    return 16.0 * float(np.abs(np.asarray(motion)).max()) * _scale(ev, normalize_t) * 2.0 ** -32


def _ulp32(d):
    d = np.maximum(np.abs(d), 2.0 ** -100)
    return 2.0 ** (np.floor(np.log2(d)) - 23)


def _delta(rng, disp, low, ladder):
    """signed target distance per event and whether it exists"""
    n = disp.shape[0]
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    if ladder:
        lo = max(2.0 ** -28, 1.05 * low)
        mag = 2.0 ** rng.uniform(np.log2(lo), -12.0, n)
        return sign * mag, np.ones(n, dtype=bool)
    lo, hi = 1.25 * low, 0.2 * _ulp32(disp)
    ok = hi > lo
    return sign * (lo + rng.random(n) * np.maximum(hi - lo, 0.0)), ok


def _verify(ev, motion, model, size, idx, axis, direction, normalize_t, want, low, ladder):
    """-> mask over idx: x' + 1e-6 (orc.warp_event) lies at the wanted side and distance of an integer."""
    warped, _ = orc.warp_event(ev, motion, model, direction, size, normalize_t)
    xs = warped[idx, axis] + 1e-6
    dist = xs - np.rint(xs)
    disp = warped[idx, axis] - ev[idx, axis]
    ok = (np.sign(dist) == np.sign(want)) & (np.abs(dist) >= low)
    ok &= np.abs(dist) <= (2.0 ** -12 * 1.001 if ladder else 0.25 * _ulp32(disp))
    return ok


def snap_time(ev, motion, model, size, idx, axis, direction="first", normalize_t=True, T=0, ladder=False, seed=0, near=None):
    """Moves ev[idx, 2] (in place on a copy) -> (events, the subset of idx that verified).  near: the new normalised time stays within
    `near` of the old one (large motions: the event keeps landing where it did)."""
    rng = np.random.default_rng(seed)
    ev = ev.copy()
    idx = np.asarray(idx, dtype=np.int64)
    idx = idx[(idx != 0) & (idx != ev.shape[0] - 1)]
    t = ev[:, 2].copy()
    t_lo, per = t.min(), t.max() - t.min()
    assert t[0] == t.min() and t[-1] == t.max()
    d, S, low = frac_of(direction), _scale(ev, normalize_t), lower_bound(ev, motion, normalize_t)
    coef, src = _coef(ev, motion, model, size, T, axis)[idx], ev[idx, axis]
    if model == "dense-flow-voxel":
        b = _bins(ev, T)[idx]
        w = 1.0 / T
        tau_lo, tau_hi = (b + 0.01) * w, (b + 0.99) * w
    else:
        tau_lo, tau_hi = np.full(len(idx), 0.002), np.full(len(idx), 0.998)
    if near is not None:
        tau_lo, tau_hi = np.maximum(tau_lo, _tau(ev)[idx] - near), np.minimum(tau_hi, _tau(ev)[idx] + near)
        idx, coef, src, tau_lo, tau_hi = (a[tau_hi > tau_lo] for a in (idx, coef, src, tau_lo, tau_hi))
    t_new, done = t[idx].copy(), np.zeros(len(idx), dtype=bool)
    want = np.zeros(len(idx))
    for _ in range(6):
        u = rng.uniform(tau_lo, tau_hi)
        K = np.rint(src + (u - d) * S * coef + 1e-6)
        delta, ok = _delta(rng, K - src, low, ladder)
        with np.errstate(divide="ignore", invalid="ignore"):
            tau = d + (K + delta - 1e-6 - src) / (S * coef)
        ok &= np.isfinite(tau) & (tau > tau_lo) & (tau < tau_hi) & (np.abs(K - src) >= 1.0) & ~done
        t_new[ok], want[ok] = t_lo + tau[ok] * per, delta[ok]
        done |= ok
    ev[idx[done], 2] = t_new[done]
    idx, want = idx[done], want[done]
    good = _verify(ev, motion, model, size, idx, axis, direction, normalize_t, want, low, ladder)
    ev[idx[~good], 2] = t[idx[~good]]  # (t holds the original times)
    return ev, idx[good]


def snap_source(ev, motion, model, size, idx, axis, direction="first", normalize_t=True, ladder=False, seed=0):
    """Moves the source fraction ev[idx, axis] inside its pixel -> (events, the subset of idx that verified)."""
    rng = np.random.default_rng(seed)
    ev, orig = ev.copy(), ev
    idx = np.asarray(idx, dtype=np.int64)
    idx = idx[(idx != 0) & (idx != ev.shape[0] - 1)]
    low = lower_bound(ev, motion, normalize_t)
    warped, _ = orc.warp_event(ev, motion, model, direction, size, normalize_t)
    disp, src = (warped[:, axis] - ev[:, axis])[idx], ev[idx, axis]
    pix = np.floor(src)
    delta, ok = _delta(rng, disp, low, ladder)
    K = np.ceil(pix + disp + 0.002)
    new = K + delta - 1e-6 - disp
    ok &= (new > pix + 0.001) & (new < pix + 0.998) & (np.abs(disp) >= 1.0)
    ev[idx[ok], axis] = new[ok]
    idx, want = idx[ok], delta[ok]
    good = _verify(ev, motion, model, size, idx, axis, direction, normalize_t, want, low, ladder)
    ev[idx[~good], axis] = orig[idx[~good], axis]
    return ev, idx[good]


def active_pixels(ev, size):
    """Source pixels that hold events: the library takes a batch for one of LONG RUNS (the run-reducing dense K3 instead of the strided one,
    the compact event copy of big segments) when n >= 8 x this count."""
    ix, iy = _pixel(ev, size, clip=True)
    return int(len(np.unique(ix * size[1] + iy)))


def one_per_pixel(ev, size, T, count, seed):
    """`count` event indices, no two from the same source pixel (and time bin)."""
    rng = np.random.default_rng(seed)
    ix, iy = _pixel(ev, size)
    key = (ix * size[1] + iy) * max(T, 1) + (_bins(ev, T) if T else 0)
    perm = rng.permutation(ev.shape[0])
    _, first = np.unique(key[perm], return_index=True)
    pick = perm[first]
    pick = pick[(pick != 0) & (pick != ev.shape[0] - 1)]
    return np.sort(rng.permutation(pick)[:count])


# ---------------------------------------------------------------------------------------------------------------------------------
# cells
# ---------------------------------------------------------------------------------------------------------------------------------
def fp64_cells(ev, motion, model, size, direction, normalize_t=True):
    """(row, col) of floor(x' + 1e-6), un-padded, as the oracle computes it."""
    warped, _ = orc.warp_event(ev, motion, model, direction, size, normalize_t)
    return np.floor(warped[:, 0] + 1e-6).astype(np.int64), np.floor(warped[:, 1] + 1e-6).astype(np.int64)


def fp32_cells(ev, motion, model, size, direction, normalize_t=True, T=0):
    """The split-base fp32 formula a kernel without exact cells evaluates: tau, d and the period rounded to fp32, tau - d rounded,
    times the period rounded, dx = fl(rx +- dt f) (one rounding: an fma), cell = ix + floor(fl(dx + 1e-6f))."""
    F = np.float32
    d32, S32 = F(frac_of(direction)), F(_scale(ev, normalize_t))
    dt = ((_tau(ev).astype(F) - d32) * S32).astype(F)
    ix, iy = _pixel(ev, size, clip=True)
    out = []
    for axis, pix in ((0, ix), (1, iy)):
        coef = _coef_clipped(ev, motion, model, size, T, axis).astype(F)
        rx = (ev[:, axis] - pix).astype(F)
        dx = (dt.astype(np.float64) * coef.astype(np.float64) + rx.astype(np.float64)).astype(F)  # (the product of two fp32 is exact in fp64)
        out.append(pix + np.floor((dx + F(1e-6)).astype(F)).astype(np.int64))
    return out[0], out[1]


def _coef_clipped(ev, motion, model, size, T, axis):
    if model == "2d-translation":
        return np.full(ev.shape[0], float(np.asarray(motion)[axis]))
    return _coef(ev, motion, model, size, T, axis)


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference's per-event reading, from the right cells or from any others
# ---------------------------------------------------------------------------------------------------------------------------------
def ref_kwargs(c):
    return dict(cost=c["cost"], sigma=c["sigma"], outer_padding=c["pad"], normalize_t=c["normalize_t"], warp_direction=c["warp_direction"])


def image_grads(c, out=None):
    """{direction: dL/d(raw votes) [Hp, Wp]} of the case, from the oracle (the blur transposed back)."""
    if out is None:
        out = weighted_objective(c["ev"], c["motion"], c["model"], c["size"], 1.0, **ref_kwargs(c))
    merged = {}
    for k, g in out["image_grads"].items():
        kk = "iwe" if k == "backward_iwe" else k
        merged[kk] = merged.get(kk, 0) + g
    res = {}
    for direction in directions_of(c):
        G = np.ascontiguousarray(merged[_key_of(c, direction)], dtype=np.float64)
        res[direction] = orc.blur3_adj(G, c["sigma"]) if c["sigma"] > 0 else G
    return res


def event_xy_grad(c, cells=None, G=None):
    """grad_events[:, 0:2] of the case in fp64: orc.vote_bwd per reference time.  cells = {direction: (row, col)}: the coordinates are
    nudged across the border into THAT cell first (by twice their distance to it: at most 2^-11 px) -- what an evaluation that took
    those cells returns."""
    G = image_grads(c) if G is None else G
    ev = orc._ev4(c["ev"])
    out = np.zeros((ev.shape[0], 2))
    for direction in directions_of(c):
        xy, _ = orc.warp_event(ev, c["motion"], c["model"], direction, c["size"], c["normalize_t"])
        if cells is not None:
            for axis in (0, 1):
                xs = xy[:, axis] + 1e-6
                move = cells[direction][axis] - np.floor(xs).astype(np.int64)
                assert np.abs(move).max() <= 1
                dist = xs - np.rint(xs)
                assert np.abs(dist[move != 0]).max(initial=0.0) <= 2.0 ** -11
                xy[:, axis] = np.where(move != 0, xy[:, axis] - 2.0 * dist, xy[:, axis])
                assert (np.floor(xy[:, axis] + 1e-6).astype(np.int64) == cells[direction][axis]).all()
        gx, gy = orc.vote_bwd(xy, c["size"], G[direction], c["pad"])
        out[:, 0] += gx
        out[:, 1] += gy
    return out


def check_per_event(tag, got, ref, c=None):
    """THE checker of tests/test_gpu_exact_cells.py: every event's (gx, gy) at 1e-4 of the column's largest reference entry."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    e = [np.abs(got[:, k] - ref[:, k]).max() / max(np.abs(ref[:, k]).max(), 1e-300) for k in range(2)]
    extra = "" if c is None else f" snapped {len(c['snapped'])} fp32-wrong {c['n_flip']}"
    print(f"[exact cells] {tag}: per-event rel err x {e[0]:.2e} y {e[1]:.2e}{extra}")
    assert max(e) <= TOL, (tag, e)
    return max(e)


# ---------------------------------------------------------------------------------------------------------------------------------
# conditions of a case (asserted by tests/test_cell_reference.py)
# ---------------------------------------------------------------------------------------------------------------------------------
def measure(c):
    """-> dict of the case's CPU figures."""
    ev, motion, model, size = c["ev"], c["motion"], c["model"], c["size"]
    low = lower_bound(ev, motion, c["normalize_t"])
    full = event_grad_objective(ev, motion, model, size, 1.0, **ref_kwargs(c))
    G = image_grads(c, full)
    ref = full["grad_events"][:, :2]
    colmax = np.abs(ref).max(axis=0)
    snapped, axes, sdir, ladder = c["snapped"], c["axes"], c["sdir"], c["ladder"]
    worst_ulp, min_dist, flips, disc = 0.0, np.inf, np.zeros(len(snapped), dtype=bool), np.zeros(len(snapped), dtype=bool)
    cells32 = {}
    for di, direction in enumerate(directions_of(c)):
        warped, _ = orc.warp_event(ev, motion, model, direction, size, c["normalize_t"])
        r64, c64 = fp64_cells(ev, motion, model, size, direction, c["normalize_t"])
        cells32[direction] = fp32_cells(ev, motion, model, size, direction, c["normalize_t"], c["T"])
        for axis in (0, 1):
            sel = np.nonzero((sdir == di) & (((axes >> axis) & 1) == 1))[0]
            if len(sel) == 0:
                continue
            idx = snapped[sel]
            xs = warped[idx, axis] + 1e-6
            dist = np.abs(xs - np.rint(xs))
            min_dist = min(min_dist, dist.min())
            nl = ~ladder[sel]
            if nl.any():
                worst_ulp = max(worst_ulp, (dist[nl] / _ulp32(warped[idx, axis] - ev[idx, axis])[nl]).max())
            flips[sel] |= cells32[direction][axis][idx] != (r64, c64)[axis][idx]
            # the same event read from the cell across the snapped border
            other = np.where(xs - np.rint(xs) >= 0, -1, 1)
            fx, fy = r64[idx].astype(np.float64), c64[idx].astype(np.float64)
            Gz = np.pad(G[direction], 2)
            ph, pw = _hvp_ref._pad2(c["pad"])
            g0 = _event_grad(Gz, fx + ph, fy + pw, warped[idx, 0] + ph, warped[idx, 1] + pw)
            g1 = _event_grad(Gz, fx + ph + (other if axis == 0 else 0), fy + pw + (other if axis == 1 else 0), warped[idx, 0] + ph, warped[idx, 1] + pw)
            disc[sel] |= (np.abs(g1[0] - g0[0]) >= 1e-2 * colmax[0]) | (np.abs(g1[1] - g0[1]) >= 1e-2 * colmax[1])
    # every event of the batch that moves at all keeps LOWER from every border: nothing in the batch is an undefined tie
    for direction in directions_of(c):
        warped, _ = orc.warp_event(ev, motion, model, direction, size, c["normalize_t"])
        xs = warped[:, :2] + 1e-6
        moved = np.abs(warped[:, :2] - ev[:, :2]) > 0
        min_dist = min(min_dist, np.abs(xs - np.rint(xs))[moved].min(initial=np.inf))
    nl = ~ladder
    return dict(n_snapped=len(snapped), n_ladder=int(ladder.sum()), lower=low, min_dist=float(min_dist), worst_ulp=float(worst_ulp),
                flip_share=float(flips[nl].mean()) if nl.any() else 0.0, n_flip=int(flips.sum()), disc_share=float(disc.mean()) if len(disc) else 0.0,
                ref=ref, full=full, cells32=cells32, G=G)


# ---------------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------------
def case(cid, model="2d-translation", motion="theta64", n=4000, size=BASE, share=0.25, pop="xy", cost="image_variance", sigma=0, pad=0,
         warp_direction="first", normalize_t=True, frac=False, outside=False, T=0, seed=0, ladder_share=0.2, mag=8.0, one=False, near=None):
    return dict(id=cid, model=model, motion_kind=motion, n=n, size=size, share=share, pop=pop, cost=cost, sigma=sigma, pad=pad,
                warp_direction=warp_direction, normalize_t=normalize_t, frac=frac, outside=outside, T=T, seed=seed, ladder_share=ladder_share,
                mag=mag, one=one, near=near)


TWO, DENSE, VOXEL = "2d-translation", "dense-flow", "dense-flow-voxel"
THETA = np.array([7.3, -4.1])

TABLE = [
    # models on the base batch (t256, eight events per thread)
    case("2dof-f64"),
    case("2dof-f32", motion="theta32", seed=1),
    case("dense-smooth", DENSE, "smooth", seed=2, share=0.45),
    case("dense-random", DENSE, "random", seed=3, share=0.45),
    case("voxel3", VOXEL, "smooth", T=3, seed=4, mag=14.0, share=0.45),
    # reference times
    case("2dof-middle", warp_direction="middle", seed=5),
    case("2dof-last", warp_direction="last", seed=6),
    case("2dof-third", warp_direction=1.0 / 3.0, seed=7),
    case("dense-middle", DENSE, "smooth", warp_direction="middle", seed=8, mag=14.0, share=0.45),
    case("dense-third", DENSE, "smooth", warp_direction=1.0 / 3.0, seed=9, mag=14.0, share=0.45),
    case("2dof-multifocal", cost="multi_focal_normalized_gradient_magnitude", sigma=1, seed=10),
    case("dense-multifocal", DENSE, "smooth", cost="multi_focal_normalized_image_variance", seed=11, mag=14.0, share=0.45),
    case("2dof-rawtime", normalize_t=False, seed=12),
    case("dense-rawtime", DENSE, "smooth", normalize_t=False, seed=13, share=0.45),
    # costs (the K3 folds)
    case("2dof-gm", cost="gradient_magnitude", seed=14),
    case("2dof-var-blur", sigma=1, seed=15),
    case("dense-gm-blur", DENSE, "smooth", cost="gradient_magnitude", sigma=1, seed=16, share=0.45),
    case("2dof-gm-blur", cost="gradient_magnitude", sigma=1, seed=32),
    case("dense-gm", DENSE, "smooth", cost="gradient_magnitude", seed=33, share=0.45),
    case("dense-var-blur", DENSE, "smooth", sigma=1, seed=34, share=0.45),
    # the entries that take an fp32 theta only (hvp, fused_iwes) at a reference time fp32 cannot hold, and with fractional sources
    case("2dof-f32-0.3", motion="theta32", warp_direction=0.3, seed=35),
    case("2dof-f32-frac", motion="theta32", frac=True, pad=3, seed=36),
    # sources
    case("2dof-frac", frac=True, pad=3, seed=17),
    case("dense-frac", DENSE, "smooth", frac=True, pad=3, seed=18, share=0.45),
    case("voxel3-frac", VOXEL, "smooth", T=3, frac=True, seed=19, mag=14.0, share=0.45),
    case("2dof-outside", frac=True, outside=True, pad=6, seed=20, motion="theta-far"),
    # density
    case("2dof-all", share=1.0, seed=21),
    case("dense-all", DENSE, "smooth", share=1.0, seed=22),
    case("2dof-one", one=True, seed=51, motion="theta-b"),
    case("dense-one", DENSE, "smooth", one=True, seed=24),
    case("2dof-none", share=0.0, seed=25),
    # dense K3 variants: long runs (n >= 8 x active pixels) against the strided short-run form of the base batch
    case("dense-long-runs", DENSE, "smooth", n=24_000, share=0.05, seed=26),
    # the clipped window (global atomics): 150 px on 130 x 173
    case("2dof-clipped", n=60_000, size=(130, 173), share=0.05, motion="theta-150", seed=51, near=0.02),
    case("dense-clipped", DENSE, "smooth", n=60_000, size=(130, 173), share=0.04, mag=150.0, seed=28, near=0.02),
    # t512 / t1024: a sparse batch on a sensor with more than 512 / 1024 segments
    case("2dof-t512", n=15_000, size=(720, 1280), share=0.25, seed=29),
    case("dense-t512", DENSE, "smooth", n=15_000, size=(720, 1280), share=0.25, seed=30),
    case("voxel10-t1024", VOXEL, "smooth", T=10, n=15_000, size=(720, 1280), share=0.25, seed=31, mag=40.0),
]
# the forced layouts of tests/_cell_worker.py: the batch the mid layout is cut from, and the 30 000-event batch for big segments
WORKER = [
    case("mid-2dof", n=600_000, size=(256, 256), share=0.02, seed=40),
    case("mid-dense", DENSE, "smooth", n=600_000, size=(256, 256), share=0.02, seed=41),
    case("mid-voxel3", VOXEL, "smooth", T=3, n=600_000, size=(256, 256), share=0.02, seed=42, mag=14.0),
    case("big-2dof", n=30_000, share=0.25, seed=43),
    case("big-dense", DENSE, "smooth", n=30_000, share=0.02, seed=44),
]
BY_ID = {c["id"]: c for c in TABLE + WORKER}
_BUILT = {}


def _motion_of(c):
    kind, size = c["motion_kind"], c["size"]
    if kind == "theta64":
        return THETA.copy()
    if kind == "theta32":
        return f32([7.3, -4.1])
    if kind == "theta-b":
        return np.array([-5.7, 6.9])
    if kind == "theta-far":
        return np.array([17.0, -21.0])
    if kind == "theta-150":
        return np.array([150.0, -140.0])
    make = smooth_flow if kind == "smooth" else random_flow
    if c["model"] == DENSE:
        return make(size, c["mag"], 900 + c["seed"])
    return np.stack([make(size, c["mag"], 900 + c["seed"] + 17 * t) for t in range(c["T"])])


def _snap_axis(ev, c, motion, idx, axis, direction, ladder, rng):
    """One population of one case on one axis: by the source fraction on fractional batches, else by the time."""
    kw = dict(direction=direction, normalize_t=c["normalize_t"], ladder=ladder, seed=int(rng.integers(1 << 30)))
    if c["frac"]:
        return snap_source(ev, motion, c["model"], c["size"], idx, axis, **kw)
    return snap_time(ev, motion, c["model"], c["size"], idx, axis, T=c["T"], near=c["near"], **kw)


def built(cid):
    """The case with its batch: ev, motion, snapped (indices), axes (bit 0: x, bit 1: y), sdir (the reference time each snapped event is
    snapped at), ladder (mask over snapped).  Built once per process."""
    if cid in _BUILT:
        return _BUILT[cid]
    c = dict(BY_ID[cid])
    model, size, T, n, seed = c["model"], c["size"], c["T"], c["n"], c["seed"]
    ev = batch(n, size, 100 + seed, c["frac"])
    motion = _motion_of(c)
    if c["normalize_t"] is False:
        motion = f32(motion / (ev[:, 2].max() - ev[:, 2].min())) if model != TWO else motion / (ev[:, 2].max() - ev[:, 2].min())
    if c["outside"]:
        rng = np.random.default_rng(300 + seed)
        out = rng.random(n) < 0.33
        out[[0, n - 1]] = False
        ev[out, 0] = rng.uniform(-25.0, size[0] + 25.0, int(out.sum()))
        ev[out, 1] = rng.uniform(-25.0, size[1] + 25.0, int(out.sum()))
    rng = np.random.default_rng(200 + seed)
    count = 1 if c["one"] else int(round(c["share"] * n))
    if model == TWO:
        pool = rng.permutation(np.arange(1, n - 1))[: (64 if c["one"] else count)]
    else:
        pool = one_per_pixel(ev, size, T, 64 if c["one"] else count, 200 + seed)
    dirs = directions_of(c)
    if c["near"] is not None:  # large motions: only events that land on the sensor (at every reference time) read a gradient
        land = np.ones(n, dtype=bool)
        for direction in dirs:
            xy, _ = orc.warp_event(ev, motion, model, direction, size, c["normalize_t"])
            land &= (xy[:, 0] > 4) & (xy[:, 0] < size[0] - 5) & (xy[:, 1] > 4) & (xy[:, 1] < size[1] - 5)
        pool = pool[land[pool]]
    snapped, axes, sdir, ladder = [], [], [], []
    for di, part in enumerate(np.array_split(rng.permutation(pool), len(dirs))):  # a share of the pool per reference time
        n_lad = 0 if c["one"] else int(round(c["ladder_share"] * len(part)))
        for members, lad in ((part[:n_lad], True), (part[n_lad:], False)):
            if len(members) == 0:
                continue
            # populations: x only, y only and -- fractional batches -- corners
            subs = np.array_split(members, 3 if c["frac"] else 2)
            found = []
            ev, keep = _snap_axis(ev, c, motion, subs[0], 0, dirs[di], lad, rng)
            found.append((keep, 1))
            ev, keep = _snap_axis(ev, c, motion, subs[1], 1, dirs[di], lad, rng)
            found.append((keep, 2))
            if c["frac"]:
                ev, keep_x = _snap_axis(ev, c, motion, subs[2], 0, dirs[di], lad, rng)
                ev, keep_xy = _snap_axis(ev, c, motion, keep_x, 1, dirs[di], lad, rng)
                found += [(np.setdiff1d(keep_x, keep_xy), 1), (keep_xy, 3)]  # (what only the first axis kept stays x-only)
            for idx, bits in found:
                snapped += list(idx)
                axes += [bits] * len(idx)
                sdir += [di] * len(idx)
                ladder += [lad] * len(idx)
    snapped, axes, ladder = np.asarray(snapped, dtype=np.int64), np.asarray(axes, dtype=np.int64), np.asarray(ladder, dtype=bool)
    if c["one"] and len(snapped) > 1:  # exactly ONE: the others go back to where they were
        flip = np.zeros(len(snapped), dtype=bool)  # the one that stays is one a kernel without exact cells gets wrong
        c64, c32 = fp64_cells(ev, motion, model, size, dirs[0], c["normalize_t"]), fp32_cells(ev, motion, model, size, dirs[0], c["normalize_t"], T)
        for axis in (0, 1):
            flip |= (((axes >> axis) & 1) == 1) & (c64[axis][snapped] != c32[axis][snapped])
        keep = int(np.argmax(~ladder & flip))
        assert flip[keep] and not ladder[keep]
        orig = batch(n, size, 100 + seed, c["frac"])
        back = np.delete(snapped, keep)
        ev[back] = orig[back]
        snapped, axes, sdir, ladder = snapped[keep:keep + 1], axes[keep:keep + 1], [sdir[keep]], ladder[keep:keep + 1]
    c.update(ev=ev, motion=motion, snapped=snapped, axes=axes, sdir=np.asarray(sdir, dtype=np.int64), ladder=ladder)
    _BUILT[cid] = c
    return c


def measured(cid):
    """built(cid) plus its CPU figures and the fp64 per-event reference (c["ref"]), once per process."""
    c = built(cid)
    if "ref" not in c:
        c.update(measure(c))
    return c


# ---------------------------------------------------------------------------------------------------------------------------------
# K candidate motions on one batch (objective_batch), and two motions on one handle (stale nibbles)
# ---------------------------------------------------------------------------------------------------------------------------------
def _motions(model, size, k, seed):
    if model == TWO:
        return np.array([[7.3, -4.1], [-5.7, 6.9], [6.1, 5.3]])[:k]
    return np.stack([smooth_flow(size, 8.0, seed + 31 * j) for j in range(k)])


def _snap_set(ev, motion, model, size, pool, seed):
    """x-only and y-only halves of `pool` snapped at `motion` (reference time first) -> (events, snapped, axis per snapped event)"""
    halves = np.array_split(np.asarray(pool), 2)
    snapped, axes = [], []
    for axis, part in enumerate(halves):
        ev, keep = snap_time(ev, motion, model, size, part, axis, seed=seed + axis)
        snapped.append(keep), axes.append(np.full(len(keep), axis))
    return ev, np.concatenate(snapped), np.concatenate(axes)


def _flips(ev, motion, model, size, idx, axes):
    c64, c32 = fp64_cells(ev, motion, model, size, "first"), fp32_cells(ev, motion, model, size, "first")
    return np.where(axes == 0, c64[0][idx] != c32[0][idx], c64[1][idx] != c32[1][idx])


def batch_case(model, K=3, n=4000, size=BASE, seed=60):
    """One batch, K motions, each with its OWN snapped third of the events -> dict(ev, motions [K, ...], snapped [K lists], n_flip [K])."""
    key = ("batch", model)
    if key in _BUILT:
        return _BUILT[key]
    ev = batch(n, size, seed)
    motions = _motions(model, size, K, seed)
    pool = np.random.default_rng(seed).permutation(np.arange(1, n - 1)) if model == TWO else one_per_pixel(ev, size, 0, n, seed)
    snapped, axes = [], []
    for k, part in enumerate(np.array_split(pool[: 3 * (len(pool) // 4)], K)):
        ev, keep, ax = _snap_set(ev, motions[k], model, size, part, seed + 7 * k)
        snapped.append(keep), axes.append(ax)
    n_flip = [int(_flips(ev, motions[k], model, size, snapped[k], axes[k]).sum()) for k in range(K)]  # (on the final batch)
    _BUILT[key] = dict(ev=ev, motions=motions, snapped=snapped, n_flip=n_flip, model=model, size=size)
    return _BUILT[key]


def state_case(model):
    """The all-snapped batch of motion A with exactly ONE further event snapped at motion B (one fp32 gets wrong)."""
    key = ("state", model)
    if key in _BUILT:
        return _BUILT[key]
    base = built("2dof-all" if model == TWO else "dense-all")
    ev, size, n = base["ev"], base["size"], base["n"]
    B = _motions(model, size, 2, 77)[1]
    free = np.setdiff1d(np.arange(1, n - 1), base["snapped"])
    if model != TWO:  # a pixel of its own
        ix, iy = _pixel(ev, size)
        pix = ix * size[1] + iy
        free = free[~np.isin(pix[free], pix[base["snapped"]])]
        _, first = np.unique(pix[free], return_index=True)
        free = free[first]
    ev2, keep = snap_time(ev, B, model, size, free[:64], 0, seed=78)
    flip = _flips(ev2, B, model, size, keep, np.zeros(len(keep), dtype=np.int64))
    one = keep[int(np.argmax(flip))]
    assert flip.any()
    out = ev.copy()
    out[one] = ev2[one]
    _BUILT[key] = dict(ev=out, A=base["motion"], B=B, one=int(one), snapped_A=base["snapped"], model=model, size=size)
    return _BUILT[key]
