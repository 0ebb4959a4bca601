"""The solver side -- patch grid -> dense flow and its gather-form adjoint (csrc/cmax_patch_kernels.h), the native patch plan and its
tail kernel's own total variation (cmax_patch_plan_evaluate / _hvp, k_patch_tail of csrc/cmax_solver.hip) and the per-patch translation
search (csrc/cmax_search_kernels.h) -- against the fp64 references of tests/_patch_ref.py and tests/_search_ref.py, on the geometry
table of tests/_patch_cases.py: every pad, odd and overlapping sliding windows, one-row and one-column grids, odd up-sampled extents, a
sensor as large as the grid, both sides of the tail's LDS / global split and of its crop switch, blur radii beyond the patch image,
one-pixel axes, the largest image the LDS admits, coarse-keyed and slab-ordered handles, the fixed point at its capacity.

Gates, all of them the project's own: the leaf operator's 1e-12 / 1e-11 (fp64) and 1e-5 / 1e-4 (fp32) of the largest entry
(test_patch_to_dense_golden); 1e-4 for the plan's loss and gradient and HVP_TOL = 1e-4 for its product (tests/test_gpu_solver.py); the
tail's TV term alone, isolated as loss(with_tv) - loss(without) on a bit-repeatable handle, at 1e-9 of ITS OWN magnitude, or where the
subtraction cannot resolve that, at the subtraction's own rounding eps64 (|contrast part| + |TV part|); the search's count exactly and
gm at 1e-4 of the largest entry of its own patch row.  The tests print what they measure; tools/probe_patch_side.py collects the worst
figures into profiles/patch_side_parity.txt."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import event_based_optical_flow_amd as E  # noqa: E402
from event_based_optical_flow_amd import functional as F  # noqa: E402
from event_based_optical_flow_amd.solver import PatchFlowObjective  # noqa: E402

import _patch_cases as C  # noqa: E402
import _patch_ref  # noqa: E402

TOL = 1e-4
HVP_TOL = 1e-4
LEAF_TOL = {torch.float64: (1e-12, 1e-11), torch.float32: (1e-5, 1e-4)}
TV_TOL = 1e-9
EPS64 = float(np.finfo(np.float64).eps)


def rel_max(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


# ---- 1. the leaf operator ----------------------------------------------------------------------------------------------------------
def measure_leaf(gid, size, dtype):
    """-> (forward error, adjoint error with a random cotangent, worst adjoint error over the one-hot cotangents), each of the largest
    entry of its reference."""
    g = C.GEOMETRY[gid]
    m_np, cot_np = C.leaf_inputs(gid, size)
    m = torch.tensor(m_np, dtype=dtype, device="cuda", requires_grad=True)
    dense = F.patch_to_dense(m, size, g["sw"], g["pad"])
    assert tuple(dense.shape) == (2,) + tuple(size) and dense.dtype == dtype
    e_fwd = rel_max(dense.detach().cpu().numpy(), _patch_ref.patch_to_dense_numpy(m_np, size, g["sw"], g["pad"]))
    (gm,) = torch.autograd.grad(dense, m, grad_outputs=torch.tensor(cot_np, dtype=dtype, device="cuda"), retain_graph=True)
    e_adj = rel_max(gm.cpu().numpy(), _patch_ref.patch_to_dense_adj_numpy(cot_np, g["patch_image_size"], size, g["sw"], g["pad"]))
    e_hot = 0.0
    for c, (i, j) in enumerate(C.band_pixels(gid, size)):
        hot = np.zeros((2,) + tuple(size))
        hot[c % 2, i, j] = 1.0
        (gh,) = torch.autograd.grad(dense, m, grad_outputs=torch.tensor(hot, dtype=dtype, device="cuda"), retain_graph=True)
        ref = _patch_ref.patch_to_dense_adj_numpy(hot, g["patch_image_size"], size, g["sw"], g["pad"])
        assert abs(ref.sum() + 1.0) <= 1e-12  # the taps of one pixel sum to one (and the operator negates)
        e_hot = max(e_hot, rel_max(gh.cpu().numpy(), ref))
    return e_fwd, e_adj, e_hot


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("gid,size", C.LEAF_CASES, ids=[f"{g}-{s[0]}x{s[1]}" for g, s in C.LEAF_CASES])
def test_patch_to_dense_and_adjoint(gid, size, dtype):
    e_fwd, e_adj, e_hot = measure_leaf(gid, size, dtype)
    print(f"[patch side] leaf {gid} {size} {dtype}: forward {e_fwd:.2e} adjoint {e_adj:.2e} one-hot adjoints {e_hot:.2e}")
    tol_fwd, tol_adj = LEAF_TOL[dtype]
    assert e_fwd <= tol_fwd and e_adj <= tol_adj and e_hot <= tol_adj, (gid, size, e_fwd, e_adj, e_hot)


# ---- 2. the native plan: value and gradient ------------------------------------------------------------------------------------------
def make_objective(ev, spec, deterministic=False):
    h = E.CMaxHandle(spec["size"])
    if deterministic:
        h.set_deterministic(True)
    h.set_events(ev, time_bin=spec["T"] if spec["time_aware"] else 0)
    assert h.n_events == len(ev)
    names = {name: w for name, w in spec["terms"]}
    if spec["tv_weight"]:
        names["total_variation"] = spec["tv_weight"]
    hybrid = len(names) > 1
    # patch_size == sliding_window and a shift of (pad - 1) windows give the table's pad through patch_pad
    shift = tuple(max(spec["pad"][k] - 1, 0) * spec["sw"][k] for k in (0, 1))
    obj = PatchFlowObjective(h, spec["t_scale"], spec["patch_image_size"], spec["sw"], spec["sw"], shift,
                             cost="hybrid" if hybrid else next(iter(names)), cost_with_weight=names if hybrid else None, blur_sigma=spec["sigma"],
                             time_aware=spec["time_aware"], time_bin=spec["T"], flow_interpolation=spec["scheme"], t0_flow_location=spec["t0"],
                             scale_later=spec["scale_later"], omit_boundary=spec["omit"])
    if obj.pad != tuple(spec["pad"]):  # pad 0 on an axis: below what patch_pad ever returns, but a geometry the library takes
        assert min(spec["pad"]) == 0
        obj.pad = tuple(spec["pad"])
        obj.__del__()  # destroys the plan made with patch_pad's value
        obj._build_native_plan()
    assert obj.has_native_plan and obj.pad == tuple(spec["pad"])
    return h, obj


def measure_plan(c):
    b = C.built_plan(c)
    h, obj = make_objective(b["ev"], b["spec"])
    loss, grad = obj.value_and_grad_numpy(b["x"])
    e_loss = abs(loss - b["loss"]) / abs(b["loss"])
    e_grad = rel_max(grad, b["grad"])
    return h, obj, b, loss, grad, e_loss, e_grad


@pytest.mark.parametrize("cid", [c["id"] for c in C.PLAN_CASES])
def test_plan_value_and_gradient(cid):
    h, obj, b, loss, grad, e_loss, e_grad = measure_plan(C.PLAN[cid])
    loss_s, grad_s = obj.value_and_grad_numpy(b["x"], with_tv=False)
    e_loss_s, e_grad_s = abs(loss_s - b["loss_smooth"]) / abs(b["loss_smooth"]), rel_max(grad_s, b["grad_smooth"])
    print(f"[patch side] plan {cid}: {len(b['ev'])} events, rel err loss {e_loss:.2e} grad {e_grad:.2e}; without TV loss {e_loss_s:.2e} grad {e_grad_s:.2e}")
    assert e_loss <= TOL and e_grad <= TOL, (cid, e_loss, e_grad)
    assert e_loss_s <= TOL and e_grad_s <= TOL, (cid, e_loss_s, e_grad_s)
    for _ in range(3):  # value only, three evaluations on one plan (the handle's vote buffers flip)
        loss_v, none = obj.value_and_grad_numpy(b["x"], want_grad=False)
        assert none is None and abs(loss_v - b["loss"]) <= TOL * abs(b["loss"])
    del obj
    h.close()


@pytest.mark.parametrize("cid", ["odd-dense", "overlap-burgers-first-T5", "46x45-dense"])
def test_plan_follows_set_t_scale(cid):
    """Another duration behind the same plan: the reference at that t_scale, and back."""
    c = C.PLAN[cid]
    b = C.built_plan(c)
    h, obj = make_objective(b["ev"], b["spec"])
    spec2 = dict(b["spec"], t_scale=0.6 * b["spec"]["t_scale"])
    loss_ref, grad_ref, _ = _patch_ref.plan(b["x"], b["ev"], spec2)
    obj.set_t_scale(spec2["t_scale"])
    loss, grad = obj.value_and_grad_numpy(b["x"])
    e_loss, e_grad = abs(loss - loss_ref) / abs(loss_ref), rel_max(grad, grad_ref)
    print(f"[patch side] plan {cid} after set_t_scale: rel err loss {e_loss:.2e} grad {e_grad:.2e}")
    assert e_loss <= TOL and e_grad <= TOL
    assert abs(loss_ref - b["loss"]) > 1e-3 * abs(b["loss"])  # it is another objective
    obj.set_t_scale(b["spec"]["t_scale"])
    loss, grad = obj.value_and_grad_numpy(b["x"])
    assert abs(loss - b["loss"]) <= TOL * abs(b["loss"]) and rel_max(grad, b["grad"]) <= TOL
    del obj
    h.close()


# ---- 3. the tail's total variation on its own ----------------------------------------------------------------------------------------
_TV_BATCH = {}


def measure_tail_tv(pis, omit):
    """One deterministic handle and plan per grid; per motion -> (kind, error of the TV value, its bound, error of the TV gradient, its
    bound), errors and bounds absolute."""
    g = C.tv_geometry(pis)
    if g["size"] not in _TV_BATCH:
        _TV_BATCH[g["size"]] = C.batch(g["size"], n=2000, seed=5)
    ev = _TV_BATCH[g["size"]]
    spec = dict(size=g["size"], patch_image_size=g["patch_image_size"], sw=g["sw"], pad=g["pad"], t_scale=C.PERIOD, terms=C.YAML_HYBRID,
                sigma=1.0, tv_weight=C.YAML_TV, omit=omit, time_aware=False, T=0, scheme="burgers", t0="middle", scale_later=False)
    h, obj = make_objective(ev, spec, deterministic=True)
    rows = []
    for kind in C.TV_MOTIONS:
        x = C.patch_motion(kind, pis, 40)
        with_tv, without = obj.value_and_grad_numpy(x), obj.value_and_grad_numpy(x, with_tv=False)
        again = obj.value_and_grad_numpy(x, with_tv=False)
        assert without[0] == again[0] and without[1].tobytes() == again[1].tobytes()  # bit-repeatable: the difference is the TV term
        tv, dtv = _patch_ref.total_variation_numpy(x.reshape((2,) + tuple(pis)), omit)
        tv, dtv = C.YAML_TV * tv, C.YAML_TV * dtv.reshape(-1)
        e_tv = abs((with_tv[0] - without[0]) - tv)
        e_dtv = np.abs((with_tv[1] - without[1]) - dtv).max()
        bound_tv = max(TV_TOL * abs(tv), EPS64 * (abs(without[0]) + abs(tv)))
        bound_dtv = max(TV_TOL * np.abs(dtv).max(), EPS64 * (np.abs(without[1]).max() + np.abs(dtv).max()))
        rows.append((kind, e_tv, bound_tv, abs(tv), e_dtv, bound_dtv, float(np.abs(dtv).max())))
    del obj
    h.close()
    return rows


@pytest.mark.parametrize("omit", [True, False], ids=["omit", "whole"])
@pytest.mark.parametrize("pis", C.TV_GRIDS, ids=[f"{a}x{b}" for a, b in C.TV_GRIDS])
def test_tail_total_variation_alone(pis, omit):
    for kind, e_tv, bound_tv, tv, e_dtv, bound_dtv, dtv in measure_tail_tv(pis, omit):
        print(f"[patch side] tail TV {pis} omit {omit} {kind}: |w TV| {tv:.3e} abs err {e_tv:.2e} (bound {bound_tv:.2e}); "
              f"|w dTV| {dtv:.3e} abs err {e_dtv:.2e} (bound {bound_dtv:.2e})")
        assert e_tv <= bound_tv, (pis, omit, kind, e_tv, bound_tv)
        assert e_dtv <= bound_dtv, (pis, omit, kind, e_dtv, bound_dtv)


# ---- 4. the plan's Hessian-vector product --------------------------------------------------------------------------------------------
def measure_hvp(c):
    b = C.built_hvp(c)
    h, obj = make_objective(b["ev"], b["spec"])
    loss, grad = obj.value_and_grad_numpy(b["x"])
    out = {"loss": abs(loss - b["loss"]) / abs(b["loss"]), "grad": rel_max(grad, b["grad"])}
    for name in ("random", "one-hot"):
        out[name] = rel_max(obj.hvp_numpy(b["x"], b["v"][name]), b["hv"][name])
    zero = obj.hvp_numpy(b["x"], b["v"]["zero"])
    assert zero.shape == b["x"].shape and not zero.any() and not b["hv"]["zero"].any()
    del obj
    h.close()
    return b, out


@pytest.mark.parametrize("cid", [c["id"] for c in C.HVP_CASES])
def test_plan_hvp(cid):
    b, e = measure_hvp(C.HVP[cid])
    print(f"[patch side] hvp {cid}: {len(b['ev'])} events, dropped {b['dropped']:.5f}, rel err loss {e['loss']:.2e} grad {e['grad']:.2e} "
          f"Hv random {e['random']:.2e} one-hot {e['one-hot']:.2e}")
    assert b["dropped"] <= C.DROP_CAP
    assert e["loss"] <= TOL and e["grad"] <= TOL, (cid, e)
    assert e["random"] <= HVP_TOL and e["one-hot"] <= HVP_TOL, (cid, e)


# ---- 5. the per-patch search ---------------------------------------------------------------------------------------------------------
def search_handle(hd):
    h = E.CMaxHandle(C.SEARCH_SENSOR).set_events(C.search_events(hd["frac"]), time_bin=hd["T"])
    if hd["slabs"]:
        h.set_time_slabs(hd["slabs"])
        assert h.time_slabs == hd["slabs"]
    return h


def compare_search(got, ref):
    """-> worst error of gm relative to the largest entry of its own patch row, after the exact checks."""
    (loss, gm, count), (loss_r, gm_r, count_r) = got, ref
    loss, gm, count = loss.cpu().numpy(), gm.double().cpu().numpy(), count.cpu().numpy()
    np.testing.assert_array_equal(count, count_r)
    assert (gm[count_r == 0] == 0).all()
    assert (gm[gm_r == 0] == 0).all()  # swept out, a zero span, an empty box: no vote in the image, exactly
    scale = np.maximum(np.abs(gm_r).max(axis=1, keepdims=True), 1e-300)
    e_gm = float((np.abs(gm - gm_r) / scale).max())
    assert np.array_equal(np.isnan(loss), np.isnan(loss_r)) and np.array_equal(np.isinf(loss), np.isinf(loss_r))
    ok = np.isfinite(loss_r)  # the reference's denominator is non-zero
    assert (loss[ok & (loss_r == 0)] == 0).all()
    ok &= loss_r != 0
    e_loss = float((np.abs(loss[ok] - loss_r[ok]) / np.abs(loss_r[ok])).max(initial=0.0))
    return e_gm, e_loss


def measure_search(hd):
    h = search_handle(hd)
    rows = []
    for image in C.SEARCH_IMAGES:
        for sigma in C.SEARCH_SIGMAS:
            got = h.patch_search(C.SEARCH_BOXES, image, C.search_candidates(), sigma)
            rows.append((image, sigma) + compare_search(got, C.built_search(hd["frac"], image, sigma)))
    h.close()
    return rows


@pytest.mark.parametrize("hid", [hd["id"] for hd in C.SEARCH_HANDLES])
def test_patch_search(hid):
    hd = next(hd for hd in C.SEARCH_HANDLES if hd["id"] == hid)
    rows = measure_search(hd)
    for image, sigma, e_gm, e_loss in rows:
        print(f"[patch side] search {hid} image {image} sigma {sigma}: gm {e_gm:.2e} of its row's largest, loss {e_loss:.2e}")
    for image, sigma, e_gm, e_loss in rows:
        assert e_gm <= TOL, (hid, image, sigma, e_gm)
        assert e_loss <= TOL, (hid, image, sigma, e_loss)


def measure_capacity():
    ev = C.capacity_events()
    h = E.CMaxHandle((16, 16)).set_events(ev)
    box, image = np.array([[0, 16, 0, 16]]), (16, 16)
    loss, gm, count = h.patch_search(box, image, np.zeros((1, 1, 2)), 0.0)
    h.close()
    import _search_ref
    _, gm_r, count_r = _search_ref.patch_search(ev, box, image, np.zeros((1, 1, 2)), 0.0)
    return gm.double().cpu().numpy(), count.cpu().numpy(), gm_r, count_r


def test_patch_search_at_the_capacity_of_the_fixed_point():
    """8191 events on one pixel, zero candidate, no blur: every vote is 2^18 exactly and the cell holds 8191 * 2^18 < 2^31.  The image is
    exact; gm is a sum of fp32 squares of exact Sobel responses (8191^2 k^2 / 64 needs more than 24 bits): two squares and one sum round
    per pixel, the block sum is fp64, one rounding to fp32 at the end -- 4 x 2^-24."""
    gm, count, gm_r, count_r = measure_capacity()
    np.testing.assert_array_equal(count, count_r)
    assert count[0] == 8191
    e = np.abs(gm / gm_r - 1.0).max()
    print(f"[patch side] search at 8191 votes on one cell: gm {gm[0]} reference {gm_r[0]} rel err {e:.2e}")
    assert e <= 4 * 2.0**-24 and gm[0, 0] == gm[0, 1]
