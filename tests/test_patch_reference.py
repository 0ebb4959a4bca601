"""CPU: the fp64 references of the solver side (tests/_patch_ref.py, tests/_search_ref.py) against the C oracle and the committed
fixtures of the reference, so that the two restatements pin each other, and the claims of the case table (tests/_patch_cases.py) that
tests/test_gpu_patch_side.py relies on.  No GPU."""
import numpy as np
import pytest

from oracle import oracle as orc

import _patch_cases as C
import _patch_ref
import _search_ref

YAML_TERMS = (("multi_focal_normalized_gradient_magnitude", 1.0),)


def rel_max(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


# ---- interpolation and adjoint ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gid,size", C.LEAF_CASES, ids=[f"{g}-{s[0]}x{s[1]}" for g, s in C.LEAF_CASES])
def test_patch_to_dense_against_the_oracle(gid, size):
    g = C.GEOMETRY[gid]
    m, cot = C.leaf_inputs(gid, size)
    dense = _patch_ref.patch_to_dense_numpy(m, size, g["sw"], g["pad"])
    adj = _patch_ref.patch_to_dense_adj_numpy(cot, g["patch_image_size"], size, g["sw"], g["pad"])
    assert rel_max(dense, orc.patch_to_dense(m, size, g["sw"], g["pad"])) <= 1e-12
    assert rel_max(adj, orc.patch_to_dense_adj(cot, g["patch_image_size"], g["sw"], g["pad"])) <= 1e-12
    # <P m, cot> == <m, P^T cot>
    assert abs((dense * cot).sum() - (m * adj).sum()) <= 1e-12 * np.abs(dense * cot).sum()


def test_every_geometry_covers_its_sensor():
    for g in C.GEOMETRIES:
        for H, W in g["sizes"]:
            assert (g["patch_image_size"][0] + 2 * g["pad"][0]) * g["sw"][0] >= H, g["id"]
            assert (g["patch_image_size"][1] + 2 * g["pad"][1]) * g["sw"][1] >= W, g["id"]
    for c in C.PLAN_CASES + C.HVP_CASES:
        assert c["size"] in C.GEOMETRY[c["gid"]]["sizes"], c["id"]
    for pis in C.TV_GRIDS:
        g = C.tv_geometry(pis)
        assert all((g["patch_image_size"][k] + 2) * g["sw"][k] >= g["size"][k] for k in (0, 1))


def test_the_table_reaches_what_it_claims():
    ids = {g["id"]: g for g in C.GEOMETRIES}
    assert ids["1x1-pad0"]["pad"] == (0, 0) and ids["3x4-exact"]["pad"] == (0, 0) and ids["3x4-odd"]["pad"] == (3, 2)
    g = ids["3x4-exact"]
    assert [(g["patch_image_size"][k] + 2 * g["pad"][k]) * g["sw"][k] for k in (0, 1)] == list(g["sizes"][0])  # sensor == up-sampled grid
    g = ids["3x4-odd"]
    assert ((g["patch_image_size"][0] + 2 * g["pad"][0]) * g["sw"][0]) % 2 == 1 and g["sw"][0] % 2 == 1 and g["sw"][1] % 2 == 1
    assert {s[0] % 2 for s in g["sizes"]} == {0, 1}
    # the tail's LDS / global split
    lds, glob = ids["45x45"]["patch_image_size"], ids["46x45"]["patch_image_size"]
    assert 2 * lds[0] * lds[1] <= C.TAIL_LDS < 2 * glob[0] * glob[1]
    assert (45, 45) in C.TV_GRIDS and (46, 45) in C.TV_GRIDS
    # crop on both sides of tv_crop = omit and ph > 2 and pw > 2
    assert (3, 2) in C.TV_GRIDS and (3, 3) in C.TV_GRIDS and (2, 7) in C.TV_GRIDS
    # the search's largest image
    h, w = C.SEARCH_IMAGES[-1]
    assert 2 * h * w * 4 <= C.SEARCH_LDS < 2 * h * (w + 1) * 4 and 2 * (h + 1) * w * 4 > C.SEARCH_LDS and (h, w) == C.SEARCH_SENSOR
    assert max(int(4.0 * s + 0.5) for s in C.SEARCH_SIGMAS) > 10
    assert {hd["T"] for hd in C.SEARCH_HANDLES} == {0, 10, 40} and 10 * 256 <= 8192 < 40 * 256  # kTileKeysMax: fine and coarse keys
    assert len(C.capacity_events()) * 2**18 < 2**31 <= (len(C.capacity_events()) + 1) * 2**18


# ---- total variation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["4x4", "8x8", "2x2", "1x1"])
@pytest.mark.parametrize("omit", [1, 0])
def test_total_variation_against_the_fixtures(golden, shape, omit):
    g = golden("costs")
    tag = f"tv_{shape}_omit{omit}"
    tv, grad = _patch_ref.total_variation_numpy(g[tag + "__flow"], bool(omit))
    assert abs(tv - float(g[tag + "__loss"])) <= 1e-12 * abs(float(g[tag + "__loss"]))
    assert np.abs(grad - g[tag + "__g"]).max() <= 1e-12 * max(np.abs(g[tag + "__g"]).max(), 1e-300)


@pytest.mark.parametrize("pis", C.TV_GRIDS, ids=[f"{a}x{b}" for a, b in C.TV_GRIDS])
@pytest.mark.parametrize("omit", [True, False])
def test_total_variation_against_the_oracle(pis, omit):
    for kind in C.TV_MOTIONS:
        x = C.patch_motion(kind, pis, 40).reshape((2,) + tuple(pis))
        tv, grad = _patch_ref.total_variation_numpy(x, omit)
        tv_o, grad_o = orc.total_variation(x, omit)
        assert abs(tv - tv_o) <= 1e-12 * max(abs(tv_o), 1e-300), (kind, tv, tv_o)
        assert np.abs(grad - grad_o).max() <= 1e-12 * max(np.abs(grad_o).max(), 1e-300), kind
        if kind == "zero":
            assert tv == 0.0 and not grad.any()  # the sub-gradient of |.| at 0 is 0


# ---- the whole plan --------------------------------------------------------------------------------------------------------------------
def _fixture_spec(g, k, tag, ev, size, **extra):
    pis, ps, sw = (tuple(int(v) for v in g[k + "__" + n]) for n in ("patch_image_size", "patch_size", "sliding_window"))
    shift = tuple(int(v) for v in (g[k + "__patch_shift"] if k + "__patch_shift" in g else g[tag + "__patch_shift"]))
    spec = dict(size=size, patch_image_size=pis, sw=sw, pad=_patch_ref.patch_pad(ps, sw, shift), t_scale=float(ev[:, 2].max() - ev[:, 2].min()),
                terms=YAML_TERMS, sigma=1.0, tv_weight=0.01, tv_omit=True, omit=True, round32=False)  # round32 False: the reference's fp64 chain
    spec.update(extra)
    return spec


@pytest.mark.parametrize("tag", ["plain", "burgers"])
@pytest.mark.parametrize("scale", [1, 3])
def test_plan_against_the_solver_fixture(golden, tag, scale):
    g = golden("solver_objective")
    k = f"{tag}_s{scale}"
    size, ev = tuple(int(v) for v in g["image_size"]), g["events"]
    spec = _fixture_spec(g, k, tag, ev, size, time_aware=(tag == "burgers"), T=10, scheme="burgers", t0="middle")
    loss, grad, _ = _patch_ref.plan(g[k + "__x"], ev, spec)
    assert abs(loss - float(g[k + "__loss"])) <= 1e-9 * abs(float(g[k + "__loss"]))
    assert rel_max(grad, np.asarray(g[k + "__grad"]).reshape(-1)) <= 1e-9


@pytest.mark.parametrize("case", ["burgers_s3", "upwind_s1", "burgers_first_s1", "negative_s3"])
def test_plan_against_the_scale_later_fixture(golden, case):
    g, gs = golden("solver_objective"), golden("solver_scale_later")
    size, ev = tuple(int(v) for v in g["image_size"]), g["events"]
    spec = _fixture_spec(gs, case, None, ev, size, time_aware=True, T=10, scheme=str(gs[case + "__flow_interpolation"]),
                         t0=str(gs[case + "__t0_flow_location"]), scale_later=True)
    loss, grad, hv = _patch_ref.plan(gs[case + "__x"], ev, spec, v=gs[case + "__v"])
    assert abs(loss - float(gs[case + "__loss"])) <= 1e-9 * abs(float(gs[case + "__loss"]))
    assert rel_max(grad, np.asarray(gs[case + "__grad"]).reshape(-1)) <= 1e-9
    assert rel_max(hv, np.asarray(gs[case + "__vhp"]).reshape(-1)) <= 1e-9


@pytest.mark.parametrize("cid", [c["id"] for c in C.HVP_CASES])
def test_share_of_border_ambiguous_events(cid):
    """The Hessian-vector cases remove the events within fp32 rounding of a cell border at the motion the device holds: at most 0.5 %."""
    ev, x, spec, dropped = C.hvp_inputs(C.HVP[cid])
    print(f"[patch reference] {cid}: {len(ev)} events kept, share dropped {dropped:.5f}")
    assert dropped <= C.DROP_CAP, (cid, dropped)


# ---- per-patch search ------------------------------------------------------------------------------------------------------------------
def _rows_close(got, ref, tol):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape
    scale = np.maximum(np.abs(ref).max(axis=1, keepdims=True), 1e-300)
    return (np.abs(got - ref) / scale).max() <= tol


@pytest.mark.parametrize("scale", [2, 3])
def test_search_against_the_fixture(golden, scale):
    g = golden("patch_search")
    k = f"s{scale}"
    loss, gm, count = _search_ref.patch_search(g["events"], g[k + "__boxes"], tuple(g[k + "__patch_size"]), g[k + "__cand"], float(g["sigma"]))
    np.testing.assert_array_equal(count, g[k + "__count"])
    assert np.abs(loss / g[k + "__loss"] - 1.0).max() <= 1e-9


@pytest.mark.parametrize("frac", [False, True], ids=["int", "frac"])
@pytest.mark.parametrize("image", C.SEARCH_IMAGES, ids=[f"{a}x{b}" for a, b in C.SEARCH_IMAGES])
def test_search_against_the_oracle(image, frac):
    ev = C.search_events(frac)
    for sigma in C.SEARCH_SIGMAS:
        loss, gm, count = C.built_search(frac, image, sigma)
        loss_o, gm_o, count_o = orc.patch_search(ev, C.SEARCH_BOXES, image, C.search_candidates(), sigma)
        np.testing.assert_array_equal(count, count_o)
        assert _rows_close(gm, gm_o, 1e-9), (image, sigma)
        assert np.array_equal(np.isnan(loss), np.isnan(loss_o)) and np.array_equal(np.isinf(loss), np.isinf(loss_o))
        ok = np.isfinite(loss_o)
        assert (np.abs(loss[ok] - loss_o[ok]) <= 1e-9 * np.abs(loss_o[ok])).all()


def test_the_search_table_reaches_what_it_claims():
    for frac in (False, True):
        ev = C.search_events(frac)
        count = C.built_search(frac, (8, 10), 0.0)[2]
        assert count[4] == 0 and count[7] == 0 and count[8] == 1 and count[6] >= 1 and count[5] == len(ev)
        inside = C._in_box(ev, C.SEARCH_BOXES[9])
        assert inside.sum() > 1 and np.ptp(ev[inside, 2]) == 0.0  # one timestamp
        gm = C.built_search(frac, (8, 10), 1.0)[1]
        assert (gm[:, 3] == 0).all()  # the sweeping candidate leaves no vote in any image
        assert (gm[9, :3] == 0).all() and gm[9, -1] > 0  # a zero span: the warped images stay empty, the un-warped one does not
        assert (gm[count == 0] == 0).all()
    # integer sources + fractional sources differ, so both are real cases
    assert not np.array_equal(C.search_events(False)[:, :2], C.search_events(True)[:, :2])
