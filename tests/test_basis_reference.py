"""The fp64 reference of the flow-basis plan (tests/_basis_ref.py) anchored to the references the project already trusts, and the
host-side properties of the feature: utils.flow_basis, the header and its ctypes mirror.  No GPU.

Anchors, at the 1e-10 the project anchors its references with:
  * the "translation" basis IS the "2d-translation" warp (x' = x + dt theta; B = -1): tests/_hvp_ref.objective(..., "2d-translation")
  * a basis made of the columns of tests/_patch_ref.patch_to_dense reproduces tests/_patch_ref.plan in loss, gradient and product
    (round32 False on both sides: the chains agree before any rounding)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import event_based_optical_flow_amd as E
from event_based_optical_flow_amd import _lib

import _basis_cases as B
import _basis_ref
import _hvp_ref
import _patch_cases as C
import _patch_ref

ANCHOR = 1e-10
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cmax_hip.h")


def rel_max(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


# ---- anchors -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(27, 40), (68, 90)], ids=["27x40", "68x90"])
@pytest.mark.parametrize("cost,sigma", [("image_variance", 0.0), ("multi_focal_normalized_gradient_magnitude", 1.0)], ids=["variance", "yaml"])
def test_translation_basis_is_the_two_dof_warp(size, cost, sigma):
    ev = C.batch(size)
    t_scale = float(ev[:, 2].max() - ev[:, 2].min())
    theta = np.array([4.0, -3.0]) / C.PERIOD
    evt = torch.as_tensor(ev)
    for round32 in (False, True):
        spec = dict(size=size, basis=E.utils.flow_basis("translation", size), t_scale=t_scale, terms=((cost, 1.0),), sigma=sigma, round32=round32)
        got = float(_basis_ref.loss(torch.as_tensor(theta), evt, spec))
        m = theta * t_scale
        m = C.f32(m) if round32 else m
        want = float(_hvp_ref.objective(evt, torch.as_tensor(m), "2d-translation", size, cost=cost, sigma=sigma))
        print(f"[basis-ref] translation {size} {cost} round32={round32}: {got!r} vs 2d-translation {want!r}, difference {abs(got - want):.1e}")
        assert abs(got - want) <= ANCHOR * abs(want)


@pytest.mark.parametrize("variant", ["dense", "burgers"])
def test_patch_columns_reproduce_the_patch_plan(variant):
    gid, size = "3x4-odd", (27, 40)
    g = C.GEOMETRY[gid]
    kw = dict(B.BURGERS) if variant == "burgers" else {}
    ev = C.batch(size)
    t_scale = float(ev[:, 2].max() - ev[:, 2].min())
    spec_p = C.spec_of(gid, size, terms=B.TWO_TERMS, tv_weight=0.0, t_scale=t_scale, **kw)
    spec_p["round32"] = False
    nx = 2 * g["patch_image_size"][0] * g["patch_image_size"][1]
    cols = np.stack([_patch_ref.patch_to_dense_numpy(np.eye(nx)[k].reshape((2,) + g["patch_image_size"]), size, g["sw"], g["pad"]) for k in range(nx)])
    spec_b = dict(size=size, basis=cols, t_scale=t_scale, terms=B.TWO_TERMS, sigma=spec_p["sigma"], omit=True, round32=False, time_aware=bool(kw),
                  T=spec_p["T"], scheme=spec_p["scheme"], t0=spec_p["t0"])
    x = C.patch_motion("random", g["patch_image_size"], 41)
    v = C.f32(np.random.default_rng(3).normal(size=nx))
    want = _patch_ref.plan(x, ev, spec_p, v=v)
    got = _basis_ref.plan(x, ev, spec_b, v=v)
    e = (abs(got[0] - want[0]) / abs(want[0]), rel_max(got[1], want[1]), rel_max(got[2], want[2]))
    print(f"[basis-ref] patch columns ({nx} fields) {variant}: rel diff loss {e[0]:.1e} grad {e[1]:.1e} Hv {e[2]:.1e}")
    assert np.abs(want[2]).max() > 0.0
    assert max(e) <= ANCHOR


# ---- the case table ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(B.HVP))
def test_the_border_filter_stays_under_the_cap(cid):
    ev, theta, spec, dropped = B.hvp_inputs(B.HVP[cid])
    print(f"[basis-ref] {cid}: {len(ev)} events kept, dropped share {dropped:.5f} (cap {B.DROP_CAP})")
    assert 0.0 <= dropped <= B.DROP_CAP
    if spec["time_aware"]:
        # the upwind selectors of the voxel chain take the sign of each flow component: no pixel may carry a rounding residue there
        D = _basis_ref.device_motion(theta, dict(spec, time_aware=False, round32=False))
        print(f"[basis-ref] {cid}: smallest |flow component| at a pixel {np.abs(D).min():.3e} px")
        assert np.abs(D).min() > 1e-6


def test_the_table_reaches_what_it_claims():
    n = [2 * h * w for h, w in B.LEAF_SIZES]
    assert all(v % 256 for v in n) and n[0] < B.ADJ_CHUNK < n[1] < 2 * B.ADJ_CHUNK and n[2] > 5 * B.ADJ_CHUNK
    assert B.ADJ_CHUNK == _lib.BASIS_ADJ_CHUNK and max(B.LEAF_K) == _lib.BASIS_MAX_K
    assert B.seam_elements(n[1]) == [0, 2047, 2048, 2159]
    for c in B.PLAN_CASES:
        ev, theta, spec = B.inputs(c)
        assert spec["basis"].shape[1:] == (2,) + c["size"] and theta.shape == (spec["basis"].shape[0],)
        if not c["id"].endswith("-zero"):
            bound = float((np.abs(theta) * np.abs(spec["basis"]).reshape(len(theta), -1).max(axis=1)).sum()) * spec["t_scale"]
            assert 1.0 < bound < 40.0, (c["id"], bound)  # a few pixels of displacement
    sb = B.smooth_basis(7, (20, 28), 1)
    assert np.array_equal(sb, sb.astype(np.float32).astype(np.float64)) and np.abs(sb).max() <= 1.0


def test_similarity_events_are_sharpest_near_the_field_that_made_them():
    """The premise of the GPU test that runs Newton-CG on these events: the similarity that generated them has a lower loss than its
    translation part alone."""
    ev = B.similarity_events()
    assert len(ev) > 2500 and np.all(np.diff(ev[:, 2]) >= 0)
    t_scale = float(ev[:, 2].max() - ev[:, 2].min())
    spec = dict(size=B.SIM_SIZE, basis=E.utils.flow_basis("similarity", B.SIM_SIZE), t_scale=t_scale, terms=B.ONE_TERM, sigma=1.0)
    true = np.array(B.SIM_TRUE) / B.PERIOD
    at_true = _basis_ref.plan(true, ev, spec)[0]
    at_translation = _basis_ref.plan(true * np.array([1.0, 1.0, 0.0, 0.0]), ev, spec)[0]
    at_zero = _basis_ref.plan(np.zeros(4), ev, spec)[0]
    print(f"[basis-ref] similarity events: loss {at_true:.6g} at the field, {at_translation:.6g} at its translation, {at_zero:.6g} at rest")
    assert at_true < min(at_translation, at_zero)


# ---- flow_basis ----------------------------------------------------------------------------------------------------------------------
def test_flow_basis_shapes_and_signs():
    size = (5, 8)
    H, W = size
    r = np.arange(H)[:, None] - (H - 1) / 2.0 + np.zeros((H, W))
    c = np.arange(W)[None, :] - (W - 1) / 2.0 + np.zeros((H, W))
    for model, K in (("translation", 2), ("similarity", 4), ("affine", 6)):
        Bm = E.utils.flow_basis(model, size)
        assert Bm.shape == (K, 2, H, W) and Bm.dtype == np.float64 and Bm.flags["C_CONTIGUOUS"]
        # theta of the translation part is the theta of "2d-translation": x' = x + dt theta = x - dt D, hence B = -1
        assert np.array_equal(Bm[0], np.stack([-np.ones(size), np.zeros(size)])) and np.array_equal(Bm[1], np.stack([np.zeros(size), -np.ones(size)]))
    S, A = E.utils.flow_basis("similarity", size), E.utils.flow_basis("affine", size)
    assert np.array_equal(S[2], np.stack([-r, -c])) and np.array_equal(S[3], np.stack([c, -r]))  # zoom, rotation
    assert np.array_equal(S[2], A[2] + A[5]) and np.array_equal(S[3], A[4] - A[3])              # a similarity is an affine map
    assert np.array_equal(A[2], np.stack([-r, 0 * r])) and np.array_equal(A[3], np.stack([-c, 0 * c]))
    # rotation about the optical axis of a camera whose principal point is the sensor's centre, unit focal lengths in pixels: the in-plane rotation
    R = E.utils.flow_basis("rotation", size, calib=(1.0, 1.0, (W - 1) / 2.0, (H - 1) / 2.0))
    assert R.shape == (3, 2, H, W)
    np.testing.assert_allclose(R[2], S[3], atol=1e-15)
    f = 50.0
    Rf = E.utils.flow_basis("rotation", size, calib=(f, f, (W - 1) / 2.0, (H - 1) / 2.0))
    i0, j0 = (H - 1) // 2, (W - 1) // 2  # next to the principal point a pan / tilt is a translation by the focal length
    assert abs(-Rf[0, 0, i0, j0] - f) < 0.5 and abs(-Rf[1, 1, i0, j0] + f) < 0.5
    with pytest.raises(ValueError, match="calib"):
        E.utils.flow_basis("rotation", size)
    with pytest.raises(ValueError, match="homography"):
        E.utils.flow_basis("homography", size)


# ---- header and binding --------------------------------------------------------------------------------------------------------------
def test_header_declares_the_new_entries():
    text = open(HEADER).read()
    for name in ("cmax_basis_to_dense", "cmax_sizeof_basis_objective", "cmax_basis_plan_create"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _lib.SIGNATURES
    assert re.search(r"#define\s+CMAX_ABI_VERSION\s+4\b", text) and _lib.ABI_VERSION == 4
    assert int(re.search(r"#define\s+CMAX_BASIS_MAX_K\s+(\d+)", text).group(1)) == _lib.BASIS_MAX_K == 64
    assert int(re.search(r"#define\s+CMAX_BASIS_ADJ_CHUNK\s+(\d+)", text).group(1)) == _lib.BASIS_ADJ_CHUNK
    # argument counts of the prototypes
    for name in ("cmax_basis_to_dense", "cmax_basis_plan_create"):
        args = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[name][1]), name


def test_descriptor_mirror_matches_the_header():
    text = open(HEADER).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*cmax_basis_objective_t;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names, size = [], 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, rest = decl.split(None, 1)
        for field in rest.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", field)
            names.append(m.group(1))
            count = int(m.group(2)) if m.group(2) else 1
            width = {"int32_t": 4, "double": 8, "cmax_objective_t": ctypes.sizeof(_lib.CmaxObjective)}[ctype]
            size = (size + min(width, 8) - 1) // min(width, 8) * min(width, 8) + width * count
    assert names == [n for n, _ in _lib.CmaxBasisObjective._fields_]
    assert size == ctypes.sizeof(_lib.CmaxBasisObjective) and size % 8 == 0
    assert _lib.CmaxBasisObjective.t_scale.offset == 40 and _lib.CmaxBasisObjective.K.offset == 28
