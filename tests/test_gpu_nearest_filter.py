"""The nearest patch filter (`patch.filter_type: "nearest"`, src/solver/patch_contrast_base.py:492-495) from the kernel up: the leaf
operator cmax_patch_to_dense_filter and its gather-form adjoint (csrc/cmax_patch_kernels.h), and the native patch plan built with
cmax_patch_objective_t::filter_type (csrc/cmax_solver.hip) -- evaluate, product, exact_flow, scale_later, graph replay -- against the
fp64 restatement tests/_mixed_ref.py, which tests/test_mixed_reference.py holds to the reference's own numbers.

Gates: the forward is a negated copy, so it is BIT-EQUAL to the indexed copy in both dtypes; the adjoint at the gates
tests/test_gpu_patch_side.py applies to the bilinear adjoint (1e-11 fp64, 1e-4 fp32 of the largest entry), one-hot cotangents on either
side of every cell border included, and bit-identical from run to run; the plan's loss, gradient and product at the project's plain 1e-4
of the largest entry.  The tests print what they measure."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from event_based_optical_flow_amd import _lib  # noqa: E402
from event_based_optical_flow_amd import functional as F  # noqa: E402

import _mixed_ref  # noqa: E402
import _nearest_cases as N  # noqa: E402
import _patch_cases as C  # noqa: E402
import _patch_ref  # noqa: E402

TOL = 1e-4
HVP_TOL = 1e-4
ADJ_TOL = {torch.float64: 1e-11, torch.float32: 1e-4}  # LEAF_TOL of tests/test_gpu_patch_side.py, the adjoint's entry
HERE = os.path.dirname(os.path.abspath(__file__))


def rel_max(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


# ---- 1. the leaf operator ----------------------------------------------------------------------------------------------------------
def leaf_inputs(gid, size):
    g = N.GEOMETRY[gid]
    rng = np.random.default_rng(2000 + 17 * size[0] + size[1] + len(gid))
    return C.f32(rng.normal(0, 30.0, (2,) + g["patch_image_size"])), C.f32(rng.normal(size=(2,) + tuple(size)))


def measure_leaf(gid, size, dtype):
    g = N.GEOMETRY[gid]
    m_np, cot_np = leaf_inputs(gid, size)
    args = (size, g["sw"], g["pad"], "nearest")
    m = torch.tensor(m_np, dtype=dtype, device="cuda", requires_grad=True)
    dense = F.patch_to_dense(m, *args)
    assert tuple(dense.shape) == (2,) + tuple(size) and dense.dtype == dtype
    fwd_equal = np.array_equal(dense.detach().cpu().numpy().astype(np.float64), _mixed_ref.patch_to_dense_numpy(m_np, *args))
    cot = torch.tensor(cot_np, dtype=dtype, device="cuda")
    (gm,) = torch.autograd.grad(dense, m, grad_outputs=cot, retain_graph=True)
    (gm2,) = torch.autograd.grad(dense, m, grad_outputs=cot, retain_graph=True)
    repeatable = gm.cpu().numpy().tobytes() == gm2.cpu().numpy().tobytes()
    e_adj = rel_max(gm.cpu().numpy(), _mixed_ref.patch_to_dense_adj_numpy(cot_np, g["patch_image_size"], *args))
    e_hot = 0.0
    for c, (i, j) in enumerate(N.border_pixels(gid, size)):
        hot = np.zeros((2,) + tuple(size))
        hot[c % 2, i, j] = 1.0
        (gh,) = torch.autograd.grad(dense, m, grad_outputs=torch.tensor(hot, dtype=dtype, device="cuda"), retain_graph=True)
        ref = _mixed_ref.patch_to_dense_adj_numpy(hot, g["patch_image_size"], *args)
        assert ref.sum() == -1.0 and np.count_nonzero(ref) == 1  # one pixel belongs to one cell (and the operator negates)
        e_hot = max(e_hot, rel_max(gh.cpu().numpy(), ref))
    return fwd_equal, repeatable, e_adj, e_hot


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("gid,size", N.LEAF_CASES, ids=[f"{g}-{s[0]}x{s[1]}" for g, s in N.LEAF_CASES])
def test_nearest_patch_to_dense_and_adjoint(gid, size, dtype):
    fwd_equal, repeatable, e_adj, e_hot = measure_leaf(gid, size, dtype)
    print(f"[nearest] leaf {gid} {size} {dtype}: forward bit-equal {fwd_equal}, adjoint repeatable {repeatable}, adjoint {e_adj:.2e}, "
          f"one-hot adjoints {e_hot:.2e}")
    assert fwd_equal, (gid, size)
    assert repeatable, (gid, size)
    assert e_adj <= ADJ_TOL[dtype] and e_hot <= ADJ_TOL[dtype], (gid, size, e_adj, e_hot)


def test_the_table_reaches_what_it_claims():
    sws = {s for g in N.GEOMETRY.values() for s in g["sw"]}
    assert 1 in sws and 25 in sws
    assert any(g["patch_image_size"] == (1, 1) for g in N.GEOMETRY.values())
    g = N.GEOMETRY["16x16-sw16x21"]  # far beyond the sensor: cells without a pixel on an axis
    size = g["sizes"][0]
    empty = [k for k in (0, 1) if (g["pad"][k] + 1) * g["sw"][k] - N.crop_offset(g, size, k) < 0]
    assert empty, "no cell of the grid lies wholly off the sensor"
    assert N.GEOMETRY["64x64-sw1"]["sw"] == (1, 1)  # one pixel per cell
    g = N.GEOMETRY["3x4-odd"]
    assert {N.crop_offset(g, s, 0) % 2 for s in g["sizes"]} == {0, 1} and {s[0] % 2 for s in g["sizes"]} == {0, 1}  # odd and even crop offsets and H
    assert {s[0] % 2 for s in N.GEOMETRY["sw25"]["sizes"]} == {0, 1}


def test_bilinear_through_the_new_entry_is_the_old_one():
    """cmax_patch_to_dense is the filter = 0 case of cmax_patch_to_dense_filter: the same bits, forward and adjoint."""
    lib = _lib.load()
    g = C.GEOMETRY["3x4-odd"]
    size, (ph, pw), (sh, sw), (pad_h, pad_w) = (27, 40), g["patch_image_size"], g["sw"], g["pad"]
    m_np, cot_np = C.leaf_inputs("3x4-odd", size)
    for dtype in (torch.float64, torch.float32):
        code = _lib.F64 if dtype == torch.float64 else _lib.F32
        for adjoint, src_np, shape in ((0, m_np, (2,) + size), (1, cot_np, (2, ph, pw))):
            src = torch.tensor(src_np, dtype=dtype, device="cuda")
            a, b = torch.empty(shape, dtype=dtype, device="cuda"), torch.empty(shape, dtype=dtype, device="cuda")
            _lib.check(lib.cmax_patch_to_dense(src.data_ptr(), code, ph, pw, pad_h, pad_w, sh, sw, size[0], size[1], adjoint, a.data_ptr(), F._stream()))
            _lib.check(lib.cmax_patch_to_dense_filter(src.data_ptr(), code, ph, pw, pad_h, pad_w, sh, sw, size[0], size[1], _lib.FILTER_BILINEAR,
                                                      adjoint, b.data_ptr(), F._stream()))
            torch.cuda.synchronize()
            assert torch.equal(a, b), (dtype, adjoint)


def test_unknown_filter_code_is_einval():
    lib = _lib.load()
    m = torch.zeros((2, 2, 2), dtype=torch.float64, device="cuda")
    out = torch.full((2, 8, 8), 5.0, dtype=torch.float64, device="cuda")
    for code in (2, -1, 7):
        rc = lib.cmax_patch_to_dense_filter(m.data_ptr(), _lib.F64, 2, 2, 1, 1, 2, 2, 8, 8, code, 0, out.data_ptr(), F._stream())
        assert rc == -1 and b"filter" in lib.cmax_last_error()  # CMAX_EINVAL
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())  # nothing was launched
    with pytest.raises(ValueError, match="filter_type"):
        F.patch_to_dense(m, (8, 8), (2, 2), (1, 1), "cubic")
    # ... and a plan
    b = N.built("plain")
    h, obj = N.make_objective(b["ev"], b["spec"], False, "nearest")
    obj.filter_type = "cubic"
    F.FILTER_CODES["cubic"] = 7
    try:
        with pytest.raises(_lib.CmaxError, match="filter_type") as err:
            obj._build_native_plan()
        assert err.value.code == -1
    finally:
        del F.FILTER_CODES["cubic"]
        obj.filter_type = "nearest"
    del obj
    h.close()


# ---- 2. the native plan ------------------------------------------------------------------------------------------------------------
def errors(b, loss, grad, hv):
    return abs(loss - b["loss"]) / abs(b["loss"]), rel_max(grad, b["grad"]), rel_max(hv, b["hv"])


@pytest.mark.parametrize("cid", list(N.PLAN_CASES))
def test_nearest_plan_value_gradient_and_product(cid):
    b = N.built(cid)
    assert b["dropped"] <= C.DROP_CAP
    h, obj = N.make_objective(b["ev"], b["spec"], b["exact_flow"], "nearest")
    assert obj.has_exact_hvp
    loss, grad = obj.value_and_grad_numpy(b["x"])
    hv = obj.hvp_numpy(b["x"], b["v"])
    e_loss, e_grad, e_hv = errors(b, loss, grad, hv)
    print(f"[nearest] plan {cid}: {len(b['ev'])} events (dropped {b['dropped']:.5f}), rel err loss {e_loss:.2e} grad {e_grad:.2e} Hv {e_hv:.2e}")
    assert e_loss <= TOL and e_grad <= TOL and e_hv <= HVP_TOL, (cid, e_loss, e_grad, e_hv)
    loss_v, none = obj.value_and_grad_numpy(b["x"], want_grad=False)
    assert none is None and abs(loss_v - b["loss"]) <= TOL * abs(b["loss"])
    # it is another objective than the bilinear one at the same point
    bil = N.built(cid, "bilinear")
    assert abs(bil["loss"] - b["loss"]) > 1e-3 * abs(b["loss"])
    del obj
    h.close()


@pytest.mark.parametrize("cid", ["plain", "burgers"])
def test_nearest_autograd_chained_path(cid):
    """PatchFlowObjective.__call__ (functional.patch_to_dense with the filter, its backward the adjoint under the same filter)."""
    b = N.built(cid)
    h, obj = N.make_objective(b["ev"], b["spec"], False, "nearest")
    x = torch.tensor(b["x"], dtype=torch.float64, device="cuda", requires_grad=True)
    loss = obj(x)
    (grad,) = torch.autograd.grad(loss, x)
    e_loss, e_grad = abs(loss.item() - b["loss"]) / abs(b["loss"]), rel_max(grad.cpu().numpy(), b["grad"])
    print(f"[nearest] autograd-chained {cid}: rel err loss {e_loss:.2e} grad {e_grad:.2e}")
    assert e_loss <= TOL and e_grad <= TOL
    if cid == "plain":  # the tensor product is exact for time-ignorant objectives
        assert rel_max(obj.hvp(x.detach(), torch.tensor(b["v"], dtype=torch.float64, device="cuda")).cpu().numpy(), b["hv"]) <= HVP_TOL
    del obj
    h.close()


@pytest.mark.parametrize("cid", ["plain", "burgers"])
def test_nearest_plan_graph_replay_in_a_child_process(cid):
    """CMAX_PLAN_GRAPHS=1 is read when a plan is created: a fresh process with it set, six evaluations and products (replayed from the
    fourth on), every one of them at the gate."""
    b = N.built(cid)
    env = dict(os.environ, CMAX_PLAN_GRAPHS="1")
    run = subprocess.run([sys.executable, os.path.join(HERE, "_nearest_plan_worker.py"), cid], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    out = json.loads(run.stdout.strip().splitlines()[-1])
    assert out["enabled"] and out["n_graphs"] >= 2, out["n_graphs"]
    worst = [0.0, 0.0, 0.0]
    for call in out["calls"]:
        worst = [max(w, e) for w, e in zip(worst, errors(b, call["loss"], np.array(call["grad"]), np.array(call["hv"])))]
    print(f"[nearest] plan {cid}, graph replay ({out['n_graphs']} graphs): worst rel err loss {worst[0]:.2e} grad {worst[1]:.2e} Hv {worst[2]:.2e}")
    assert worst[0] <= TOL and worst[1] <= TOL and worst[2] <= HVP_TOL


@pytest.mark.parametrize("cid", ["plain", "burgers"])
def test_bilinear_plan_through_the_new_field(cid):
    """A bilinear plan whose descriptor carries filter_type = CMAX_FILTER_BILINEAR explicitly, and one from a caller that does not know
    the argument (the slot is the zero it was as padding): the bilinear reference at the gate, and each other's numbers at the
    run-to-run tolerance of tests/test_gpu_weights.py::test_refused_patch_plans (fp32 atomics: 1e-6 loss, 1e-5 gradient, 1e-4 product)."""
    b = N.built(cid, "bilinear")
    ref_loss, ref_grad, ref_hv = _patch_ref.plan(b["x"], b["ev"], {k: v for k, v in b["spec"].items() if k != "filter"}, v=b["v"])
    assert abs(ref_loss - b["loss"]) <= 1e-9 * abs(ref_loss) and rel_max(b["grad"], ref_grad) <= 1e-9 and rel_max(b["hv"], ref_hv) <= 1e-9
    got = []
    for filter_type in (None, "bilinear"):
        h, obj = N.make_objective(b["ev"], b["spec"], False, filter_type)
        loss, grad = obj.value_and_grad_numpy(b["x"])
        hv = obj.hvp_numpy(b["x"], b["v"])
        e_loss, e_grad, e_hv = errors(b, loss, grad, hv)
        assert e_loss <= TOL and e_grad <= TOL and e_hv <= HVP_TOL, (filter_type, e_loss, e_grad, e_hv)
        got.append((loss, grad, hv))
        del obj
        h.close()
    (l0, g0, hv0), (l1, g1, hv1) = got
    print(f"[nearest] bilinear plan {cid}, old caller vs explicit field: loss {abs(l1 - l0) / abs(l0):.2e} grad {rel_max(g1, g0):.2e} Hv {rel_max(hv1, hv0):.2e}")
    assert abs(l1 - l0) <= 1e-6 * abs(l0) and rel_max(g1, g0) <= 1e-5 and rel_max(hv1, hv0) <= 1e-4


def test_descriptor_size_on_the_device_library():
    assert _lib.load().cmax_sizeof_patch_objective() == ctypes.sizeof(_lib.CmaxPatchObjective)
