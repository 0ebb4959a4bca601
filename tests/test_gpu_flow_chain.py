"""The time-aware flow kernels (csrc/cmax_flow.hip, csrc/cmax_flow_dual.h) against the torch fp64 restatement of tests/_flow_ref.py,
on the case table of tests/_flow_cases.py: every tile seam of the 16 x 32 tiles, fields with exact zeros, both launch forms of
voxel_construct on both sides of their switch, fp32 and fp64, the atomic and the order-free (leaf-deterministic) adjoints, and the
dual-number second-order kernels.  tests/test_flow_reference.py anchors the restatement to the oracle and the reference's fixtures.

Every adjoint is compared with the restatement evaluated AT THE DEVICE'S OWN VOXEL (upcast to fp64): the kernels read their selectors
(sign, max / min and their ties) from the saved voxel, so a last-bit difference between the two forwards cannot flip one, and every
pixel is compared -- nothing is masked.  Bounds: 1e-10 (fp64) and 2e-4 (fp32) of the largest entry of the reference array, the bounds
of test_random_leaf_operators_against_oracle, with no slack added."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _flow_cases as C  # noqa: E402
import _flow_ref as R  # noqa: E402
from event_based_optical_flow_amd import _lib  # noqa: E402
from event_based_optical_flow_amd import functional as F  # noqa: E402

DEV = "cuda"
TORCH = {"float64": torch.float64, "float32": torch.float32}
CASES = [pytest.param(dtype, case, id=f"{dtype}-{C.case_id(case)}") for dtype in TORCH for case in C.cases(dtype)]
STEP_CASES = [pytest.param(dtype, shape, id=f"{dtype}-{shape[0]}x{shape[1]}") for dtype in TORCH for shape in C.SHAPES]

WORST = {}  # (check, dtype, scheme) -> (largest error relative to its bound's scale, case): printed when the module is done


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for (check, dtype, scheme), (err, where) in sorted(WORST.items()):
        print(f"\nflow-chain parity  {check:<28s} {dtype} {scheme:<7s} max rel err {err:.2e}  at {where}", end="")
    print()


def dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=TORCH[dtype], device=DEV)


def up(t):
    return t.detach().to("cpu", torch.float64)


def close(got, ref, check, dtype, scheme, where):
    got, ref = up(got), ref.detach()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), (check, dtype, scheme, where)
    err = (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)
    key = (check, dtype, scheme)
    if err >= WORST.get(key, (-1.0, None))[0]:
        WORST[key] = (err, where)
    assert err <= C.TOL[dtype], (check, dtype, scheme, where, err)


class leaf_deterministic:
    """cmax_set_leaf_deterministic is process-wide: set it for a block and put the previous value back."""

    def __init__(self, enable):
        self.enable = enable

    def __enter__(self):
        self.prev = F.set_leaf_deterministic(self.enable)

    def __exit__(self, *exc):
        F.set_leaf_deterministic(self.prev)


_INPUTS = {}  # (dtype, case) -> fp64 CPU tensors (F, dF, gV, dgV), exact in dtype
_TAN = {}     # (dtype, scheme, case) -> (V, dV) of the restatement: computed once, never written to


def inputs(dtype, case):
    if (dtype, case) not in _INPUTS:
        shape, T, _, name = case
        _INPUTS[dtype, case] = tuple(torch.from_numpy(a) for a in (C.field(name, shape, dtype),) + C.directions(shape, T, dtype))
    return _INPUTS[dtype, case]


def ref_tan(dtype, scheme, case):
    if (dtype, scheme, case) not in _TAN:
        _, T, loc, _ = case
        f, dF, _, _ = inputs(dtype, case)
        _TAN[dtype, scheme, case] = R.tan(f, dF, T, scheme, loc)
    return _TAN[dtype, scheme, case]


# ---- 1. one step and its adjoint ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", R.SCHEMES)
@pytest.mark.parametrize("dtype,shape", STEP_CASES)
def test_flow_step_and_adjoint(dtype, shape, scheme):
    gout = torch.from_numpy(C.directions(shape, 1, dtype)[0])
    for name in C.FIELDS:
        f = torch.from_numpy(C.field(name, shape, dtype))
        for dt in (0.25, -0.1, 0.0):
            where = f"{shape[0]}x{shape[1]} {name} dt={dt}"
            out_ref, vjp_ref = R.step(f, dt, scheme), R.step_vjp(f, dt, scheme, gout)
            for det in (False, True):
                with leaf_deterministic(det):
                    x = dev(f, dtype).requires_grad_()
                    out = F.flow_step(x, dt, scheme)
                    (g,) = torch.autograd.grad(out, x, grad_outputs=dev(gout, dtype))
                close(out, out_ref, "1 step", dtype, scheme, where)
                close(g, vjp_ref, "1 step adjoint" + (" det" if det else ""), dtype, scheme, where)


# ---- 2. the voxel, every bin ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", R.SCHEMES)
@pytest.mark.parametrize("dtype,case", CASES)
def test_voxel_every_bin(dtype, case, scheme):
    _, T, loc, _ = case
    V = F.construct_dense_flow_voxel(dev(inputs(dtype, case)[0], dtype), T, scheme, loc)
    close(V, ref_tan(dtype, scheme, case)[0], "2 voxel", dtype, scheme, C.case_id(case))


# ---- 3. the adjoint, at the device's voxel ----------------------------------------------------------------------------------
def device_adjoint(f, gV, T, scheme, loc):
    x = f.clone().requires_grad_()
    V = F.construct_dense_flow_voxel(x, T, scheme, loc)
    (g,) = torch.autograd.grad(V, x, grad_outputs=gV)
    return V.detach(), g


@pytest.mark.parametrize("scheme", R.SCHEMES)
@pytest.mark.parametrize("dtype,case", CASES)
def test_voxel_adjoint_at_the_device_voxel(dtype, case, scheme):
    _, T, loc, _ = case
    f, _, gV, _ = inputs(dtype, case)
    V, g = device_adjoint(dev(f, dtype), dev(gV, dtype), T, scheme, loc)
    g_ref = R.adj_at(up(V), gV, scheme, loc)
    close(g, g_ref, "3 voxel adjoint", dtype, scheme, C.case_id(case))
    with leaf_deterministic(True):
        V1, g1 = device_adjoint(dev(f, dtype), dev(gV, dtype), T, scheme, loc)
        _, g2 = device_adjoint(dev(f, dtype), dev(gV, dtype), T, scheme, loc)
    assert torch.equal(V1, V)
    close(g1, g_ref, "3 voxel adjoint det", dtype, scheme, C.case_id(case))
    assert torch.equal(g1, g2), "the order-free adjoint differs between two runs"


# ---- 4. voxel and tangent (dual numbers) ------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", R.SCHEMES)
@pytest.mark.parametrize("dtype,case", CASES)
def test_voxel_tangent(dtype, case, scheme):
    _, T, loc, _ = case
    f, dF, _, _ = inputs(dtype, case)
    V, dV = F.voxel_construct_tan(dev(f, dtype), dev(dF, dtype), T, scheme, loc)
    V_ref, dV_ref = ref_tan(dtype, scheme, case)
    close(V, V_ref, "4 tan: voxel", dtype, scheme, C.case_id(case))
    close(dV, dV_ref, "4 tan: tangent", dtype, scheme, C.case_id(case))
    # the dual kernels and the first-order ones run the same arithmetic on the value, whichever launch form the latter took
    assert torch.equal(V, F.construct_dense_flow_voxel(dev(f, dtype), T, scheme, loc))


# ---- 5. second-order adjoint, at the device's (V, dV) -----------------------------------------------------------------------
@pytest.mark.parametrize("scheme", R.SCHEMES)
@pytest.mark.parametrize("dtype,case", CASES)
def test_voxel_adjoint_tangent_at_the_device_voxel(dtype, case, scheme):
    _, T, loc, _ = case
    f, dF, gV, dgV = inputs(dtype, case)
    V, dV = F.voxel_construct_tan(dev(f, dtype), dev(dF, dtype), T, scheme, loc)
    gF_ref, dgF_ref = R.adj_tan_at(up(V), up(dV), gV, dgV, scheme, loc)
    for det in (False, True):
        tag = " det" if det else ""
        with leaf_deterministic(det):
            gF, dgF = F.voxel_construct_adj_tan(V, dV, dev(gV, dtype), dev(dgV, dtype), scheme, loc)
            again = F.voxel_construct_adj_tan(V, dV, dev(gV, dtype), dev(dgV, dtype), scheme, loc) if det else None
        close(gF, gF_ref, "5 adj_tan: gF" + tag, dtype, scheme, C.case_id(case))
        close(dgF, dgF_ref, "5 adj_tan: dgF" + tag, dtype, scheme, C.case_id(case))
        if det:
            assert torch.equal(gF, again[0]) and torch.equal(dgF, again[1]), "the order-free second-order adjoint differs between two runs"


# ---- 6. bad arguments ---------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_einval_and_launch_nothing():
    lib = _lib.load()
    H, W, T = 5, 7, 3
    f = torch.full((2, H, W), 2.0, dtype=torch.float64, device=DEV)
    out = torch.full((T, 2, H, W), -7.0, dtype=torch.float64, device=DEV)
    p, o, s = f.data_ptr(), out.data_ptr(), F._stream()
    EINVAL = -1  # CMAX_EINVAL, include/cmax_hip.h
    vox, step, dt = lib.cmax_voxel_construct, lib.cmax_flow_step, ctypes.c_double(0.1)
    bad = [  # (what, call, what the message has to name)
        ("T = 0", lambda: vox(p, _lib.F64, 0, 0, H, W, _lib.SCHEME_BURGERS, o, s), b"bad argument: voxel_construct"),
        ("t0 = T", lambda: vox(p, _lib.F64, T, T, H, W, _lib.SCHEME_BURGERS, o, s), b"bad argument: voxel_construct"),
        ("t0 < 0", lambda: vox(p, _lib.F64, T, -1, H, W, _lib.SCHEME_UPWIND, o, s), b"bad argument: voxel_construct"),
        ("scheme", lambda: vox(p, _lib.F64, T, 1, H, W, 2, o, s), b"voxel_construct: scheme"),
        ("dtype", lambda: vox(p, 7, T, 1, H, W, _lib.SCHEME_UPWIND, o, s), b"voxel_construct: dtype"),
        ("step scheme", lambda: step(p, _lib.F64, H, W, dt, -1, o, s), b"flow_step: scheme"),
        ("step dtype", lambda: step(p, 2, H, W, dt, _lib.SCHEME_BURGERS, o, s), b"flow_step: dtype"),
        ("step F == out", lambda: step(p, _lib.F64, H, W, dt, _lib.SCHEME_BURGERS, p, s), b"bad argument: flow_step"),
    ]
    for what, call, names in bad:
        assert call() == EINVAL, what
        msg = lib.cmax_last_error()
        assert msg and names in msg, (what, msg)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((f == 2.0).all())
    # the same buffers with good arguments: the calls above left the library usable
    assert lib.cmax_voxel_construct(p, _lib.F64, T, 1, H, W, _lib.SCHEME_BURGERS, o, s) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[1], f)
