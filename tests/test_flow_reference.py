"""No GPU.  tests/_flow_ref.py -- the torch fp64 restatement the voxel-chain kernels are compared with in tests/test_gpu_flow_chain.py --
against the C oracle on every case of that test's table, against the golden fixtures of the reference (flow_voxel.npz, at the
tolerances tests/test_oracle_golden.py holds the oracle to), its second-order parts against central differences, and its tie rule
against values worked out by hand."""
import numpy as np
import pytest
import torch

import _flow_cases as C
import _flow_ref as R
from oracle import oracle as orc

DTYPES = ("float64", "float32")
ORC_STEP = {"burgers": (orc.burgers_step, orc.burgers_step_adj), "upwind": (orc.upwind_step, orc.upwind_step_adj)}


def t64(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64)


def rel(got, ref):
    """Largest difference relative to the largest entry of the reference."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)


def test_case_table_straddles_the_launch_form_switch():
    assert C.tiled_chain_limit("float64") == 10 and C.tiled_chain_limit("float32") == 19
    assert C.long_T("float64") == [(21, "middle"), (22, "middle"), (11, "first"), (12, "first")]
    assert C.long_T("float32") == [(39, "middle"), (40, "middle"), (20, "first"), (21, "first")]
    assert [C.chains(T, loc) for T, loc in C.long_T("float64")] == [(10, 10), (11, 10), (0, 10), (0, 11)]
    for dtype in DTYPES:
        for shape in C.SHAPES:
            f = {name: C.field(name, shape, dtype) for name in C.FIELDS}
            assert all(np.abs(a).max() <= 3.0 and np.array_equal(a, a.astype(dtype).astype(np.float64)) for a in f.values())
            assert (f["rough"] != 0).all() and (f["smooth"] != 0).all()
            assert (f["kinks"][0] == 0).any() and (f["kinks"][1] == 0).any()
        k = C.field("kinks", (35, 70), dtype)
        assert (k[:, 14:19, 30:35] == 0).all() and (k[0, 15] == 0).all() and (k[1, :, 31] == 0).all() and (k[1, 15, :30] != 0).all()
        assert (np.sign(k[:, 2:8, 3:9]) == np.where(np.add.outer(np.arange(2, 8), np.arange(3, 9)) % 2 == 0, 1, -1)).all()


@pytest.mark.parametrize("scheme", R.SCHEMES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_step_equals_the_oracle(dtype, scheme):
    step, adj = ORC_STEP[scheme]
    for shape in C.SHAPES:
        gout = C.directions(shape, 1, dtype)[0]
        for name in C.FIELDS:
            f = C.field(name, shape, dtype)
            for dt in (0.25, -0.1, 0.0):
                assert rel(R.step(t64(f), dt, scheme).numpy(), step(f, dt)) <= 1e-12, (shape, name, dt)
                assert rel(R.step_vjp(t64(f), dt, scheme, t64(gout)).numpy(), adj(f, dt, gout)) <= 1e-12, (shape, name, dt)


@pytest.mark.parametrize("scheme", R.SCHEMES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_voxel_and_adjoint_equal_the_oracle_on_every_case(dtype, scheme):
    worst = [0.0, 0.0, 0.0]
    for case in C.cases(dtype):
        shape, T, loc, name = case
        f = C.field(name, shape, dtype)
        _, gV, _ = C.directions(shape, T, dtype)
        x = t64(f).requires_grad_()
        V = R.voxel(x, T, scheme, loc)
        V_orc = orc.construct_dense_flow_voxel(f, T, scheme, loc)
        e_v = rel(V.detach().numpy(), V_orc)
        gF_orc = orc.construct_dense_flow_voxel_adj(V_orc, gV, scheme, loc)
        e_at = rel(R.adj_at(t64(V_orc), t64(gV), scheme, loc).numpy(), gF_orc)
        (g_auto,) = torch.autograd.grad(V, x, grad_outputs=t64(gV))
        e_auto = rel(g_auto.numpy(), gF_orc)
        worst = [max(w, e) for w, e in zip(worst, (e_v, e_at, e_auto))]
        assert max(e_v, e_at, e_auto) <= 1e-12, (C.case_id(case), e_v, e_at, e_auto)
    print(f"reference vs oracle {dtype} {scheme}: voxel {worst[0]:.1e}  adj_at {worst[1]:.1e}  autograd {worst[2]:.1e}")


@pytest.mark.parametrize("fname", ["rand", "smooth", "withzeros"])
@pytest.mark.parametrize("dt", [0.1, -0.1, 0.01, -0.037, 0.0])
@pytest.mark.parametrize("scheme", R.SCHEMES)
def test_golden_flow_steps(golden, fname, dt, scheme):
    g = golden("flow_voxel")
    fl, tag = t64(g[f"flow_{fname}"]), f"{fname}_dt{dt}"
    np.testing.assert_allclose(R.step(fl, dt, scheme).numpy(), g[f"{scheme}_step_{tag}"], rtol=1e-11, atol=1e-12)
    if dt != 0.0:
        vjp = R.step_vjp(fl, dt, scheme, t64(g[f"{scheme}_cot_{tag}"]))
        np.testing.assert_allclose(vjp.numpy(), g[f"{scheme}_vjp_{tag}"], rtol=1e-10, atol=1e-11)


@pytest.mark.parametrize("fname", ["smooth", "withzeros"])
@pytest.mark.parametrize("T,loc", [(10, "middle"), (5, "middle"), (4, "first")])
@pytest.mark.parametrize("scheme", R.SCHEMES)
def test_golden_voxels(golden, fname, T, loc, scheme):
    g = golden("flow_voxel")
    tag = f"{scheme}_{fname}_T{T}_{loc}"
    x = t64(g[f"flow_{fname}"]).requires_grad_()
    V = R.voxel(x, T, scheme, loc)
    np.testing.assert_allclose(V.detach().numpy(), g[f"voxel_{tag}"], rtol=1e-10, atol=1e-11)
    cot = t64(g[f"voxel_cot_{tag}"])
    (g_auto,) = torch.autograd.grad(V, x, grad_outputs=cot)
    np.testing.assert_allclose(g_auto.numpy(), g[f"voxel_vjp_{tag}"], rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(R.adj_at(V.detach(), cot, scheme, loc).numpy(), g[f"voxel_vjp_{tag}"], rtol=1e-9, atol=1e-10)


@pytest.mark.parametrize("scheme", R.SCHEMES)
@pytest.mark.parametrize("loc", ["middle", "first"])
def test_second_order_against_difference_quotients(scheme, loc):
    """On a smooth flow that stays away from zero (no selector changes inside the difference quotient) `tan` is the central
    difference of `voxel`, and `adj_tan_at` that of `adj_at` along the voxel plus the part linear in dgV: 1e-6 / 2e-6, the bounds of
    test_voxel_chain_second_order_against_difference_quotients on the GPU."""
    shape, T, eps = (17, 33), 7, 1e-6
    i, j = np.meshgrid(np.arange(shape[0]) / 16.0, np.arange(shape[1]) / 32.0, indexing="ij")
    f = t64(np.stack([2.0 + 0.8 * np.sin(1.3 * i + 0.7 * j), -1.5 + 0.6 * np.cos(0.8 * i - 1.1 * j)]))
    dF, gV, dgV = (t64(a) for a in C.directions(shape, T, "float64"))
    V, dV = R.tan(f, dF, T, scheme, loc)
    assert torch.equal(V, R.voxel(f, T, scheme, loc)) and V.abs().min() > 0.5
    Vp, Vm = R.voxel(f + eps * dF, T, scheme, loc), R.voxel(f - eps * dF, T, scheme, loc)
    e_tan = rel(dV, (Vp - Vm) / (2 * eps))
    gF, dgF = R.adj_tan_at(V, dV, gV, dgV, scheme, loc)
    assert torch.equal(gF, R.adj_at(V, gV, scheme, loc))
    fd = (R.adj_at(Vp, gV, scheme, loc) - R.adj_at(Vm, gV, scheme, loc)) / (2 * eps) + R.adj_at(V, dgV, scheme, loc)
    e_adj = rel(dgF, fd)
    print(f"reference vs central differences {scheme} {loc}: tan {e_tan:.1e}  adj_tan_at {e_adj:.1e}")
    assert e_tan <= 1e-6 and e_adj <= 2e-6


def _hand_field():
    """3 x 3, zero at the centre in both channels; its four neighbours (above, below, left, right): u = 1, 3, 2, 5 and v = 1, -1, 0, 4."""
    f = torch.zeros(2, 3, 3, dtype=torch.float64)
    f[0, 0, 1], f[0, 2, 1], f[0, 1, 0], f[0, 1, 2] = 1.0, 3.0, 2.0, 5.0
    f[1, 0, 1], f[1, 2, 1], f[1, 1, 0], f[1, 1, 2] = 1.0, -1.0, 0.0, 4.0
    dF = torch.zeros_like(f)
    dF[0, 1, 1], dF[1, 1, 1] = 1.0, 2.0  # (du, dv) at the centre, nothing elsewhere
    return f, dF


def test_tie_rule_by_hand_upwind():
    """T = 2 from the first bin: one step of tau = 1/2.  At the centre u = v = 0, so max(., 0) and min(., 0) are both at their tie and
    each hands HALF of the tangent on; their values are 0, so the differences of the tangent drop out:
        d u_new = du - tau/2 (du (u_below - u_above) + dv (u_right - u_left)) = 1 - (1 (3 - 1) + 2 (5 - 2)) / 4 = -1
        d v_new = dv - tau/2 (du (v_below - v_above) + dv (v_right - v_left)) = 2 - (1 (-1 - 1) + 2 (4 - 0)) / 4 = 1/2
    A rule that gave the tie to neither side would leave (du, dv) = (1, 2)."""
    f, dF = _hand_field()
    _, dV = R.tan(f, dF, 2, "upwind", "first")
    assert torch.equal(dV[0], dF)
    assert dV[1, 0, 1, 1].item() == -1.0 and dV[1, 1, 1, 1].item() == 0.5


def test_tie_rule_by_hand_burgers():
    """Same field and step.  The cross terms tie like the upwind ones; the Burgers term B(u) = (u^2 sign(u) - max(sign(u_above), 0)
    u_above^2 - min(sign(u_below), 0) u_below^2) / 2 has no derivative through sign(), and its own derivative |u| du vanishes at u = 0:
        d u_new = du - tau/2 dv (u_right - u_left) = 1 - 2 (5 - 2) / 4 = -1/2
        d v_new = dv - tau/2 du (v_below - v_above) = 2 - 1 (-1 - 1) / 4 = 5/2
    Seen from the pixel BELOW the centre, the centre is the zero neighbour u_above: sign(0) = 0 switches that term off, so neither the
    tangent of that pixel nor the second derivative of its step with respect to the centre sees the centre's u at all -- there is no
    1/2 in the Burgers term, at either order."""
    f, dF = _hand_field()
    _, dV = R.tan(f, dF, 2, "burgers", "first")
    assert dV[1, 0, 1, 1].item() == -0.5 and dV[1, 1, 1, 1].item() == 2.5
    assert dV[1, 0, 2, 1].item() == 0.0 and dV[1, 0, 0, 1].item() == 0.0
    # second order: gV picks u of the pixel below the centre in bin 1, the voxel moves along u of the centre in bin 0
    V = R.voxel(f, 2, "burgers", "first")
    dV0, gV = torch.zeros_like(V), torch.zeros_like(V)
    dV0[0, 0, 1, 1] = 1.0
    gV[1, 0, 2, 1] = 1.0
    gF, dgF = R.adj_tan_at(V, dV0, gV, torch.zeros_like(V), "burgers", "first")
    assert gF[0, 2, 1].item() == 1.0 - 0.5 * (1.0 + 3.0)  # the pixel itself, u = 3, v = -1: 1 - tau (-min(v, 0) + |u|)
    assert torch.count_nonzero(dgF).item() == 0
