"""Anchors tests/_iwe_ref.py -- the fp64 reference of the IWE layer -- without a GPU:
    images                against the committed oracle's vote / blur3 (weights included)                      at 1e-12
    VJP of a random G     against the oracle's blur3_adj -> vote_bwd -> motion_grad, grad_w against its gw    at 1e-10
    composed with a cost  against _hvp_ref.value_grad_hvp (loss, gradient, H v) on cases of tests/_hvp_cases   at 1e-10
    JVP, vjp_tan          against central differences of the reference's own images and VJP
and caps the share of events the border filter removes from every batch the GPU tests use (second-order quantities are not defined on
a cell border) at 0.5 %."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc

import _hvp_cases as C
import _iwe_cases as IC
import _iwe_ref as IR


def rel_max(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


SMALL = [c["id"] for c in IC.CASES if c["n"] <= 2000 and c["t_slice"] is None][:8] + \
        [c["id"] for c in IC.CASES if c["group"] in ("fracpad", "outside", "rawtime")][:4]


def test_every_gpu_batch_keeps_its_events():
    cases = list(IC.ALL.values())
    assert len(cases) >= 30
    for c in cases:
        b = C.inputs(c)
        assert b["dropped"] <= C.DROP_CAP, (c["id"], b["dropped"])
        assert len(b["ev"]) > 0


@pytest.mark.parametrize("cid", SMALL)
@pytest.mark.parametrize("wname", ["none", "zeros"])
def test_images_and_vjp_against_the_oracle(cid, wname):
    c = IC.ALL[cid]
    b = IC.built(c, wname)
    cfg, ev, w = b["cfg"], b["ev"], b["w"]
    wo = 1.0 if w is None else w
    G = b["cot"]["G"]
    gm, gw = np.zeros_like(b["gm"]), np.zeros(len(ev))
    planes = list(cfg["directions"]) + ([None] if cfg["with_orig"] else [])
    for k, direction in enumerate(planes):
        if direction is None:
            warped, aux = ev, None
        else:
            warped, aux = orc.warp_event(ev, b["motion"], c["model"], direction, c["size"], c["normalize_t"])
        img = orc.vote(warped, c["size"], c["pad"], wo)
        img = orc.blur3(img, c["sigma"]) if c["sigma"] > 0 else img
        assert rel_max(b["images"][k], img) <= 1e-12, (cid, k)
        Gk = orc.blur3_adj(G[k], c["sigma"]) if c["sigma"] > 0 else G[k]
        gx, gy, g_w = orc.vote_bwd(warped, c["size"], Gk, c["pad"], wo, want_gw=True)
        gw += g_w
        if aux is not None:
            gm += orc.motion_grad(ev, b["motion"], c["model"], aux, gx, gy)
    assert rel_max(b["gm"], gm) <= 1e-10, (cid, rel_max(b["gm"], gm))
    assert rel_max(b["gw"], gw) <= 1e-10, (cid, rel_max(b["gw"], gw))


@pytest.mark.parametrize("cid", [c["id"] for c in C.CASES if c["group"] == "matrix" and c["n"] <= 2000][:12])
def test_composed_with_a_torch_cost_it_is_the_hvp_reference(cid):
    """loss, gradient and H v of the built-in costs written in torch on the layer's images == _hvp_ref.value_grad_hvp."""
    c = C.ALL[cid]
    b = C.built(c)
    cfg = IC.layer_config(c)
    cost = IR.torch_cost(c["cost"], c["omit"], c["direction"])
    ev, m = IR._t(b["ev"]), IR._t(b["motion"]).requires_grad_()
    imgs = IR.images_t(ev, m, torch.ones(len(b["ev"]), dtype=torch.float64), c["model"], c["size"], cfg["directions"], sigma=c["sigma"],
                       outer_padding=c["pad"], normalize_t=c["normalize_t"], t_range=b["t_range"], with_orig=cfg["with_orig"])
    arg = {"omit_boundary": c["omit"]}
    keys = ["forward_iwe", "backward_iwe", "middle_iwe"] if len(cfg["directions"]) == 3 else ["iwe"]
    for k, key in enumerate(keys):
        arg[key] = imgs[k]
    if cfg["with_orig"]:
        arg["orig_iwe"] = imgs[len(keys)]
    loss = cost(arg)
    (g,) = torch.autograd.grad(loss, m, create_graph=True)
    (hv,) = torch.autograd.grad((g * IR._t(b["v"]).reshape(m.shape)).sum(), m)
    assert abs(float(loss.detach()) - b["loss"]) <= 1e-10 * abs(b["loss"])
    assert rel_max(g.detach().numpy(), b["grad"]) <= 1e-10
    assert rel_max(hv.numpy(), b["hv"]) <= 1e-10


@pytest.mark.parametrize("cid", SMALL[:6])
@pytest.mark.parametrize("wname", ["none", "polarity"])
def test_jvp_and_vjp_tan_against_central_differences(cid, wname):
    c = IC.ALL[cid]
    b = IC.built(c, wname)
    cfg, L = b["cfg"], b["layer"]
    G, Gp = b["cot"]["G"], b["cot"]["Gp"]
    v = b["v"]
    h = 1e-6 * max(np.abs(b["motion"]).max(), 1.0) / np.abs(v).max()

    def at(step):
        return IR.Layer(b["ev"], b["motion"] + step * v, c["model"], c["size"], cfg["directions"], b["w"], sigma=c["sigma"], outer_padding=c["pad"],
                        normalize_t=c["normalize_t"], t_range=b["t_range"], with_orig=cfg["with_orig"])

    Lp, Lm = at(h), at(-h)
    n_ref = len(cfg["directions"])
    fd_images = (Lp.images() - Lm.images())[:n_ref] / (2 * h)
    assert rel_max(b["jv"], fd_images) <= 2e-7, rel_max(b["jv"], fd_images)
    fd_mixed = (Lp.vjp(G)[0] - Lm.vjp(G)[0]) / (2 * h)
    assert rel_max(b["vt_mixed"], fd_mixed) <= 2e-7 or not np.abs(fd_mixed).max() > 1e-9 * np.abs(b["gm"]).max(), rel_max(b["vt_mixed"], fd_mixed)
    # the part that is linear in G' is the VJP of G'
    assert rel_max(b["vt"] - b["vt_mixed"], L.vjp(Gp)[0]) <= 1e-10
    # <G, J v> = <J^T G, v>
    lhs, rhs = float((G[:n_ref] * b["jv"]).sum()), float((b["gm"] * v.reshape(b["gm"].shape)).sum())
    assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), abs(rhs), 1e-300)
