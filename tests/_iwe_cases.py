"""The cases of the IWE-layer tests, shared by tests/test_iwe_reference.py (no GPU: anchors tests/_iwe_ref.py and caps the share of events
the border filter removes) and tests/test_gpu_iwe_layer.py / tests/_iwe_layer_worker.py.  Batches, motions and tangents are those of
tests/_hvp_cases.py (imported, not edited): a case here is one of its cases read as a LAYER configuration -- the reference times its cost
warps to, its blur, padding, time normalisation, and the un-warped image where its cost reads one -- plus a weight set and seeded
random image cotangents.  The fp64 answers are computed once per process and shared."""
import numpy as np

import _hvp_cases as C
import _hvp_ref as R
import _iwe_ref as IR
import _weighted_ref as WR

WEIGHT_SETS = ("none", "uniform", "polarity", "zeros", "w100", "hdr")  # "hdr" (1000 : 1) is outside the supported range: printed only


def _pick(group, **want):
    out = [c for c in C.CASES if c["group"] == group and all(c[k] == v for k, v in want.items())]
    assert out, (group, want)
    return out


def _select():
    two, dense, voxel = C.MODELS
    iv, gm, niv, ngm, mfiv, mfgm = C.COSTS
    out = []
    # 3 models x (n_ref 1 | n_ref 1 + un-warped | n_ref 3 + un-warped) x sigma 0 / 1: 60 / 2000 / 30 000 events, voxel T = 2 and 5
    for cost in (iv, niv, mfgm):
        out += _pick("matrix", cost=cost)
    out += _pick("fracpad", frac=True, pad=3)  # fractional sources, padding 3, reference time 1/3
    out += _pick("reftime", warp_direction=0.3)
    out += _pick("rawtime", cost=iv)  # normalize_t = False
    out += _pick("outside", cost=iv)  # off-sensor 2-DoF events, padding 0 and 3
    out += [c for c in _pick("clipped") if (c["model"], c["cost"]) in ((two, iv), (dense, gm))]  # the clipped window, with and without slabs
    return out


CASES = _select()
ALL = {c["id"]: c for c in CASES}
# weighted handles: one 30 000-event case per model (and one blurred), every weight set
WEIGHTED = [c["id"] for c in CASES if c["group"] == "matrix" and c["n"] == 30_000 and c["cost"] in (C.COSTS[0], C.COSTS[5])][:4] + \
           [c["id"] for c in CASES if c["group"] == "clipped" and c["slabs"] == 4]
# every case of the forced segment layouts (tests/_iwe_layer_worker.py)
LAYOUT_CASES = {k: [c for c in v if c["cost"] in (C.COSTS[0], C.COSTS[1])][:4] for k, v in C.LAYOUT_CASES.items()}
for _v in LAYOUT_CASES.values():
    ALL.update({c["id"]: c for c in _v})


def layer_config(c):
    """The keyword arguments of CMaxHandle.iwes / fused_iwes for case c."""
    return dict(motion_model=c["model"], directions=tuple(R.cost_directions(c["cost"], c["warp_direction"])), sigma=float(c["sigma"]),
                normalize_t=c["normalize_t"], with_orig="normalized" in c["cost"])


def weights(name, ev, seed=3):
    if name == "none":
        return None
    if name == "w100":
        return IR.weight_set_100(ev, seed)
    return WR.weight_set(name, ev, seed)


def cotangents(c, shape, images=None):
    """Seeded image cotangents: G and G' random dense; `onehot` on the pixel that holds the most votes of image 0; `border` non-zero only
    in the outermost two rows / columns of the padded image (the padding included)."""
    rng = np.random.default_rng(9000 + c["seed"])
    G, Gp = C.f32(rng.normal(0.0, 1.0, shape)), C.f32(rng.normal(0.0, 1.0, shape))
    onehot = np.zeros(shape)
    if images is not None:
        r, col = np.unravel_index(int(np.abs(images[0]).argmax()), images[0].shape)
        onehot[0, r, col] = 1.0
    border = G.copy()
    m = 2 + c["pad"]
    border[:, m:-m, m:-m] = 0.0
    return dict(G=G, Gp=Gp, onehot=onehot, border=border)


_BUILT = {}


def built(c, wname="none"):
    """inputs(c), the layer's configuration and weights, the cotangents and the fp64 answers: images, (gm, gw) = VJP of G, J v, and
    vjp_tan(v, G, G') / vjp_tan(v, G, 0)."""
    key = (c["id"], wname)
    if key not in _BUILT:
        b = dict(C.inputs(c))
        cfg = layer_config(c)
        b["cfg"], b["w"] = cfg, weights(wname, b["ev"])
        L = IR.Layer(b["ev"], b["motion"], c["model"], c["size"], cfg["directions"], b["w"], sigma=c["sigma"], outer_padding=c["pad"],
                     normalize_t=c["normalize_t"], t_range=b["t_range"], with_orig=cfg["with_orig"])
        b["layer"] = L
        b["images"] = L.images()
        b["cot"] = cotangents(c, b["images"].shape, b["images"])
        G, Gp = b["cot"]["G"], b["cot"]["Gp"]
        b["gm"], b["gw"] = L.vjp(G)
        b["jv"] = L.jvp(b["v"])
        b["vt"] = L.vjp_tan(b["v"], G, Gp)
        b["vt_mixed"] = L.vjp_tan(b["v"], G, None)
        _BUILT[key] = b
    return _BUILT[key]
