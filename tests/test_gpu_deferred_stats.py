"""The 2-DoF plain-variance objective takes sum I and sum I^2 from K3's gather (deferred statistics, csrc/cmax_event_kernels.inc):
the image is the sum of the events' bilinear votes, so over the region Omega the variance is taken over

    sum_p I[p]^2 = sum_e sum_{c in corners(e)} w_ec I[c] 1_Omega(c),        sum_p I[p] = sum_e sum_c w_ec 1_Omega(c),

and no pass over the image is made.  Everything here goes against the fp64 oracle at the project's plain gate (loss, the per-reference-
time contrasts result[1 + k] and the gradient: 1e-4), on the smallest shapes at which the new sums can go wrong: sizes that are no
multiple of the 16-pixel tile, windows inside one tile / over the border of Omega / mostly outside the image, omit_boundary on and
off, one to three reference times, off-sensor events, a clipped window, an image without contrast (the cancellation's worst case)
and a sharp one.  Oracle references are computed once per case and shared.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import event_based_optical_flow_amd as E  # noqa: E402
from event_based_optical_flow_amd import _lib  # noqa: E402
from event_based_optical_flow_amd import functional as F  # noqa: E402
from oracle import oracle as orc  # noqa: E402

TOL = 1e-4
MODEL = "2d-translation"
SHAPES = {"37x53": ((37, 53), 6_000, 101), "48x64": ((48, 64), 20_000, 102)}
THETAS = [(0.0, 0.0), (0.3, -0.2), (12.3, -7.7), (-40.0, 25.0)]
# (reference time, multiplier) per image, as the multi-focal costs list them (cmax._COST_TABLE) -- here without the normalisation
REFS = {1: (("first", 1.0),), 2: (("first", 1.0), ("last", 1.0)), 3: (("last", 1.0), ("first", 1.0), ("middle", 2.0))}


def rel_max(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@functools.lru_cache(maxsize=None)
def uniform_events(shape):
    size, n, seed = SHAPES[shape]
    ev = E.utils.generate_events(n, size[0], size[1], 0.0, 0.05, seed=seed)
    ev.setflags(write=False)
    return ev


def descriptor(refs=REFS[1], omit=True, direction="minimize", negate=False):
    d = E.make_descriptor("image_variance", MODEL, direction=direction, omit_boundary=omit)
    d.n_ref = len(refs)
    for k, (ref_dir, mult) in enumerate(refs):
        d.ref_mode[k], d.ref_frac[k] = F.direction_to_ref(ref_dir)
        d.mult[k] = mult
    d.negate = int(negate)
    return d


def oracle_sum(ev, theta, size, refs=REFS[1], omit=True, direction="minimize", pad=0):
    """The plain variance summed over reference times: (loss, gradient, [variance per reference time], [image per reference time])."""
    loss, grad, contrasts, images = 0.0, np.zeros(2), [], []
    for ref_dir, mult in refs:
        r = orc.objective(ev, np.asarray(theta, np.float64), MODEL, size, cost="image_variance", sigma=0, outer_padding=pad,
                          omit_boundary=omit, direction=direction, warp_direction=ref_dir)
        loss += mult * r["loss"]
        grad += mult * r["grad"]
        contrasts.append(orc.variance(r["iwes"]["iwe"], omit, 1, want_grad=False)[0])
        images.append(r["iwes"]["iwe"])
    return loss, grad, contrasts, images


@functools.lru_cache(maxsize=None)
def uniform_reference(shape, theta, n_ref, omit):
    return oracle_sum(uniform_events(shape), theta, SHAPES[shape][0], REFS[n_ref], omit)


def assert_gate(res, grad, ref, label=""):
    loss, g, contrasts = ref[0], ref[1], ref[2]
    res, grad = np.asarray(res, np.float64), np.asarray(grad, np.float64)
    e_loss = abs(res[0] - loss) / abs(loss)
    e_k = max(abs(res[1 + k] - v) / abs(v) for k, v in enumerate(contrasts))
    e_grad = rel_max(grad, g)
    print(f"[deferred stats] {label}: rel err loss {e_loss:.2e} contrasts {e_k:.2e} gradient {e_grad:.2e}")
    assert e_loss <= TOL and e_k <= TOL and e_grad <= TOL, (label, e_loss, e_k, e_grad)


@pytest.mark.parametrize("n_ref", [1, 2, 3])
@pytest.mark.parametrize("omit", [True, False])
@pytest.mark.parametrize("theta", THETAS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_small_shapes_against_the_oracle(shape, theta, omit, n_ref):
    """Zero motion: no exact-cell candidates; sub-pixel motion: every window inside one tile; 12 px: windows across tiles and over the
    border of Omega; 40 px on a 48-px image: most votes leave the image.  Twice per handle: the vote images are double-buffered."""
    size = SHAPES[shape][0]
    h = E.CMaxHandle(size).set_events(uniform_events(shape))
    desc = descriptor(REFS[n_ref], omit)
    ref = uniform_reference(shape, theta, n_ref, omit)
    for rep in range(2):
        res, grad = h.evaluate(desc, np.array(theta))
        assert_gate(res.cpu().numpy(), grad.cpu().numpy(), ref, f"{shape} theta {theta} omit {omit} n_ref {n_ref} #{rep}")


@pytest.mark.parametrize("direction,negate", [("maximize", False), ("minimize", True)])
def test_minimize_and_negate_toggled(direction, negate):
    size, theta = SHAPES["48x64"][0], (12.3, -7.7)
    ev = uniform_events("48x64")
    loss, grad, contrasts, _ = oracle_sum(ev, theta, size, REFS[3], True, direction)
    sign = -1.0 if negate else 1.0  # cmax_objective_t::negate flips loss and gradient, not the contrasts
    h = E.CMaxHandle(size).set_events(ev)
    res, g = h.evaluate(descriptor(REFS[3], True, direction, negate), np.array(theta))
    assert_gate(res.cpu().numpy(), g.cpu().numpy(), (sign * loss, sign * grad, contrasts), f"direction {direction} negate {negate}")


def test_image_without_contrast():
    """Every pixel receives the same integer count at theta = 0: the variance is exactly 0 there and stays tiny at theta = (0.5, 0.5),
    so (sum I^2 - sum I * mu) cancels completely.  The gate's own scale for the loss is the mean square the difference is taken from:
    |loss - oracle| <= 1e-4 max(sum I^2 / npix, |oracle|) -- not a relative error on a quantity that is zero."""
    size, per_pixel = (48, 64), 4
    rr, cc = np.meshgrid(np.arange(size[0]), np.arange(size[1]), indexing="ij")
    n = per_pixel * rr.size
    rng = np.random.default_rng(7)
    ev = np.empty((n, 4))
    ev[:, 0] = np.tile(rr.ravel(), per_pixel)
    ev[:, 1] = np.tile(cc.ravel(), per_pixel)
    ev[:, 2] = np.sort(rng.uniform(0.0, 0.05, n))
    ev[:, 3] = 1.0
    ev[:, :2] = ev[rng.permutation(n), :2]  # (times stay sorted; which pixel fires when is random)
    h = E.CMaxHandle(size).set_events(ev)
    for omit in (True, False):
        desc = descriptor(REFS[1], omit)
        for theta in ((0.0, 0.0), (0.5, 0.5)):
            loss, grad, _, images = oracle_sum(ev, theta, size, REFS[1], omit)
            i0 = 1 if omit else 0
            omega = images[0][i0:size[0] - i0, i0:size[1] - i0]
            scale = max(float((omega ** 2).sum()) / omega.size, abs(loss))
            res, g = h.evaluate(desc, np.array(theta))
            err = abs(res[0].item() - loss)
            print(f"[deferred stats] no contrast, omit {omit}, theta {theta}: loss {res[0].item():.6e} oracle {loss:.6e} |diff| / scale {err / scale:.2e}")
            assert err <= TOL * scale
            if theta == (0.0, 0.0):
                assert float(np.var(omega)) == 0.0  # (the construction: the oracle's image is flat over Omega)
            else:
                assert rel_max(g.cpu().numpy(), grad) <= TOL


def test_sharp_image():
    """Dots at their true motion (bench.py's structured stream, 2 500 dots at 260 x 346, scaled to 200 dots at 48 x 64): pixels of a
    few hundred votes beside empty ones -- nothing cancels, and hundreds of events share a cell."""
    size, n, v = (48, 64), 20_000, (9.0, -6.0)
    ev = E.utils.generate_structured_events(n, size[0], size[1], v, n_dots=200, seed=5)
    h = E.CMaxHandle(size).set_events(ev)
    for theta in (v, (8.6, -5.7)):
        res, g = h.evaluate(descriptor(), np.array(theta))
        assert_gate(res.cpu().numpy(), g.cpu().numpy(), oracle_sum(ev, theta, size), f"sharp image, theta {theta}")


def off_sensor_batch(size, n, seed):
    rng = np.random.default_rng(seed)
    ev = E.utils.generate_events(n, size[0], size[1], 0.0, 0.05, seed=seed + 1)
    out = rng.random(n) < 0.33
    ev[out, 0] = rng.uniform(-25.0, size[0] + 25.0, int(out.sum()))
    ev[out, 1] = rng.uniform(-25.0, size[1] + 25.0, int(out.sum()))
    off = (np.floor(ev[:, 0]) < 0) | (np.floor(ev[:, 0]) >= size[0]) | (np.floor(ev[:, 1]) < 0) | (np.floor(ev[:, 1]) >= size[1])
    return ev, off


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("omit", [True, False])
def test_off_sensor_events_kept_and_dropped(pad, omit):
    """Kept off-sensor events vote wherever they land; what lands outside the image (and, with omit_boundary, on its outermost ring)
    is in neither sum.  The same batch with set_keep_outside(False) is the batch without them."""
    size, theta = (48, 64), (17.0, -21.0)
    ev, off = off_sensor_batch(size, 20_000, 40)
    desc = descriptor(REFS[1], omit)
    h = E.CMaxHandle(size, outer_padding=pad).set_keep_outside(True).set_events(ev)
    assert h.batch_info()["outside"] == int(off.sum()) > 1000
    res, g = h.evaluate(desc, np.array(theta))
    assert_gate(res.cpu().numpy(), g.cpu().numpy(), oracle_sum(ev, theta, size, REFS[1], omit, pad=pad), f"off-sensor kept, pad {pad} omit {omit}")
    # (cmax_set_events takes t_min / t_max over ALL events it is handed, dropped ones included; the oracle sees the survivors only, so the
    # handle is given their extremes -- on uniform events the gradient is a small difference of border terms, and a time base that is
    # off by a few events' spacing shows in it)
    t_kept = ev[~off, 2]
    h2 = E.CMaxHandle(size, outer_padding=pad).set_keep_outside(False).set_events(ev, tmin=t_kept.min(), tmax=t_kept.max(), on_dropped="ignore")
    assert h2.batch_info()["dropped"] == int(off.sum())
    res2, g2 = h2.evaluate(desc, np.array(theta))
    assert_gate(res2.cpu().numpy(), g2.cpu().numpy(), oracle_sum(ev[~off], theta, size, REFS[1], omit, pad=pad), f"off-sensor dropped, pad {pad} omit {omit}")


@pytest.mark.parametrize("pad", [0, 6])
def test_off_sensor_golden_fixture(golden, pad):
    """... and the reference's own numbers for such a batch (tests/golden/outside_sensor.npz)."""
    g = golden("outside_sensor")
    size = tuple(int(v) for v in g["image_size"])
    tag = f"pad{pad}__image_variance__s0"
    h = E.CMaxHandle(size, outer_padding=pad).set_keep_outside(True).set_events(g["events"])
    res, grad = h.evaluate(E.make_descriptor("image_variance", MODEL), g["theta"])
    assert abs(res[0].item() - float(g[tag + "__loss"])) <= TOL * abs(float(g[tag + "__loss"]))
    assert rel_max(grad.cpu().numpy(), g[tag + "__grad"]) <= TOL


def test_clipped_window():
    """theta = (300, -300) on 64 x 96 without time slabs: a segment's bounding box is far beyond the 8192 LDS words, the window is clipped and
    the corners outside it are gathered from global memory -- into the same sums.  (No entry point reads the published window's flag:
    parity only.)"""
    size, n, theta = (64, 96), 20_000, (300.0, -300.0)
    ev = E.utils.generate_events(n, size[0], size[1], 0.0, 0.05, seed=77)
    h = E.CMaxHandle(size).set_events(ev)
    for omit in (True, False):
        res, g = h.evaluate(descriptor(REFS[1], omit), np.array(theta))
        assert_gate(res.cpu().numpy(), g.cpu().numpy(), oracle_sum(ev, theta, size, REFS[1], omit), f"clipped window, omit {omit}")


def test_forms_agree():
    """cmax_objective, cmax_objective_raw + cmax_finalize_raw_host, cmax_objective_host and the middle candidate of a 3-candidate
    cmax_objective_batch fold the same six sums: 1e-12 relative (the order of the atomics differs, so not bit for bit)."""
    size, theta = SHAPES["48x64"][0], (12.3, -7.7)
    h = E.CMaxHandle(size).set_events(uniform_events("48x64"))
    desc = descriptor()
    res_d, grad_d = h.evaluate(desc, np.array(theta))
    res_d, grad_d = res_d.cpu().numpy(), grad_d.cpu().numpy()
    assert_gate(res_d, grad_d, uniform_reference("48x64", theta, 1, True), "device form")
    call, _, finalize = h.prepare_raw(desc, np.array(theta))
    call()
    res_r, grad_r = finalize()
    res_h, grad_h = h.evaluate_host(desc, np.array(theta))
    res_b, grad_b = h.evaluate_batch(desc, np.array([(3.0, 1.0), theta, (-6.5, 2.25)]))
    res_b, grad_b = res_b.cpu().numpy()[1], grad_b.cpu().numpy()[1]
    for name, res, grad in (("raw", res_r, grad_r), ("host", res_h, grad_h), ("batch", res_b, grad_b)):
        e_res = np.abs(res[:2] - res_d[:2]).max() / np.abs(res_d[:2]).max()
        e_grad = rel_max(grad, grad_d)
        print(f"[deferred stats] {name} form vs device form: result {e_res:.2e} gradient {e_grad:.2e}")
        assert e_res <= 1e-12 and e_grad <= 1e-12, (name, e_res, e_grad)


def raw_sums(h, desc, theta):
    """(S1x, S1y, S2x, S2y, sum I, sum I^2) per accumulator line of reference time 0, and the finished (result, grad)."""
    call, raw, finalize = h.prepare_raw(desc, np.array(theta))
    call()
    res, grad = finalize()
    lines = raw.cpu().numpy()[0].reshape(_lib.RAW_LINES, -1)[:, :6]
    return lines, res, grad


def test_interior_and_border_workgroups():
    """S2 (the bilinear difference of 1_Omega) and an event's share of sum I are evaluated only by workgroups whose window touches the
    border of Omega.  Events in the central 16 x 16 pixels: every workgroup is interior -- S2 is exactly 0.0 and sum I is exactly the
    number of events.  Events in the outermost two pixels only: every workgroup is a border one.  Both against the oracle."""
    size, theta, n = SHAPES["48x64"][0], (0.3, -0.2), 20_000
    rng = np.random.default_rng(9)
    t = np.sort(rng.uniform(0.0, 0.05, n))
    centre = np.stack([rng.integers(16, 32, n), rng.integers(24, 40, n), t, np.ones(n)], axis=1).astype(np.float64)
    ring_r, ring_c = np.nonzero(np.pad(np.zeros((size[0] - 4, size[1] - 4), bool), 2, constant_values=True))
    pick = rng.integers(0, ring_r.size, n)
    ring = np.stack([ring_r[pick], ring_c[pick], t, np.ones(n)], axis=1).astype(np.float64)
    for omit in (True, False):
        desc = descriptor(REFS[1], omit)
        lines, res, grad = raw_sums(E.CMaxHandle(size).set_events(centre), desc, theta)
        assert np.all(lines[:, 2:4] == 0.0), lines[:, 2:4]
        assert lines[:, 4].sum() == float(n)
        assert_gate(res, grad, oracle_sum(centre, theta, size, REFS[1], omit), f"interior workgroups, omit {omit}")
        lines, res, grad = raw_sums(E.CMaxHandle(size).set_events(ring), desc, theta)
        assert np.any(lines[:, 2:4] != 0.0)
        assert_gate(res, grad, oracle_sum(ring, theta, size, REFS[1], omit), f"border workgroups, omit {omit}")
