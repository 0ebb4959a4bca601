"""The image-side kernels (csrc/cmax_fused.hip, csrc/cmax_image_kernels.h: vote image -> loss and G = dL/dIWE) against fp64 references on
the table of tests/_image_cases.py: every seam of the 8 x 32 tiles from both sides, padded shapes from 1 x 9 up (below, at and above the
Hp, Wp >= 4 limit of the fused forms), events concentrated along the border, caller-supplied images, and every path an evaluation can
take -- in this process and, for the five switches that are read once per process, in children (tests/_image_worker.py).

Whole-call evaluations are held to the committed oracle (orc.objective), caller-supplied images to tests/_image_ref.py;
tests/test_image_reference.py anchors both without a GPU.  The gate is the project's own, plain:
    loss      |L - L_ref| / |L_ref|                  <= 1e-4
    gradient  max|g - g_ref| / max|g_ref|            <= 1e-4
    image     max|I - I_ref| / max|I_ref|            <= 1e-4     h.last_iwe(k), the image the contrast was evaluated on (blurred when
                                                                 sigma > 0), for every reference time of the row
The worst error of each path is printed when the module is done; measured figures: profiles/image_side_parity.txt.

The deferred 2-DoF variance sums I^2 from fp32 terms, so a flat contrast costs it digits (mean^2 / variance x 2^-24):
tests/test_image_reference.py holds every such row of the table to a quarter of the gate (STATISTICS_BUDGET), and the 2-DoF border batch of
3 x 5 is drawn with another seed for it (_image_cases.RESEED)."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oracle as orc  # noqa: E402

import _image_cases as C  # noqa: E402
import _image_ref as IR  # noqa: E402
from _image_worker import descriptor, handle, images, launches, n_ref  # noqa: E402
from _weight_grad_ref import weight_grad_objective  # noqa: E402

TOL = 1e-4
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_LIMIT_S = 240
WORST = {}  # (path, quantity) -> (error, row)
_REF = {}   # row id -> orc.objective result: computed once, never written to


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.time()
    yield
    for (path, what), (err, where) in sorted(WORST.items()):
        print(f"\nimage-side parity  {path:<20s} {what:<8s} max rel err {err:.2e}  at {where}", end="")
    print(f"\nimage-side parity  the module took {time.time() - t0:.1f} s")


def ids(rows):
    return [c["id"] for c in rows]


def rel_max(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def oracle(c, motion=None, key=None):
    key = key or c["id"]
    if key not in _REF:
        b = C.built(c)
        _REF[key] = orc.objective(b["ev"], b["motion"] if motion is None else motion, c["model"], c["size"], **C.ref_kwargs(c))
    return _REF[key]


def gate(path, where, loss=None, ref_loss=None, grad=None, ref_grad=None, imgs=None, ref_imgs=None):
    """records every error of the row, then asserts all of them"""
    errs = {}
    if loss is not None:
        assert np.isfinite(loss), (path, where, loss)
        errs["loss"] = abs(loss - ref_loss) / abs(ref_loss)
    if grad is not None:
        assert np.isfinite(grad).all(), (path, where)
        errs["gradient"] = rel_max(grad, ref_grad)
    if imgs is not None:
        assert len(imgs) == len(ref_imgs)
        errs["image"] = max(rel_max(a, b) for a, b in zip(imgs, ref_imgs))
    for what, e in errs.items():
        if e >= WORST.get((path, what), (-1.0, None))[0]:
            WORST[path, what] = (e, where)
    assert all(e <= TOL for e in errs.values()), (path, where, errs)
    return errs


def T(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


# ---- whole call ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.PATHS["default"], ids=ids(C.PATHS["default"]))
def test_whole_call_default(c):
    """k_blur_stats_adj_var (iv1); k_stats_gimage_gm / k_blur_stats_gimage_gm (gm, ngm, mfgm); kFoldStatsInside (dense iv0); the deferred
    statistics (2-DoF iv0); k_stats + kFoldScale (normalised).  Below Hp, Wp = 4 eval_plan's k1_sums_ok is false and the same rows take
    the two-kernel forms and k_stats -> kFoldStats.  The border rows hold the mean K1 sums from its votes (RefArgs::musum, band_weight,
    border_weight)."""
    b, ref = C.built(c), oracle(c)
    h = handle(c, b["ev"])
    res, grad = h.evaluate(descriptor(c), b["motion"])
    gate("whole call", c["id"], res[0].item(), ref["loss"], grad.double().cpu().numpy(), ref["grad"], images(h, c), IR.oracle_images(ref, c["cost"]))
    h.close()


@pytest.mark.parametrize("c", C.PATHS["value_only"], ids=ids(C.PATHS["value_only"]))
def test_whole_call_value_only(c):
    """want_grad = False: k_blur_stats_var, k_stats, k_finalize"""
    b, ref = C.built(c), oracle(c)
    h = handle(c, b["ev"])
    res, grad = h.evaluate(descriptor(c), b["motion"], want_grad=False)
    assert grad is None
    gate("value only", c["id"], res[0].item(), ref["loss"], imgs=images(h, c), ref_imgs=IR.oracle_images(ref, c["cost"]))
    h.close()


# ---- vote + finish -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.PATHS["finish"], ids=ids(C.PATHS["finish"]))
def test_vote_then_finish(c):
    """objective_finish(desc, m, objective_vote(desc, m)): no job of K1 is available to the kernels behind it (EvalPlan::whole is false) --
    k_blur_stats_var + k_gimage_blur_adj_var, the fused gradient-magnitude kernels with K3 deriving its own windows, k_stats -> kFoldStats"""
    b, ref = C.built(c), oracle(c)
    h, desc = handle(c, b["ev"]), descriptor(c)
    votes = h.objective_vote(desc, b["motion"])
    assert votes.shape[0] == C.n_slots(c)
    res, grad = h.objective_finish(desc, b["motion"], votes)
    gate("vote + finish", c["id"], res[0].item(), ref["loss"], grad.double().cpu().numpy(), ref["grad"], images(h, c), IR.oracle_images(ref, c["cost"]))
    h.close()


OFFSET_IDS = [f"{p}-{c['id']}" for p, c in C.OFFSETS]


@pytest.mark.parametrize("pattern,c", C.OFFSETS, ids=OFFSET_IDS)
def test_finish_on_a_caller_supplied_image(pattern, c):
    """objective_finish on objective_vote(...) + offset, the one way to hand these kernels an ARBITRARY image: spikes in the corners and on
    the first pixels inside the omitted boundary, a +-1 checkerboard across every tile seam, a smooth ramp with negative values, a
    constant -- 0.25 x to 1 x the vote image's own maximum.  Against _image_ref.objective_from_images."""
    b = C.built(c)
    h, desc = handle(c, b["ev"]), descriptor(c)
    votes = h.objective_vote(desc, b["motion"])
    ref_votes = IR.vote_images(b["ev"], b["motion"], c["model"], c["size"], c["cost"], c["pad"])
    assert rel_max(votes.double().cpu().numpy(), ref_votes) <= TOL
    offs = C.offsets(pattern, c, float(ref_votes.max()))
    loss, grad, imgs = IR.value_grad_images(b["ev"], b["motion"], c["model"], c["size"], offs, **C.ref_kwargs(c))
    supplied = votes + T(np.stack(offs), torch.float32)  # (kept until the images are read: without a blur last_iwe is the caller's buffer)
    res, g = h.objective_finish(desc, b["motion"], supplied)
    gate("finish + " + pattern, c["id"], res[0].item(), loss, g.double().cpu().numpy(), grad, images(h, c), imgs[: n_ref(c)])
    h.close()


# ---- deterministic mode --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.PATHS["deterministic"], ids=ids(C.PATHS["deterministic"]))
def test_deterministic_mode(c):
    """set_deterministic(True): k_blur3, k_stats<., 1024>, k_gimage, k_blur3_adj (finish_gimage: `h->deterministic` -- those launches carry
    no profile bracket, read_profile cannot tell them from the fused ones)"""
    b, ref = C.built(c), oracle(c)
    h = handle(c, b["ev"], deterministic=True)
    res, grad = h.evaluate(descriptor(c), b["motion"])
    gate("deterministic", c["id"], res[0].item(), ref["loss"], grad.double().cpu().numpy(), ref["grad"], images(h, c), IR.oracle_images(ref, c["cost"]))
    res2, grad2 = h.evaluate(descriptor(c), b["motion"])
    assert torch.equal(res[0], res2[0]) and torch.equal(grad, grad2)
    h.close()


# ---- pointwise G through the weight gradient -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.PATHS["weight_grad"], ids=ids(C.PATHS["weight_grad"]))
def test_weight_gradient_reads_G_at_every_pixel(c):
    """evaluate_weight_grad at zero motion with integral sources on EVERY sensor pixel: dL/dw_e is the sum over the reference times of
    G_k[pixel(e)] (plus the un-warped image's term of a normalised cost) -- k_gimage, k_blur3_adj, k_gimage_orig, compared per event,
    i.e. per pixel, with tests/_weight_grad_ref.py.  (1 to 4 events per pixel: one each would give a constant image without contrast.)"""
    ev, zero = C.weight_grad_batch(c)  # (the row's own motion for a normalised cost: at zero motion its derivative vanishes identically)
    ref = weight_grad_objective(ev, zero, c["model"], c["size"], 1.0, **C.ref_kwargs(c))
    assert np.abs(ref["grad_w"]).max() > 0
    h = handle(c, ev)
    res, _, gw = h.evaluate_weight_grad(descriptor(c), zero)
    gate("weight gradient", c["id"], res[0].item(), ref["loss"], gw.double().cpu().numpy(), ref["grad_w"], images(h, c), IR.oracle_images(ref, c["cost"]))
    h.close()


# ---- one handle, several evaluations ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.PATHS["repeated"], ids=ids(C.PATHS["repeated"]))
def test_repeated_evaluations_on_one_handle(c):
    """Four evaluations with different motions on one handle: the double-buffered vote images and musum buffers, the cached un-warped
    statistics.  The third is value-only, so that a clearing job of the launches behind K1 is skipped once."""
    b = C.built(c, repeated=True)
    h, desc = handle(c, b["ev"]), descriptor(c)
    for it, m in enumerate(b["motions"]):
        ref = orc.objective(b["ev"], m, c["model"], c["size"], **C.ref_kwargs(c))
        res, grad = h.evaluate(desc, m, want_grad=it != 2)
        gate("repeated", f"{c['id']} evaluation {it}", res[0].item(), ref["loss"], None if grad is None else grad.double().cpu().numpy(), ref["grad"],
             images(h, c), IR.oracle_images(ref, c["cost"]))
    h.close()


# ---- which kernels ran -----------------------------------------------------------------------------------------------------------------
def test_launch_counts_tell_the_paths_apart():
    """CMaxHandle.read_profile() counts the bracketed launches per class, on a handle of its own (profiling never wraps a compared
    evaluation).  What it cannot tell apart: deterministic mode and the weight gradient (their image kernels carry no bracket), CMAX_NSUB
    (stat_nsub) and CMAX_STAT_SWEEPS (EvalPlan::stat_blocks) change a launch's shape, not its count."""
    def counts(c, call):
        return launches(c, C.built(c)["ev"], call)

    def whole(c, **kw):
        return counts(c, lambda h, desc: h.evaluate(desc, C.built(c)["motion"], **kw))

    def finish(c):
        return counts(c, lambda h, desc: h.objective_finish(desc, C.built(c)["motion"], h.objective_vote(desc, C.built(c)["motion"])))

    big, small = (18, 66), (3, 5)  # (an even pixel count: K1 can clear the flow gradient, which the statistics inside K3 need)
    p = whole(C.case(big, "image_variance@1", True))  # fused_bv: ONE image kernel
    assert (p["stats"], p["gimage"], p["grad"]) == (1, 0, 1), p
    p = whole(C.case(small, "image_variance@1", True))  # k1_sums_ok false below 4: the two-kernel form
    assert (p["stats"], p["gimage"], p["grad"]) == (1, 1, 1), p
    p = finish(C.case(big, "image_variance@1", True))  # no K1 job: the two-kernel form
    assert (p["stats"], p["gimage"]) == (1, 1), p
    p = whole(C.case(big, "image_variance@0", True))  # stats_inside: no statistics launch
    assert (p["stats"], p["gimage"], p["grad"]) == (0, 0, 1), p
    p = whole(C.case(small, "image_variance@0", True))  # k_stats -> kFoldStats
    assert (p["stats"], p["gimage"], p["grad"]) == (1, 0, 1), p
    p = finish(C.case(big, "image_variance@0", True))
    assert (p["stats"], p["gimage"]) == (1, 0), p
    for label in ("gradient_magnitude@0", "gradient_magnitude@1"):  # fused_gm: statistics and G in one launch of the `stats` class
        p = whole(C.case(big, label, True))
        assert (p["stats"], p["gimage"], p["grad"]) == (1, 0, 1), (label, p)
    p = whole(C.case(big, "image_variance@0", True, model="2d-translation"))  # deferred: K3 gathers the statistics
    assert (p["stats"], p["gimage"], p["grad"]) == (0, 0, 1), p
    p = whole(C.case((17, 65), "image_variance@0", True))  # 2 H W no multiple of 4 and a work list that is not group-aligned: a k_stats launch
    assert (p["stats"], p["gimage"], p["grad"]) == (1, 0, 1), p
    p = whole(C.case(big, "image_variance@1", True), want_grad=False)  # value only: k_blur_stats_var, k_finalize, no K3
    assert (p["stats"], p["gimage"], p["grad"], p["finish"]) == (1, 0, 0, 1), p


# ---- the five switches, each in a child process ------------------------------------------------------------------------------------------
_child_failed = []
# what the launch counts of the child's profiled row (18 x 66, single reference time) have to be: (stats, gimage, grad)
CHILD_COUNTS = {"no_fused_blurvar": (1, 1, 1),  # k_blur_stats_var + k_gimage_blur_adj_var where the default has (1, 0, 1)
                "no_stats_inside": (1, 0, 1),   # a k_stats launch where the default has (0, 0, 1)
                "tan2": (1, 0, 0),              # k_tan_stats_var, and no pass over the events for the gradient
                "sweeps1": (0, 0, 1), "sweeps8": (0, 0, 1)}  # the statistics inside K3, whatever the number of sweeps


@pytest.mark.parametrize("child", list(C.CHILDREN))
def test_path_switches_in_a_child_process(child, tmp_path):
    """CMAX_NO_FUSED_BLURVAR=1 (the two-kernel blurred variance with a gradient on the whole call), CMAX_NO_STATS_INSIDE=1 (k_stats ->
    kFoldStats where the default takes kFoldStatsInside), CMAX_TAN2=1 (k_vote_tan2 -> k_tan_stats_var -> k_finish_deferred: 2-DoF plain
    variance, and the normalised variance on its second evaluation, on the border set with votes one row above and one column left of the
    image), CMAX_NSUB=1 / 32 (the accumulator-count extremes of every statistics kernel, with and without a gradient) and
    CMAX_STAT_SWEEPS=1 / 8 (the statistics workgroups inside K3; 27 x 101 has an odd pixel count: unless its work list is group-aligned it keeps its k_stats launch,
    so 7 x 130 runs as well).  Children run one at a time, each under its own time limit; after one that
    died or timed out no further child is started."""
    if _child_failed:
        pytest.fail(f"not started: an earlier child failed ({_child_failed[0]})")
    switches, rows, mode = C.CHILDREN[child]
    env = dict(os.environ)
    for name in C.SWITCHES:
        env.pop(name, None)
    env.update(switches)
    out = str(tmp_path / f"{child}.npz")
    t0 = time.time()
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_image_worker.py"), child, out], env=env, cwd=ROOT, capture_output=True, text=True,
                           timeout=CHILD_LIMIT_S)
    except subprocess.TimeoutExpired as e:
        _child_failed.append(f"{child}: timed out")
        pytest.fail(f"child {child} {switches} exceeded {CHILD_LIMIT_S} s\n{e.stderr}")
    print(f"[image side] child {child} {switches}: {len(rows)} rows, {time.time() - t0:.1f} s")
    if p.returncode != 0:
        _child_failed.append(f"{child}: exit status {p.returncode}")
        pytest.fail(f"child {child} {switches} ended with status {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    got = dict(np.load(out))
    counts = tuple(int(got["profile/" + k]) for k in ("stats", "gimage", "grad"))
    print(f"[image side] child {child}: launches (stats, gimage, grad) = {counts} on {got['profile/id']}")
    failed = []
    for c in rows:
        ref, cid = oracle(c), c["id"]
        ref_imgs = IR.oracle_images(ref, c["cost"])
        try:
            gate("child " + child, cid, float(got[cid + "/loss"]), ref["loss"], got[cid + "/grad"], ref["grad"],
                 [got[f"{cid}/iwe{k}"] for k in range(n_ref(c))], ref_imgs)
            if mode == "both":
                gate("child " + child + " value", cid, float(got[cid + "/vloss"]), ref["loss"], imgs=[got[f"{cid}/viwe{k}"] for k in range(n_ref(c))],
                     ref_imgs=ref_imgs)
        except AssertionError as e:
            failed.append(str(e)[:300])
    assert not failed, (child, len(failed), failed[:10])
    if child in CHILD_COUNTS:
        assert counts == CHILD_COUNTS[child], (child, counts)
