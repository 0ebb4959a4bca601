"""TEST INFRASTRUCTURE ONLY: the fp64 value the per-patch translation search (k_search_range / k_patch_search,
csrc/cmax_search_kernels.h) is held to.  numpy + scipy, independent of oracle/cmax_oracle.c:
    crop        x0 <= x < x1 and y0 <= y < y1 on the (possibly fractional) coordinates, shifted to the patch origin
    warp        x' = x + theta (t - t_mid), t_mid the middle of the PATCH'S OWN time span; a zero span normalises by 0: no vote lands
    vote        cell floor(x' + 1e-8), fractions from x', four corners by np.add.at; corners outside the patch image are dropped
    blur        scipy.ndimage.gaussian_filter(img, sigma) itself (mode 'reflect', truncate 4): the call the reference makes
    cost        mean(gx^2 + gy^2) of Sobel / 8 on np.pad(mode='reflect') (OpenCV's BORDER_REFLECT_101), edge padding on a one-pixel axis
Anchored to tests/golden/patch_search.npz and to oracle.patch_search by tests/test_patch_reference.py."""
import numpy as np
from scipy.ndimage import gaussian_filter


def crop(events, box):
    x0, x1, y0, y1 = (int(v) for v in box)
    ev = np.asarray(events, dtype=np.float64)
    keep = (ev[:, 0] >= x0) & (ev[:, 0] < x1) & (ev[:, 1] >= y0) & (ev[:, 1] < y1)
    out = ev[keep].copy()
    out[:, 0] -= x0
    out[:, 1] -= y0
    return out


def vote(x, y, size):
    h, w = int(size[0]), int(size[1])
    img = np.zeros(h * w)
    ok = np.isfinite(x) & np.isfinite(y)
    x, y = x[ok], y[ok]
    r0, c0 = np.floor(x + 1e-8), np.floor(y + 1e-8)
    a, b = x - r0, y - c0
    r0, c0 = r0.astype(np.int64), c0.astype(np.int64)
    for dr, dc, wgt in ((0, 0, (1 - a) * (1 - b)), (1, 0, a * (1 - b)), (0, 1, (1 - a) * b), (1, 1, a * b)):
        r, c = r0 + dr, c0 + dc
        inside = (r >= 0) & (r < h) & (c >= 0) & (c < w)
        np.add.at(img, r[inside] * w + c[inside], wgt[inside])
    return img.reshape(h, w)


def gradmag(img):
    p = img
    for axis in (0, 1):  # reflect-101 per axis; a one-pixel axis has nothing to reflect: its single line is repeated
        p = np.pad(p, [(1, 1) if k == axis else (0, 0) for k in (0, 1)], mode="reflect" if img.shape[axis] > 1 else "edge")
    gc = ((p[:-2, 2:] - p[:-2, :-2]) + 2.0 * (p[1:-1, 2:] - p[1:-1, :-2]) + (p[2:, 2:] - p[2:, :-2])) / 8.0
    gr = ((p[2:, :-2] - p[:-2, :-2]) + 2.0 * (p[2:, 1:-1] - p[:-2, 1:-1]) + (p[2:, 2:] - p[:-2, 2:])) / 8.0
    return float(np.mean(gc * gc + gr * gr))


def small_patch_gm(events, box, patch_image_size, theta, sigma):
    """-> (gradient magnitude of the patch image, events in the box).  theta None: the un-warped image."""
    ev = crop(events, box)
    x, y = ev[:, 0], ev[:, 1]
    if theta is not None and len(ev):
        lo, hi = ev[:, 2].min(), ev[:, 2].max()
        if hi > lo:
            d = ev[:, 2] - (lo + 0.5 * (hi - lo))
            x, y = x + float(theta[0]) * d, y + float(theta[1]) * d
        else:
            x = y = np.full(len(ev), np.nan)
    img = vote(x, y, patch_image_size)
    if sigma > 0:
        img = gaussian_filter(img, sigma)
    return gradmag(img), len(ev)


def patch_search(events, boxes, patch_image_size, candidates, sigma):
    """-> (loss [n_patch, n_cand] = gm[:, -1:] / gm[:, :-1], gm [n_patch, n_cand + 1], count [n_patch])."""
    boxes = np.asarray(boxes).reshape(-1, 4)
    cands = np.asarray(candidates, dtype=np.float64).reshape(len(boxes), -1, 2)
    gm = np.zeros((len(boxes), cands.shape[1] + 1))
    count = np.zeros(len(boxes), dtype=np.int64)
    for p, box in enumerate(boxes):
        for c in range(cands.shape[1]):
            gm[p, c], _ = small_patch_gm(events, box, patch_image_size, cands[p, c], sigma)
        gm[p, -1], count[p] = small_patch_gm(events, box, patch_image_size, None, sigma)
    with np.errstate(divide="ignore", invalid="ignore"):
        loss = gm[:, -1:] / gm[:, :-1]
    return loss, gm, count
