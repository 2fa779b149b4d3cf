"""A numpy / scipy restatement of stain2stain_amd.morphology, every value an integer.

  d2_brute / d2_indices   squared distance to the nearest background (or foreground) pixel, FAR where there is none:
                          a brute-force minimum, and the nearest-site indices of scipy's exact transform
  disc, morphology        true discs and the four operations as thresholds of d2
  fill_holes              background components that touch no border line
  boundary                m & ~binary_erosion(m, cross, border_value=0)
  agreement               the pooled boundary distances: max, nearest-rank percentile, sum of isqrt(65536 s), within
"""
import math

import numpy as np
from scipy import ndimage

FAR = 2 ** 31 - 1
CROSS = ndimage.generate_binary_structure(2, 1)
SQUARE = ndimage.generate_binary_structure(2, 2)


def sites_of(mask, to):
    m = np.asarray(mask) != 0
    return ~m if to == "background" else m


def d2_brute(mask, to="background"):
    """int64 [H, W]: the minimum over the sites, one pixel at a time."""
    s = sites_of(mask, to)
    H, W = s.shape
    ys, xs = np.nonzero(s)
    out = np.full((H, W), FAR, np.int64)
    if ys.size == 0:
        return out
    for y in range(H):
        for x in range(W):
            out[y, x] = ((ys - y) ** 2 + (xs - x) ** 2).min()
    return out


def d2_indices(mask, to="background"):
    """int64 [H, W] from the nearest-site indices of scipy.ndimage.distance_transform_edt (exact, no float distance)."""
    s = sites_of(mask, to)
    H, W = s.shape
    if not s.any():
        return np.full((H, W), FAR, np.int64)
    idx = ndimage.distance_transform_edt(~s, return_distances=False, return_indices=True)
    yy, xx = np.mgrid[0:H, 0:W]
    return ((idx[0] - yy).astype(np.int64) ** 2 + (idx[1] - xx).astype(np.int64) ** 2)


def d2(mask, to="background", max_dist=None):
    d = d2_indices(mask, to)
    if max_dist is not None:
        d = np.where(d > math.floor(max_dist * max_dist), FAR, d)
    return d.astype(np.int32)


def d2_batch(masks, to="background", max_dist=None):
    return np.stack([d2(m, to, max_dist) for m in masks])


def r2_of(radius):
    return min(math.floor(radius * radius), FAR - 1)


def disc(radius):
    """The pixels within ``radius`` of the centre: bool [2k+1, 2k+1], k = floor(radius)."""
    k = int(math.floor(radius))
    yy, xx = np.mgrid[-k:k + 1, -k:k + 1]
    return (yy * yy + xx * xx) <= r2_of(radius)


def dilate(mask, radius):
    return (d2_indices(mask, "foreground") <= r2_of(radius)).astype(np.uint8)


def erode(mask, radius):
    return (d2_indices(mask, "background") > r2_of(radius)).astype(np.uint8)


def morphology(mask, op, radius):
    if op == "dilate":
        return dilate(mask, radius)
    if op == "erode":
        return erode(mask, radius)
    if op == "open":
        return dilate(erode(mask, radius), radius)
    if op == "close":
        return erode(dilate(mask, radius), radius)
    raise ValueError(op)


def scipy_dilate(mask, radius):
    return ndimage.binary_dilation(np.asarray(mask) != 0, disc(radius), border_value=0).astype(np.uint8)


def scipy_erode(mask, radius):
    return ndimage.binary_erosion(np.asarray(mask) != 0, disc(radius), border_value=1).astype(np.uint8)


def scipy_morphology(mask, op, radius):
    if op == "dilate":
        return scipy_dilate(mask, radius)
    if op == "erode":
        return scipy_erode(mask, radius)
    if op == "open":
        return scipy_dilate(scipy_erode(mask, radius), radius)
    return scipy_erode(scipy_dilate(mask, radius), radius)


def fill_holes(mask, connectivity=4):
    m = np.asarray(mask) != 0
    lab, n = ndimage.label(~m, CROSS if connectivity == 4 else SQUARE)
    edge = np.unique(np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]]))
    hole = (lab > 0) & ~np.isin(lab, edge)
    return (m | hole).astype(np.uint8)


def boundary(mask):
    m = np.asarray(mask) != 0
    return (m & ~ndimage.binary_erosion(m, CROSS, border_value=0)).astype(np.uint8)


def pooled(pred, target):
    """(S int64, |dP|, |dT|): distances from dP to dT, then from dT to dP."""
    bp, bt = boundary(pred) != 0, boundary(target) != 0
    to_t, to_p = d2_indices(bt, "foreground"), d2_indices(bp, "foreground")
    return np.concatenate([to_t[bp], to_p[bt]]).astype(np.int64), int(bp.sum()), int(bt.sum())


def agreement(pred, target, tolerance=2, percentile=95):
    """One sample: the dict of mask_boundary_agreement as numpy scalars."""
    H, W = np.asarray(pred).shape
    S, n_p, n_t = pooled(pred, target)
    n = n_p + n_t
    tol2 = r2_of(tolerance)
    if n == 0:
        max_d2 = pq = sum_q8 = within = 0
        valid = 0
    elif n_p == 0 or n_t == 0:
        max_d2 = pq = (H - 1) ** 2 + (W - 1) ** 2
        sum_q8, within, valid = n * math.isqrt(65536 * max_d2), 0, 0
    else:
        k = (percentile * n + 99) // 100
        max_d2, pq = int(S.max()), int(np.sort(S)[k - 1])
        sum_q8 = sum(math.isqrt(65536 * int(s)) for s in S)
        within, valid = int((S <= tol2).sum()), 1
    return {"max_d2": np.int32(max_d2), "pq_d2": np.int32(pq), "sum_q8": np.int64(sum_q8), "within": np.int64(within),
            "boundary_pred": np.int64(n_p), "boundary_target": np.int64(n_t), "valid": np.int32(valid),
            "hausdorff": np.sqrt(np.float64(max_d2)), "hd": np.sqrt(np.float64(pq)),
            "assd": np.float64(sum_q8) / np.float64(256 * n) if n else np.float64(0.0),
            "surface_dice": np.float64(within) / np.float64(n) if n else np.float64(1.0)}


def agreement_batch(pred, target, tolerance=2, percentile=95):
    rows = [agreement(p, t, tolerance, percentile) for p, t in zip(pred, target)]
    return {k: np.stack([r[k] for r in rows]) for k in rows[0]}


INT_KEYS = ("max_d2", "pq_d2", "sum_q8", "within", "boundary_pred", "boundary_target", "valid")
F64_KEYS = ("hausdorff", "hd", "assd", "surface_dice")


# ---- patterns ---------------------------------------------------------------------------------------------------------
def bernoulli(shape, p, seed):
    return (np.random.default_rng(seed).random(shape) < p).astype(np.uint8)


def checkerboard(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return ((yy + xx) & 1).astype(np.uint8)


def stripes(H, W, axis=0):
    yy, xx = np.mgrid[0:H, 0:W]
    return ((yy if axis == 0 else xx) & 1).astype(np.uint8)


def corners(H, W):
    """Four masks with a single foreground pixel in one corner each."""
    out = np.zeros((4, H, W), np.uint8)
    out[0, 0, 0] = out[1, 0, W - 1] = out[2, H - 1, 0] = out[3, H - 1, W - 1] = 1
    return out


def discs(H, W, items):
    """items: (cy, cx, r) triples."""
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), np.uint8)
    for cy, cx, r in items:
        m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 1
    return m


def two_discs(H, W):
    return discs(H, W, [(H * 0.3, W * 0.3, min(H, W) * 0.2), (H * 0.7, W * 0.65, min(H, W) * 0.15)])


def ring(H, W, cy, cx, r_out, r_in):
    m = discs(H, W, [(cy, cx, r_out)])
    m[discs(H, W, [(cy, cx, r_in)]) > 0] = 0
    return m


def patterns(H, W, seed=0):
    """(name, mask) pairs: the patterns every shape is checked on."""
    yield "background", np.zeros((H, W), np.uint8)
    yield "foreground", np.ones((H, W), np.uint8)
    for i, c in enumerate(corners(H, W)):
        yield f"corner {i}", c
    for p in (0.001, 0.3, 0.7, 0.98):
        yield f"bernoulli {p}", bernoulli((H, W), p, seed + int(p * 1000))
    yield "checkerboard", checkerboard(H, W)
    yield "row stripes", stripes(H, W, 0)
    yield "column stripes", stripes(H, W, 1)
    yield "two discs", two_discs(H, W)
