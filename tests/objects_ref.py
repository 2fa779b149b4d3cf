"""CPU restatement of stain2stain_amd.objects with scipy.ndimage.label and numpy.  Nothing here imports
the package.

  object     a maximal 4- (cross) or 8-connected (3 x 3 ones) set of foreground pixels
  numbering  1..count in raster order of each object's first pixel: what scipy.ndimage.label gives, pinned here on small
             masks by a pure-Python flood fill (``flood_label``) that numbers that way by construction
  filter     objects of fewer than ``min_area`` pixels are dropped and the rest renumbered in the same order
Everything is an integer except the centroid, fp32(double(sum) / double(area)), and the ratios, each one correctly
rounded division of exact integers.
"""
import numpy as np
from scipy import ndimage


def structure(connectivity):
    assert connectivity in (4, 8)
    return np.ones((3, 3), dtype=bool) if connectivity == 8 else ndimage.generate_binary_structure(2, 1)


def flood_label(mask, connectivity):
    """Labels of a small 2-D mask by a flood fill started at every unlabelled foreground pixel in raster order."""
    mask = np.asarray(mask) != 0
    H, W = mask.shape
    nb = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    lab, n = np.zeros((H, W), np.int32), 0
    for y, x in zip(*np.nonzero(mask)):                    # np.nonzero walks in raster order
        if lab[y, x]:
            continue
        n, stack = n + 1, [(y, x)]
        lab[y, x] = n
        while stack:
            cy, cx = stack.pop()
            for dy, dx in nb:
                yy, xx = cy + dy, cx + dx
                if 0 <= yy < H and 0 <= xx < W and mask[yy, xx] and not lab[yy, xx]:
                    lab[yy, xx] = n
                    stack.append((yy, xx))
    return lab, n


def label(mask, connectivity=8, min_area=1):
    """(labels int32 [H, W], count, areas int64 [count]) of one 2-D mask: label, filter, renumber."""
    lab, n = ndimage.label(np.asarray(mask) != 0, structure=structure(connectivity))
    area = np.bincount(lab.ravel(), minlength=n + 1)
    keep = area >= min_area
    keep[0] = False
    number = np.zeros(n + 1, np.int32)
    number[keep] = np.arange(1, int(keep.sum()) + 1, dtype=np.int32)     # scipy's order is kept
    return number[lab].astype(np.int32), int(keep.sum()), area[keep].astype(np.int64)


def components(mask, connectivity=8, min_area=1, max_objects=None):
    """What label_components returns for one 2-D mask, as numpy arrays."""
    lab, n, area = label(mask, connectivity, min_area)
    hist = np.zeros(32, np.int64)
    if n:
        np.add.at(hist, np.floor(np.log2(area)).astype(np.int64), 1)
    out = {"labels": lab, "count": np.int32(n), "kept_pixels": np.int64(area.sum()),
           "largest": np.int32(area.max() if n else 0), "size_hist": hist}
    if max_objects is not None:
        M = max_objects
        ys, xs = np.nonzero(lab)
        k = lab[ys, xs].astype(np.int64) - 1
        big = np.iinfo(np.int32).max
        y0, x0 = np.full(max(n, 1), big, np.int64), np.full(max(n, 1), big, np.int64)
        y1, x1 = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64)
        np.minimum.at(y0, k, ys)
        np.minimum.at(x0, k, xs)
        np.maximum.at(y1, k, ys + 1)
        np.maximum.at(x1, k, xs + 1)
        sy = np.zeros(max(n, 1), np.int64)
        sx = np.zeros(max(n, 1), np.int64)
        np.add.at(sy, k, ys)
        np.add.at(sx, k, xs)
        t = min(n, M)
        tab_area, bbox = np.zeros(M, np.int32), np.zeros((M, 4), np.int32)
        cen = np.zeros((M, 2), np.float32)
        tab_area[:t] = area[:t]
        bbox[:t] = np.stack([y0, x0, y1, x1], axis=1)[:t]
        a = area[:t].astype(np.float64)
        cen[:t, 0] = (sy[:t].astype(np.float64) / a).astype(np.float32)
        cen[:t, 1] = (sx[:t].astype(np.float64) / a).astype(np.float32)
        out.update(area=tab_area, bbox=bbox, centroid=cen)
    return out


def batch(masks, connectivity=8, min_area=1, max_objects=None):
    """``components`` of every sample of [B, H, W], stacked."""
    per = [components(m, connectivity, min_area, max_objects) for m in masks]
    return {k: np.stack([p[k] for p in per]) for k in per[0]}


def touched(lab_pred, lab_target):
    """(prediction objects that share a pixel with a target object, target objects that share one with a prediction)."""
    both = (lab_pred > 0) & (lab_target > 0)
    return len(np.unique(lab_pred[both])), len(np.unique(lab_target[both]))


def agreement(lab_pred, n_pred, lab_target, n_target):
    """The object-level scores of one sample; the ratios as float32 of a double quotient."""
    hp, ht = touched(lab_pred, lab_target)
    rec = ht / n_target if n_target else (1.0 if n_pred == 0 else 0.0)
    pre = hp / n_pred if n_pred else (1.0 if n_target == 0 else 0.0)
    f1 = ((2.0 * pre) * rec) / (pre + rec) if pre + rec > 0 else 0.0
    return {"count_pred": np.int32(n_pred), "count_target": np.int32(n_target),
            "count_abs_err": np.int32(abs(n_pred - n_target)), "recall": np.float32(rec), "precision": np.float32(pre),
            "f1": np.float32(f1)}


# ---- the test patterns ------------------------------------------------------------------------------------------------
def serpentine(H, W):
    """Even rows full, odd rows one pixel at alternately the right and the left end: one one-pixel-wide snake."""
    m = np.zeros((H, W), np.uint8)
    m[0::2] = 1
    m[1::4, W - 1] = 1
    m[3::4, 0] = 1
    return m


def checkerboard(H, W):
    return ((np.add.outer(np.arange(H), np.arange(W)) & 1) == 0).astype(np.uint8)


def diagonals(N):
    return np.eye(N, dtype=np.uint8), np.ascontiguousarray(np.eye(N, dtype=np.uint8)[:, ::-1])


def bernoulli(shape, p, seed):
    return (np.random.default_rng(seed).random(shape) < p).astype(np.uint8)
