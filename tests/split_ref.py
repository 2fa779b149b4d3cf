"""CPU restatement of stain2stain_amd.split in numpy, vectorised with shifted arrays.  Nothing here
imports the package.

  key     key(p) = d2[p] * 2^31 + (y W + x) as one int64 (d2 < 2^31, H W < 2^31): the lexicographic order of (d2, index)
  ascent  up(p) = the foreground neighbour of largest key if above key(p), else p; roots by pointer doubling
  best    per basin a, the largest (min(d2[p], d2[q]) << 32 | root(q)) over neighbouring pixels of a higher basin
  join    P(a) <= core2 or m 2^20 >= neck_q^2 P(a), neck_q = rint(1024 neck), core2 = floor(min_core^2); one round
  number  parts by first raster pixel, filter by min_area, renumber; the tables as objects_ref.components
"""
import math

import numpy as np
from scipy import ndimage

import morphology_ref as MR
import objects_ref as O

FAR = MR.FAR
KEYS = ("labels", "count", "basins", "kept_pixels", "largest", "size_hist")
TABLE = ("area", "bbox", "centroid")


def offsets(connectivity):
    assert connectivity in (4, 8)
    return [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if (dy or dx) and (connectivity == 8 or dy == 0 or dx == 0)]


def shifted(a, dy, dx, fill):
    """out[y, x] = a[y + dy, x + dx], ``fill`` outside the image."""
    H, W = a.shape
    out = np.full_like(a, fill)
    ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
    xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
    out[yd, xd] = a[ys, xs]
    return out


def chase(ptr):
    """The fixed point of a flat pointer array from every element, by doubling."""
    while True:
        nxt = ptr[ptr]
        if np.array_equal(nxt, ptr):
            return ptr
        ptr = nxt


def neck_q_of(neck):
    return int(round(neck * 1024))


def core2_of(min_core):
    return min(math.floor(min_core * min_core), FAR - 1)


def basins_of(d2, connectivity=8):
    """(root int64 [H, W] = the raster index of every foreground pixel's root, -1 on the background; key int64 [H, W])."""
    d = np.asarray(d2).astype(np.int64)
    H, W = d.shape
    fg = d > 0
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    key = np.where(fg, (d << 31) | idx, -1)
    best, up = key.copy(), idx.copy()
    for dy, dx in offsets(connectivity):
        nk, ni = shifted(key, dy, dx, -1), shifted(idx, dy, dx, -1)
        better = fg & (nk > best)
        best, up = np.where(better, nk, best), np.where(better, ni, up)
    root = chase(up.ravel()).reshape(H, W)
    return np.where(fg, root, -1), key


def parts_of(d2, connectivity=8, neck=0.75, min_core=0.0):
    """(part int64 [H, W] = the raster index of the root of every foreground pixel's part, -1 on the background; the
    number of basins)."""
    d = np.asarray(d2).astype(np.int64)
    H, W = d.shape
    root, key = basins_of(d, connectivity)
    fg = root >= 0
    flat_key, flat_d = key.ravel(), d.ravel()
    best = np.zeros(H * W, np.int64)
    for dy, dx in offsets(connectivity):
        rq, dq = shifted(root, dy, dx, -1), shifted(d, dy, dx, 0)
        pair = fg & (rq >= 0) & (rq != root)
        pair[pair] = flat_key[rq[pair]] > flat_key[root[pair]]
        cand = (np.minimum(d, dq)[pair] << 32) | rq[pair]
        np.maximum.at(best, root[pair], cand)
    roots = np.flatnonzero(root.ravel() == np.arange(H * W))
    link = np.arange(H * W, dtype=np.int64)
    m, b, P = best[roots] >> 32, best[roots] & 0xFFFFFFFF, flat_d[roots]
    nq = neck_q_of(neck)
    join = (best[roots] > 0) & ((P <= core2_of(min_core)) | ((m << 20) >= nq * nq * P))
    link[roots[join]] = b[join]
    top = chase(link)
    part = np.where(fg, top[np.where(fg, root, 0)], -1)
    return part, len(roots)


def number(part, min_area=1):
    """(labels int32, count, areas int64 [count]): parts in raster order of their first pixel, filtered, renumbered."""
    flat = part.ravel()
    fg = flat >= 0
    ids, first, inv, area = np.unique(flat[fg], return_index=True, return_inverse=True, return_counts=True)
    order = np.argsort(first, kind="stable")                   # np.unique's first occurrences are raster positions
    keep = area[order] >= min_area
    num_sorted = np.zeros(len(ids), np.int32)
    num_sorted[keep] = np.arange(1, int(keep.sum()) + 1, dtype=np.int32)
    num = np.zeros(len(ids), np.int32)
    num[order] = num_sorted
    lab = np.zeros(flat.shape, np.int32)
    lab[fg] = num[inv]
    return lab.reshape(part.shape), int(keep.sum()), area[order][keep].astype(np.int64)


def tables(lab, n, area, max_objects=None):
    """The per-sample statistics and the optional table of objects_ref.components, from a numbered label image."""
    hist = np.zeros(32, np.int64)
    if n:
        np.add.at(hist, np.floor(np.log2(area)).astype(np.int64), 1)
    out = {"labels": lab, "count": np.int32(n), "kept_pixels": np.int64(area.sum()),
           "largest": np.int32(area.max() if n else 0), "size_hist": hist}
    if max_objects is not None:
        M = max_objects
        ys, xs = np.nonzero(lab)
        k = lab[ys, xs].astype(np.int64) - 1
        t = min(n, M)
        tab_area, bbox, cen = np.zeros(M, np.int32), np.zeros((M, 4), np.int32), np.zeros((M, 2), np.float32)
        for j in range(t):
            sel = k == j
            y, x = ys[sel], xs[sel]
            tab_area[j] = area[j]
            bbox[j] = (y.min(), x.min(), y.max() + 1, x.max() + 1)
            cen[j] = (np.float32(np.float64(y.sum()) / np.float64(area[j])), np.float32(np.float64(x.sum()) / np.float64(area[j])))
        out.update(area=tab_area, bbox=bbox, centroid=cen)
    return out


def split_d2(d2, connectivity=8, neck=0.75, min_core=0.0, min_area=1, max_objects=None):
    """What split_objects returns for one 2-D distance map, as numpy arrays (without "d2")."""
    part, nb = parts_of(d2, connectivity, neck, min_core)
    lab, n, area = number(part, min_area)
    out = tables(lab, n, area, max_objects)
    out["basins"] = np.int32(nb)
    return out


def split(mask, connectivity=8, neck=0.75, min_core=0.0, min_area=1, max_objects=None):
    return split_d2(MR.d2(mask), connectivity, neck, min_core, min_area, max_objects)


def batch(masks, **kw):
    per = [split(m, **kw) for m in masks]
    return {k: np.stack([p[k] for p in per]) for k in per[0]}


def check_properties(mask, lab, connectivity):
    """The three properties that follow from the definition, for labels computed with min_area = 1."""
    m = np.asarray(mask) != 0
    assert np.array_equal(lab > 0, m)
    comp, _ = ndimage.label(m, structure=O.structure(connectivity))
    n = int(lab.max())
    if n == 0:
        return
    # every part is connected: labelling the parts one connectivity class at a time finds exactly one piece each
    pieces = sum(ndimage.label(lab == k, structure=O.structure(connectivity))[1] for k in range(1, n + 1))
    assert pieces == n
    # every part lies inside one component
    lo = ndimage.minimum(comp, lab, index=np.arange(1, n + 1))
    hi = ndimage.maximum(comp, lab, index=np.arange(1, n + 1))
    assert np.array_equal(lo, hi) and lo.min() > 0


# ---- the test patterns ------------------------------------------------------------------------------------------------
def disc(H, W, cy, cx, r):
    return MR.discs(H, W, [(cy, cx, r)])


def disc_pair(distance, r=12, H=64, W=64):
    """Two discs of radius ``r`` on row 32 whose centres are ``distance`` apart."""
    left = 32 - (distance + 1) // 2
    return MR.discs(H, W, [(32, left, r), (32, left + distance, r)])


def three_discs(r=10):
    """Three mutually touching discs."""
    return MR.discs(64, 64, [(20, 20, r), (20, 38, r), (36, 29, r)])


def rectangle(h=12, w=40, H=64, W=64):
    m = np.zeros((H, W), np.uint8)
    m[(H - h) // 2:(H - h) // 2 + h, (W - w) // 2:(W - w) // 2 + w] = 1
    return m


def rotated_rectangle(h=10, w=44, degrees=33, H=64, W=64):
    """An h x w rectangle turned about the image centre, nearest-neighbour: a plateau ridge with bumps along its sides."""
    return (ndimage.rotate(rectangle(h, w, H, W), degrees, reshape=False, order=0) > 0).astype(np.uint8)


def ellipse(H=64, W=64, cy=32, cx=32, a_y=10.0, a_x=700.0 ** 0.5):
    yy, xx = np.mgrid[0:H, 0:W]
    return (((yy - cy) ** 2 / (a_y * a_y) + (xx - cx) ** 2 / (a_x * a_x)) <= 1.0).astype(np.uint8)


def smoothed_noise(N=96, seed=0, sigma=3.0, level=0.02):
    """A field of blobs that touch and merge: Gaussian-smoothed white noise above ``level``."""
    return (ndimage.gaussian_filter(np.random.default_rng(seed).standard_normal((N, N)), sigma) > level).astype(np.uint8)
