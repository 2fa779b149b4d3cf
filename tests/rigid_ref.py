"""CPU restatement of stain2stain_amd.rigid in numpy int64: the overview maps, the sample positions of
a rigid transform with their clamps, the warp, the inset of the search crops, the search over angles and the
composition with the local field.  The search level and the dense displacement are those of ``registration_ref`` and
``region_warp_ref``, imported unchanged.  Nothing here imports the package: angle tables are arguments (the tests take
them from ``rotation_table``), so libm cannot make the two disagree.

Everything is integer arithmetic, so every byte, shift and transform must be bit-equal to the kernels'; scores are one
float64 division and one square root away from equal integers.
"""
import functools

import numpy as np

import region_warp_ref as Wr
import registration_ref as R

ONE = 1 << 24
LIMITS = (ONE, ONE, 1 << 36, 1 << 36, ONE, ONE)


def overview(u8, w, ds):
    """uint8 [H, W, 3] -> uint8 [H // ds, W // ds]: the block average of the structure byte over whole blocks."""
    f = R.structure(u8, w, 1).astype(np.int64)
    h, wd = f.shape[0] // ds, f.shape[1] // ds
    s = f[:h * ds, :wd * ds].reshape(h, ds, wd, ds).sum((1, 3))
    return ((s + ds * ds // 2) // (ds * ds)).astype(np.uint8)


def clamped(T):
    return tuple(min(max(int(v), -lim), lim) for v, lim in zip(T, LIMITS))


def positions(T, y, x, dy=0, dx=0):
    """(sy, sx) in 1/16 pixel; y, x, dy, dx python ints or int64 arrays that broadcast."""
    c, s, ty, tx, Cy, Cx = clamped(T)
    Uy, Ux = 32 * y + 2 * dy - 16 * Cy, 32 * x + 2 * dx - 16 * Cx
    Vy, Vx = c * Uy - s * Ux, s * Uy + c * Ux
    return ((Vy + (Cy << 28) + ONE) >> 25) + ty, ((Vx + (Cx << 28) + ONE) >> 25) + tx


def warp(img, T, field=None, cell=None, max_shift=64, nearest=None, fill=255):
    """uint8 [H, W, 3] or [H, W] through the transform T and, with ``field``, the dense displacement of 3.22."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    nearest = (img.ndim == 2) if nearest is None else nearest
    y, x = np.arange(H, dtype=np.int64)[:, None], np.arange(W, dtype=np.int64)[None, :]
    dy = dx = 0
    if field is not None:
        d = Wr.dense(field, H, W, cell, max_shift)
        dy, dx = d[..., 0], d[..., 1]
    sy, sx = positions(T, y, x, dy, dx)
    sy, sx = np.broadcast_to(sy, (H, W)), np.broadcast_to(sx, (H, W))
    if nearest:
        return Wr._taps(img, (sy + 8) >> 4, (sx + 8) >> 4, fill).astype(np.uint8)
    iy, ix, fy, fx = sy >> 4, sx >> 4, sy & 15, sx & 15
    if img.ndim == 3:
        fy, fx = fy[..., None], fx[..., None]
    p00, p01 = Wr._taps(img, iy, ix, fill), Wr._taps(img, iy, ix + 1, fill)
    p10, p11 = Wr._taps(img, iy + 1, ix, fill), Wr._taps(img, iy + 1, ix + 1, fill)
    out = ((16 - fy) * ((16 - fx) * p00 + fx * p01) + fy * ((16 - fx) * p10 + fx * p11) + 128) >> 8
    return out.astype(np.uint8)


def inset_ok(tables, h, w, m):
    for T in tables:
        for y in (m, h - 1 - m):
            for x in (m, w - 1 - m):
                sy, sx = positions(T, y, x)
                if not (0 <= sy and sy + 15 <= 16 * (h - 1) and 0 <= sx and sx + 15 <= 16 * (w - 1)):
                    return False
    return True


def inset(tables, h, w):
    """The smallest m >= 0 whose crop corners sample inside the map, all four taps, under every transform."""
    return next(m for m in range((min(h, w) + 1) // 2) if inset_ok(tables, h, w, m))


def overview_transforms(table, h, w):
    return [(int(c), int(s), 0, 0, h - 1, w - 1) for c, s in table]


def register(src, tgt, table, angles, ds=16, radius=32, src_stains="hed", tgt_stains="hdab", stain=0):
    """``register_rigid``: ``table`` int [A, 2] = (cos, sin) in Q24 of ``angles`` (degrees)."""
    a = overview(src, R.weights(src_stains, stain), ds)
    b = overview(tgt, R.weights(tgt_stains, stain), ds)
    h, w = a.shape
    A = len(table)
    Tk = overview_transforms(table, h, w)
    bk = np.stack([warp(b, T, nearest=False, fill=0) for T in Tk])
    m = inset(Tk, h, w)
    lev = R.level(np.stack([a[m:h - m, m:w - m]] * A), bk[:, m:h - m, m:w - m], radius, None, 1)
    valid = lev["valid"] == 1
    out = {"scores": lev["score"], "shifts": lev["shift"], "inset": m, "maps": (a, b, bk), "level": lev,
           "valid": int(valid.any())}
    Cy, Cx = ds * h - 1, ds * w - 1
    if not valid.any():
        out.update(transform=np.array([ONE, 0, 0, 0, Cy, Cx], np.int64), angle_index=-1, angle=0.0,
                   shift=np.zeros(2, np.int32), score=0.0, margin=0.0, angle_margin=0.0)
        return out
    best = lev["score"][valid].max()
    k = min((k for k in range(A) if valid[k] and lev["score"][k] == best), key=lambda k: (abs(angles[k]), angles[k]))
    c, s = int(table[k][0]), int(table[k][1])
    dy, dx = int(lev["shift"][k][0]), int(lev["shift"][k][1])
    ty = (16 * ds * (c * dy - s * dx) + (1 << 23)) >> 24
    tx = (16 * ds * (s * dy + c * dx) + (1 << 23)) >> 24
    far = [lev["score"][i] for i in range(A) if valid[i] and abs(i - k) > 1]
    out.update(transform=np.array([c, s, ty, tx, Cy, Cx], np.int64), angle_index=k, angle=float(angles[k]),
               shift=lev["shift"][k], score=float(best), margin=float(lev["margin"][k]),
               angle_margin=float(best - max(far)) if far else 0.0)
    return out


def shift_field(src, tgt, cell, **register_kwargs):
    """``region_shift_field`` on arrays: one ``registration_ref.register`` batch per row of cells."""
    H, W = src.shape[:2]
    Gy, Gx = H // cell, W // cell
    out = {"shift": np.zeros((Gy, Gx, 2), np.int32), "valid": np.zeros((Gy, Gx), np.int32),
           "score": np.zeros((Gy, Gx)), "margin": np.zeros((Gy, Gx))}
    gap = np.zeros((Gy, Gx))                                   # the lead of every cell's best score over its second
    for gy in range(Gy):
        cells = [np.stack([img[gy * cell:(gy + 1) * cell, gx * cell:(gx + 1) * cell] for gx in range(Gx)])
                 for img in (src, tgt)]
        lev = R.register(cells[0], cells[1], **register_kwargs)
        for k in out:
            out[k][gy] = lev[k]
        gap[gy] = [R.runner_up_gap(sc, (sc.shape[0] - 1) // 2) for sc in lev["scores"]]
    out["gap"] = gap
    return out


def align(src, tgt, table, angles, cell, masks=(), rigid=None, max_shift=64, fill=255, mask_fill=0, min_score=0.5,
          min_margin=0.05, max_dev=2, **register_kwargs):
    """``align_regions``: the rigid stage, the local field against the intermediate, one resampling of the original."""
    rg = register(src, tgt, table, angles, **(rigid or {}))
    T = rg["transform"]
    mid = warp(tgt, T, fill=fill)
    measured = shift_field(src, mid, cell, **register_kwargs)
    rel = Wr.reliable(measured["valid"], measured["score"], measured["margin"], measured["shift"], min_score,
                      min_margin, max_shift)
    field, kept, stats = Wr.clean(measured["shift"], rel, max_dev, max_shift)
    return {"aligned": warp(tgt, T, field, cell, max_shift, fill=fill),
            "masks": [warp(mk, T, field, cell, max_shift, nearest=True, fill=mask_fill) for mk in masks],
            "field": field, "kept": kept, "stats": stats, "score": measured["score"], "transform": T,
            "angle": rg["angle"], "rigid_score": rg["score"], "rigid_valid": rg["valid"], "intermediate": mid,
            "measured": measured}


# ---- planted pairs ---------------------------------------------------------------------------------------------------
PLANTS = [(3.0, (6, -10)), (-5.0, (-12, 4)), (0.0, (0, 0))]
SEARCH_ANGLES = [float(k) for k in range(-6, 7)]
SEARCH = {"ds": 2, "radius": 8}


@functools.lru_cache(maxsize=None)
def base_pair():
    src, tgt = R.pair(192, 192, 3, 0, 0)
    src.setflags(write=False)
    tgt.setflags(write=False)
    return src, tgt


def inverse(T):
    """The transform that undoes T = (c, s, ty, tx, Cy, Cx) up to rounding: the angle negated, t' = -R^T t."""
    c, s, ty, tx, Cy, Cx = (int(v) for v in T)
    return (c, -s, -((c * ty + s * tx + (1 << 23)) >> 24), -((-s * ty + c * tx + (1 << 23)) >> 24), Cy, Cx)


def planted(cs, shift):
    """(src, tgt'): the base pair with its target resampled through the inverse of the rotation ``cs`` = (cos, sin) in
    Q24 about the centre plus ``shift`` pixels, so that the search finds that angle and that translation."""
    src, tgt = base_pair()
    H, W = tgt.shape[:2]
    T = (int(cs[0]), int(cs[1]), 16 * shift[0], 16 * shift[1], H - 1, W - 1)
    moved = warp(tgt, inverse(T), fill=255)
    moved.setflags(write=False)
    return src, moved
