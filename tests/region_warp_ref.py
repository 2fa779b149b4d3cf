"""CPU restatement of stain2stain_amd.warp in numpy: the dense displacement of a shift field, the
image and mask sampling through it, and the cleaning of a measured shift field.  Nothing here imports the package.

Everything is integer arithmetic (displacements in 1/16 pixel, int64 intermediates), so fields, ``kept``, the statistics
and every warped byte must be bit-equal to the kernels'.
"""
import numpy as np

SUB = 16
MAX_SHIFT = 1024
MAX_CELLS = 65536
MAX_CELL = 16384


def axis(n, cell, G):
    """(g0, g1, w) int64 [n] of one axis: node g is the centre of cell g; in doubled coordinates span = 2 cell,
    u = 2 p + 1 - cell.  Positions outside the node centres take the nearest node's value."""
    p = np.arange(n, dtype=np.int64)
    if G < 2:
        z = np.zeros(n, np.int64)
        return z, z.copy(), z.copy()
    span = 2 * cell
    u = 2 * p + 1 - cell
    g0 = np.clip(u // span, 0, G - 2)                          # numpy's // is the floor
    return g0, g0 + 1, np.clip(u - g0 * span, 0, span)


def dense(D, H, W, cell, max_shift=64):
    """int64 [H, W, 2]: the field D int [Gy, Gx, 2] (1/16 px) interpolated to every pixel and clamped."""
    D = np.asarray(D).astype(np.int64)
    Gy, Gx = D.shape[:2]
    assert D.shape == (Gy, Gx, 2) and Gy == H // cell and Gx == W // cell and Gy >= 1 and Gx >= 1
    span = 2 * cell
    y0, y1, wy = axis(H, cell, Gy)
    x0, x1, wx = axis(W, cell, Gx)
    wy, wx = wy[:, None, None], wx[None, :, None]
    top = (span - wx) * D[y0][:, x0] + wx * D[y0][:, x1]
    bot = (span - wx) * D[y1][:, x0] + wx * D[y1][:, x1]
    num = (span - wy) * top + wy * bot
    d = (num + span * span // 2) // (span * span)
    return np.clip(d, -SUB * max_shift, SUB * max_shift)


def _taps(T, r, c, fill):
    H, W = T.shape[:2]
    ok = (r >= 0) & (r < H) & (c >= 0) & (c < W)
    v = T[np.clip(r, 0, H - 1), np.clip(c, 0, W - 1)].astype(np.int64)
    v[~ok] = fill
    return v


def warp(T, D, cell, max_shift=64, fill=255):
    """uint8 [H, W, 3] (bilinear in 1/16 px) or uint8 [H, W] (nearest) through the field D."""
    T = np.asarray(T)
    H, W = T.shape[:2]
    d = dense(D, H, W, cell, max_shift)
    sy = SUB * np.arange(H, dtype=np.int64)[:, None] + d[..., 0]
    sx = SUB * np.arange(W, dtype=np.int64)[None, :] + d[..., 1]
    if T.ndim == 2:
        return _taps(T, (sy + 8) >> 4, (sx + 8) >> 4, fill).astype(np.uint8)
    iy, ix, fy, fx = sy >> 4, sx >> 4, (sy & 15)[..., None], (sx & 15)[..., None]
    p00, p01 = _taps(T, iy, ix, fill), _taps(T, iy, ix + 1, fill)
    p10, p11 = _taps(T, iy + 1, ix, fill), _taps(T, iy + 1, ix + 1, fill)
    out = ((16 - fy) * ((16 - fx) * p00 + fx * p01) + fy * ((16 - fx) * p10 + fx * p11) + 128) >> 8
    return out.astype(np.uint8)


def shifted(T, dy, dx, fill):
    """``shift_tiles`` of one image or mask: out[y, x] = T[y + dy, x + dx] inside, ``fill`` outside."""
    T = np.asarray(T)
    H, W = T.shape[:2]
    out = np.full_like(T, fill)
    ys = [y for y in range(H) if 0 <= y + dy < H]
    xs = [x for x in range(W) if 0 <= x + dx < W]
    if ys and xs:
        out[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] = T[ys[0] + dy:ys[-1] + 1 + dy, xs[0] + dx:xs[-1] + 1 + dx]
    return out


def reliable(valid, score, margin, shift, min_score=0.5, min_margin=0.05, max_shift=64):
    """uint8 [Gy, Gx]: the cells whose measured shift may be trusted."""
    shift = np.asarray(shift).astype(np.int64)
    ok = (np.asarray(valid) == 1) & (np.asarray(score) >= min_score) & (np.asarray(margin) >= min_margin)
    return (ok & (np.abs(shift).max(-1) <= max_shift)).astype(np.uint8)


def _neighbours(gy, gx, Gy, Gx):
    return [(gy + a, gx + b) for a in (-1, 0, 1) for b in (-1, 0, 1)
            if (a or b) and 0 <= gy + a < Gy and 0 <= gx + b < Gx]


def clean(shift, rel, max_dev=2, max_shift=64):
    """(field int32 [Gy, Gx, 2] in 1/16 px, kept uint8 [Gy, Gx], stats int32 [2] = kept cells, fill iterations).
    A cell whose shift exceeds ``max_shift`` is unreliable whatever ``rel`` says."""
    shift = np.asarray(shift).astype(np.int64)
    Gy, Gx = shift.shape[:2]
    rel = (np.asarray(rel) != 0) & (np.abs(shift).max(-1) <= max_shift)
    kept = rel.copy()
    for gy in range(Gy):
        for gx in range(Gx):
            if not rel[gy, gx]:
                continue
            nb = [shift[p] for p in _neighbours(gy, gx, Gy, Gx) if rel[p]]        # the input state
            if len(nb) < 3:
                continue
            k = (len(nb) - 1) // 2
            med = [sorted(int(v[c]) for v in nb)[k] for c in (0, 1)]
            if max(abs(int(shift[gy, gx, 0]) - med[0]), abs(int(shift[gy, gx, 1]) - med[1])) > max_dev:
                kept[gy, gx] = False
    field = np.where(kept[..., None], SUB * shift, 0)
    known = kept.copy()
    its = 0
    if known.any():
        while not known.all():
            nf, nk = field.copy(), known.copy()
            for gy in range(Gy):
                for gx in range(Gx):
                    if known[gy, gx]:
                        continue
                    nb = [field[p] for p in _neighbours(gy, gx, Gy, Gx) if known[p]]   # the previous iteration
                    if nb:
                        n = len(nb)
                        s = np.sum(nb, axis=0)
                        nf[gy, gx] = (2 * s + n) // (2 * n)
                        nk[gy, gx] = True
            field, known = nf, nk
            its += 1
            assert its <= max(Gy, Gx)
    return field.astype(np.int32), kept.astype(np.uint8), np.array([int(kept.sum()), its], np.int32)


def glass_pair():
    """The end-to-end input: a 128 x 192 pair with the planted shift (3, -5) whose cell (1, 1) of the 64-pixel grid is
    glass (255) in both images."""
    import registration_ref as R
    src, tgt = R.pair(128, 192, 21, 3, -5)
    src, tgt = src.copy(), tgt.copy()
    src[64:128, 64:128] = 255
    tgt[64:128, 64:128] = 255
    return src, tgt
