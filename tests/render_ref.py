"""Numpy restatement (int64 throughout) of the rendering definitions of DESIGN.md 3.32 / include/stain2stain_hip.h: the
class and label overlay with its edge rule, the heat map with both node look-ups, the three comparisons, the box
thumbnail, the palette, the colour maps, the heat quantisation and the panel composition.  Written from the definitions,
pixel formulas vectorised over whole arrays; nothing here shares code with the package."""
import numpy as np

QMAX = 65280
PALETTE8 = [(230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180), (70, 240, 240),
            (240, 50, 230)]
ANCHORS = {"gray": [(0, (0, 0, 0)), (255, (255, 255, 255))],
           "heat": [(0, (0, 0, 0)), (85, (255, 0, 0)), (170, (255, 255, 0)), (255, (255, 255, 255))],
           "blue_red": [(0, (0, 0, 255)), (128, (255, 255, 255)), (255, (255, 0, 0))]}


def mix(b, c, a):
    b, c, a = np.asarray(b, np.int64), np.asarray(c, np.int64), np.asarray(a, np.int64)
    return (b * (256 - a) + c * a + 128) >> 8


def palette():
    p = np.zeros((256, 3), np.int64)
    for k in range(1, 256):
        p[k] = PALETTE8[(k - 1) % 8]
    return p.astype(np.uint8)


def colormap(name):
    anchors = ANCHORS[name]
    out = np.zeros((256, 3), np.int64)
    for (i0, c0), (i1, c1) in zip(anchors, anchors[1:]):
        for i in range(i0, i1 + 1):
            for ch in range(3):
                out[i, ch] = (c0[ch] * (i1 - i) + c1[ch] * (i - i0) + (i1 - i0) // 2) // (i1 - i0)
    return out.astype(np.uint8)


# ---- classes and labels ---------------------------------------------------------------------------------------------------
def identity_and_index(mask):
    """(id, k) int64 of a uint8 / bool class mask or an int32 label image."""
    m = np.asarray(mask)
    if m.dtype == np.int32:
        L = m.astype(np.int64)
        return np.maximum(L, 0), np.where(L <= 0, 0, (L - 1) % 255 + 1)
    m = m.astype(np.int64)
    return m, m


def edges(ident, r):
    """bool [H, W]: id != 0 and some offset with 1 <= |dy| + |dx| <= r leaves the region or meets another identity."""
    ident = np.asarray(ident, np.int64)
    H, W = ident.shape
    edge = np.zeros((H, W), bool)
    if r < 1:
        return edge
    pad = np.full((H + 2 * r, W + 2 * r), -1, np.int64)                  # -1: outside, never an identity
    pad[r:r + H, r:r + W] = ident
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if 1 <= abs(dy) + abs(dx) <= r:
                edge |= pad[r + dy:r + dy + H, r + dx:r + dx + W] != ident
    return edge & (ident != 0)


def render_classes(base, mask, pal=None, fill_alpha=None, r=1, edge_alpha=256, edge_rgb=None, alpha=96):
    base = np.asarray(base).astype(np.int64)
    pal = (palette() if pal is None else np.asarray(pal)).astype(np.int64)
    fa = np.array([0] + [alpha] * 255, np.int64) if fill_alpha is None else np.asarray(fill_alpha, np.int64)
    ident, k = identity_and_index(mask)
    e = edges(ident, r)
    colour = pal[k]
    a = fa[k]
    if edge_rgb is not None:
        colour = np.where(e[..., None], np.asarray(edge_rgb, np.int64)[None, None, :], colour)
    a = np.where(e, edge_alpha, a)
    return mix(base, colour, a[..., None]).astype(np.uint8)


# ---- heat -------------------------------------------------------------------------------------------------------------
def quantize(values, lo=0.0, hi=1.0):
    scale = float(QMAX) / (float(hi) - float(lo))
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.asarray(values).astype(np.float64) - float(lo)
        t = np.floor(t * scale + 0.5)
    t = np.where(np.isnan(t), 0.0, t)
    return np.clip(t, 0.0, float(QMAX)).astype(np.int32)


def _axis(n, G, cell):
    """(g0, g1, w) int64 [n] of the doubled-coordinate interpolation along one axis."""
    p = np.arange(n, dtype=np.int64)
    span = 2 * cell
    if G == 1:
        z = np.zeros(n, np.int64)
        return z, z, z
    u = 2 * p + 1 - cell
    g0 = np.clip(u // span, 0, G - 2)                                    # numpy's // floors
    return g0, g0 + 1, np.clip(u - g0 * span, 0, span)


def heat_index(Q, H, W, cell, smooth):
    Q = np.asarray(Q).astype(np.int64)
    Gy, Gx = Q.shape
    if smooth:
        span = 2 * cell
        y0, y1, wy = _axis(H, Gy, cell)
        x0, x1, wx = _axis(W, Gx, cell)
        wy, wx = wy[:, None], wx[None, :]
        top = (span - wx) * Q[y0][:, x0] + wx * Q[y0][:, x1]
        bot = (span - wx) * Q[y1][:, x0] + wx * Q[y1][:, x1]
        num = (span - wy) * top + wy * bot
        d = (num + span * span // 2) // (span * span)
    else:
        gy = np.minimum(np.arange(H) // cell, Gy - 1)
        gx = np.minimum(np.arange(W) // cell, Gx - 1)
        d = Q[gy][:, gx]
    d = np.clip(d, 0, QMAX)
    return (d + 128) >> 8


def render_heat(base, Q, cell, lut, alpha=128, min_index=0, smooth=True):
    base = np.asarray(base).astype(np.int64)
    H, W = base.shape[:2]
    idx = heat_index(Q, H, W, cell, smooth)
    on = idx >= min_index
    out = mix(base, np.asarray(lut).astype(np.int64)[idx], alpha)
    return np.where(on[..., None], out, base).astype(np.uint8)


# ---- compare ----------------------------------------------------------------------------------------------------------
def compare(a, b, mode, cell=64, alpha=128, gain=4):
    a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    H, W = a.shape[:2]
    if mode in (0, "checker"):
        odd = ((np.arange(H)[:, None] // cell + np.arange(W)[None, :] // cell) & 1) == 1
        return np.where(odd[..., None], b, a).astype(np.uint8)
    if mode in (1, "blend"):
        return mix(a, b, alpha).astype(np.uint8)
    return np.minimum(255, np.abs(a - b) * gain).astype(np.uint8)


# ---- thumbnail --------------------------------------------------------------------------------------------------------
def box_down(img, f):
    img = np.asarray(img)
    H, W = img.shape[:2]
    Ho, Wo = -(-H // f), -(-W // f)
    out = np.zeros((Ho, Wo) + img.shape[2:], np.int64)
    for Y in range(Ho):
        for X in range(Wo):
            block = img[Y * f:min(H, (Y + 1) * f), X * f:min(W, (X + 1) * f)].astype(np.int64)
            n = block.shape[0] * block.shape[1]
            if img.ndim == 3:
                out[Y, X] = (2 * block.reshape(n, -1).sum(0) + n) // (2 * n)
            else:
                out[Y, X] = block.max()
    return out.astype(np.uint8)


def box_down_fast(img, f):
    """The same by cumulative sums (images) / reduceat (masks): for the larger shapes of the GPU tests."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    ys, xs = np.arange(0, H, f), np.arange(0, W, f)
    if img.ndim == 2:
        return np.maximum.reduceat(np.maximum.reduceat(img, ys, 0), xs, 1).astype(np.uint8)
    s = np.add.reduceat(np.add.reduceat(img.astype(np.int64), ys, 0), xs, 1)
    n = (np.minimum(ys + f, H) - ys)[:, None] * (np.minimum(xs + f, W) - xs)[None, :]
    return ((2 * s + n[..., None]) // (2 * n[..., None])).astype(np.uint8)


# ---- panels -------------------------------------------------------------------------------------------------------------
def compose(images, cols=None, gap=8, fill=255):
    n = len(images)
    cols = n if cols is None else min(cols, n)
    rows = -(-n // cols)
    H, W = images[0].shape[:2]
    out = np.full((rows * H + (rows - 1) * gap, cols * W + (cols - 1) * gap) + images[0].shape[2:], fill, np.uint8)
    for i, im in enumerate(images):
        y, x = (i // cols) * (H + gap), (i % cols) * (W + gap)
        out[y:y + H, x:x + W] = im
    return out


# ---- synthetic inputs -------------------------------------------------------------------------------------------------
def random_region(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def random_labels(H, W, seed, special=True):
    """int32 [H, W]: blobs of a few labels on background, with negatives, 0, 255, 256 and 2^31 - 1 among them."""
    rng = np.random.default_rng(seed)
    pool = np.array([0, 0, 0, 1, 2, 3, 255, 256, 257, 511, -1, -7, -2 ** 31, 2 ** 31 - 1] if special else [0, 0, 1, 2, 3],
                    np.int64)
    coarse = rng.integers(0, len(pool), (-(-H // 3), -(-W // 3)))
    lab = pool[np.kron(coarse, np.ones((3, 3), np.int64))[:H, :W]]
    speck = rng.random((H, W)) < 0.1
    lab = np.where(speck, pool[rng.integers(0, len(pool), (H, W))], lab)
    return lab.astype(np.int32)
