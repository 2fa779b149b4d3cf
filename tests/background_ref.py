"""CPU restatement of stain2stain_amd.background in numpy and scipy: what the GPU must equal bit for bit.

Grey morphology comes in three forms that tests/test_background_cpu.py holds against each other: ``*_brute`` (the
definition, one footprint offset at a time: tiny shapes), ``*_scipy`` (``scipy.ndimage.grey_erosion`` /
``grey_dilation`` with the footprint, ``mode="constant"`` and ``cval`` the type's maximum / minimum) and the plain names
(the footprint as a stack of row spans, each a ``minimum_filter1d``: what the GPU tests take their references from,
because it is linear in the radius and works on a stack of images at once).  Concentrations, tissue and the save
conversion come from tests/stain_quant_ref.py, the bin from tests/stain_calibrate_ref.py.  Nothing here imports the
package.
"""
import math

import numpy as np
from scipy import ndimage

import stain_calibrate_ref as C
import stain_quant_ref as Q

NB = 4096
OPS = ("erode", "dilate", "open", "close", "tophat", "bothat")
FOOTPRINTS = ("disc", "square")


# ---- footprints ------------------------------------------------------------------------------------------------------
def half_widths(radius, kind="disc"):
    """w[|dy|] for |dy| = 0..R: the footprint is the rows dy with the columns -w..w."""
    if kind == "disc":
        r2 = int(math.floor(radius * radius))
        R = math.isqrt(r2)
        return [math.isqrt(r2 - dy * dy) for dy in range(R + 1)]
    R = int(math.floor(radius))
    return [R] * (R + 1)


def footprint(radius, kind="disc"):
    """bool [2R + 1, 2R + 1]: dy^2 + dx^2 <= floor(radius^2), or |dy|, |dx| <= floor(radius)."""
    if kind == "disc":
        r2 = int(math.floor(radius * radius))
        R = math.isqrt(r2)
        y, x = np.mgrid[-R:R + 1, -R:R + 1]
        return y * y + x * x <= r2
    R = int(math.floor(radius))
    return np.ones((2 * R + 1, 2 * R + 1), bool)


def _lims(dtype):
    i = np.iinfo(dtype)
    return i.min, i.max


# ---- erosion and dilation, three ways --------------------------------------------------------------------------------
def _brute(x, radius, kind, mx):
    """The definition: every offset of the footprint, one by one, over the pixels whose neighbour at that offset lies in
    the image."""
    x = np.asarray(x)
    H, W = x.shape
    F = footprint(radius, kind)
    R = F.shape[0] // 2
    pick = np.maximum if mx else np.minimum
    out = x.copy()                                            # the offset (0, 0)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            if F[dy + R, dx + R] and y0 < y1 and x0 < x1:
                out[y0:y1, x0:x1] = pick(out[y0:y1, x0:x1], x[y0 + dy:y1 + dy, x0 + dx:x1 + dx])
    return out


def erode_brute(x, radius, kind="disc"):
    return _brute(x, radius, kind, False)


def dilate_brute(x, radius, kind="disc"):
    return _brute(x, radius, kind, True)


def erode_scipy(x, radius, kind="disc"):
    x = np.asarray(x)
    return ndimage.grey_erosion(x, footprint=footprint(radius, kind), mode="constant", cval=_lims(x.dtype)[1])


def dilate_scipy(x, radius, kind="disc"):
    x = np.asarray(x)
    return ndimage.grey_dilation(x, footprint=footprint(radius, kind), mode="constant", cval=_lims(x.dtype)[0])


def _spans(x, radius, kind, mx):
    x = np.asarray(x)
    lo, hi = _lims(x.dtype)
    fill = lo if mx else hi
    w = half_widths(radius, kind)
    R = len(w) - 1
    H = x.shape[-2]
    pad = np.full(x.shape[:-2] + (H + 2 * R, x.shape[-1]), fill, x.dtype)
    pad[..., R:R + H, :] = x
    filt = ndimage.maximum_filter1d if mx else ndimage.minimum_filter1d
    pick = np.maximum if mx else np.minimum
    acc = np.full(x.shape, fill, x.dtype)
    for dy in range(-R, R + 1):
        rows = pad[..., R + dy:R + dy + H, :]
        acc = pick(acc, filt(rows, 2 * w[abs(dy)] + 1, axis=-1, mode="constant", cval=fill))
    return acc


def erode(x, radius, kind="disc"):
    """[..., H, W]: the minimum over the in-image pixels of the footprint."""
    return _spans(x, radius, kind, False)


def dilate(x, radius, kind="disc"):
    return _spans(x, radius, kind, True)


_FORMS = {"spans": (erode, dilate), "scipy": (erode_scipy, dilate_scipy), "brute": (erode_brute, dilate_brute)}


def _saturate(v, dtype):
    lo, hi = _lims(dtype)
    return np.clip(v, lo, hi).astype(dtype)


def all_ops(x, radius, kind="disc", form="spans"):
    """{op: result} of the six operations; the differences in wider integers, saturated to the dtype."""
    x = np.asarray(x)
    er, di = _FORMS[form]
    e, d = er(x, radius, kind), di(x, radius, kind)
    o, c = di(e, radius, kind), er(d, radius, kind)
    wide = x.astype(np.int64)
    return {"erode": e, "dilate": d, "open": o, "close": c, "tophat": _saturate(wide - o.astype(np.int64), x.dtype),
            "bothat": _saturate(c.astype(np.int64) - wide, x.dtype)}


def morph(x, op, radius, kind="disc", form="spans"):
    return all_ops(x, radius, kind, form)[op]


# scipy's own compositions take ONE cval for both halves, so within 2 floor(radius) of an image edge they follow another
# border convention than "nothing outside the image"; away from the edges they are the same functions.
def scipy_composite(x, op, radius, kind="disc"):
    x = np.asarray(x)
    fn = {"open": ndimage.grey_opening, "close": ndimage.grey_closing, "tophat": ndimage.white_tophat,
          "bothat": ndimage.black_tophat}[op]
    return fn(x, footprint=footprint(radius, kind), mode="constant", cval=0)


def interior(a, radius):
    """The pixels farther than 2 floor(radius) from every edge (possibly none)."""
    m = 2 * int(math.floor(radius))
    return np.asarray(a)[..., m:a.shape[-2] - m, m:a.shape[-1] - m]


# ---- the box mean, the bins, the corrected numbers ---------------------------------------------------------------------
def box_mean(b, smooth):
    """s = (2 sum + n) // (2 n), sum and n over the in-image pixels of the (2 smooth + 1)^2 window; [..., H, W] >= 0."""
    b = np.asarray(b)
    if smooth == 0:
        return b.copy()
    k = 2 * smooth + 1
    size = (1,) * (b.ndim - 2) + (k, k)
    w = np.ones(size, np.int64)
    s = ndimage.convolve(b.astype(np.int64), w, mode="constant", cval=0)
    n = ndimage.convolve(np.ones(b.shape, np.int64), w, mode="constant", cval=0)
    return ((2 * s + n) // (2 * n)).astype(b.dtype)


def box_mean_brute(b, smooth):
    b = np.asarray(b)
    H, W = b.shape
    out = np.empty_like(b)
    for y in range(H):
        for x in range(W):
            win = b[max(y - smooth, 0):y + smooth + 1, max(x - smooth, 0):x + smooth + 1].astype(np.int64)
            out[y, x] = (2 * int(win.sum()) + win.size) // (2 * win.size)
    return out


def bins(u8, m32, stain=1):
    """uint8 [..., 3] -> int16 [...]: bin(c_stain) of every pixel, the bin of tests/stain_calibrate_ref.py."""
    return C.bins32(Q.concentrations32(np.asarray(u8), m32)[..., stain]).astype(np.int16)


def background(u8, m32, radius, stain=1, smooth=2, kind="disc"):
    """int16 [B, H, W]: open(box mean(bins))."""
    return morph(box_mean(bins(u8, m32, stain), smooth), "open", radius, kind)


def corrected(u8, m32, radius, j, stain=1, smooth=2, kind="disc", white=220, black=0, pool=False):
    """uint8 [B, H, W, 3] -> dict of numpy arrays named as stain_quantify_corrected names them (+ "bins", "bg")."""
    u8 = np.asarray(u8)
    B = u8.shape[0]
    b = bins(u8, m32, stain)
    bg = np.zeros_like(b) if radius is None else background(u8, m32, radius, stain, smooth, kind)
    t = np.maximum(b.astype(np.int32) - bg.astype(np.int32), 0).astype(np.int16)
    tis = Q.tissue(u8, white, black)
    pos = tis & (t >= j)
    hist = np.zeros((B, 3, NB), np.int64)
    for n in range(B):
        hist[n, stain] = np.bincount(t[n][tis[n]], minlength=NB)
    tissue = tis.reshape(B, -1).sum(1).astype(np.int64)
    positive = pos.reshape(B, -1).sum(1).astype(np.int64)
    sum_t = (t.astype(np.int64) * tis).reshape(B, -1).sum(1)
    if pool:
        hist, tissue, positive, sum_t = (v.sum(0, keepdims=True) for v in (hist, tissue, positive, sum_t))
    den = np.maximum(tissue, 1).astype(np.float64)
    return {"tissue": tissue, "positive": positive, "sum_t": sum_t, "burden": positive.astype(np.float64) / den,
            "mean_t": sum_t.astype(np.float64) / den, "hist": hist,
            "mask": (pos.astype(np.uint8) | (tis.astype(np.uint8) << 1)), "corrected": t, "bins": b, "bg": bg}


def agreement(pred_u8, target_u8, m32, radius, j, stain=1, smooth=2, kind="disc", white=220, black=0):
    """float64 [B] each; Dice and IoU are 1 when both masks are empty (the convention of stain_agreement)."""
    a = corrected(pred_u8, m32, radius, j, stain, smooth, kind, white, black)
    b = corrected(target_u8, m32, radius, j, stain, smooth, kind, white, black)
    B = a["mask"].shape[0]
    both = ((a["mask"] & b["mask"] & 1) != 0).reshape(B, -1).sum(1).astype(np.float64)
    na, nb = a["positive"].astype(np.float64), b["positive"].astype(np.float64)
    union = na + nb - both
    empty = union == 0
    return {"burden_pred": a["burden"], "burden_target": b["burden"], "burden_abs_err": np.abs(a["burden"] - b["burden"]),
            "dice": np.where(empty, 1.0, 2.0 * both / np.where(empty, 1.0, na + nb)),
            "iou": np.where(empty, 1.0, both / np.where(empty, 1.0, union))}


# ---- patterns ----------------------------------------------------------------------------------------------------------
def discs(H, W, items):
    y, x = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), bool)
    for cy, cx, r in items:
        m |= (y - cy) ** 2 + (x - cx) ** 2 <= r * r
    return m


def patterns(H, W, dtype, seed):
    """[(name, [H, W] array of dtype)]: values in 0..4095 (int16) or 0..255 (uint8), and the full signed range."""
    rng = np.random.default_rng(seed)
    top = 4095 if dtype == np.int16 else 255
    y, x = np.mgrid[0:H, 0:W]
    low = np.full((H, W), top, np.int64)
    low[H // 2, W // 3] = 3
    high = np.full((H, W), 2, np.int64)
    high[H // 3, W // 2] = top
    out = [("random", rng.integers(0, top + 1, size=(H, W))),
           ("constant", np.full((H, W), top // 3, np.int64)),
           ("one low", low), ("one high", high),
           ("ramp x", x * top // max(W - 1, 1)), ("ramp y", top - y * top // max(H - 1, 1)),
           ("disc mask", discs(H, W, [(H // 2, W // 2, min(H, W) // 3), (2, 3, 4), (H - 1, W - 5, 6)]).astype(np.int64)),
           ("sparse", np.where(rng.random((H, W)) < 0.1, rng.integers(0, top + 1, size=(H, W)), top // 2))]
    if dtype == np.int16:
        out.append(("signed", rng.integers(-32768, 32768, size=(H, W))))
    return [(n, a.astype(dtype)) for n, a in out]


def stack(H, W, dtype, seed):
    """(names, [P, H, W]) of ``patterns``."""
    ps = patterns(H, W, dtype, seed)
    return [n for n, _ in ps], np.stack([a for _, a in ps])
