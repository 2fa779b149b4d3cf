"""The tile quality control of stain2stain_amd/qc.py (csrc/qc.hip) restated in numpy int64, by brute
force: per-pixel maps of the whole image, then plain sums over each window.  Shared by tests/test_qc_cpu.py and
tests/test_qc_gpu.py; nothing here imports the package."""
import numpy as np

KEYS = ("tissue", "focus_n", "lap_sum", "lap_sq", "luma_sum", "green", "blue", "dark")
DEFAULTS = dict(white=220, black=0, ink_chroma=40, dark=60)


def luma(img):
    a = img.astype(np.int64)
    return (77 * a[..., 0] + 150 * a[..., 1] + 29 * a[..., 2] + 128) >> 8


def pixel_maps(img, white=220, black=0, ink_chroma=40, dark=60):
    """int64 [H, W, 8]: what every pixel of the uint8 [H, W, 3] image adds to the eight counts."""
    a = img.astype(np.int64)
    H, W = a.shape[:2]
    R, G, B = a[..., 0], a[..., 1], a[..., 2]
    mx, mn = a.max(-1), a.min(-1)
    tissue = (mn < white) & (mx >= black)
    Y = luma(img)
    L = np.zeros((H, W), np.int64)
    if H >= 3 and W >= 3:
        L[1:-1, 1:-1] = Y[:-2, 1:-1] + Y[2:, 1:-1] + Y[1:-1, :-2] + Y[1:-1, 2:] - 4 * Y[1:-1, 1:-1]
    inner = np.zeros((H, W), bool)
    inner[1:H - 1, 1:W - 1] = True
    focus = tissue & inner
    green = tissue & (G - np.maximum(R, B) >= ink_chroma)
    blue = tissue & (B - R >= ink_chroma) & (G >= R)
    dk = tissue & (mx < dark)
    return np.stack([tissue, focus, np.where(focus, L, 0), np.where(focus, L * L, 0), np.where(tissue, Y, 0), green, blue,
                     dk], -1).astype(np.int64)


def window_counts(maps, top, left, win_h, win_w):
    """The eight counts of the window clipped to the image, and its in-image area."""
    H, W = maps.shape[:2]
    y0, y1, x0, x1 = max(top, 0), min(top + win_h, H), max(left, 0), min(left + win_w, W)
    if y0 >= y1 or x0 >= x1:
        return np.zeros(8, np.int64), 0
    return maps[y0:y1, x0:x1].reshape(-1, 8).sum(0), (y1 - y0) * (x1 - x0)


def derive(counts, area):
    """The fp64 values from int64 counts [..., 8] and areas [...]; 0 where the denominator is 0."""
    c = np.asarray(counts, np.int64).astype(np.float64)
    area = np.asarray(area, np.float64)

    def over(num, den):
        return np.where(den > 0, num / np.maximum(den, 1.0), 0.0)

    t, fn = c[..., 0], c[..., 1]
    mean = c[..., 2] / np.maximum(fn, 1.0)
    return {"focus": np.where(fn > 0, c[..., 3] / np.maximum(fn, 1.0) - mean * mean, 0.0), "tissue_frac": over(t, area),
            "ink_frac": over(c[..., 5] + c[..., 6], t), "dark_frac": over(c[..., 7], t), "mean_luma": over(c[..., 4], t)}


def windows(img, origins, win_h, win_w, **thr):
    maps = pixel_maps(img, **thr)
    got = [window_counts(maps, int(t), int(l), win_h, win_w) for t, l in origins]
    counts = np.stack([c for c, _ in got]) if got else np.zeros((0, 8), np.int64)
    area = np.array([a for _, a in got], np.int64)
    return dict(derive(counts, area), counts=counts, area=area)


def tiles(batch, **thr):
    """tile_qc: every tile of a uint8 [B, H, W, 3] batch is its own image."""
    H, W = batch.shape[1:3]
    each = [windows(t, [(0, 0)], H, W, **thr) for t in batch]
    return {k: np.concatenate([e[k] for e in each]) for k in each[0]}


def axis_origins(L, tile, overlap):
    if L <= tile:
        return [0]
    S = tile - overlap
    n = -(-(L - tile) // S) + 1
    return [min(i * S, L - tile) for i in range(n)]


def plan(H, W, tile, overlap):
    return [(y, x) for y in axis_origins(H, tile, overlap) for x in axis_origins(W, tile, overlap)]


def region(img, tile, overlap, **thr):
    H, W = img.shape[:2]
    return windows(img, plan(H, W, tile, overlap), tile, tile, **thr)


def cell_map(img, cell, **thr):
    H, W = img.shape[:2]
    Gy, Gx = -(-H // cell), -(-W // cell)
    flat = windows(img, [(gy * cell, gx * cell) for gy in range(Gy) for gx in range(Gx)], cell, cell, **thr)
    return {k: v.reshape(Gy, Gx, *v.shape[1:]) for k, v in flat.items()}


def keep(q, min_tissue=0.05, max_ink=0.01, max_dark=0.5, min_focus=None, min_focus_rel=None):
    focus = np.asarray(q["focus"], np.float64)
    has = np.asarray(q["tissue_frac"]) >= min_tissue
    k = has & (np.asarray(q["ink_frac"]) <= max_ink) & (np.asarray(q["dark_frac"]) <= max_dark)
    if min_focus is not None:
        k = k & (focus >= min_focus)
    if min_focus_rel is not None and has.any():
        vals = sorted(focus[has].tolist())
        k = k & (focus >= min_focus_rel * vals[(len(vals) - 1) // 2])
    return k


def window_sums(counts, win, stride):
    counts = np.asarray(counts, np.int64)
    Gy, Gx = counts.shape[:2]
    ny, nx = (Gy - win) // stride + 1, (Gx - win) // stride + 1
    out = np.zeros((ny, nx) + counts.shape[2:], np.int64)
    for i in range(ny):
        for j in range(nx):
            out[i, j] = counts[i * stride:i * stride + win, j * stride:j * stride + win].reshape(win * win, -1).sum(0) \
                .reshape(counts.shape[2:])
    return out


# ---- synthetic material ------------------------------------------------------------------------------------------------
HED = np.array([[0.65, 0.70, 0.29], [0.07, 0.99, 0.11], [0.27, 0.57, 0.78]])      # Ruifrok & Johnston 2001


def stain_palette(n, seed, cmax=2.5):
    """n colours of Beer-Lambert mixtures of the unit H, E and DAB vectors with concentrations in [0, cmax]."""
    rng = np.random.default_rng(seed)
    basis = HED / np.linalg.norm(HED, axis=1, keepdims=True)
    od = rng.uniform(0.0, cmax, (n, 3)) @ basis
    return np.clip(np.round(255.0 * 10.0 ** (-od)), 0, 255).astype(np.uint8)


def gaussian_blur(img, sigma):
    """A separable Gaussian on a float [H, W, C] image, edges replicated."""
    if sigma <= 0:
        return img.astype(np.float64)
    r = int(np.ceil(3 * sigma))
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    out = img.astype(np.float64)
    for axis in (0, 1):
        pad = [(r, r) if a == axis else (0, 0) for a in range(out.ndim)]
        p = np.pad(out, pad, mode="edge")
        out = sum(k[i] * np.take(p, np.arange(i, i + out.shape[axis]), axis=axis) for i in range(2 * r + 1))
    return out


def synthetic_he(H, W, seed, sigma=0.0, noise=1.0):
    """An H&E-like uint8 tile: nuclei (haematoxylin blobs) on an eosin ground, blurred by sigma, plus sensor noise."""
    rng = np.random.default_rng(seed)
    basis = HED / np.linalg.norm(HED, axis=1, keepdims=True)
    conc = np.zeros((H, W, 3))
    conc[..., 1] = 0.5 + 0.2 * rng.random((H, W))
    yy, xx = np.mgrid[:H, :W]
    for _ in range(max(4, H * W // 160)):
        cy, cx, rad = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(1.5, 3.5)
        conc[..., 0] += 1.2 * ((yy - cy) ** 2 + (xx - cx) ** 2 < rad * rad)
    rgb = gaussian_blur(255.0 * 10.0 ** (-(conc @ basis)), sigma)
    return np.clip(np.round(rgb + rng.normal(0.0, noise, rgb.shape)), 0, 255).astype(np.uint8)
