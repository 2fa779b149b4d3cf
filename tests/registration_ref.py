"""CPU restatement of stain2stain_amd.registration in numpy: the integer structure maps, the integer
sums of the search, the float64 score, the total-order pick and the two-level form, plus a generator of synthetic
H&E / H-DAB pairs with a planted shift.  Nothing here imports the package.

Everything counted is an integer, so maps, ``tsum`` and ``sums`` must be bit-equal to the kernels'; the scores are one
float64 division and one square root away from those integers.
"""
import numpy as np

import stain_norm_ref as N
import stain_quant_ref as Q

MAX_RADIUS = 32
MAX_TEMPLATE = 1 << 18


def q_table():
    """int64 [256]: rint(od(u) * 2^12), the table of DESIGN.md 3.18."""
    return N.q_table()


def weights(stains="hed", stain=0, gain=100.0):
    """int64 [3]: rint(m[ch][stain] * gain * 16), m the float64 unmixing matrix of the basis."""
    return np.rint(Q.unmix64(stains)[:, stain] * float(gain) * 16.0).astype(np.int64)


def structure(u8, w, ds=1):
    """uint8 [..., H, W, 3] -> uint8 [..., H // ds, W // ds]."""
    acc = (q_table()[np.asarray(u8)] * np.asarray(w, dtype=np.int64)).sum(-1)
    f = np.clip((acc + (1 << 15)) >> 16, 0, 255)
    if ds > 1:
        H, W = f.shape[-2:]
        h, wd = H // ds, W // ds
        f = f[..., :h * ds, :wd * ds].reshape(f.shape[:-2] + (h, ds, wd, ds)).sum((-3, -1))
        f = (f + ds * ds // 2) // (ds * ds)
    return f.astype(np.uint8)


def search(a, b, R, cy=0, cx=0):
    """One sample: (tsum int64 [3], sums int64 [S, S, 3], scores float64 [S, S]).  An empty template gives zeros."""
    a, b = np.asarray(a), np.asarray(b)
    h, w = a.shape
    S = 2 * R + 1
    cy, cx = int(cy), int(cx)
    my, mx = R + abs(cy), R + abs(cx)
    tsum, sums, scores = np.zeros(3, np.int64), np.zeros((S, S, 3), np.int64), np.zeros((S, S), np.float64)
    if h - 2 * my < 1 or w - 2 * mx < 1:
        return tsum, sums, scores
    t = a[my:h - my, mx:w - mx].astype(np.int64)
    n, sa, saa = t.size, int(t.sum()), int((t * t).sum())
    tsum[:] = (n, sa, saa)
    va = n * saa - sa * sa
    for iy in range(S):
        for ix in range(S):
            dy, dx = cy + iy - R, cx + ix - R
            win = b[my + dy:h - my + dy, mx + dx:w - mx + dx].astype(np.int64)
            assert win.shape == t.shape
            sb, sbb, sab = int(win.sum()), int((win * win).sum()), int((t * win).sum())
            sums[iy, ix] = (sb, sbb, sab)
            vb = n * sbb - sb * sb
            num = n * sab - sa * sb
            assert max(abs(va), abs(vb), abs(num)) < 1 << 53
            if va != 0 and vb != 0:
                scores[iy, ix] = float(num) / np.sqrt(float(va) * float(vb))
    return tsum, sums, scores


def order(scores, R):
    """The linear indices of the S x S scores in the total order of the pick, best first."""
    S = 2 * R + 1
    iy, ix = np.mgrid[0:S, 0:S]
    d2 = (iy - R) ** 2 + (ix - R) ** 2
    return np.lexsort((ix.ravel(), iy.ravel(), d2.ravel(), -scores.ravel()))


def pick(tsum, scores, R, cy=0, cx=0, ds=1):
    """(shift (dy, dx) in full-resolution pixels, score, score_center, margin, valid) of one sample."""
    n, sa, saa = (int(v) for v in tsum)
    clamp = lambda v: int(min(max(v, -(1 << 31)), (1 << 31) - 1))    # noqa: E731
    if n == 0 or n * saa - sa * sa == 0:
        return (clamp(int(cy) * ds), clamp(int(cx) * ds)), 0.0, 0.0, 0.0, 0
    S = 2 * R + 1
    best = int(order(scores, R)[0])
    py, px = best // S, best % S
    margin = 0.0
    if R >= 2:
        iy, ix = np.mgrid[0:S, 0:S]
        outside = (np.abs(iy - py) > 1) | (np.abs(ix - px) > 1)
        margin = float(scores[py, px] - scores[outside].max())
    return ((int(cy) + py - R) * ds, (int(cx) + px - R) * ds), float(scores[py, px]), float(scores[R, R]), margin, 1


def runner_up_gap(scores, R):
    """The best score minus the second best in the total order."""
    o = order(scores, R)
    flat = scores.ravel()
    return float(flat[o[0]] - flat[o[1]]) if flat.size > 1 else float("inf")


def level(a, b, R, center=None, ds=1):
    """One search level over a batch of maps: a dict of numpy arrays, ``shift`` in full-resolution pixels."""
    B = a.shape[0]
    S = 2 * R + 1
    out = {"tsum": np.zeros((B, 3), np.int64), "sums": np.zeros((B, S, S, 3), np.int64),
           "scores": np.zeros((B, S, S)), "shift": np.zeros((B, 2), np.int32), "score": np.zeros(B),
           "score_center": np.zeros(B), "margin": np.zeros(B), "valid": np.zeros(B, np.int32)}
    for s in range(B):
        cy, cx = (0, 0) if center is None else (int(center[s][0]), int(center[s][1]))
        out["tsum"][s], out["sums"][s], out["scores"][s] = search(a[s], b[s], R, cy, cx)
        sh, sc, s0, mg, ok = pick(out["tsum"][s], out["scores"][s], R, cy, cx, ds)
        out["shift"][s], out["score"][s], out["score_center"][s], out["margin"][s], out["valid"][s] = sh, sc, s0, mg, ok
    return out


def register(src, tgt, radius=16, downsample=1, refine=True, center=None, src_stains="hed", tgt_stains="hdab",
             stain=0):
    """``register_pairs`` on uint8 [B, H, W, 3] arrays.  ``center`` is in pixels of the first level searched."""
    ws, wt = weights(src_stains, stain), weights(tgt_stains, stain)
    ds = downsample
    R0 = -(-radius // ds)
    first = level(structure(src, ws, ds), structure(tgt, wt, ds), R0, center, ds)
    if ds == 1 or not refine:
        return first
    return level(structure(src, ws, 1), structure(tgt, wt, 1), ds, first["shift"], 1)


# ---- synthetic pairs -------------------------------------------------------------------------------------------------
def blobs(H, W, seed, count, rmax):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    c = np.zeros((H, W))
    for _ in range(count):
        y, x, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(1.5, rmax)
        c = np.maximum(c, np.clip(1.5 - np.hypot(yy - y, xx - x) / r, 0, 1) * rng.uniform(0.5, 1.5))
    return c


def pair(H, W, seed, dy, dx, pad=24):
    """(src, tgt) uint8 [H, W, 3]: one haematoxylin blob field rendered into an H&E tile and, displaced so that
    ``tgt[y + dy, x + dx]`` is the tissue at ``src[y, x]``, into an H-DAB tile whose DAB blobs are independent;
    concentration noise 0.02."""
    assert max(abs(dy), abs(dx)) <= pad
    rng = np.random.default_rng(seed + 1000)
    hx = blobs(H + 2 * pad, W + 2 * pad, seed, (H * W) // 60, 3.5)
    e = blobs(H, W, seed + 1, (H * W) // 200, 9.0) * 0.6
    d = blobs(H, W, seed + 2, (H * W) // 400, 6.0) * 1.2
    hs = hx[pad:pad + H, pad:pad + W]
    ht = hx[pad - dy:pad - dy + H, pad - dx:pad - dx + W]
    src = Q.synthesise(np.stack([hs, e, np.zeros_like(e)], -1) + rng.normal(0, 0.02, (H, W, 3)), "hed")
    tgt = Q.synthesise(np.stack([0.7 * ht, d, np.zeros_like(d)], -1) + rng.normal(0, 0.02, (H, W, 3)), "hdab")
    return src, tgt


def batch(H, W, seed, shifts):
    """Three pairs: the planted ``shifts`` in turn, repeated to fill the batch."""
    pairs = [pair(H, W, seed + 10 * n, *shifts[n % len(shifts)]) for n in range(3)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


# name: (H, W, radius at the level searched first, downsample, refine, planted shifts, seed)
CASES = {
    "corners": (70, 90, 5, 1, False, [(-5, 5), (5, -5), (0, 0)], 1),
    "workload_radius": (70, 90, 16, 1, False, [(16, -16), (-9, 13)], 4),
    "aligned": (64, 64, 8, 1, False, [(3, -7)], 9),
    "odd_ds2": (71, 93, 6, 2, False, [(-12, 8)], 6),
    "two_level": (96, 100, 4, 4, True, [(-13, 9)], 7),
}


def case(name):
    """(src, tgt, planted int [3, 2], register_pairs keyword arguments) of one row of the table."""
    H, W, R, ds, refine, shifts, seed = CASES[name]
    src, tgt = batch(H, W, seed, shifts)
    planted = np.array([shifts[n % len(shifts)] for n in range(3)], np.int32)
    return src, tgt, planted, {"radius": R * ds, "downsample": ds, "refine": refine}
