"""CPU restatement of stain2stain_amd.stain_norm in numpy.  Nothing here imports the package.

  moments, angle_hist, conc_hist   the integer results of the three fit passes: float32 operation by operation where the
                                   kernels compute in float32, so every count must be equal
  plane, vectors, max_conc, fit    the host steps between the passes, in float64
  apply64                          the apply pass evaluated in float64 from the same fp32 constants; ``unrounded`` is the
                                   level before rounding, which decides where a last-bit difference may show
  textbook                         Macenko's method as published: np.cov, eigh, arctan2, np.percentile
"""
import math

import numpy as np

NB = 4096
CONC_MAX = 4.0
REF_VECTORS = np.array([[0.5626, 0.7201, 0.4062], [0.2159, 0.8012, 0.5581]])
REF_MAX_CONC = np.array([1.9705, 1.0308]) / np.log(10.0)


def od_table32():
    return (-np.log10(np.maximum(np.arange(256), 1) / 255.0)).astype(np.float32)


def q_table():
    return np.rint(od_table32().astype(np.float64) * 4096.0).astype(np.int64)


def u_beta(beta=0.15):
    return int(math.floor(255.0 * math.exp(-beta)))


def kept(u8, beta=0.15, black=0):
    mx = np.asarray(u8).astype(np.int32).max(-1)
    return (mx <= u_beta(beta)) & (mx >= black)


def moments(u8, beta=0.15, black=0):
    """The ten exact integers n, sum q_c, sum q_c q_d (rr rg rb gg gb bb) over the kept pixels, as Python ints."""
    q = q_table()[np.asarray(u8)][kept(u8, beta, black)].reshape(-1, 3)
    out = [int(q.shape[0])] + [int(q[:, c].sum()) for c in range(3)]
    out += [int((q[:, c] * q[:, d]).sum()) for c in range(3) for d in range(c, 3)]
    return out


def plane(mom):
    """float32 [3, 2]: the eigenvectors of the two largest eigenvalues of the covariance, signed by the convention."""
    n = float(mom[0])
    s1 = np.array(mom[1:4], dtype=np.float64)
    s2 = np.zeros((3, 3))
    it = iter(mom[4:])
    for c in range(3):
        for d in range(c, 3):
            s2[c, d] = s2[d, c] = float(next(it))
    cov = (s2 / n - np.outer(s1, s1) / n ** 2) / 2.0 ** 24
    w, v = np.linalg.eigh(cov)
    v1, v2 = v[:, 2], v[:, 1]
    if v1.sum() < 0:
        v1 = -v1
    if v2[np.abs(v2).argmax()] < 0:
        v2 = -v2
    return np.stack([v1, v2], axis=1).astype(np.float32), w


def _dot3(od, c):
    """((od_r c_r) + (od_g c_g)) + (od_b c_b) in float32, every operation rounded on its own."""
    c = np.asarray(c, dtype=np.float32)
    out = ((od[..., 0] * c[0]) + (od[..., 1] * c[1])) + (od[..., 2] * c[2])
    assert out.dtype == np.float32
    return out


def _bins(f):
    return np.minimum(np.maximum(np.floor(f), np.float32(0)), np.float32(NB - 1)).astype(np.int64)


def angle_hist(u8, plane32, beta=0.15, black=0):
    """int64 [NB]: the diamond-angle histogram of the kept pixels in the float32 [3, 2] plane."""
    plane32 = np.asarray(plane32, dtype=np.float32)
    od = od_table32()[np.asarray(u8)][kept(u8, beta, black)].reshape(-1, 3)
    x, y = _dot3(od, plane32[:, 0]), _dot3(od, plane32[:, 1])
    d = np.abs(x) + np.abs(y)
    ok = d != 0
    s = y[ok] / d[ok]
    t = (s + np.float32(1.0)) * np.float32(NB // 2)
    assert t.dtype == np.float32
    return np.bincount(_bins(t), minlength=NB).astype(np.int64)


def conc_hist(u8, m32, beta=0.15, black=0):
    """int64 [2, NB]: the histograms of c_0 and c_1 of the kept pixels; m32: float32 [3, 3], c = od @ m."""
    m32 = np.asarray(m32, dtype=np.float32)
    od = od_table32()[np.asarray(u8)][kept(u8, beta, black)].reshape(-1, 3)
    out = []
    for k in range(2):
        f = _dot3(od, m32[:, k]) * np.float32(NB / CONC_MAX)
        assert f.dtype == np.float32
        out.append(np.bincount(_bins(f), minlength=NB).astype(np.int64))
    return np.stack(out)


def rank_bin(hist, p):
    total = int(np.sum(hist))
    rank = max(1, math.ceil(p / 100.0 * total))
    return int(np.searchsorted(np.cumsum(hist), rank, side="left"))


def vectors(hist, plane32, alpha=1.0):
    """float64 [2, 3] from the angle histogram, haematoxylin (the larger R component) first."""
    pl = np.asarray(plane32).astype(np.float64)
    out = []
    for p in (alpha, 100.0 - alpha):
        s = (rank_bin(hist, p) + 0.5) * 2.0 / NB - 1.0
        v = pl[:, 0] * (1.0 - abs(s)) + pl[:, 1] * s
        out.append(v / np.linalg.norm(v))
    if out[0][0] < out[1][0]:
        out.reverse()
    return np.stack(out)


def unmix32(vec):
    """float32 [3, 3] m with c = od @ m: the inverse of the basis completed by the normalised cross product."""
    vec = np.asarray(vec, dtype=np.float64)
    vec = vec / np.linalg.norm(vec, axis=1, keepdims=True)
    c = np.cross(vec[0], vec[1])
    return np.linalg.inv(np.vstack([vec, c / np.linalg.norm(c)])).astype(np.float32)


def max_conc(hists, pct=99.0):
    return np.array([(rank_bin(hists[k], pct) + 1) * CONC_MAX / NB for k in range(2)])


def fit(u8, alpha=1.0, beta=0.15, pct=99.0, black=0):
    """The whole fit on its own: {"plane", "vectors", "max_conc", "pixels"}."""
    mom = moments(u8, beta, black)
    pl, _ = plane(mom)
    vec = vectors(angle_hist(u8, pl, beta, black), pl, alpha)
    return {"plane": pl, "vectors": vec, "max_conc": max_conc(conc_hist(u8, unmix32(vec), beta, black), pct),
            "pixels": mom[0]}


def apply64(u8, m32, scale32, ref32):
    """(uint8 [..., 3], unrounded float64 [..., 3]): the apply pass evaluated in float64 from the fp32 constants the
    kernel gets: m32 [3, 3], scale32 [2] = reference max_conc / max_conc, ref32 [2, 3]."""
    od = od_table32().astype(np.float64)[np.asarray(u8)]
    c = od @ np.asarray(m32, dtype=np.float32).astype(np.float64)[:, :2]
    c = c * np.asarray(scale32, dtype=np.float32).astype(np.float64)
    od2 = c @ np.asarray(ref32, dtype=np.float32).astype(np.float64)
    raw = 255.0 * 10.0 ** (-od2)
    return np.clip(np.rint(raw), 0, 255).astype(np.uint8), raw


def network(u8):
    """uint8 [B, H, W, 3] -> float32 [B, 3, H, W] = (u / 255 - 0.5) / 0.5, each operation in float32."""
    x = (np.asarray(u8).astype(np.float32) / np.float32(255.0) - np.float32(0.5)) / np.float32(0.5)
    return np.ascontiguousarray(np.moveaxis(x, -1, -3))


def textbook(u8, alpha=1.0, beta=0.15):
    """Macenko et al. 2009 as published, in float64 and natural-log OD: (vectors [2, 3] haematoxylin first, kept)."""
    px = np.asarray(u8).reshape(-1, 3).astype(np.float64)
    od = -np.log(np.maximum(px, 1.0) / 255.0)
    od = od[(od >= beta).all(axis=1)]
    w, v = np.linalg.eigh(np.cov(od.T))
    e = v[:, [2, 1]]
    if e[:, 0].sum() < 0:
        e[:, 0] = -e[:, 0]
    proj = od @ e
    phi = np.arctan2(proj[:, 1], proj[:, 0])
    lo, hi = (np.percentile(phi, p, method="inverted_cdf") for p in (alpha, 100.0 - alpha))
    vec = [e @ np.array([np.cos(a), np.sin(a)]) for a in (lo, hi)]
    if vec[0][0] < vec[1][0]:
        vec.reverse()
    return np.stack(vec), od.shape[0]


def synthetic_he(H, W, seed, glass=0.25):
    """uint8 [H, W, 3]: an H&E image of known vectors: gamma-distributed concentrations, ``glass`` of the pixels bare
    slide, +-1 level of noise.  Returns (image, the float64 [2, 3] vectors)."""
    rng = np.random.default_rng(seed)
    vec = np.array([[0.65, 0.70, 0.29], [0.07, 0.99, 0.11]])
    vec = vec / np.linalg.norm(vec, axis=1, keepdims=True)
    conc = np.stack([rng.gamma(2.0, 0.22, size=(H, W)), rng.gamma(2.0, 0.18, size=(H, W))], axis=-1)
    img = np.rint(255.0 * 10.0 ** (-(conc @ vec)))
    bare = rng.random((H, W)) < glass
    img[bare] = rng.integers(235, 256, size=(int(bare.sum()), 3))
    img += rng.integers(-1, 2, size=(H, W, 3))
    return np.clip(img, 0, 255).astype(np.uint8), vec
