"""CPU restatement of stain2stain_amd.stain_quant in numpy, twice:

  *32  the definition in float32, operation by operation as the kernels round it: what the GPU must equal bit for bit
  *64  a plain float64 evaluation (double log10, double unmix): what the float32 restatement is judged against

Nothing here imports the package.
"""
import numpy as np

HDAB = np.array([[0.650, 0.704, 0.286], [0.268, 0.570, 0.776]])
HED = np.array([[0.65, 0.70, 0.29], [0.07, 0.99, 0.11], [0.27, 0.57, 0.78]])


def stain_matrix(stains):
    """float64 [3, 3]: unit rows, a missing third row the normalised cross product."""
    m = {"hdab": HDAB, "hed": HED}[stains] if isinstance(stains, str) else np.asarray(stains, dtype=np.float64)
    m = m / np.linalg.norm(m, axis=1, keepdims=True)
    if m.shape[0] == 2:
        c = np.cross(m[0], m[1])
        m = np.vstack([m, c / np.linalg.norm(c)])
    return m


def unmix64(stains):
    """float64 [3, 3] m with c = od @ m."""
    return np.linalg.inv(stain_matrix(stains))


def od_table64():
    return -np.log10(np.maximum(np.arange(256), 1) / 255.0)


def od_table32():
    return od_table64().astype(np.float32)


def quantise(x):
    """fp32 network range -> uint8 by the save conversion trunc(clamp((x * 0.5 + 0.5) * 255, 0, 255)), in float32."""
    x = np.asarray(x, dtype=np.float32)
    u = (x * np.float32(0.5) + np.float32(0.5)) * np.float32(255.0)
    return np.minimum(np.maximum(u, np.float32(0.0)), np.float32(255.0)).astype(np.int32).astype(np.uint8)


def nchw_to_u8(x):
    """fp32 [B, 3, H, W] -> uint8 [B, H, W, 3]."""
    return np.ascontiguousarray(quantise(x).transpose(0, 2, 3, 1))


def concentrations32(u8, m32):
    """uint8 [..., 3] -> float32 [..., 3]; m32: float32 [3, 3].  ((od_r m_rk) + (od_g m_gk)) + (od_b m_bk), each
    operation a float32 numpy operation, so each is rounded on its own."""
    m32 = np.asarray(m32, dtype=np.float32)
    od = od_table32()[np.asarray(u8)]
    r, g, b = od[..., 0:1], od[..., 1:2], od[..., 2:3]
    c = ((r * m32[0][None, :]) + (g * m32[1][None, :])) + (b * m32[2][None, :])
    assert c.dtype == np.float32
    return c


def concentrations64(u8, m64):
    return od_table64()[np.asarray(u8)] @ np.asarray(m64, dtype=np.float64)


def tissue(u8, white=220, black=0):
    u = np.asarray(u8).astype(np.int32)
    return (u.min(-1) < white) & (u.max(-1) >= black)


def positive32(u8, m32, thresholds, white=220, black=0):
    """bool [..., 3]: tissue and c_k > float32(threshold_k)."""
    thr = np.asarray(thresholds, dtype=np.float32)
    return tissue(u8, white, black)[..., None] & (concentrations32(u8, m32) > thr)


def positive64(u8, m64, thresholds, white=220, black=0):
    thr = np.asarray(thresholds, dtype=np.float32).astype(np.float64)
    return tissue(u8, white, black)[..., None] & (concentrations64(u8, m64) > thr)


def quantify32(u8, m32, thresholds, white=220, black=0):
    """uint8 [B, H, W, 3] -> per-sample dict (numpy): tissue, positive int64; od_sum, burden, mean_od float64."""
    u8 = np.asarray(u8)
    t = tissue(u8, white, black)
    c = concentrations32(u8, m32)
    pos = t[..., None] & (c > np.asarray(thresholds, dtype=np.float32))
    n_t = t.sum(axis=(1, 2)).astype(np.int64)
    n_p = pos.sum(axis=(1, 2)).astype(np.int64)
    od_sum = (np.maximum(c, np.float32(0)).astype(np.float64) * t[..., None]).sum(axis=(1, 2))
    den = np.maximum(n_t, 1).astype(np.float64)[:, None]
    return {"tissue": n_t, "positive": n_p, "od_sum": od_sum, "burden": n_p / den, "mean_od": od_sum / den}


def agreement32(pred_u8, target_u8, m32, thresholds, stain=1, white=220, black=0):
    """uint8 [B, H, W, 3] pairs -> per-sample dict of float64 [B]."""
    pa = positive32(pred_u8, m32, thresholds, white, black)[..., stain]
    pb = positive32(target_u8, m32, thresholds, white, black)[..., stain]
    ta = np.maximum(tissue(pred_u8, white, black).sum(axis=(1, 2)), 1).astype(np.float64)
    tb = np.maximum(tissue(target_u8, white, black).sum(axis=(1, 2)), 1).astype(np.float64)
    both = (pa & pb).sum(axis=(1, 2)).astype(np.float64)
    na, nb = pa.sum(axis=(1, 2)).astype(np.float64), pb.sum(axis=(1, 2)).astype(np.float64)
    union = na + nb - both
    empty = union == 0
    ba, bb = na / ta, nb / tb
    return {"burden_pred": ba, "burden_target": bb, "burden_abs_err": np.abs(ba - bb),
            "dice": np.where(empty, 1.0, 2.0 * both / np.where(empty, 1.0, na + nb)),
            "iou": np.where(empty, 1.0, both / np.where(empty, 1.0, union))}


def cell_counts32(region_u8, m32, thresholds, cell, stain=1, white=220, black=0):
    """uint8 [H, W, 3] -> (tissue, positive) int64 [Gy, Gx]; ragged edge cells count only their own pixels."""
    H, W = region_u8.shape[:2]
    Gy, Gx = -(-H // cell), -(-W // cell)
    t = tissue(region_u8, white, black)
    p = positive32(region_u8, m32, thresholds, white, black)[..., stain]
    nt, npos = np.zeros((Gy, Gx), np.int64), np.zeros((Gy, Gx), np.int64)
    for gy in range(Gy):
        for gx in range(Gx):
            sl = (slice(gy * cell, (gy + 1) * cell), slice(gx * cell, (gx + 1) * cell))
            nt[gy, gx], npos[gy, gx] = t[sl].sum(), p[sl].sum()
    return nt, npos


def synthesise(conc, stains):
    """Known concentrations [..., 3] -> uint8 RGB by Beer-Lambert: I = 255 * 10^(-(c @ M)), rounded to nearest."""
    od = np.asarray(conc, dtype=np.float64) @ stain_matrix(stains)
    return np.clip(np.rint(255.0 * 10.0 ** (-od)), 0, 255).astype(np.uint8)
