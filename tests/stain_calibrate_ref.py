"""CPU restatement of stain2stain_amd.stain_calibrate in numpy and Python integers: what the GPU must
equal bit for bit.  Concentrations, tissue and the save conversion come from tests/stain_quant_ref.py; the rules are
written as the definitions read, with Python's unbounded integers where the kernels use 128 bits and ``float(int)``
(one rounding to nearest even) where they convert.  Nothing here imports the package.
"""
import math

import numpy as np

import stain_quant_ref as Q

NB = 4096
SCALE = np.float32(1024.0)


def bins32(c):
    """float32 concentrations -> int bins: clamp(ceil(c * 1024) - 1, 0, 4095), every step a float32 operation."""
    c = np.asarray(c)
    assert c.dtype == np.float32
    t = np.ceil(c * SCALE) - np.float32(1.0)
    assert t.dtype == np.float32
    return np.minimum(np.maximum(t, np.float32(0.0)), np.float32(NB - 1)).astype(np.int64)


def histogram(u8, m32, white=220, black=0, pool=False):
    """uint8 [B, H, W, 3] -> (hist int64 [O, 3, NB], tissue int64 [O]); O = B, or 1 pooled."""
    u8 = np.asarray(u8)
    B = u8.shape[0]
    t = Q.tissue(u8, white, black)
    b = bins32(Q.concentrations32(u8, m32))
    hist = np.zeros((B, 3, NB), np.int64)
    for n in range(B):
        for k in range(3):
            hist[n, k] = np.bincount(b[n, ..., k][t[n]], minlength=NB)
    tissue = t.reshape(B, -1).sum(1).astype(np.int64)
    if pool:
        return hist.sum(0, keepdims=True), tissue.sum(keepdims=True)
    return hist, tissue


def pair_histogram(a_u8, b_u8, m32, stain=1, jt=0, white=220, black=0, pool=False):
    """uint8 [B, H, W, 3] pairs -> (hist int64 [O, 4, NB], tissue int64 [O, 2])."""
    a_u8, b_u8 = np.asarray(a_u8), np.asarray(b_u8)
    B = a_u8.shape[0]
    ta, tb = Q.tissue(a_u8, white, black), Q.tissue(b_u8, white, black)
    ba = bins32(Q.concentrations32(a_u8, m32)[..., stain])
    bb = bins32(Q.concentrations32(b_u8, m32)[..., stain])
    hist = np.zeros((B, 4, NB), np.int64)
    for n in range(B):
        both = ta[n] & tb[n]
        hist[n, 0] = np.bincount(ba[n][ta[n]], minlength=NB)
        hist[n, 1] = np.bincount(bb[n][tb[n]], minlength=NB)
        hist[n, 2] = np.bincount(np.minimum(ba[n], bb[n])[both], minlength=NB)
        if jt:
            hist[n, 3] = np.bincount(ba[n][both & (bb[n] >= jt)], minlength=NB)
    tissue = np.stack([ta.reshape(B, -1).sum(1), tb.reshape(B, -1).sum(1)], 1).astype(np.int64)
    if pool:
        return hist.sum(0, keepdims=True), tissue.sum(0, keepdims=True)
    return hist, tissue


def suffix(h):
    """positive[j] = sum over b >= j of h[b], as a list of Python integers."""
    out, s = [0] * len(h), 0
    for b in range(len(h) - 1, -1, -1):
        s += int(h[b])
        out[b] = s
    return out


def otsu_sigma(pos, s1, j):
    """sigma(j) as the kernels form it: the exact integer A, one rounding, three double operations."""
    N, S, P = pos[0], s1[0], pos[j]
    if P == 0 or P == N:
        return 0.0
    a = float(N * s1[j] - P * S)
    return (a * a) / (float(P) * float(N - P))


def otsu(h):
    """(bin, valid) of one histogram."""
    pos = suffix(h)
    s1 = suffix([b * int(v) for b, v in enumerate(h)])
    best, arg = 0.0, 0
    for j in range(1, NB):
        s = otsu_sigma(pos, s1, j)
        if s > best:
            best, arg = s, j
    return (arg, 1) if best > 0.0 else (0, 0)


def triangle(h, coarse=16):
    """(bin, valid) of one histogram: Zack's rule on the right tail of the histogram summed in groups of ``coarse``."""
    g = [sum(int(v) for v in h[i:i + coarse]) for i in range(0, len(h), coarse)]
    p = max(range(len(g)), key=lambda i: (g[i], -i))
    nz = [i for i, v in enumerate(g) if v > 0]
    e = nz[-1] if nz else -1
    if e <= p + 1:
        return 0, 0
    T = {i: g[p] * (e - p) + (g[e] - g[p]) * (i - p) - g[i] * (e - p) for i in range(p + 1, e)}
    return coarse * max(T, key=lambda i: (T[i], -i)), 1


def quantile(h, q):
    """(bin, valid): the smallest j >= 1 with positive[j] <= floor(q N); none, or no tissue: (4095, 0)."""
    pos = suffix(h)
    N = pos[0]
    K = math.floor(q * float(N))
    if N > 0:
        for j in range(1, NB):
            if pos[j] <= K:
                return j, 1
    return NB - 1, 0


def thresholds(hist, coarse=16, quantiles=(0.05,)):
    """hist int64 [O, 3, NB] -> dict of numpy arrays shaped as stain_thresholds returns them."""
    O = hist.shape[0]
    nq = len(quantiles)
    bins = np.zeros((O, 3, 2 + nq), np.int32)
    valid = np.zeros((O, 3, 2 + nq), np.int32)
    positive = np.zeros((O, 3, NB), np.int64)
    for o in range(O):
        for k in range(3):
            h = hist[o, k]
            positive[o, k] = suffix(h)
            rules = [otsu(h), triangle(h, coarse)] + [quantile(h, q) for q in quantiles]
            for c, (b, v) in enumerate(rules):
                bins[o, k, c], valid[o, k, c] = b, v
    thr = bins.astype(np.float64) / 1024.0
    return {"positive": positive, "otsu": thr[..., 0], "otsu_bin": bins[..., 0], "otsu_valid": valid[..., 0],
            "triangle": thr[..., 1], "triangle_bin": bins[..., 1], "triangle_valid": valid[..., 1],
            "quantile": thr[..., 2:], "quantile_bin": bins[..., 2:], "quantile_valid": valid[..., 2:]}


def _dice(both, den):
    return 1.0 if den == 0 else float(2 * both) / float(den)


def match(hist4, jt):
    """One owner's hist int64 [4, NB] -> dict of Python / numpy values named as match_thresholds names them."""
    pa, pb, bc, bd = (suffix(hist4[r]) for r in range(4))
    out = {"positive_pred": np.array(pa, np.int64), "positive_target": np.array(pb, np.int64),
           "both_common": np.array(bc, np.int64),
           "dice_common": np.array([_dice(bc[j], pa[j] + pb[j]) for j in range(NB)])}
    if not jt:
        return out
    Na, Nb, pbt = pa[0], pb[0], pb[jt]
    ok = int(Na > 0 and Nb > 0)
    mj = min(range(1, NB), key=lambda j: (abs(pa[j] * Nb - pbt * Na), j))
    frac = [(1, 1) if pa[j] + pbt == 0 else (2 * bd[j], pa[j] + pbt) for j in range(NB)]
    bj = 1
    for j in range(2, NB):
        if frac[j][0] * frac[bj][1] > frac[bj][0] * frac[j][1]:
            bj = j
    bt = float(pbt) / float(max(Nb, 1))
    bpm = float(pa[mj]) / float(max(Na, 1))
    out.update({"both_cond": np.array(bd, np.int64),
                "dice_cond": np.array([_dice(bd[j], pa[j] + pbt) for j in range(NB)]),
                "match_burden": mj / 1024.0, "match_burden_bin": mj, "match_burden_valid": ok,
                "best_dice": bj / 1024.0, "best_dice_bin": bj, "best_dice_valid": ok,
                "dice_at_best": _dice(bd[bj], pa[bj] + pbt), "burden_pred_at_best": float(pa[bj]) / float(max(Na, 1)),
                "burden_target": bt, "burden_pred_at_match": bpm, "burden_abs_err_at_match": abs(bpm - bt),
                "dice_at_match": _dice(bd[mj], pa[mj] + pbt)})
    return out
