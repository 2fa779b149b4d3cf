"""CPU restatement of stain2stain_amd.zonal in numpy and Python integers: what the GPU must equal,
integer for integer and double for double.  Nothing here imports the package.

  columns, tabulate      the per-pixel integers, and their sums by zone byte
  table / pair_table     the per-zone integer tables of uint8 [B, H, W, 3] images and a byte zone map [B, H, W]
  derived / pair_derived the fp64 values, by the operations include/stain2stain_hip.h spells out
  overlap, assign        pixels of every object in every zone; the arg-max with its tie rule, in Python integers
  squared_edges, bands   E_i = floor(e_i^2) and the band rule on two squared distance maps
  distance_zones         the band rule on morphology_ref's exact squared distances
"""
from fractions import Fraction

import numpy as np

import morphology_ref as MR
import stain_quant_ref as R

FAR = MR.FAR


def q32(c):
    """min((int)rintf(fmaxf(c, 0) * 1024), 4095) in float32 (rint: to nearest even, as rintf)."""
    c = np.asarray(c, dtype=np.float32)
    s = np.rint(np.maximum(c, np.float32(0)) * np.float32(1024))
    assert s.dtype == np.float32
    return np.minimum(s.astype(np.int64), 4095)


def _owners(x, pool):
    """[B, ...] per-sample integer tables -> per owner."""
    return x.sum(0, keepdims=True) if pool else x


def tabulate(cols, zones, Z, pool=False):
    """Integer columns [B, H, W, K] summed by zone byte -> (int64 [O, Z, K]; unzoned int64 [O])."""
    cols, zones = np.asarray(cols, np.int64), np.asarray(zones).astype(np.int64)
    B, K = cols.shape[0], cols.shape[-1]
    tab = np.zeros((B, Z, K), np.int64)
    unz = np.zeros(B, np.int64)
    for n in range(B):
        sel = zones[n] < Z
        unz[n] = int((~sel).sum())
        zn, c = zones[n][sel], cols[n][sel]
        for k in range(K):                       # (float64 weights: exact, the sums stay far below 2^53)
            tab[n, :, k] = np.bincount(zn, weights=c[:, k], minlength=Z).astype(np.int64)
    return _owners(tab, pool), _owners(unz, pool)


def columns(u8, m32, thresholds, white=220, black=0):
    """int64 [B, H, W, 8] per pixel: 1, tissue, positive_0..2, q_0..2 (0 off tissue)."""
    u8 = np.asarray(u8)
    t = R.tissue(u8, white, black)
    c = R.concentrations32(u8, m32)
    pos = t[..., None] & (c > np.asarray(thresholds, dtype=np.float32))
    q = q32(c) * t[..., None]
    return np.concatenate([np.ones_like(t)[..., None], t[..., None], pos, q], axis=-1).astype(np.int64)


def pair_columns(a, b, m32, thresholds, stain=1, white=220, black=0):
    """int64 [B, H, W, 6] per pixel: 1, tissue_a, tissue_b, positive in both, in a only, in b only."""
    a, b = np.asarray(a), np.asarray(b)
    ta, tb = R.tissue(a, white, black), R.tissue(b, white, black)
    pa = R.positive32(a, m32, thresholds, white, black)[..., stain]
    pb = R.positive32(b, m32, thresholds, white, black)[..., stain]
    return np.stack([np.ones_like(ta), ta, tb, pa & pb, pa & ~pb, ~pa & pb], axis=-1).astype(np.int64)


def table(u8, zones, Z, m32, thresholds, white=220, black=0, pool=False):
    """-> (int64 [O, Z, 8] = pixels, tissue, positive_0..2, sum q_0..2 (over tissue); unzoned int64 [O])."""
    return tabulate(columns(u8, m32, thresholds, white, black), zones, Z, pool)


def pair_table(a, b, zones, Z, m32, thresholds, stain=1, white=220, black=0, pool=False):
    """-> (int64 [O, Z, 6] = pixels, tissue_a, tissue_b, positive in both, in a only, in b only; unzoned [O])."""
    return tabulate(pair_columns(a, b, m32, thresholds, stain, white, black), zones, Z, pool)


def derived(tab, unz):
    """The fp64 values of a single table: each one or two IEEE double operations on exact integers."""
    tab, unz = np.asarray(tab, np.int64), np.asarray(unz, np.int64)
    pixels, tissue = tab[..., 0], tab[..., 1]
    td = np.maximum(tissue, 1).astype(np.float64)[..., None]
    total = unz + pixels.sum(-1)
    return {"burden": tab[..., 2:5].astype(np.float64) / td,
            "mean_conc": (tab[..., 5:8].astype(np.float64) / td) / 1024.0,
            "tissue_frac": tissue.astype(np.float64) / np.maximum(pixels, 1).astype(np.float64),
            "area_frac": pixels.astype(np.float64) / np.maximum(total, 1).astype(np.float64)[..., None]}


def pair_derived(tab):
    tab = np.asarray(tab, np.int64)
    ta, tb, both = tab[..., 1], tab[..., 2], tab[..., 3]
    na, nb, uni = both + tab[..., 4], both + tab[..., 5], both + tab[..., 4] + tab[..., 5]
    ba = na.astype(np.float64) / np.maximum(ta, 1).astype(np.float64)
    bb = nb.astype(np.float64) / np.maximum(tb, 1).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        dice = np.where(na + nb == 0, 1.0, (2 * both).astype(np.float64) / (na + nb).astype(np.float64))
        iou = np.where(uni == 0, 1.0, both.astype(np.float64) / uni.astype(np.float64))
    return {"burden_pred": ba, "burden_target": bb, "burden_abs_err": np.abs(ba - bb), "dice": dice, "iou": iou}


def per_mm2(objects, tissue, mpp):
    """(double)objects / ((double)tissue * (mpp * mpp * 1e-6)), 0 without tissue."""
    scale = mpp * mpp * 1e-6
    objects, tissue = np.asarray(objects, np.int64), np.asarray(tissue, np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(tissue > 0, objects.astype(np.float64) / (tissue.astype(np.float64) * scale), 0.0)


# ---- objects by zone ---------------------------------------------------------------------------------------------------
def overlap(labels, zones, Z, M):
    """-> (overlap int32 [B, M, Z], area int32 [B, M], count int32 [B])."""
    labels, zones = np.asarray(labels), np.asarray(zones).astype(np.int64)
    B = labels.shape[0]
    ov = np.zeros((B, M, Z), np.int32)
    area = np.zeros((B, M), np.int32)
    count = np.zeros(B, np.int32)
    for n in range(B):
        count[n] = max(int(labels[n].max()), 0)
        sel = (labels[n] >= 1) & (labels[n] <= M)
        lab, zn = labels[n][sel].astype(np.int64) - 1, zones[n][sel]
        area[n] = np.bincount(lab, minlength=M)
        zoned = zn < Z
        ov[n] = np.bincount(lab[zoned] * Z + zn[zoned], minlength=M * Z).reshape(M, Z)
    return ov, area, count


def assign(ov, area, count):
    """The arg-max in Python integers: the zone of largest overlap, ties to the smaller zone; -1 without a zoned pixel
    and in rows at or beyond min(count, M).  -> zone int32 [B, M], zone_pixels int64 [B, M], objects, object_pixels
    int64 [B, Z]."""
    ov = np.asarray(ov)
    B, M, Z = ov.shape
    zone = np.full((B, M), -1, np.int32)
    zpix = np.zeros((B, M), np.int64)
    objects, opix = np.zeros((B, Z), np.int64), np.zeros((B, Z), np.int64)
    for n in range(B):
        for m in range(min(int(count[n]), M)):
            best, bz = 0, -1
            for z in range(Z):
                v = int(ov[n, m, z])
                if v > best:
                    best, bz = v, z
            if bz >= 0:
                zone[n, m], zpix[n, m] = bz, best
                objects[n, bz] += 1
                opix[n, bz] += int(area[n, m])
    return zone, zpix, objects, opix


def object_zones(labels, zones, Z, M):
    ov, area, count = overlap(labels, zones, Z, M)
    zone, zpix, objects, opix = assign(ov, area, count)
    return {"zone": zone, "zone_pixels": zpix, "area": area, "count": count, "objects": objects, "object_pixels": opix,
            "overlap": ov}


# ---- distance bands ----------------------------------------------------------------------------------------------------
def squared_edges(edges):
    """E_i = floor(e_i^2), exactly, as Python integers."""
    return [int(Fraction(float(e)) ** 2) for e in edges]


def bands(d2_bg, d2_fg, E, side="both"):
    """uint8 like the maps.  Foreground iff d2_bg > 0: #{i : d2_bg > E_i}; background: n + 1 + #{i : d2_fg > E_i}."""
    d2_bg, d2_fg = np.asarray(d2_bg, np.int64), np.asarray(d2_fg, np.int64)
    Ea = np.asarray(E, np.int64)
    n = len(E)
    inside = (d2_bg[..., None] > Ea).sum(-1)
    outside = n + 1 + (d2_fg[..., None] > Ea).sum(-1)
    fg = d2_bg > 0
    out = np.where(fg, inside, outside)
    if side == "inside":
        out = np.where(fg, out, 255)
    elif side == "outside":
        out = np.where(fg, 255, out)
    return out.astype(np.uint8)


def distance_zones(masks, edges, side="both"):
    """masks [B, H, W] -> (uint8 [B, H, W], num_zones) on morphology_ref's exact squared distances."""
    E = squared_edges(edges)
    out = np.stack([bands(MR.d2(m, "background"), MR.d2(m, "foreground"), E, side) for m in np.asarray(masks)])
    return out, 2 * len(E) + 2
