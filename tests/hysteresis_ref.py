"""CPU restatement of stain2stain_amd.hysteresis in numpy and scipy: what the GPU must equal bit for bit.
Nothing here imports the package.

  selection   ``scipy.ndimage.label`` of the mask, ``bincount`` of the labels under ``marker & mask``: a component is
              selected iff (its seeds >= min_seed) != invert; everything ``label_components`` returns is then
              tests/objects_ref.py on the selected pixels
  dual mask   bit 0 = tissue and t >= j_low, bit 1 = tissue, bit 2 = tissue and t >= j_high, and the three counts
  stains      t = the bins (radius None) or the corrected t of tests/background_ref.py
"""
import numpy as np
from scipy import ndimage

import background_ref as G
import objects_ref as O
import stain_quant_ref as Q


# ---- selection -------------------------------------------------------------------------------------------------------
def selected(mask, marker, connectivity=8, min_seed=1, invert=False):
    """(bool [H, W] of the selected components, candidates, seeded, seed_pixels) of one 2-D mask and marker."""
    mask, marker = np.asarray(mask) != 0, np.asarray(marker) != 0
    lab, n = ndimage.label(mask, structure=O.structure(connectivity))
    seeds = np.bincount(lab[marker & mask], minlength=n + 1)
    has = seeds >= min_seed
    has[0] = False
    keep = has != bool(invert)
    keep[0] = False
    return keep[lab], n, int(has.sum()), int((marker & mask).sum())


def select(mask, marker, connectivity=8, min_seed=1, invert=False, min_area=1, max_objects=None):
    """What select_components(..., return_mask=True) returns for one 2-D mask, as numpy arrays."""
    sel, cand, seeded, pixels = selected(mask, marker, connectivity, min_seed, invert)
    out = O.components(sel, connectivity, min_area, max_objects)
    out.update(candidates=np.int32(cand), seeded=np.int32(seeded), seed_pixels=np.int64(pixels), mask=sel.astype(np.uint8))
    return out


def select_batch(masks, markers, **kw):
    per = [select(m, k, **kw) for m, k in zip(masks, markers)]
    return {k: np.stack([p[k] for p in per]) for k in per[0]}


def propagation(mask, marker, connectivity=8):
    """scipy's own binary reconstruction."""
    mask, marker = np.asarray(mask) != 0, np.asarray(marker) != 0
    return ndimage.binary_propagation(marker & mask, mask=mask, structure=O.structure(connectivity))


def border(H, W):
    b = np.zeros((H, W), bool)
    b[0], b[-1], b[:, 0], b[:, -1] = True, True, True, True
    return b


def clear_border(mask, connectivity=8):
    mask = np.asarray(mask) != 0
    return selected(mask, border(*mask.shape), connectivity, 1, True)[0]


# ---- the dual mask ---------------------------------------------------------------------------------------------------
def dual(t, tissue, j_low, j_high, pool=False):
    """(byte [B, H, W], counts int64 [owners, 3] = tissue, weak, strong) of int16 t [B, H, W] and bool tissue."""
    t = np.asarray(t)
    tis = np.ones(t.shape, bool) if tissue is None else np.asarray(tissue) != 0
    weak, strong = tis & (t >= j_low), tis & (t >= j_high)
    byte = weak.astype(np.uint8) | (tis.astype(np.uint8) << 1) | (strong.astype(np.uint8) << 2)
    B = t.shape[0]
    counts = np.stack([v.reshape(B, -1).sum(1) for v in (tis, weak, strong)], axis=1).astype(np.int64)
    return byte, (counts.sum(0, keepdims=True) if pool else counts)


def hysteresis(t, tissue, j_low, j_high, connectivity=8, min_seed=1):
    """uint8 0 / 1 [B, H, W]: the weak components with at least min_seed strong pixels."""
    byte, _ = dual(t, tissue, j_low, j_high)
    return np.stack([selected(b & 1, b & 4, connectivity, min_seed)[0] for b in byte]).astype(np.uint8)


# ---- stains ----------------------------------------------------------------------------------------------------------
def stain_t(u8, m32, radius, stain=1, smooth=2, kind="disc", white=220, black=0):
    """(t int16 [B, H, W], tissue bool [B, H, W]) of uint8 [B, H, W, 3] images."""
    u8 = np.asarray(u8)
    b = G.bins(u8, m32, stain)
    tis = Q.tissue(u8, white, black)
    if radius is None:
        return b, tis
    bg = G.background(u8, m32, radius, stain, smooth, kind)
    return np.maximum(b.astype(np.int32) - bg.astype(np.int32), 0).astype(np.int16), tis


def stain_objects(u8, m32, j_low, j_high, radius=None, stain=1, smooth=2, kind="disc", white=220, black=0,
                  connectivity=8, min_seed=1, min_area=1, max_objects=None):
    """What stain_objects_hysteresis(..., return_labels=True, return_mask=True) returns (without per_mm2)."""
    t, tis = stain_t(u8, m32, radius, stain, smooth, kind, white, black)
    byte, counts = dual(t, tis, j_low, j_high)
    r = select_batch(byte & 1, byte & 4, connectivity=connectivity, min_seed=min_seed, min_area=min_area,
                     max_objects=max_objects)
    tissue = counts[:, 0]
    out = {"count": r["count"], "tissue": tissue, "positive": r["kept_pixels"],
           "burden": r["kept_pixels"].astype(np.float64) / np.maximum(tissue, 1).astype(np.float64),
           "largest": r["largest"], "size_hist": r["size_hist"], "labels": r["labels"],
           "mask": r["mask"] | (tis.astype(np.uint8) << 1), "weak": counts[:, 1], "strong": counts[:, 2],
           "candidates": r["candidates"], "seeded": r["seeded"]}
    if max_objects is not None:
        out.update({k: r[k] for k in ("area", "bbox", "centroid")})
    return out


def agreement(pred_u8, target_u8, m32, j_low, j_high, radius=None, **kw):
    """float64 [B] each; Dice and IoU are 1 when both masks are empty."""
    a = stain_objects(pred_u8, m32, j_low, j_high, radius, **kw)
    b = stain_objects(target_u8, m32, j_low, j_high, radius, **kw)
    B = a["mask"].shape[0]
    both = ((a["mask"] & b["mask"] & 1) != 0).reshape(B, -1).sum(1).astype(np.float64)
    na, nb = a["positive"].astype(np.float64), b["positive"].astype(np.float64)
    union = na + nb - both
    empty = union == 0
    return {"burden_pred": a["burden"], "burden_target": b["burden"], "burden_abs_err": np.abs(a["burden"] - b["burden"]),
            "dice": np.where(empty, 1.0, 2.0 * both / np.where(empty, 1.0, na + nb)),
            "iou": np.where(empty, 1.0, both / np.where(empty, 1.0, union))}


# ---- the case the feature exists for ---------------------------------------------------------------------------------
PLAQUE_CENTRES = ((20, 30), (60, 70), (30, 120), (70, 140))


def plaques(H=96, W=160, seed=880):
    """int16 [H, W] bin plane: 40 everywhere, four blobs (halo discs d^2 <= 81 at 200, cores d^2 <= 9 at 400) and 2 %
    speckles at 250 farther than 13 px from every blob centre (with the default seed: 247 of them in 229 8-connected
    objects).  Returns (t, the union of the halo discs)."""
    y, x = np.mgrid[0:H, 0:W]
    t = np.full((H, W), 40, np.int16)
    halo, far = np.zeros((H, W), bool), np.ones((H, W), bool)
    for cy, cx in PLAQUE_CENTRES:
        d2 = (y - cy) ** 2 + (x - cx) ** 2
        halo |= d2 <= 81
        far &= d2 > 13 * 13
    t[halo] = 200
    for cy, cx in PLAQUE_CENTRES:
        t[(y - cy) ** 2 + (x - cx) ** 2 <= 9] = 400
    speck = (np.random.default_rng(seed).random((H, W)) < 0.02) & far
    t[speck] = 250
    return t, halo
