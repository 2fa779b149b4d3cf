"""Splitting touching stain objects at their necks: a watershed of the exact squared distance map, on the GPU.

``label_components`` makes an object of every connected component of a positive mask, so two plaques that touch over a
few pixels are counted once and measured as one elongated blob.  Here a component is cut where it is thin compared with
what lies on either side.  With ``d2`` the squared distance to the background (``distance_transform``):

  key        key(p) = (d2[p], y W + x), compared lexicographically: a strict total order, so nothing below is ever a tie
  neighbours the 4 or 8 (``connectivity``) foreground neighbours inside the image; foreground = ``d2 > 0``
  basin      up(p) = the neighbour of largest key if that exceeds key(p), else p.  The pixels whose up-chain ends in the
             same root r are a basin, its peak P = d2[r] (its core radius squared)
  neck       over every pair of neighbouring pixels (p, q) with a = root(p) != b = root(q) and key(b) > key(a), best(a)
             = the largest (min(d2[p], d2[q]), b): the thickest passage from a to a higher basin, squared half-width m
  join       a links to that b iff P(a) <= floor(min_core^2) or m 2^20 >= rint(1024 neck)^2 P(a), i.e. sqrt(m / P(a))
             >= neck: the neck is at least ``neck`` times as thick as the thinner side's core.  Links rise in key, so
             they form a forest; a part is one of its trees
  one round  nothing is re-evaluated after a join: a second round would depend on the order of the first
  numbering  parts of at least ``min_area`` pixels are numbered 1..count in raster order of their first pixel, the others
             get 0: the numbering stage of ``label_components``, shared with it

Every choice is a maximum over a strict total order and everything counted is an integer: the result is exact, does not
depend on scheduling and is bit-reproducible.  Every part is connected, lies inside one component of the mask, and with
``min_area=1`` the parts cover the mask exactly.  ``neck=0`` is NOT ``label_components``: a basin joins only the ONE higher
neighbour it shares its thickest neck with, so two tops with a lower basin between them stay apart.  With
``connectivity=4`` a ridge that runs diagonally (a rotated rectangle) breaks into a basin per step whose necks are thin,
and is over-segmented at a high ``neck``; use 8 unless the mask itself was labelled with 4.

The kernels are ``csrc/split.hip``: thirteen launches after the distance transform, no host synchronisation, scratch
from the shared workspace.  ``H, W <= MAX_SIDE`` = 32767 and ``B <= 65535``.  GPU only.  DESIGN.md section 3.27.

The reference publishes no object measurement: these numbers have no counterpart there.
"""
from __future__ import annotations

import math
import operator
from typing import Dict, Optional, Sequence

import torch

from . import _native, ops
from ._regionio import gpu_device
from .morphology import MAX_SIDE, _check_mask, _squared, distance_transform
from .objects import (_FG_POSITIVE, _check_mpp, _check_pixels, _density, _label, _object_args, _scratch, _stain_dict,
                      _stain_mask, _words)
from .region import _check_thresholds
from .stain_quant import DEFAULT_THRESHOLDS, _image_kind, _kernel_args, _stain_index

TILE = (32, 64)                    # rows x columns of the ascent pass's tile: ST_H, ST_W of csrc/split.hip
NECK_ONE = 1024                    # the neck ratio is compared in 1/1024


def _split_args(neck, min_core, what: str):
    """(neck_q = rint(1024 neck), core2 = floor(min_core^2))."""
    try:
        neck = float(neck)
    except (TypeError, ValueError):
        raise TypeError(f"{what}: neck must be a number, got {type(neck).__name__}") from None
    if not (math.isfinite(neck) and 0.0 <= neck <= 1.0):
        raise ValueError(f"{what}: neck must lie in [0, 1], got {neck}")
    return int(round(neck * NECK_ONE)), _squared(min_core, "min_core", what)


def _split(d2: torch.Tensor, B: int, H: int, W: int, connectivity: int, neck_q: int, core2: int, min_area: int, M: int,
           what: str) -> Dict[str, torch.Tensor]:
    """The splitting launches on a dense int32 [B, H, W] distance map; every tensor [B, ...]."""
    dev = d2.device
    L = ops._L()
    words = L.s2s_split_words(B, H, W)
    _native.check(words if words < 0 else 0, what)
    scratch = ops._workspace(dev, words, "split").view(torch.int32)
    labels = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    basins = torch.empty((B,), dtype=torch.int32, device=dev)
    kept = torch.zeros((B,), dtype=torch.int64, device=dev)
    largest = torch.zeros((B,), dtype=torch.int32, device=dev)
    hist = torch.zeros((B, 32), dtype=torch.int64, device=dev)
    res = {"labels": labels, "count": count, "kept_pixels": kept, "largest": largest, "size_hist": hist}
    area = bbox = sums = None
    if M:
        area = torch.zeros((B, M), dtype=torch.int32, device=dev)
        bbox = torch.zeros((B, M, 4), dtype=torch.int32, device=dev)
        sums = torch.zeros((B, M, 2), dtype=torch.int64, device=dev)
    rc = L.s2s_split_label(d2.data_ptr(), B, H, W, connectivity, neck_q, core2, min_area, M, scratch.data_ptr(),
                           labels.data_ptr(), count.data_ptr(), basins.data_ptr(), kept.data_ptr(), largest.data_ptr(),
                           hist.data_ptr(), area.data_ptr() if M else 0, bbox.data_ptr() if M else 0,
                           sums.data_ptr() if M else 0, ops._stream())
    _native.check(rc, what)
    if M:
        centroid = torch.empty((B, M, 2), dtype=torch.float32, device=dev)
        _native.check(L.s2s_objects_centroid(count.data_ptr(), area.data_ptr(), sums.data_ptr(), B, M,
                                             centroid.data_ptr(), ops._stream()), what)
        res.update(area=area, bbox=bbox, centroid=centroid)
    res.update(basins=basins, d2=d2)
    return res


def _check_d2(d2, mask: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(d2, torch.Tensor):
        raise TypeError(f"{what}: d2 must be a torch.Tensor, got {type(d2).__name__}")
    if d2.dtype != torch.int32 or d2.shape != mask.shape:
        raise ValueError(f"{what}: d2 must be int32 of the mask's shape {list(mask.shape)}, got {d2.dtype} "
                         f"{list(d2.shape)}")
    if d2.device != mask.device:
        raise ValueError(f"{what}: d2 is on {d2.device}, the mask on {mask.device}")
    return d2


def split_objects(mask: torch.Tensor, *, neck: float = 0.75, min_core: float = 0.0, connectivity: int = 8,
                  min_area: int = 1, max_objects: Optional[int] = None,
                  d2: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """The parts of a bool or uint8 (nonzero = foreground) mask ``[B, H, W]`` or ``[H, W]`` on the GPU: its connected
    components, cut at their necks (the module docstring has the definition).  Row-strided views are read in place by
    ``distance_transform``; ``d2`` (int32, the mask's shape, ``distance_transform(mask)``) skips that transform, and the
    foreground is then ``d2 > 0``.

    ``neck`` in [0, 1]: a basin joins its best higher neighbour iff the neck between them is at least ``neck`` times as
    thick as the basin's own core; 0 joins every basin to that neighbour, 1 joins only across a neck as thick as the
    core.  The default 0.75 is a convention, not a calibration: calibrate on your own slides.  ``min_core`` (pixels):
    basins whose core radius is at most this are joined whatever the neck, which removes the bumps of a ragged outline.
    ``neck=0`` is not ``label_components``: a basin joins one neighbour only, so two tops separated by a lower basin
    stay apart.  ``connectivity=4`` over-segments diagonal ridges at a high ``neck``.

    Returns the keys of ``label_components`` over the parts (``"labels"`` can be handed to ``object_features``
    unchanged) plus ``"basins"`` int32 ``[B]``, the number of basins before joining, and ``"d2"`` int32, the distance
    map; without a batch dimension the leading ``B`` is dropped.  Exact and bit-reproducible; a sample's values do not
    depend on its batch mates; no host synchronisation."""
    what = "split_objects"
    B, H, W = _check_mask(mask, what)
    neck_q, core2 = _split_args(neck, min_core, what)
    connectivity, min_area, M = _object_args(connectivity, min_area, max_objects, what)
    if d2 is not None:
        d2 = _check_d2(d2, mask, what)
    dev = gpu_device(what, mask, host_ok=False)
    with torch.no_grad():
        if d2 is None:
            d2 = distance_transform(mask)
        d = d2.detach().contiguous()
        d = d if d.dim() == 3 else d[None]
        res = _split(d, B, H, W, connectivity, neck_q, core2, min_area, M, what)
    return res if mask.dim() == 3 else {k: v[0] for k, v in res.items()}


def stain_object_split(img: torch.Tensor, *, stain: int = 1, stains="hdab",
                       thresholds: Sequence[float] = DEFAULT_THRESHOLDS, white: int = 220, black: int = 0,
                       neck: float = 0.75, min_core: float = 0.0, connectivity: int = 8, min_area: int = 1,
                       max_objects: Optional[int] = None, mpp: Optional[float] = None,
                       return_labels: bool = False) -> Dict[str, torch.Tensor]:
    """``stain_objects`` with touching objects split at their necks: the keys of ``stain_objects`` (``"count"``,
    ``"tissue"``, ``"positive"``, ``"burden"``, ``"largest"``, ``"size_hist"``, ``"per_mm2"`` with ``mpp``, the table with
    ``max_objects``, ``"labels"`` on request), computed on the parts of ``split_objects`` (``neck``, ``min_core`` as
    there; calibrate them on your own slides), plus ``"components"`` int32 ``[B]``: the connected components of the same
    positive mask at the same ``connectivity`` and ``min_area=1``, what ``stain_objects`` would count.  Images and the
    other arguments as ``stain_objects``.  No host synchronisation."""
    what = "stain_object_split"
    kind, B, H, W = _image_kind(img, what)
    _check_pixels(H, W, what)
    if H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError(f"{what}: {H} x {W} exceeds the limit of {MAX_SIDE} pixels a side")
    stain = _stain_index(stain)
    table, unmix = _kernel_args(stains, thresholds)
    white, black = _check_thresholds(white, black)
    neck_q, core2 = _split_args(neck, min_core, what)
    connectivity, min_area, M = _object_args(connectivity, min_area, max_objects, what)
    mpp = _check_mpp(mpp, what)
    dev = gpu_device(what, img, host_ok=False)
    with torch.no_grad():
        mask, tissue = _stain_mask(img, kind, B, H, W, table, unmix, white, black, stain, what)
        positive = mask & _FG_POSITIVE
        comp = _label(mask.data_ptr(), W, H * W, _FG_POSITIVE, B, H, W, dev, connectivity, 1, 0, what)
        res = _split(distance_transform(positive), B, H, W, connectivity, neck_q, core2, min_area, M, what)
        burden, per_mm2 = _density(res, tissue, mpp, what)
    out = _stain_dict(res, tissue, burden, per_mm2, M, return_labels)
    out["components"] = comp["count"]
    return out


def _check_labels(labels, count, name: str, what: str):
    if not isinstance(labels, torch.Tensor) or not isinstance(count, torch.Tensor):
        raise TypeError(f"{what}: labels_{name} and count_{name} must be torch.Tensors")
    if labels.dtype != torch.int32 or labels.dim() not in (2, 3):
        raise ValueError(f"{what}: labels_{name} must be int32 [B, H, W] or [H, W], got {labels.dtype} "
                         f"{list(labels.shape)}")
    B = int(labels.shape[0]) if labels.dim() == 3 else 1
    H, W = int(labels.shape[-2]), int(labels.shape[-1])
    if B < 1 or H < 1 or W < 1 or B > 65535:
        raise ValueError(f"{what}: labels_{name} {list(labels.shape)}: empty, or more than 65535 samples")
    _check_pixels(H, W, what)
    if count.dtype != torch.int32 or tuple(count.shape) != tuple(labels.shape[:-2]):
        raise ValueError(f"{what}: count_{name} must be int32 {list(labels.shape[:-2])}, got {count.dtype} "
                         f"{list(count.shape)}")
    return B, H, W


def label_agreement(labels_pred: torch.Tensor, count_pred: torch.Tensor, labels_target: torch.Tensor,
                    count_target: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The object-level agreement of ``stain_object_agreement`` between any two label images (int32 ``[B, H, W]`` or
    ``[H, W]``, objects 1..count, as ``label_components`` or ``split_objects`` write them) and their counts (int32
    ``[B]`` or scalars): ``"count_pred"``, ``"count_target"``, ``"count_abs_err"`` (int32) and ``"recall"``,
    ``"precision"``, ``"f1"`` (fp32), by the same kernels.  This is how split labels are compared.  No host
    synchronisation."""
    what = "label_agreement"
    B, H, W = _check_labels(labels_pred, count_pred, "pred", what)
    if _check_labels(labels_target, count_target, "target", what) != (B, H, W) or labels_pred.dim() != labels_target.dim():
        raise ValueError(f"{what}: labels_pred {list(labels_pred.shape)} and labels_target {list(labels_target.shape)} "
                         f"differ in shape")
    dev = gpu_device(what, labels_pred, count_pred, labels_target, count_target, host_ok=False)
    with torch.no_grad():
        lp, lt = labels_pred.detach().contiguous(), labels_target.detach().contiguous()
        cp, ct = count_pred.detach().contiguous().view(B), count_target.detach().contiguous().view(B)
        hits = torch.empty((B, 2), dtype=torch.int32, device=dev)
        scores = torch.empty((B, 3), dtype=torch.float32, device=dev)
        err = torch.empty((B,), dtype=torch.int32, device=dev)
        L = ops._L()
        scratch = _scratch(dev, _words(B, H, W, hits=True))
        _native.check(L.s2s_objects_hits(lp.data_ptr(), lt.data_ptr(), B, H, W, scratch.data_ptr(), hits.data_ptr(),
                                         ops._stream()), what)
        _native.check(L.s2s_objects_scores(cp.data_ptr(), ct.data_ptr(), hits.data_ptr(), B, scores.data_ptr(),
                                           err.data_ptr(), ops._stream()), what)
    out = {"count_pred": cp, "count_target": ct, "count_abs_err": err, "recall": scores[:, 0], "precision": scores[:, 1],
           "f1": scores[:, 2]}
    return out if labels_pred.dim() == 3 else {k: v[0] for k, v in out.items()}
