"""Stain object analysis: connected-component labelling of positive masks on the GPU, a minimum object size, per-object
measurements and object-level agreement between a generated stain and the real one.

The positive-area burden of ``stain_quantify`` cannot tell ten plaques of 400 pixels from one blob of 4000, and Dice
hardly sees a missed small object.  Here the positive mask of one stain (``tissue and c_k > threshold_k``, the rule of
``stain_quant``) or any byte mask (the mask head's ``logits > 0``) is cut into its connected components:

  object      a maximal 4- or 8-connected set of foreground pixels; kept iff its area >= ``min_area``
  numbering   kept objects are numbered 1..count in raster order of their first pixel, the numbering of
              ``scipy.ndimage.label`` (after the filter: filter, then renumber)
  per sample  count, kept pixels, the largest area, a histogram of floor(log2(area)) over 32 bins
  per object  (the first ``max_objects`` numbers) area, bounding box ``y0, x0, y1, x1`` end-exclusive, centroid
              = fp32(double(coordinate sum) / area)
  paired      an object is hit when it shares a pixel with an object of the other image; recall = hit target objects /
              target objects, precision = hit prediction objects / prediction objects

Everything counted is an integer, so the results are exact and bit-reproducible; the only roundings are the final
divisions.  The labelling is block-based union-find in HIP (``csrc/objects.hip``): nine launches on the current stream,
no host synchronisation, scratch from the shared workspace.  A sample is limited to ``MAX_PIXELS`` = 2^31 - 2 pixels.
GPU only.  DESIGN.md section 3.19.

The reference publishes no object measurement: these numbers have no counterpart there.
"""
from __future__ import annotations

import ctypes
import math
import operator
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import _native, ops
from ._regionio import DEFAULT_HOST_BAND, BandSource, batch_layout, check_region, gpu_device, gpu_rows
from .image_metrics import _check_pair
from .region import _check_thresholds
from .stain_quant import DEFAULT_THRESHOLDS, _image_kind, _kernel_args, _stain_index, plan_stain_bands

TILE = (32, 64)                    # rows x columns of the local pass's tile: OT_H, OT_W of csrc/objects.hip
MAX_PIXELS = 2 ** 31 - 2           # per sample: parents are int32 raster indices
_FG_ANY, _FG_POSITIVE = 255, 1     # foreground bits of a user's mask / of the stain mask (bit 1 of that one is tissue)


def _check_pixels(H: int, W: int, what: str) -> None:
    if H * W > MAX_PIXELS:
        raise ValueError(f"{what}: {H} x {W} = {H * W} pixels exceed the limit of 2^31 - 2 = {MAX_PIXELS} per sample")


def _object_args(connectivity, min_area, max_objects, what: str) -> Tuple[int, int, int]:
    connectivity, min_area = operator.index(connectivity), operator.index(min_area)
    if connectivity not in (4, 8):
        raise ValueError(f"{what}: connectivity must be 4 or 8, got {connectivity}")
    if not 1 <= min_area <= MAX_PIXELS:
        raise ValueError(f"{what}: min_area must be at least 1, got {min_area}")
    if max_objects is None:
        return connectivity, min_area, 0
    max_objects = operator.index(max_objects)
    if not 1 <= max_objects <= MAX_PIXELS:
        raise ValueError(f"{what}: max_objects must be None or at least 1, got {max_objects}")
    return connectivity, min_area, max_objects


def _check_mpp(mpp, what: str) -> Optional[float]:
    if mpp is None:
        return None
    mpp = float(mpp)
    if not (math.isfinite(mpp) and mpp > 0.0):
        raise ValueError(f"{what}: mpp (micrometres per pixel) must be positive, got {mpp}")
    return mpp


def _check_mask(mask, what: str) -> Tuple[int, int, int]:
    if not isinstance(mask, torch.Tensor):
        raise TypeError(f"{what}: the mask must be a torch.Tensor, got {type(mask).__name__}")
    if mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"{what}: the mask must be bool or uint8, got {mask.dtype}")
    if mask.dim() not in (2, 3):
        raise ValueError(f"{what}: the mask must be [B, H, W] or [H, W], got {list(mask.shape)}")
    B = int(mask.shape[0]) if mask.dim() == 3 else 1
    H, W = int(mask.shape[-2]), int(mask.shape[-1])
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"{what}: empty mask {list(mask.shape)}")
    if B > 65535:
        raise ValueError(f"{what}: at most 65535 samples, got {B}")
    _check_pixels(H, W, what)
    return B, H, W


def _mask_bytes(mask: torch.Tensor, B: int, H: int, W: int) -> Tuple[torch.Tensor, int, int]:
    """(uint8 [B, H, W] view, row pitch, sample stride); a view whose rows are not contiguous bytes is copied."""
    m = mask.detach()
    m = m.view(torch.uint8) if m.dtype == torch.bool else m
    m = m if m.dim() == 3 else m[None]
    pitch = m.stride(1) if H > 1 else W
    img = m.stride(0) if B > 1 else pitch * H
    if (W > 1 and m.stride(2) != 1) or pitch < W or img < pitch * H:
        m = m.contiguous()
        pitch, img = W, W * H
    return m, pitch, img


def _words(B: int, H: int, W: int, hits: bool = False) -> int:
    L = ops._L()
    n = (L.s2s_objects_hit_words if hits else L.s2s_objects_words)(B, H, W)
    _native.check(n if n < 0 else 0, "objects_words")
    return n


def _scratch(dev, words: int) -> torch.Tensor:
    return ops._workspace(dev, words, "objects").view(torch.int32)


def _label(ptr: int, pitch: int, img: int, fg: int, B: int, H: int, W: int, dev, connectivity: int, min_area: int,
           M: int, what: str) -> Dict[str, torch.Tensor]:
    """The labelling launches on a byte mask; every tensor [B, ...]."""
    scratch = _scratch(dev, _words(B, H, W))
    labels = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    kept = torch.zeros((B,), dtype=torch.int64, device=dev)
    largest = torch.zeros((B,), dtype=torch.int32, device=dev)
    hist = torch.zeros((B, 32), dtype=torch.int64, device=dev)
    res = {"labels": labels, "count": count, "kept_pixels": kept, "largest": largest, "size_hist": hist}
    area = bbox = sums = None
    if M:
        area = torch.zeros((B, M), dtype=torch.int32, device=dev)
        bbox = torch.zeros((B, M, 4), dtype=torch.int32, device=dev)
        sums = torch.zeros((B, M, 2), dtype=torch.int64, device=dev)
    L = ops._L()
    rc = L.s2s_objects_label(ptr, pitch, img, fg, B, H, W, connectivity, min_area, M, scratch.data_ptr(),
                             labels.data_ptr(), count.data_ptr(), kept.data_ptr(), largest.data_ptr(), hist.data_ptr(),
                             area.data_ptr() if M else 0, bbox.data_ptr() if M else 0, sums.data_ptr() if M else 0,
                             ops._stream())
    _native.check(rc, what)
    if M:
        centroid = torch.empty((B, M, 2), dtype=torch.float32, device=dev)
        _native.check(L.s2s_objects_centroid(count.data_ptr(), area.data_ptr(), sums.data_ptr(), B, M,
                                             centroid.data_ptr(), ops._stream()), what)
        res.update(area=area, bbox=bbox, centroid=centroid)
    return res


def label_components(mask: torch.Tensor, *, connectivity: int = 8, min_area: int = 1,
                     max_objects: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """Connected components of a bool or uint8 (nonzero = foreground) mask ``[B, H, W]`` or ``[H, W]`` on the GPU;
    row-strided views (a crop of a larger mask) are read in place.  This is also what one applies to the mask head's
    ``logits > 0``.

    Returns device tensors: ``"labels"`` int32 of the mask's shape (0: background or an object smaller than ``min_area``;
    kept objects 1..count in raster order of their first pixel, as ``scipy.ndimage.label`` numbers them), ``"count"``
    int32 ``[B]``, ``"kept_pixels"`` int64 ``[B]``, ``"largest"`` int32 ``[B]`` and ``"size_hist"`` int64 ``[B, 32]``
    (objects by ``floor(log2(area))``); without a batch dimension the leading ``B`` is dropped.  With ``max_objects`` = M
    also ``"area"`` int32 ``[B, M]``, ``"bbox"`` int32 ``[B, M, 4]`` (``y0, x0, y1, x1``, end-exclusive) and ``"centroid"``
    fp32 ``[B, M, 2]`` (y, x) of the objects numbered 1..M; rows at or beyond ``count`` are zero, and when ``count``
    exceeds M the objects beyond M are labelled and counted but not tabulated.  ``connectivity`` 4 or 8.  Exact and
    bit-reproducible; a sample's values do not depend on its batch mates; no host synchronisation."""
    B, H, W = _check_mask(mask, "label_components")
    connectivity, min_area, M = _object_args(connectivity, min_area, max_objects, "label_components")
    dev = gpu_device("label_components", mask, host_ok=False)
    with torch.no_grad():
        m, pitch, img = _mask_bytes(mask, B, H, W)
        res = _label(m.data_ptr(), pitch, img, _FG_ANY, B, H, W, dev, connectivity, min_area, M, "label_components")
    return res if mask.dim() == 3 else {k: v[0] for k, v in res.items()}


def _stain_mask(img: torch.Tensor, kind: str, B: int, H: int, W: int, table, unmix, white: int, black: int, stain: int,
                what: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mask uint8 [B, H, W]: bit 0 positive, bit 1 tissue; tissue int64 [B]) of a batch."""
    dev = img.device
    mask = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    tissue = torch.zeros((B,), dtype=torch.int64, device=dev)
    L = ops._L()
    if kind == "f32":
        a = img.detach().contiguous()
        rc = L.s2s_stain_mask_f32(a.data_ptr(), B, H, W, table, unmix, white, black, stain, mask.data_ptr(), W, H * W,
                                  tissue.data_ptr(), ops._stream())
    else:
        a, pitch, stride = batch_layout(img, what, copy=True)
        rc = L.s2s_stain_mask_u8(a.data_ptr(), pitch, stride, B, 0, H, H, W, table, unmix, white, black, stain,
                                 mask.data_ptr(), W, H * W, tissue.data_ptr(), ops._stream())
    _native.check(rc, what)
    return mask, tissue


def _density(res: Dict[str, torch.Tensor], tissue: torch.Tensor, mpp: Optional[float], what: str):
    """(burden fp32 [B], per_mm2 fp64 [B] or None)."""
    B, dev = tissue.shape[0], tissue.device
    burden = torch.empty((B,), dtype=torch.float32, device=dev)
    per_mm2 = torch.empty((B,), dtype=torch.float64, device=dev) if mpp is not None else None
    scale = (ctypes.c_double * 1)(mpp * mpp * 1e-6) if mpp is not None else None
    rc = ops._L().s2s_objects_density(res["kept_pixels"].data_ptr(), tissue.data_ptr(), res["count"].data_ptr(), B, scale,
                                      burden.data_ptr(), per_mm2.data_ptr() if mpp is not None else 0, ops._stream())
    _native.check(rc, what)
    return burden, per_mm2


_TABLE = ("area", "bbox", "centroid")


def _stain_dict(res, tissue, burden, per_mm2, M: int, return_labels: bool) -> Dict[str, torch.Tensor]:
    out = {"count": res["count"], "tissue": tissue, "positive": res["kept_pixels"], "burden": burden,
           "largest": res["largest"], "size_hist": res["size_hist"]}
    if per_mm2 is not None:
        out["per_mm2"] = per_mm2
    if M:
        out.update({k: res[k] for k in _TABLE})
    if return_labels:
        out["labels"] = res["labels"]
    return out


def stain_objects(img: torch.Tensor, *, stain: int = 1, stains="hdab",
                  thresholds: Sequence[float] = DEFAULT_THRESHOLDS, white: int = 220, black: int = 0,
                  connectivity: int = 8, min_area: int = 1, max_objects: Optional[int] = None,
                  mpp: Optional[float] = None, return_labels: bool = False) -> Dict[str, torch.Tensor]:
    """The positive objects (plaques, cells) of stain ``stain`` in uint8 ``[B, H, W, 3]`` or fp32 ``[B, 3, H, W]`` images
    on the GPU; images, ``stains``, ``thresholds``, ``white`` and ``black`` as ``stain_quantify``.

    Returns device tensors ``[B]``: ``"count"`` int32 (objects of at least ``min_area`` pixels), ``"tissue"`` int64,
    ``"positive"`` int64 (the pixels of the kept objects; with ``min_area=1`` the positive count of ``stain_quantify``),
    ``"burden"`` fp32 = positive / max(tissue, 1), ``"largest"`` int32 and ``"size_hist"`` int64 ``[B, 32]``.  With
    ``mpp`` (micrometres per pixel) also ``"per_mm2"`` fp64 = count / (tissue * mpp^2 * 1e-6), objects per square
    millimetre of tissue, 0 when there is no tissue.  ``max_objects``: the table of ``label_components``;
    ``return_labels``: its ``"labels"``.  One mask launch, the labelling and one small finalize on the current stream,
    no host synchronisation."""
    kind, B, H, W = _image_kind(img, "stain_objects")
    _check_pixels(H, W, "stain_objects")
    stain = _stain_index(stain)
    table, unmix = _kernel_args(stains, thresholds)
    white, black = _check_thresholds(white, black)
    connectivity, min_area, M = _object_args(connectivity, min_area, max_objects, "stain_objects")
    mpp = _check_mpp(mpp, "stain_objects")
    dev = gpu_device("stain_objects", img, host_ok=False)
    with torch.no_grad():
        mask, tissue = _stain_mask(img, kind, B, H, W, table, unmix, white, black, stain, "stain_objects")
        res = _label(mask.data_ptr(), W, H * W, _FG_POSITIVE, B, H, W, dev, connectivity, min_area, M, "stain_objects")
        burden, per_mm2 = _density(res, tissue, mpp, "stain_objects")
    return _stain_dict(res, tissue, burden, per_mm2, M, return_labels)


def stain_object_agreement(pred: torch.Tensor, target: torch.Tensor, *, stain: int = 1, stains="hdab",
                           thresholds: Sequence[float] = DEFAULT_THRESHOLDS, white: int = 220, black: int = 0,
                           connectivity: int = 8, min_area: int = 1) -> Dict[str, torch.Tensor]:
    """Whether a generated stain finds the same objects as the real one: ``"count_pred"``, ``"count_target"``,
    ``"count_abs_err"`` (int32 ``[B]``) and ``"recall"``, ``"precision"``, ``"f1"`` (fp32 ``[B]``).  A target object is
    found when a kept prediction object shares a pixel with it: recall = found target objects / count_target, precision
    = prediction objects that touch a target object / count_pred.  A ratio whose count is 0 is 1 when the other count is
    0 too and 0 otherwise; f1 is 0 when precision + recall = 0.  Inputs as ``stain_agreement``."""
    _check_pair(pred, target, "stain_object_agreement")
    kind, B, H, W = _image_kind(pred, "stain_object_agreement")
    _check_pixels(H, W, "stain_object_agreement")
    stain = _stain_index(stain)
    table, unmix = _kernel_args(stains, thresholds)
    white, black = _check_thresholds(white, black)
    connectivity, min_area, _ = _object_args(connectivity, min_area, None, "stain_object_agreement")
    dev = gpu_device("stain_object_agreement", pred, target, host_ok=False)
    what = "stain_object_agreement"
    with torch.no_grad():
        res = []
        for t in (pred, target):
            mask, _ = _stain_mask(t, kind, B, H, W, table, unmix, white, black, stain, what)
            res.append(_label(mask.data_ptr(), W, H * W, _FG_POSITIVE, B, H, W, dev, connectivity, min_area, 0, what))
        hits = torch.empty((B, 2), dtype=torch.int32, device=dev)
        scores = torch.empty((B, 3), dtype=torch.float32, device=dev)
        err = torch.empty((B,), dtype=torch.int32, device=dev)
        L = ops._L()
        scratch = _scratch(dev, _words(B, H, W, hits=True))
        _native.check(L.s2s_objects_hits(res[0]["labels"].data_ptr(), res[1]["labels"].data_ptr(), B, H, W,
                                         scratch.data_ptr(), hits.data_ptr(), ops._stream()), what)
        _native.check(L.s2s_objects_scores(res[0]["count"].data_ptr(), res[1]["count"].data_ptr(), hits.data_ptr(), B,
                                           scores.data_ptr(), err.data_ptr(), ops._stream()), what)
    return {"count_pred": res[0]["count"], "count_target": res[1]["count"], "count_abs_err": err,
            "recall": scores[:, 0], "precision": scores[:, 1], "f1": scores[:, 2]}


def region_stain_objects(region_u8: torch.Tensor, *, band_rows: Optional[int] = None, stain: int = 1, stains="hdab",
                         thresholds: Sequence[float] = DEFAULT_THRESHOLDS, white: int = 220, black: int = 0,
                         connectivity: int = 8, min_area: int = 1, max_objects: Optional[int] = None,
                         mpp: Optional[float] = None, return_labels: bool = False) -> Dict[str, torch.Tensor]:
    """``stain_objects`` over one whole uint8 ``[H, W, 3]`` region on the GPU or on the host (any row pitch): device
    scalars ``"count"``, ``"tissue"``, ``"positive"``, ``"burden"``, ``"largest"``, ``"size_hist"`` ``[32]``, ``"per_mm2"``
    with ``mpp``, the table ``[M, ...]`` with ``max_objects`` and ``"labels"`` ``[H, W]`` on request.

    The byte mask is built band by band (``plan_stain_bands``; a host region goes through one pinned buffer and one GPU
    band buffer of ``band_rows`` rows, default 512, and never sits on the GPU as RGB), then the whole mask is labelled
    once: an object that spans a band seam is one object.  GPU memory is about 9 bytes per pixel (mask, parents,
    labels).  The result is bit-equal for every ``band_rows`` and for host and GPU input.  Raises ``ValueError`` when
    ``H * W`` exceeds ``MAX_PIXELS`` = 2^31 - 2."""
    what = "region_stain_objects"
    H, W, _ = check_region(region_u8, what)
    _check_pixels(H, W, what)
    stain = _stain_index(stain)
    table, unmix = _kernel_args(stains, thresholds)
    white, black = _check_thresholds(white, black)
    connectivity, min_area, M = _object_args(connectivity, min_area, max_objects, what)
    mpp = _check_mpp(mpp, what)
    if band_rows is None and not region_u8.is_cuda:
        band_rows = DEFAULT_HOST_BAND
    bands = plan_stain_bands(H, H, band_rows)
    dev = gpu_device(what, region_u8)
    with torch.no_grad():
        src = BandSource(region_u8, max(r1 - r0 for _, _, r0, r1 in bands), dev)
        mask = torch.empty((1, H, W), dtype=torch.uint8, device=dev)
        tissue = torch.zeros((1,), dtype=torch.int64, device=dev)
        L = ops._L()
        for _, _, r0, r1 in bands:
            ptr, pitch = gpu_rows(src.rows(r0, r1))
            rc = L.s2s_stain_mask_u8(ptr, pitch, pitch * (r1 - r0), 1, r0, r1 - r0, H, W, table, unmix, white, black,
                                     stain, mask.data_ptr(), W, H * W, tissue.data_ptr(), ops._stream())
            _native.check(rc, what)
        res = _label(mask.data_ptr(), W, H * W, _FG_POSITIVE, 1, H, W, dev, connectivity, min_area, M, what)
        burden, per_mm2 = _density(res, tissue, mpp, what)
    out = _stain_dict(res, tissue, burden, per_mm2, M, return_labels)
    return {k: v[0] for k, v in out.items()}
