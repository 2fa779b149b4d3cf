"""Zonal stain quantification: the burden, the mean concentration and the objects of a stain per class of a zone map.

A pathologist reports the burden per anatomical or annotated zone: grey against white matter, tumour against stroma, the
class map of the multiclass mask head, a hand-drawn ROI, the first 100 um under the tissue edge.  A ZONE MAP is one byte
per pixel (uint8, bool accepted) next to the image: ``[B, H, W]`` for tiles, ``[H, W]`` for a region, any row pitch.  With
``num_zones`` = Z (1..256) a pixel whose byte is >= Z belongs to no zone: 255 is the ignore value for every Z <= 255, and
the number of such pixels is reported per owner as ``unzoned``.

  table[o][z]   = pixels, tissue, positive_0..2, sum q_0..2 of owner o's pixels with zone byte z
  positive_k    : tissue and c_k > thresholds[k], exactly as ``stain_quantify`` decides it
  q_k           = min((int)rintf(fmaxf(c_k, 0) * 1024), 4095), the grid of ``object_features`` (3.26).  Unlike there it
                  is summed over TISSUE pixels only, so that ``mean_conc`` is a mean over the same pixels the burden
                  divides by
  burden_k      = positive_k / max(tissue, 1);  mean_conc_k = (sum q_k / max(tissue, 1)) / 1024
  tissue_frac   = tissue / max(pixels, 1);      area_frac = pixels / (all pixels of the owner, unzoned included)

An owner is one sample, the whole batch (``pool=True``) or one whole region.  Every count is an exact integer and every
derived value a double formed by a fixed sequence of operations from those integers (include/stain2stain_hip.h), so
results are bit-equal for host and GPU input, for every banding, run to run, and equal to the numpy restatement of
tests/zonal_ref.py.  ``object_zones`` assigns every object of a label image to the zone that holds most of it;
``distance_zones`` turns a mask into bands of distance from its edge.  The calls launch on the current stream and wait
for nothing, so the batch forms can be captured.  GPU only.  DESIGN.md section 3.34.

The reference publishes no stain measurement: these numbers have no counterpart there.
"""
from __future__ import annotations

import ctypes
import math
import operator
from fractions import Fraction
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import _native, ops
from ._regionio import DEFAULT_HOST_BAND, BandSource, batch_layout, check_region, gpu_device, gpu_rows
from .image_metrics import _check_pair
from .morphology import FAR, _check_mask, distance_transform
from .object_features import _check_labels
from .objects import _check_mpp, _object_args, stain_objects
from .region import _check_thresholds
from .stain_quant import DEFAULT_THRESHOLDS, _image_kind, _kernel_args, _stain_index

MAX_ZONES = 256          # ZN_MAX_Z of csrc/zonal.hip: a zone is a byte
MAX_EDGES = 126          # ZN_MAX_EDGES: 2 n + 2 zones and 255 left for "no zone"
_SIDES = {"both": 0, "inside": 1, "outside": 2}


# ---- arguments -------------------------------------------------------------------------------------------------------
def _check_num_zones(num_zones, what: str) -> int:
    Z = operator.index(num_zones)
    if not 1 <= Z <= MAX_ZONES:
        raise ValueError(f"{what}: num_zones must lie in 1..{MAX_ZONES}, got {Z}")
    return Z


def _zone_bytes(zones, shape: Tuple[int, ...], what: str) -> torch.Tensor:
    """The zone map as a uint8 view of ``shape``."""
    if not isinstance(zones, torch.Tensor):
        raise TypeError(f"{what}: the zone map must be a torch.Tensor, got {type(zones).__name__}")
    if zones.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f"{what}: the zone map must be uint8 or bool, got {zones.dtype}")
    if tuple(zones.shape) != tuple(shape):
        raise ValueError(f"{what}: the zone map must be {list(shape)} like the image, got {list(zones.shape)}")
    zones = zones.detach()
    return zones.view(torch.uint8) if zones.dtype == torch.bool else zones


def _check_band_rows(band_rows, what: str) -> Optional[int]:
    if band_rows is None:
        return None
    band_rows = operator.index(band_rows)
    if band_rows < 1:
        raise ValueError(f"{what}: band_rows must be positive, got {band_rows}")
    return band_rows


def _region_bands(H: int, band_rows: Optional[int], any_host: bool):
    if band_rows is None:
        band_rows = DEFAULT_HOST_BAND if any_host else H
    return [(r0, min(r0 + band_rows, H)) for r0 in range(0, H, band_rows)]


_SINGLE, _PAIRED = 8, 6          # columns of the two tables


def _new(owners: int, Z: int, cols: int, dev, extra: Optional[dict] = None) -> Dict:
    res = {"counts": torch.empty((owners, Z, cols), dtype=torch.int64, device=dev),
           "unzoned": torch.empty((owners,), dtype=torch.int64, device=dev),
           "derived": torch.empty((owners, Z, 8 if cols == _SINGLE else 5), dtype=torch.float64, device=dev),
           "num_zones": Z}
    c, d = res["counts"], res["derived"]
    if cols == _SINGLE:
        res.update(pixels=c[..., 0], tissue=c[..., 1], positive=c[..., 2:5], sum_q=c[..., 5:8], burden=d[..., 0:3],
                   mean_conc=d[..., 3:6], tissue_frac=d[..., 6], area_frac=d[..., 7])
    else:
        res.update(pixels=c[..., 0], tissue_pred=c[..., 1], tissue_target=c[..., 2], both=c[..., 3], pred_only=c[..., 4],
                   target_only=c[..., 5], burden_pred=d[..., 0], burden_target=d[..., 1], burden_abs_err=d[..., 2],
                   dice=d[..., 3], iou=d[..., 4])
    if extra:
        res.update(extra)
    return res


def _check_out_type(out, what: str) -> None:
    if out is not None and not isinstance(out, dict):
        raise TypeError(f"{what}: out must be an earlier result of this call, got {type(out).__name__}")


def _check_out(out, owners: int, Z: int, cols: int, dev, what: str, extra: Optional[dict] = None) -> Dict:
    """An earlier result of the same call that this one adds into."""
    if not isinstance(out, dict) or any(k not in out for k in ("counts", "unzoned", "derived", "num_zones")):
        raise TypeError(f"{what}: out must be an earlier result of this call")
    c, u, d = out["counts"], out["unzoned"], out["derived"]
    ok = all(isinstance(t, torch.Tensor) and t.is_contiguous() for t in (c, u, d))
    if not ok or c.dtype != torch.int64 or tuple(c.shape) != (owners, Z, cols) or u.dtype != torch.int64 or \
            tuple(u.shape) != (owners,) or d.dtype != torch.float64 or tuple(d.shape[:2]) != (owners, Z):
        raise ValueError(f"{what}: out must hold int64 counts [{owners}, {Z}, {cols}] of {owners} owner(s) and {Z} zones")
    if c.device != dev:
        raise ValueError(f"{what}: out lives on {c.device}, the images on {dev}")
    for k, v in (extra or {}).items():
        if out.get(k) != v:
            raise ValueError(f"{what}: out was taken with another {k}")
    return out


def _finalize(res: Dict, paired: bool, what: str) -> None:
    c = res["counts"]
    rc = ops._L().s2s_zonal_finalize(c.data_ptr(), res["unzoned"].data_ptr(), c.shape[0], c.shape[1], int(paired),
                                     res["derived"].data_ptr(), ops._stream())
    _native.check(rc, what)


# ---- batches ---------------------------------------------------------------------------------------------------------
def _batch(images, zones, num_zones, stain, stains, thresholds, white, black, pool, out, what: str) -> Dict:
    paired = len(images) == 2
    if paired:
        _check_pair(images[0], images[1], what)
    kind, B, H, W = _image_kind(images[0], what)
    Z = _check_num_zones(num_zones, what)
    zones = _zone_bytes(zones, (B, H, W), what)
    extra = {"stain": _stain_index(stain)} if paired else None
    table, unmix = _kernel_args(stains, thresholds)
    white, black = _check_thresholds(white, black)
    _check_out_type(out, what)
    dev = gpu_device(what, *images, zones, host_ok=False)
    owners, cols = (1 if pool else B), (_PAIRED if paired else _SINGLE)
    L = ops._L()
    with torch.no_grad():
        if out is None:
            out, reset = _new(owners, Z, cols, dev, extra), 1
        else:
            out, reset = _check_out(out, owners, Z, cols, dev, what, extra), 0
        zones, zp, zs = batch_layout(zones, what, "the zone map", copy=True)
        tail = (table, unmix, white, black) + ((extra["stain"],) if paired else ()) + \
               (int(pool), reset, out["counts"].data_ptr(), out["unzoned"].data_ptr(), ops._stream())
        if kind == "f32":
            imgs = [t.detach().contiguous() for t in images]
            fn = L.s2s_zonal_pair_f32 if paired else L.s2s_zonal_f32
            rc = fn(*(t.data_ptr() for t in imgs), zones.data_ptr(), zp, zs, B, H, W, Z, *tail)
        else:
            lay = [batch_layout(t, what, copy=True) for t in images]
            fn = L.s2s_zonal_pair_u8 if paired else L.s2s_zonal_u8
            rc = fn(*(v for t, p, s in lay for v in (t.data_ptr(), p, s)), zones.data_ptr(), zp, zs, B, 0, H, H, W, Z,
                    *tail)
        _native.check(rc, what)
        _finalize(out, paired, what)
    return out


def stain_zonal(img: torch.Tensor, zones: torch.Tensor, num_zones: int, *, stains="hdab",
                thresholds: Sequence[float] = DEFAULT_THRESHOLDS, white: int = 220, black: int = 0, pool: bool = False,
                out: Optional[Dict] = None) -> Dict:
    """The stain burden per zone of uint8 ``[B, H, W, 3]`` (crop views and any row pitch allowed) or fp32
    ``[B, 3, H, W]`` (the network's range, through the save conversion) images on the GPU, with the zone map ``zones``
    uint8 or bool ``[B, H, W]`` (any row pitch) and ``num_zones`` = Z in 1..256; a byte >= Z is no zone.

    Returns device tensors for O owners (B, or 1 with ``pool``: the whole batch): ``"counts"`` int64 ``[O, Z, 8]`` =
    pixels, tissue, positive_0..2, sum_q_0..2 and ``"unzoned"`` int64 ``[O]``; the views ``"pixels"``, ``"tissue"``
    ``[O, Z]``, ``"positive"``, ``"sum_q"`` ``[O, Z, 3]``; fp64 ``"burden"`` = positive / max(tissue, 1) and
    ``"mean_conc"`` = (sum_q / max(tissue, 1)) / 1024 ``[O, Z, 3]``, ``"tissue_frac"`` = tissue / max(pixels, 1) and
    ``"area_frac"`` = pixels / (the owner's pixels, unzoned included) ``[O, Z]``.  ``sum_q`` is the sum over the zone's
    TISSUE pixels of ``q_k = min(rint(max(c_k, 0) * 1024), 4095)``: the grid of ``object_features``, which sums it over
    every pixel of an object; here ``mean_conc`` is a mean over the same pixels the burden divides by.  A zone without
    pixels gives zeros, never NaN.  ``out=z`` adds into an earlier result of the same shape and returns it (a
    dataset-level table over a validation loader: ``z = stain_zonal(batch, zones, Z, pool=True, out=z)`` per batch; an
    owner may hold 2^40 pixels).  ``stains``, ``thresholds``, ``white``, ``black`` as ``stain_quantify``; the default
    thresholds are a convention, calibrate them on your own slides.  One counting launch and one finalize on the current
    stream (one more without ``out``: it zeroes the table), no host synchronisation; bit-reproducible, and a sample's
    table does not depend on its batch mates."""
    return _batch((img,), zones, num_zones, 0, stains, thresholds, white, black, pool, out, "stain_zonal")


def stain_zonal_agreement(pred: torch.Tensor, target: torch.Tensor, zones: torch.Tensor, num_zones: int, *,
                          stain: int = 1, stains="hdab", thresholds: Sequence[float] = DEFAULT_THRESHOLDS,
                          white: int = 220, black: int = 0, pool: bool = False, out: Optional[Dict] = None) -> Dict:
    """``stain_agreement`` per zone: how well a generated stain agrees with the real one on what is positive for stain
    ``stain``, over one shared zone map.  Inputs as ``stain_zonal``, both images of one kind and shape.

    ``"counts"`` int64 ``[O, Z, 6]`` = pixels, tissue_pred, tissue_target, positive in both, in the prediction only, in
    the target only (also as the views ``"pixels"``, ``"tissue_pred"``, ``"tissue_target"``, ``"both"``,
    ``"pred_only"``, ``"target_only"``), ``"unzoned"`` int64 ``[O]`` and fp64 ``[O, Z]``: ``"burden_pred"``,
    ``"burden_target"``, ``"burden_abs_err"``, ``"dice"`` and ``"iou"`` of the two positive masks inside the zone, double
    quotients of the integers, 1 where the denominator is 0 (the convention of ``stain_agreement``).  ``out=`` adds into
    an earlier result taken with the same ``stain``.  One fused launch reads both images and the map once."""
    return _batch((pred, target), zones, num_zones, stain, stains, thresholds, white, black, pool, out,
                  "stain_zonal_agreement")


# ---- regions ---------------------------------------------------------------------------------------------------------
def _region(images, zones, num_zones, band_rows, stain, stains, thresholds, white, black, out, what: str, stats_of):
    paired = len(images) == 2
    if paired:
        _check_pair(images[0], images[1], what)
    H, W, _ = check_region(images[0], what)
    for t in images[1:]:
        check_region(t, what)
    Z = _check_num_zones(num_zones, what)
    zones = _zone_bytes(zones, (H, W), what)
    check_region(zones, what, mask_ok=True)
    band_rows = _check_band_rows(band_rows, what)
    extra = {"stain": _stain_index(stain)} if paired else None
    table, unmix = _kernel_args(stains, thresholds)
    white, black = _check_thresholds(white, black)
    _check_out_type(out, what)
    dev = gpu_device(what, *images, zones)
    bands = _region_bands(H, band_rows, not all(t.is_cuda for t in (*images, zones)))
    buf_rows = max(r1 - r0 for r0, r1 in bands)
    cols = _PAIRED if paired else _SINGLE
    L = ops._L()
    fn = L.s2s_zonal_pair_u8 if paired else L.s2s_zonal_u8
    with torch.no_grad():
        if out is None:
            out, reset = _new(1, Z, cols, dev, extra), 1
        else:
            out, reset = _check_out(out, 1, Z, cols, dev, what, extra), 0
        src = [BandSource(t, buf_rows, dev) for t in (*images, zones)]
        for r0, r1 in bands:
            n = r1 - r0
            views = [gpu_rows(s.rows(r0, r1)) for s in src]
            rc = fn(*(v for ptr, pitch in views for v in (ptr, pitch, pitch * n)), 1, r0, n, H, W, Z, table, unmix, white,
                    black, *((extra["stain"],) if paired else ()), 0, reset, out["counts"].data_ptr(),
                    out["unzoned"].data_ptr(), ops._stream())
            _native.check(rc, what)
            reset = 0
        _finalize(out, paired, what)
    stats_of.last_stats = {"bands": len(bands), "band_rows": buf_rows, "band_bytes": sum(s.band_bytes for s in src)}
    return out


def region_stain_zonal(region_u8: torch.Tensor, zones_u8: torch.Tensor, num_zones: int, *,
                       band_rows: Optional[int] = None, stains="hdab", thresholds: Sequence[float] = DEFAULT_THRESHOLDS,
                       white: int = 220, black: int = 0, out: Optional[Dict] = None) -> Dict:
    """``stain_zonal`` of one whole uint8 ``[H, W, 3]`` region with its ``[H, W]`` zone map, each on the GPU or on the
    host, any row pitch: one owner, the tensors of ``stain_zonal`` with O = 1, on the GPU.  A host region or map is
    streamed through one pinned buffer and one GPU band buffer of ``band_rows`` rows each (``None``: everything on the
    GPU in one launch, otherwise bands of 512 rows); the bands add up in integers, so the result is bit-equal for every
    ``band_rows`` >= 1 and for host and GPU input, and equal to ``stain_zonal(region[None], zones[None], Z)``.  ``out=``
    adds into an earlier result (several regions of one slide).  ``region_stain_zonal.last_stats``: bands, band_rows,
    band_bytes of the last call."""
    return _region((region_u8,), zones_u8, num_zones, band_rows, 0, stains, thresholds, white, black, out,
                   "region_stain_zonal", region_stain_zonal)


region_stain_zonal.last_stats: Optional[Dict[str, int]] = None


def region_stain_zonal_agreement(pred_u8: torch.Tensor, target_u8: torch.Tensor, zones_u8: torch.Tensor, num_zones: int,
                                 *, band_rows: Optional[int] = None, stain: int = 1, stains="hdab",
                                 thresholds: Sequence[float] = DEFAULT_THRESHOLDS, white: int = 220, black: int = 0,
                                 out: Optional[Dict] = None) -> Dict:
    """``stain_zonal_agreement`` of one whole uint8 ``[H, W, 3]`` region pair over one ``[H, W]`` zone map (each of the
    three on the GPU or on the host, any row pitch): one owner.  Banding and its bit equality as
    ``region_stain_zonal``."""
    return _region((pred_u8, target_u8), zones_u8, num_zones, band_rows, stain, stains, thresholds, white, black, out,
                   "region_stain_zonal_agreement", region_stain_zonal_agreement)


region_stain_zonal_agreement.last_stats: Optional[Dict[str, int]] = None


# ---- objects by zone ---------------------------------------------------------------------------------------------------
def _check_max_objects(max_objects, B: int, Z: int, what: str) -> int:
    M = operator.index(max_objects)
    if M < 1:
        raise ValueError(f"{what}: max_objects must be at least 1, got {M}")
    if B * M * Z >= 2 ** 31:
        raise ValueError(f"{what}: B * max_objects * num_zones = {B * M * Z} must stay below 2^31")
    return M


def object_zones(labels: torch.Tensor, zones: torch.Tensor, num_zones: int, *, max_objects: int = 256,
                 return_overlap: bool = False) -> Dict[str, torch.Tensor]:
    """The zone of every object of a label image: ``labels`` int32 ``[B, H, W]`` (or ``[H, W]``) on the GPU as
    ``label_components``, ``split_objects`` and ``stain_objects`` write them (0 background, objects 1..count; labels above
    ``max_objects`` = M are not tabulated, ``count`` is the largest label seen), ``zones`` a zone map of the same shape.

    The zone of an object is the one that holds most of its pixels, ties to the smaller zone; -1 when none of its
    pixels has a zone.  Returns device tensors: ``"zone"`` int32 ``[B, M]`` (-1 in rows at or beyond min(count, M)),
    ``"zone_pixels"`` int64 ``[B, M]`` (the object's pixels inside its zone), ``"area"`` int32 ``[B, M]`` (all its pixels),
    ``"count"`` int32 ``[B]``, and per zone ``"objects"`` int64 ``[B, Z]`` (objects assigned to it) and
    ``"object_pixels"`` int64 ``[B, Z]`` (the sum of their full areas, pixels outside the zone included);
    ``return_overlap`` adds ``"overlap"`` int32 ``[B, M, Z]``, the pixels of object m + 1 in zone z.  Without a batch
    dimension the leading ``B`` is dropped.  Every choice is a maximum over a strict order of integers: exact, and the
    same run to run.  Two launches after the zeroing, no host synchronisation."""
    what = "object_zones"
    B, H, W = _check_labels(labels, what)
    Z = _check_num_zones(num_zones, what)
    zones = _zone_bytes(zones, tuple(labels.shape), what)
    M = _check_max_objects(max_objects, B, Z, what)
    dev = gpu_device(what, labels, zones, host_ok=False)
    L = ops._L()
    with torch.no_grad():
        lab = labels.detach().contiguous()
        zb, zp, zs = batch_layout(zones if zones.dim() == 3 else zones[None], what, "the zone map", copy=True)
        overlap = torch.zeros((B, M, Z), dtype=torch.int32, device=dev)
        area = torch.zeros((B, M), dtype=torch.int32, device=dev)
        count = torch.zeros((B,), dtype=torch.int32, device=dev)
        per_zone = torch.zeros((2, B, Z), dtype=torch.int64, device=dev)
        zone = torch.empty((B, M), dtype=torch.int32, device=dev)
        zone_pixels = torch.empty((B, M), dtype=torch.int64, device=dev)
        _native.check(L.s2s_zonal_object_overlap(lab.data_ptr(), zb.data_ptr(), zp, zs, B, H, W, Z, M, overlap.data_ptr(),
                                                 area.data_ptr(), count.data_ptr(), ops._stream()), what)
        _native.check(L.s2s_zonal_object_assign(overlap.data_ptr(), area.data_ptr(), count.data_ptr(), B, Z, M,
                                                zone.data_ptr(), zone_pixels.data_ptr(), per_zone[0].data_ptr(),
                                                per_zone[1].data_ptr(), ops._stream()), what)
    res = {"zone": zone, "zone_pixels": zone_pixels, "area": area, "count": count, "objects": per_zone[0],
           "object_pixels": per_zone[1]}
    if return_overlap:
        res["overlap"] = overlap
    return res if labels.dim() == 3 else {k: v[0] for k, v in res.items()}


def stain_zonal_objects(img: torch.Tensor, zones: torch.Tensor, num_zones: int, *, stain: int = 1, stains="hdab",
                        thresholds: Sequence[float] = DEFAULT_THRESHOLDS, white: int = 220, black: int = 0,
                        connectivity: int = 8, min_area: int = 1, max_objects: int = 256,
                        mpp: Optional[float] = None) -> Dict:
    """Burden and objects per zone in one call: ``stain_zonal(img, zones, Z)`` (one owner per sample), the positive
    objects of stain ``stain`` as ``stain_objects`` labels them (``connectivity``, ``min_area``), and their zones as
    ``object_zones`` assigns them (``max_objects``).

    Returns ``stain_zonal``'s keys and ``"objects"``, ``"object_pixels"`` int64 ``[B, Z]``, ``"count"`` int32 ``[B]``
    (all objects, as ``stain_objects`` counts them), ``"zone"`` and ``"zone_pixels"`` ``[B, M]``.  With ``mpp``
    (micrometres per pixel) also ``"per_mm2"`` fp64 ``[B, Z]`` = (double)objects / ((double)tissue * (mpp * mpp * 1e-6)),
    the objects per square millimetre of the zone's tissue, 0 where the zone has no tissue.  Objects beyond
    ``max_objects`` are counted in ``count`` but assigned to no zone.  No host synchronisation."""
    what = "stain_zonal_objects"
    mpp = _check_mpp(mpp, what)
    _, B, _, _ = _image_kind(img, what)
    Z = _check_num_zones(num_zones, what)
    _check_max_objects(max_objects, B, Z, what)
    _object_args(connectivity, min_area, None, what)
    res = stain_zonal(img, zones, Z, stains=stains, thresholds=thresholds, white=white, black=black)
    obj = stain_objects(img, stain=stain, stains=stains, thresholds=thresholds, white=white, black=black,
                        connectivity=connectivity, min_area=min_area, return_labels=True)
    oz = object_zones(obj["labels"], zones, Z, max_objects=max_objects)
    res.update(objects=oz["objects"], object_pixels=oz["object_pixels"], zone=oz["zone"], zone_pixels=oz["zone_pixels"],
               count=obj["count"])
    if mpp is not None:
        with torch.no_grad():
            per_mm2 = torch.empty((B, Z), dtype=torch.float64, device=res["counts"].device)
            scale = (ctypes.c_double * 1)(mpp * mpp * 1e-6)
            rc = ops._L().s2s_zonal_object_density(res["objects"].data_ptr(), res["counts"].data_ptr(), B, Z, scale,
                                                   per_mm2.data_ptr(), ops._stream())
            _native.check(rc, what)
        res["per_mm2"] = per_mm2
    return res


# ---- distance bands ----------------------------------------------------------------------------------------------------
def squared_edges(edges, what: str = "distance_zones") -> Tuple[int, ...]:
    """``E_i = floor(e_i^2)`` as Python integers for a strictly ascending list of 1..126 distances ``e_i >= 0`` in
    pixels; each must stay below ``FAR`` = 2^31 - 1.  Formed exactly (2.5 -> 6)."""
    try:
        es = [float(e) for e in edges]
    except (TypeError, ValueError):
        raise ValueError(f"{what}: edges must be a sequence of numbers, got {edges!r}") from None
    if not 1 <= len(es) <= MAX_EDGES:
        raise ValueError(f"{what}: edges must hold 1..{MAX_EDGES} distances, got {len(es)}")
    if not all(math.isfinite(e) and e >= 0.0 for e in es) or any(b <= a for a, b in zip(es, es[1:])):
        raise ValueError(f"{what}: edges must be finite, not negative and strictly ascending, got {edges!r}")
    E = tuple(int(Fraction(e) ** 2) for e in es)
    if E[-1] >= FAR:
        raise ValueError(f"{what}: floor(edge^2) must stay below 2^31 - 1, got an edge of {es[-1]}")
    return E


def distance_zones(mask: torch.Tensor, edges: Sequence[float], side: str = "both") -> Tuple[torch.Tensor, int]:
    """A zone map of distance bands around the edge of a bool or uint8 (nonzero = foreground) mask ``[B, H, W]`` or
    ``[H, W]``: ``(zones, num_zones)`` with ``zones`` uint8 of the mask's shape and ``num_zones`` = 2 n + 2 for the n
    ``edges`` (strictly ascending distances in pixels, 1 <= n <= 126).

    With ``E_i = floor(e_i^2)`` and the exact squared distances of ``distance_transform``: a foreground pixel gets
    ``#{i : d2_to_background > E_i}``, zones 0..n from the rim inwards; a background pixel gets
    ``n + 1 + #{i : d2_to_foreground > E_i}``, zones n + 1..2 n + 1 from the rim outwards.  A sample without background
    (or foreground) has the distance ``FAR``, which exceeds every ``E_i``: the deepest band.  ``side="inside"`` writes
    255 (no zone) on the background, ``"outside"`` on the foreground.  ``distance_zones(tissue, [100 / mpp],
    side="inside")`` is zone 0 = the first 100 um under the tissue edge, zone 1 = the rest.  A host mask is uploaded
    whole and the map comes back to the host.  Two distance transforms and one launch, no host synchronisation."""
    what = "distance_zones"
    B, H, W = _check_mask(mask, what)
    if side not in _SIDES:
        raise ValueError(f"{what}: side must be one of {', '.join(map(repr, _SIDES))}, got {side!r}")
    E = squared_edges(edges, what)
    dev = gpu_device(what, mask)
    with torch.no_grad():
        m = mask.detach() if mask.is_cuda else mask.detach().to(dev)
        d_bg, d_fg = distance_transform(m, "background").contiguous(), distance_transform(m, "foreground").contiguous()
        out = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
        rc = ops._L().s2s_zonal_bands(d_bg.data_ptr(), d_fg.data_ptr(), B, H, W, (ctypes.c_int * len(E))(*E), len(E),
                                      _SIDES[side], out.data_ptr(), ops._stream())
        _native.check(rc, what)
    out = out if mask.dim() == 3 else out[0]
    return (out if mask.is_cuda else out.to(mask.device)), 2 * len(E) + 2
