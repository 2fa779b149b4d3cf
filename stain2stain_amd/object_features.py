"""Stain object morphometry: per-object shape, thickness and stain intensity on the GPU.

``stain_objects`` says how many plaques there are, how large each is and where it sits.  What a stain is read for goes
one step further: is an object compact or diffuse, round or elongated, densely or faintly stained, how thick is its
core, and is it cut by the tile edge.  Per object numbered 1..M of a label image (``label_components``):

  area, bbox     pixels; ``y0, x0, y1, x1`` end-exclusive
  moments        the sums of y, x, y^2, x^2 and yx over the pixels
  edges          the crack length: the pairs (pixel of the object, one of its four neighbours) whose neighbour carries
                 another label or lies outside the image
  boundary       the object's pixels with at least one such neighbour (``mask_boundary`` of the object alone)
  border         1 iff the object has a pixel in the first or last row or column
  max_d2         the largest squared distance from a pixel of the object to the nearest pixel whose label is 0
  sum_q, ...     sum, sum of squares and maximum of q = min(rint(max(c, 0) * 1024), 4095), c the fp32 concentration of
                 ``stain_separate``: the 1/1024 grid of the concentration histograms; no tissue gate
  derived        fp64, from exact integer numerators: centroid, equivalent diameter, central second moments per pixel,
                 major / minor axis, eccentricity, orientation, compactness, mean / std / max concentration, inscribed
                 radius

Every table is an integer accumulated by integer atomics, so the results are exact and bit-reproducible; the derived
values follow one fixed order of operations (include/stain2stain_hip.h).  The kernels are ``csrc/object_features.hip``: a
wave finds its distinct labels by ballot, a workgroup gathers them in an LDS table of ``LDS_SLOTS`` labels, one set of
64-bit atomics per workgroup and label reaches memory.  ``H, W <= MAX_SIDE`` = 32767 and ``B <= 65535``.  GPU only.
DESIGN.md section 3.26.

The reference publishes no object measurement: these numbers have no counterpart there.
"""
from __future__ import annotations

import operator
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import _native, ops
from ._regionio import DEFAULT_HOST_BAND, BandSource, batch_layout, check_region, gpu_device, gpu_rows
from .morphology import FAR, MAX_SIDE, distance_transform
from .objects import (_FG_POSITIVE, _check_mpp, _density, _label, _object_args, _stain_dict, _stain_mask)
from .region import _check_thresholds
from .stain_quant import DEFAULT_THRESHOLDS, _image_kind, _kernel_args, _stain_index, plan_stain_bands

TILE = (64, 64)              # rows x columns of the shape pass's workgroup tile: OF_TH, OF_TW of csrc/object_features.hip
LDS_SLOTS = 64               # labels a workgroup gathers in LDS before it falls back to global atomics: OF_SLOTS
N_DERIVED = 15               # fp64 values per object: OF_NF
# name -> column(s) of the finalize's [B, M, N_DERIVED] table
_DERIVED = {"centroid": slice(0, 2), "equivalent_diameter": 2, "mu_yy": 3, "mu_xx": 4, "mu_yx": 5, "major_axis": 6,
            "minor_axis": 7, "eccentricity": 8, "orientation": 9, "compactness": 10}
_DERIVED_INTENSITY = {"mean_conc": 11, "std_conc": 12, "max_conc": 13}
_DERIVED_THICKNESS = {"inscribed_radius": 14}
_UM = ("equivalent_diameter", "major_axis", "minor_axis", "inscribed_radius")
_SUMMARY = ("eccentricity", "compactness", "mean_conc", "inscribed_radius")


def _check_labels(labels, what: str) -> Tuple[int, int, int]:
    if not isinstance(labels, torch.Tensor):
        raise TypeError(f"{what}: labels must be a torch.Tensor, got {type(labels).__name__}")
    if labels.dtype != torch.int32:
        raise ValueError(f"{what}: labels must be int32, got {labels.dtype}")
    if labels.dim() not in (2, 3):
        raise ValueError(f"{what}: labels must be [B, H, W] or [H, W], got {list(labels.shape)}")
    B = int(labels.shape[0]) if labels.dim() == 3 else 1
    H, W = int(labels.shape[-2]), int(labels.shape[-1])
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"{what}: empty label image {list(labels.shape)}")
    if B > 65535:
        raise ValueError(f"{what}: at most 65535 samples, got {B}")
    _check_sides(H, W, what)
    return B, H, W


def _check_sides(H: int, W: int, what: str) -> None:
    if H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError(f"{what}: {H} x {W} exceeds the limit of {MAX_SIDE} pixels a side")


def _check_max_objects(max_objects, B: int, what: str) -> int:
    M = operator.index(max_objects)
    if M < 1 or B * M > 2 ** 31 - 1:
        raise ValueError(f"{what}: max_objects must be at least 1 (and B * max_objects below 2^31), got {M}")
    return M


def _check_image(image, labels: torch.Tensor, B: int, H: int, W: int, what: str) -> Tuple[torch.Tensor, str]:
    """The image as a batch of B (a [H, W] label image takes [H, W, 3] / [3, H, W] or a batch of one) and its kind."""
    if not isinstance(image, torch.Tensor):
        raise TypeError(f"{what}: image must be a torch.Tensor, got {type(image).__name__}")
    if labels.dim() == 2 and image.dim() == 3:
        image = image[None]
    kind, Bi, Hi, Wi = _image_kind(image, what)
    if (Bi, Hi, Wi) != (B, H, W):
        raise ValueError(f"{what}: image {list(image.shape)} does not match labels {list(labels.shape)}")
    return image, kind


def _tables(dev, B: int, M: int, intensity: bool, thickness: bool) -> Dict[str, torch.Tensor]:
    """The zeroed integer tables, one dense tensor per quantity (the kernels index them as [B][M][...])."""
    z = lambda *shape, dtype: torch.zeros(shape, dtype=dtype, device=dev)
    t = {"count": z(B, dtype=torch.int32), "area": z(B, M, dtype=torch.int64), "bbox": z(B, M, 4, dtype=torch.int32),
         "moments": z(B, M, 5, dtype=torch.int64), "edges": z(B, M, dtype=torch.int64),
         "boundary": z(B, M, dtype=torch.int64), "border": z(B, M, dtype=torch.int32)}
    if thickness:
        t["max_d2"] = z(B, M, dtype=torch.int32)
    if intensity:
        t.update(sum_q=z(B, M, dtype=torch.int64), sum_q2=z(B, M, dtype=torch.int64), max_q=z(B, M, dtype=torch.int32))
    return t


def _shape_pass(labels: torch.Tensor, d2: Optional[torch.Tensor], t: Dict[str, torch.Tensor], B: int, H: int, W: int,
                M: int, what: str) -> None:
    rc = ops._L().s2s_objfeat_shape(labels.data_ptr(), d2.data_ptr() if d2 is not None else 0, B, H, W, M,
                                    t["count"].data_ptr(), t["area"].data_ptr(), t["bbox"].data_ptr(),
                                    t["moments"].data_ptr(), t["edges"].data_ptr(), t["boundary"].data_ptr(),
                                    t["border"].data_ptr(), t["max_d2"].data_ptr() if d2 is not None else 0, ops._stream())
    _native.check(rc, what)


def _intensity_pass(labels: torch.Tensor, image: torch.Tensor, kind: str, t: Dict[str, torch.Tensor], B: int, H: int,
                    W: int, M: int, table, unmix, stain: int, what: str) -> None:
    L = ops._L()
    if kind == "f32":
        a = image.detach().contiguous()
        rc = L.s2s_objfeat_intensity_f32(labels.data_ptr(), a.data_ptr(), B, H, W, M, table, unmix, stain,
                                         t["sum_q"].data_ptr(), t["sum_q2"].data_ptr(), t["max_q"].data_ptr(),
                                         ops._stream())
    else:
        a, pitch, stride = batch_layout(image, what, copy=True)
        rc = L.s2s_objfeat_intensity_u8(labels.data_ptr(), a.data_ptr(), pitch, stride, B, 0, H, H, W, M, table, unmix,
                                        stain, t["sum_q"].data_ptr(), t["sum_q2"].data_ptr(), t["max_q"].data_ptr(),
                                        ops._stream())
    _native.check(rc, what)


def _finalize(t: Dict[str, torch.Tensor], B: int, M: int, mpp: Optional[float], what: str) -> Dict[str, torch.Tensor]:
    """The integer tables -> the result dict [B, ...] with the fp64 derived values (and the micrometre keys)."""
    dev = t["count"].device
    intensity, thickness = "sum_q" in t, "max_d2" in t
    out = torch.empty((B, M, N_DERIVED), dtype=torch.float64, device=dev)
    rc = ops._L().s2s_objfeat_finalize(t["count"].data_ptr(), t["area"].data_ptr(), t["moments"].data_ptr(),
                                       t["edges"].data_ptr(), t["sum_q"].data_ptr() if intensity else 0,
                                       t["sum_q2"].data_ptr() if intensity else 0,
                                       t["max_q"].data_ptr() if intensity else 0,
                                       t["max_d2"].data_ptr() if thickness else 0, B, M, out.data_ptr(), ops._stream())
    _native.check(rc, what)
    res = dict(t)
    cols = dict(_DERIVED)
    if intensity:
        cols.update(_DERIVED_INTENSITY)
    if thickness:
        cols.update(_DERIVED_THICKNESS)
    for name, c in cols.items():
        res[name] = out[:, :, c]
    if mpp is not None:
        res["area_um2"] = t["area"].to(torch.float64) * (mpp * mpp)
        for name in _UM:
            if name in res:
                res[name + "_um"] = res[name] * mpp
    return res


def _features(labels: torch.Tensor, image, kind, B: int, H: int, W: int, M: int, table, unmix, stain: int,
              thickness: bool, mpp: Optional[float], what: str) -> Dict[str, torch.Tensor]:
    """labels: int32 [B, H, W], contiguous, on the GPU."""
    dev = labels.device
    t = _tables(dev, B, M, image is not None, thickness)
    d2 = distance_transform(labels > 0, to="background") if thickness else None
    _shape_pass(labels, d2, t, B, H, W, M, what)
    if image is not None:
        _intensity_pass(labels, image, kind, t, B, H, W, M, table, unmix, stain, what)
    return _finalize(t, B, M, mpp, what)


def object_features(labels: torch.Tensor, max_objects: int = 256, image: Optional[torch.Tensor] = None, stain: int = 1,
                    stains="hdab", thickness: bool = True, mpp: Optional[float] = None) -> Dict[str, torch.Tensor]:
    """Per-object shape, thickness and stain intensity of a label image: ``labels`` int32 ``[B, H, W]`` or ``[H, W]`` on
    the GPU, 0 = background, objects 1..count as ``label_components`` numbers them (any label image works: ``"count"`` is
    its largest label).  The first M = ``max_objects`` objects are tabulated; an object numbered above M is left out but
    still counts as a different label for its neighbours.

    Returns device tensors, ``[B, M, ...]`` (without a batch dimension the leading B is dropped); rows at or beyond
    ``min(count, M)`` are zero:

      ``"count"`` int32 ``[B]``; ``"area"`` int64; ``"bbox"`` int32 ``[.., 4]`` (y0, x0, y1, x1, end-exclusive);
      ``"moments"`` int64 ``[.., 5]`` (sums of y, x, y^2, x^2, yx); ``"edges"`` int64, the crack length; ``"boundary"``
      int64, the pixels with a 4-neighbour of another label or outside the image; ``"border"`` int32, 1 iff the object
      touches the first or last row or column (such an object is cut by the tile: ``object_feature_summary`` leaves it
      out);
      fp64 ``"centroid"`` ``[.., 2]`` (y, x), ``"equivalent_diameter"`` = sqrt(4 area / pi), ``"mu_yy"``, ``"mu_xx"``,
      ``"mu_yx"`` (central second moments per pixel), ``"major_axis"`` = 4 sqrt(l1) and ``"minor_axis"`` = 4 sqrt(l2)
      of the moment matrix's eigenvalues l1 >= l2, ``"eccentricity"`` = sqrt(1 - l2 / l1) (0 for a single pixel),
      ``"orientation"`` = 0.5 atan2(2 mu_yx, mu_xx - mu_yy): the angle of the major axis from the column axis toward
      increasing rows, in (-pi/2, pi/2], 0 for an isotropic object, and ``"compactness"`` = 4 pi area / edges^2.

    The moments are those of the pixel centres: NO 1/12 pixel-extent term is added, which is the convention of
    ``skimage.measure.regionprops`` (a single pixel has axes 0, an a x b rectangle mu_yy = (a^2 - 1) / 12).  The crack
    length overestimates a smooth perimeter (by 4 / pi for a large disc: 8 r against 2 pi r), so a digital disc scores a compactness below
    1 (about pi^2 / 16 = 0.62); the value is not clamped.

    ``thickness=True`` adds ``"max_d2"`` int32 and ``"inscribed_radius"`` fp64 = sqrt(max_d2): the largest distance from
    a pixel of the object to the nearest pixel whose label is 0, from ``distance_transform(labels > 0)``.  With
    connectivity-4 labels a diagonally adjacent other object is NOT background, so two such objects are measured as one
    body; a sample without any zero label gives ``FAR`` and ``inf``.

    ``image`` (uint8 ``[B, H, W, 3]`` or fp32 ``[B, 3, H, W]`` of the labels' shape, as ``stain_quantify``) adds
    ``"sum_q"``, ``"sum_q2"`` int64, ``"max_q"`` int32 of q = min(rint(max(c, 0) * 1024), 4095), c the concentration of
    stain ``stain`` under ``stains``, over every pixel of the object (no tissue gate), and fp64 ``"mean_conc"``,
    ``"std_conc"`` (population) and ``"max_conc"`` in concentration units.

    ``mpp`` (micrometres per pixel) adds ``"area_um2"``, ``"equivalent_diameter_um"``, ``"major_axis_um"``,
    ``"minor_axis_um"`` and ``"inscribed_radius_um"``.  Exact and bit-reproducible integers; a sample's values do not
    depend on its batch mates; three launches plus the distance transform's four and one per image; no host
    synchronisation."""
    what = "object_features"
    B, H, W = _check_labels(labels, what)
    M = _check_max_objects(max_objects, B, what)
    mpp = _check_mpp(mpp, what)
    kind = table = unmix = None
    if image is not None:
        image, kind = _check_image(image, labels, B, H, W, what)
        stain = _stain_index(stain)
        table, unmix = _kernel_args(stains, DEFAULT_THRESHOLDS)
    dev = gpu_device(what, labels, *([image] if image is not None else []), host_ok=False)
    with torch.no_grad():
        lab = labels.detach()
        lab = (lab if lab.dim() == 3 else lab[None]).contiguous()
        res = _features(lab, image, kind, B, H, W, M, table, unmix, stain, bool(thickness), mpp, what)
    return res if labels.dim() == 3 else {k: v[0] for k, v in res.items()}


def stain_object_features(img: torch.Tensor, max_objects: int = 256, stain: int = 1, stains="hdab",
                          thresholds: Sequence[float] = DEFAULT_THRESHOLDS, white: int = 220, black: int = 0,
                          connectivity: int = 8, min_area: int = 1, thickness: bool = True, mpp: Optional[float] = None,
                          return_labels: bool = False) -> Dict[str, torch.Tensor]:
    """The stain mask, the labelling and ``object_features`` in one call on uint8 ``[B, H, W, 3]`` or fp32
    ``[B, 3, H, W]`` images on the GPU: the keys of ``object_features(labels, max_objects, image=img, ...)`` (the
    integer ``"area"`` int64, ``"bbox"`` and fp64 ``"centroid"`` are this module's) plus the per-sample keys of
    ``stain_objects``: ``"tissue"``, ``"positive"``, ``"burden"``, ``"largest"``, ``"size_hist"``, ``"per_mm2"`` with
    ``mpp`` and ``"labels"`` on request.  Arguments as ``stain_objects``."""
    what = "stain_object_features"
    kind, B, H, W = _image_kind(img, what)
    _check_sides(H, W, what)
    if B > 65535:
        raise ValueError(f"{what}: at most 65535 samples, got {B}")
    M = _check_max_objects(max_objects, B, what)
    stain = _stain_index(stain)
    table, unmix = _kernel_args(stains, thresholds)
    white, black = _check_thresholds(white, black)
    connectivity, min_area, _ = _object_args(connectivity, min_area, None, what)
    mpp = _check_mpp(mpp, what)
    dev = gpu_device(what, img, host_ok=False)
    with torch.no_grad():
        mask, tissue = _stain_mask(img, kind, B, H, W, table, unmix, white, black, stain, what)
        res = _label(mask.data_ptr(), W, H * W, _FG_POSITIVE, B, H, W, dev, connectivity, min_area, 0, what)
        burden, per_mm2 = _density(res, tissue, mpp, what)
        out = _stain_dict(res, tissue, burden, per_mm2, 0, return_labels)
        out.update(_features(res["labels"], img, kind, B, H, W, M, table, unmix, stain, bool(thickness), mpp, what))
    return out


def region_stain_object_features(region_u8: torch.Tensor, max_objects: int = 4096, band_rows: Optional[int] = None,
                                 stain: int = 1, stains="hdab", thresholds: Sequence[float] = DEFAULT_THRESHOLDS,
                                 white: int = 220, black: int = 0, connectivity: int = 8, min_area: int = 1,
                                 thickness: bool = True, mpp: Optional[float] = None,
                                 return_labels: bool = False) -> Dict[str, torch.Tensor]:
    """``stain_object_features`` over one whole uint8 ``[H, W, 3]`` region on the GPU or on the host (any row pitch),
    without the batch dimension.  The byte mask is built band by band and labelled once, as in
    ``region_stain_objects``; the shape and thickness passes run over the whole label image; the intensity pass runs
    band by band through the same band source, its integer sums accumulating across the bands, so a host region never
    sits on the GPU as RGB.  The result is bit-equal for every ``band_rows`` and for host and GPU input."""
    what = "region_stain_object_features"
    H, W, _ = check_region(region_u8, what)
    _check_sides(H, W, what)
    M = _check_max_objects(max_objects, 1, what)
    stain = _stain_index(stain)
    table, unmix = _kernel_args(stains, thresholds)
    white, black = _check_thresholds(white, black)
    connectivity, min_area, _ = _object_args(connectivity, min_area, None, what)
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
        res = _label(mask.data_ptr(), W, H * W, _FG_POSITIVE, 1, H, W, dev, connectivity, min_area, 0, what)
        burden, per_mm2 = _density(res, tissue, mpp, what)
        out = _stain_dict(res, tissue, burden, per_mm2, 0, return_labels)
        labels = res["labels"]
        t = _tables(dev, 1, M, True, bool(thickness))
        d2 = distance_transform(labels > 0, to="background") if thickness else None
        _shape_pass(labels, d2, t, 1, H, W, M, what)
        for _, _, r0, r1 in bands:
            ptr, pitch = gpu_rows(src.rows(r0, r1))
            rc = L.s2s_objfeat_intensity_u8(labels.data_ptr(), ptr, pitch, pitch * (r1 - r0), 1, r0, r1 - r0, H, W, M,
                                            table, unmix, stain, t["sum_q"].data_ptr(), t["sum_q2"].data_ptr(),
                                            t["max_q"].data_ptr(), ops._stream())
            _native.check(rc, what)
        out.update(_finalize(t, 1, M, mpp, what))
    return {k: v[0] for k, v in out.items()}


def object_feature_summary(f: Dict[str, torch.Tensor], exclude_border: bool = True) -> Dict[str, torch.Tensor]:
    """Per-sample summaries of a feature table (the dict of ``object_features`` and its relatives), as device tensors
    ``[B]`` (scalars without a batch dimension) that ``EvalAccumulator`` can take: ``"objects"`` int64, the tabulated
    objects (rows below ``min(count, M)`` with a pixel), with ``exclude_border`` those that touch no border line only;
    over these, fp64 ``"<name>_mean"`` and ``"<name>_area_mean"`` (weighted by area) of ``eccentricity``,
    ``compactness`` and, where the table has them, ``mean_conc`` and ``inscribed_radius``; ``"median_area"`` fp64, the
    k-th smallest area with k = (objects + 1) // 2; ``"valid"`` int32, 0 for a sample with no such object, whose values
    are all 0.  Plain torch on the table: no kernel of this package, no host synchronisation."""
    if not isinstance(f, dict) or "area" not in f or "count" not in f:
        raise TypeError("object_feature_summary: expected the dict of object_features")
    area = f["area"]
    batched = area.dim() == 2
    view = (lambda v: v) if batched else (lambda v: v[None])
    area, count, border = view(area), view(f["count"]), view(f["border"])
    M = area.shape[1]
    keep = (torch.arange(M, device=area.device)[None, :] < count[:, None]) & (area > 0)
    if exclude_border:
        keep = keep & (border == 0)
    n = keep.sum(dim=1)
    w = torch.where(keep, area, torch.zeros_like(area)).to(torch.float64)
    wsum = w.sum(dim=1)
    nd = n.to(torch.float64)
    some = n > 0
    zero = torch.zeros_like(nd)
    out = {"objects": n, "valid": some.to(torch.int32)}
    for name in _SUMMARY:
        if name not in f:
            continue
        v = torch.where(keep, view(f[name]), torch.zeros_like(w))
        out[name + "_mean"] = torch.where(some, v.sum(dim=1) / torch.clamp(nd, min=1.0), zero)
        out[name + "_area_mean"] = torch.where(some, (v * w).sum(dim=1) / torch.clamp(wsum, min=1.0), zero)
    big = torch.full_like(area, torch.iinfo(torch.int64).max)
    ordered = torch.sort(torch.where(keep, area, big), dim=1).values
    k = torch.clamp((n + 1) // 2 - 1, min=0)
    med = ordered.gather(1, k[:, None])[:, 0]
    out["median_area"] = torch.where(some, med, torch.zeros_like(med)).to(torch.float64)
    return out if batched else {k_: v[0] for k_, v in out.items()}
