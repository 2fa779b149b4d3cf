"""Hysteresis (double) thresholding and binary reconstruction: connected components selected by what they contain.

Every stain number of ``stain_quant``, ``objects`` and ``background`` turns a concentration map into a mask with ONE
threshold.  A plaque has a dense core and a diffuse halo: a threshold high enough to reject haze and speckle keeps the
cores only (every area too small, large plaques in pieces), one low enough to keep the halo keeps every speckle as an
"object".  Double thresholding keeps both ends:

  weak        tissue and t >= low          (the mask that is labelled)
  strong      tissue and t >= high         (the marker), low <= high, both on the 1/1024 OD grid
  positive    the weak pixels connected, through weak pixels, to a strong one

and the primitive under it is binary reconstruction, here for any byte mask and marker:

  seeds(C)    the pixels of component C of ``mask`` at which ``marker`` is set
  selected    (seeds(C) >= min_seed) != invert
  reductions  ``reconstruct_mask`` = ``scipy.ndimage.binary_propagation(marker & mask, mask=mask)``; ``clear_border``
              (marker = the image border, ``invert``); marker = mask, or no marker with ``invert``: ``label_components``

The kernels are ``s2s_objects_label_seeded`` (``csrc/objects.hip``: the labelling of ``label_components`` with three more
passes between its flatten pass and its numbering stage, the parent array as the per-root seed counter) and
``s2s_hyst_mask`` (``csrc/hysteresis.hip``: the dual-threshold byte and its counts in one pass).  Everything is an
integer, so results are exact and bit-reproducible and the tests compare for equality.  No call waits for the device
except ``hysteresis_thresholds``.  ``t`` is ``bin(c)`` of ``concentration_bins`` or, with ``radius``, the top-hat of
``stain_quantify_corrected``.  The defaults (8-connectivity, ``min_seed=1``, triangle / Otsu as the pair of thresholds)
are conventions to calibrate, not calibrations; ``skimage.filters.apply_hysteresis_threshold`` labels with
4-connectivity.  GPU only.  DESIGN.md section 3.37.

The reference publishes no stain measurement: these numbers have no counterpart there.
"""
from __future__ import annotations

import operator
from typing import Dict, Optional, Tuple

import torch

from . import _native, ops
from ._regionio import BandSource, check_region, gpu_device, gpu_rows
from .background import (_Args, _background, _bins_batch, _check_sides, _new_counts, _planes, _tiles)
from .image_metrics import _check_pair
from .objects import (_FG_ANY, _FG_POSITIVE, MAX_PIXELS, _check_mask, _check_mpp, _check_pixels, _density, _mask_bytes,
                      _object_args, _scratch, _stain_dict, _words)
from .stain_calibrate import BINS_PER_OD, _check_band_rows, _region_bands, threshold_bin

_SEED_STRONG = 4             # bit 2 of the dual-threshold byte
_RULES = ("otsu", "triangle")
_PAIR_KEYS = ("burden_pred", "burden_target", "burden_abs_err", "dice", "iou")


# ---- arguments -------------------------------------------------------------------------------------------------------
def _check_min_seed(min_seed, what: str) -> int:
    if isinstance(min_seed, bool):
        raise TypeError(f"{what}: min_seed must be an int, got bool")
    min_seed = operator.index(min_seed)
    if not 1 <= min_seed <= MAX_PIXELS:
        raise ValueError(f"{what}: min_seed must lie in 1..{MAX_PIXELS}, got {min_seed}")
    return min_seed


def _check_low_high(low, high, what: str) -> Tuple[int, int]:
    j_low, j_high = threshold_bin(low), threshold_bin(high)
    if j_low > j_high:
        raise ValueError(f"{what}: low must not exceed high, got {low!r} > {high!r}")
    return j_low, j_high


# ---- launches --------------------------------------------------------------------------------------------------------
def _select(mask_ptr: int, pitch: int, img: int, fg: int, marker_ptr: int, mpitch: int, mimg: int, seed_bits: int,
            min_seed: int, invert: bool, B: int, H: int, W: int, dev, connectivity: int, min_area: int, M: int,
            want_mask: bool, what: str) -> Dict[str, torch.Tensor]:
    """The seeded labelling launches on a byte mask and a byte marker; every tensor [B, ...]."""
    scratch = _scratch(dev, _words(B, H, W))
    labels = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    kept = torch.zeros((B,), dtype=torch.int64, device=dev)
    largest = torch.zeros((B,), dtype=torch.int32, device=dev)
    hist = torch.zeros((B, 32), dtype=torch.int64, device=dev)
    candidates = torch.empty((B,), dtype=torch.int32, device=dev)
    seeded = torch.empty((B,), dtype=torch.int32, device=dev)
    seed_pixels = torch.empty((B,), dtype=torch.int64, device=dev)
    res = {"labels": labels, "count": count, "kept_pixels": kept, "largest": largest, "size_hist": hist,
           "candidates": candidates, "seeded": seeded, "seed_pixels": seed_pixels}
    area = bbox = sums = None
    if M:
        area = torch.zeros((B, M), dtype=torch.int32, device=dev)
        bbox = torch.zeros((B, M, 4), dtype=torch.int32, device=dev)
        sums = torch.zeros((B, M, 2), dtype=torch.int64, device=dev)
    out = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if want_mask else None
    L = ops._L()
    rc = L.s2s_objects_label_seeded(mask_ptr, pitch, img, fg, marker_ptr, mpitch, mimg, seed_bits, min_seed, int(invert),
                                    B, H, W, connectivity, min_area, M, scratch.data_ptr(), labels.data_ptr(),
                                    count.data_ptr(), kept.data_ptr(), largest.data_ptr(), hist.data_ptr(),
                                    area.data_ptr() if M else 0, bbox.data_ptr() if M else 0,
                                    sums.data_ptr() if M else 0, out.data_ptr() if want_mask else 0, W, H * W,
                                    candidates.data_ptr(), seeded.data_ptr(), seed_pixels.data_ptr(), ops._stream())
    _native.check(rc, what)
    if M:
        centroid = torch.empty((B, M, 2), dtype=torch.float32, device=dev)
        _native.check(L.s2s_objects_centroid(count.data_ptr(), area.data_ptr(), sums.data_ptr(), B, M,
                                             centroid.data_ptr(), ops._stream()), what)
        res.update(area=area, bbox=bbox, centroid=centroid)
    if want_mask:
        res["mask"] = out
    return res


def _dual_mask(t_ptr: int, tissue_ptr: int, B: int, rows: int, W: int, row0: int, nrows: int, j_low: int, j_high: int,
               pool: bool, reset: int, counts: torch.Tensor, mask_ptr: int, out_img: int, what: str) -> None:
    rc = ops._L().s2s_hyst_mask(t_ptr, tissue_ptr, B, rows, W, row0, nrows, j_low, j_high, int(pool), reset,
                                counts.data_ptr(), mask_ptr, out_img, ops._stream())
    _native.check(rc, what)


def _batch_mask(tiles, kind: str, B: int, H: int, W: int, a: "_Args", j_high: int, pool: bool, reset: int,
                counts: torch.Tensor, dev) -> torch.Tensor:
    """The dual-threshold byte [B, H, W] of a batch of images: bins, with a radius the background and the corrected t
    (the launches of ``stain_quantify_corrected``), then one ``s2s_hyst_mask``.  ``counts`` int64 [owners, 3]."""
    N = B * H * W
    (b, s, bg), tissue = _planes(dev, N, 3)
    _bins_batch(tiles, kind, B, H, W, a, b, tissue)
    t = b
    if a.radius is not None:
        _background(b, s, bg, B, H, W, a, dev)
        c3, h3 = _new_counts(B, dev)
        rc = ops._L().s2s_grey_corrected(b.data_ptr(), bg.data_ptr(), tissue.data_ptr(), B, H, W, 0, H, a.j, a.stain, 0,
                                         1, c3.data_ptr(), h3.data_ptr(), 0, s.data_ptr(), H * W, ops._stream())
        _native.check(rc, a.what)
        t = s                                                # the box mean's plane is free after the opening
    mask = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    _dual_mask(t.data_ptr(), tissue.data_ptr(), B, H, W, 0, H, a.j, j_high, pool, reset, counts, mask.data_ptr(), H * W,
               a.what)
    return mask


def _burden(positive: torch.Tensor, counts: torch.Tensor, what: str) -> torch.Tensor:
    owners = counts.shape[0]
    burden = torch.empty((owners,), dtype=torch.float64, device=counts.device)
    _native.check(ops._L().s2s_hyst_finalize(positive.data_ptr(), counts.data_ptr(), owners, burden.data_ptr(),
                                             ops._stream()), what)
    return burden


def _objects_result(res, counts, mpp, M: int, return_labels: bool, return_mask: bool, what: str) -> Dict:
    tissue = counts[:, 0].contiguous()
    burden = _burden(res["kept_pixels"], counts, what)
    per_mm2 = _density(res, tissue, mpp, what)[1] if mpp is not None else None
    out = _stain_dict(res, tissue, burden, per_mm2, M, return_labels)
    out.update(weak=counts[:, 1], strong=counts[:, 2], candidates=res["candidates"], seeded=res["seeded"])
    if return_mask:
        out["mask"] = res["mask"]
    return out


# ---- masks and markers -----------------------------------------------------------------------------------------------
def select_components(mask: torch.Tensor, marker: torch.Tensor, *, connectivity: int = 8, min_seed: int = 1,
                      invert: bool = False, min_area: int = 1, max_objects: Optional[int] = None,
                      return_mask: bool = False) -> Dict[str, torch.Tensor]:
    """The connected components of ``mask`` that hold at least ``min_seed`` pixels of ``marker`` (``invert``: those that
    do not).  ``mask`` and ``marker`` are bool or uint8 (nonzero = set) ``[B, H, W]`` or ``[H, W]`` of one shape on the
    GPU; row-strided views are read in place.  Marker pixels outside the mask count for nothing.

    Returns the keys of ``label_components`` computed on the selected components (``"labels"``, ``"count"``,
    ``"kept_pixels"``, ``"largest"``, ``"size_hist"``, the table with ``max_objects``; ``min_area`` filters after the
    selection) and ``"candidates"`` int32 ``[B]`` (the components of the mask), ``"seeded"`` int32 ``[B]`` (those with at
    least ``min_seed`` seeds, whatever ``invert`` and ``min_area`` say), ``"seed_pixels"`` int64 ``[B]`` (marker and mask);
    ``return_mask``: ``"mask"`` uint8 0 / 1, the selected components before the area filter.  Exact and
    bit-reproducible; a sample's values do not depend on its batch mates; no host synchronisation."""
    what = "select_components"
    B, H, W = _check_mask(mask, what)
    if _check_mask(marker, what) != (B, H, W) or marker.dim() != mask.dim():
        raise ValueError(f"{what}: mask {list(mask.shape)} and marker {list(marker.shape)} differ in shape")
    connectivity, min_area, M = _object_args(connectivity, min_area, max_objects, what)
    min_seed = _check_min_seed(min_seed, what)
    dev = gpu_device(what, mask, marker, host_ok=False)
    with torch.no_grad():
        m, pitch, img = _mask_bytes(mask, B, H, W)
        k, kpitch, kimg = _mask_bytes(marker, B, H, W)
        res = _select(m.data_ptr(), pitch, img, _FG_ANY, k.data_ptr(), kpitch, kimg, _FG_ANY, min_seed, bool(invert), B, H,
                      W, dev, connectivity, min_area, M, bool(return_mask), what)
    return res if mask.dim() == 3 else {k_: v[0] for k_, v in res.items()}


def _as_mask_dtype(out: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    out = out if like.dim() == 3 else out[0]
    return out.view(torch.bool) if like.dtype == torch.bool else out


def reconstruct_mask(mask: torch.Tensor, marker: torch.Tensor, connectivity: int = 8) -> torch.Tensor:
    """Binary reconstruction: the components of ``mask`` that hold a pixel of ``marker``, in the mask's dtype and shape
    with values 0 / 1.  Equal to ``scipy.ndimage.binary_propagation(marker & mask, mask=mask, structure=...)`` with the
    cross (4) or the 3 x 3 square (8)."""
    what = "reconstruct_mask"
    B, H, W = _check_mask(mask, what)
    if _check_mask(marker, what) != (B, H, W) or marker.dim() != mask.dim():
        raise ValueError(f"{what}: mask {list(mask.shape)} and marker {list(marker.shape)} differ in shape")
    connectivity, _, _ = _object_args(connectivity, 1, None, what)
    dev = gpu_device(what, mask, marker, host_ok=False)
    with torch.no_grad():
        m, pitch, img = _mask_bytes(mask, B, H, W)
        k, kpitch, kimg = _mask_bytes(marker, B, H, W)
        res = _select(m.data_ptr(), pitch, img, _FG_ANY, k.data_ptr(), kpitch, kimg, _FG_ANY, 1, False, B, H, W, dev,
                      connectivity, 1, 0, True, what)
    return _as_mask_dtype(res["mask"], mask)


def clear_border(mask: torch.Tensor, connectivity: int = 8) -> torch.Tensor:
    """``mask`` without the components that touch its first or last row or column (objects cut by the field of view), in
    the mask's dtype and shape with values 0 / 1.  The marker, the image border, is built on the device."""
    what = "clear_border"
    B, H, W = _check_mask(mask, what)
    connectivity, _, _ = _object_args(connectivity, 1, None, what)
    dev = gpu_device(what, mask, host_ok=False)
    with torch.no_grad():
        m, pitch, img = _mask_bytes(mask, B, H, W)
        border = torch.zeros((H, W), dtype=torch.uint8, device=dev)
        border[0], border[-1], border[:, 0], border[:, -1] = 1, 1, 1, 1
        # one border image serves every sample: marker_img_stride is only read for B > 1, and must not let samples
        # overlap, so the batch gets its own copies
        k = border[None].expand(B, H, W).contiguous() if B > 1 else border[None]
        res = _select(m.data_ptr(), pitch, img, _FG_ANY, k.data_ptr(), W, H * W, _FG_ANY, 1, True, B, H, W, dev,
                      connectivity, 1, 0, True, what)
    return _as_mask_dtype(res["mask"], mask)


def hysteresis_mask(t: torch.Tensor, low: float, high: float, *, tissue: Optional[torch.Tensor] = None,
                    connectivity: int = 8, min_seed: int = 1) -> torch.Tensor:
    """The hysteresis mask of int16 ``t`` ``[B, H, W]`` or ``[H, W]`` on the 1/1024 OD grid (``concentration_bins``, or
    the ``"corrected"`` of ``stain_quantify_corrected``) on the GPU: uint8 0 / 1, 1 on the pixels with ``t >= low * 1024``
    that are connected through such pixels to at least ``min_seed`` pixels with ``t >= high * 1024``.  ``tissue`` (bool
    or uint8 of the same shape; ``None``: every pixel) gates both.  ``low <= high``, both ``j / 1024`` with ``j`` in
    1..4095 (``ValueError`` otherwise).  The defaults are conventions to calibrate (``hysteresis_thresholds``)."""
    what = "hysteresis_mask"
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: t must be a torch.Tensor, got {type(t).__name__}")
    if t.dtype != torch.int16 or t.dim() not in (2, 3) or min(t.shape) < 1:
        raise ValueError(f"{what}: t must be a non-empty int16 [B, H, W] or [H, W], got {t.dtype} {list(t.shape)}")
    B = int(t.shape[0]) if t.dim() == 3 else 1
    H, W = int(t.shape[-2]), int(t.shape[-1])
    _check_sides(B, H, W, what)
    _check_pixels(H, W, what)
    if tissue is not None:
        if _check_mask(tissue, what) != (B, H, W) or tissue.dim() != t.dim():
            raise ValueError(f"{what}: t {list(t.shape)} and tissue {list(tissue.shape)} differ in shape")
    j_low, j_high = _check_low_high(low, high, what)
    connectivity, _, _ = _object_args(connectivity, 1, None, what)
    min_seed = _check_min_seed(min_seed, what)
    dev = gpu_device(what, *((t,) if tissue is None else (t, tissue)), host_ok=False)
    with torch.no_grad():
        tt = t.detach().contiguous()
        tis = None
        if tissue is not None:
            tis = tissue.detach().contiguous()
            tis = tis.view(torch.uint8) if tis.dtype == torch.bool else tis
        counts = torch.empty((B, 3), dtype=torch.int64, device=dev)
        dual = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
        _dual_mask(tt.data_ptr(), tis.data_ptr() if tis is not None else 0, B, H, W, 0, H, j_low, j_high, False, 1, counts,
                   dual.data_ptr(), H * W, what)
        res = _select(dual.data_ptr(), W, H * W, _FG_POSITIVE, dual.data_ptr(), W, H * W, _SEED_STRONG, min_seed, False, B,
                      H, W, dev, connectivity, 1, 0, True, what)
        out = res["mask"] & 1                                # (bit 1 of the selected byte is the tissue)
    return out if t.dim() == 3 else out[0]


# ---- stains ----------------------------------------------------------------------------------------------------------
def stain_objects_hysteresis(tiles: torch.Tensor, low: float, high: float, *, radius: Optional[float] = None,
                             smooth: int = 2, footprint: str = "disc", stain: int = 1, stains="hdab", white: int = 220,
                             black: int = 0, connectivity: int = 8, min_seed: int = 1, min_area: int = 1,
                             max_objects: Optional[int] = None, mpp: Optional[float] = None,
                             return_labels: bool = False, return_mask: bool = False) -> Dict[str, torch.Tensor]:
    """``stain_objects`` on the hysteresis mask of stain ``stain``, for uint8 ``[B, H, W, 3]`` or fp32 ``[B, 3, H, W]``
    images on the GPU: an object is a component of ``tissue and t >= low`` that holds at least ``min_seed`` pixels with
    ``t >= high``.  ``radius=None``: t = bin(c); with a radius t is the top-hat of ``stain_quantify_corrected`` (its
    launches: the opening runs once).

    Returns the keys of ``stain_objects``: ``"count"``, ``"tissue"``, ``"positive"`` (the pixels of the kept objects),
    ``"burden"`` fp64 = positive / max(tissue, 1), ``"largest"``, ``"size_hist"``, ``"per_mm2"`` with ``mpp``, the table
    with ``max_objects``, ``"labels"`` on request (they feed ``object_features``, ``split_objects``, ``object_zones`` and
    ``render_classes`` unchanged); and ``"weak"``, ``"strong"`` int64 ``[B]`` (tissue pixels at or above ``low`` /
    ``high``: the positive counts of the two single thresholds), ``"candidates"``, ``"seeded"`` int32 ``[B]`` (weak
    components; those with enough strong pixels).  ``return_mask``: ``"mask"`` uint8 (bit 0 the selected pixels before
    the area filter, bit 1 tissue: the byte of ``stain_quantify_corrected``).  ``low == high`` is the single threshold of
    ``stain_objects`` / ``stain_objects_corrected``.  ``low``, ``high``, ``min_seed`` and the connectivity are
    conventions to calibrate.  No host synchronisation."""
    what = "stain_objects_hysteresis"
    kind, B, H, W = _tiles(tiles, what)
    _check_pixels(H, W, what)
    j_low, j_high = _check_low_high(low, high, what)
    a = _Args(what, radius, low, stain, stains, smooth, footprint, white, black)
    connectivity, min_area, M = _object_args(connectivity, min_area, max_objects, what)
    min_seed = _check_min_seed(min_seed, what)
    mpp = _check_mpp(mpp, what)
    dev = gpu_device(what, tiles, host_ok=False)
    with torch.no_grad():
        counts = torch.empty((B, 3), dtype=torch.int64, device=dev)
        dual = _batch_mask(tiles, kind, B, H, W, a, j_high, False, 1, counts, dev)
        res = _select(dual.data_ptr(), W, H * W, _FG_POSITIVE, dual.data_ptr(), W, H * W, _SEED_STRONG, min_seed, False, B,
                      H, W, dev, connectivity, min_area, M, bool(return_mask), what)
        return _objects_result(res, counts, mpp, M, return_labels, bool(return_mask), what)


def stain_agreement_hysteresis(generated: torch.Tensor, target: torch.Tensor, low: float, high: float, *,
                               radius: Optional[float] = None, smooth: int = 2, footprint: str = "disc",
                               stain: int = 1, stains="hdab", white: int = 220, black: int = 0, connectivity: int = 8,
                               min_seed: int = 1) -> Dict[str, torch.Tensor]:
    """``stain_agreement_corrected`` on the two hysteresis masks: ``{"burden_pred", "burden_target", "burden_abs_err",
    "dice", "iou"}``, each fp64 ``[B]`` on the device; Dice and IoU are 1 when both masks are empty."""
    what = "stain_agreement_hysteresis"
    _check_pair(generated, target, what)
    kind, B, H, W = _tiles(generated, what)
    _check_pixels(H, W, what)
    j_low, j_high = _check_low_high(low, high, what)
    a = _Args(what, radius, low, stain, stains, smooth, footprint, white, black)
    connectivity, _, _ = _object_args(connectivity, 1, None, what)
    min_seed = _check_min_seed(min_seed, what)
    dev = gpu_device(what, generated, target, host_ok=False)
    L = ops._L()
    with torch.no_grad():
        sides = []
        for t in (generated, target):
            counts = torch.empty((B, 3), dtype=torch.int64, device=dev)
            dual = _batch_mask(t, kind, B, H, W, a, j_high, False, 1, counts, dev)
            res = _select(dual.data_ptr(), W, H * W, _FG_POSITIVE, dual.data_ptr(), W, H * W, _SEED_STRONG, min_seed,
                          False, B, H, W, dev, connectivity, 1, 0, True, what)
            # the layout s2s_grey_pair_finalize reads: tissue, positive (the weak count gives way to the selected one)
            counts[:, 1] = res["kept_pixels"]
            sides.append((counts, res["mask"]))
        both = torch.empty((B,), dtype=torch.int64, device=dev)
        out = torch.empty((B, 5), dtype=torch.float64, device=dev)
        _native.check(L.s2s_grey_pair(sides[0][1].data_ptr(), sides[1][1].data_ptr(), B, H, W, both.data_ptr(),
                                      ops._stream()), what)
        _native.check(L.s2s_grey_pair_finalize(sides[0][0].data_ptr(), sides[1][0].data_ptr(), both.data_ptr(), B,
                                               out.data_ptr(), ops._stream()), what)
    return {k: out[:, i] for i, k in enumerate(_PAIR_KEYS)}


def region_stain_objects_hysteresis(region_u8: torch.Tensor, low: float, high: float, *, radius: Optional[float] = None,
                                    band_rows: Optional[int] = None, smooth: int = 2, footprint: str = "disc",
                                    stain: int = 1, stains="hdab", white: int = 220, black: int = 0,
                                    connectivity: int = 8, min_seed: int = 1, min_area: int = 1,
                                    max_objects: Optional[int] = None, mpp: Optional[float] = None,
                                    return_labels: bool = False, return_mask: bool = False) -> Dict[str, torch.Tensor]:
    """``stain_objects_hysteresis`` of one whole uint8 ``[H, W, 3]`` region on the GPU or on the host (any row pitch):
    device scalars, the table ``[M, ...]``, ``"labels"`` / ``"mask"`` ``[H, W]`` on request.

    The dual-threshold byte is built band by band (``band_rows``; ``None``: a GPU region in one piece, a host region in
    bands of 512 rows; with a radius every band carries the halo of ``region_stain_quantify_corrected``,
    ``2 * floor(radius) + smooth`` rows), then the whole mask is labelled once: an object across a band seam is one
    object, and its seed may lie in another band.  Bit-equal for every ``band_rows``, for host and GPU input, and equal
    to the batch call on ``region[None]``."""
    what = "region_stain_objects_hysteresis"
    H, W, _ = check_region(region_u8, what)
    _check_sides(1, H, W, what)
    _check_pixels(H, W, what)
    band_rows = _check_band_rows(band_rows)
    j_low, j_high = _check_low_high(low, high, what)
    a = _Args(what, radius, low, stain, stains, smooth, footprint, white, black)
    connectivity, min_area, M = _object_args(connectivity, min_area, max_objects, what)
    min_seed = _check_min_seed(min_seed, what)
    mpp = _check_mpp(mpp, what)
    dev = gpu_device(what, region_u8)
    bands = [(max(r0 - a.halo, 0), r0, r1, min(r1 + a.halo, H))
             for r0, r1 in _region_bands(H, band_rows, not region_u8.is_cuda)]
    buf_rows = max(h1 - h0 for h0, _, _, h1 in bands)
    L = ops._L()
    with torch.no_grad():
        counts = torch.empty((1, 3), dtype=torch.int64, device=dev)
        dual = torch.empty((1, H, W), dtype=torch.uint8, device=dev)
        src = BandSource(region_u8, buf_rows, dev)
        (b, s, bg), tissue = _planes(dev, buf_rows * W, 3)
        c3, h3 = _new_counts(1, dev) if a.radius is not None else (None, None)
        reset = 1
        for h0, r0, r1, h1 in bands:
            rows = h1 - h0
            ptr, pitch = gpu_rows(src.rows(h0, h1))
            _native.check(L.s2s_grey_bins_u8(ptr, pitch, pitch * rows, 1, rows, W, a.table, a.unmix, a.white, a.black,
                                             a.stain, b.data_ptr(), tissue.data_ptr(), ops._stream()), what)
            if a.radius is not None:
                _background(b, s, bg, 1, rows, W, a, dev)
                # t of the band's own rows, dense, into the box mean's plane (free after the opening)
                rc = L.s2s_grey_corrected(b.data_ptr(), bg.data_ptr(), tissue.data_ptr(), 1, rows, W, r0 - h0, r1 - r0,
                                          a.j, a.stain, 0, 1, c3.data_ptr(), h3.data_ptr(), 0, s.data_ptr(),
                                          (r1 - r0) * W, ops._stream())
                _native.check(rc, what)
                _dual_mask(s.data_ptr(), tissue[(r0 - h0) * W:].data_ptr(), 1, r1 - r0, W, 0, r1 - r0, j_low, j_high,
                           False, reset, counts, dual[0, r0:].data_ptr(), (r1 - r0) * W, what)
            else:
                _dual_mask(b.data_ptr(), tissue.data_ptr(), 1, rows, W, r0 - h0, r1 - r0, j_low, j_high, False, reset,
                           counts, dual[0, r0:].data_ptr(), (r1 - r0) * W, what)
            reset = 0
        res = _select(dual.data_ptr(), W, H * W, _FG_POSITIVE, dual.data_ptr(), W, H * W, _SEED_STRONG, min_seed, False, 1,
                      H, W, dev, connectivity, min_area, M, bool(return_mask), what)
        out = _objects_result(res, counts, mpp, M, return_labels, bool(return_mask), what)
    return {k: v[0] for k, v in out.items()}


# ---- the pair of thresholds ------------------------------------------------------------------------------------------
def hysteresis_thresholds(t: Dict[str, torch.Tensor], low: str = "triangle", high: str = "otsu", stain: int = 1,
                          fallback: Optional[Tuple[float, float]] = None, *, owner: int = 0) -> Tuple[float, float]:
    """``(low, high)`` as two host floats on the 1/1024 grid for the calls above, from the result ``t`` of
    ``stain_thresholds`` / ``calibrate_thresholds``: the ``"<rule>_bin"`` of the rules ``low`` and ``high`` (``"triangle"``
    or ``"otsu"``) for stain ``stain`` of owner ``owner``, over 1024.  ``high`` is raised to ``low`` where a rule puts it
    below.  Where a rule has no answer the matching entry of ``fallback = (low, high)`` is taken, and ``ValueError`` is
    raised without one.  Triangle / Otsu as the pair is a convention to calibrate.  Like ``thresholds_tuple`` this is
    the one call of the module that waits for the device."""
    what = "hysteresis_thresholds"
    for rule in (low, high):
        if rule not in _RULES:
            raise ValueError(f"{what}: a rule must be one of {', '.join(map(repr, _RULES))}, got {rule!r}")
    if not isinstance(t, dict) or any(r + "_bin" not in t or r + "_valid" not in t for r in (low, high)):
        raise TypeError(f"{what}: t must be a result of stain_thresholds or calibrate_thresholds")
    stain, owner = operator.index(stain), operator.index(owner)
    if not 0 <= stain <= 2:
        raise ValueError(f"{what}: stain must be 0, 1 or 2, got {stain}")
    if not 0 <= owner < t[low + "_bin"].shape[0]:
        raise ValueError(f"{what}: owner must lie in 0..{t[low + '_bin'].shape[0] - 1}, got {owner}")
    if fallback is not None:
        fallback = tuple(float(v) for v in fallback)
        if len(fallback) != 2:
            raise ValueError(f"{what}: fallback must be two numbers (low, high), got {fallback!r}")
        fallback = tuple(threshold_bin(v) for v in fallback)
    picked = torch.stack([t[low + "_bin"][owner, stain], t[low + "_valid"][owner, stain],
                          t[high + "_bin"][owner, stain], t[high + "_valid"][owner, stain]]).tolist()      # the sync
    js = []
    for i, rule in enumerate((low, high)):
        j, ok = int(picked[2 * i]), int(picked[2 * i + 1])
        if not ok:
            if fallback is None:
                raise ValueError(f"{what}: the {rule} rule has no answer for stain {stain} of owner {owner} "
                                 "(pass fallback=)")
            j = fallback[i]
        js.append(min(max(j, 1), 4095))
    js[1] = max(js[1], js[0])
    return js[0] / BINS_PER_OD, js[1] / BINS_PER_OD
