"""Dense region alignment: clean a measured shift field, interpolate it to a sub-pixel displacement per pixel and
resample the target region (and its masks) through it.

``region_shift_field`` measures one integer shift per cell; ``shift_tiles`` can only move whole tiles, so a region
aligned cell by cell tears wherever neighbouring cells disagree, and a glass or mismatched cell has no usable shift at
all.  This module turns the field into an aligned region (``csrc/warp.hip``):

  field            int32 ``[Gy, Gx, 2]`` = (dy, dx) in 1/16 pixel (``SUB = 16``); node (gy, gx) is the centre of cell
                   (gy, gx), Gy = H // cell, Gx = W // cell
  displacement     per axis, in doubled coordinates: span = 2 cell, u = 2 p + 1 - cell; for G >= 2: g0 = clamp(floor(u /
                   span), 0, G - 2), g1 = g0 + 1, w = clamp(u - g0 span, 0, span); for G = 1: g0 = g1 = 0, w = 0; in int64
                   num = (span - wy) ((span - wx) D[y0][x0] + wx D[y0][x1]) + wy ((span - wx) D[y1][x0] + wx D[y1][x1]),
                   d = floor((num + span^2 / 2) / span^2), clamped to +-16 max_shift per component inside the kernel
  image sampling   sy = 16 y + d_y, iy = sy >> 4, fy = sy & 15, columns alike; the four taps at (iy, ix) .. (iy + 1,
                   ix + 1), ``fill`` for a tap outside the region; out = ((16 - fy) ((16 - fx) p00 + fx p01) + fy ((16 - fx)
                   p10 + fx p11) + 128) >> 8
  mask sampling    nearest: iy = (sy + 8) >> 4, ix alike, one tap; class indices are never blended
  cleaning         a reliable cell with at least 3 reliable 8-neighbours is dropped when it lies more than ``max_dev``
                   pixels (Chebyshev) from their component-wise lower median; the kept cells seed the field with 16 *
                   shift; Jacobi iterations give every unknown cell with n >= 1 known neighbours floor((2 sum + n) /
                   (2 n)) of their values until none is unknown

``out[y, x]`` is the target brought onto ``src[y, x]``, the direction of ``shift_tiles``; a constant field
``16 * (dy, dx)`` reproduces ``shift_tiles`` byte for byte.  Everything is integer arithmetic, so results are
bit-reproducible and bit-equal for host and GPU input and for every banding.  With GPU regions nothing here waits for
the device.  GPU only.

The reference publishes no registration: these functions have no counterpart there.
"""
from __future__ import annotations

import operator
from typing import Dict, Optional, Sequence

import torch

from . import _native, ops
from ._regionio import DEFAULT_HOST_BAND, BandSink, BandSource, batch_layout, check_region, gpu_device
from .registration import region_shift_field

SUB = 16                     # displacement units per pixel
MAX_SHIFT = 1024             # WP_MAX_SHIFT of csrc/warp.hip
MAX_CELLS = 65536            # nodes of a field: the cleaning kernel is one workgroup
MAX_CELL = 1 << 14           # span^2 times an int32 node stays inside int64

_CLEAN_KEYS = ("min_score", "min_margin", "max_dev")
_WARP_KEYS = ("fill", "band_rows")


def _check_max_shift(max_shift, what: str) -> int:
    max_shift = operator.index(max_shift)
    if not 0 <= max_shift <= MAX_SHIFT:
        raise ValueError(f"{what}: max_shift must lie in 0..{MAX_SHIFT}, got {max_shift}")
    return max_shift


def _check_fill(fill, what: str) -> int:
    fill = operator.index(fill)
    if not 0 <= fill <= 255:
        raise ValueError(f"{what}: fill must lie in 0..255, got {fill}")
    return fill


# ---- cleaning ----------------------------------------------------------------------------------------------------------
def clean_shift_field(field_or_shift, *, reliable: Optional[torch.Tensor] = None, min_score: float = 0.5,
                      min_margin: float = 0.05, max_dev: int = 2, max_shift: int = 64) -> Dict[str, torch.Tensor]:
    """A measured shift field made usable: outliers dropped, every cell without a usable shift filled from its
    neighbours.  One launch of one workgroup; nothing waits for the device.

    ``field_or_shift``: ``region_shift_field``'s dict as it comes, or its ``"shift"`` alone, int32 ``[Gy, Gx, 2]`` in
    pixels on the GPU.  ``reliable``: uint8 or bool ``[Gy, Gx]`` on the device; ``None``: from the dict as ``valid == 1 &
    score >= min_score & margin >= min_margin``, in torch on the device (every cell for a bare shift tensor).  A cell
    whose shift exceeds ``max_shift`` pixels is unreliable whatever ``reliable`` says.  ``max_dev``: the largest distance
    in pixels from the neighbours' lower median that a cell may have.

    Returns device tensors: ``"field"`` int32 ``[Gy, Gx, 2]`` in 1/16 pixel, ``"kept"`` uint8 ``[Gy, Gx]`` (1 measured,
    0 filled) and ``"stats"`` int32 ``[2]`` = cells kept, fill iterations run.  No cell kept: the field is all zeros."""
    what = "clean_shift_field"
    max_shift = _check_max_shift(max_shift, what)
    max_dev = operator.index(max_dev)
    if max_dev < 0:
        raise ValueError(f"{what}: max_dev must not be negative, got {max_dev}")
    min_score, min_margin = float(min_score), float(min_margin)
    if min_score != min_score or min_margin != min_margin:
        raise ValueError(f"{what}: min_score and min_margin must be numbers, got {min_score} and {min_margin}")
    info = None
    shift = field_or_shift
    if isinstance(field_or_shift, dict):
        info = field_or_shift
        for k in ("shift",) + (() if reliable is not None else ("valid", "score", "margin")):
            if k not in info:
                raise ValueError(f"{what}: the field dict has no {k!r} (pass region_shift_field's result as it comes)")
        shift = info["shift"]
    if not isinstance(shift, torch.Tensor):
        raise TypeError(f"{what}: shift must be a torch.Tensor or region_shift_field's dict, got {type(shift).__name__}")
    if shift.dtype != torch.int32 or shift.dim() != 3 or shift.shape[2] != 2 or min(shift.shape) < 1:
        raise ValueError(f"{what}: shift must be a non-empty int32 [Gy, Gx, 2], got {shift.dtype} {list(shift.shape)}")
    Gy, Gx = int(shift.shape[0]), int(shift.shape[1])
    if Gy * Gx > MAX_CELLS:
        raise ValueError(f"{what}: a field has at most {MAX_CELLS} cells, got {Gy} x {Gx}")
    if reliable is not None:
        if not isinstance(reliable, torch.Tensor):
            raise TypeError(f"{what}: reliable must be a torch.Tensor, got {type(reliable).__name__}")
        if reliable.dtype not in (torch.uint8, torch.bool) or tuple(reliable.shape) != (Gy, Gx):
            raise ValueError(f"{what}: reliable must be uint8 or bool [{Gy}, {Gx}], got {reliable.dtype} "
                             f"{list(reliable.shape)}")
    if not shift.is_cuda:
        raise ValueError(f"{what}: shift must be on the GPU (there is no CPU path)")
    dev = shift.device
    with torch.no_grad():
        if reliable is not None:
            if reliable.device != dev:
                raise ValueError(f"{what}: reliable must be on the shift's device")
            rel = reliable.to(torch.uint8).contiguous()
        elif info is not None:
            for k in ("valid", "score", "margin"):
                t = info[k]
                if not isinstance(t, torch.Tensor) or tuple(t.shape) != (Gy, Gx) or t.device != dev:
                    raise ValueError(f"{what}: {k!r} must be a [{Gy}, {Gx}] tensor on the shift's device")
            rel = ((info["valid"] == 1) & (info["score"] >= min_score) & (info["margin"] >= min_margin)).to(torch.uint8)
        else:
            rel = torch.ones((Gy, Gx), dtype=torch.uint8, device=dev)
        shift = shift.contiguous()
        field = torch.empty((Gy, Gx, 2), dtype=torch.int32, device=dev)
        kept = torch.empty((Gy, Gx), dtype=torch.uint8, device=dev)
        stats = torch.empty((2,), dtype=torch.int32, device=dev)
        work = torch.empty((6 * Gy * Gx,), dtype=torch.int32, device=dev)
        rc = ops._L().s2s_field_clean(shift.data_ptr(), rel.data_ptr(), Gy, Gx, max_dev, max_shift, field.data_ptr(),
                                      kept.data_ptr(), stats.data_ptr(), work.data_ptr(), ops._stream())
        _native.check(rc, what)
    return {"field": field, "kept": kept, "stats": stats}


# ---- the warp ----------------------------------------------------------------------------------------------------------
def _check_field(field, H: int, W: int, cell: int, what: str):
    if not isinstance(field, torch.Tensor):
        raise TypeError(f"{what}: field must be a torch.Tensor, got {type(field).__name__}")
    if cell < 1 or cell > min(H, W, MAX_CELL):
        raise ValueError(f"{what}: cell {cell} does not fit the {H} x {W} region (at most {MAX_CELL})")
    Gy, Gx = H // cell, W // cell
    if Gy * Gx > MAX_CELLS:
        raise ValueError(f"{what}: a field has at most {MAX_CELLS} cells, got {Gy} x {Gx}")
    if field.dtype != torch.int32 or tuple(field.shape) != (Gy, Gx, 2):
        raise ValueError(f"{what}: field must be int32 [{Gy}, {Gx}, 2] in 1/{SUB} pixel for cell {cell}, got "
                         f"{field.dtype} {list(field.shape)}")
    if not field.is_cuda:
        raise ValueError(f"{what}: field must be on the GPU (there is no CPU path)")
    return Gy, Gx


def warp_region(region_u8: torch.Tensor, field: torch.Tensor, cell: int, *, max_shift: int = 64, fill: int = 255,
                band_rows: Optional[int] = None) -> torch.Tensor:
    """A uint8 ``[H, W, 3]`` image (bilinear in 1/16 pixel) or ``[H, W]`` mask (nearest) resampled through ``field``:
    ``out[y, x]`` is the region at ``(y, x)`` plus the displacement interpolated from the field's nodes, ``fill``
    outside the region.  Applied to the target of a pair with the cleaned field of ``region_shift_field`` it brings the
    target onto the source.

    ``region_u8`` lives on the GPU (any row pitch, crop views) or on the host; the result is contiguous and on the
    input's device.  ``field``: int32 ``[H // cell, W // cell, 2]`` in 1/16 pixel on the device, any values: the kernel
    clamps the displacement to ``max_shift`` pixels.  A GPU region is warped in one launch (``band_rows`` rows per launch
    when given).  A host region is streamed in bands of ``band_rows`` output rows (``None``: 512) with a halo of
    ``max_shift + 1`` rows through pinned staging in both directions, a band's download overlapping the next band's upload.  The
    bytes do not depend on ``band_rows`` or on where the region lives."""
    what = "warp_region"
    H, W, C = check_region(region_u8, what, mask_ok=True)
    cell = operator.index(cell)
    max_shift, fill = _check_max_shift(max_shift, what), _check_fill(fill, what)
    if band_rows is not None:
        band_rows = operator.index(band_rows)
        if band_rows < 1:
            raise ValueError(f"{what}: band_rows must be positive, got {band_rows}")
    Gy, Gx = _check_field(field, H, W, cell, what)
    dev = gpu_device(what, region_u8)
    if field.device != dev:
        raise ValueError(f"{what}: field must be on the region's device")
    on_gpu = region_u8.is_cuda
    step = min(band_rows or (H if on_gpu else DEFAULT_HOST_BAND), H)
    halo = max_shift + 1
    L = ops._L()
    rowb = W * C
    with torch.no_grad():
        field = field.contiguous()
        fp = field.data_ptr()
        if on_gpu:
            out = torch.empty(tuple(region_u8.shape), dtype=torch.uint8, device=dev)
            pitch = batch_layout(region_u8[None], what, "the region")[1]
            for r0 in range(0, H, step):
                n = min(step, H - r0)
                rc = L.s2s_warp_region_u8(region_u8.data_ptr(), pitch, 0, H, fp, Gy, Gx, cell, max_shift, H, W, C, fill,
                                          r0, n, out.data_ptr() + r0 * rowb, rowb, ops._stream())
                _native.check(rc, what)
            return out
        src, sink = BandSource(region_u8, min(step + 2 * halo, H), dev), BandSink(region_u8.shape, step)
        band = torch.empty((step,) + tuple(region_u8.shape[1:]), dtype=torch.uint8, device=dev)
        for r0 in range(0, H, step):
            n = min(step, H - r0)
            s0, s1 = max(0, r0 - halo), min(H, r0 + n + halo)
            rows = src.rows(s0, s1)
            rc = L.s2s_warp_region_u8(rows.data_ptr(), rowb, s0, s1 - s0, fp, Gy, Gx, cell, max_shift, H, W, C, fill,
                                      r0, n, band.data_ptr(), rowb, ops._stream())
            _native.check(rc, what)
            sink.put(band, r0, r0 + n)
        return sink.close()[0]


def register_region(src_region_u8: torch.Tensor, tgt_region_u8: torch.Tensor, cell: int = 256, *,
                    masks: Sequence[torch.Tensor] = (), **kwargs) -> Dict[str, object]:
    """The target region aligned to the source: ``region_shift_field``, ``clean_shift_field``, ``warp_region`` of the
    target and a nearest warp of every mask of ``masks`` (uint8 ``[H, W]``, in the target's frame).

    ``kwargs``: ``max_shift`` (64) for the cleaning and the warp; ``min_score``, ``min_margin``, ``max_dev`` as
    ``clean_shift_field``; ``fill`` (255), ``mask_fill`` (0) and ``band_rows`` as ``warp_region``; everything else goes
    to ``register_pairs`` (``radius``, ``downsample``, the stain bases).

    Returns ``"aligned"`` (uint8 ``[H, W, 3]`` on the target's device), ``"masks"`` (a list, each on its mask's
    device), ``"field"`` int32 ``[Gy, Gx, 2]`` in 1/16 pixel, ``"kept"``, ``"stats"`` (as ``clean_shift_field``) and
    ``"score"`` float64 ``[Gy, Gx]`` on the device."""
    what = "register_region"
    max_shift = _check_max_shift(kwargs.pop("max_shift", 64), what)
    clean_kw = {k: kwargs.pop(k) for k in _CLEAN_KEYS if k in kwargs}
    warp_kw = {k: kwargs.pop(k) for k in _WARP_KEYS if k in kwargs}
    mask_fill = _check_fill(kwargs.pop("mask_fill", 0), what)
    masks = list(masks)
    H, W, C = check_region(tgt_region_u8, what, mask_ok=True)
    if C != 3:
        raise ValueError(f"{what}: the regions must be [H, W, 3] RGB images, got {list(tgt_region_u8.shape)}")
    for m in masks:
        if check_region(m, what, mask_ok=True) != (H, W, 1):
            raise ValueError(f"{what}: a mask must be uint8 [{H}, {W}], got {list(m.shape)}")
    measured = region_shift_field(src_region_u8, tgt_region_u8, cell, **kwargs)
    cleaned = clean_shift_field(measured, max_shift=max_shift, **clean_kw)
    aligned = warp_region(tgt_region_u8, cleaned["field"], cell, max_shift=max_shift, **warp_kw)
    warp_kw["fill"] = mask_fill
    moved = [warp_region(m, cleaned["field"], cell, max_shift=max_shift, **warp_kw) for m in masks]
    return {"aligned": aligned, "masks": moved, "field": cleaned["field"], "kept": cleaned["kept"],
            "stats": cleaned["stats"], "score": measured["score"]}
