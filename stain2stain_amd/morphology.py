"""Mask morphology and boundary metrics on the GPU, built on an exact Euclidean distance transform.

A byte mask (the tissue rule, the positive-stain mask, the mask head's ``logits > 0``) could so far be numbered
(``label_components``) but not cleaned, and two masks could be compared by overlap only.  Everything here is an integer
function of squared distances, so the results are exact and bit-reproducible:

  foreground   a byte that is not 0 (bool masks are viewed as bytes)
  D_bg[y, x]   the minimum over the background pixels (y', x') of the same sample of (y - y')^2 + (x - x')^2, ``FAR`` =
               2^31 - 1 when the sample has none; 0 on background pixels.  D_fg: the roles swapped.
  border       there is nothing outside the image: it holds neither background nor foreground sites
  disc         with r2 = floor(radius^2): dilate = D_fg <= r2, erode = D_bg > r2, open = dilate(erode(m)), close =
               erode(dilate(m)).  Erosion therefore does not eat in from the image edge.
  holes        m, or any 4-connected (``connectivity=8``: 8-connected) component of the background that touches no pixel
               of the first or last row or column
  boundary     the foreground pixels with a 4-neighbour that is background or lies outside the image
  agreement    S = the pooled squared distances from every pixel of one boundary to the nearest pixel of the other one,
               both ways; max, nearest-rank percentile, sum of floor(256 sqrt(s)) and #{s <= floor(tolerance^2)}

The kernels are ``csrc/morphology.hip``: a column pass over segments of ``SEGMENT`` rows, a row pass that searches outward
in LDS, a radix select for the percentile.  Every call runs on the current stream without host synchronisation, with
scratch from the shared workspace.  ``H, W <= MAX_SIDE`` = 32767 and ``B <= 65535``.  GPU only.  DESIGN.md section 3.24.

The reference publishes no mask morphology or boundary metric: these numbers have no counterpart there.
"""
from __future__ import annotations

import math
import operator
from typing import Dict, Optional, Tuple

import torch

from . import _native, ops
from ._regionio import gpu_device
from .objects import _mask_bytes

FAR = 2 ** 31 - 1            # "no site in this sample" / "beyond max_dist"
MAX_SIDE = 32767             # H^2 + W^2 < 2^31
SEGMENT = 64                 # rows per segment of the column pass: MO_SEG of csrc/morphology.hip
ROW_PACK = 1024              # the row pass packs ROW_PACK // W rows into one workgroup ...
PACK_WIDTH = ROW_PACK // 2   # ... so rows wider than this are alone in theirs: the one width-dependent path
_OPS = ("dilate", "erode", "open", "close")


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
    if H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError(f"{what}: {H} x {W} exceeds the limit of {MAX_SIDE} pixels a side")
    return B, H, W


def _squared(value, name: str, what: str) -> int:
    """floor(value^2) of a finite value >= 0, capped below FAR."""
    try:
        value = float(value)
    except (TypeError, ValueError):
        raise TypeError(f"{what}: {name} must be a number, got {type(value).__name__}") from None
    if not (math.isfinite(value) and value >= 0.0):
        raise ValueError(f"{what}: {name} must be finite and not negative, got {value}")
    return min(int(math.floor(value * value)), FAR - 1)


def _device(what: str, *masks: torch.Tensor) -> torch.device:
    """The GPU the call runs on: the masks' own, or the current one for host masks (uploaded whole)."""
    if len({m.device for m in masks}) > 1:
        raise RuntimeError(f"stain2stain_amd: {what}: the masks are on different devices")
    return gpu_device(what, *masks)


def _scratch(dev, words: int, what: str) -> torch.Tensor:
    _native.check(words if words < 0 else 0, what)
    return ops._workspace(dev, words, "morphology").view(torch.int32)


def _bytes(mask: torch.Tensor, dev, B: int, H: int, W: int):
    return _mask_bytes(mask if mask.is_cuda else mask.to(dev), B, H, W)


def _like(out: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """``out`` [B, H, W] on the GPU -> the mask's dtype, shape and device."""
    out = out.view(torch.bool) if mask.dtype == torch.bool else out
    out = out if mask.dim() == 3 else out[0]
    return out if mask.is_cuda else out.to(mask.device)


def distance_transform(mask: torch.Tensor, to: str = "background", max_dist: Optional[float] = None) -> torch.Tensor:
    """The exact squared Euclidean distance transform of a bool or uint8 (nonzero = foreground) mask ``[B, H, W]`` or
    ``[H, W]``: int32 of the same shape, the squared distance of every pixel to the nearest background pixel
    (``to="background"``; 0 on the background itself) or foreground pixel (``to="foreground"``) of its sample, ``FAR`` =
    2^31 - 1 where the sample has none.  There is nothing outside the image.  ``max_dist``: values above
    ``floor(max_dist^2)`` are reported as ``FAR`` and the search stops there.  Equal to the squared distances behind
    ``scipy.ndimage.distance_transform_edt``.  Row-strided GPU views are read in place; a host mask is uploaded whole
    and the result comes back to the host.  Four launches, no host synchronisation."""
    what = "distance_transform"
    B, H, W = _check_mask(mask, what)
    if to not in ("background", "foreground"):
        raise ValueError(f"{what}: to must be 'background' or 'foreground', got {to!r}")
    bound = FAR if max_dist is None else _squared(max_dist, "max_dist", what)
    dev = _device(what, mask)
    with torch.no_grad():
        m, pitch, img = _bytes(mask, dev, B, H, W)
        L = ops._L()
        scratch = _scratch(dev, L.s2s_morph_words(B, H, W, 0), what)
        out = torch.empty((B, H, W), dtype=torch.int32, device=dev)
        _native.check(L.s2s_morph_edt(m.data_ptr(), pitch, img, B, H, W, int(to == "foreground"), bound,
                                      scratch.data_ptr(), out.data_ptr(), ops._stream()), what)
    out = out if mask.dim() == 3 else out[0]
    return out if mask.is_cuda else out.to(mask.device)


def _threshold(m: torch.Tensor, pitch: int, img: int, B: int, H: int, W: int, erode: bool, r2: int, dev,
               what: str) -> torch.Tensor:
    L = ops._L()
    scratch = _scratch(dev, L.s2s_morph_words(B, H, W, 0), what)
    out = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    _native.check(L.s2s_morph_threshold(m.data_ptr(), pitch, img, B, H, W, int(erode), r2, scratch.data_ptr(),
                                        out.data_ptr(), ops._stream()), what)
    return out


def mask_morphology(mask: torch.Tensor, op: str, radius: float) -> torch.Tensor:
    """Dilation, erosion, opening or closing (``op`` = ``"dilate"``, ``"erode"``, ``"open"``, ``"close"``) of a bool or
    uint8 mask ``[B, H, W]`` or ``[H, W]`` by the true disc of ``radius`` pixels (any finite radius >= 0, fractional
    ones included): with r2 = floor(radius^2), dilate = D_fg <= r2 and erode = D_bg > r2, one threshold of the exact
    distance transform each; open = dilate(erode(m)), close = erode(dilate(m)).  Returns the mask's dtype, values 0 / 1.

    Border convention: nothing lies outside the image, so dilation sees no foreground there and erosion does not eat in
    from the image edge.  That is ``scipy.ndimage.binary_dilation(..., border_value=0)`` and
    ``binary_erosion(..., border_value=1)`` with a disc structuring element; it is deliberately NOT the convention of
    ``scipy.ndimage.binary_closing`` / ``binary_opening``, which erode with ``border_value=0`` and so strip closed
    tissue off the image edge.  Four launches per threshold, no int32 map, no host synchronisation."""
    what = "mask_morphology"
    B, H, W = _check_mask(mask, what)
    if op not in _OPS:
        raise ValueError(f"{what}: op must be one of {_OPS}, got {op!r}")
    r2 = _squared(radius, "radius", what)
    dev = _device(what, mask)
    with torch.no_grad():
        m, pitch, img = _bytes(mask, dev, B, H, W)
        out = _threshold(m, pitch, img, B, H, W, op in ("erode", "open"), r2, dev, what)
        if op in ("open", "close"):
            out = _threshold(out, W, H * W, B, H, W, op == "close", r2, dev, what)
    return _like(out, mask)


def fill_holes(mask: torch.Tensor, connectivity: int = 4) -> torch.Tensor:
    """The mask with its holes filled: a hole is a component of the background that touches no pixel of the first or
    last row or column.  ``connectivity`` 4 (``scipy.ndimage.binary_fill_holes``) or 8 is the connectivity of the
    BACKGROUND.  Returns the mask's dtype, values 0 / 1.  The background is labelled by the kernels of
    ``label_components``; about 9 bytes of scratch per pixel, no host synchronisation."""
    what = "fill_holes"
    B, H, W = _check_mask(mask, what)
    connectivity = operator.index(connectivity)
    if connectivity not in (4, 8):
        raise ValueError(f"{what}: connectivity must be 4 or 8, got {connectivity}")
    dev = _device(what, mask)
    with torch.no_grad():
        m, pitch, img = _bytes(mask, dev, B, H, W)
        L = ops._L()
        scratch = _scratch(dev, L.s2s_morph_fill_holes_words(B, H, W), what)
        out = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
        _native.check(L.s2s_morph_fill_holes(m.data_ptr(), pitch, img, B, H, W, connectivity, scratch.data_ptr(),
                                             out.data_ptr(), ops._stream()), what)
    return _like(out, mask)


def mask_boundary(mask: torch.Tensor) -> torch.Tensor:
    """The boundary of a mask: its foreground pixels with a 4-neighbour that is background or lies outside the image
    (``m & ~binary_erosion(m, cross, border_value=0)``).  The mask's dtype, values 0 / 1.  ``mask_boundary_agreement``
    evaluates the same rule inside its kernels and never stores it."""
    what = "mask_boundary"
    B, H, W = _check_mask(mask, what)
    dev = _device(what, mask)
    with torch.no_grad():
        m, pitch, img = _bytes(mask, dev, B, H, W)
        out = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
        _native.check(ops._L().s2s_morph_boundary(m.data_ptr(), pitch, img, B, H, W, out.data_ptr(), ops._stream()), what)
    return _like(out, mask)


def _check_agreement(tolerance, percentile, what: str) -> Tuple[int, int]:
    tol2 = _squared(tolerance, "tolerance", what)
    percentile = operator.index(percentile)
    if not 1 <= percentile <= 100:
        raise ValueError(f"{what}: percentile must be an int in 1..100, got {percentile}")
    return tol2, percentile


def mask_boundary_agreement(pred: torch.Tensor, target: torch.Tensor, tolerance: float = 2,
                            percentile: int = 95) -> Dict[str, torch.Tensor]:
    """How far the boundary of ``pred`` lies from the boundary of ``target`` (two masks of one shape, ``[B, H, W]`` or
    ``[H, W]``).  Per sample, S pools the squared distance from every boundary pixel of ``pred`` to the nearest one of
    ``target`` and from every boundary pixel of ``target`` to the nearest one of ``pred``; n = |S|.

    Returns tensors ``[B]`` (scalars without a batch dimension): ``"max_d2"`` int32 = max S; ``"pq_d2"`` int32 = the k-th
    smallest of S, k = (percentile n + 99) // 100 (nearest rank); ``"sum_q8"`` int64 = the sum of isqrt(65536 s), every
    distance in 1/256 pixel, rounded down; ``"within"`` int64 = #{s <= floor(tolerance^2)}; ``"boundary_pred"``,
    ``"boundary_target"`` int64; ``"valid"`` int32; and the fp64 values ``"hausdorff"`` = sqrt(max_d2), ``"hd"`` =
    sqrt(pq_d2), ``"assd"`` = sum_q8 / (256 n) (below the float definition by less than 1/256 pixel) and
    ``"surface_dice"`` = within / n.  Never inf or NaN: with both boundaries empty every integer is 0, surface_dice 1,
    valid 0; with exactly one empty max_d2 = pq_d2 = (H-1)^2 + (W-1)^2, sum_q8 = n isqrt(65536 max_d2), within 0,
    valid 0; otherwise valid 1.  Sixteen launches, no host synchronisation, no boundary or distance map stored."""
    what = "mask_boundary_agreement"
    B, H, W = _check_mask(pred, what)
    if _check_mask(target, what) != (B, H, W) or pred.dim() != target.dim():
        raise ValueError(f"{what}: pred {list(pred.shape)} and target {list(target.shape)} differ in shape")
    tol2, percentile = _check_agreement(tolerance, percentile, what)
    dev = _device(what, pred, target)
    with torch.no_grad():
        p, ppitch, pimg = _bytes(pred, dev, B, H, W)
        t, tpitch, timg = _bytes(target, dev, B, H, W)
        L = ops._L()
        scratch = _scratch(dev, L.s2s_morph_words(B, H, W, 1), what)
        i32 = torch.empty((3, B), dtype=torch.int32, device=dev)
        i64 = torch.empty((4, B), dtype=torch.int64, device=dev)
        f64 = torch.empty((4, B), dtype=torch.float64, device=dev)
        _native.check(L.s2s_morph_boundary_agreement(p.data_ptr(), ppitch, pimg, t.data_ptr(), tpitch, timg, B, H, W, tol2,
                                                     percentile, scratch.data_ptr(), ops._stream()), what)
        _native.check(L.s2s_morph_boundary_finalize(scratch.data_ptr(), B, H, W, i32[0].data_ptr(), i32[1].data_ptr(),
                                                    i64[0].data_ptr(), i64[1].data_ptr(), i64[2].data_ptr(),
                                                    i64[3].data_ptr(), i32[2].data_ptr(), f64[0].data_ptr(),
                                                    f64[1].data_ptr(), f64[2].data_ptr(), f64[3].data_ptr(),
                                                    ops._stream()), what)
    out = {"hausdorff": f64[0], "hd": f64[1], "assd": f64[2], "surface_dice": f64[3], "max_d2": i32[0], "pq_d2": i32[1],
           "sum_q8": i64[0], "within": i64[1], "boundary_pred": i64[2], "boundary_target": i64[3], "valid": i32[2]}
    if pred.dim() == 2:
        out = {k: v[0] for k, v in out.items()}
    return out if pred.is_cuda else {k: v.to(pred.device) for k, v in out.items()}
