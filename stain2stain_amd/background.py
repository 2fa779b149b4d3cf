"""Stain background subtraction: grey-scale opening and top-hat on the GPU, and the stain numbers taken after it.

Every burden, object count and Dice of ``stain_quant``, ``objects`` and ``stain_calibrate`` compares the raw
concentration ``c_k`` with one global threshold.  Real DAB carries a non-specific haze that varies over a section, and a
sampler adds a smooth one of its own; a global threshold counts it as positive area and merges the plaques that stand on
it.  The classic remedy sits between colour deconvolution and the threshold: estimate the background as the grey-scale
opening of the concentration map by a disc larger than the objects, subtract it, threshold what stands out (the white
top-hat).  Everything here is integer arithmetic on the 1/1024 OD grid:

  grid        b = bin(c_k) = clamp(ceil(c_k * 1024) - 1, 0, 4095), the fp32 sequence of ``stain_calibrate``, for EVERY
              pixel (no tissue gate).  b >= j <=> c_k > j / 1024, so nothing subtracted gives ``stain_quantify``'s counts.
  footprints  "disc": {(dy, dx): dy^2 + dx^2 <= floor(radius^2)}, the r2 convention of ``mask_morphology``; "square":
              |dy|, |dx| <= floor(radius).  There is nothing outside the image: minima and maxima run over the in-image
              pixels of the footprint only, so erosion does not eat in from the edge and dilation brings nothing in
              (``scipy.ndimage.grey_erosion(mode="constant", cval=<type max>)`` / ``grey_dilation(cval=<type min>)``).
  operations  erode = min, dilate = max over the footprint; open = dilate(erode(x)); close = erode(dilate(x));
              tophat = x - open(x); bothat = close(x) - x, formed in 32 bits and saturated to the dtype.
  smoothing   a raw opening follows noise troughs, so the background may be taken from a box mean first:
              s = (2 * sum + n) // (2 * n), sum and n over the in-image pixels of the (2 * smooth + 1)^2 window
              (``smooth=0``: s = b).
  corrected   bg = open(s, radius, footprint); t = max(b - bg, 0); ``radius=None``: bg = 0, t = b.
  positive    tissue (the rule of ``stain_quantify``: ``white``, ``black``) and t >= j, j = ``threshold_bin(threshold)``:
              the threshold must lie on the grid (j / 1024, j in 1..4095; ``ValueError`` otherwise).

Border behaviour: "nothing outside the image" means an opening UNDERESTIMATES a background that rises towards an image
edge (the footprint there reaches only inwards, towards lower values), so a tile cut from a region keeps a rim of haze
within ``radius`` of its edges.  ``region_stain_quantify_corrected`` is the answer for tiles cut from a region: it
streams the region in bands that carry a halo of ``2 * floor(radius) + smooth`` rows and is exact at every band seam.

The kernels are ``csrc/grey_morph.hip``: span tables of power-of-two row windows, a column gather whose work is linear in
the radius, one counting kernel.  ``radius <= MAX_RADIUS`` = 128, ``smooth <= MAX_SMOOTH`` = 16, ``H, W <= 32767``,
``B <= 65535``.  Every call runs on the current stream without host synchronisation, with scratch from the shared
workspace; results are bit-equal to tests/background_ref.py (scipy and numpy), for host and GPU input and for every
banding.  GPU only.  DESIGN.md section 3.36.

The reference publishes no stain measurement: these numbers have no counterpart there.
"""
from __future__ import annotations

import math
import operator
from typing import Dict, Optional, Tuple

import torch

from . import _native, ops
from ._regionio import BandSource, batch_layout, check_region, gpu_device, gpu_rows
from .image_metrics import _check_pair
from .objects import _FG_POSITIVE, _check_mpp, _check_pixels, _density, _label, _object_args, _stain_dict
from .region import _check_thresholds
from .stain_calibrate import NB, _check_band_rows, _check_out, _region_bands, threshold_bin
from .stain_quant import DEFAULT_THRESHOLDS, _image_kind, _kernel_args, _stain_index

MAX_RADIUS = 128             # GM_MAX_RADIUS of csrc/grey_morph.hip
MAX_SMOOTH = 16              # GM_MAX_SMOOTH
MAX_SIDE = 32767
MAX_BATCH = 65535
DEFAULT_THRESHOLD = 205 / 1024           # the grid point next to the conventional 0.2 OD: a convention, not a calibration
_OPS = ("erode", "dilate", "open", "close", "tophat", "bothat")
_FOOTPRINTS = ("disc", "square")
_OPEN = 2
_DTYPES = {torch.uint8: 0, torch.int16: 1}


# ---- arguments -------------------------------------------------------------------------------------------------------
def _check_radius(radius, what: str, none_ok: bool = False) -> Optional[float]:
    if radius is None and none_ok:
        return None
    if isinstance(radius, (bool, str)) or radius is None:
        raise TypeError(f"{what}: radius must be a number, got {type(radius).__name__}")
    try:
        radius = float(radius)
    except (TypeError, ValueError):
        raise TypeError(f"{what}: radius must be a number, got {type(radius).__name__}") from None
    if not (math.isfinite(radius) and radius >= 0.0):
        raise ValueError(f"{what}: radius must be finite and not negative, got {radius}")
    if radius > MAX_RADIUS:
        raise ValueError(f"{what}: radius must be at most MAX_RADIUS = {MAX_RADIUS}, got {radius}")
    return radius


def _check_footprint(footprint, radius: float, what: str) -> Tuple[int, int]:
    """(footprint code, size) of the C ABI: the disc's floor(radius^2), the square's floor(radius)."""
    if footprint not in _FOOTPRINTS:
        raise ValueError(f"{what}: footprint must be one of {_FOOTPRINTS}, got {footprint!r}")
    if footprint == "disc":
        return 0, int(math.floor(radius * radius))
    return 1, int(math.floor(radius))


def _check_smooth(smooth, what: str) -> int:
    if isinstance(smooth, bool):
        raise TypeError(f"{what}: smooth must be an int, got bool")
    smooth = operator.index(smooth)
    if not 0 <= smooth <= MAX_SMOOTH:
        raise ValueError(f"{what}: smooth must lie in 0..{MAX_SMOOTH}, got {smooth}")
    return smooth


def _check_sides(B: int, H: int, W: int, what: str) -> None:
    if B > MAX_BATCH:
        raise ValueError(f"{what}: at most {MAX_BATCH} samples, got {B}")
    if H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError(f"{what}: {H} x {W} exceeds the limit of {MAX_SIDE} pixels a side")


def _check_grey(x, what: str) -> Tuple[int, int, int]:
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{what}: the image must be a torch.Tensor, got {type(x).__name__}")
    if x.dtype not in _DTYPES:
        raise ValueError(f"{what}: the image must be uint8 or int16, got {x.dtype}")
    if x.dim() not in (2, 3):
        raise ValueError(f"{what}: the image must be [B, H, W] or [H, W], got {list(x.shape)}")
    B = int(x.shape[0]) if x.dim() == 3 else 1
    H, W = int(x.shape[-2]), int(x.shape[-1])
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"{what}: empty image {list(x.shape)}")
    _check_sides(B, H, W, what)
    return B, H, W


class _Args:
    """What the corrected calls share, checked before anything touches the device."""

    def __init__(self, what, radius, threshold, stain, stains, smooth, footprint, white, black):
        self.what = what
        self.radius = _check_radius(radius, what, none_ok=True)
        self.j = threshold_bin(threshold)
        self.stain = _stain_index(stain)
        self.smooth = _check_smooth(smooth, what)
        self.fp, self.size = _check_footprint(footprint, self.radius or 0.0, what)
        self.table, self.unmix = _kernel_args(stains, DEFAULT_THRESHOLDS)
        self.white, self.black = _check_thresholds(white, black)
        self.halo = 0 if self.radius is None else 2 * int(math.floor(self.radius)) + self.smooth


# ---- launches --------------------------------------------------------------------------------------------------------
def _morph(src_ptr: int, dtype: int, pitch: int, img: int, B: int, H: int, W: int, op: int, fp: int, size: int, dev,
           out: torch.Tensor, what: str) -> None:
    L = ops._L()
    words = L.s2s_grey_words(B, H, W, fp, size)
    _native.check(words if words < 0 else 0, what)
    scratch = ops._workspace(dev, words, "grey_morph")
    _native.check(L.s2s_grey_morph(src_ptr, dtype, pitch, img, B, H, W, op, fp, size, scratch.data_ptr(), out.data_ptr(),
                                   ops._stream()), what)


def _planes(dev, N: int, n16: int):
    """``n16`` int16 planes and one byte plane of N elements each from the shared workspace."""
    n = (N + 3) // 4 * 4                                     # every plane starts 4-byte aligned
    buf = ops._workspace(dev, (2 * n * n16 + n) // 4, "background").view(torch.int16)
    planes = [buf[i * n:i * n + N] for i in range(n16)]
    tissue = buf[n16 * n:].view(torch.uint8)[:N]
    return planes, tissue


def _bins_batch(img: torch.Tensor, kind: str, B: int, H: int, W: int, a: "_Args", bins: torch.Tensor,
                tissue: Optional[torch.Tensor]) -> None:
    L = ops._L()
    tp = tissue.data_ptr() if tissue is not None else 0
    if kind == "f32":
        img = img.detach().contiguous()
        rc = L.s2s_grey_bins_f32(img.data_ptr(), B, H, W, a.table, a.unmix, a.white, a.black, a.stain, bins.data_ptr(), tp,
                                 ops._stream())
    else:
        img, pitch, stride = batch_layout(img, a.what, copy=True)
        rc = L.s2s_grey_bins_u8(img.data_ptr(), pitch, stride, B, H, W, a.table, a.unmix, a.white, a.black, a.stain,
                                bins.data_ptr(), tp, ops._stream())
    _native.check(rc, a.what)


def _background(b: torch.Tensor, s: torch.Tensor, bg: torch.Tensor, B: int, H: int, W: int, a: "_Args", dev) -> None:
    """bg = open(box mean(b)) on dense int16 planes; ``s`` holds the mean."""
    src = b
    if a.smooth:
        _native.check(ops._L().s2s_grey_box_mean(b.data_ptr(), B, H, W, a.smooth, s.data_ptr(), ops._stream()), a.what)
        src = s
    _morph(src.data_ptr(), 1, W, H * W, B, H, W, _OPEN, a.fp, a.size, dev, bg, a.what)


def _new_counts(owners: int, dev):
    return (torch.empty((owners, 3), dtype=torch.int64, device=dev),
            torch.empty((owners, 3, NB), dtype=torch.int64, device=dev))


def _result(counts: torch.Tensor, hist: torch.Tensor, a: "_Args") -> Dict:
    owners = counts.shape[0]
    fin = torch.empty((owners, 2), dtype=torch.float64, device=counts.device)
    _native.check(ops._L().s2s_grey_corrected_finalize(counts.data_ptr(), owners, fin.data_ptr(), ops._stream()), a.what)
    return {"hist": hist, "counts": counts, "tissue": counts[:, 0], "positive": counts[:, 1], "sum_t": counts[:, 2],
            "burden": fin[:, 0], "mean_t": fin[:, 1], "stain": a.stain, "threshold_bin": a.j}


def _count_batch(tiles: torch.Tensor, kind: str, B: int, H: int, W: int, a: "_Args", pool: bool, reset: int,
                 counts: torch.Tensor, hist: torch.Tensor, want_mask: bool, want_corrected: bool, dev):
    """The launches of one batch: bins, background, counts.  (mask, corrected), either None."""
    N = B * H * W
    (b, s, bg), tissue = _planes(dev, N, 3)
    _bins_batch(tiles, kind, B, H, W, a, b, tissue)
    if a.radius is not None:
        _background(b, s, bg, B, H, W, a, dev)
    mask = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if want_mask else None
    corrected = torch.empty((B, H, W), dtype=torch.int16, device=dev) if want_corrected else None
    rc = ops._L().s2s_grey_corrected(b.data_ptr(), bg.data_ptr() if a.radius is not None else 0, tissue.data_ptr(), B, H,
                                     W, 0, H, a.j, a.stain, int(pool), reset, counts.data_ptr(), hist.data_ptr(),
                                     mask.data_ptr() if want_mask else 0, corrected.data_ptr() if want_corrected else 0,
                                     H * W, ops._stream())
    _native.check(rc, a.what)
    return mask, corrected


def _tiles(tiles, what: str):
    kind, B, H, W = _image_kind(tiles, what)
    _check_sides(B, H, W, what)
    return kind, B, H, W


# ---- public calls ----------------------------------------------------------------------------------------------------
def grey_morphology(x: torch.Tensor, op: str, radius: float, footprint: str = "disc") -> torch.Tensor:
    """Grey-scale ``"erode"``, ``"dilate"``, ``"open"``, ``"close"``, ``"tophat"`` or ``"bothat"`` of a uint8 or int16
    image ``[B, H, W]`` or ``[H, W]`` by a flat ``"disc"`` (``dy^2 + dx^2 <= floor(radius^2)``) or ``"square"``
    (``|dy|, |dx| <= floor(radius)``); any finite radius in 0..``MAX_RADIUS``.  Returns the image's dtype and shape.

    There is nothing outside the image (see the module docstring): equal to ``scipy.ndimage.grey_erosion`` /
    ``grey_dilation`` with ``mode="constant"`` and ``cval`` the type's maximum / minimum, and to the compositions of the
    two; the top-hats are differences in 32 bits saturated to the dtype.  On 0 / 1 masks erode, dilate, open and close
    equal ``mask_morphology``.  Row-strided GPU views are read in place; a host image is uploaded whole and the result
    comes back to the host.  Work is linear in the radius; no host synchronisation."""
    what = "grey_morphology"
    B, H, W = _check_grey(x, what)
    if op not in _OPS:
        raise ValueError(f"{what}: op must be one of {_OPS}, got {op!r}")
    fp, size = _check_footprint(footprint, _check_radius(radius, what), what)
    dev = gpu_device(what, x)
    with torch.no_grad():
        m = x.detach() if x.is_cuda else x.detach().to(dev)
        m = m if m.dim() == 3 else m[None]
        pitch = m.stride(1) if H > 1 else W
        img = m.stride(0) if B > 1 else pitch * H
        if (W > 1 and m.stride(2) != 1) or pitch < W or img < pitch * H:
            m = m.contiguous()
            pitch, img = W, W * H
        out = torch.empty((B, H, W), dtype=x.dtype, device=dev)
        _morph(m.data_ptr(), _DTYPES[x.dtype], pitch, img, B, H, W, _OPS.index(op), fp, size, dev, out, what)
    out = out if x.dim() == 3 else out[0]
    return out if x.is_cuda else out.to(x.device)


def concentration_bins(tiles: torch.Tensor, *, stain: int = 1, stains="hdab") -> torch.Tensor:
    """``bin(c_stain)`` of every pixel of uint8 ``[B, H, W, 3]`` or fp32 ``[B, 3, H, W]`` images (as ``stain_quantify``)
    on the GPU: int16 ``[B, H, W]``, values 0..4095, no tissue gate.  One launch."""
    what = "concentration_bins"
    kind, B, H, W = _tiles(tiles, what)
    a = _Args(what, None, DEFAULT_THRESHOLD, stain, stains, 0, "disc", 220, 0)
    dev = gpu_device(what, tiles, host_ok=False)
    with torch.no_grad():
        out = torch.empty((B, H, W), dtype=torch.int16, device=dev)
        _bins_batch(tiles, kind, B, H, W, a, out, None)
    return out


def stain_background(tiles: torch.Tensor, radius: float, *, stain: int = 1, stains="hdab", smooth: int = 2,
                     footprint: str = "disc") -> torch.Tensor:
    """The background estimate of stain ``stain``: ``open(box mean(bin(c_stain)), radius, footprint)`` as int16
    ``[B, H, W]`` on the 1/1024 OD grid.  ``radius`` should exceed the radius of the largest object to keep."""
    what = "stain_background"
    kind, B, H, W = _tiles(tiles, what)
    _check_radius(radius, what)
    a = _Args(what, radius, DEFAULT_THRESHOLD, stain, stains, smooth, footprint, 220, 0)
    dev = gpu_device(what, tiles, host_ok=False)
    with torch.no_grad():
        (b, s), _ = _planes(dev, B * H * W, 2)
        out = torch.empty((B, H, W), dtype=torch.int16, device=dev)
        _bins_batch(tiles, kind, B, H, W, a, b, None)
        _background(b, s, out, B, H, W, a, dev)
    return out


def stain_quantify_corrected(tiles: torch.Tensor, radius: Optional[float], threshold: float = DEFAULT_THRESHOLD, *,
                             stain: int = 1, stains="hdab", smooth: int = 2, footprint: str = "disc", white: int = 220,
                             black: int = 0, pool: bool = False, out: Optional[Dict] = None,
                             return_mask: bool = False, return_corrected: bool = False) -> Dict:
    """The burden of stain ``stain`` after background subtraction, for uint8 ``[B, H, W, 3]`` or fp32 ``[B, 3, H, W]``
    images on the GPU: t = max(b - open(box mean(b)), 0), positive = tissue and t >= ``threshold`` * 1024.

    Returns device tensors per owner (``[B]``, or ``[1]`` with ``pool``: one owner over the batch): ``"tissue"``,
    ``"positive"`` int64; ``"burden"`` fp64 = positive / max(tissue, 1); ``"sum_t"`` int64 (t over tissue, in 1/1024 OD)
    and ``"mean_t"`` fp64 = sum_t / max(tissue, 1); ``"hist"`` int64 ``[owners, 3, 4096]`` whose row ``stain`` is the
    histogram of t over tissue (the other rows stay zero), so the result feeds ``stain_thresholds`` and the threshold
    can be calibrated AFTER the subtraction; the suffix sums of that row are ``positive`` at every threshold.
    ``return_mask``: ``"mask"`` uint8 ``[B, H, W]`` (bit 0 positive, bit 1 tissue: what the labelling takes);
    ``return_corrected``: ``"corrected"`` int16 ``[B, H, W]`` = t.  ``radius=None`` subtracts nothing: ``positive`` and
    ``tissue`` are those of ``stain_quantify(thresholds=(threshold,) * 3)``.  ``out=q`` adds into an earlier result of
    the same stain, threshold and owners and returns it (``pool=True, out=q`` per batch: a loader).  ``threshold`` must
    lie on the grid (``ValueError``).  No host synchronisation."""
    what = "stain_quantify_corrected"
    kind, B, H, W = _tiles(tiles, what)
    a = _Args(what, radius, threshold, stain, stains, smooth, footprint, white, black)
    dev = gpu_device(what, tiles, host_ok=False)
    owners = 1 if pool else B
    with torch.no_grad():
        if out is None:
            counts, hist = _new_counts(owners, dev)
            reset = 1
        else:
            hist = _check_out(out, 3, owners, ("counts", "stain", "threshold_bin"), dev, what)
            if out["stain"] != a.stain or out["threshold_bin"] != a.j:
                raise ValueError(f"{what}: out was taken with another stain or threshold")
            counts, reset = out["counts"], 0
        mask, corrected = _count_batch(tiles, kind, B, H, W, a, pool, reset, counts, hist, return_mask, return_corrected,
                                       dev)
        res = _result(counts, hist, a)
    if out is not None:
        out.update(res)
        res = out
    if return_mask:
        res["mask"] = mask
    if return_corrected:
        res["corrected"] = corrected
    return res


def stain_objects_corrected(tiles: torch.Tensor, radius: Optional[float], threshold: float = DEFAULT_THRESHOLD, *,
                            stain: int = 1, stains="hdab", smooth: int = 2, footprint: str = "disc", white: int = 220,
                            black: int = 0, connectivity: int = 8, min_area: int = 1,
                            max_objects: Optional[int] = None, mpp: Optional[float] = None,
                            return_labels: bool = False) -> Dict[str, torch.Tensor]:
    """``stain_objects`` on the corrected positive mask: the keys of ``stain_objects`` (``count``, ``tissue``,
    ``positive``, ``burden``, ``largest``, ``size_hist``, ``per_mm2`` with ``mpp``, the table with ``max_objects``,
    ``labels`` on request).  The labels feed ``object_features``, ``split_objects``, ``object_zones`` and
    ``render_classes`` unchanged."""
    what = "stain_objects_corrected"
    kind, B, H, W = _tiles(tiles, what)
    _check_pixels(H, W, what)
    a = _Args(what, radius, threshold, stain, stains, smooth, footprint, white, black)
    connectivity, min_area, M = _object_args(connectivity, min_area, max_objects, what)
    mpp = _check_mpp(mpp, what)
    dev = gpu_device(what, tiles, host_ok=False)
    with torch.no_grad():
        counts, hist = _new_counts(B, dev)
        mask, _ = _count_batch(tiles, kind, B, H, W, a, False, 1, counts, hist, True, False, dev)
        tissue = counts[:, 0].contiguous()
        res = _label(mask.data_ptr(), W, H * W, _FG_POSITIVE, B, H, W, dev, connectivity, min_area, M, what)
        burden, per_mm2 = _density(res, tissue, mpp, what)
    return _stain_dict(res, tissue, burden, per_mm2, M, return_labels)


_PAIR_KEYS = ("burden_pred", "burden_target", "burden_abs_err", "dice", "iou")


def stain_agreement_corrected(generated: torch.Tensor, target: torch.Tensor, radius: Optional[float],
                              threshold: float = DEFAULT_THRESHOLD, *, stain: int = 1, stains="hdab", smooth: int = 2,
                              footprint: str = "disc", white: int = 220, black: int = 0) -> Dict[str, torch.Tensor]:
    """``stain_agreement`` after background subtraction of both images: ``{"burden_pred", "burden_target",
    "burden_abs_err", "dice", "iou"}``, each fp64 ``[B]`` on the device; Dice and IoU are those of the two corrected
    positive masks and 1 when both are empty.  Inputs as ``stain_agreement``."""
    what = "stain_agreement_corrected"
    _check_pair(generated, target, what)
    kind, B, H, W = _tiles(generated, what)
    a = _Args(what, radius, threshold, stain, stains, smooth, footprint, white, black)
    dev = gpu_device(what, generated, target, host_ok=False)
    L = ops._L()
    with torch.no_grad():
        sides = []
        for t in (generated, target):
            counts, hist = _new_counts(B, dev)
            mask, _ = _count_batch(t, kind, B, H, W, a, False, 1, counts, hist, True, False, dev)
            sides.append((counts, mask))
        both = torch.empty((B,), dtype=torch.int64, device=dev)
        out = torch.empty((B, 5), dtype=torch.float64, device=dev)
        _native.check(L.s2s_grey_pair(sides[0][1].data_ptr(), sides[1][1].data_ptr(), B, H, W, both.data_ptr(),
                                      ops._stream()), what)
        _native.check(L.s2s_grey_pair_finalize(sides[0][0].data_ptr(), sides[1][0].data_ptr(), both.data_ptr(), B,
                                               out.data_ptr(), ops._stream()), what)
    return {k: out[:, i] for i, k in enumerate(_PAIR_KEYS)}


def region_stain_quantify_corrected(region_u8: torch.Tensor, radius: Optional[float],
                                    threshold: float = DEFAULT_THRESHOLD, *, band_rows: Optional[int] = None,
                                    stain: int = 1, stains="hdab", smooth: int = 2, footprint: str = "disc",
                                    white: int = 220, black: int = 0, return_mask: bool = False,
                                    return_corrected: bool = False) -> Dict:
    """``stain_quantify_corrected`` of one whole uint8 ``[H, W, 3]`` region on the GPU or on the host (any row pitch): one
    owner, the keys of the batch call with a leading 1, ``"mask"`` / ``"corrected"`` ``[H, W]`` on request.

    The region is streamed in bands of ``band_rows`` rows (``None``: a GPU region in one piece, a host region in bands of
    512 rows), each with a halo of ``2 * floor(radius) + smooth`` rows above and below (cut at the region's own edges)
    that is computed but not counted: every counted pixel sees exactly the rows it sees in the whole region, so the
    result is bit-equal for every ``band_rows``, for host and GPU input, and equal to the batch call on
    ``region[None]``.  A host region goes through one pinned buffer and one GPU band buffer.
    ``region_stain_quantify_corrected.last_stats``: bands, band_rows (halo included), band_bytes of the last call."""
    what = "region_stain_quantify_corrected"
    H, W, _ = check_region(region_u8, what)
    _check_sides(1, H, W, what)
    band_rows = _check_band_rows(band_rows)
    a = _Args(what, radius, threshold, stain, stains, smooth, footprint, white, black)
    dev = gpu_device(what, region_u8)
    bands = [(max(r0 - a.halo, 0), r0, r1, min(r1 + a.halo, H))
             for r0, r1 in _region_bands(H, band_rows, not region_u8.is_cuda)]
    buf_rows = max(h1 - h0 for h0, _, _, h1 in bands)
    L = ops._L()
    with torch.no_grad():
        counts, hist = _new_counts(1, dev)
        mask = torch.empty((H, W), dtype=torch.uint8, device=dev) if return_mask else None
        corrected = torch.empty((H, W), dtype=torch.int16, device=dev) if return_corrected else None
        src = BandSource(region_u8, buf_rows, dev)
        (b, s, bg), tissue = _planes(dev, buf_rows * W, 3)
        reset = 1
        for h0, r0, r1, h1 in bands:
            rows = h1 - h0
            ptr, pitch = gpu_rows(src.rows(h0, h1))
            _native.check(L.s2s_grey_bins_u8(ptr, pitch, pitch * rows, 1, rows, W, a.table, a.unmix, a.white, a.black,
                                             a.stain, b.data_ptr(), tissue.data_ptr(), ops._stream()), what)
            if a.radius is not None:
                _background(b, s, bg, 1, rows, W, a, dev)
            rc = L.s2s_grey_corrected(b.data_ptr(), bg.data_ptr() if a.radius is not None else 0, tissue.data_ptr(), 1,
                                      rows, W, r0 - h0, r1 - r0, a.j, a.stain, 0, reset, counts.data_ptr(),
                                      hist.data_ptr(), mask[r0:].data_ptr() if return_mask else 0,
                                      corrected[r0:].data_ptr() if return_corrected else 0, (r1 - r0) * W, ops._stream())
            _native.check(rc, what)
            reset = 0
        res = _result(counts, hist, a)
    if return_mask:
        res["mask"] = mask
    if return_corrected:
        res["corrected"] = corrected
    region_stain_quantify_corrected.last_stats = {"bands": len(bands), "band_rows": buf_rows,
                                                  "band_bytes": src.band_bytes}
    return res


region_stain_quantify_corrected.last_stats: Optional[Dict[str, int]] = None
