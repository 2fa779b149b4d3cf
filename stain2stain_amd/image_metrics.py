"""Image quality of generated tiles and whole regions against their paired targets: PSNR, SSIM, MAE and MSE.

Each metric is per sample, over all channels; L is the data range:

  mse  = mean (a - b)^2        mae = mean |a - b|        psnr = 10 log10(L^2 / mse), +inf when mse == 0
  ssim = Wang et al. 2004 as skimage (``gaussian_weights=True, use_sample_covariance=False``) and torchmetrics define
         it: a ``window`` x ``window`` separable Gaussian (sigma 1.5, normalised), C1 = (k1 L)^2, C2 = (k2 L)^2, biased
         local moments, only the (H - window + 1)(W - window + 1) positions per channel whose window lies inside the
         image, the mean over channels and positions

One fused pass and one small finalize launch (``csrc/image_metrics.hip``): no blurred map goes to memory, nothing waits
for the device, and the results are device tensors that feed ``EvalAccumulator``.  DESIGN.md section 3.15.

The reference publishes no image metric (its inference scripts plot source | target | generated): these numbers have no
counterpart there.
"""
from __future__ import annotations

import ctypes
import math
import operator
from typing import Callable, Dict, List, Optional, Tuple

import torch

from . import _native, ops
from ._regionio import BandSource, batch_layout, check_region, gpu_device, gpu_rows

BLOCK_ROWS = 32          # valid rows (and columns) of one workgroup: IQ_TH of csrc/image_metrics.hip
MAX_WINDOW = 11
KEYS = ("psnr", "ssim", "mae", "mse")
_DEFAULT_HOST_BLOCKS = 32          # block rows per band of a host region when band_rows is not given


def gaussian_taps(window: int = 11, sigma: float = 1.5) -> List[float]:
    """The ``window`` taps exp(-(i - window // 2)^2 / (2 sigma^2)), normalised to sum 1 (in double)."""
    window = _check_window(window)
    sigma = float(sigma)
    if not sigma > 0.0:
        raise ValueError(f"sigma must be positive, got {sigma}")
    r = window // 2
    w = [math.exp(-((i - r) ** 2) / (2.0 * sigma * sigma)) for i in range(window)]
    s = math.fsum(w)
    return [v / s for v in w]


def _check_window(window) -> int:
    window = operator.index(window)
    if window < 1 or window > MAX_WINDOW or window % 2 == 0:
        raise ValueError(f"window must be odd and in [1, {MAX_WINDOW}], got {window}")
    return window


def plan_bands(H: int, window: int = 11, band_rows: Optional[int] = None) -> List[Tuple[int, int, int, int]]:
    """The bands a region of ``H`` rows is scored in: ``(first block row, block rows, first image row, end image row)``.

    The valid SSIM rows 0 .. H - window are cut into fixed blocks of ``BLOCK_ROWS``; a band is a whole number of
    consecutive blocks and reads the image rows of its blocks plus the window's ``window - 1`` halo rows, so consecutive
    bands re-read that halo.  ``band_rows`` is the height of the band buffer in image rows: a band takes
    ``(band_rows - (window - 1)) // BLOCK_ROWS`` blocks (at least one is needed); ``None``: one band.  Every block row
    and so every valid row lies in exactly one band whatever ``band_rows`` is, which is why the result does not depend
    on it.  Pure host arithmetic."""
    H, window = operator.index(H), _check_window(window)
    if H < window:
        raise ValueError(f"the image must have at least window = {window} rows, got {H}")
    nby = -(-(H - window + 1) // BLOCK_ROWS)
    if band_rows is None:
        per = nby
    else:
        band_rows = operator.index(band_rows)
        per = (band_rows - (window - 1)) // BLOCK_ROWS
        if per < 1:
            raise ValueError(f"band_rows must be at least {BLOCK_ROWS + window - 1} "
                             f"(one block of {BLOCK_ROWS} rows plus the window's halo), got {band_rows}")
    bands = []
    for by0 in range(0, nby, per):
        n = min(per, nby - by0)
        bands.append((by0, n, by0 * BLOCK_ROWS, min(H, (by0 + n) * BLOCK_ROWS + window - 1)))
    return bands


def _metric_args(window, sigma, k1, k2):
    window = _check_window(window)
    taps = gaussian_taps(window, sigma)
    return window, (ctypes.c_float * window)(*taps), float(k1), float(k2)


def _check_pair(pred, target, what: str) -> None:
    for name, t in (("pred", pred), ("target", target)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(t).__name__}")
    if pred.dtype != target.dtype:
        raise ValueError(f"{what}: pred is {pred.dtype} but target is {target.dtype}")
    if tuple(pred.shape) != tuple(target.shape):
        raise ValueError(f"{what}: pred {list(pred.shape)} and target {list(target.shape)} differ in shape")


def _finalize(part: torch.Tensor, B: int, C: int, H: int, W: int, window: int, L: float,
              device) -> Dict[str, torch.Tensor]:
    out = torch.empty((4, B), dtype=torch.float32, device=device)
    _native.check(ops._L().s2s_image_quality_finalize(part.data_ptr(), B, C, H, W, window, float(L), out.data_ptr(),
                                                      ops._stream()), "image_quality_finalize")
    return {k: out[i] for i, k in enumerate(KEYS)}


def _partials(device, B: int, H: int, W: int, window: int) -> torch.Tensor:
    nblk = ops._L().s2s_image_quality_blocks(H, W, window)
    _native.check(nblk if nblk < 0 else 0, "image_quality_blocks")
    return ops._workspace(device, 2 * 3 * B * nblk, "image_quality").view(torch.float64)


def image_quality(pred: torch.Tensor, target: torch.Tensor, *, quantize: bool = True, window: int = 11,
                  sigma: float = 1.5, k1: float = 0.01, k2: float = 0.03) -> Dict[str, torch.Tensor]:
    """{"psnr", "ssim", "mae", "mse"} of ``pred`` against ``target``, each an fp32 ``[B]`` tensor on their device.

    fp32 ``[B, C, H, W]`` pairs (C in 1..4) are in the network's normalised range.  ``quantize=True`` scores what one
    would measure from the saved PNGs: both go through the reference's save conversion,
    ``trunc(clamp((x * 0.5 + 0.5) * 255, 0, 255))``, and L = 255.  ``quantize=False`` scores ``clamp(x * 0.5 + 0.5, 0,
    1)`` with L = 1.  uint8 ``[B, H, W, 3]`` pairs (row and sample pitches are free, pixels contiguous within a row)
    are scored as they are, L = 255; ``quantize`` plays no role.

    One metrics kernel and one finalize kernel on the current stream, no host synchronisation: usable inside
    ``ops.capture_graph``; the partial sums live in an ``ops.workspace_owner`` workspace.  Bit-reproducible, and a
    sample's values do not depend on its batch mates.  There is no CPU path."""
    _check_pair(pred, target, "image_quality")
    window, taps, k1, k2 = _metric_args(window, sigma, k1, k2)
    if pred.dtype == torch.float32:
        if pred.dim() != 4 or not 1 <= pred.shape[1] <= 4:
            raise ValueError(f"image_quality: fp32 images must be [B, C, H, W] with C in 1..4, got {list(pred.shape)}")
        B, C, H, W = (int(v) for v in pred.shape)
    elif pred.dtype == torch.uint8:
        if pred.dim() != 4 or pred.shape[3] != 3:
            raise ValueError(f"image_quality: uint8 images must be [B, H, W, 3], got {list(pred.shape)}")
        B, H, W, C = (int(v) for v in pred.shape)
    else:
        raise ValueError(f"image_quality: images must be float32 or uint8, got {pred.dtype}")
    if B < 1:
        raise ValueError("image_quality: empty batch")
    if H < window or W < window:
        raise ValueError(f"image_quality: H and W must be at least the window ({window}), got {H} x {W}")
    part = _partials(gpu_device("image_quality", pred, target, host_ok=False), B, H, W, window)
    L = ops._L()
    if pred.dtype == torch.float32:
        a, b = pred.detach().contiguous(), target.detach().contiguous()
        rc = L.s2s_image_quality_f32(a.data_ptr(), b.data_ptr(), B, C, H, W, int(bool(quantize)), window, taps, k1, k2,
                                     part.data_ptr(), ops._stream())
        rng = 255.0 if quantize else 1.0
    else:
        (a, pa, ia), (b, pb, ib) = (batch_layout(t, "image_quality", copy=True) for t in (pred, target))
        rc = L.s2s_image_quality_u8(a.data_ptr(), pa, ia, b.data_ptr(), pb, ib, B, 0, H, H, W, 0,
                                    -(-(H - window + 1) // BLOCK_ROWS), window, taps, k1, k2, part.data_ptr(),
                                    ops._stream())
        rng = 255.0
    _native.check(rc, "image_quality")
    return _finalize(part, B, C, H, W, window, rng, pred.device)


def region_quality(pred_u8: torch.Tensor, target_u8: torch.Tensor, *, band_rows: Optional[int] = None,
                   window: int = 11, sigma: float = 1.5, k1: float = 0.01, k2: float = 0.03) -> Dict[str, torch.Tensor]:
    """{"psnr", "ssim", "mae", "mse"} of a whole uint8 ``[H, W, 3]`` region against its target, as fp32 device scalars.

    Each image may live on the GPU or on the host and have any row pitch (a crop view of a slide array works without a
    copy).  The region is scored in bands of whole blocks of ``BLOCK_ROWS`` valid rows (``plan_bands``); a host image
    is streamed through a pinned staging buffer and a GPU band buffer of ``band_rows`` rows, the window's halo rows read
    again by the next band, so GPU memory does not grow with H beyond the three partial sums per block.  ``band_rows``
    ``None``: a GPU image is scored in one launch, a host image in bands of 32 blocks.  The partial sums are indexed by
    the block's place in the whole region and summed in a fixed order: the result is bit-equal for every ``band_rows``
    and for host and GPU input.  ``region_quality.last_stats``: bands, band_rows, band_bytes of the last call."""
    _check_pair(pred_u8, target_u8, "region_quality")
    H, W, _ = check_region(pred_u8, "region_quality")
    check_region(target_u8, "region_quality")
    window, taps, k1, k2 = _metric_args(window, sigma, k1, k2)
    if H < window or W < window:
        raise ValueError(f"region_quality: H and W must be at least the window ({window}), got {H} x {W}")
    any_host = not (pred_u8.is_cuda and target_u8.is_cuda)
    if band_rows is None and any_host:
        band_rows = _DEFAULT_HOST_BLOCKS * BLOCK_ROWS + window - 1
    bands = plan_bands(H, window, band_rows)
    dev = gpu_device("region_quality", pred_u8, target_u8)
    buf_rows = max(r1 - r0 for _, _, r0, r1 in bands)
    with torch.no_grad():
        src = [BandSource(t, buf_rows, dev) for t in (pred_u8, target_u8)]
        part = _partials(dev, 1, H, W, window)
        L = ops._L()
        for by0, nby, r0, r1 in bands:
            a, b = src[0].rows(r0, r1), src[1].rows(r0, r1)
            (pa, pitch_a), (pb, pitch_b) = gpu_rows(a), gpu_rows(b)
            rc = L.s2s_image_quality_u8(pa, pitch_a, pitch_a * (r1 - r0), pb, pitch_b, pitch_b * (r1 - r0), 1, r0,
                                        r1 - r0, H, W, by0, nby, window, taps, k1, k2, part.data_ptr(), ops._stream())
            _native.check(rc, "region_quality")
        out = _finalize(part, 1, 3, H, W, window, 255.0, dev)
    region_quality.last_stats = {"bands": len(bands), "band_rows": buf_rows,
                                 "band_bytes": sum(s.band_bytes for s in src)}
    return {k: v[0] for k, v in out.items()}


region_quality.last_stats: Optional[Dict[str, int]] = None


def generation_quality(sampler: Callable, source: torch.Tensor, target: torch.Tensor, accumulator=None,
                       stain: Optional[dict] = None, **metric_args) -> Dict[str, torch.Tensor]:
    """``image_quality(sampler(source), target, **metric_args)``: the per-sample dict of one generated batch.  A sampler
    that returns a tuple (image, ...) is scored on its image.  ``accumulator`` (an ``EvalAccumulator``): the batch means
    of the keys are added to it with weight B, so its epoch mean is the mean over every image.  ``stain``: a dict of
    ``stain_quant.stain_agreement``'s keyword arguments (``{}`` for its defaults) adds ``"stain/burden_abs_err"``,
    ``"stain/dice"`` and ``"stain/iou"``; ``None`` (the default) changes nothing."""
    pred = sampler(source)
    if isinstance(pred, tuple):
        pred = pred[0]
    if not isinstance(pred, torch.Tensor):
        raise TypeError(f"generation_quality: the sampler must return a tensor, got {type(pred).__name__}")
    values = image_quality(pred, target, **metric_args)
    if stain is not None:
        from . import stain_quant
        values.update(stain_quant.agreement_values(pred, target, stain))
    if accumulator is not None:
        accumulator.add({k: v.mean() for k, v in values.items()}, int(pred.shape[0]))
    return values
