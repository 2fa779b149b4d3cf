"""Stain threshold calibration: exact histograms of the stain concentrations and the threshold rules read off them.

``stain_quantify``, ``stain_agreement``, the object calls, ``tile_qc`` and the renderers all take a concentration
threshold whose default (0.2 OD) is a convention.  This module calibrates it on one's own slides without leaving the GPU:

  bin(c)        = clamp(ceil(c * 1024) - 1, 0, 4095) in fp32, so for j in 1..4095:  bin(c) >= j  <=>  c > j / 1024
  hist[o][k][b] = tissue pixels of owner o (a sample, the pooled batch, a whole region) with bin(c_k) = b
  positive[j]   = sum over b >= j of hist[b]: for j >= 1 bit-equal to stain_quantify(thresholds=(j / 1024,) * 3)
  Otsu, triangle (Zack 1977, on the histogram summed in groups of ``coarse`` bins) and quantiles of the tissue pixels

and, for a generated stain against the real one, the threshold on the prediction that reproduces the target's burden or
maximises the Dice of the two positive masks at a given target threshold, with the complete Dice curves.

Concentration, tissue rule and input kinds are those of ``stain_quant``.  Every count is an exact
integer and every rule is evaluated on the device in integers (128 bits where needed) or in doubles produced by a fixed
sequence of operations, so results are bit-equal for host and GPU input, for every banding, run to run, and equal to the
plain Python restatement of tests/stain_calibrate_ref.py.  The batch calls launch on the current stream and wait for
nothing, so they can be captured; ``thresholds_tuple`` is the one place that reads a result back.  GPU only.
DESIGN.md section 3.33.

The reference publishes no stain measurement: these numbers have no counterpart there.
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
from .stain_quant import DEFAULT_THRESHOLDS, _image_kind, _kernel_args, _stain_index

NB = 4096                # bins: SC_NB of csrc/stain_calibrate.hip
BINS_PER_OD = 1024       # bin j holds c in (j / 1024, (j + 1) / 1024]; bin 0 everything <= 1 / 1024, bin 4095 the rest
MAX_QUANTILES = 8        # SC_MAX_Q
ALL_STAINS = 7           # the stain mask of the C ABI: every stain of the basis
_METHODS = ("otsu", "triangle", "quantile")


# ---- arguments -------------------------------------------------------------------------------------------------------
def threshold_bin(threshold) -> int:
    """The bin j of an on-grid threshold j / 1024, j in 1..4095; ``ValueError`` for anything else."""
    try:
        v = float(threshold) * BINS_PER_OD
    except (TypeError, ValueError):
        raise ValueError(f"a threshold must be a number, got {threshold!r}") from None
    if not math.isfinite(v) or v != math.floor(v) or not 1 <= v <= NB - 1:
        raise ValueError(f"the threshold must be j / {BINS_PER_OD} with j in 1..{NB - 1}, got {threshold!r}")
    return int(v)


def _check_coarse(coarse) -> int:
    coarse = operator.index(coarse)
    if coarse < 1 or coarse > NB or coarse & (coarse - 1):
        raise ValueError(f"coarse must be a power of two in 1..{NB}, got {coarse}")
    return coarse


def _check_quantiles(quantiles) -> Tuple[float, ...]:
    try:
        qs = tuple(float(q) for q in quantiles)
    except TypeError:
        raise ValueError(f"quantiles must be a sequence of numbers, got {quantiles!r}") from None
    if len(qs) > MAX_QUANTILES or not all(0.0 <= q <= 1.0 for q in qs):
        raise ValueError(f"quantiles must be at most {MAX_QUANTILES} numbers in [0, 1], got {quantiles!r}")
    return qs


def _check_band_rows(band_rows) -> Optional[int]:
    if band_rows is None:
        return None
    band_rows = operator.index(band_rows)
    if band_rows < 1:
        raise ValueError(f"band_rows must be positive, got {band_rows}")
    return band_rows


def _check_out(out, nhist: int, owners: int, keys: Sequence[str], dev, what: str, target_bin=None, stain=None):
    """The tensors of an earlier result that this call adds into."""
    if not isinstance(out, dict) or "hist" not in out or any(k not in out for k in keys):
        raise TypeError(f"{what}: out must be an earlier result of this call")
    hist = out["hist"]
    if not isinstance(hist, torch.Tensor) or hist.dtype != torch.int64 or tuple(hist.shape) != (owners, nhist, NB) \
            or not hist.is_contiguous():
        raise ValueError(f"{what}: out['hist'] must be a contiguous int64 [{owners}, {nhist}, {NB}] tensor")
    if hist.device != dev:
        raise ValueError(f"{what}: out lives on {hist.device}, the images on {dev}")
    if target_bin is not None and (out.get("target_bin") != target_bin or out.get("stain") != stain):
        raise ValueError(f"{what}: out was taken with another stain or target_threshold")
    return hist


def _new(owners: int, nhist: int, ntissue: int, dev):
    return (torch.empty((owners, nhist, NB), dtype=torch.int64, device=dev),
            torch.empty((owners, ntissue), dtype=torch.int64, device=dev))


# ---- single histograms -----------------------------------------------------------------------------------------------
def _hist_batch(img, kind, B, H, W, table, unmix, white, black, pool, reset, hist, tissue, what):
    L = ops._L()
    if kind == "f32":
        img = img.detach().contiguous()
        rc = L.s2s_stain_hist_f32(img.data_ptr(), B, H, W, table, unmix, white, black, ALL_STAINS, int(pool), reset,
                                  hist.data_ptr(), tissue.data_ptr(), ops._stream())
    else:
        img, pitch, stride = batch_layout(img, what, copy=True)
        rc = L.s2s_stain_hist_u8(img.data_ptr(), pitch, stride, B, 0, H, H, W, table, unmix, white, black, ALL_STAINS,
                                 int(pool), reset, hist.data_ptr(), tissue.data_ptr(), ops._stream())
    _native.check(rc, what)


def stain_histogram(tiles: torch.Tensor, *, stains="hdab", white: int = 220, black: int = 0, pool: bool = False,
                    out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """The concentration histograms of uint8 ``[B, H, W, 3]`` (crop views and any row pitch allowed) or fp32
    ``[B, 3, H, W]`` (the network's range, through the save conversion) images on the GPU.

    Returns device tensors ``"hist"`` int64 ``[B, 3, 4096]`` (``[1, 3, 4096]`` with ``pool``: one histogram over the
    whole batch) and ``"tissue"`` int64 ``[B]`` / ``[1]``; ``hist[o, k].sum() == tissue[o]``.  ``out=h`` adds into an
    earlier result of the same shape and returns it: a dataset-level histogram over a validation loader is
    ``h = stain_histogram(batch, pool=True, out=h)`` per batch (an owner may hold 2^40 pixels).  ``stains`` as
    ``stain_matrix``; ``white`` / ``black`` as ``tissue_counts``.  One launch on the current stream (two without
    ``out``: the first zeroes the result), no host synchronisation; bit-reproducible, and a sample's histogram does not
    depend on its batch mates."""
    what = "stain_histogram"
    kind, B, H, W = _image_kind(tiles, what)
    table, unmix = _kernel_args(stains, DEFAULT_THRESHOLDS)
    white, black = _check_thresholds(white, black)
    dev = gpu_device(what, tiles, host_ok=False)
    owners = 1 if pool else B
    with torch.no_grad():
        if out is None:
            hist, tissue = _new(owners, 3, 1, dev)
            out = {"hist": hist, "tissue": tissue.view(owners)}
            reset = 1
        else:
            hist, reset = _check_out(out, 3, owners, ("tissue",), dev, what), 0
        _hist_batch(tiles, kind, B, H, W, table, unmix, white, black, pool, reset, hist, out["tissue"], what)
    return out


def _region_bands(H: int, band_rows: Optional[int], any_host: bool):
    if band_rows is None:
        band_rows = DEFAULT_HOST_BAND if any_host else H
    return [(r0, min(r0 + band_rows, H)) for r0 in range(0, H, band_rows)]


def region_stain_histogram(region_u8: torch.Tensor, *, band_rows: Optional[int] = None, stains="hdab",
                           white: int = 220, black: int = 0,
                           out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """``stain_histogram`` of one whole uint8 ``[H, W, 3]`` region, on the GPU or on the host, any row pitch: ``"hist"``
    int64 ``[1, 3, 4096]`` and ``"tissue"`` int64 ``[1]`` on the GPU.  A host region is streamed through one pinned
    buffer and one GPU band buffer of ``band_rows`` rows (``None``: a GPU region in one launch, a host region in bands of
    512 rows); the bands add up in integers, so the result is bit-equal for every ``band_rows`` and for host and GPU
    input, and equal to ``stain_histogram(region[None])``.  ``out=`` adds into an earlier result (several regions of
    one slide).  ``region_stain_histogram.last_stats``: bands, band_rows, band_bytes of the last call."""
    what = "region_stain_histogram"
    H, W, _ = check_region(region_u8, what)
    band_rows = _check_band_rows(band_rows)
    table, unmix = _kernel_args(stains, DEFAULT_THRESHOLDS)
    white, black = _check_thresholds(white, black)
    dev = gpu_device(what, region_u8)
    bands = _region_bands(H, band_rows, not region_u8.is_cuda)
    buf_rows = max(r1 - r0 for r0, r1 in bands)
    with torch.no_grad():
        if out is None:
            hist, tissue = _new(1, 3, 1, dev)
            out = {"hist": hist, "tissue": tissue.view(1)}
            reset = 1
        else:
            hist, reset = _check_out(out, 3, 1, ("tissue",), dev, what), 0
        src = BandSource(region_u8, buf_rows, dev)
        for r0, r1 in bands:
            ptr, pitch = gpu_rows(src.rows(r0, r1))
            rc = ops._L().s2s_stain_hist_u8(ptr, pitch, pitch * (r1 - r0), 1, r0, r1 - r0, H, W, table, unmix, white,
                                            black, ALL_STAINS, 0, reset, hist.data_ptr(), out["tissue"].data_ptr(),
                                            ops._stream())
            _native.check(rc, what)
            reset = 0
    region_stain_histogram.last_stats = {"bands": len(bands), "band_rows": buf_rows, "band_bytes": src.band_bytes}
    return out


region_stain_histogram.last_stats: Optional[Dict[str, int]] = None


# ---- the rules -------------------------------------------------------------------------------------------------------
def stain_thresholds(h: Dict[str, torch.Tensor], *, coarse: int = 16,
                     quantiles: Sequence[float] = (0.05,)) -> Dict[str, torch.Tensor]:
    """Thresholds from the histograms ``h`` of ``stain_histogram`` / ``region_stain_histogram`` (``O`` owners), all on
    the device:

    ``"positive"`` int64 ``[O, 3, 4096]``: ``positive[o, k, j]`` tissue pixels with ``c_k > j / 1024`` (``j = 0``: all
    tissue): the burden curve, for ``j >= 1`` bit-equal to ``stain_quantify(thresholds=(j / 1024,) * 3)["positive"]``.
    ``"otsu"``, ``"triangle"`` fp64 ``[O, 3]`` and ``"quantile"`` fp64 ``[O, 3, Q]``: thresholds in OD, each with its
    ``"*_bin"`` (int32; threshold = bin / 1024) and ``"*_valid"`` (int32).  Otsu maximises the between-class variance
    of the binned tissue concentrations; the triangle rule (right tail) runs on the histogram summed in groups of
    ``coarse`` bins (a power of two; 16: 256 groups of 1/64 OD: at a few thousand pixels the fine histogram is too sparse
    and the rule picks a noise spike); quantile ``q`` is the smallest threshold that leaves at most ``floor(q N)`` of the
    ``N`` tissue pixels positive.  ``valid`` is 0 where a rule has no answer (no tissue, a single occupied bin, a peak at
    the tail's end): the bin is then 0 (4095 for a quantile).  One launch, no host synchronisation."""
    if not isinstance(h, dict) or "hist" not in h:
        raise TypeError("stain_thresholds: h must be a result of stain_histogram or region_stain_histogram")
    hist = h["hist"]
    if not isinstance(hist, torch.Tensor) or hist.dtype != torch.int64 or hist.dim() != 3 or \
            tuple(hist.shape[1:]) != (3, NB) or hist.shape[0] < 1:
        raise ValueError(f"stain_thresholds: h['hist'] must be int64 [owners, 3, {NB}]")
    coarse, qs = _check_coarse(coarse), _check_quantiles(quantiles)
    dev = gpu_device("stain_thresholds", hist, host_ok=False)
    O, Q = int(hist.shape[0]), len(qs)
    with torch.no_grad():
        hist = hist.contiguous()
        positive = torch.empty((O, 3, NB), dtype=torch.int64, device=dev)
        bins = torch.empty((O, 3, 2 + Q), dtype=torch.int32, device=dev)
        valid = torch.empty((O, 3, 2 + Q), dtype=torch.int32, device=dev)
        thr = torch.empty((O, 3, 2 + Q), dtype=torch.float64, device=dev)
        rc = ops._L().s2s_stain_thresholds(hist.data_ptr(), 3 * O, coarse, (ctypes.c_double * max(Q, 1))(*qs), Q,
                                           positive.data_ptr(), bins.data_ptr(), valid.data_ptr(), thr.data_ptr(),
                                           ops._stream())
        _native.check(rc, "stain_thresholds")
    return {"positive": positive, "tissue": h["tissue"],
            "otsu": thr[..., 0], "otsu_bin": bins[..., 0], "otsu_valid": valid[..., 0],
            "triangle": thr[..., 1], "triangle_bin": bins[..., 1], "triangle_valid": valid[..., 1],
            "quantile": thr[..., 2:], "quantile_bin": bins[..., 2:], "quantile_valid": valid[..., 2:]}


def calibrate_thresholds(tiles_or_region: torch.Tensor, *, stains="hdab", white: int = 220, black: int = 0,
                         pool: bool = False, band_rows: Optional[int] = None, coarse: int = 16,
                         quantiles: Sequence[float] = (0.05,)) -> Dict[str, torch.Tensor]:
    """Histogram and rules in one call: ``stain_thresholds`` of ``stain_histogram`` (a 4-D batch) or of
    ``region_stain_histogram`` (a uint8 ``[H, W, 3]`` region); the histogram is returned too, as ``"hist"``."""
    coarse, quantiles = _check_coarse(coarse), _check_quantiles(quantiles)
    if isinstance(tiles_or_region, torch.Tensor) and tiles_or_region.dim() == 3:
        h = region_stain_histogram(tiles_or_region, band_rows=band_rows, stains=stains, white=white, black=black)
    else:
        h = stain_histogram(tiles_or_region, stains=stains, white=white, black=black, pool=pool)
    t = stain_thresholds(h, coarse=coarse, quantiles=quantiles)
    t["hist"] = h["hist"]
    return t


def thresholds_tuple(t: Dict[str, torch.Tensor], method: str = "triangle", owner: int = 0, *, quantile: int = 0,
                     fallback: Optional[Sequence[float]] = None) -> Tuple[float, float, float]:
    """Three host floats for the ``thresholds=`` argument of ``stain_quantify`` and its relatives, from the result ``t``
    of ``stain_thresholds``: ``method`` ``"otsu"``, ``"triangle"`` or ``"quantile"`` (the ``quantile``-th of the call)
    of owner ``owner``.  Where the rule was not valid for a stain, ``fallback[k]`` is taken, and ``ValueError`` is raised
    without a ``fallback``.  This is the one call of the module that waits for the device."""
    if method not in _METHODS:
        raise ValueError(f"method must be one of {', '.join(map(repr, _METHODS))}, got {method!r}")
    if not isinstance(t, dict) or method not in t:
        raise TypeError("thresholds_tuple: t must be a result of stain_thresholds or calibrate_thresholds")
    owner, quantile = operator.index(owner), operator.index(quantile)
    thr, ok = t[method], t[method + "_valid"]
    if not 0 <= owner < thr.shape[0]:
        raise ValueError(f"owner must lie in 0..{thr.shape[0] - 1}, got {owner}")
    if method == "quantile":
        if not 0 <= quantile < thr.shape[2]:
            raise ValueError(f"quantile must lie in 0..{thr.shape[2] - 1}, got {quantile}")
        thr, ok = thr[..., quantile], ok[..., quantile]
    if fallback is not None:
        fallback = [float(v) for v in fallback]
        if len(fallback) != 3:
            raise ValueError(f"fallback must be three numbers, got {fallback!r}")
    values, oks = thr[owner].tolist(), ok[owner].tolist()          # the sync
    res = []
    for k in range(3):
        if oks[k]:
            res.append(float(values[k]))
        elif fallback is None:
            raise ValueError(f"thresholds_tuple: the {method} rule has no answer for stain {k} of owner {owner} "
                             "(pass fallback=)")
        else:
            res.append(fallback[k])
    return tuple(res)


# ---- pairs -----------------------------------------------------------------------------------------------------------
def _pair_result(hist, tissue, stain: int, jt: int) -> Dict:
    return {"hist": hist, "tissue_pred": tissue[:, 0], "tissue_target": tissue[:, 1], "tissue": tissue, "stain": stain,
            "target_bin": jt}


def _pair_args(stain, target_threshold):
    return _stain_index(stain), 0 if target_threshold is None else threshold_bin(target_threshold)


def stain_pair_histogram(pred: torch.Tensor, target: torch.Tensor, *, stain: int = 1,
                         target_threshold: Optional[float] = None, stains="hdab", white: int = 220, black: int = 0,
                         pool: bool = False, out: Optional[Dict] = None) -> Dict:
    """The joint histograms of stain ``stain`` of a generated batch and the real one (both as ``stain_histogram``'s
    input, of one kind and shape): ``"hist"`` int64 ``[B, 4, 4096]`` (``[1, 4, 4096]`` pooled) on the device with rows
    0: the prediction's tissue by its bin, 1: the target's tissue by its bin, 2: pixels that are tissue in both by the
    smaller of the two bins, 3 (only with ``target_threshold``): pixels that are tissue in both and positive in the
    target at ``target_threshold`` by the prediction's bin; ``"tissue_pred"`` / ``"tissue_target"`` int64 ``[B]``.
    ``target_threshold`` must lie on the grid (``j / 1024``, ``j`` in 1..4095; ``ValueError`` otherwise).  ``out=``
    adds into an earlier result taken with the same ``stain`` and ``target_threshold``.  One fused launch reads both
    images once; no host synchronisation.  Feed the result to ``match_thresholds``."""
    what = "stain_pair_histogram"
    _check_pair(pred, target, what)
    kind, B, H, W = _image_kind(pred, what)
    stain, jt = _pair_args(stain, target_threshold)
    table, unmix = _kernel_args(stains, DEFAULT_THRESHOLDS)
    white, black = _check_thresholds(white, black)
    dev = gpu_device(what, pred, target, host_ok=False)
    owners = 1 if pool else B
    L = ops._L()
    with torch.no_grad():
        if out is None:
            out, reset = _pair_result(*_new(owners, 4, 2, dev), stain, jt), 1
        else:
            _check_out(out, 4, owners, ("tissue",), dev, what, jt, stain)
            reset = 0
        hist, tissue = out["hist"], out["tissue"]
        if kind == "f32":
            a, b = pred.detach().contiguous(), target.detach().contiguous()
            rc = L.s2s_stain_pair_hist_f32(a.data_ptr(), b.data_ptr(), B, H, W, table, unmix, white, black, stain, jt,
                                           int(pool), reset, hist.data_ptr(), tissue.data_ptr(), ops._stream())
        else:
            a, pa, ia = batch_layout(pred, what, copy=True)
            b, pb, ib = batch_layout(target, what, copy=True)
            rc = L.s2s_stain_pair_hist_u8(a.data_ptr(), pa, ia, b.data_ptr(), pb, ib, B, 0, H, H, W, table, unmix,
                                          white, black, stain, jt, int(pool), reset, hist.data_ptr(),
                                          tissue.data_ptr(), ops._stream())
        _native.check(rc, what)
    return out


def region_stain_pair_histogram(pred_u8: torch.Tensor, target_u8: torch.Tensor, *, band_rows: Optional[int] = None,
                                stain: int = 1, target_threshold: Optional[float] = None, stains="hdab",
                                white: int = 220, black: int = 0, out: Optional[Dict] = None) -> Dict:
    """``stain_pair_histogram`` of one whole uint8 ``[H, W, 3]`` region pair (each on the GPU or on the host, any row
    pitch): one owner.  Banding and its bit equality as ``region_stain_histogram``."""
    what = "region_stain_pair_histogram"
    _check_pair(pred_u8, target_u8, what)
    H, W, _ = check_region(pred_u8, what)
    check_region(target_u8, what)
    band_rows = _check_band_rows(band_rows)
    stain, jt = _pair_args(stain, target_threshold)
    table, unmix = _kernel_args(stains, DEFAULT_THRESHOLDS)
    white, black = _check_thresholds(white, black)
    dev = gpu_device(what, pred_u8, target_u8)
    bands = _region_bands(H, band_rows, not (pred_u8.is_cuda and target_u8.is_cuda))
    buf_rows = max(r1 - r0 for r0, r1 in bands)
    with torch.no_grad():
        if out is None:
            out, reset = _pair_result(*_new(1, 4, 2, dev), stain, jt), 1
        else:
            _check_out(out, 4, 1, ("tissue",), dev, what, jt, stain)
            reset = 0
        src = [BandSource(t, buf_rows, dev) for t in (pred_u8, target_u8)]
        for r0, r1 in bands:
            (pa, pitch_a), (pb, pitch_b) = (gpu_rows(s.rows(r0, r1)) for s in src)
            rc = ops._L().s2s_stain_pair_hist_u8(pa, pitch_a, pitch_a * (r1 - r0), pb, pitch_b, pitch_b * (r1 - r0), 1,
                                                 r0, r1 - r0, H, W, table, unmix, white, black, stain, jt, 0, reset,
                                                 out["hist"].data_ptr(), out["tissue"].data_ptr(), ops._stream())
            _native.check(rc, what)
            reset = 0
    region_stain_pair_histogram.last_stats = {"bands": len(bands), "band_rows": buf_rows,
                                              "band_bytes": sum(s.band_bytes for s in src)}
    return out


region_stain_pair_histogram.last_stats: Optional[Dict[str, int]] = None


def match_thresholds(p: Dict) -> Dict[str, torch.Tensor]:
    """What the pair histograms ``p`` of ``stain_pair_histogram`` / ``region_stain_pair_histogram`` say about the
    threshold to put on the generated stain (``O`` owners, everything on the device, one launch):

    ``"positive_pred"``, ``"positive_target"``, ``"both_common"`` int64 ``[O, 4096]``: the positive counts of either
    image and of their intersection at the common threshold ``j / 1024``; ``"dice_common"`` fp64 ``[O, 4096]``
    = 2 both / (pred + target), 1 where both masks are empty: for ``j >= 1`` the counts behind
    ``stain_agreement(thresholds=(j / 1024,) * 3)``.

    With a ``target_threshold`` ``jt / 1024`` also ``"both_cond"`` int64 and ``"dice_cond"`` fp64 ``[O, 4096]``
    (prediction positive at ``j / 1024``, target positive at ``jt / 1024``) and the two matching rules, fp64 ``[O]`` in OD
    with ``"*_bin"`` and ``"*_valid"`` int32 ``[O]``: ``"match_burden"``, the smallest threshold that minimises
    ``|burden_pred(j) - burden_target(jt)|`` (compared exactly, by cross-multiplication), and ``"best_dice"``, the
    smallest threshold that maximises ``dice_cond``; ``"dice_at_best"``, ``"burden_pred_at_best"`` (at ``best_dice``),
    ``"burden_target"``, ``"burden_pred_at_match"``, ``"burden_abs_err_at_match"``, ``"dice_at_match"`` fp64 ``[O]``.
    ``valid`` is 0 when either image has no tissue."""
    if not isinstance(p, dict) or "hist" not in p or "target_bin" not in p:
        raise TypeError("match_thresholds: p must be a result of stain_pair_histogram or region_stain_pair_histogram")
    hist = p["hist"]
    if not isinstance(hist, torch.Tensor) or hist.dtype != torch.int64 or hist.dim() != 3 or \
            tuple(hist.shape[1:]) != (4, NB) or hist.shape[0] < 1:
        raise ValueError(f"match_thresholds: p['hist'] must be int64 [owners, 4, {NB}]")
    jt = operator.index(p["target_bin"])
    if not 0 <= jt <= NB - 1:
        raise ValueError(f"match_thresholds: target_bin must lie in 0..{NB - 1}, got {jt}")
    dev = gpu_device("match_thresholds", hist, host_ok=False)
    O = int(hist.shape[0])
    with torch.no_grad():
        hist = hist.contiguous()
        counts = torch.empty((O, 4, NB), dtype=torch.int64, device=dev)
        dice = torch.empty((O, 2, NB), dtype=torch.float64, device=dev)
        bins = torch.empty((O, 2), dtype=torch.int32, device=dev)
        valid = torch.empty((O, 2), dtype=torch.int32, device=dev)
        vals = torch.empty((O, 8), dtype=torch.float64, device=dev)
        rc = ops._L().s2s_stain_pair_thresholds(hist.data_ptr(), O, jt, counts.data_ptr(), dice.data_ptr(),
                                                bins.data_ptr(), valid.data_ptr(), vals.data_ptr(), ops._stream())
        _native.check(rc, "match_thresholds")
    res = {"positive_pred": counts[:, 0], "positive_target": counts[:, 1], "both_common": counts[:, 2],
           "dice_common": dice[:, 0]}
    if jt:
        res.update({"both_cond": counts[:, 3], "dice_cond": dice[:, 1],
                    "match_burden": vals[:, 0], "match_burden_bin": bins[:, 0], "match_burden_valid": valid[:, 0],
                    "best_dice": vals[:, 1], "best_dice_bin": bins[:, 1], "best_dice_valid": valid[:, 1],
                    "dice_at_best": vals[:, 2], "burden_pred_at_best": vals[:, 3], "burden_target": vals[:, 4],
                    "burden_pred_at_match": vals[:, 5], "burden_abs_err_at_match": vals[:, 6],
                    "dice_at_match": vals[:, 7]})
    return res
