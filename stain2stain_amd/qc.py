"""Tile quality control: focus, marker ink and dark artefacts of tiles, of a region's tiles and of a region's cells.

The tissue rule (``tissue_counts``, ``translate_region(min_tissue=)``) counts three kinds of pixels as tissue that no
sampler or trainer should see: out-of-focus areas, pathologists' pen marks, and very dark artefacts such as folds, dust
and black ink.  This module measures them in one integer pass over the bytes (``csrc/qc.hip``):

  mx, mn     = max / min(R, G, B);   tissue = mn < white and mx >= black, the rule of ``tissue_counts``
  Y          = (77 R + 150 G + 29 B + 128) >> 8
  L(y, x)    = Y(y-1, x) + Y(y+1, x) + Y(y, x-1) + Y(y, x+1) - 4 Y(y, x)
  focus px   = a tissue pixel with 1 <= y <= H - 2 and 1 <= x <= W - 2 of the IMAGE (for a region the whole region, for
               a batch each tile): its neighbours may lie outside the window, and they may be glass
  green      = tissue and G - max(R, B) >= ink_chroma
  blue       = tissue and B - R >= ink_chroma and G >= R    (haematoxylin has G below R, marker blue has not)
  dark       = tissue and mx < dark

Per window (its rectangle clipped to the image) ``counts[..., 8]`` int64 =
``tissue, focus_n, lap_sum, lap_sq, luma_sum, green, blue, dark`` (``COUNT_KEYS``), and from those integers, in fp64 and
0 where the denominator is 0:

  focus = lap_sq / focus_n - (lap_sum / focus_n)^2      the variance of the Laplacian
  tissue_frac = tissue / area (the window's pixels inside the image);   ink_frac = (green + blue) / tissue
  dark_frac = dark / tissue;   mean_luma = luma_sum / tissue

A numpy int64 restatement is bit-equal.  Because a focus pixel is defined on the image, the counts of disjoint windows
that tile an image add up exactly to the image's: the cell map can be summed into any window (``window_sums``).  The ink
and dark rules and every default threshold are conventions, not calibrations: calibrate on your own slides.

One reduce launch and one small finalize launch per band, on the current stream; with GPU input nothing waits for the
device.  GPU only.  The reference publishes no quality control: these functions have no counterpart there.
"""
from __future__ import annotations

import bisect
import operator
from typing import Dict, List, Optional, Tuple

import torch

from . import _native, ops
from ._regionio import DEFAULT_HOST_BAND, BandSource, batch_layout, check_region, gpu_device, gpu_rows
from .region import _axis_origins, _check_thresholds, plan_tiles
from .stain_quant import _check_cell

CHUNK_ROWS = 16                    # rows of one wave's chunk: QC_CH of csrc/qc.hip
COUNT_KEYS = ("tissue", "focus_n", "lap_sum", "lap_sq", "luma_sum", "green", "blue", "dark")
DERIVED_KEYS = ("focus", "tissue_frac", "ink_frac", "dark_frac", "mean_luma")
# Conventions, not calibrations: marker ink is far more saturated than any mixture of haematoxylin, eosin and DAB, and a
# fold or a speck of dust is darker than stained tissue.  Calibrate on your own slides.
DEFAULT_INK_CHROMA = 40
DEFAULT_DARK = 60


def _check_qc_thresholds(white, black, ink_chroma, dark) -> Tuple[int, int, int, int]:
    white, black = _check_thresholds(white, black)
    ink_chroma, dark = operator.index(ink_chroma), operator.index(dark)
    if not 1 <= ink_chroma <= 255:
        raise ValueError(f"ink_chroma must lie in 1..255, got {ink_chroma}")
    if not 0 <= dark <= 256:
        raise ValueError(f"dark must lie in 0..256, got {dark}")
    return white, black, ink_chroma, dark


def _chunks(win_h: int, win_w: int) -> int:
    n = ops._L().s2s_qc_chunks(win_h, win_w)
    _native.check(n if n < 0 else 0, "qc_chunks")
    return n


def _finalize(slab, owners: int, nchunk: int, accumulate: bool, origins, n: int, H: int, W: int, win_h: int, win_w: int,
              counts, derived, what: str) -> None:
    _native.check(ops._L().s2s_qc_finalize(slab.data_ptr(), owners, nchunk, int(accumulate), origins.data_ptr(), n, H, W,
                                           win_h, win_w, counts.data_ptr(), derived.data_ptr(), ops._stream()), what)


def _result(counts: torch.Tensor, derived: torch.Tensor) -> Dict[str, torch.Tensor]:
    return dict({"counts": counts}, **{k: derived[:, i] for i, k in enumerate(DERIVED_KEYS)})


def tile_qc(tiles_u8: torch.Tensor, *, white: int = 220, black: int = 0, ink_chroma: int = DEFAULT_INK_CHROMA,
            dark: int = DEFAULT_DARK) -> Dict[str, torch.Tensor]:
    """Quality numbers of every tile of a uint8 ``[B, H, W, 3]`` batch on the GPU (crop views, any row pitch): device
    tensors ``"counts"`` int64 ``[B, 8]`` (``COUNT_KEYS``) and ``"focus"``, ``"tissue_frac"``, ``"ink_frac"``,
    ``"dark_frac"``, ``"mean_luma"`` fp64 ``[B]``, as the module states them; each tile is its own image.  ``white`` /
    ``black`` as ``tissue_counts``; ``ink_chroma`` in 1..255 and ``dark`` in 0..256 are conventions: calibrate on your
    own slides.  One reduce and one finalize launch on the current stream, no host synchronisation; bit-reproducible,
    and a tile's values do not depend on its batch mates."""
    what = "tile_qc"
    if not isinstance(tiles_u8, torch.Tensor):
        raise TypeError(f"{what}: tiles must be a torch.Tensor, got {type(tiles_u8).__name__}")
    if tiles_u8.dtype != torch.uint8:
        raise ValueError(f"{what}: tiles must be uint8, got {tiles_u8.dtype}")
    if tiles_u8.dim() != 4 or tiles_u8.shape[3] != 3 or min(tiles_u8.shape) < 1:
        raise ValueError(f"{what}: tiles must be a non-empty [B, H, W, 3] batch, got {list(tiles_u8.shape)}")
    B, H, W = (int(v) for v in tiles_u8.shape[:3])
    thr = _check_qc_thresholds(white, black, ink_chroma, dark)
    if not tiles_u8.is_cuda:
        raise RuntimeError(f"stain2stain_amd: {what} needs GPU tensors (there is no CPU path)")
    dev = tiles_u8.device
    with torch.no_grad():
        t, pitch, stride = batch_layout(tiles_u8, what, copy=True)
        nchunk = _chunks(H, W)
        origins = torch.zeros((1, 2), dtype=torch.int32, device=dev)
        slab = ops._workspace(dev, 2 * B * nchunk * 8, "qc").view(torch.int64)
        counts = torch.empty((B, 8), dtype=torch.int64, device=dev)
        derived = torch.empty((B, len(DERIVED_KEYS)), dtype=torch.float64, device=dev)
        _native.check(ops._L().s2s_qc_windows_u8(t.data_ptr(), pitch, stride, B, 0, H, H, W, origins.data_ptr(), 1, H, W,
                                                 0, H, *thr, slab.data_ptr(), ops._stream()), what)
        _finalize(slab, B, nchunk, False, origins, 1, H, W, H, W, counts, derived, what)
    return _result(counts, derived)


def plan_qc_bands(H: int, band_rows: Optional[int] = None) -> List[Tuple[int, int]]:
    """The bands ``(first image row, end image row)`` a region of ``H`` rows is reduced in: runs of ``band_rows`` rows
    (any number from 1 on; ``None``: one band).  A band's launch reads one more row on either side where the image has
    one.  Pure host arithmetic."""
    H = operator.index(H)
    if H < 1:
        raise ValueError(f"H must be positive, got {H}")
    if band_rows is None:
        return [(0, H)]
    band_rows = operator.index(band_rows)
    if band_rows < 1:
        raise ValueError(f"band_rows must be at least 1, got {band_rows}")
    return [(r0, min(r0 + band_rows, H)) for r0 in range(0, H, band_rows)]


def _reduce_windows(region: torch.Tensor, H: int, W: int, plan: torch.Tensor, nx: int, win_h: int, win_w: int,
                    band_rows, thr, what: str, stats_of) -> Dict[str, torch.Tensor]:
    """counts and derived values of the ``win_h x win_w`` windows at ``plan``, host int32 ``[ny * nx, 2]`` = (top, left),
    a row-major grid whose tops do not decrease.  The origins are uploaded once from pinned memory; a band's launch
    covers only the window rows it touches, and the finalize adds into their counts."""
    dev = gpu_device(what, region)
    if band_rows is None and not region.is_cuda:
        band_rows = DEFAULT_HOST_BAND
    bands = plan_qc_bands(H, band_rows)
    N = int(plan.shape[0])
    tops = plan[::nx, 0].tolist()
    nchunk = _chunks(win_h, win_w)
    buf_rows = min(H, max(r1 - r0 for r0, r1 in bands) + 2)
    with torch.no_grad():
        host = torch.empty((N, 2), dtype=torch.int32, pin_memory=True)
        host.copy_(plan)
        origins = host.to(dev, non_blocking=True)            # the one upload; a band's windows are a slice
        src = BandSource(region, buf_rows, dev)
        # a band adds into the counts of the windows it touches, and leaves the fp64 values of the counts so far
        counts = torch.zeros((N, 8), dtype=torch.int64, device=dev)
        derived = torch.empty((N, len(DERIVED_KEYS)), dtype=torch.float64, device=dev)
        for r0, r1 in bands:
            i0, i1 = bisect.bisect_right(tops, r0 - win_h), bisect.bisect_left(tops, r1)    # tops in (r0 - win_h, r1)
            if i0 >= i1:
                continue
            p0, n = i0 * nx, (i1 - i0) * nx
            b0, b1 = max(r0 - 1, 0), min(r1 + 1, H)
            ptr, pitch = gpu_rows(src.rows(b0, b1))
            slab = ops._workspace(dev, 2 * n * nchunk * 8, "qc").view(torch.int64)
            _native.check(ops._L().s2s_qc_windows_u8(ptr, pitch, pitch * (b1 - b0), 1, b0, b1 - b0, H, W,
                                                     origins[p0:p0 + n].data_ptr(), n, win_h, win_w, r0, r1, *thr,
                                                     slab.data_ptr(), ops._stream()), what)
            _finalize(slab, n, nchunk, True, origins[p0:p0 + n], n, H, W, win_h, win_w, counts[p0:p0 + n],
                      derived[p0:p0 + n], what)
        res = _result(counts, derived)
    stats_of.last_stats = {"bands": len(bands), "band_rows": buf_rows, "windows": N,
                           "band_bytes": src.band_bytes}
    return res


def region_qc(region_u8: torch.Tensor, tile: int = 256, overlap: int = 32, *, band_rows: Optional[int] = None,
              white: int = 220, black: int = 0, ink_chroma: int = DEFAULT_INK_CHROMA,
              dark: int = DEFAULT_DARK) -> Dict[str, torch.Tensor]:
    """``tile_qc``'s numbers for every tile of ``plan_tiles(H, W, tile, overlap)`` of a uint8 ``[H, W, 3]`` region, ``[N]``
    (``"counts"`` ``[N, 8]``) in plan order on the device: what ``qc_keep`` turns into ``translate_region``'s ``keep``.

    The image is the whole region: a tile's border pixels take their Laplacian across the tile's edge.  A tile's area is
    its intersection with the region.  The region may live on the GPU or on the host and have any row pitch.  A GPU
    region takes one launch; a host region is streamed through one pinned buffer and one GPU band buffer in bands of
    ``band_rows`` rows (any number from 1 on; default 512) plus a row of halo on either side.  The counts are bit-equal
    for host and GPU input and for every ``band_rows``.  ``region_qc.last_stats``: bands, band_rows, windows, band_bytes
    of the last call.  Thresholds as ``tile_qc``."""
    H, W, _ = check_region(region_u8, "region_qc")
    plan = plan_tiles(H, W, tile, overlap)
    thr = _check_qc_thresholds(white, black, ink_chroma, dark)
    tile = operator.index(tile)
    nx = len(_axis_origins(W, tile, operator.index(overlap)))
    return _reduce_windows(region_u8, H, W, plan, nx, min(tile, H), min(tile, W), band_rows, thr, "region_qc", region_qc)


region_qc.last_stats: Optional[Dict[str, int]] = None


def region_qc_map(region_u8: torch.Tensor, cell: int = 256, *, band_rows: Optional[int] = None, white: int = 220,
                  black: int = 0, ink_chroma: int = DEFAULT_INK_CHROMA,
                  dark: int = DEFAULT_DARK) -> Dict[str, torch.Tensor]:
    """``tile_qc``'s numbers per ``cell`` x ``cell`` cell of a uint8 ``[H, W, 3]`` region: ``[Gy, Gx]`` (``"counts"``
    ``[Gy, Gx, 8]``) on the device, Gy = ceil(H / cell), Gx = ceil(W / cell); ragged edge cells count their own pixels.
    The cells tile the region, so their counts add up exactly to those of the whole region, and ``window_sums`` turns
    the map into the counts of any window of whole cells.  Input, banding and bit equality as ``region_qc``;
    ``region_qc_map.last_stats`` likewise."""
    H, W, _ = check_region(region_u8, "region_qc_map")
    cell = _check_cell(cell)
    thr = _check_qc_thresholds(white, black, ink_chroma, dark)
    Gy, Gx = -(-H // cell), -(-W // cell)
    ys, xs = torch.arange(Gy, dtype=torch.int32) * cell, torch.arange(Gx, dtype=torch.int32) * cell
    plan = torch.stack([ys[:, None].expand(Gy, Gx), xs[None, :].expand(Gy, Gx)], -1).reshape(-1, 2)
    res = _reduce_windows(region_u8, H, W, plan, Gx, min(cell, H), min(cell, W), band_rows, thr, "region_qc_map",
                          region_qc_map)
    return {k: v.reshape(Gy, Gx, *v.shape[1:]) for k, v in res.items()}


region_qc_map.last_stats: Optional[Dict[str, int]] = None


def _fraction(v, name: str) -> float:
    v = float(v)
    if not 0.0 <= v <= 1.0:
        raise ValueError(f"qc_keep: {name} must lie in [0, 1], got {v}")
    return v


def qc_keep(q: Dict[str, torch.Tensor], *, min_tissue: float = 0.05, max_ink: float = 0.01, max_dark: float = 0.5,
            min_focus: Optional[float] = None, min_focus_rel: Optional[float] = None) -> torch.Tensor:
    """Which tiles of a ``tile_qc`` / ``region_qc`` / ``region_qc_map`` result are worth a sampler or a training loop: a
    bool tensor of ``q``'s shape on ``q``'s device.  A tile is kept iff ``tissue_frac >= min_tissue`` and ``ink_frac <=
    max_ink`` and ``dark_frac <= max_dark`` and, when given, ``focus >= min_focus`` and ``focus >= min_focus_rel * m``,
    m the lower median (element (n - 1) // 2 of the sorted values) of ``focus`` over the n tiles that pass the tissue
    test; with n = 0 the relative test drops nothing.  Focus depends on the scanner, the objective and the stain, which
    is why the relative form exists; all defaults are conventions: calibrate on your own slides.  Torch on the device,
    no host synchronisation."""
    if not isinstance(q, dict) or any(k not in q for k in DERIVED_KEYS[:4]):
        raise TypeError("qc_keep: q must be the dict tile_qc, region_qc or region_qc_map return")
    min_tissue, max_ink, max_dark = (_fraction(min_tissue, "min_tissue"), _fraction(max_ink, "max_ink"),
                                     _fraction(max_dark, "max_dark"))
    for name, v in (("min_focus", min_focus), ("min_focus_rel", min_focus_rel)):
        if v is not None and not float(v) >= 0.0:
            raise ValueError(f"qc_keep: {name} must be None or a number >= 0, got {v}")
    focus = q["focus"]
    has_tissue = q["tissue_frac"] >= min_tissue
    keep = has_tissue & (q["ink_frac"] <= max_ink) & (q["dark_frac"] <= max_dark)
    if min_focus is not None:
        keep = keep & (focus >= float(min_focus))
    if min_focus_rel is not None and focus.numel() > 0:
        inf = torch.full_like(focus, float("inf"))
        ordered = torch.sort(torch.where(has_tissue, focus, inf).reshape(-1)).values
        n = has_tissue.sum()
        median = ordered.gather(0, ((n - 1) // 2).clamp(min=0).reshape(1))
        bound = torch.where(n > 0, float(min_focus_rel) * median, torch.full_like(median, float("-inf")))
        keep = keep & (focus >= bound)
    return keep


def window_sums(counts: torch.Tensor, win: int = 2, stride: int = 1) -> torch.Tensor:
    """Box sums of ``win`` x ``win`` cells of an int64 map ``[Gy, Gx, ...]`` (``region_qc_map``'s ``"counts"``, or
    ``region_stain_map``'s counts) at every ``stride``-th cell: int64 ``[(Gy - win) // stride + 1, (Gx - win) // stride + 1,
    ...]`` on the map's device, entry (i, j) the sum over cells ``[i stride, i stride + win) x [j stride, j stride + win)``.
    Because the cell counts are additive these are the exact counts of windows of several cells: what one scores crop
    windows with when mining training tiles.  Plain torch (an integral image by ``cumsum``) on either device."""
    if not isinstance(counts, torch.Tensor):
        raise TypeError(f"window_sums: counts must be a torch.Tensor, got {type(counts).__name__}")
    if counts.dtype != torch.int64 or counts.dim() < 2 or counts.shape[0] < 1 or counts.shape[1] < 1:
        raise ValueError(f"window_sums: counts must be a non-empty int64 [Gy, Gx, ...] map, got {counts.dtype} "
                         f"{list(counts.shape)}")
    win, stride = operator.index(win), operator.index(stride)
    Gy, Gx = int(counts.shape[0]), int(counts.shape[1])
    if not 1 <= win <= min(Gy, Gx):
        raise ValueError(f"window_sums: win must lie in 1..{min(Gy, Gx)} for a {Gy} x {Gx} map, got {win}")
    if stride < 1:
        raise ValueError(f"window_sums: stride must be at least 1, got {stride}")
    S = torch.zeros((Gy + 1, Gx + 1) + tuple(counts.shape[2:]), dtype=torch.int64, device=counts.device)
    S[1:, 1:] = counts.cumsum(0).cumsum(1)
    box = S[win:, win:] - S[:-win, win:] - S[win:, :-win] + S[:-win, :-win]
    return box[::stride, ::stride].contiguous()
