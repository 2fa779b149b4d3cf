"""Stain quantification: colour deconvolution and the positive-area burden of tiles, batches and whole regions.

The number a pathologist reads off an IHC slide is the share of tissue that is positive.  Following Ruifrok & Johnston
(2001) a pixel's optical densities are unmixed into stain concentrations, and a pixel is positive for a stain when it is
tissue and its concentration exceeds a threshold:

  od(u)    = -log10(max(u, 1) / 255) per uint8 channel value, from a 256-entry fp32 table computed here in double
  basis    = 3 x 3, rows = the stains' unit OD vectors (``stain_matrix``); m = its inverse, in double, rounded to fp32
  c_k      = ((od_r * m_rk) + (od_g * m_gk)) + (od_b * m_bk), every product and sum rounded to fp32 on its own
  tissue   = min(R, G, B) < white and max(R, G, B) >= black, the rule of ``tissue_counts``
  positive = tissue and c_k > threshold_k;    burden_k = positive_k / max(tissue, 1)   (an all-glass tile gives 0)
  mean_od_k = sum over tissue of max(c_k, 0) / max(tissue, 1)

A numpy float32 restatement of these lines is bit-equal to the kernels (``csrc/stain_quant.hip``), so the counts are
exact integers.  fp32 ``[B, 3, H, W]`` input is in the network's range and always goes through the save conversion
``trunc(clamp((x * 0.5 + 0.5) * 255, 0, 255))`` of ``image_quality(quantize=True)``: the number reported is what one
would measure from the saved PNG.  There is no unquantised mode (it would need a device log and lose the exactness).

Everything is one fused pass plus one small finalize launch on the current stream; nothing waits for the device, so the
batch wrappers can be captured.  GPU only.  DESIGN.md section 3.17.

The reference publishes no stain measurement: these numbers have no counterpart there.
"""
from __future__ import annotations

import ctypes
import math
import operator
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _native, ops
from ._regionio import DEFAULT_HOST_BAND, BandSource, batch_layout, check_region, gpu_device, gpu_rows
from .image_metrics import _check_pair
from .region import _check_thresholds

CHUNK_ROWS = 16          # rows of one workgroup's chunk: SQ_CH of csrc/stain_quant.hip
# A convention, not a calibration: 0.2 OD is a common starting point for "DAB positive" in open-source pathology tools.
# The right value depends on the scanner, the chromogen and the counterstain: calibrate on your own slides.
DEFAULT_THRESHOLDS = (0.2, 0.2, 0.2)

_NAMED = {
    # Ruifrok & Johnston 2001, table of the H DAB vectors; the residual is the cross product
    "hdab": [[0.650, 0.704, 0.286], [0.268, 0.570, 0.776]],
    # the same paper's H E DAB basis as scikit-image's rgb_from_hed states it
    "hed": [[0.65, 0.70, 0.29], [0.07, 0.99, 0.11], [0.27, 0.57, 0.78]],
}
_SINGULAR = 1e-6         # |det| of a basis of unit rows lies in [0, 1]


def od_table() -> torch.Tensor:
    """The 256 optical densities -log10(max(u, 1) / 255) as fp32 (computed in double, rounded once); u = 0 takes the
    entry of u = 1."""
    return torch.tensor([-math.log10(max(u, 1) / 255.0) for u in range(256)], dtype=torch.float64).to(torch.float32)


def stain_matrix(stains="hdab") -> torch.Tensor:
    """The stain basis as a float64 ``[3, 3]`` host tensor whose rows are unit OD vectors.

    ``stains``: ``"hdab"`` (haematoxylin, DAB, residual), ``"hed"`` (haematoxylin, eosin, DAB) or an array-like ``[2, 3]``
    or ``[3, 3]`` of the stains' OD vectors.  Rows are normalised to unit length; a missing third row is the normalised
    cross product of the first two.  A zero row or a singular basis raises ``ValueError``."""
    if isinstance(stains, str):
        if stains not in _NAMED:
            raise ValueError(f"stains must be one of {', '.join(map(repr, _NAMED))} or an array, got {stains!r}")
        stains = _NAMED[stains]
    m = torch.as_tensor(stains, dtype=torch.float64).detach().to("cpu")
    if m.dim() != 2 or m.shape[1] != 3 or m.shape[0] not in (2, 3):
        raise ValueError(f"a stain basis must be [2, 3] or [3, 3], got {list(m.shape)}")
    if not torch.isfinite(m).all():
        raise ValueError("a stain basis must be finite")
    rows = [[float(v) for v in r] for r in m.tolist()]
    unit = []
    for r in rows:
        n = math.sqrt(math.fsum(v * v for v in r))
        if n == 0.0:
            raise ValueError("a stain vector has zero length")
        unit.append([v / n for v in r])
    if len(unit) == 2:
        a, b = unit
        c = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
        n = math.sqrt(math.fsum(v * v for v in c))
        if n < _SINGULAR:
            raise ValueError("the stain basis is singular (the two vectors are parallel)")
        unit.append([v / n for v in c])
    if abs(_det(unit)) < _SINGULAR:
        raise ValueError("the stain basis is singular")
    return torch.tensor(unit, dtype=torch.float64)


def _det(m) -> float:
    return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
            + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))


def unmix_matrix(stains="hdab") -> torch.Tensor:
    """fp32 ``[3, 3]`` m with concentrations = od @ m: the inverse of ``stain_matrix(stains)`` taken in double (the
    adjugate over the determinant) and rounded to fp32 once.  These are the nine numbers the kernels get."""
    M = stain_matrix(stains).tolist()
    d = _det(M)
    cof = [[M[(j + 1) % 3][(i + 1) % 3] * M[(j + 2) % 3][(i + 2) % 3]
            - M[(j + 1) % 3][(i + 2) % 3] * M[(j + 2) % 3][(i + 1) % 3] for j in range(3)] for i in range(3)]
    return torch.tensor([[v / d for v in r] for r in cof], dtype=torch.float64).to(torch.float32)


def _thresholds(thresholds) -> List[float]:
    try:
        thr = [float(v) for v in thresholds]
    except TypeError:
        raise ValueError(f"thresholds must be three numbers, got {thresholds!r}") from None
    if len(thr) != 3 or not all(math.isfinite(v) for v in thr):
        raise ValueError(f"thresholds must be three finite numbers, got {thresholds!r}")
    return thr


def _stain_index(stain) -> int:
    stain = operator.index(stain)
    if not 0 <= stain <= 2:
        raise ValueError(f"stain must be 0, 1 or 2, got {stain}")
    return stain


def _kernel_args(stains, thresholds):
    """(od table, unmix) as the host float arrays of the C ABI."""
    m = unmix_matrix(stains).reshape(-1).tolist()
    thr = torch.tensor(_thresholds(thresholds), dtype=torch.float32).tolist()
    return (ctypes.c_float * 256)(*od_table().tolist()), (ctypes.c_float * 12)(*m, *thr)


def _image_kind(img, what: str) -> Tuple[str, int, int, int]:
    """("u8" | "f32", B, H, W) of a batch; raises on anything else."""
    if not isinstance(img, torch.Tensor):
        raise TypeError(f"{what}: images must be torch.Tensor, got {type(img).__name__}")
    if img.dtype == torch.uint8:
        if img.dim() != 4 or img.shape[3] != 3:
            raise ValueError(f"{what}: uint8 images must be [B, H, W, 3], got {list(img.shape)}")
        kind, (B, H, W) = "u8", (int(v) for v in img.shape[:3])
    elif img.dtype == torch.float32:
        if img.dim() != 4 or img.shape[1] != 3:
            raise ValueError(f"{what}: fp32 images must be [B, 3, H, W], got {list(img.shape)}")
        kind, B, (H, W) = "f32", int(img.shape[0]), (int(v) for v in img.shape[2:])
    else:
        raise ValueError(f"{what}: images must be uint8 or float32, got {img.dtype}")
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"{what}: empty image batch {list(img.shape)}")
    return kind, B, H, W


def _chunks(cell_h: int, cell_w: int) -> int:
    n = ops._L().s2s_stain_quant_chunks(cell_h, cell_w)
    _native.check(n if n < 0 else 0, "stain_quant_chunks")
    return n


def _partials(device, owners: int, nchunk: int, K: int) -> torch.Tensor:
    return ops._workspace(device, 2 * owners * nchunk * K, "stain_quant").view(torch.float64)


def _finalize(part: torch.Tensor, owners: int, nchunk: int, paired: bool, device):
    counts = torch.empty((owners, 5 if paired else 4), dtype=torch.int64, device=device)
    sums = None if paired else torch.empty((owners, 3), dtype=torch.float64, device=device)
    out = torch.empty((owners, 5 if paired else 6), dtype=torch.float32, device=device)
    _native.check(ops._L().s2s_stain_quant_finalize(part.data_ptr(), owners, nchunk, int(paired), counts.data_ptr(),
                                                    0 if paired else sums.data_ptr(), out.data_ptr(), ops._stream()),
                  "stain_quant_finalize")
    return counts, sums, out


def _single_dict(counts, sums, out, shape) -> Dict[str, torch.Tensor]:
    return {"tissue": counts[:, 0].reshape(shape), "positive": counts[:, 1:].reshape(*shape, 3),
            "od_sum": sums.reshape(*shape, 3), "burden": out[:, :3].reshape(*shape, 3),
            "mean_od": out[:, 3:].reshape(*shape, 3)}


_PAIR_KEYS = ("burden_pred", "burden_target", "burden_abs_err", "dice", "iou")


def _pair_dict(out, shape) -> Dict[str, torch.Tensor]:
    return {k: out[:, i].reshape(shape) for i, k in enumerate(_PAIR_KEYS)}


def _launch_batch(a: torch.Tensor, b: Optional[torch.Tensor], kind: str, B: int, H: int, W: int, table, unmix,
                  white: int, black: int, stain: int, what: str):
    """One reduce launch over a batch (one owner per sample) and its finalize."""
    paired = b is not None
    nchunk = _chunks(H, W)
    K = 5 if paired else 7
    dev = a.device
    part = _partials(dev, B, nchunk, K)
    L = ops._L()
    if kind == "f32":
        a = a.detach().contiguous()
        b = b.detach().contiguous() if paired else None
        rc = L.s2s_stain_quant_f32(a.data_ptr(), b.data_ptr() if paired else 0, int(paired), B, H, W, table, unmix,
                                   white, black, stain, part.data_ptr(), ops._stream())
    else:
        a, pa, ia = batch_layout(a, what, copy=True)
        if paired:
            b, pb, ib = batch_layout(b, what, copy=True)
        rc = L.s2s_stain_quant_u8(a.data_ptr(), pa, ia, b.data_ptr() if paired else 0, pb if paired else 0,
                                  ib if paired else 0, int(paired), B, 0, H, H, W, H, W, 0, -(-H // CHUNK_ROWS), table,
                                  unmix, white, black, stain, part.data_ptr(), ops._stream())
    _native.check(rc, what)
    return _finalize(part, B, nchunk, paired, dev)


def stain_quantify(img: torch.Tensor, *, stains="hdab", thresholds: Sequence[float] = DEFAULT_THRESHOLDS,
                   white: int = 220, black: int = 0) -> Dict[str, torch.Tensor]:
    """Per-sample stain burden of uint8 ``[B, H, W, 3]`` (crop views and any row pitch allowed) or fp32 ``[B, 3, H, W]``
    (the network's range, through the save conversion) images on the GPU.

    Returns device tensors: ``"tissue"`` int64 ``[B]``, ``"positive"`` int64 ``[B, 3]`` (tissue pixels with
    ``c_k > thresholds[k]``), ``"od_sum"`` fp64 ``[B, 3]`` (sum over tissue of ``max(c_k, 0)``), ``"burden"`` fp32
    ``[B, 3]`` = positive / max(tissue, 1) and ``"mean_od"`` fp32 ``[B, 3]`` = od_sum / max(tissue, 1).  ``stains`` as
    ``stain_matrix``; ``white`` / ``black`` as ``tissue_counts``.  The default ``thresholds`` are a convention, not
    calibrated values: calibrate them on your own slides.  One reduce kernel and one finalize kernel on the current
    stream, no host synchronisation; bit-reproducible, and a sample's values do not depend on its batch mates."""
    kind, B, H, W = _image_kind(img, "stain_quantify")
    table, unmix = _kernel_args(stains, thresholds)
    white, black = _check_thresholds(white, black)
    gpu_device("stain_quantify", img, host_ok=False)
    with torch.no_grad():
        counts, sums, out = _launch_batch(img, None, kind, B, H, W, table, unmix, white, black, 0, "stain_quantify")
    return _single_dict(counts, sums, out, (B,))


def stain_agreement(pred: torch.Tensor, target: torch.Tensor, *, stain: int = 1, stains="hdab",
                    thresholds: Sequence[float] = DEFAULT_THRESHOLDS, white: int = 220,
                    black: int = 0) -> Dict[str, torch.Tensor]:
    """How well a generated stain agrees with the real one on what is positive: ``{"burden_pred", "burden_target",
    "burden_abs_err", "dice", "iou"}``, each fp32 ``[B]`` on the device, for stain ``stain`` of the basis (1: DAB in
    ``"hdab"``).  Dice and IoU are those of the two positive masks and 1 when both are empty.  Inputs as
    ``stain_quantify``, both of one kind and shape.  One fused launch that reads both images once plus the finalize."""
    _check_pair(pred, target, "stain_agreement")
    kind, B, H, W = _image_kind(pred, "stain_agreement")
    stain = _stain_index(stain)
    table, unmix = _kernel_args(stains, thresholds)
    white, black = _check_thresholds(white, black)
    gpu_device("stain_agreement", pred, target, host_ok=False)
    with torch.no_grad():
        _, _, out = _launch_batch(pred, target, kind, B, H, W, table, unmix, white, black, stain, "stain_agreement")
    return _pair_dict(out, (B,))


def stain_separate(img: torch.Tensor, *, stains="hdab") -> torch.Tensor:
    """The stain concentrations of every pixel as fp32 ``[B, 3, H, W]``; input as ``stain_quantify``."""
    kind, B, H, W = _image_kind(img, "stain_separate")
    table, unmix = _kernel_args(stains, DEFAULT_THRESHOLDS)
    dev = gpu_device("stain_separate", img, host_ok=False)
    with torch.no_grad():
        out = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
        if kind == "f32":
            a, pitch, stride = img.detach().contiguous(), W, 3 * H * W
        else:
            a, pitch, stride = batch_layout(img, "stain_separate", copy=True)
        rc = ops._L().s2s_stain_separate(a.data_ptr(), int(kind == "f32"), pitch, stride, B, H, W, table, unmix,
                                         out.data_ptr(), ops._stream())
        _native.check(rc, "stain_separate")
    return out


def plan_stain_bands(H: int, cell: int, band_rows: Optional[int] = None) -> List[Tuple[int, int, int, int]]:
    """The bands a region of ``H`` rows is reduced in: ``(first chunk row, chunk rows, first image row, end image row)``.

    Every cell row (``cell`` image rows) is cut into ``ceil(cell / CHUNK_ROWS)`` chunk rows of ``CHUNK_ROWS`` rows, the
    last one shorter when ``cell`` is no multiple; a band is a run of consecutive chunk rows whose image rows fit
    ``band_rows`` (at least ``CHUNK_ROWS``; ``None``: one band).  Where a chunk's partial sums are stored depends on its
    place in the region alone, which is why the result does not depend on ``band_rows``.  Pure host arithmetic."""
    H, cell = operator.index(H), operator.index(cell)
    if H < 1 or cell < 1:
        raise ValueError(f"H and cell must be positive, got {H} and {cell}")
    ncy = -(-cell // CHUNK_ROWS)
    total = -(-H // cell) * ncy
    if band_rows is None:
        return [(0, total, 0, H)]
    band_rows = operator.index(band_rows)
    if band_rows < CHUNK_ROWS:
        raise ValueError(f"band_rows must be at least {CHUNK_ROWS}, got {band_rows}")

    def rows(g):
        gy, cy = divmod(g, ncy)
        top = gy * cell + cy * CHUNK_ROWS
        return min(top, H), min(top + CHUNK_ROWS, (gy + 1) * cell, H)

    bands, g0 = [], 0
    while g0 < total:
        r0, r1 = rows(g0)
        g = g0 + 1
        while g < total and min(rows(g)[1], H) - r0 <= band_rows:
            r1 = max(r1, rows(g)[1])
            g += 1
        bands.append((g0, g - g0, r0, r1))
        g0 = g
    return bands


def _check_cell(cell) -> int:
    cell = operator.index(cell)
    if cell < 1:
        raise ValueError(f"cell must be positive, got {cell}")
    return cell


def _reduce_region(images, H: int, W: int, cell_h: int, cell_w: int, band_rows, table, unmix, white, black, stain,
                   what: str, stats_of):
    """The reduce launches of one region (or a pair), band by band, and the finalize."""
    paired = len(images) == 2
    any_host = not all(t.is_cuda for t in images)
    if band_rows is None and any_host:
        band_rows = DEFAULT_HOST_BAND
    bands = plan_stain_bands(H, cell_h, band_rows)
    dev = gpu_device(what, *images)
    Gy, Gx = -(-H // cell_h), -(-W // cell_w)
    nchunk = _chunks(cell_h, cell_w)
    K = 5 if paired else 7
    buf_rows = max(r1 - r0 for _, _, r0, r1 in bands)
    with torch.no_grad():
        src = [BandSource(t, buf_rows, dev) for t in images]
        part = _partials(dev, Gy * Gx, nchunk, K)
        L = ops._L()
        for g0, ng, r0, r1 in bands:
            views = [s.rows(r0, r1) for s in src]
            pa, pitch_a = gpu_rows(views[0])
            pb, pitch_b = gpu_rows(views[1]) if paired else (0, 0)
            for gs in range(g0, g0 + ng, 65535):       # (grid.y)
                n = min(65535, g0 + ng - gs)
                rc = L.s2s_stain_quant_u8(pa, pitch_a, pitch_a * (r1 - r0), pb, pitch_b, pitch_b * (r1 - r0),
                                          int(paired), 1, r0, r1 - r0, H, W, cell_h, cell_w, gs, n, table, unmix,
                                          white, black, stain, part.data_ptr(), ops._stream())
                _native.check(rc, what)
        res = _finalize(part, Gy * Gx, nchunk, paired, dev)
    stats_of.last_stats = {"bands": len(bands), "band_rows": buf_rows,
                           "band_bytes": sum(s.band_bytes for s in src)}
    return res, (Gy, Gx)


def region_stain_map(region_u8: torch.Tensor, *, cell: int = 256, band_rows: Optional[int] = None, stain: int = 1,
                     stains="hdab", thresholds: Sequence[float] = DEFAULT_THRESHOLDS, white: int = 220,
                     black: int = 0) -> Dict[str, torch.Tensor]:
    """The burden heat map of a whole uint8 ``[H, W, 3]`` region: per ``cell`` x ``cell`` cell the ``"tissue"`` count,
    the ``"positive"`` count of stain ``stain`` (int64 ``[Gy, Gx]``), its ``"burden"`` and ``"mean_od"`` (fp32
    ``[Gy, Gx]``), Gy = ceil(H / cell), Gx = ceil(W / cell); ragged edge cells count only their own pixels.

    The region may live on the GPU or on the host and have any row pitch.  A host image is staged through one pinned
    buffer and one GPU band buffer of ``band_rows`` rows (``plan_stain_bands``; ``None``: a GPU image in one launch, a
    host image in bands of 512 rows), so GPU memory does not grow with H beyond the partial sums.  A chunk's partial
    index depends on the region alone: the result is bit-equal for every ``band_rows`` and for host and GPU input.
    ``region_stain_map.last_stats``: bands, band_rows, band_bytes of the last call.  Other arguments as
    ``stain_quantify``."""
    H, W, _ = check_region(region_u8, "region_stain_map")
    cell, stain = _check_cell(cell), _stain_index(stain)
    table, unmix = _kernel_args(stains, thresholds)
    white, black = _check_thresholds(white, black)
    (counts, sums, out), grid = _reduce_region([region_u8], H, W, min(cell, H), min(cell, W), band_rows, table, unmix,
                                               white, black, 0, "region_stain_map", region_stain_map)
    return {"tissue": counts[:, 0].reshape(grid), "positive": counts[:, 1 + stain].reshape(grid),
            "burden": out[:, stain].reshape(grid), "mean_od": out[:, 3 + stain].reshape(grid)}


region_stain_map.last_stats: Optional[Dict[str, int]] = None


def region_stain_agreement(pred_u8: torch.Tensor, target_u8: torch.Tensor, *, cell: Optional[int] = None,
                           band_rows: Optional[int] = None, stain: int = 1, stains="hdab",
                           thresholds: Sequence[float] = DEFAULT_THRESHOLDS, white: int = 220,
                           black: int = 0) -> Dict[str, torch.Tensor]:
    """``stain_agreement`` over a whole uint8 ``[H, W, 3]`` region pair (each on the GPU or the host, any row pitch):
    fp32 device scalars, or ``[Gy, Gx]`` grids per ``cell`` x ``cell`` cell when ``cell`` is given.  Banding and its
    bit equality as ``region_stain_map``."""
    _check_pair(pred_u8, target_u8, "region_stain_agreement")
    H, W, _ = check_region(pred_u8, "region_stain_agreement")
    check_region(target_u8, "region_stain_agreement")
    stain = _stain_index(stain)
    ch, cw = (H, W) if cell is None else (min(_check_cell(cell), H), min(_check_cell(cell), W))
    table, unmix = _kernel_args(stains, thresholds)
    white, black = _check_thresholds(white, black)
    (_, _, out), grid = _reduce_region([pred_u8, target_u8], H, W, ch, cw, band_rows, table, unmix, white, black,
                                       stain, "region_stain_agreement", region_stain_agreement)
    return _pair_dict(out, () if cell is None else grid)


region_stain_agreement.last_stats: Optional[Dict[str, int]] = None


def agreement_values(pred: torch.Tensor, target: torch.Tensor, stain_args: dict) -> Dict[str, torch.Tensor]:
    """What ``stain=`` adds to ``generation_quality`` / ``evaluate_generation``: ``{"stain/burden_abs_err", "stain/dice",
    "stain/iou"}`` of ``stain_agreement(pred, target, **stain_args)``."""
    if not isinstance(stain_args, dict):
        raise TypeError(f"stain must be None or a dict of stain_agreement's arguments, got {type(stain_args).__name__}")
    v = stain_agreement(pred, target, **stain_args)
    return {"stain/burden_abs_err": v["burden_abs_err"], "stain/dice": v["dice"], "stain/iou": v["iou"]}
