"""Macenko stain normalisation (Macenko et al., ISBI 2009) of H&E tiles, batches and whole regions.

H&E slides differ in colour between labs and scanners.  The method estimates the slide's own two stain vectors from
its optical-density (OD) cloud and re-expresses every pixel in a reference basis at a reference intensity.  Everything
that is counted on the device is an exact integer, so a fit is bit-equal run to run, for every banding and for host and
GPU input (``csrc/stain_norm.hip``):

  kept     = black <= max(R, G, B) <= u_beta, u_beta = floor(255 * exp(-beta)): every channel's natural-log OD >= beta
  pass A   n, sum q_c, sum q_c q_d over the kept pixels in int64, q(u) = rint(od(u) * 2^12) from ``od_table``
  host     cov = (S2 / n - S1 S1^T / n^2) / 2^24; the eigenvectors v1, v2 of its two largest eigenvalues (float64),
           sum(v1) > 0, the largest-magnitude component of v2 > 0, rounded to fp32: the ``plane`` [3, 2]
  pass B   x = od . v1, y = od . v2 (fp32, every operation rounded on its own), s = y / (|x| + |y|), the "diamond
           angle", monotone in atan2(y, x) for x > 0; histogram of bin = clamp(floor((s + 1) * NB / 2), 0, NB - 1)
  host     the bins of the ``alpha`` and ``100 - alpha`` percentiles -> s_p = (k + 0.5) * 2 / NB - 1 ->
           normalise(v1 * (1 - |s_p|) + v2 * s_p); haematoxylin (row 0) is the vector with the larger R component
  pass C   c_0, c_1 of ``unmix_matrix(vectors)`` exactly as ``stain_quantify`` computes them; two histograms of
           bin = clamp(floor(c_k * NB / CONC_MAX), 0, NB - 1); max_conc_k = the upper edge of the bin that holds the
           ``conc_percentile`` rank
  apply    c'_k = c_k * (reference max_conc_k / max_conc_k), od' = c'_0 ref_0 + c'_1 ref_1,
           u' = clamp(rint(255 * 10^(-od')), 0, 255); no pixel is gated (glass has OD ~ 0 and stays white)

The rank of percentile p in a histogram of n pixels is max(1, ceil(p / 100 * n)); its bin is the first whose cumulative
count reaches the rank.  A fitted ``StainFit.vectors`` is a ``[2, 3]`` basis that ``stain_quantify``, ``stain_agreement``,
``stain_separate`` and ``region_stain_map`` accept as ``stains=``: the calibration their documentation asks for.

Fitting reads three small results back to the host (it is a per-slide calibration, not a captured step); applying a fit
is one launch that neither allocates after its output, synchronises nor reads back.  GPU only.

The reference publishes no stain normalisation: these functions have no counterpart there.
"""
from __future__ import annotations

import ctypes
import functools
import math
import operator
from dataclasses import dataclass
from typing import Callable, List, Optional, Tuple

import torch

from . import _native, ops
from ._regionio import DEFAULT_HOST_BAND, BandSink, BandSource, batch_layout, check_region, gpu_device, gpu_rows
from .stain_quant import od_table, unmix_matrix

NB = 4096                # histogram bins: SN_NB of csrc/stain_norm.hip
CONC_MAX = 4.0           # the concentration histograms cover [0, CONC_MAX) in log10 OD
MOMENT_BITS = 12         # q(u) = rint(od(u) * 2^MOMENT_BITS)
MIN_PIXELS = 16          # fewer kept pixels than this is no OD cloud to fit
CHUNK_ROWS = 16          # rows of one workgroup's chunk in pass A: SN_CH of csrc/stain_norm.hip
_MAX_BAND = CHUNK_ROWS * 65535     # (grid.y)
_DEGENERATE = 1e-12      # a second eigenvalue below this share of the first is rounding noise of a one-stain cloud


@dataclass(frozen=True)
class StainFit:
    """The stains of one slide.  ``vectors``: float64 ``[2, 3]`` unit OD vectors, haematoxylin first; ``max_conc``:
    float64 ``[2]``, the ``conc_percentile`` concentration of each stain in log10 OD; ``plane``: the fp32 ``[3, 2]``
    eigenvector pair pass B projected on (``None`` for constants that were not fitted here); ``pixels``: the pixels kept
    for the fit.  All on the host."""
    vectors: torch.Tensor
    max_conc: torch.Tensor
    plane: Optional[torch.Tensor]
    pixels: int
    alpha: float
    beta: float
    conc_percentile: float


# the constants distributed with Macenko's method; its maximum concentrations are in natural-log OD
REFERENCE_HE = StainFit(vectors=torch.tensor([[0.5626, 0.7201, 0.4062], [0.2159, 0.8012, 0.5581]], dtype=torch.float64),
                        max_conc=torch.tensor([1.9705 / math.log(10.0), 1.0308 / math.log(10.0)], dtype=torch.float64),
                        plane=None, pixels=0, alpha=1.0, beta=0.15, conc_percentile=99.0)


# ---- host arithmetic -------------------------------------------------------------------------------------------------
def u_beta(beta: float) -> int:
    """The largest byte whose natural-log OD is at least ``beta``: floor(255 * exp(-beta)); 219 for 0.15."""
    beta = float(beta)
    if not math.isfinite(beta) or beta < 0.0:
        raise ValueError(f"beta must be a finite non-negative number, got {beta}")
    return int(math.floor(255.0 * math.exp(-beta)))


def q_table() -> torch.Tensor:
    """int32 ``[256]``: rint(od(u) * 2^12), taken in double from the fp32 ``od_table``."""
    return torch.round(od_table().to(torch.float64) * float(1 << MOMENT_BITS)).to(torch.int32)


def _percent(p, what: str, lo_open: float, hi: float, hi_open: bool) -> float:
    p = float(p)
    if not math.isfinite(p) or p <= lo_open or p > hi or (hi_open and p == hi):
        raise ValueError(f"{what} must lie in ({lo_open}, {hi}{')' if hi_open else ']'}, got {p}")
    return p


def rank_bin(hist, p: float) -> int:
    """The first bin of ``hist`` whose cumulative count reaches max(1, ceil(p / 100 * total))."""
    counts = [int(v) for v in torch.as_tensor(hist).reshape(-1).tolist()]
    total = sum(counts)
    if total < 1:
        raise ValueError("an empty histogram has no percentile")
    rank = max(1, math.ceil(p / 100.0 * total))
    run = 0
    for k, c in enumerate(counts):
        run += c
        if run >= rank:
            return k
    return len(counts) - 1


def plane_from_moments(moments) -> torch.Tensor:
    """The fp32 ``[3, 2]`` plane (columns v1, v2) of the ten int64 moments of pass A.  ``ValueError`` when fewer than 16
    pixels were kept or the cloud does not span a plane (a blank or single-colour image)."""
    m = [int(v) for v in torch.as_tensor(moments).reshape(-1).tolist()]
    if len(m) != 10:
        raise ValueError(f"expected ten moments, got {len(m)}")
    n, s1, s2 = m[0], m[1:4], m[4:]
    if n < MIN_PIXELS:
        raise ValueError(f"only {n} pixels pass the OD cut-off: at least {MIN_PIXELS} are needed to fit the stains")
    idx = {(0, 0): 0, (0, 1): 1, (0, 2): 2, (1, 1): 3, (1, 2): 4, (2, 2): 5}
    scale = float(1 << (2 * MOMENT_BITS))
    cov = [[(s2[idx[(min(c, d), max(c, d))]] / n - (s1[c] * s1[d]) / (n * n)) / scale for d in range(3)]
           for c in range(3)]
    w, v = torch.linalg.eigh(torch.tensor(cov, dtype=torch.float64))          # ascending
    if not float(w[1]) > _DEGENERATE * max(float(w[2]), 0.0) or not float(w[1]) > 0.0:
        raise ValueError("the optical densities of the kept pixels do not span a plane (a single-colour image?)")
    v1, v2 = v[:, 2].clone(), v[:, 1].clone()
    if float(v1.sum()) < 0.0:
        v1 = -v1
    if float(v2[int(v2.abs().argmax())]) < 0.0:
        v2 = -v2
    return torch.stack([v1, v2], dim=1).to(torch.float32)


def vectors_from_histogram(hist, plane: torch.Tensor, alpha: float = 1.0) -> torch.Tensor:
    """float64 ``[2, 3]``: the stain vectors at the ``alpha`` and ``100 - alpha`` percentiles of the angle histogram of
    pass B, haematoxylin (the larger R component) first."""
    alpha = _percent(alpha, "alpha", 0.0, 50.0, True)
    pl = torch.as_tensor(plane).to(torch.float64)
    v1, v2 = pl[:, 0], pl[:, 1]
    vecs = []
    for p in (alpha, 100.0 - alpha):
        s = (rank_bin(hist, p) + 0.5) * 2.0 / NB - 1.0
        v = v1 * (1.0 - abs(s)) + v2 * s
        vecs.append(v / v.norm())
    if float(vecs[0][0]) < float(vecs[1][0]):
        vecs.reverse()
    return torch.stack(vecs)


def max_conc_from_histograms(hists, conc_percentile: float = 99.0) -> torch.Tensor:
    """float64 ``[2]``: the upper edge of the bin that holds the ``conc_percentile`` rank of each histogram of pass C."""
    pct = _percent(conc_percentile, "conc_percentile", 0.0, 100.0, False)
    hists = torch.as_tensor(hists)
    return torch.tensor([(rank_bin(hists[k], pct) + 1) * CONC_MAX / NB for k in range(2)], dtype=torch.float64)


# ---- the device passes -----------------------------------------------------------------------------------------------
def _check_image(img, what: str) -> Tuple[int, int, int]:
    """(B, H, W) of a uint8 [H, W, 3] image (GPU or host) or a [B, H, W, 3] GPU batch."""
    if not isinstance(img, torch.Tensor):
        raise TypeError(f"{what}: the image must be a torch.Tensor, got {type(img).__name__}")
    if img.dim() == 3:
        return (1,) + check_region(img, what)[:2]
    if img.dtype != torch.uint8 or img.dim() != 4 or img.shape[3] != 3 or min(img.shape[:3]) < 1:
        raise ValueError(f"{what}: expected a non-empty uint8 [H, W, 3] or [B, H, W, 3] image, got {img.dtype} "
                         f"{list(img.shape)}")
    if not img.is_cuda:
        raise RuntimeError(f"stain2stain_amd: {what} needs a batch on the GPU (a host image is one [H, W, 3] region)")
    return tuple(int(v) for v in img.shape[:3])


def _bands(H: int, band_rows: Optional[int], on_gpu: bool) -> List[Tuple[int, int]]:
    """[r0, r1) row ranges: whole chunk rows of pass A, at most ``band_rows`` rows each."""
    if band_rows is None:
        band_rows = _MAX_BAND if on_gpu else DEFAULT_HOST_BAND
    band_rows = operator.index(band_rows)
    if band_rows < CHUNK_ROWS:
        raise ValueError(f"band_rows must be at least {CHUNK_ROWS}, got {band_rows}")
    step = min(band_rows // CHUNK_ROWS * CHUNK_ROWS, _MAX_BAND)
    return [(r0, min(r0 + step, H)) for r0 in range(0, H, step)]


def _each_band(img: torch.Tensor, band_rows, what: str, launch: Callable) -> None:
    """``launch(ptr, pitch, img_stride, B, r0, rows, H, W, first)`` for every band of ``img``, in order."""
    B, H, W = _check_image(img, what)
    if img.dim() == 4:
        t, pitch, stride = batch_layout(img, what, copy=True)
        if H > _MAX_BAND:
            raise ValueError(f"{what}: a batch image has at most {_MAX_BAND} rows")
        _native.check(launch(t.data_ptr(), pitch, stride, B, 0, H, H, W, True), what)
        return
    bands = _bands(H, band_rows, img.is_cuda)
    src = BandSource(img, max(r1 - r0 for r0, r1 in bands), gpu_device(what, img))
    for i, (r0, r1) in enumerate(bands):
        ptr, pitch = gpu_rows(src.rows(r0, r1))
        _native.check(launch(ptr, pitch, pitch * (r1 - r0), 1, r0, r1 - r0, H, W, i == 0), what)


def _c_floats(values) -> ctypes.Array:
    values = [float(v) for v in values]
    return (ctypes.c_float * len(values))(*values)


@functools.lru_cache(maxsize=None)
def _od_floats() -> ctypes.Array:
    """``od_table`` as the host array of the C ABI (read-only; built once)."""
    return _c_floats(od_table().tolist())


def moments(img_u8: torch.Tensor, *, beta: float = 0.15, black: int = 0,
            band_rows: Optional[int] = None) -> torch.Tensor:
    """Pass A: int64 ``[10]`` on the device: n, sum q_r q_g q_b, sum q_r q_r, q_r q_g, q_r q_b, q_g q_g, q_g q_b, q_b q_b
    over the kept pixels of a uint8 ``[H, W, 3]`` image (GPU or host) or a ``[B, H, W, 3]`` GPU batch (pooled)."""
    B, H, W = _check_image(img_u8, "stain moments")
    ub, black = u_beta(beta), _check_black(black)
    dev = gpu_device("stain moments", img_u8)
    L = ops._L()
    slots = L.s2s_stain_moments_slots(B, H, W)
    _native.check(slots if slots < 0 else 0, "stain_moments_slots")
    qt = (ctypes.c_int * 256)(*q_table().tolist())
    with torch.no_grad():
        part = ops._workspace(dev, 2 * 10 * slots, "stain_norm").view(torch.int64)
        out = torch.empty((10,), dtype=torch.int64, device=dev)
        _each_band(img_u8, band_rows, "stain moments",
                   lambda ptr, pitch, stride, b, r0, rows, h, w, first: L.s2s_stain_moments_u8(
                       ptr, pitch, stride, b, r0, rows, h, w, qt, ub, black, part.data_ptr(), ops._stream()))
        _native.check(L.s2s_stain_moments_finalize(part.data_ptr(), slots, out.data_ptr(), ops._stream()),
                      "stain_moments_finalize")
    return out


def angle_histogram(img_u8: torch.Tensor, plane: torch.Tensor, *, beta: float = 0.15, black: int = 0,
                    band_rows: Optional[int] = None) -> torch.Tensor:
    """Pass B: int64 ``[NB]`` on the device, the histogram of the kept pixels' diamond angle in the fp32 ``[3, 2]``
    ``plane``; pixels that project onto the origin are not counted."""
    _check_image(img_u8, "stain angle histogram")
    plane = torch.as_tensor(plane).detach().to("cpu", torch.float32)
    if tuple(plane.shape) != (3, 2) or not torch.isfinite(plane).all():
        raise ValueError(f"plane must be a finite [3, 2] array, got {list(plane.shape)}")
    ub, black = u_beta(beta), _check_black(black)
    dev = gpu_device("stain angle histogram", img_u8)
    L = ops._L()
    table, coef = _od_floats(), _c_floats(plane.reshape(-1).tolist())
    with torch.no_grad():
        hist = torch.empty((NB,), dtype=torch.int64, device=dev)
        _each_band(img_u8, band_rows, "stain angle histogram",
                   lambda ptr, pitch, stride, b, r0, rows, h, w, first: L.s2s_stain_angle_hist_u8(
                       ptr, pitch, stride, b, r0, rows, h, w, table, coef, ub, black, int(first), hist.data_ptr(),
                       ops._stream()))
    return hist


def concentration_histogram(img_u8: torch.Tensor, vectors, *, beta: float = 0.15, black: int = 0,
                            band_rows: Optional[int] = None) -> torch.Tensor:
    """Pass C: int64 ``[2, NB]`` on the device, the histograms of the kept pixels' two stain concentrations under
    ``unmix_matrix(vectors)``; bin width ``CONC_MAX / NB``, both ends clamped."""
    _check_image(img_u8, "stain concentration histogram")
    ub, black = u_beta(beta), _check_black(black)
    table, coef = _od_floats(), _c_floats(unmix_matrix(vectors).reshape(-1).tolist())
    dev = gpu_device("stain concentration histogram", img_u8)
    L = ops._L()
    with torch.no_grad():
        hist = torch.empty((2, NB), dtype=torch.int64, device=dev)
        _each_band(img_u8, band_rows, "stain concentration histogram",
                   lambda ptr, pitch, stride, b, r0, rows, h, w, first: L.s2s_stain_conc_hist_u8(
                       ptr, pitch, stride, b, r0, rows, h, w, table, coef, ub, black, int(first), hist.data_ptr(),
                       ops._stream()))
    return hist


def _check_black(black) -> int:
    black = operator.index(black)
    if not 0 <= black <= 255:
        raise ValueError(f"black must lie in 0..255, got {black}")
    return black


def fit_stains(img_u8: torch.Tensor, *, alpha: float = 1.0, beta: float = 0.15, conc_percentile: float = 99.0,
               black: int = 0, band_rows: Optional[int] = None) -> StainFit:
    """Fit the two stain vectors and their maximum concentrations to a uint8 ``[H, W, 3]`` H&E image (on the GPU or on
    the host, any row pitch) or a ``[B, H, W, 3]`` GPU batch, which is pooled into one fit.

    ``alpha``: the percentile of the angle distribution the vectors are read at (and ``100 - alpha``); ``beta``:
    Macenko's natural-log OD cut-off, a pixel is kept iff every channel's OD reaches it; ``conc_percentile``: the
    percentile of each stain's concentration that ``max_conc`` reports; ``black``: pixels whose brightest channel is
    below it are specks, not tissue.  A host region is streamed through pinned bands of ``band_rows`` rows (a multiple
    of 16 is used; ``None``: 512), once per pass; the result does not depend on it.  Raises ``ValueError`` when fewer
    than 16 pixels are kept or their optical densities do not span a plane (a blank or single-colour image).
    Three passes over the bytes and three small read-backs; synchronises with the device."""
    _check_image(img_u8, "fit_stains")
    alpha = _percent(alpha, "alpha", 0.0, 50.0, True)
    conc_percentile = _percent(conc_percentile, "conc_percentile", 0.0, 100.0, False)
    u_beta(beta), _check_black(black)
    kw = {"beta": beta, "black": black, "band_rows": band_rows}
    m = moments(img_u8, **kw).cpu()
    plane = plane_from_moments(m)
    hist = angle_histogram(img_u8, plane, **kw).cpu()
    if int(hist.sum()) < 1:
        raise ValueError("no kept pixel has a direction in the stain plane")
    vectors = vectors_from_histogram(hist, plane, alpha)
    conc = concentration_histogram(img_u8, vectors, **kw).cpu()
    return StainFit(vectors=vectors, max_conc=max_conc_from_histograms(conc, conc_percentile), plane=plane,
                    pixels=int(m[0]), alpha=alpha, beta=float(beta), conc_percentile=conc_percentile)


def _apply_args(fit: StainFit, reference: StainFit):
    for name, f in (("fit", fit), ("reference", reference)):
        if not isinstance(f, StainFit):
            raise TypeError(f"{name} must be a StainFit, got {type(f).__name__}")
    mc, rc = (torch.as_tensor(f.max_conc, dtype=torch.float64).reshape(-1) for f in (fit, reference))
    ref = torch.as_tensor(reference.vectors, dtype=torch.float64)
    if mc.numel() != 2 or rc.numel() != 2 or tuple(ref.shape) != (2, 3):
        raise ValueError("a StainFit holds [2, 3] vectors and two maximum concentrations")
    if not (torch.isfinite(mc).all() and torch.isfinite(rc).all() and torch.isfinite(ref).all() and (mc > 0).all()
            and (rc > 0).all()):
        raise ValueError("maximum concentrations must be finite and positive, reference vectors finite")
    scale = (rc / mc).to(torch.float32)
    coef = unmix_matrix(fit.vectors).reshape(-1).tolist() + scale.tolist() + ref.to(torch.float32).reshape(-1).tolist()
    return _od_floats(), _c_floats(coef)


def stain_normalize(tiles_u8: torch.Tensor, fit: Optional[StainFit] = None, *, reference: StainFit = REFERENCE_HE,
                    network_input: bool = False) -> torch.Tensor:
    """A uint8 ``[B, H, W, 3]`` GPU batch (crop views and any row pitch allowed) with its stains re-expressed in
    ``reference``'s basis and intensity.  ``fit``: the batch's own stains (``fit_stains``; ``None``: fitted on the batch
    itself, which synchronises).  Returns uint8 ``[B, H, W, 3]``, or with ``network_input=True`` fp32 ``[B, 3, H, W]``
    equal to ``(u8 / 255 - 0.5) / 0.5`` of those bytes: normalisation, ``to_tensor`` and ``Normalize(0.5, 0.5)`` in one
    pass.  One launch on the current stream; with a given ``fit`` nothing waits for the device."""
    if not isinstance(tiles_u8, torch.Tensor):
        raise TypeError(f"stain_normalize: tiles must be a torch.Tensor, got {type(tiles_u8).__name__}")
    if tiles_u8.dim() != 4:
        raise ValueError(f"stain_normalize: tiles must be uint8 [B, H, W, 3], got {list(tiles_u8.shape)}")
    B, H, W = _check_image(tiles_u8, "stain_normalize")
    if fit is None:
        fit = fit_stains(tiles_u8)
    table, coef = _apply_args(fit, reference)
    with torch.no_grad():
        t, pitch, stride = batch_layout(tiles_u8, "stain_normalize", copy=True)
        if network_input:
            out = torch.empty((B, 3, H, W), dtype=torch.float32, device=t.device)
        else:
            out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=t.device)
        rc = ops._L().s2s_stain_normalize_u8(t.data_ptr(), pitch, stride, B, H, W, table, coef, out.data_ptr(), 3 * W,
                                             3 * W * H, int(network_input), ops._stream())
        _native.check(rc, "stain_normalize")
    return out


def normalize_region(region_u8: torch.Tensor, fit: Optional[StainFit] = None, *, reference: StainFit = REFERENCE_HE,
                     band_rows: Optional[int] = None) -> torch.Tensor:
    """``stain_normalize`` of a whole uint8 ``[H, W, 3]`` region (any row pitch): uint8 ``[H, W, 3]`` on the input's
    device.  A GPU region is one launch.  A host region is staged in and out through pinned bands of ``band_rows`` rows
    (``None``: 512), so GPU memory does not grow with H; the bytes do not depend on the banding.  ``fit=None`` fits on
    the region itself first."""
    H, W, _ = check_region(region_u8, "normalize_region")
    if fit is None:
        fit = fit_stains(region_u8, band_rows=band_rows)
    table, coef = _apply_args(fit, reference)
    bands = _bands(H, band_rows, region_u8.is_cuda)
    dev = gpu_device("normalize_region", region_u8)
    L = ops._L()
    with torch.no_grad():
        if region_u8.is_cuda:
            out = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
            ptr, pitch = gpu_rows(region_u8)
            _native.check(L.s2s_stain_normalize_u8(ptr, pitch, pitch * H, 1, H, W, table, coef, out.data_ptr(), 3 * W,
                                                   3 * W * H, 0, ops._stream()), "normalize_region")
            return out
        rows = max(r1 - r0 for r0, r1 in bands)
        src, sink = BandSource(region_u8, rows, dev), BandSink((H, W, 3), rows)
        band = torch.empty((rows, W, 3), dtype=torch.uint8, device=dev)
        for r0, r1 in bands:
            n = r1 - r0
            ptr, pitch = gpu_rows(src.rows(r0, r1))
            _native.check(L.s2s_stain_normalize_u8(ptr, pitch, pitch * n, 1, n, W, table, coef, band.data_ptr(), 3 * W,
                                                   3 * W * n, 0, ops._stream()), "normalize_region")
            sink.put(band, r0, r1)
        return sink.close()[0]
