"""Rigid region pre-alignment: the rotation and the offset between two whole regions, measured on block-averaged
structure maps and undone by one resampling.

``register_region`` assumes that the two regions agree to within a few pixels; two scans of one section differ by
hundreds of pixels and a degree or two.  This module measures that placement and removes it, so that the local field of
section 3.22 can finish the alignment (``csrc/rigid.hip``):

  overview         F = (sum of the ds x ds block of the structure byte f of 3.21 + ds^2 / 2) // ds^2 over whole blocks, ds a
                   power of two up to 64; for ds in {1, 2, 4} bit-equal to ``structure_map``
  transform        int64 ``[6]`` = (c, s, ty, tx, Cy, Cx): cosine and sine in Q24, the translation in 1/16 pixel, the
                   doubled centre (``Cy = H - 1`` for the centre of an H-row region); clamped to +-2^24, +-2^36, +-2^24
  position         for output pixel (y, x) and a displacement (dy, dx) in 1/16 pixel (0 without a field, else the dense
                   displacement of 3.22 with its clamp), in int64: Uy = 32 y + 2 dy - 16 Cy, Ux = 32 x + 2 dx - 16 Cx,
                   Vy = c Uy - s Ux, Vx = s Uy + c Ux, sy = ((Vy + (Cy << 28) + 2^24) >> 25) + ty, sx alike with Cx, tx
  sampling         ``warp_region``'s: bilinear in 1/16 pixel (iy = sy >> 4, fy = sy & 15, ``fill`` for a tap outside,
                   + 128, >> 8) or nearest ((sy + 8) >> 4)
  search           the overview of the target is rotated by every angle of a list in one launch; one level of the search
                   of 3.21 over the angles as its batch, on crops that no fill pixel enters; the best valid angle wins

In words ``out[p] = tgt[C + R (p + d - C) + t]`` with ``R = [[cos, -sin], [sin, cos]]`` acting on (y, x).  Everything is
integer arithmetic, so results are bit-reproducible and bit-equal for host and GPU input and for every banding.  With
GPU regions nothing here waits for the device.  GPU only.

Out of scope: regions of different shapes (the caller pads them), mirrored sections, scale or shear, a finer second
angle level.  The reference publishes no registration: these functions have no counterpart there.
"""
from __future__ import annotations

import ctypes
import math
import operator
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _native, ops
from ._regionio import DEFAULT_HOST_BAND, BandSink, BandSource, batch_layout, check_region, gpu_device, gpu_rows
from .registration import (DEFAULT_GAIN, _check_radius, _check_search, _level, _q_ints, region_shift_field,
                           structure_weights)
from .warp import _CLEAN_KEYS, _WARP_KEYS, _check_field, _check_fill, _check_max_shift, clean_shift_field

ONE = 1 << 24                # cosine and sine are in Q24
MAX_DOWNSAMPLE = 64          # RD_MAX_DS of csrc/rigid.hip
MAX_SIZE = 1 << 20           # rows and columns of a region the rigid warp takes
MAX_BATCH = 65535            # transforms of one launch
_LIMITS = (ONE, ONE, 1 << 36, 1 << 36, ONE, ONE)


# ---- host arithmetic -------------------------------------------------------------------------------------------------
def rotation_table(angles_deg) -> torch.Tensor:
    """Host int64 ``[A, 2]`` = ``rint(cos * 2^24), rint(sin * 2^24)`` of angles in degrees; multiples of 90 degrees are
    exact."""
    rows = []
    for a in ([angles_deg] if isinstance(angles_deg, (int, float)) else list(angles_deg)):
        a = float(a)
        if a != a or a in (float("inf"), float("-inf")):
            raise ValueError(f"rotation_table: angles must be finite, got {a}")
        q, r = divmod(a, 90.0)
        if r == 0.0:
            rows.append([(ONE, 0), (0, ONE), (-ONE, 0), (0, -ONE)][int(q) % 4])
        else:
            rad = math.radians(a)
            rows.append((int(round(math.cos(rad) * ONE)), int(round(math.sin(rad) * ONE))))    # round(): half to even
    return torch.tensor(rows, dtype=torch.int64).reshape(-1, 2)


def rigid_transform(angle_deg: float, shift=(0, 0), *, shape=None, center=None) -> torch.Tensor:
    """Host int64 ``[6]``: the rotation by ``angle_deg`` about the centre of a region of ``shape`` = (H, W) (or about
    ``center`` = (cy, cx) in pixels) followed by the translation ``shift`` = (dy, dx) in pixels, rounded to 1/16."""
    if (shape is None) == (center is None):
        raise ValueError("rigid_transform: give the region's shape or a center, not both")
    if shape is not None:
        Cy, Cx = operator.index(shape[0]) - 1, operator.index(shape[1]) - 1
    else:
        Cy, Cx = int(round(2.0 * float(center[0]))), int(round(2.0 * float(center[1])))
    c, s = rotation_table([angle_deg])[0].tolist()
    return torch.tensor([c, s, int(round(16.0 * float(shift[0]))), int(round(16.0 * float(shift[1]))), Cy, Cx],
                        dtype=torch.int64)


def _clamped(vals: Sequence[int]) -> Tuple[int, ...]:
    return tuple(min(max(int(v), -lim), lim) for v, lim in zip(vals, _LIMITS))


def _position(T: Sequence[int], y: int, x: int) -> Tuple[int, int]:
    """(sy, sx) in 1/16 pixel of output pixel (y, x) without a field; ``T`` is clamped already."""
    c, s, ty, tx, Cy, Cx = T
    Uy, Ux = 32 * y - 16 * Cy, 32 * x - 16 * Cx
    return (((c * Uy - s * Ux + (Cy << 28) + ONE) >> 25) + ty, ((s * Uy + c * Ux + (Cx << 28) + ONE) >> 25) + tx)


def _band_rows(T: Sequence[int], r0: int, n: int, H: int, W: int, halo: int) -> Tuple[int, int]:
    """The region rows [lo, hi) that output rows [r0, r0 + n) read: the position is affine in the pixel, so its extremes
    lie at the band's four corners; ``halo`` rows more each way.  At least one row, inside the region."""
    iys = [_position(T, y, x)[0] >> 4 for y in (r0, r0 + n - 1) for x in (0, W - 1)]
    lo = min(max(min(iys) - halo, 0), H - 1)
    return lo, min(max(max(iys) + halo + 1, lo + 1), H)


def _inset(tables: Sequence[Sequence[int]], h: int, w: int) -> Optional[int]:
    """The smallest m >= 0 for which the four corners of the crop [m, h - m) x [m, w - m) sample inside the h x w map,
    all four taps, under every transform; ``None`` when there is none."""
    def inside(T, y, x):
        sy, sx = _position(T, y, x)
        return 0 <= sy and sy + 15 <= 16 * (h - 1) and 0 <= sx and sx + 15 <= 16 * (w - 1)

    for m in range(0, (min(h, w) + 1) // 2):
        if all(inside(T, y, x) for T in tables for y in (m, h - 1 - m) for x in (m, w - 1 - m)):
            return m
    return None


def _check_overview_ds(ds) -> int:
    ds = operator.index(ds)
    if ds < 1 or ds > MAX_DOWNSAMPLE or ds & (ds - 1):
        raise ValueError(f"downsample must be a power of two in 1..{MAX_DOWNSAMPLE}, got {ds}")
    return ds


def _check_band_rows(band_rows, what: str) -> Optional[int]:
    if band_rows is None:
        return None
    band_rows = operator.index(band_rows)
    if band_rows < 1:
        raise ValueError(f"{what}: band_rows must be positive, got {band_rows}")
    return band_rows


def _check_transform(transform, what: str) -> Tuple[torch.Tensor, Optional[int]]:
    if not isinstance(transform, torch.Tensor):
        raise TypeError(f"{what}: transform must be a torch.Tensor, got {type(transform).__name__}")
    if transform.dtype != torch.int64:
        raise ValueError(f"{what}: transform must be int64, got {transform.dtype}")
    if transform.dim() not in (1, 2) or transform.shape[-1] != 6 or transform.shape[0] < 1:
        raise ValueError(f"{what}: transform must be int64 [6] or [A, 6], got {list(transform.shape)}")
    A = int(transform.shape[0]) if transform.dim() == 2 else None
    if A is not None and A > MAX_BATCH:
        raise ValueError(f"{what}: at most {MAX_BATCH} transforms go into one launch, got {A}")
    return transform.contiguous(), A


def _upload(host: torch.Tensor, dev) -> torch.Tensor:
    return host.pin_memory().to(dev, non_blocking=True)


# ---- overview maps ---------------------------------------------------------------------------------------------------
def structure_overview(region_u8: torch.Tensor, downsample: int = 16, *, stains="hed", stain: int = 0,
                       gain: float = DEFAULT_GAIN, band_rows: Optional[int] = None) -> torch.Tensor:
    """The structure map of a whole uint8 ``[H, W, 3]`` region, block-averaged by ``downsample`` (a power of two up to
    64): uint8 ``[H // downsample, W // downsample]`` on the device.  For 1, 2 and 4 it is ``structure_map`` bit for bit.

    The region lives on the GPU (any row pitch, crop views) or on the host; a host region is streamed in bands of
    ``band_rows`` rows (rounded down to a multiple of ``downsample``; ``None``: 512) through one pinned buffer.  One
    launch per band, one launch for a GPU region unless ``band_rows`` is given."""
    what = "structure_overview"
    ds = _check_overview_ds(downsample)
    w = structure_weights(stains, stain, gain)
    H, W, _ = check_region(region_u8, what)
    if H < ds or W < ds:
        raise ValueError(f"{what}: the {H} x {W} region is smaller than one {ds} x {ds} block")
    band_rows = _check_band_rows(band_rows, what)
    if band_rows is not None:
        band_rows = max(band_rows // ds, 1) * ds               # whole blocks
    dev = gpu_device(what, region_u8)
    h, wd = H // ds, W // ds
    rows = h * ds
    on_gpu = region_u8.is_cuda
    step = min(band_rows or (rows if on_gpu else DEFAULT_HOST_BAND), rows)
    wi = (ctypes.c_int * 3)(*w.tolist())
    L = ops._L()
    with torch.no_grad():
        out = torch.empty((h, wd), dtype=torch.uint8, device=dev)
        src = BandSource(region_u8, step, dev)
        for r0 in range(0, rows, step):
            n = min(step, rows - r0)
            ptr, pitch = gpu_rows(src.rows(r0, r0 + n))
            rc = L.s2s_structure_overview_u8(ptr, pitch, n, W, _q_ints(), wi, ds, out.data_ptr() + (r0 // ds) * wd,
                                             ops._stream())
            _native.check(rc, what)
    return out


# ---- the rigid warp --------------------------------------------------------------------------------------------------
def rigid_warp(region_u8: torch.Tensor, transform: torch.Tensor, *, field: Optional[torch.Tensor] = None,
               cell: Optional[int] = None, max_shift: int = 64, nearest: Optional[bool] = None, fill: int = 255,
               band_rows: Optional[int] = None) -> torch.Tensor:
    """A uint8 ``[H, W, 3]`` or ``[H, W]`` region resampled through a rigid transform and, with ``field``, the dense
    displacement of ``warp_region`` in the same pass: ``out[p] = region[C + R (p + d - C) + t]``, ``fill`` outside.

    ``transform``: int64 ``[6]`` = (c, s, ty, tx, Cy, Cx) on the host or on the device (``rigid_transform`` builds one);
    the kernel reads it from device memory, so a GPU call never waits.  ``[A, 6]`` gives ``[A, ...]`` results in one
    launch; this form takes GPU regions only and no field.  ``nearest``: ``None`` is nearest for ``[H, W]`` and bilinear
    for ``[H, W, 3]``; ``False`` on ``[H, W]`` blends a byte map.  ``field``: int32 ``[H // cell, W // cell, 2]`` in 1/16
    pixel on the device with its ``cell`` and ``max_shift``, as ``warp_region`` takes them.

    A host region is streamed in bands of ``band_rows`` output rows (``None``: 512); the source rows of a band are the
    extremes of its four corners' positions, one row more each way, and with a field the reach of the rotated
    displacement more.  A device-resident transform is copied to the host first for that: the one wait.  The bytes do
    not depend on ``band_rows`` or on where the region lives."""
    what = "rigid_warp"
    H, W, C = check_region(region_u8, what, mask_ok=True)
    if H > MAX_SIZE or W > MAX_SIZE:
        raise ValueError(f"{what}: a region has at most {MAX_SIZE} rows and columns, got {H} x {W}")
    T, A = _check_transform(transform, what)
    max_shift, fill = _check_max_shift(max_shift, what), _check_fill(fill, what)
    band_rows = _check_band_rows(band_rows, what)
    nearest = (C == 1) if nearest is None else bool(nearest)
    on_gpu = region_u8.is_cuda
    if A is not None and field is not None:
        raise ValueError(f"{what}: a batch of transforms takes no field")
    if A is not None and not on_gpu:
        raise ValueError(f"{what}: a batch of transforms takes a GPU region only")
    Gy = Gx = 0
    if field is not None:
        if cell is None:
            raise ValueError(f"{what}: a field needs its cell")
        cell = operator.index(cell)
        Gy, Gx = _check_field(field, H, W, cell, what)
    tensors = [region_u8] + ([T] if T.is_cuda else []) + ([field] if field is not None else [])
    dev = gpu_device(what, *tensors, mismatch=ValueError)
    L = ops._L()
    rowb = W * C
    with torch.no_grad():
        if field is not None:
            field = field.contiguous()                         # held for the whole call: the kernels read it
        fp = field.data_ptr() if field is not None else 0
        cell_i = cell if field is not None else 0
        if on_gpu:
            Td = T if T.is_cuda else _upload(T, dev)
            out = torch.empty(((A,) if A is not None else ()) + tuple(region_u8.shape), dtype=torch.uint8, device=dev)
            pitch = batch_layout(region_u8[None], what, "the region")[1]
            step = min(band_rows or H, H)
            for r0 in range(0, H, step):
                n = min(step, H - r0)
                rc = L.s2s_rigid_warp_u8(region_u8.data_ptr(), pitch, 0, H, Td.data_ptr(), A or 1, fp, Gy, Gx, cell_i,
                                         max_shift, H, W, C, int(nearest), fill, r0, n, out.data_ptr() + r0 * rowb, rowb,
                                         H * rowb, ops._stream())
                _native.check(rc, what)
            return out
        Th = T.cpu() if T.is_cuda else T                       # the one wait of a host call with a device transform
        Td = T if T.is_cuda else _upload(T, dev)
        vals = _clamped(Th.tolist())
        halo = 1
        if field is not None:                                  # the rotated displacement reaches (|c| + |s|) max_shift
            halo = -(-((abs(vals[0]) + abs(vals[1])) * max_shift) // ONE) + 2
        step = min(band_rows or DEFAULT_HOST_BAND, H)
        bands = [(r0, min(step, H - r0)) for r0 in range(0, H, step)]
        need = [_band_rows(vals, r0, n, H, W, halo) for r0, n in bands]
        src = BandSource(region_u8, max(hi - lo for lo, hi in need), dev)
        sink = BandSink(region_u8.shape, step)
        band = torch.empty((step,) + tuple(region_u8.shape[1:]), dtype=torch.uint8, device=dev)
        for (r0, n), (lo, hi) in zip(bands, need):
            rows = src.rows(lo, hi)
            rc = L.s2s_rigid_warp_u8(rows.data_ptr(), rowb, lo, hi - lo, Td.data_ptr(), 1, fp, Gy, Gx, cell_i, max_shift,
                                     H, W, C, int(nearest), fill, r0, n, band.data_ptr(), rowb, 0, ops._stream())
            _native.check(rc, what)
            sink.put(band, r0, r0 + n)
        return sink.close()[0]


# ---- the search ------------------------------------------------------------------------------------------------------
def _angle_list(max_angle, angle_step, angles, what: str) -> List[float]:
    if angles is not None:
        out = [float(a) for a in angles]
        if not out:
            raise ValueError(f"{what}: angles must not be empty")
    else:
        max_angle, angle_step = float(max_angle), float(angle_step)
        if not max_angle >= 0.0 or not angle_step > 0.0 or max_angle == float("inf"):
            raise ValueError(f"{what}: max_angle must be >= 0 and angle_step > 0, got {max_angle} and {angle_step}")
        n = int(math.floor(max_angle / angle_step + 1e-9))
        out = [k * angle_step for k in range(-n, n + 1)]
    if len(out) > MAX_BATCH:
        raise ValueError(f"{what}: at most {MAX_BATCH} angles, got {len(out)}")
    return out


def register_rigid(src_region_u8: torch.Tensor, tgt_region_u8: torch.Tensor, *, downsample: int = 16,
                   max_angle: float = 5.0, angle_step: float = 0.5, angles=None, radius: int = 32, src_stains="hed",
                   tgt_stains="hdab", stain: int = 0, gain: float = DEFAULT_GAIN) -> Dict[str, torch.Tensor]:
    """The rigid transform that brings the target region onto the source: ``rigid_warp(tgt, result["transform"])`` is the
    target in the source's frame, up to the residual that ``register_region`` measures.

    Two uint8 ``[H, W, 3]`` regions of one shape, each on the GPU or on the host.  Their overviews at ``downsample`` are
    compared on stain ``stain``: the target's is rotated by ``k * angle_step`` for every ``|k * angle_step| <= max_angle``
    (or by the explicit ``angles``, in degrees) in one launch, and one level of the search of ``register_pairs`` with
    ``radius`` overview pixels runs over the angles as its batch, on the crops inset so far that no fill pixel enters a
    window.  Among valid angles the highest score wins, then the smallest ``|angle|``, then the smallest angle.

    Returns device tensors: ``"transform"`` int64 ``[6]`` about the region's centre ``(ds h - 1, ds w - 1)``, the identity
    when no angle is valid; ``"angle_index"`` int32 (-1 then); ``"angle"`` float64 in degrees; ``"shift"`` int32 ``[2]``
    in overview pixels; ``"score"``, ``"margin"`` (of the chosen surface) and ``"angle_margin"`` (the best score minus
    the best among the angles more than one place away in the list, 0 if there is none: a place is one ``angle_step``
    of the default list, so give explicit ``angles`` in ascending order; validity depends on the source's crop alone, so
    the angles are valid or invalid together) float64; ``"scores"`` float64 ``[A]``; ``"shifts"`` int32 ``[A, 2]``;
    ``"valid"`` int32."""
    what = "register_rigid"
    ds, radius = _check_overview_ds(downsample), _check_radius(radius)
    H, W, _ = check_region(src_region_u8, what)
    if check_region(tgt_region_u8, what) != (H, W, 3):
        raise ValueError(f"{what}: the regions differ in shape")
    if H < ds or W < ds:
        raise ValueError(f"{what}: the {H} x {W} regions are smaller than one {ds} x {ds} block")
    angs = _angle_list(max_angle, angle_step, angles, what)
    A = len(angs)
    table = rotation_table(angs).tolist()
    h, w = H // ds, W // ds
    hint = "raise downsample or lower radius / max_angle"
    if h > MAX_SIZE or w > MAX_SIZE:
        raise ValueError(f"{what}: the {h} x {w} overview is too large; {hint}")
    m = _inset([(c, s, 0, 0, h - 1, w - 1) for c, s in table], h, w)
    if m is None:
        raise ValueError(f"{what}: no part of the {h} x {w} overview stays inside under every angle; {hint}")
    try:
        _check_search(h - 2 * m, w - 2 * m, radius, what)
    except ValueError as e:
        raise ValueError(f"{e} (the {h} x {w} overview inset by {m}); {hint}") from None
    dev = gpu_device(what, src_region_u8, tgt_region_u8, mismatch=ValueError)
    order = sorted(range(A), key=lambda k: (abs(angs[k]), angs[k]))
    rank = [0] * A
    for r, k in enumerate(order):
        rank[k] = r
    ints = [v for c, s in table for v in (c, s, 0, 0, h - 1, w - 1)]
    ints += [v for c, s in table + [[ONE, 0]] for v in (c, s)] + rank
    with torch.no_grad():
        a = structure_overview(src_region_u8, ds, stains=src_stains, stain=stain, gain=gain)
        b = structure_overview(tgt_region_u8, ds, stains=tgt_stains, stain=stain, gain=gain)
        up = _upload(torch.tensor(ints, dtype=torch.int64), dev)
        deg = _upload(torch.tensor(angs + [0.0], dtype=torch.float64), dev)
        Tk, cs, rk = up[:6 * A].view(A, 6), up[6 * A:8 * A + 2].view(A + 1, 2), up[8 * A + 2:]
        bk = rigid_warp(b, Tk, nearest=False, fill=0)
        ac = a[m:h - m, m:w - m].expand(A, h - 2 * m, w - 2 * m).contiguous()
        lev = _level(ac, bk[:, m:h - m, m:w - m].contiguous(), radius, None, 1)
        valid, score = lev["valid"] == 1, lev["score"]
        ok = valid.any()
        sc = torch.where(valid, score, float("-inf"))
        best = sc.max()
        k = torch.where(valid & (sc == best), rk, A).argmin()
        k = torch.where(ok, k, A).reshape(1)                    # row A: the identity, zeros
        pad = lambda t: torch.cat([t, torch.zeros((1,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)])   # noqa: E731
        c, s = cs.index_select(0, k)[0].unbind()
        shift = pad(lev["shift"]).index_select(0, k)[0]
        dy, dx = shift.to(torch.int64).unbind()
        ty = (16 * ds * (c * dy - s * dx) + (1 << 23)) >> 24
        tx = (16 * ds * (s * dy + c * dx) + (1 << 23)) >> 24
        centre = torch.zeros((2,), dtype=torch.int64, device=dev)
        transform = torch.cat([torch.stack([c, s, ty, tx]), centre])
        transform[4] += ds * h - 1
        transform[5] += ds * w - 1
        far = valid & ((torch.arange(A, device=dev) - k).abs() > 1)
        other = torch.where(far, score, float("-inf")).max()
        angle_margin = torch.where(far.any() & ok, best - other, 0.0)
    return {"transform": transform, "angle_index": torch.where(ok, k[0], -1).to(torch.int32),
            "angle": deg.index_select(0, k)[0], "shift": shift, "score": pad(score).index_select(0, k)[0],
            "margin": pad(lev["margin"]).index_select(0, k)[0], "angle_margin": angle_margin, "scores": score,
            "shifts": lev["shift"], "valid": ok.to(torch.int32)}


# ---- composition -----------------------------------------------------------------------------------------------------
def align_regions(src_region_u8: torch.Tensor, tgt_region_u8: torch.Tensor, cell: int = 256, *,
                  masks: Sequence[torch.Tensor] = (), rigid: Optional[dict] = None, **kwargs) -> Dict[str, object]:
    """The target region aligned to the source, rigidly and then locally, in ONE resampling of the original target:
    ``register_rigid(**rigid)``, an intermediate ``rigid_warp`` of the target, ``region_shift_field`` of the source
    against it, ``clean_shift_field``, and ``rigid_warp`` of the original target (and, nearest, of every mask of
    ``masks``) through the transform and the cleaned field together.

    ``kwargs`` as ``register_region`` routes them: ``max_shift`` (64), ``min_score``, ``min_margin``, ``max_dev``,
    ``fill`` (255), ``mask_fill`` (0), ``band_rows``; everything else goes to ``register_pairs``.

    Returns ``register_region``'s keys (``"aligned"``, ``"masks"``, ``"field"``, ``"kept"``, ``"stats"``, ``"score"``)
    plus ``"transform"``, ``"angle"``, ``"rigid_score"`` and ``"rigid_valid"`` of the rigid stage.  With GPU regions
    nothing waits for the device; with a host target or mask the transform is read back once."""
    what = "align_regions"
    max_shift = _check_max_shift(kwargs.pop("max_shift", 64), what)
    clean_kw = {k: kwargs.pop(k) for k in _CLEAN_KEYS if k in kwargs}
    warp_kw = {k: kwargs.pop(k) for k in _WARP_KEYS if k in kwargs}
    mask_fill = _check_fill(kwargs.pop("mask_fill", 0), what)
    masks = list(masks)
    H, W, C = check_region(tgt_region_u8, what, mask_ok=True)
    if C != 3:
        raise ValueError(f"{what}: the regions must be [H, W, 3] RGB images, got {list(tgt_region_u8.shape)}")
    for mk in masks:
        if check_region(mk, what, mask_ok=True) != (H, W, 1):
            raise ValueError(f"{what}: a mask must be uint8 [{H}, {W}], got {list(mk.shape)}")
    rg = register_rigid(src_region_u8, tgt_region_u8, **(rigid or {}))
    T = rg["transform"]
    if not all(t.is_cuda for t in [tgt_region_u8] + masks):
        T = T.cpu()                                            # the one wait of a call with a host target or mask
    mid = rigid_warp(tgt_region_u8, T, **warp_kw)
    measured = region_shift_field(src_region_u8, mid, cell, **kwargs)
    cleaned = clean_shift_field(measured, max_shift=max_shift, **clean_kw)
    both = dict(field=cleaned["field"], cell=cell, max_shift=max_shift)
    aligned = rigid_warp(tgt_region_u8, T, **both, **warp_kw)
    warp_kw["fill"] = mask_fill
    moved = [rigid_warp(mk, T, nearest=True, **both, **warp_kw) for mk in masks]
    return {"aligned": aligned, "masks": moved, "field": cleaned["field"], "kept": cleaned["kept"],
            "stats": cleaned["stats"], "score": measured["score"], "transform": rg["transform"], "angle": rg["angle"],
            "rigid_score": rg["score"], "rigid_valid": rg["valid"]}
