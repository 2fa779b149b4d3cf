"""Paired tile registration: the integer shift between a source tile and its target, and what to do with it.

The flow-matching loss, ``paired_augment``'s shared crop and the pixel-wise metrics all assume that source pixel (y, x)
and target pixel (y, x) are the same piece of tissue.  A destain / restain pair is the same section scanned twice, so
what is left between the two tiles is a small rigid offset that varies over the slide.  This module measures it,
rejects pairs that do not match and hands aligned tiles on (``csrc/registration.hip``):

  structure byte   q(u) = rint(od(u) * 2^12) (``q_table`` of 3.18); w[ch] = rint(m[ch][k] * gain * 16), m the float64
                   unmixing matrix of the tile's basis, k the stain (0: haematoxylin, which both stains contain);
                   acc = w_r q[R] + w_g q[G] + w_b q[B] in int32; f = clamp((acc + 2^15) >> 16, 0, 255); with
                   ``downsample`` ds in {1, 2, 4}: F = (sum of the ds x ds block of f + ds^2 / 2) / ds^2, whole blocks only
  search           maps a, b of [B, h, w], radius R <= 32, a per-sample centre (cy, cx) on the device; margins
                   my = R + |cy|, mx = R + |cx|; the template a[my : h - my, mx : w - mx] of n pixels against the windows
                   b[my + dy : h - my + dy, mx + dx : w - mx + dx] for (dy, dx) in centre + [-R, R]^2; the sums
                   n, sum a, sum a^2 (``tsum``) and sum b, sum b^2, sum a b (``sums``) in int64
  score            va = n sum a^2 - (sum a)^2, vb alike, num = n sum a b - sum a sum b, exact in int64;
                   score = double(num) / sqrt(double(va) * double(vb)), 0 when va or vb is 0 (ZNCC)
  pick             highest score, then smallest (dy - cy)^2 + (dx - cx)^2, then smallest dy, then smallest dx

``shift = (dy, dx)`` means that ``tgt[y + dy, x + dx]`` is the tissue at ``src[y, x]``.  Everything counted is an integer,
so the result is bit-reproducible for every launch geometry.  Unless a function says otherwise nothing here waits for
the device.  GPU only.

The reference publishes no registration: these functions have no counterpart there.
"""
from __future__ import annotations

import ctypes
import functools
import operator
import random
from typing import Dict, Optional

import torch

from . import _native, ops
from ._regionio import BandSource, batch_layout, check_region, gpu_device, gpu_rows
from .image_metrics import image_quality
from .stain_norm import q_table
from .stain_quant import _det, _stain_index, stain_matrix

MAX_RADIUS = 32              # RG_MAX_R of csrc/registration.hip
MAX_TEMPLATE = 1 << 18       # template pixels at the centre 0: n * sum(a b) stays below 2^53
DEFAULT_GAIN = 100.0         # structure levels per unit of stain concentration


# ---- host arithmetic -------------------------------------------------------------------------------------------------
def structure_weights(stains="hed", stain: int = 0, gain: float = DEFAULT_GAIN) -> torch.Tensor:
    """Host int32 ``[3]``: ``rint(m[ch][stain] * gain * 16)`` with ``m`` the inverse of ``stain_matrix(stains)`` in
    float64 (the adjugate over the determinant).  ``stains`` as ``stain_matrix`` takes it: a name or a ``[2, 3]`` /
    ``[3, 3]`` array (a ``StainFit.vectors`` is one)."""
    stain = _stain_index(stain)
    gain = float(gain)
    if not gain > 0.0 or gain != gain or gain == float("inf"):
        raise ValueError(f"gain must be a finite positive number, got {gain}")
    M = stain_matrix(stains).tolist()
    d = _det(M)
    col = [(M[(stain + 1) % 3][(i + 1) % 3] * M[(stain + 2) % 3][(i + 2) % 3]
            - M[(stain + 1) % 3][(i + 2) % 3] * M[(stain + 2) % 3][(i + 1) % 3]) / d for i in range(3)]
    w = [int(round(v * gain * 16.0)) for v in col]            # round(): half to even, as rint
    if (1 << 15) + int(q_table().max()) * sum(abs(v) for v in w) > (1 << 31) - 1:
        raise ValueError(f"gain {gain} is too large for this basis: the int32 accumulator would overflow")
    return torch.tensor(w, dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def _q_ints() -> ctypes.Array:
    return (ctypes.c_int * 256)(*q_table().tolist())


def _check_downsample(ds) -> int:
    ds = operator.index(ds)
    if ds not in (1, 2, 4):
        raise ValueError(f"downsample must be 1, 2 or 4, got {ds}")
    return ds


def _check_radius(radius) -> int:
    radius = operator.index(radius)
    if radius < 0:
        raise ValueError(f"radius must not be negative, got {radius}")
    return radius


def _u8_layout(t, name: str, what: str, channels: Optional[int] = 3):
    """(B, H, W, row pitch, sample stride) of a uint8 ``[B, H, W, 3]`` (``channels=None``: ``[B, H, W]``) GPU batch
    whose pixels are contiguous within a row.  Rows may be padded and samples may interleave (cells of a region)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(t).__name__}")
    shape = "[B, H, W, 3]" if channels else "[B, H, W]"
    if t.dtype != torch.uint8:
        raise ValueError(f"{what}: {name} must be uint8 {shape}, got {t.dtype}")
    if t.dim() != (4 if channels else 3) or (channels and t.shape[3] != channels) or min(t.shape) < 1:
        raise ValueError(f"{what}: {name} must be a non-empty uint8 {shape}, got {list(t.shape)}")
    _, pitch, img = batch_layout(t, what, name, interleave=True)
    if not t.is_cuda:
        raise ValueError(f"{what}: {name} must be on the GPU (there is no CPU path)")
    return (*(int(v) for v in t.shape[:3]), pitch, img)


def _as_u8(t, name: str, what: str) -> torch.Tensor:
    """uint8 ``[B, H, W, 3]`` as it is; fp32 ``[B, 3, H, W]`` in the network's range through the save conversion
    ``trunc(clamp((x * 0.5 + 0.5) * 255, 0, 255))`` of 3.17, in torch."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(t).__name__}")
    if t.dtype == torch.float32:
        if t.dim() != 4 or t.shape[1] != 3 or min(t.shape) < 1:
            raise ValueError(f"{what}: fp32 {name} must be a non-empty [B, 3, H, W], got {list(t.shape)}")
        if not t.is_cuda:
            raise ValueError(f"{what}: {name} must be on the GPU (there is no CPU path)")
        with torch.no_grad():
            u = ((t.detach() * 0.5 + 0.5) * 255.0).clamp(0.0, 255.0).to(torch.uint8)
            return u.permute(0, 2, 3, 1).contiguous()
    return t


def _check_center(center, B: int, dev, what: str) -> Optional[torch.Tensor]:
    if center is None:
        return None
    if not isinstance(center, torch.Tensor):
        raise TypeError(f"{what}: center must be a torch.Tensor, got {type(center).__name__}")
    if center.dtype != torch.int32 or tuple(center.shape) != (B, 2):
        raise ValueError(f"{what}: center must be int32 [{B}, 2], got {center.dtype} {list(center.shape)}")
    if center.device != dev:
        raise ValueError(f"{what}: center must be on the images' device")
    return center.contiguous()


# ---- the device calls ------------------------------------------------------------------------------------------------
def _structure(t: torch.Tensor, B: int, H: int, W: int, pitch: int, img: int, w: torch.Tensor, ds: int) -> torch.Tensor:
    out = torch.empty((B, H // ds, W // ds), dtype=torch.uint8, device=t.device)
    wi = (ctypes.c_int * 3)(*w.tolist())
    rc = ops._L().s2s_structure_map_u8(t.data_ptr(), pitch, img, B, H, W, _q_ints(), wi, ds, out.data_ptr(),
                                       ops._stream())
    _native.check(rc, "structure_map")
    return out


def structure_map(tiles_u8: torch.Tensor, stains="hed", stain: int = 0, downsample: int = 1,
                  gain: float = DEFAULT_GAIN) -> torch.Tensor:
    """The structure bytes of a uint8 ``[B, H, W, 3]`` GPU batch (crop views and any row pitch allowed) or an fp32
    ``[B, 3, H, W]`` batch in the network's range: uint8 ``[B, H // downsample, W // downsample]``.  One launch."""
    what = "structure_map"
    ds = _check_downsample(downsample)
    w = structure_weights(stains, stain, gain)
    t = _as_u8(tiles_u8, "tiles_u8", what)
    B, H, W, pitch, img = _u8_layout(t, "tiles_u8", what)
    if H < ds or W < ds:
        raise ValueError(f"{what}: the {H} x {W} images are smaller than one {ds} x {ds} block")
    with torch.no_grad():
        return _structure(t, B, H, W, pitch, img, w, ds)


def _check_search(h: int, w: int, R: int, what: str) -> None:
    if R > MAX_RADIUS:
        raise ValueError(f"{what}: the search radius at one level is at most {MAX_RADIUS}, got {R}")
    if h <= 2 * R or w <= 2 * R:
        raise ValueError(f"{what}: {h} x {w} structure maps are too small for radius {R}")
    if (h - 2 * R) * (w - 2 * R) > MAX_TEMPLATE:
        raise ValueError(f"{what}: the template of {h - 2 * R} x {w - 2 * R} pixels exceeds {MAX_TEMPLATE}")


def _level(a: torch.Tensor, b: torch.Tensor, R: int, center: Optional[torch.Tensor], ds: int) -> Dict[str, torch.Tensor]:
    """One search level over structure maps: the sums launch and the pick launch."""
    B, h, w = (int(v) for v in a.shape)
    S = 2 * R + 1
    dev = a.device
    tsum = torch.empty((B, 3), dtype=torch.int64, device=dev)
    sums = torch.empty((B, S, S, 3), dtype=torch.int64, device=dev)
    shift = torch.empty((B, 2), dtype=torch.int32, device=dev)
    score = torch.empty((B, 3), dtype=torch.float64, device=dev)
    valid = torch.empty((B,), dtype=torch.int32, device=dev)
    c_ptr = 0 if center is None else center.data_ptr()
    L = ops._L()
    _native.check(L.s2s_register_sums(a.data_ptr(), b.data_ptr(), B, h, w, R, c_ptr, tsum.data_ptr(), sums.data_ptr(),
                                      ops._stream()), "register_sums")
    _native.check(L.s2s_register_pick(tsum.data_ptr(), sums.data_ptr(), c_ptr, B, R, ds, shift.data_ptr(),
                                      score.data_ptr(), valid.data_ptr(), ops._stream()), "register_pick")
    return {"shift": shift, "score": score[:, 0], "score_center": score[:, 1], "margin": score[:, 2], "valid": valid,
            "tsum": tsum, "sums": sums}


def surface_scores(tsum: torch.Tensor, sums: torch.Tensor) -> torch.Tensor:
    """float64 ``[B, S, S]``: the score of every shift from the integer sums, in torch on their device."""
    n, sa, saa = (tsum[:, k].reshape(-1, 1, 1) for k in range(3))
    sb, sbb, sab = sums[..., 0], sums[..., 1], sums[..., 2]
    va, vb, num = n * saa - sa * sa, n * sbb - sb * sb, n * sab - sa * sb
    ok = (va != 0) & (vb != 0)
    den = torch.sqrt(va.to(torch.float64) * vb.to(torch.float64))
    return torch.where(ok, num.to(torch.float64) / torch.where(ok, den, torch.ones_like(den)), torch.zeros_like(den))


def register_pairs(src_u8: torch.Tensor, tgt_u8: torch.Tensor, *, radius: int = 16, downsample: int = 1,
                   refine: bool = True, center: Optional[torch.Tensor] = None, src_stains="hed", tgt_stains="hdab",
                   stain: int = 0, gain: float = DEFAULT_GAIN, return_surface: bool = False) -> Dict[str, torch.Tensor]:
    """The integer shift of every pair of a batch: ``tgt[y + dy, x + dx]`` is the tissue at ``src[y, x]``.

    ``src_u8`` / ``tgt_u8``: uint8 ``[B, H, W, 3]`` on the GPU (crop views, any row pitch and any base alignment), or
    fp32 ``[B, 3, H, W]`` in the network's range, which goes through the save conversion; each in its own stain basis
    (``src_stains`` / ``tgt_stains`` as ``stain_matrix`` takes them), compared on stain ``stain``.  ``radius``: shifts up
    to this many pixels each way are tried.  ``downsample`` ds: the maps are block-averaged first and ``ceil(radius / ds)``
    is searched at that level; with ``refine`` a second search of radius ds at full resolution around the coarse shift
    follows (two sums launches in total) and the numbers returned are those of the fine level; without it the coarse
    shift times ds is returned.  The radius of one level is at most 32.  ``center``: int32 ``[B, 2]`` on the device, the
    shift the first level searches around, in that level's pixels.

    Returns device tensors: ``"shift"`` int32 ``[B, 2]`` in full-resolution pixels; ``"score"``, ``"score_center"`` (the
    score at the centre) and ``"margin"`` (the best score minus the best outside the 3 x 3 neighbourhood of the peak, 0
    for a radius below 2) as float64 ``[B]``; ``"valid"`` int32 ``[B]``, 0 for a flat source map or an empty template,
    where ``shift`` is the centre and the scores are 0.  ``return_surface=True`` adds ``"tsum"`` int64 ``[B, 3]``,
    ``"sums"`` int64 ``[B, S, S, 3]`` and ``"scores"`` float64 ``[B, S, S]`` of the level returned."""
    what = "register_pairs"
    ds, radius = _check_downsample(downsample), _check_radius(radius)
    ws, wt = structure_weights(src_stains, stain, gain), structure_weights(tgt_stains, stain, gain)
    for name, t in (("src_u8", src_u8), ("tgt_u8", tgt_u8)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(t).__name__}")
    if src_u8.dtype != tgt_u8.dtype:
        raise ValueError(f"{what}: src_u8 is {src_u8.dtype} but tgt_u8 is {tgt_u8.dtype}")
    if tuple(src_u8.shape) != tuple(tgt_u8.shape):
        raise ValueError(f"{what}: src_u8 {list(src_u8.shape)} and tgt_u8 {list(tgt_u8.shape)} differ in shape")
    s, t = _as_u8(src_u8, "src_u8", what), _as_u8(tgt_u8, "tgt_u8", what)
    B, H, W, sp, si = _u8_layout(s, "src_u8", what)
    _, _, _, tp, ti = _u8_layout(t, "tgt_u8", what)
    if s.device != t.device:
        raise ValueError(f"{what}: the images are on different devices")
    center = _check_center(center, B, s.device, what)
    R0 = -(-radius // ds)
    if H < ds or W < ds:
        raise ValueError(f"{what}: the {H} x {W} images are smaller than one {ds} x {ds} block")
    _check_search(H // ds, W // ds, R0, what)
    two = ds > 1 and bool(refine)
    if two:
        _check_search(H, W, ds, what)
    with torch.no_grad():
        out = _level(_structure(s, B, H, W, sp, si, ws, ds), _structure(t, B, H, W, tp, ti, wt, ds), R0, center, ds)
        if two:
            out = _level(_structure(s, B, H, W, sp, si, ws, 1), _structure(t, B, H, W, tp, ti, wt, 1), ds,
                         out["shift"], 1)
        if return_surface:
            out["scores"] = surface_scores(out["tsum"], out["sums"])
        else:
            del out["tsum"], out["sums"]
    return out


def shift_tiles(tiles_u8: torch.Tensor, shift: torch.Tensor, fill: int = 255) -> torch.Tensor:
    """``out[b, y, x] = tiles_u8[b, y + dy, x + dx]`` with ``(dy, dx) = shift[b]`` inside the image and ``fill``
    outside: applied to the target of a pair with ``register_pairs``' shift it brings the target onto the source.
    ``tiles_u8``: uint8 ``[B, H, W, 3]`` images or ``[B, H, W]`` masks on the GPU (views allowed); ``shift``: int32
    ``[B, 2]`` on the device, any values.  Returns a contiguous tensor of the input's shape.  One launch."""
    what = "shift_tiles"
    if not isinstance(tiles_u8, torch.Tensor):
        raise TypeError(f"{what}: tiles_u8 must be a torch.Tensor, got {type(tiles_u8).__name__}")
    C = None if tiles_u8.dim() == 3 else 3
    B, H, W, pitch, img = _u8_layout(tiles_u8, "tiles_u8", what, C)
    fill = operator.index(fill)
    if not 0 <= fill <= 255:
        raise ValueError(f"{what}: fill must lie in 0..255, got {fill}")
    if not isinstance(shift, torch.Tensor):
        raise TypeError(f"{what}: shift must be a torch.Tensor, got {type(shift).__name__}")
    if shift.dtype != torch.int32 or tuple(shift.shape) != (B, 2) or shift.device != tiles_u8.device:
        raise ValueError(f"{what}: shift must be int32 [{B}, 2] on the images' device, got {shift.dtype} "
                         f"{list(shift.shape)} on {shift.device}")
    c = C or 1
    with torch.no_grad():
        out = torch.empty(tuple(tiles_u8.shape), dtype=torch.uint8, device=tiles_u8.device)
        rc = ops._L().s2s_shift_tiles_u8(tiles_u8.data_ptr(), pitch, img, B, H, W, c, shift.contiguous().data_ptr(),
                                         fill, out.data_ptr(), c * W, c * W * H, ops._stream())
        _native.check(rc, what)
    return out


def overlap_boxes(shift: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """int32 ``[B, 4]`` = (top, left, height, width) of the area where the source and the target shifted by
    ``shift_tiles`` both exist: the rows y with ``0 <= y + dy < H`` and the columns alike; height and width are 0 where
    there is none.  Computed with torch on ``shift``'s device (a host tensor works too)."""
    if not isinstance(shift, torch.Tensor):
        raise TypeError(f"overlap_boxes: shift must be a torch.Tensor, got {type(shift).__name__}")
    if shift.dim() != 2 or shift.shape[1] != 2 or shift.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"overlap_boxes: shift must be an integer [B, 2] tensor, got {shift.dtype} {list(shift.shape)}")
    H, W = operator.index(H), operator.index(W)
    if H < 1 or W < 1:
        raise ValueError(f"overlap_boxes: H and W must be positive, got {H} and {W}")
    d = shift.to(torch.int64)
    cols = []
    for k, size in enumerate((H, W)):                          # scalars only: no constant goes up to the device
        lo = (-d[:, k]).clamp(min=0, max=size)
        hi = (size - d[:, k]).clamp(max=size)
        cols.append((lo, (hi - lo).clamp(min=0)))
    return torch.stack([cols[0][0], cols[1][0], cols[0][1], cols[1][1]], dim=1).to(torch.int32)


def sample_crop_params_within(boxes, size: int, rng: Optional[random.Random] = None) -> torch.Tensor:
    """Crop parameters for ``paired_augment`` that stay inside the overlap of an aligned pair: host int32 ``[B, 5]`` in
    ``sample_d4_params``' layout (top, left, hflip, vflip, transpose).  ``boxes``: HOST integer ``[B, 4]``
    (``overlap_boxes(...).cpu()``).  Per sample, in this order: ``rng.randint`` for top and for left, then one
    ``rng.random() > 0.5`` for each of the three flags.  ``ValueError`` when a box is smaller than ``size``."""
    rng = rng or random
    size = operator.index(size)
    if size < 1:
        raise ValueError(f"size must be positive, got {size}")
    b = torch.as_tensor(boxes)
    if b.is_cuda:
        raise ValueError("sample_crop_params_within: boxes must be a host tensor (overlap_boxes(...).cpu())")
    if b.dim() != 2 or b.shape[1] != 4 or b.is_floating_point():
        raise ValueError(f"sample_crop_params_within: boxes must be an integer [B, 4] tensor, got {list(b.shape)}")
    rows = []
    for n, (top, left, bh, bw) in enumerate(b.tolist()):
        if bh < size or bw < size:
            raise ValueError(f"sample_crop_params_within: box {n} ({bh} x {bw}) is smaller than the {size} x {size} crop")
        rows.append([top + rng.randint(0, bh - size), left + rng.randint(0, bw - size), int(rng.random() > 0.5),
                     int(rng.random() > 0.5), int(rng.random() > 0.5)])
    return torch.tensor(rows, dtype=torch.int32).reshape(-1, 5)


def registered_quality(generated: torch.Tensor, target: torch.Tensor, radius: int = 8, *, stains="hdab",
                       **image_quality_kwargs) -> Dict[str, torch.Tensor]:
    """``image_quality`` of a generated image against a target that is registered to it first, so that a few pixels
    of offset between the pair are not scored as an error of the model.  Both images are in the target's stain basis
    ``stains``.  The target is shifted onto the generated image and both are scored on their central
    ``[radius : -radius, radius : -radius]`` crop, which every shift within the radius covers.  Inputs: uint8
    ``[B, H, W, 3]`` or fp32 ``[B, 3, H, W]`` (through the save conversion) on the GPU.  Returns ``image_quality``'s
    dict plus ``"shift"`` and ``"score"``."""
    what = "registered_quality"
    radius = _check_radius(radius)
    if image_quality_kwargs.get("quantize", True) is not True:
        raise ValueError(f"{what}: images are scored as saved bytes; quantize=False is not available")
    image_quality_kwargs.pop("quantize", None)
    reg = register_pairs(generated, target, radius=radius, src_stains=stains, tgt_stains=stains)
    g, t = _as_u8(generated, "generated", what), _as_u8(target, "target", what)
    H, W = int(g.shape[1]), int(g.shape[2])
    moved = shift_tiles(t, reg["shift"])
    r = radius
    out = dict(image_quality(g[:, r:H - r, r:W - r], moved[:, r:H - r, r:W - r], **image_quality_kwargs))
    out["shift"], out["score"] = reg["shift"], reg["score"]
    return out


def region_shift_field(src_region_u8: torch.Tensor, tgt_region_u8: torch.Tensor, cell: int = 256,
                       **register_kwargs) -> Dict[str, torch.Tensor]:
    """The shift of every whole ``cell`` x ``cell`` cell of two uint8 ``[H, W, 3]`` regions (each on the GPU or on the
    host, any row pitch): ``"shift"`` int32 ``[Gy, Gx, 2]``, ``"score"`` and ``"margin"`` float64 ``[Gy, Gx]``,
    ``"valid"`` int32 ``[Gy, Gx]`` on the device, Gy = H // cell, Gx = W // cell.  One row of cells is one
    ``register_pairs`` batch read in place (sample stride 3 * cell, row pitch that of the region); a host region is
    uploaded one cell row at a time through a pinned buffer, which waits for the previous upload.  ``register_kwargs``
    as ``register_pairs`` (no ``center``, no ``return_surface``)."""
    what = "region_shift_field"
    H, W, _ = check_region(src_region_u8, what)
    if check_region(tgt_region_u8, what) != (H, W, 3):
        raise ValueError(f"{what}: the regions differ in shape")
    cell = operator.index(cell)
    if cell < 1 or cell > H or cell > W:
        raise ValueError(f"{what}: cell {cell} does not fit the {H} x {W} regions")
    for k in ("center", "return_surface"):
        if k in register_kwargs:
            raise ValueError(f"{what}: {k} is not available here")
    dev = gpu_device(what, src_region_u8, tgt_region_u8, mismatch=ValueError)
    Gy, Gx = H // cell, W // cell
    keys = ("shift", "score", "margin", "valid")
    rows = {k: [] for k in keys}
    with torch.no_grad():
        src = [BandSource(t, cell, dev) for t in (src_region_u8, tgt_region_u8)]
        for gy in range(Gy):
            views = []
            for s in src:
                band = s.rows(gy * cell, (gy + 1) * cell)
                pitch = gpu_rows(band)[1]
                views.append(band.as_strided((Gx, cell, cell, 3), (3 * cell, pitch, 3, 1)))
            out = register_pairs(views[0], views[1], **register_kwargs)
            for k in keys:
                rows[k].append(out[k])
    return {k: torch.stack(v) for k, v in rows.items()}
