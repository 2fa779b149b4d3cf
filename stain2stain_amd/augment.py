"""Fused paired training-input augmentation: crop, the eight symmetries of the square, stain jitter, class masks.

The reference's ``use_augmentation=True`` branch crops and flips source and target with shared parameters
(src/data/paired_data_module.py:170-199); its multiclass dataset does the same to a third image, the class mask, and
hands it on unnormalised (src/data/paired_data_multiclassmask.py:104-135).  ``paired_augment`` is that chain in one
launch (``csrc/augment.hip``), with two things the reference does not have:

  transpose   a fifth parameter column.  With ``f = crop[::-1 if vflip][:, ::-1 if hflip]`` the output is
              ``f.swapaxes(0, 1)`` when it is set: two flips and a transpose generate all eight symmetries of the
              square (D4), the 90 degree rotations among them
  stain map   12 fp32 numbers per sample and image kind, ``A`` ([3, 3], row-major) and ``b`` ([3]), applied in
              optical-density space: ``od' = od @ A + b`` with ``od = od_table()[byte]``, then
              ``u' = clamp(rint(255 * 10 ** -od'), 0, 255)``.  ``stain_jitter_maps`` folds the stain augmentation of
              Tellez et al. (2018), ``c' = alpha * c + beta`` per stain concentration, into such a map

With ``white`` given, a pixel with ``min(R, G, B) >= white`` keeps its bytes: glass is not tinted (the tissue rule of
``tissue_counts``).  Without a map the bytes pass and the result is bit-equal to ``paired_crop_flip_normalize``.

Parameters and maps are small host tensors; they go up in one small asynchronous copy from pinned memory.  Nothing here
waits for the device.  GPU only.
"""
from __future__ import annotations

import math
import operator
import random
from collections import deque
from typing import Optional, Tuple

import numpy as np
import torch

from . import _native, ops
from ._regionio import batch_layout
from .data import sample_crop_flip_params
from .stain_norm import _od_floats
from .stain_quant import stain_matrix

_MASK_KINDS = {torch.float32: 1, torch.uint8: 2, torch.int64: 3}
_PINNED = deque(maxlen=8)      # host tables whose asynchronous copies may still be in flight


# ---- samplers (host) -------------------------------------------------------------------------------------------------
def sample_d4_params(batch: int, src_hw: Tuple[int, int], size: int, rng: Optional[random.Random] = None,
                     transpose: bool = True) -> torch.Tensor:
    """int32 ``[B, 5]`` = (top, left, hflip, vflip, transpose).  The first four columns are those of
    ``sample_crop_flip_params`` (the same draws in the same order: equal under the same seed); after them one
    ``rng.random() > 0.5`` per sample decides the transpose.  ``transpose=False`` draws nothing more and leaves the
    column 0."""
    rng = rng or random
    p4 = sample_crop_flip_params(batch, src_hw, size, rng)
    t = [int(rng.random() > 0.5) if transpose else 0 for _ in range(batch)]
    return torch.cat([p4.reshape(batch, 4), torch.tensor(t, dtype=torch.int32).reshape(batch, 1)], dim=1)


def _sigma(v, name: str) -> float:
    v = float(v)
    if not math.isfinite(v) or v < 0.0:
        raise ValueError(f"{name} must be a finite non-negative number, got {v}")
    return v


def sample_stain_jitter(batch: int, sigma_alpha: float = 0.05, sigma_beta: float = 0.01,
                        rng: Optional[random.Random] = None) -> torch.Tensor:
    """float64 ``[B, 6]`` = (alpha0, alpha1, alpha2, beta0, beta1, beta2) with alpha ~ U[1 - sigma_alpha, 1 + sigma_alpha]
    and beta ~ U[-sigma_beta, sigma_beta]: six ``rng.uniform`` draws per sample, in that order.  The defaults are a
    convention (the "light" H&E setting of Tellez et al. 2018 and of open-source pathology toolkits), not a calibration:
    how much colour shift a model has to tolerate depends on the labs and scanners it will meet."""
    rng = rng or random
    batch = operator.index(batch)
    if batch < 1:
        raise ValueError(f"batch must be positive, got {batch}")
    sa, sb = _sigma(sigma_alpha, "sigma_alpha"), _sigma(sigma_beta, "sigma_beta")
    rows = []
    for _ in range(batch):
        alpha = [rng.uniform(1.0 - sa, 1.0 + sa) for _ in range(3)]
        rows.append(alpha + [rng.uniform(-sb, sb) for _ in range(3)])
    return torch.tensor(rows, dtype=torch.float64)


def _bases(stains, B: int) -> torch.Tensor:
    """float64 ``[B, 3, 3]``: one ``stain_matrix`` per sample."""
    def is_basis(s) -> bool:                   # a name, a 2-d array, or a list of rows of numbers
        return isinstance(s, str) or getattr(s, "ndim", None) == 2 or (
            isinstance(s, (list, tuple)) and len(s) > 0 and isinstance(s[0], (list, tuple)))

    if isinstance(stains, (list, tuple)):
        batch = len(stains) > 0 and is_basis(stains[0])
    else:
        batch = getattr(stains, "ndim", None) == 3
    if not batch:
        return stain_matrix(stains).expand(B, 3, 3)
    per = [stain_matrix(s) for s in stains]
    if len(per) != B:
        raise ValueError(f"stains: {len(per)} bases for a batch of {B}")
    return torch.stack(per)


def stain_jitter_maps(jitter, stains="hed") -> torch.Tensor:
    """Fold a stain jitter into the kernels' OD map: host float64 ``[B, 6]`` (``sample_stain_jitter``) -> host fp32
    ``[B, 12]`` = ``A`` row-major, then ``b``.  With ``M = stain_matrix(stains)`` (unit rows), in float64 and rounded to
    fp32 once: ``A = inv(M) @ diag(alpha) @ M`` and ``b = beta @ M``, so that ``od @ A + b`` are the optical densities
    of the concentrations ``alpha * c + beta``.

    ``stains``: a name (``"hed"``, ``"hdab"``), a ``[2, 3]`` or ``[3, 3]`` array (a ``StainFit.vectors`` is one), or one
    basis per sample as a list or a ``[B, 2 | 3, 3]`` array: the tiles of a batch come from different slides.
    ``ValueError`` for a singular basis or a non-finite jitter."""
    j = torch.as_tensor(jitter, dtype=torch.float64).detach().to("cpu")
    if j.dim() != 2 or j.shape[1] != 6 or j.shape[0] < 1:
        raise ValueError(f"jitter must be [B, 6] = (alpha0..2, beta0..2), got {list(j.shape)}")
    if not torch.isfinite(j).all():
        raise ValueError("jitter must be finite")
    B = int(j.shape[0])
    M = _bases(stains, B)
    # inv(M) diag(alpha) M evaluated as I + inv(M) diag(alpha - 1) M: the same matrix, but the rounding of the two
    # products scales with the jitter and not with 1, and alpha = 1 gives the identity exactly
    A = torch.eye(3, dtype=torch.float64) + torch.linalg.inv(M) @ torch.diag_embed(j[:, :3] - 1.0) @ M
    b = (j[:, None, 3:] @ M)[:, 0]
    maps = torch.cat([A.reshape(B, 9), b], dim=1).to(torch.float32)
    if not torch.isfinite(maps).all():
        raise ValueError("the folded stain map is not finite")
    return maps


# ---- argument checks -------------------------------------------------------------------------------------------------
def _check_u8(t, name: str, last: Optional[int], what: str):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(t).__name__}")
    dims = 4 if last else 3
    shape = "[B, H, W, 3]" if last else "[B, H, W]"
    if t.dtype != torch.uint8:
        raise ValueError(f"{what}: {name} must be uint8 {shape}, got {t.dtype}")
    if t.dim() != dims or (last and t.shape[3] != last) or min(t.shape) < 1:
        raise ValueError(f"{what}: {name} must be a non-empty uint8 {shape}, got {list(t.shape)}")
    if not t.is_cuda:
        raise ValueError(f"{what}: {name} must be on the GPU (there is no CPU path)")
    if last:
        if t.stride(3) != 1 or (t.shape[2] > 1 and t.stride(2) != 3):
            raise ValueError(f"{what}: the pixels of {name} must be contiguous within a row")
    elif t.shape[2] > 1 and t.stride(2) != 1:
        raise ValueError(f"{what}: the pixels of {name} must be contiguous within a row")


def _check_params(params, B: int, H: int, W: int, size: int, what: str) -> torch.Tensor:
    if not isinstance(params, torch.Tensor):
        raise TypeError(f"{what}: params must be a torch.Tensor, got {type(params).__name__}")
    if params.is_cuda or params.dtype != torch.int32:
        raise ValueError(f"{what}: params must be a host int32 tensor, got {params.dtype} on {params.device}")
    if params.dim() != 2 or params.shape[0] != B or params.shape[1] not in (4, 5):
        raise ValueError(f"{what}: params must be [{B}, 4] or [{B}, 5], got {list(params.shape)}")
    a = params.numpy()                                  # a view: two reductions instead of six tensor round trips
    lo, hi = a.min(0).tolist(), a.max(0).tolist()
    if lo[0] < 0 or lo[1] < 0 or hi[0] + size > H or hi[1] + size > W:
        raise ValueError(f"{what}: params has a crop window outside the {H} x {W} image")
    if min(lo[2:]) < 0 or max(hi[2:]) > 1:
        raise ValueError(f"{what}: the flip and transpose flags of params must be 0 or 1")
    return params


def _check_map(m, name: str, B: int, what: str) -> Optional[torch.Tensor]:
    if m is None:
        return None
    if not isinstance(m, torch.Tensor):
        raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(m).__name__}")
    if m.is_cuda or m.dtype != torch.float32 or tuple(m.shape) != (B, 12):
        raise ValueError(f"{what}: {name} must be a host fp32 [{B}, 12] tensor, got {m.dtype} {list(m.shape)} on "
                         f"{m.device}")
    if not np.isfinite(m.numpy()).all():
        raise ValueError(f"{what}: {name} must be finite")
    return m


def _check_white(white, what: str) -> int:
    if white is None:
        return -1
    white = operator.index(white)
    if not 0 <= white <= 255:
        raise ValueError(f"{what}: white must lie in 0..255, got {white}")
    return white


def _upload(dev: torch.device, params: Optional[torch.Tensor], maps) -> list:
    """The host tables in one pinned buffer and one asynchronous copy; returns their device addresses (0: absent)."""
    parts = [None if params is None else params.numpy().reshape(-1)]
    parts += [None if m is None else m.numpy().reshape(-1).view(np.int32) for m in maps]
    host = torch.empty((sum(p.size for p in parts if p is not None),), dtype=torch.int32, pin_memory=True)
    words = host.numpy()
    at, offs = 0, []
    for p in parts:
        offs.append(None if p is None else at)
        if p is not None:
            words[at:at + p.size] = p
            at += p.size
    _PINNED.append(host)
    buf = host.to(dev, non_blocking=True)
    return [buf] + [0 if o is None else buf.data_ptr() + 4 * o for o in offs]


# ---- the device calls ------------------------------------------------------------------------------------------------
def paired_augment(src_u8: torch.Tensor, tgt_u8: torch.Tensor, params: torch.Tensor, size: int, *,
                   mask_u8: Optional[torch.Tensor] = None, mask_dtype: torch.dtype = torch.float32,
                   src_map: Optional[torch.Tensor] = None, tgt_map: Optional[torch.Tensor] = None,
                   white: Optional[int] = None, return_u8: bool = False):
    """Crop, flip, transpose, stain-map and normalise a batch of paired tiles in one launch.

    ``src_u8`` / ``tgt_u8``: uint8 ``[B, H, W, 3]`` on the GPU, pixels contiguous within a row (crop views of a larger
    array work without a copy); ``mask_u8``: uint8 ``[B, H, W]``, the class mask, which takes the same geometry;
    ``params``: host int32 ``[B, 4]`` or ``[B, 5]`` = (top, left, hflip, vflip[, transpose]) (``sample_d4_params``);
    ``src_map`` / ``tgt_map``: host fp32 ``[B, 12]`` (``stain_jitter_maps``), ``None``: that image's colours stay;
    ``white``: 0..255, pixels with ``min(R, G, B) >= white`` keep their bytes under a map; ``None``: every pixel is mapped.

    Returns ``(src, tgt)`` as fp32 ``[B, 3, size, size]`` = ``(u / 255 - 0.5) / 0.5``; with a mask ``(src, tgt, mask)``,
    the mask ``[B, 1, size, size]`` in ``mask_dtype`` (float32, uint8 or int64) holding the byte's value, unscaled as in
    the reference; ``return_u8=True`` appends the two augmented uint8 ``[B, size, size, 3]`` images.  With ``[B, 4]``
    params and no map the first two are bit-equal to ``paired_crop_flip_normalize``.  Nothing waits for the device."""
    what = "paired_augment"
    _check_u8(src_u8, "src_u8", 3, what)
    _check_u8(tgt_u8, "tgt_u8", 3, what)
    if tuple(src_u8.shape) != tuple(tgt_u8.shape):
        raise ValueError(f"{what}: src_u8 {list(src_u8.shape)} and tgt_u8 {list(tgt_u8.shape)} differ in shape")
    B, H, W = (int(v) for v in src_u8.shape[:3])
    if mask_u8 is not None:
        _check_u8(mask_u8, "mask_u8", None, what)
        if tuple(mask_u8.shape) != (B, H, W):
            raise ValueError(f"{what}: mask_u8 must be {[B, H, W]}, got {list(mask_u8.shape)}")
    if mask_dtype not in _MASK_KINDS:
        raise ValueError(f"{what}: mask_dtype must be torch.float32, torch.uint8 or torch.int64, got {mask_dtype}")
    size = operator.index(size)
    if size < 1 or size > H or size > W:
        raise ValueError(f"{what}: size {size} does not fit the {H} x {W} images")
    params = _check_params(params, B, H, W, size, what)
    src_map, tgt_map = _check_map(src_map, "src_map", B, what), _check_map(tgt_map, "tgt_map", B, what)
    white = _check_white(white, what)
    dev = src_u8.device
    if tgt_u8.device != dev or (mask_u8 is not None and mask_u8.device != dev):
        raise ValueError(f"{what}: the images are on different devices")
    with torch.no_grad():
        s, sp, si = batch_layout(src_u8, what, "src_u8")
        t, tp, ti = batch_layout(tgt_u8, what, "tgt_u8")
        mp, mi = batch_layout(mask_u8, what, "mask_u8")[1:] if mask_u8 is not None else (0, 0)
        keep, p_ptr, sm_ptr, tm_ptr = _upload(dev, params, (src_map, tgt_map))
        out_s = torch.empty((B, 3, size, size), dtype=torch.float32, device=dev)
        out_t = torch.empty_like(out_s)
        out_m = torch.empty((B, 1, size, size), dtype=mask_dtype, device=dev) if mask_u8 is not None else None
        u8_s = torch.empty((B, size, size, 3), dtype=torch.uint8, device=dev) if return_u8 else None
        u8_t = torch.empty_like(u8_s) if return_u8 else None
        ptr = lambda x: 0 if x is None else x.data_ptr()      # noqa: E731
        table = _od_floats() if (src_map is not None or tgt_map is not None) else None
        rc = ops._L().s2s_paired_augment(s.data_ptr(), sp, si, t.data_ptr(), tp, ti, ptr(mask_u8), mp, mi, B, H, W, size,
                                         p_ptr, int(params.shape[1]), sm_ptr, tm_ptr, table, white, out_s.data_ptr(),
                                         out_t.data_ptr(), ptr(out_m), _MASK_KINDS[mask_dtype] if out_m is not None else 0,
                                         ptr(u8_s), ptr(u8_t), ops._stream())
        _native.check(rc, what)
        del keep
    out = (out_s, out_t) + ((out_m,) if out_m is not None else ()) + ((u8_s, u8_t) if return_u8 else ())
    return out


def stain_augment(tiles_u8: torch.Tensor, maps: torch.Tensor, *, white: Optional[int] = None,
                  network_input: bool = False) -> torch.Tensor:
    """The stain map alone: uint8 ``[B, H, W, 3]`` on the GPU (any H and W, crop views allowed) under host fp32
    ``[B, 12]`` ``maps`` -> uint8 ``[B, H, W, 3]``, or with ``network_input=True`` fp32 ``[B, 3, H, W]`` =
    ``(u8 / 255 - 0.5) / 0.5`` of those bytes.  ``white`` as ``paired_augment``.  One launch, no synchronisation."""
    what = "stain_augment"
    _check_u8(tiles_u8, "tiles_u8", 3, what)
    B, H, W = (int(v) for v in tiles_u8.shape[:3])
    if maps is None:
        raise TypeError(f"{what}: maps must be a host fp32 [B, 12] tensor, got None")
    maps = _check_map(maps, "maps", B, what)
    white = _check_white(white, what)
    with torch.no_grad():
        t, pitch, stride = batch_layout(tiles_u8, what, "tiles_u8")
        keep, _, m_ptr = _upload(t.device, None, (maps,))
        if network_input:
            out = torch.empty((B, 3, H, W), dtype=torch.float32, device=t.device)
        else:
            out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=t.device)
        rc = ops._L().s2s_stain_augment_u8(t.data_ptr(), pitch, stride, B, H, W, m_ptr, _od_floats(), white,
                                           out.data_ptr(), 3 * W, 3 * W * H, int(network_input), ops._stream())
        _native.check(rc, what)
        del keep
    return out


class PairedAugmenter:
    """Samples the geometry and the stain jitter of a batch and applies them in one ``paired_augment`` launch.

    ``size``: the crop; ``sigma_alpha`` / ``sigma_beta``: as ``sample_stain_jitter``; ``src_stains`` / ``tgt_stains``:
    the stain basis of each image kind as ``stain_jitter_maps`` takes it, ``None``: that kind's colours are untouched
    (the default for the target: its colours are what the model is to learn); ``transpose``: draw the fifth parameter
    (all eight symmetries) or keep to the four of two flips; ``white``: as ``paired_augment``; ``rng``: a
    ``random.Random``.  Per call the draws are, in this order: ``sample_d4_params``, the source's
    ``sample_stain_jitter`` (when ``src_stains`` is given), the target's (when ``tgt_stains`` is given)."""

    def __init__(self, size: int, sigma_alpha: float = 0.05, sigma_beta: float = 0.01, src_stains="hed",
                 tgt_stains=None, transpose: bool = True, white: Optional[int] = None,
                 rng: Optional[random.Random] = None):
        self.size = operator.index(size)
        if self.size < 1:
            raise ValueError(f"size must be positive, got {size}")
        self.sigma_alpha, self.sigma_beta = _sigma(sigma_alpha, "sigma_alpha"), _sigma(sigma_beta, "sigma_beta")
        for s in (src_stains, tgt_stains):
            if s is not None and not isinstance(s, (list, tuple)) and getattr(s, "ndim", 2) != 3:
                stain_matrix(s)                            # a bad basis fails here, not in the first step
        self.src_stains, self.tgt_stains = src_stains, tgt_stains
        self.transpose = bool(transpose)
        _check_white(white, "PairedAugmenter")
        self.white = white
        self.rng = rng or random

    def _maps(self, stains, B: int) -> Optional[torch.Tensor]:
        if stains is None:
            return None
        return stain_jitter_maps(sample_stain_jitter(B, self.sigma_alpha, self.sigma_beta, self.rng), stains)

    def __call__(self, src_u8: torch.Tensor, tgt_u8: torch.Tensor, mask_u8: Optional[torch.Tensor] = None,
                 mask_dtype: torch.dtype = torch.float32):
        _check_u8(src_u8, "src_u8", 3, "PairedAugmenter")
        B, H, W = (int(v) for v in src_u8.shape[:3])
        params = sample_d4_params(B, (H, W), self.size, self.rng, self.transpose)
        src_map = self._maps(self.src_stains, B)
        tgt_map = self._maps(self.tgt_stains, B)
        return paired_augment(src_u8, tgt_u8, params, self.size, mask_u8=mask_u8, mask_dtype=mask_dtype,
                              src_map=src_map, tgt_map=tgt_map, white=self.white)
