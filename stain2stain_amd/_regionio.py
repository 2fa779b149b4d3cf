"""What every whole-region call shares on the host side: the layout of uint8 regions and batches, the GPU a call runs
on, and the pinned bands a host region is streamed through, to the GPU (``BandSource``) and back (``BandSink``).

A region is uint8 ``[H, W, 3]`` (or an ``[H, W]`` mask) on the GPU or on the host, with any row pitch and pixels that
are contiguous within a row; a batch is ``[B, H, W, 3]`` or ``[B, H, W]`` on the GPU.  Private to the package: the
feature modules take their plumbing from here and not from each other."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

DEFAULT_HOST_BAND = 512            # band rows of a host region when band_rows is not given


# ---- layout ----------------------------------------------------------------------------------------------------------
def _pixels_contiguous(t: torch.Tensor, C: int) -> bool:
    """The last dimensions of ``t`` are ``[W, 3]`` (C = 3) or ``[W]`` (C = 1): one row is W * C consecutive bytes."""
    if C == 1:
        return t.shape[-1] == 1 or t.stride(-1) == 1
    return t.stride(-1) == 1 and (t.shape[-2] == 1 or t.stride(-2) == C)


def check_region(t, what: str, mask_ok: bool = False) -> Tuple[int, int, int]:
    """(H, W, C) of a non-empty uint8 ``[H, W, 3]`` region (C = 3) or, with ``mask_ok``, ``[H, W]`` mask (C = 1) whose
    pixels are contiguous within a row.  The row pitch is free: host rows may even overlap, GPU rows are checked where
    their pitch is taken (``gpu_rows``, ``batch_layout``)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: the region must be a torch.Tensor, got {type(t).__name__}")
    if t.dtype != torch.uint8:
        raise ValueError(f"{what}: the region must be uint8, got {t.dtype}")
    is_mask = mask_ok and t.dim() == 2
    if not (is_mask or (t.dim() == 3 and t.shape[2] == 3)) or min(t.shape) < 1:
        kinds = "[H, W, 3] image or [H, W] mask" if mask_ok else "[H, W, 3] RGB image"
        raise ValueError(f"{what}: the region must be a non-empty {kinds}, got {list(t.shape)}")
    C = 1 if is_mask else 3
    if not _pixels_contiguous(t, C):
        raise ValueError(f"{what}: pixels within a row must be contiguous")
    return int(t.shape[0]), int(t.shape[1]), C


def gpu_rows(view: torch.Tensor) -> Tuple[int, int]:
    """(data_ptr, row pitch in bytes) of a uint8 ``[rows, W, 3]`` or ``[rows, W]`` GPU view whose pixels are contiguous
    within a row: what a kernel reads a band through."""
    if view.dtype != torch.uint8 or view.dim() not in (2, 3) or (view.dim() == 3 and view.shape[2] != 3):
        raise RuntimeError("stain2stain_amd: expected a uint8 [rows, W, 3] image or [rows, W] mask")
    C = 3 if view.dim() == 3 else 1
    if not _pixels_contiguous(view, C):
        raise RuntimeError("stain2stain_amd: image pixels must be contiguous within a row")
    rows, W = view.shape[0], view.shape[1]
    pitch = view.stride(0) if rows > 1 else C * W
    if pitch < C * W:
        raise RuntimeError("stain2stain_amd: image rows overlap")
    if not view.is_cuda:
        raise RuntimeError("stain2stain_amd: tensor is not on the GPU (there is no CPU path)")
    return view.data_ptr(), pitch


def batch_layout(t: torch.Tensor, what: str, name: str = "the uint8 images", *, copy: bool = False,
                 interleave: bool = False) -> Tuple[torch.Tensor, int, int]:
    """(tensor, row pitch, sample stride) in bytes of a uint8 ``[B, H, W, 3]`` or ``[B, H, W]`` batch.  A view whose
    pixels are not contiguous within a row is copied with ``copy`` and rejected without.  A single row takes the pitch
    C * W and a single sample the stride pitch * H, whatever the view's own strides say.  Rows must not overlap, and
    neither must samples unless ``interleave`` allows it (the cells of one cell row of a region: stride 3 * cell)."""
    C = 3 if t.dim() == 4 else 1
    if not _pixels_contiguous(t, C):
        if not copy:
            raise ValueError(f"{what}: the pixels of {name} must be contiguous within a row")
        t = t.contiguous()
    B, H, W = (int(v) for v in t.shape[:3])
    pitch = t.stride(1) if H > 1 else C * W
    stride = t.stride(0) if B > 1 else pitch * H
    if pitch < C * W or stride < (1 if interleave else pitch * H):
        raise ValueError(f"{what}: the rows or samples of {name} overlap")
    return t, pitch, stride


# ---- device ----------------------------------------------------------------------------------------------------------
def gpu_device(what: str, *tensors: torch.Tensor, host_ok: bool = True, mismatch=RuntimeError) -> torch.device:
    """The GPU the call ``what`` runs on: that of its GPU tensors, which must agree (``mismatch`` is raised otherwise),
    or the current one when every tensor lives on the host.  ``host_ok=False``: a host tensor is refused."""
    gpu = [t.device for t in tensors if t.is_cuda]
    if not host_ok and len(gpu) < len(tensors):
        raise RuntimeError(f"stain2stain_amd: {what} needs GPU tensors (there is no CPU path)")
    if any(d != gpu[0] for d in gpu):
        raise mismatch(f"stain2stain_amd: {what}: the tensors are on different devices")
    if gpu:
        return gpu[0]
    if not torch.cuda.is_available():
        raise RuntimeError(f"stain2stain_amd: {what} needs a GPU (there is no CPU path)")
    return torch.device("cuda", torch.cuda.current_device())


# ---- streaming -------------------------------------------------------------------------------------------------------
class BandSource:
    """Rows [r0, r1) of a uint8 region as a GPU view: the region's own rows when it lives on the GPU, otherwise a band
    buffer of ``rows`` rows fed through one pinned staging buffer.  ``band_bytes``: the size of that buffer (0 on the
    GPU).  The view of a host region is good until the next ``rows`` call."""

    def __init__(self, img: torch.Tensor, rows: int, device):
        self.img, self.on_gpu, self.band_bytes = img, img.is_cuda, 0
        if not self.on_gpu:
            shape = (rows,) + tuple(img.shape[1:])
            self.stage = torch.empty(shape, dtype=torch.uint8, pin_memory=True)
            self.band = torch.empty(shape, dtype=torch.uint8, device=device)
            self.band_bytes = self.band.numel()
            self.ready = None                     # the GPU's last read of the staging buffer

    def rows(self, r0: int, r1: int) -> torch.Tensor:
        if self.on_gpu:
            return self.img[r0:r1]
        if self.ready is not None:
            self.ready.synchronize()              # the previous upload has left the staging buffer
        n = r1 - r0
        self.stage[:n].copy_(self.img[r0:r1])
        self.band[:n].copy_(self.stage[:n], non_blocking=True)
        self.ready = torch.cuda.Event()
        self.ready.record()
        return self.band[:n]


class BandSink:
    """The host result of a banded call: uint8 of ``shape`` (``[H, W, 3]`` or ``[H, W]``) and, with ``f_channels``, fp32
    ``[H, W, f_channels]`` beside it, filled band by band from GPU rows through one pinned staging buffer each, at most
    ``rows`` rows at a time.  The copy out of the GPU rows is ordered on the current stream, so they may be written
    again at once; the staging buffers are reused only after the event behind the copy."""

    def __init__(self, shape, rows: int, f_channels: Optional[int] = None):
        shape = tuple(shape)
        self.u8 = torch.empty(shape, dtype=torch.uint8)
        self.stage = torch.empty((rows,) + shape[1:], dtype=torch.uint8, pin_memory=True)
        self.f = self.stage_f = None
        if f_channels:
            self.f = torch.empty(shape[:2] + (f_channels,), dtype=torch.float32)
            self.stage_f = torch.empty((rows, shape[1], f_channels), dtype=torch.float32, pin_memory=True)
        self.pending = None                       # rows in flight: (event, r0, r1)

    def _drain(self) -> None:
        if self.pending is not None:
            ev, r0, r1 = self.pending
            ev.synchronize()
            self.u8[r0:r1] = self.stage[:r1 - r0]
            if self.f is not None:
                self.f[r0:r1] = self.stage_f[:r1 - r0]
            self.pending = None

    def put(self, gpu_u8: torch.Tensor, r0: int, r1: int, gpu_f: Optional[torch.Tensor] = None) -> None:
        """Result rows [r0, r1) are the first r1 - r0 rows of ``gpu_u8`` (and of ``gpu_f``)."""
        self._drain()                             # the staging buffers are free again
        n = r1 - r0
        self.stage[:n].copy_(gpu_u8[:n], non_blocking=True)
        if self.f is not None:
            self.stage_f[:n].copy_(gpu_f[:n], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.pending = (ev, r0, r1)

    def close(self) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """(uint8 result, fp32 result or None), every band landed."""
        self._drain()
        return self.u8, self.f
