"""Result rendering: turn what the analysis calls return into pictures a person can look at.

``translate_region`` returns a region, ``region_stain_map`` and ``region_qc_map`` node maps, ``label_components``,
``stain_objects(return_labels=True)`` and ``split_objects`` label images, the tissue rule and ``mask_morphology`` byte
masks, ``register_region`` and ``align_regions`` an aligned target.  This module draws them over the region
(``csrc/render.hip``), in integers:

  mix(b, c, a)     (b (256 - a) + c a + 128) >> 8 per channel, a in 0..256: a = 0 is b, a = 256 is c
  classes, labels  id(p) = the mask byte, or max(L, 0); colour index k(p) = the mask byte, or 0 for L <= 0 and
                   ((L - 1) mod 255) + 1 otherwise.  p is an edge pixel iff outline >= 1, id(p) != 0 and an offset with
                   1 <= |dy| + |dx| <= outline leads outside the region or to another identity (identities, not colours:
                   touching parts of one colour keep their own outlines).  out = mix(base, edge colour, outline_alpha) on
                   edge pixels and mix(base, palette[k], class_alpha[k]) elsewhere
  heat             a node map Q int32 [Gy, Gx] in 0..65280 over cell x cell cells, Gy in {H // cell, ceil(H / cell)};
                   d = Q[min(y // cell, Gy - 1)][min(x // cell, Gx - 1)], or with ``smooth`` the dense interpolation of
                   ``warp_region`` between the cell centres; idx = (d + 128) >> 8; out = mix(base, lut[idx], alpha) where
                   idx >= min_index, base elsewhere
  compare          checkerboard of cell x cell squares, mix(a, b, alpha), or min(255, |a - b| gain)
  thumbnail        [ceil(H / f), ceil(W / f)]: floor((2 sum + n) / (2 n)) over the n pixels of a block inside the region;
                   for a mask the block's maximum

A numpy int64 restatement is bit-equal, for host and GPU input and for every banding.  A GPU region takes one launch per
layer and nothing waits for the device; a host region is streamed in bands of output rows through pinned staging, masks
and labels with their halo of ``outline`` rows.  GPU only.  The reference's inference scripts end in a matplotlib panel
of source, generated stain and target composed on the host; ``compose_panels`` is that figure.
"""
from __future__ import annotations

import functools
import operator
from collections import OrderedDict
from typing import Callable, List, Optional, Sequence, Tuple

import torch

from . import _native, ops
from ._regionio import DEFAULT_HOST_BAND, BandSink, BandSource, check_region, gpu_device, gpu_rows

MAX_OUTLINE = 4              # RD_MAX_R of csrc/render.hip
MAX_CELL = 1 << 14           # heat: span^2 * 65280 stays below 2^46
MAX_NODES = 65536
MAX_FACTOR = 256
QMAX = 65280                 # 255 * 256: the node value of colour index 255
COMPARE_MODES = ("checker", "blend", "difference")

_PALETTE8 = ((230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180),
             (70, 240, 240), (240, 50, 230))
_COLORMAPS = {
    "gray": ((0, (0, 0, 0)), (255, (255, 255, 255))),
    "heat": ((0, (0, 0, 0)), (85, (255, 0, 0)), (170, (255, 255, 0)), (255, (255, 255, 255))),
    "blue_red": ((0, (0, 0, 255)), (128, (255, 255, 255)), (255, (255, 0, 0))),
}


# ---- palettes and colour tables -------------------------------------------------------------------------------------------
def default_palette() -> torch.Tensor:
    """The class palette, host uint8 ``[256, 3]``: index 0 is black, index k >= 1 entry ``(k - 1) % 8`` of eight
    well-separated colours."""
    return _palette_host().clone()


@functools.lru_cache(maxsize=None)
def _palette_host() -> torch.Tensor:
    rows = [(0, 0, 0)] + [_PALETTE8[(k - 1) % 8] for k in range(1, 256)]
    return torch.tensor(rows, dtype=torch.uint8)


def colormap(name: str) -> torch.Tensor:
    """A colour table, host uint8 ``[256, 3]``: ``"gray"``, ``"heat"`` (black, red, yellow, white) or ``"blue_red"``
    (blue, white, red), piecewise linear between its anchors in integers:
    ``c = (c0 (i1 - i) + c1 (i - i0) + (i1 - i0) // 2) // (i1 - i0)``."""
    return _colormap_host(name).clone()


def _colormap_host(name) -> torch.Tensor:
    if not isinstance(name, str) or name not in _COLORMAPS:
        raise ValueError(f"colormap: name must be one of {sorted(_COLORMAPS)}, got {name!r}")
    return _build_colormap(name)


@functools.lru_cache(maxsize=None)
def _build_colormap(name: str) -> torch.Tensor:
    anchors = _COLORMAPS[name]
    rows = []
    for i in range(256):
        (i0, c0), (i1, c1) = next((a, b) for a, b in zip(anchors, anchors[1:]) if a[0] <= i <= b[0])
        rows.append([(u * (i1 - i) + v * (i - i0) + (i1 - i0) // 2) // (i1 - i0) for u, v in zip(c0, c1)])
    return torch.tensor(rows, dtype=torch.uint8)


_TABLES: "OrderedDict[tuple, Tuple[torch.Tensor, torch.Tensor]]" = OrderedDict()
_TABLES_MAX = 64


def _device_table(host: torch.Tensor, dev: torch.device) -> torch.Tensor:
    """``host`` (a small contiguous host tensor) on ``dev``: one pinned upload per device and content, kept with its
    pinned source, so a call with a table it has seen costs no copy and no call waits for the device."""
    key = (dev.index, host.dtype, tuple(host.shape), host.numpy().tobytes())
    hit = _TABLES.get(key)
    if hit is None:
        pinned = host.pin_memory()
        hit = (pinned, pinned.to(dev, non_blocking=True))
        _TABLES[key] = hit
        while len(_TABLES) > _TABLES_MAX:
            _TABLES.popitem(last=False)
    else:
        _TABLES.move_to_end(key)
    return hit[1]


def _check_table(table, what: str, name: str) -> torch.Tensor:
    """A caller's uint8 ``[256, 3]`` table, on the host or on a GPU."""
    if not isinstance(table, torch.Tensor):
        raise TypeError(f"{what}: {name} must be a uint8 [256, 3] torch.Tensor, got {type(table).__name__}")
    if table.dtype != torch.uint8 or tuple(table.shape) != (256, 3):
        raise ValueError(f"{what}: {name} must be uint8 [256, 3], got {table.dtype} {list(table.shape)}")
    return table


def _place_table(table: torch.Tensor, dev: torch.device, what: str, name: str) -> torch.Tensor:
    """A checked table on ``dev``: a device tensor is taken as it is, a host tensor is uploaded (once per content)."""
    if table.is_cuda:
        if table.device != dev:
            raise ValueError(f"{what}: {name} must be on the host or on the region's device")
        return table.contiguous()
    return _device_table(table.contiguous(), dev)


def _in_range(v, lo: int, hi: int, what: str, name: str) -> int:
    v = operator.index(v)
    if not lo <= v <= hi:
        raise ValueError(f"{what}: {name} must lie in {lo}..{hi}, got {v}")
    return v


def _check_band_rows(band_rows, what: str) -> Optional[int]:
    if band_rows is None:
        return None
    band_rows = operator.index(band_rows)
    if band_rows < 1:
        raise ValueError(f"{what}: band_rows must be positive, got {band_rows}")
    return band_rows


# ---- the band driver ------------------------------------------------------------------------------------------------------
def _same_side(what: str, first: torch.Tensor, *others: torch.Tensor) -> None:
    for t in others:
        if t.device != first.device:
            raise ValueError(f"{what}: the region and every image, mask or label image with it must live on one device, "
                             f"got {first.device} and {t.device}")


def _row_bytes(t: torch.Tensor) -> torch.Tensor:
    """A uint8 ``[H, W, 3]`` / ``[H, W]`` region as it is; a bool mask or an int32 label image as its bytes, ``[H, W]`` or
    ``[H, 4 W]``."""
    return t if t.dtype == torch.uint8 else t.view(torch.uint8)


def _check_out(out, region: torch.Tensor, what: str) -> None:
    if not isinstance(out, torch.Tensor):
        raise TypeError(f"{what}: out must be a torch.Tensor, got {type(out).__name__}")
    if out.dtype != torch.uint8 or out.shape != region.shape or out.device != region.device:
        raise ValueError(f"{what}: out must be uint8 {list(region.shape)} on the region's device, got {out.dtype} "
                         f"{list(out.shape)} on {out.device}")
    H, W = int(region.shape[0]), int(region.shape[1])
    check_region(out, what)
    po, pr = out.data_ptr(), region.data_ptr()
    so, sr = (out.stride(0), region.stride(0)) if H > 1 else (3 * W, 3 * W)
    if so < 3 * W:
        raise ValueError(f"{what}: the rows of out overlap")
    if po == pr and so == sr:
        return
    if po < pr + (H - 1) * sr + 3 * W and pr < po + (H - 1) * so + 3 * W:
        raise ValueError(f"{what}: out may be the region itself but must not overlap it in part")


def _run(what: str, inputs: Sequence[Tuple[torch.Tensor, Callable[[int, int], Tuple[int, int]]]], out_shape, out,
         band_rows: Optional[int], host_band: int, launch) -> torch.Tensor:
    """Run ``launch`` over bands of output rows.  ``inputs``: (uint8 rows ``[H, ...]``, need) with ``need(r0, n)`` the
    input rows ``[s0, s1)`` that output rows ``[r0, r0 + n)`` read; all on one device.  ``launch(r0, n, views, ptr,
    pitch)`` gets per input ``(ptr, pitch, s0, s1 - s0)`` and the output rows' pointer and pitch and returns a status.
    GPU inputs are read in place (one launch unless ``band_rows``); host inputs go through a ``BandSource`` each and the
    result through a ``BandSink``.  Returns the result, ``out`` when given."""
    first = inputs[0][0]
    dev = gpu_device(what, first)
    rows_out = int(out_shape[0])
    rowb = 1
    for v in out_shape[1:]:
        rowb *= int(v)
    with torch.no_grad():
        if first.is_cuda:
            step = min(band_rows or rows_out, rows_out)
            res = out if out is not None else torch.empty(tuple(out_shape), dtype=torch.uint8, device=dev)
            optr, opitch = gpu_rows(res)
            placed = [gpu_rows(t) for t, _ in inputs]
            for r0 in range(0, rows_out, step):
                n = min(step, rows_out - r0)
                views = []
                for (ptr, pitch), (_, need) in zip(placed, inputs):
                    s0, s1 = need(r0, n)
                    views.append((ptr + s0 * pitch, pitch, s0, s1 - s0))
                _native.check(launch(r0, n, views, optr + r0 * opitch, opitch), what)
            return res
        step = min(band_rows or host_band, rows_out)
        sources = []
        for t, need in inputs:
            most = max(need(r0, min(step, rows_out - r0))[1] - need(r0, min(step, rows_out - r0))[0]
                       for r0 in range(0, rows_out, step))
            sources.append(BandSource(t, most, dev))
        sink = BandSink(out_shape, step)
        band = torch.empty((step,) + tuple(out_shape[1:]), dtype=torch.uint8, device=dev)
        for r0 in range(0, rows_out, step):
            n = min(step, rows_out - r0)
            views = []
            for src, (_, need) in zip(sources, inputs):
                s0, s1 = need(r0, n)
                views.append(gpu_rows(src.rows(s0, s1)) + (s0, s1 - s0))
            _native.check(launch(r0, n, views, band.data_ptr(), rowb), what)
            sink.put(band, r0, r0 + n)
        res = sink.close()[0]
        if out is not None:
            out.copy_(res)
            return out
        return res


def _own_rows(r0: int, n: int) -> Tuple[int, int]:
    return r0, r0 + n


# ---- class and label overlays -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=257)
def _uniform_alpha(alpha: int) -> torch.Tensor:
    return torch.tensor([0] + [alpha] * 255, dtype=torch.int32)


def _fill_alpha(alpha: int, class_alpha, what: str) -> torch.Tensor:
    """The fill alpha table, int32 ``[256]``: a device tensor as it is (the kernel clamps its entries to 0..256), anything
    else checked and on the host."""
    if class_alpha is None:
        return _uniform_alpha(alpha)
    if isinstance(class_alpha, torch.Tensor) and class_alpha.is_cuda:
        if class_alpha.dtype != torch.int32 or tuple(class_alpha.shape) != (256,):
            raise ValueError(f"{what}: a device class_alpha must be int32 [256], got {class_alpha.dtype} "
                             f"{list(class_alpha.shape)}")
        return class_alpha
    if isinstance(class_alpha, torch.Tensor):
        if class_alpha.is_floating_point() or class_alpha.dtype == torch.bool or class_alpha.dim() != 1:
            raise ValueError(f"{what}: class_alpha must hold 256 integers, got {class_alpha.dtype} "
                             f"{list(class_alpha.shape)}")
        class_alpha = class_alpha.tolist()
    try:
        values = [operator.index(v) for v in class_alpha]
    except TypeError:
        raise TypeError(f"{what}: class_alpha must be None or 256 integers in 0..256") from None
    if len(values) != 256 or min(values) < 0 or max(values) > 256:
        raise ValueError(f"{what}: class_alpha must be 256 integers in 0..256, got {len(values)} in "
                         f"{min(values, default=0)}..{max(values, default=0)}")
    return torch.tensor(values, dtype=torch.int32)


def render_classes(region_u8: torch.Tensor, mask_or_labels: torch.Tensor, *, palette: Optional[torch.Tensor] = None,
                   alpha: int = 96, class_alpha=None, outline: int = 1, outline_alpha: int = 256,
                   outline_rgb: Optional[Sequence[int]] = None, out: Optional[torch.Tensor] = None,
                   band_rows: Optional[int] = None) -> torch.Tensor:
    """A class mask or a label image drawn over a uint8 ``[H, W, 3]`` region: every class or object tinted with its
    palette colour and outlined.

    ``mask_or_labels``: a uint8 class mask ``[H, W]`` (a bool mask is classes 0 and 1) or an int32 label image ``[H, W]``
    as ``label_components``, ``stain_objects(return_labels=True)`` and ``split_objects`` write them, on the region's
    device; row-strided views are read in place.  ``palette``: uint8 ``[256, 3]`` (``None``: ``default_palette()``).
    ``alpha`` in 0..256 tints every class but 0; ``class_alpha``, 256 integers in 0..256, sets the tint per colour index
    instead.  ``outline`` in 0..4 is the edge radius in pixels (city-block), ``outline_alpha`` its opacity,
    ``outline_rgb`` a fixed edge colour (``None``: the palette colour).  ``out``: the result's buffer, which may be the
    region itself (the layers of ``render_region`` after the first run in place) but must not overlap it in part.

    A GPU region is one launch (``band_rows`` rows per launch when given) and nothing waits for the device; a host
    region is streamed in bands of ``band_rows`` rows (``None``: 512), the mask with a halo of ``outline`` rows.  The
    result is on the input's device and its bytes depend neither on the banding nor on where the region lives."""
    what = "render_classes"
    H, W, _ = check_region(region_u8, what)
    m = mask_or_labels
    if not isinstance(m, torch.Tensor):
        raise TypeError(f"{what}: the mask must be a torch.Tensor, got {type(m).__name__}")
    if m.dtype not in (torch.uint8, torch.bool, torch.int32):
        raise ValueError(f"{what}: the mask must be uint8 or bool classes or int32 labels, got {m.dtype}")
    if tuple(m.shape) != (H, W):
        raise ValueError(f"{what}: the mask must be [{H}, {W}] like the region, got {list(m.shape)}")
    if W > 1 and m.stride(1) != 1:
        raise ValueError(f"{what}: the mask's pixels within a row must be contiguous")
    if W == 1 and m.stride(1) != 1:
        m = m.contiguous()                                    # a one-column view: its only stride is the row's
    alpha = _in_range(alpha, 0, 256, what, "alpha")
    r = _in_range(outline, 0, MAX_OUTLINE, what, "outline")
    edge_alpha = _in_range(outline_alpha, 0, 256, what, "outline_alpha")
    edge_rgb = -1
    if outline_rgb is not None:
        rgb = [operator.index(v) for v in outline_rgb]
        if len(rgb) != 3 or min(rgb) < 0 or max(rgb) > 255:
            raise ValueError(f"{what}: outline_rgb must be three integers in 0..255, got {rgb}")
        edge_rgb = (rgb[0] << 16) | (rgb[1] << 8) | rgb[2]
    band_rows = _check_band_rows(band_rows, what)
    _same_side(what, region_u8, m)
    if out is not None:
        _check_out(out, region_u8, what)
    pal = _check_table(_palette_host() if palette is None else palette, what, "palette")
    fa = _fill_alpha(alpha, class_alpha, what)
    dev = gpu_device(what, region_u8)
    pal, fa = _place_table(pal, dev, what, "palette"), _place_table(fa, dev, what, "class_alpha")
    L = ops._L()
    fn = L.s2s_render_labels_u8 if m.dtype == torch.int32 else L.s2s_render_classes_u8

    def halo(r0: int, n: int) -> Tuple[int, int]:
        return max(0, r0 - r), min(H, r0 + n + r)

    def launch(r0, n, views, optr, opitch):
        (bp, bpitch, _, _), (mp, mpitch, m0, mrows) = views
        return fn(bp, bpitch, mp, mpitch, m0, mrows, pal.data_ptr(), fa.data_ptr(), r, edge_alpha, edge_rgb, H, W, r0, n,
                  optr, opitch, ops._stream())

    return _run(what, [(region_u8, _own_rows), (_row_bytes(m), halo)], (H, W, 3), out, band_rows, DEFAULT_HOST_BAND,
                launch)


# ---- heat maps ------------------------------------------------------------------------------------------------------------
def quantize_map(values: torch.Tensor, lo: float = 0.0, hi: float = 1.0) -> torch.Tensor:
    """A real or integer map as the node values of ``render_heat``, int32 in 0..65280 on the map's device, in float64:
    ``q = clamp(floor((v - lo) (65280 / (hi - lo)) + 0.5), 0, 65280)``, NaN to 0.  Plain torch, no host wait."""
    scale = float(QMAX) / (float(hi) - float(lo))
    t = values.to(torch.float64) - float(lo)
    t = torch.floor(t * scale + 0.5)
    return torch.nan_to_num(t, nan=0.0).clamp(0.0, float(QMAX)).to(torch.int32)


def render_heat(region_u8: torch.Tensor, values: torch.Tensor, cell: int, *, lo: float = 0.0, hi: float = 1.0,
                lut="heat", alpha: int = 128, min_index: int = 0, smooth: bool = True, quantized: bool = False,
                out: Optional[torch.Tensor] = None, band_rows: Optional[int] = None) -> torch.Tensor:
    """A per-cell map drawn over a uint8 ``[H, W, 3]`` region through a colour table.

    ``values``: any real or integer ``[Gy, Gx]`` map with one value per ``cell`` x ``cell`` cell, such as
    ``region_stain_map``'s burden or ``region_qc_map``'s focus; Gy is ``H // cell`` or ``ceil(H / cell)`` and at least 1,
    Gx alike.  It is quantised on the device by ``quantize_map(values, lo, hi)``: ``lo`` maps to colour index 0 and
    ``hi`` to 255.  An int32 map passed with ``quantized=True`` goes to the kernel as it is (which clamps it to
    0..65280).  The map is tiny and always goes to the GPU whole.  ``lut``: ``"heat"``, ``"gray"``, ``"blue_red"`` or a
    uint8 ``[256, 3]`` table.  ``alpha`` in 0..256 is the opacity; pixels whose colour index lies below ``min_index``
    (0..256) keep the base.  ``smooth``: interpolate between the cell centres as ``warp_region`` interpolates its field,
    instead of one flat colour per cell.  ``out``, ``band_rows``, devices and banding as ``render_classes``."""
    what = "render_heat"
    H, W, _ = check_region(region_u8, what)
    if not isinstance(values, torch.Tensor):
        raise TypeError(f"{what}: values must be a torch.Tensor, got {type(values).__name__}")
    if values.dim() != 2 or values.dtype == torch.bool or values.is_complex():
        raise ValueError(f"{what}: values must be a real or integer [Gy, Gx] map, got {values.dtype} {list(values.shape)}")
    cell = operator.index(cell)
    if not 1 <= cell <= MAX_CELL:
        raise ValueError(f"{what}: cell must lie in 1..{MAX_CELL}, got {cell}")
    Gy, Gx = int(values.shape[0]), int(values.shape[1])
    for G, n, name in ((Gy, H, "Gy"), (Gx, W, "Gx")):
        if G < 1 or G not in (n // cell, -(-n // cell)):
            raise ValueError(f"{what}: {name} must be {n} // {cell} or ceil({n} / {cell}) and at least 1, got {G}")
    if Gy * Gx > MAX_NODES:
        raise ValueError(f"{what}: a map has at most {MAX_NODES} nodes, got {Gy} x {Gx}")
    if quantized:
        if values.dtype != torch.int32:
            raise ValueError(f"{what}: a quantized map must be int32, got {values.dtype}")
    else:
        lo, hi = float(lo), float(hi)
        if not hi > lo or hi - lo == float("inf"):
            raise ValueError(f"{what}: hi must be a finite number above lo, got lo {lo} and hi {hi}")
    alpha = _in_range(alpha, 0, 256, what, "alpha")
    min_index = _in_range(min_index, 0, 256, what, "min_index")
    band_rows = _check_band_rows(band_rows, what)
    if out is not None:
        _check_out(out, region_u8, what)
    table = _check_table(_colormap_host(lut) if isinstance(lut, str) else lut, what, "lut")
    dev = gpu_device(what, region_u8)
    if values.is_cuda and values.device != dev:
        raise ValueError(f"{what}: values must be on the host or on the region's device")
    table = _place_table(table, dev, what, "lut")
    with torch.no_grad():
        q = values.to(dev)
        q = (q if quantized else quantize_map(q, lo, hi)).contiguous()
    fn = ops._L().s2s_render_heat_u8

    def launch(r0, n, views, optr, opitch):
        bp, bpitch = views[0][:2]
        return fn(bp, bpitch, q.data_ptr(), Gy, Gx, cell, table.data_ptr(), alpha, min_index, 1 if smooth else 0, H, W,
                  r0, n, optr, opitch, ops._stream())

    return _run(what, [(region_u8, _own_rows)], (H, W, 3), out, band_rows, DEFAULT_HOST_BAND, launch)


# ---- comparison -------------------------------------------------------------------------------------------------------
def compare_regions(a_u8: torch.Tensor, b_u8: torch.Tensor, mode: str = "checker", *, cell: int = 64, alpha: int = 128,
                    gain: int = 4, band_rows: Optional[int] = None) -> torch.Tensor:
    """Two uint8 ``[H, W, 3]`` regions of one shape in one picture: whether ``register_region`` or ``align_regions``
    held, and where a generated stain differs from its target.  ``mode``: ``"checker"`` (``a`` where ``y // cell + x //
    cell`` is even, ``b`` elsewhere), ``"blend"`` (``mix(a, b, alpha)``) or ``"difference"`` (``min(255, |a - b| gain)``);
    ``cell`` at least 1, ``alpha`` in 0..256, ``gain`` in 1..255.  Devices and banding as ``render_classes``."""
    what = "compare_regions"
    H, W, _ = check_region(a_u8, what)
    if check_region(b_u8, what)[:2] != (H, W):
        raise ValueError(f"{what}: the regions must have one shape, got {list(a_u8.shape)} and {list(b_u8.shape)}")
    if mode not in COMPARE_MODES:
        raise ValueError(f"{what}: mode must be one of {COMPARE_MODES}, got {mode!r}")
    cell = _in_range(cell, 1, 1 << 30, what, "cell")
    alpha = _in_range(alpha, 0, 256, what, "alpha")
    gain = _in_range(gain, 1, 255, what, "gain")
    band_rows = _check_band_rows(band_rows, what)
    _same_side(what, a_u8, b_u8)
    fn, m = ops._L().s2s_render_compare_u8, COMPARE_MODES.index(mode)

    def launch(r0, n, views, optr, opitch):
        (ap, apitch, _, _), (bp, bpitch, _, _) = views
        return fn(ap, apitch, bp, bpitch, m, cell, alpha, gain, H, W, r0, n, optr, opitch, ops._stream())

    return _run(what, [(a_u8, _own_rows), (b_u8, _own_rows)], (H, W, 3), None, band_rows, DEFAULT_HOST_BAND, launch)


# ---- thumbnails -------------------------------------------------------------------------------------------------------
def downsample_region(region_u8: torch.Tensor, factor: int, *, band_rows: Optional[int] = None) -> torch.Tensor:
    """The thumbnail of a uint8 ``[H, W, 3]`` region or ``[H, W]`` mask: ``[ceil(H / factor), ceil(W / factor)]``, each
    pixel the rounded mean (for a mask the maximum) of the pixels of its ``factor`` x ``factor`` block that lie inside
    the region; ``factor`` in 1..256, 1 is a copy.  ``band_rows`` counts output rows (host default: 512 // factor, at
    least 1); devices and banding as ``render_classes``."""
    what = "downsample_region"
    H, W, C = check_region(region_u8, what, mask_ok=True)
    f = _in_range(factor, 1, MAX_FACTOR, what, "factor")
    band_rows = _check_band_rows(band_rows, what)
    Ho, Wo = -(-H // f), -(-W // f)
    fn = ops._L().s2s_box_down_u8

    def need(r0: int, n: int) -> Tuple[int, int]:
        return r0 * f, min(H, (r0 + n) * f)

    def launch(r0, n, views, optr, opitch):
        sp, spitch, s0, srows = views[0]
        return fn(sp, spitch, s0, srows, H, W, C, f, r0, n, optr, opitch, ops._stream())

    shape = (Ho, Wo, 3) if C == 3 else (Ho, Wo)
    return _run(what, [(region_u8, need)], shape, None, band_rows, max(1, DEFAULT_HOST_BAND // f), launch)


# ---- composition ------------------------------------------------------------------------------------------------------
def render_region(region_u8: torch.Tensor, layers: Sequence[tuple], *, band_rows: Optional[int] = None) -> torch.Tensor:
    """Several layers over one region: ``layers`` is a list of ``("classes", mask_or_labels, {options})`` and ``("heat",
    values, cell, {options})`` entries (the options of ``render_classes`` and ``render_heat``; the dict may be left
    out), applied in order.  The first writes a fresh result and the rest run in place on it, so the region itself is
    never written.  One launch per layer for a GPU region."""
    what = "render_region"
    check_region(region_u8, what)
    band_rows = _check_band_rows(band_rows, what)
    layers = list(layers)
    if not layers:
        raise ValueError(f"{what}: at least one layer is needed")
    calls: List[tuple] = []
    for i, layer in enumerate(layers):
        if not isinstance(layer, (tuple, list)) or not layer or layer[0] not in ("classes", "heat"):
            raise ValueError(f"{what}: layer {i} must be ('classes', mask, {{...}}) or ('heat', values, cell, {{...}})")
        nargs = 1 if layer[0] == "classes" else 2
        if len(layer) not in (1 + nargs, 2 + nargs):
            raise ValueError(f"{what}: layer {i} ({layer[0]!r}) takes {nargs} argument(s) and an optional dict of options")
        opts = dict(layer[1 + nargs]) if len(layer) == 2 + nargs else {}
        if "out" in opts or "band_rows" in opts:
            raise ValueError(f"{what}: layer {i} must not set out or band_rows")
        calls.append((render_classes if layer[0] == "classes" else render_heat, tuple(layer[1:1 + nargs]), opts))
    res = None
    for fn, args, opts in calls:
        res = fn(region_u8 if res is None else res, *args, out=res, band_rows=band_rows, **opts)
    return res


def compose_panels(images: Sequence[torch.Tensor], *, cols: Optional[int] = None, gap: int = 8,
                   fill: int = 255) -> torch.Tensor:
    """Equally shaped uint8 images (``[H, W, 3]`` or ``[H, W]``) tiled into one, row by row with ``cols`` images per row
    (``None``: all in one row), ``gap`` pixels of ``fill`` between them and in the cells left over: the source /
    generated / target figure.  Plain torch copies on the images' device."""
    what = "compose_panels"
    images = list(images)
    if not images:
        raise ValueError(f"{what}: at least one image is needed")
    for im in images:
        if not isinstance(im, torch.Tensor):
            raise TypeError(f"{what}: every image must be a torch.Tensor, got {type(im).__name__}")
    first = images[0]
    if first.dtype != torch.uint8 or not (first.dim() == 2 or (first.dim() == 3 and first.shape[2] == 3)) \
            or min(first.shape) < 1:
        raise ValueError(f"{what}: an image must be a non-empty uint8 [H, W, 3] or [H, W], got {first.dtype} "
                         f"{list(first.shape)}")
    for im in images[1:]:
        if im.dtype != first.dtype or im.shape != first.shape or im.device != first.device:
            raise ValueError(f"{what}: the images must share dtype, shape and device, got {list(im.shape)} on {im.device} "
                             f"beside {list(first.shape)} on {first.device}")
    n = len(images)
    cols = n if cols is None else _in_range(cols, 1, 1 << 20, what, "cols")
    gap = _in_range(gap, 0, 1 << 20, what, "gap")
    fill = _in_range(fill, 0, 255, what, "fill")
    rows = -(-n // cols)
    cols = min(cols, n)
    H, W = int(first.shape[0]), int(first.shape[1])
    shape = (rows * H + (rows - 1) * gap, cols * W + (cols - 1) * gap) + tuple(first.shape[2:])
    out = torch.full(shape, fill, dtype=torch.uint8, device=first.device)
    for i, im in enumerate(images):
        y, x = (i // cols) * (H + gap), (i % cols) * (W + gap)
        out[y:y + H, x:x + W] = im
    return out
