"""Tiled whole-region stain translation: a uint8 RGB region of any size in, the translated uint8 region out.

The region is cut into overlapping ``tile`` x ``tile`` tiles (``plan_tiles``), the tiles run through a sampler in
batches of a fixed size, and the tile outputs are blended with a feathered window, so tile borders leave no seams.
Everything between two sampler calls is HIP (``csrc/region.hip``): tile gather and normalisation, weighted
accumulation into a ring of image rows, and finalisation (division by the weight sum, the reference's uint8 save
conversion, clearing the ring).  DESIGN.md section 3.11.

The reference's inference scripts (src/infer_simple_flowmatching.py, notebooks/infer_any2any.ipynb) translate one
image at a time at batch 1; ``translate_region`` is the loop around them.
"""
from __future__ import annotations

import operator
import types
from typing import Callable, Dict, List, Optional

import torch

from . import ops
from ._regionio import BandSink, BandSource, check_region, gpu_device


def _axis_origins(L: int, tile: int, overlap: int) -> List[int]:
    if L <= tile:
        return [0]
    S = tile - overlap
    n = -(-(L - tile) // S) + 1
    return [min(i * S, L - tile) for i in range(n)]


def plan_tiles(H: int, W: int, tile: int, overlap: int) -> torch.Tensor:
    """Tile origins ``(top, left)`` as int32 [N, 2], row-major (every tile of the first tile row, then the next row).

    Each axis of length L is planned alone with stride S = tile - overlap: one origin 0 when L <= tile, otherwise
    n = ceil((L - tile) / S) + 1 origins min(i * S, L - tile), the last tile flush with the edge.  The network's own
    constraint on the tile size (a multiple of 2^(levels-1)) is not checked here."""
    H, W, tile, overlap = (operator.index(v) for v in (H, W, tile, overlap))
    if tile < 1:
        raise ValueError(f"tile must be >= 1, got {tile}")
    if overlap < 0 or overlap >= tile:
        raise ValueError(f"overlap must lie in [0, tile), got {overlap} with tile {tile}")
    if H < 1 or W < 1:
        raise ValueError(f"region must be at least 1 x 1, got {H} x {W}")
    ys, xs = _axis_origins(H, tile, overlap), _axis_origins(W, tile, overlap)
    return torch.tensor([[y, x] for y in ys for x in xs], dtype=torch.int32).reshape(-1, 2)


def band_rows_for(H: int, W: int, tile: int, overlap: int, batch: int) -> int:
    """Rows of the accumulator ring: the rows the tiles of one batch can span -- ``batch`` consecutive plan entries
    touch at most k tile rows, whose origins lie within (k - 1) * stride -- plus one tile height.  Independent of H
    once the region has k tile rows."""
    n_rows, n_cols = len(_axis_origins(H, tile, overlap)), len(_axis_origins(W, tile, overlap))
    k = min(n_rows, (batch + n_cols - 2) // n_cols + 1)
    return min(H, (k - 1) * (tile - overlap) + tile)


def _check_output(out, batch: int, tile: int, device: torch.device, what: str, channels=None) -> torch.Tensor:
    if not isinstance(out, torch.Tensor):
        raise TypeError(f"translate_region: sampler {what} must be a tensor, got {type(out).__name__}")
    if out.dtype != torch.float32 or out.device != device:
        raise ValueError(f"translate_region: sampler {what} must be fp32 on {device}, got {out.dtype} on {out.device}")
    ok_c = out.dim() == 4 and (out.shape[1] == 3 if channels is None else 1 <= out.shape[1] <= channels)
    if not ok_c or tuple(out.shape[:1]) + tuple(out.shape[2:]) != (batch, tile, tile):
        want = f"[{batch}, 3, {tile}, {tile}]" if channels is None else f"[{batch}, 1..{channels}, {tile}, {tile}]"
        raise ValueError(f"translate_region: sampler {what} must have shape {want}, got {list(out.shape)}")
    return out.contiguous()


@torch.no_grad()
def translate_region(image: torch.Tensor, sampler: Callable, *, tile: int = 256, overlap: int = 32, batch: int = 32,
                     return_float: bool = False, min_tissue: Optional[float] = None,
                     keep: Optional[torch.Tensor] = None, white: int = 220, black: int = 0,
                     mask_channels: Optional[int] = None):
    """Translate a whole uint8 RGB region tile by tile and blend the tiles without seams.

    ``image``: uint8 [H, W, 3] on the GPU or the host, any row pitch (a crop view of a larger slide array works without
    a copy), pixels contiguous within a row.  ``sampler``: called with fp32 [batch, 3, tile, tile] on the GPU (the
    normalised tiles, ``(u / 255 - 0.5) / 0.5``); returns fp32 [batch, 3, tile, tile] or a tuple (image, probabilities
    [batch, Cm, tile, tile]) with Cm <= 5.  For a ``FlowUNet``: ``lambda x: euler_generate(net, x, 50, graph=True)``;
    for ``MultiTaskFlowMatchingModule``: ``multitask_sampler(module, 50)``.  A higher-order fixed-step scheme with fewer
    evaluations: ``lambda x: fixed_step_generate(net, x, 6, "rk4", graph=True)``.  The reference's adaptive solver, one step size
    per tile: ``lambda x: dopri5_generate(net, x, per_sample=True, graph=True)`` or
    ``multitask_sampler(module, 1, method="dopri5")``.

    Every sampler call gets exactly ``batch`` tiles (a short last batch is padded by repeating its last tile, the padded
    outputs are discarded), so a captured-graph sampler is captured once per region.  The tile outputs are weighted by
    a separable window ramping over ``overlap`` pixels at every tile edge and normalised by the weight sum; with a
    fixed-step (Euler) sampler or per-sample dopri5 (``per_sample=True``) each tile's result is independent of its
    batch mates; with the batch-wide dopri5 (the default ``per_sample=False``) it is not (its step control uses one
    error norm over the whole batch).

    Returns the uint8 [H, W, 3] region on the input's device (the reference's save conversion of the blended image,
    ``trunc(clamp((x * 0.5 + 0.5) * 255, 0, 255))``).  With a tuple-returning sampler the result is a tuple that also
    holds the blended probabilities, fp32 [H, W, Cm] (class maps do not blend: take the argmax of these); with
    ``return_float`` it also holds the blended fp32 image [H, W, 3], last.  Both are views of one [H, W, 3 + Cm] buffer.

    Working memory on the GPU does not grow with H: the accumulator ring holds ``band_rows`` image rows, and a host
    image is staged in and out through one pinned buffer of that height per direction.  ``translate_region.last_stats``
    describes the last call: tiles, batches, band_rows, accumulator_bytes, channels, kept, skipped, sampler_calls.

    Background tiles can skip the sampler.  ``min_tissue``: a fraction in [0, 1]; tile n is kept
    iff ``counts[n] >= min_tissue * areas[n]`` with ``tissue_counts(image, tile, overlap, white=white, black=black)``
    (a pixel is tissue iff ``min(R, G, B) < white and max(R, G, B) >= black``); the counts are copied to the host once.
    ``keep``: the caller's own bool [N] mask in plan order instead (from a thumbnail, say); the two exclude each other,
    and with both None nothing is skipped.  The kept tiles are compacted into sampler calls of exactly ``batch`` tiles
    (``plan_region_batches``); a pixel no kept tile covers is the source pixel, its bytes copied (and probability 0);
    where kept and skipped tiles overlap, the skipped ones enter the blend as the normalised source, so there are no
    seams.  The output channels must then be known before the first sampler call: ``mask_channels`` is the sampler's
    number of probability channels (default: its ``mask_channels`` attribute, which ``multitask_sampler`` sets, else 0)."""
    H, W, _ = check_region(image, "translate_region")
    batch = operator.index(batch)
    if batch < 1:
        raise ValueError(f"batch must be >= 1, got {batch}")
    plan = plan_tiles(H, W, tile, overlap)
    if tile % 4:
        raise ValueError(f"tile must be a multiple of 4, got {tile}")
    skipping = min_tissue is not None or keep is not None
    C = None                                              # output channels: the first sampler call tells
    if skipping:
        if min_tissue is not None and keep is not None:
            raise ValueError("translate_region: keep and min_tissue exclude each other")
        white, black = _check_thresholds(white, black)
        if min_tissue is not None:
            min_tissue = float(min_tissue)
            if not 0.0 <= min_tissue <= 1.0:
                raise ValueError(f"translate_region: min_tissue must lie in [0, 1], got {min_tissue}")
        if mask_channels is None:
            mask_channels = getattr(sampler, "mask_channels", 0)
        C = 3 + operator.index(mask_channels)             # a range without kept tiles is finalised before any call
        if not 3 <= C <= 8:
            raise ValueError(f"translate_region: mask_channels must lie in 0..5, got {C - 3}")
    N = plan.shape[0]
    on_gpu = image.is_cuda
    dev = gpu_device("translate_region", image)
    band_rows = band_rows_for(H, W, tile, overlap, batch)
    source = BandSource(image, band_rows, dev)
    tops = plan[:, 0].tolist()
    if min_tissue is not None:
        counts = _count_tissue(source, plan, plan.to(dev), tile, white, black, dev).tolist()
        if min(counts) < 0:                               # .tolist(): the one host synchronisation skipping adds
            raise RuntimeError("translate_region: a tile was counted outside its band")
        keep = torch.tensor([c >= min_tissue * a for c, a in zip(counts, _tile_areas(plan, H, W, tile).tolist())],
                            dtype=torch.bool)
    elif isinstance(keep, torch.Tensor):
        keep = keep.cpu()
    if skipping:
        ranges = plan_region_batches(plan, keep, batch, band_rows, tile)
        kept = keep.tolist()
    else:
        ranges = [(p0, min(p0 + batch, N)) for p0 in range(0, N, batch)]
        kept = [True] * N
    # one upload: per range its kept origins, padded to `batch` by repeating the last one, then its skipped origins
    rows, layout = [], []
    for p0, p1 in ranges:
        ks = [p for p in range(p0, p1) if kept[p]]
        ss = [p for p in range(p0, p1) if not kept[p]]
        ko = len(rows)
        if ks:
            rows += ks + [ks[-1]] * (batch - len(ks))
        layout.append((len(ks), len(ss), ko, len(rows)))
        rows += ss
    origins = plan[rows].contiguous().to(dev)
    n_kept = sum(kept)
    x = torch.empty((batch, 3, tile, tile), dtype=torch.float32, device=dev) if n_kept else None
    ws = torch.zeros((band_rows, W), dtype=torch.float32, device=dev) if skipping else None
    acc = out_u8 = out_f = sink = None
    if C is not None:
        acc, out_u8, out_f, sink = _result_buffers(H, W, C, band_rows, return_float, on_gpu, dev)
    fin = 0                                               # rows [0, fin) are final; fin is the range's first top
    calls = 0
    for (p0, p1), (nk, ns, ko, so) in zip(ranges, layout):
        r0, r1 = tops[p0], min(H, tops[p1 - 1] + tile)
        done = tops[p1] if p1 < N else H                  # no later tile covers rows above the next range's first top
        if on_gpu:
            src, src_top = image, 0
        else:
            rs = r1 if nk else done                       # without kept tiles only the rows to finalise are read
            src, src_top = source.rows(r0, rs) if rs > r0 else None, r0
        if ns:
            ops.region_skip_weight(origins[so:so + ns], tile, overlap, ws, H, r0, r1)
        if nk:
            ops.region_gather(src, src_top, H, W, origins[ko:ko + batch], tile, x)
            out = sampler(x)
            calls += 1
            probs = None
            if isinstance(out, tuple):
                if len(out) != 2:
                    raise ValueError(f"translate_region: a tuple from the sampler must be (image, probabilities), "
                                     f"got {len(out)} items")
                out, probs = out
                probs = _check_output(probs, batch, tile, dev, "probabilities", channels=5)
            out = _check_output(out, batch, tile, dev, "image")
            c_now = 3 + (0 if probs is None else probs.shape[1])
            if acc is None:
                C = c_now
                acc, out_u8, out_f, sink = _result_buffers(H, W, C, band_rows, return_float, on_gpu, dev)
            elif c_now != C:
                raise ValueError(f"translate_region: the sampler changed its output channels: {C - 3} probability "
                                 f"channels were expected (mask_channels, or its first call), it returned {c_now - 3}")
            ops.region_blend(out[:nk], None if probs is None else probs[:nk], origins[ko:ko + nk], overlap, acc,
                             band_rows, H, W, r0, r1)
        if done > fin:
            out_top = 0 if on_gpu else fin                # a host result leaves through the band buffers' first rows
            if skipping:
                ops.region_finalize_mixed(acc, ws, fin, done, src, src_top, out_u8, out_f, out_top)
            else:
                ops.region_finalize(acc, fin, done, out_u8, out_f, out_top)
            if sink is not None:
                sink.put(out_u8, fin, done, out_f)
            fin = done
    res_u8, res_f = (out_u8, out_f) if on_gpu else sink.close()
    translate_region.last_stats = {"tiles": N, "batches": len(ranges), "band_rows": band_rows,
                                   "accumulator_bytes": (acc.numel() + (ws.numel() if skipping else 0)) * 4,
                                   "channels": C, "kept": n_kept, "skipped": N - n_kept, "sampler_calls": calls}
    extra = []
    if C > 3:
        extra.append(res_f[..., 3:])
    if return_float:
        extra.append(res_f[..., :3])
    return (res_u8, *extra) if extra else res_u8


def _result_buffers(H: int, W: int, C: int, band_rows: int, return_float: bool, on_gpu: bool, dev):
    """(accumulator ring, uint8 and fp32 rows the finalize writes, sink): for a GPU image the rows are the whole result
    and there is no sink; for a host image they are band buffers that a ``BandSink`` empties."""
    acc = torch.zeros((band_rows, W, C + 1), dtype=torch.float32, device=dev)
    want_f = return_float or C > 3
    rows = H if on_gpu else band_rows
    out_u8 = torch.empty((rows, W, 3), dtype=torch.uint8, device=dev)
    out_f = torch.empty((rows, W, C), dtype=torch.float32, device=dev) if want_f else None
    sink = None if on_gpu else BandSink((H, W, 3), band_rows, C if want_f else None)
    return acc, out_u8, out_f, sink


translate_region.last_stats: Optional[Dict[str, int]] = None


# ---- tissue-aware regions: background tiles skip the sampler --------------------------------
def _check_thresholds(white, black):
    white, black = operator.index(white), operator.index(black)
    if not 1 <= white <= 256:
        raise ValueError(f"white must lie in 1..256, got {white}")
    if not 0 <= black <= 255:
        raise ValueError(f"black must lie in 0..255, got {black}")
    return white, black


def _count_tissue(source: BandSource, plan, origins, tile, white, black, dev):
    """int32 [N] tissue counts on the GPU.  A GPU image takes one launch; a host image streams once through ``source``
    (at least min(H, tile) rows), one tile row of the plan per band."""
    H, W = int(source.img.shape[0]), int(source.img.shape[1])
    N = plan.shape[0]
    counts = torch.empty((N,), dtype=torch.int32, device=dev)
    if source.on_gpu:
        ops.region_tissue_count(source.img, 0, H, W, origins[:N], tile, white, black, counts)
        return counts
    tops = plan[:, 0].tolist()
    p0 = 0
    while p0 < N:
        p1 = p0 + 1
        while p1 < N and tops[p1] == tops[p0]:
            p1 += 1
        r0, r1 = tops[p0], min(H, tops[p0] + tile)
        ops.region_tissue_count(source.rows(r0, r1), r0, H, W, origins[p0:p1], tile, white, black, counts[p0:p1])
        p0 = p1
    return counts


def _tile_areas(plan: torch.Tensor, H: int, W: int, tile: int) -> torch.Tensor:
    return ((plan[:, 0] + tile).clamp(max=H) - plan[:, 0]) * ((plan[:, 1] + tile).clamp(max=W) - plan[:, 1])


@torch.no_grad()
def tissue_counts(image: torch.Tensor, tile: int = 256, overlap: int = 32, *, white: int = 220, black: int = 0):
    """Tissue pixels per tile of ``plan_tiles(H, W, tile, overlap)``: (counts int32 [N] on the GPU, areas int32 [N] on
    the host).  A pixel is tissue iff ``min(R, G, B) < white and max(R, G, B) >= black`` (integer, exact); ``white`` in
    1..256, ``black`` in 0..255, 0 disabling the dark test.  A tile's area is its intersection with the image: the
    reflected padding of a region smaller than a tile is not counted.  ``image`` as for ``translate_region``; a host
    image is streamed once through a pinned buffer, one tile row of the plan per band."""
    H, W, _ = check_region(image, "tissue_counts")
    white, black = _check_thresholds(white, black)
    plan = plan_tiles(H, W, tile, overlap)
    dev = gpu_device("tissue_counts", image)
    source = BandSource(image, min(H, operator.index(tile)), dev)
    return _count_tissue(source, plan, plan.to(dev), tile, white, black, dev), _tile_areas(plan, H, W, tile)


def plan_region_batches(plan: torch.Tensor, keep: torch.Tensor, batch: int, band_rows: int, tile: int):
    """Cut the plan into contiguous ranges ``[p0, p1)`` for a region whose tiles with ``keep[n]`` false skip the
    sampler: a list of (p0, p1) that partitions [0, N) in order.  Greedy: each range is the longest that holds at most
    ``batch`` kept tiles and spans at most ``band_rows`` image rows, ``tops[p1 - 1] + tile - tops[p0] <= band_rows``, so
    it fits the accumulator ring.  (Tiles of the first tile's own row always fit: they span the same rows, which matters
    only for a region lower than a tile, where ``band_rows`` = H < tile.)  With ``keep`` all true the ranges are the
    fixed ``batch``-sized slices, whose span ``band_rows_for`` bounds.  Host only."""
    batch, band_rows, tile = operator.index(batch), operator.index(band_rows), operator.index(tile)
    if batch < 1:
        raise ValueError(f"batch must be >= 1, got {batch}")
    if band_rows < 1 or tile < 1:
        raise ValueError(f"band_rows and tile must be >= 1, got {band_rows} and {tile}")
    if not isinstance(plan, torch.Tensor) or plan.dim() != 2 or plan.shape[1] != 2:
        raise ValueError("plan must be the [N, 2] tensor of plan_tiles")
    N = plan.shape[0]
    if not isinstance(keep, torch.Tensor):
        raise TypeError(f"keep must be a bool tensor, got {type(keep).__name__}")
    if keep.dtype != torch.bool:
        raise ValueError(f"keep must be a bool tensor, got {keep.dtype}")
    if tuple(keep.shape) != (N,):
        raise ValueError(f"keep must have shape [{N}] (one entry per tile, plan order), got {list(keep.shape)}")
    tops, kept = plan[:, 0].tolist(), keep.tolist()
    ranges = []
    p0 = 0
    while p0 < N:
        p1, nk = p0 + 1, int(kept[p0])
        while (p1 < N and nk + kept[p1] <= batch
               and (tops[p1] == tops[p0] or tops[p1] + tile - tops[p0] <= band_rows)):
            nk += kept[p1]
            p1 += 1
        ranges.append((p0, p1))
        p0 = p1
    return ranges


def multitask_sampler(module, num_steps: int, graph: bool = True, *, method: str = "euler", atol: float = 1e-4,
                      rtol: float = 1e-4) -> Callable:
    """Sampler for ``translate_region`` from a ``MultiTaskFlowMatchingModule``: (the ``num_steps``-step Euler image,
    the mask head's probabilities on the source tiles -- sigmoid(logits) for the binary head, softmax(logits) over the
    classes for the multiclass one).  Class maps cannot be blended; take the argmax of the blended probabilities.
    ``graph``: one captured Euler step replayed ``num_steps`` times, captured once per batch shape (and again after the
    module's parameters change).  The module is put in eval mode, as its ``generate`` does.
    ``method="dopri5"``: the reference's adaptive solver at ``atol`` / ``rtol`` instead, with a step size per tile
    (``dopri5_integrate(..., per_sample=True)``), so every tile is independent of its batch mates; ``graph`` then
    captures one whole attempted step; ``num_steps`` plays no role.  ``method`` "midpoint", "heun", "rk4" or "rk4_38":
    ``num_steps`` steps of that fixed-step Runge-Kutta scheme (``fixed_step_integrate``); ``graph`` then captures one
    whole step (its evaluations, stage launches and combine)."""
    from .samplers import SOLVER_METHODS, _prep_source, solve
    num_steps = operator.index(num_steps)
    if method not in SOLVER_METHODS:
        raise ValueError(f"method must be one of {', '.join(map(repr, SOLVER_METHODS))}, got {method!r}")
    if num_steps < 1:
        raise ValueError(f"num_steps must be >= 1, got {num_steps}")
    flow = module.forward_flow                            # one bound method: the network a kept capture is matched on
    captures = types.SimpleNamespace()                    # this closure's capture lives here, not on the module

    def sample(x: torch.Tensor):
        module.eval()
        logits = module.forward_segmentation(x)
        probs = torch.softmax(logits, dim=1) if module.num_classes is not None else torch.sigmoid(logits)
        return solve(flow, _prep_source(x), method, num_steps, atol, rtol, graph=graph,
                     per_sample=method == "dopri5", cache_on=captures), probs.float()

    sample.mask_channels = 1 if module.num_classes is None else int(module.num_classes)   # translate_region's layout
    return sample
