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
                     return_float: bool = False):
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
    describes the last call: tiles, batches, band_rows, accumulator_bytes, channels."""
    if not isinstance(image, torch.Tensor):
        raise TypeError(f"translate_region: image must be a torch.Tensor, got {type(image).__name__}")
    if image.dtype != torch.uint8:
        raise ValueError(f"translate_region: image must be uint8, got {image.dtype}")
    if image.dim() != 3 or image.shape[2] != 3:
        raise ValueError(f"translate_region: image must be [H, W, 3] RGB, got {list(image.shape)}")
    H, W = int(image.shape[0]), int(image.shape[1])
    if image.stride(2) != 1 or (W > 1 and image.stride(1) != 3):
        raise ValueError("translate_region: pixels within a row must be contiguous")
    batch = operator.index(batch)
    if batch < 1:
        raise ValueError(f"batch must be >= 1, got {batch}")
    plan = plan_tiles(H, W, tile, overlap)
    if tile % 4:
        raise ValueError(f"tile must be a multiple of 4, got {tile}")
    on_gpu = image.is_cuda
    dev = image.device if on_gpu else torch.device("cuda", torch.cuda.current_device())
    N = plan.shape[0]
    nb = -(-N // batch)
    padded = torch.cat([plan, plan[-1:].expand(nb * batch - N, 2)]) if nb * batch > N else plan
    tops = plan[:, 0].tolist()
    origins = padded.to(dev)                              # one upload; a batch is a slice
    band_rows = band_rows_for(H, W, tile, overlap, batch)
    x = torch.empty((batch, 3, tile, tile), dtype=torch.float32, device=dev)
    if not on_gpu:
        stage_in = torch.empty((band_rows, W, 3), dtype=torch.uint8, pin_memory=True)
        band_in = torch.empty((band_rows, W, 3), dtype=torch.uint8, device=dev)
        in_ready = None                                   # the GPU's last read of stage_in
    acc = out_u8 = out_f = None
    C = Cm = 0
    fin = 0                                               # rows [0, fin) are final
    pending = None                                        # host output rows in flight: (event, r0, r1)

    def drain():                                          # host image: staged output rows -> the result
        ev, a, b = pending
        ev.synchronize()
        res_u8[a:b] = stage_u8[:b - a]
        if res_f is not None:
            res_f[a:b] = stage_f[:b - a]

    for bi in range(nb):
        p0, pn = bi * batch, min(batch, N - bi * batch)
        r0, r1 = tops[p0], min(H, tops[p0 + pn - 1] + tile)
        if on_gpu:
            ops.region_gather(image, 0, H, W, origins[p0:p0 + batch], tile, x)
        else:
            if in_ready is not None:
                in_ready.synchronize()                    # the previous upload has left stage_in
            stage_in[:r1 - r0].copy_(image[r0:r1])
            band_in[:r1 - r0].copy_(stage_in[:r1 - r0], non_blocking=True)
            in_ready = torch.cuda.Event()
            in_ready.record()
            ops.region_gather(band_in[:r1 - r0], r0, H, W, origins[p0:p0 + batch], tile, x)
        out = sampler(x)
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
            C, Cm = c_now, c_now - 3
            acc = torch.zeros((band_rows, W, C + 1), dtype=torch.float32, device=dev)
            want_f = return_float or Cm > 0
            if on_gpu:
                res_u8 = out_u8 = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
                res_f = out_f = torch.empty((H, W, C), dtype=torch.float32, device=dev) if want_f else None
            else:
                res_u8 = torch.empty((H, W, 3), dtype=torch.uint8)
                res_f = torch.empty((H, W, C), dtype=torch.float32) if want_f else None
                out_u8 = torch.empty((band_rows, W, 3), dtype=torch.uint8, device=dev)
                out_f = torch.empty((band_rows, W, C), dtype=torch.float32, device=dev) if want_f else None
                stage_u8 = torch.empty((band_rows, W, 3), dtype=torch.uint8, pin_memory=True)
                stage_f = torch.empty((band_rows, W, C), dtype=torch.float32, pin_memory=True) if want_f else None
        elif c_now != C:
            raise ValueError("translate_region: the sampler changed its output channels between calls")
        ops.region_blend(out[:pn], None if probs is None else probs[:pn], origins[p0:p0 + pn], overlap, acc,
                         band_rows, H, W, r0, r1)
        done = tops[p0 + pn] if bi + 1 < nb else H        # no later tile covers rows above the next tile's top
        if done > fin:
            if on_gpu:
                ops.region_finalize(acc, fin, done, out_u8, out_f, 0)
            else:
                ops.region_finalize(acc, fin, done, out_u8, out_f, fin)
                if pending is not None:
                    drain()                               # stage_u8 / stage_f are free again
                n = done - fin
                stage_u8[:n].copy_(out_u8[:n], non_blocking=True)
                if out_f is not None:
                    stage_f[:n].copy_(out_f[:n], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                pending = (ev, fin, done)
            fin = done
    if pending is not None:
        drain()
    translate_region.last_stats = {"tiles": N, "batches": nb, "band_rows": band_rows,
                                   "accumulator_bytes": acc.numel() * acc.element_size(), "channels": C}
    extra = []
    if Cm:
        extra.append(res_f[..., 3:])
    if return_float:
        extra.append(res_f[..., :3])
    return (res_u8, *extra) if extra else res_u8


translate_region.last_stats: Optional[Dict[str, int]] = None


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

    return sample
