"""Case tables and float64 references for the weight-gradient kernels of the CFM / multitask step, form by form (a helper
module of the suite, not a conftest; no HIP calls in here):

  * the 3x3 weight gradient (ops.conv3x3_wgrad): one row per launch form -- tile walks of 1, 2 ... 6 tiles per split, even
    and uneven, both workgroup orders, both folds and the edge of the fold choice, one and two sources, channel tails;
  * the stem weight / bias gradient (ops.stem_wgrad): more tiles than workgroups, two channel groups, Cout tails;
  * the 1x1 head (ops.head_fwd / ops.head_bwd): every lanes-per-pixel instantiation, both one-thread-per-pixel fallbacks,
    the block cap of the backward, the refused shapes.

The plans in the tables are those of the library with no switch set; tests/test_wgrad_forms_cpu.py holds the library's
plan queries to them and to the list of forms the tables must contain.

References are float64 on the operands exactly as the kernel reads them (bf16 mode: rounded to bf16; fp32 mode: as
given).  Every reference comes with its YARDSTICK: the deviation from float64, in the max norm and in L2, of the same
quantity computed by torch on the CPU in float32 -- what plain fp32 accumulation costs at that shape, from the reference
side alone.  References are cached: computed once per (row, dtype) and shared by the tests; treat them as read-only."""
from __future__ import annotations

import functools
from typing import Dict, List, Optional, Tuple

import torch

import stepwise_ref as SR

BF = torch.bfloat16
YARD_FLOOR = 1e-7          # one_pixel: nine single products, which fp32 gets exactly

# ---------------------------------------------------------------------------------------------------------------------
# 3x3 weight gradient.  name: (B, H, W, c0, c1, Cout), then the bf16 plan with no switch set: splits, 8x16 pixel tiles,
# XCD-aware order, waves per fold group.  (The fp32 kernel has the same splits, tiles and fold and no XCD-aware order.)
# ---------------------------------------------------------------------------------------------------------------------
CONV3X3: Dict[str, Tuple[Tuple[int, ...], Tuple[int, int, int, int]]] = {
    "walk3_64x64":   ((6, 90, 120, 64, 0, 64), (256, 576, 1, 16)),      # 2 / 3 tiles a split
    "walk3_128":     ((2, 75, 100, 128, 0, 128), (64, 140, 1, 16)),     # 2 / 3
    "two_src_tails": ((3, 43, 70, 96, 40, 136), (28, 90, 0, 4)),        # 3 / 4, the ci tile 64..127 spans both sources
    "one_tile_each": ((2, 50, 90, 64, 128, 64), (84, 84, 0, 16)),       # 1, fold 16 with 84 % 16 != 0
    "even_walk3":    ((1, 70, 110, 192, 0, 200), (21, 63, 0, 4)),       # 3 each, fold 4 with 21 % 4 != 0
    "wide":          ((2, 33, 49, 256, 0, 320), (12, 40, 1, 4)),        # 3 / 4
    "tiny_maps":     ((40, 7, 15, 64, 0, 64), (40, 40, 1, 16)),         # H < 8 and W < 16: no interior tile
    "c8":            ((1, 130, 150, 8, 0, 8), (170, 170, 0, 16)),
    "deep":          ((1, 24, 48, 512, 0, 512), (4, 9, 1, 4)),          # 2 / 3
    "half_ci_tile":  ((2, 40, 60, 24, 8, 520), (28, 40, 0, 4)),         # 1 / 2, both sources inside half a ci tile
    "one_split":     ((1, 24, 32, 1024, 0, 1024), (1, 6, 1, 4)),        # one workgroup column walks all 6 tiles
    "two_splits":    ((1, 20, 40, 1536, 0, 512), (2, 9, 1, 4)),         # 4 / 5
    "one_row":       ((3, 1, 200, 16, 0, 64), (39, 39, 0, 16)),
    "one_pixel":     ((1, 1, 1, 8, 0, 8), (1, 1, 0, 4)),
    "fold_edge":     ((2, 75, 100, 128, 0, 256), (32, 140, 1, 16)),     # Cout Cin == 32768 and S == 32: the last fold 16
    "fold_above":    ((2, 75, 100, 136, 0, 256), (21, 140, 0, 4)),      # the nearest shape above it
}
FOLD_LIMIT = 32768         # wgrad_reduce_kernel<16> for Cout Cin <= this and S >= 32


def conv3x3_walks(name: str, splits: Optional[int] = None) -> List[List[bool]]:
    """Per split, the tiles it walks (tile z, z + S, ...), each as "is interior" (the whole 10 x 18 halo inside the image:
    conv3x3_wgrad_dma_kernel's path without per-lane bounds tests)."""
    (B, H, W, _, _, _), (S, tiles, _, _) = CONV3X3[name]
    S = splits or S
    ty, tx = -(-H // 8), -(-W // 16)
    assert tiles == B * ty * tx
    out = []
    for z in range(S):
        walk = []
        for t in range(z, tiles, S):
            y0, x0 = (t // tx) % ty * 8, (t % tx) * 16
            walk.append(y0 >= 1 and y0 + 9 <= H and x0 >= 1 and x0 + 17 <= W)
        out.append(walk)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# stem weight / bias gradient: (B, H, W, Cin, Cout), then 16x16 tiles, workgroups (s2s_stem_wgrad_blocks), slabs = 2 x
# workgroups (what stem_wgrad_reduce_kernel folds per channel group: its unrolled loop runs for more than 32 slabs)
# ---------------------------------------------------------------------------------------------------------------------
STEM: Dict[str, Tuple[Tuple[int, ...], Tuple[int, int, int]]] = {
    "walk_512":      ((3, 224, 208, 3, 64), (546, 512, 1024)),          # 34 workgroups take a second tile
    "two_groups":    ((1, 100, 90, 6, 72), (42, 42, 84)),               # two channel groups, Cout tail in a second co tile
    "cout136":       ((2, 37, 53, 4, 136), (24, 24, 48)),               # three co tiles, the second channel group has 1 channel
    "one_channel":   ((5, 16, 16, 1, 8), (5, 5, 10)),                   # fewer than 32 slabs: the tail loop alone
    "partial_15":    ((1, 15, 15, 2, 64), (1, 1, 2)),
    "partial_17x33": ((1, 17, 33, 5, 64), (6, 6, 12)),
    "directed":      ((2, 21, 30, 3, 16), (8, 8, 16)),
}

# ---------------------------------------------------------------------------------------------------------------------
# head: (C, Cout) -> the family s2s_head_family reports (forward and backward alike): lanes per pixel, or 104 / 108
# ---------------------------------------------------------------------------------------------------------------------
HEAD_MO4, HEAD_MO8 = 104, 108
HEAD: Dict[Tuple[int, int], int] = {}
for _c, _pp in ((8, 1), (16, 2), (32, 4), (64, 8), (128, 16), (256, 32), (512, 64)):
    HEAD[(_c, 1)] = HEAD[(_c, 3)] = _pp
HEAD[(64, 4)] = 8
for _c in (24, 40, 72):
    HEAD[(_c, 1)] = HEAD[(_c, 3)] = HEAD_MO4
for _c in (16, 24):
    HEAD[(_c, 5)] = HEAD[(_c, 8)] = HEAD_MO8
# (B, H, W): 1 and 63 pixels (less than a workgroup's share), 1260 (two images: the NCHW index changes image inside a
# workgroup), 40000 (625 blocks of 64 pixels on the backward's 512 workgroups: an uneven share)
HEAD_PIXELS = [(1, 1, 1), (1, 7, 9), (2, 18, 35), (2, 100, 200)]
HEAD_BLOCK_CAP = 512


def head_pixels(C: int) -> List[Tuple[int, int, int]]:
    return HEAD_PIXELS[:3] if C >= 512 else HEAD_PIXELS


# refused launches: (C, Cout, forward) -- Cout (C + 1) = 2052 > 2048 in the backward; Cout > 8 in both
HEAD_REFUSED = [(512, 4, False), (64, 9, True), (64, 9, False)]


# ---------------------------------------------------------------------------------------------------------------------
# operands, references, yardsticks
# ---------------------------------------------------------------------------------------------------------------------
def _uniform(shape, g) -> torch.Tensor:
    return torch.rand(shape, generator=g) * 2 - 1


def as_read(t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """fp32 values as a kernel of that mode reads them."""
    return SR.bf(t) if dtype == BF else t.float()


def deviation(a: torch.Tensor, ref: torch.Tensor) -> Tuple[float, float]:
    """(max-norm relative, relative L2) of a against the float64 ref."""
    return SR.rel_max(a, ref), SR.rel_l2(a, ref)


def _seed(name) -> int:
    return sum((i + 1) * ord(ch) for i, ch in enumerate(str(name))) % 100003


@functools.lru_cache(maxsize=None)
def conv3x3_case(name: str, dtype: torch.dtype) -> dict:
    """x, dy: NCHW fp32 as the kernel reads them; ref: float64 [Cout, Cin, 3, 3]; yard: (max, l2) of torch's fp32."""
    (B, H, W, c0, c1, cout), _ = CONV3X3[name]
    g = torch.Generator().manual_seed(_seed(name))
    x = as_read(_uniform((B, c0 + c1, H, W), g), dtype)
    dy = as_read(_uniform((B, cout, H, W), g), dtype)
    with SR.cpu_thread_share():
        ref = torch.nn.grad.conv2d_weight(x.double(), (cout, c0 + c1, 3, 3), dy.double(), padding=1)
        yard = deviation(SR.conv3x3_wgrad(x, dy), ref)
    return {"x": x, "dy": dy, "ref": ref, "yard": yard}


@functools.lru_cache(maxsize=None)
def stem_case(name: str, dtype: torch.dtype) -> dict:
    """x: NCHW fp32 image as given (the bf16 kernel rounds it itself: SR.stem_image); dy NCHW as read; ref / ref_db."""
    (B, H, W, cin, cout), _ = STEM[name]
    g = torch.Generator().manual_seed(_seed(name))
    x = _uniform((B, cin, H, W), g)
    dy = as_read(_uniform((B, cout, H, W), g), dtype)
    xr = as_read(x, dtype)
    with SR.cpu_thread_share():
        ref = torch.nn.grad.conv2d_weight(xr.double(), (cout, cin, 3, 3), dy.double(), padding=1)
        yard = deviation(SR.conv3x3_wgrad(xr, dy), ref)
    ref_db = dy.double().sum((0, 2, 3))
    yard_db = deviation(dy.sum((0, 2, 3)), ref_db)
    return {"x": x, "dy": dy, "ref": ref, "ref_db": ref_db, "yard": yard, "yard_db": yard_db}


@functools.lru_cache(maxsize=None)
def head_case(C: int, cout: int, pixels: Tuple[int, int, int], dtype: torch.dtype) -> dict:
    """x NHWC as read, w [Cout, C, 1, 1], b, dy NCHW (all fp32); float64 einsum references v (NCHW), dx (NHWC), dw, db and
    the yardsticks of v, dw and db."""
    B, H, W = pixels
    g = torch.Generator().manual_seed(_seed((C, cout, pixels)))
    x = as_read(_uniform((B, H, W, C), g), dtype)
    w = _uniform((cout, C, 1, 1), g) * 0.3
    b = torch.rand(cout, generator=g) - 0.5
    dy = torch.rand((B, cout, H, W), generator=g) - 0.5
    wm, x64, dy64 = w.double().reshape(cout, C), x.double(), dy.double()
    v = torch.einsum("bhwc,oc->bohw", x64, wm) + b.double().reshape(1, cout, 1, 1)
    dx = torch.einsum("bohw,oc->bhwc", dy64, wm)
    dw = torch.einsum("bohw,bhwc->oc", dy64, x64).reshape(cout, C, 1, 1)
    db = dy64.sum((0, 2, 3))
    wf = w.reshape(cout, C)
    yard_v = deviation(torch.einsum("bhwc,oc->bohw", x, wf) + b.reshape(1, cout, 1, 1), v)
    yard_dw = deviation(torch.einsum("bohw,bhwc->oc", dy, x).reshape(cout, C, 1, 1), dw)
    yard_db = deviation(dy.sum((0, 2, 3)), db)
    return {"x": x, "w": w, "b": b, "dy": dy, "v": v, "dx": dx, "dw": dw, "db": db,
            "yard_v": yard_v, "yard_dw": yard_dw, "yard_db": yard_db}


def ratios(err: Tuple[float, float], yard: Tuple[float, float]) -> Tuple[float, float]:
    """kernel deviation / yardstick, (max, l2), the yardstick floored at YARD_FLOOR."""
    return err[0] / max(yard[0], YARD_FLOOR), err[1] / max(yard[1], YARD_FLOOR)


def worst_tap_and_tile(got: torch.Tensor, ref: torch.Tensor) -> str:
    """For a failure message: the tap and the 64 x 64 (co, ci) tile of an OIHW gradient with the largest deviation."""
    d = (got.detach().cpu().double() - ref).abs() / max(float(ref.abs().max()), 1e-30)
    cout, cin, kh, kw = d.shape
    if not bool(torch.isfinite(d).all()):
        bad = (~torch.isfinite(d)).nonzero()[0].tolist()
        return f"non-finite at (co, ci, kh, kw) = {bad}, {int((~torch.isfinite(d)).sum())} such elements"
    tap = d.amax((0, 1))
    t = int(tap.argmax())
    pad = torch.zeros(-(-cout // 64) * 64, -(-cin // 64) * 64, dtype=d.dtype)
    pad[:cout, :cin] = d.amax((2, 3))
    tiles = pad.reshape(pad.shape[0] // 64, 64, pad.shape[1] // 64, 64).amax((1, 3))
    k = int(tiles.argmax())
    co_t, ci_t = divmod(k, tiles.shape[1])
    return (f"worst tap (kh, kw) = ({t // kw}, {t % kw}): {float(tap.flatten()[t]):.2e}; worst 64x64 tile (co, ci) = "
            f"({co_t}, {ci_t}): {float(tiles[co_t, ci_t]):.2e}")
