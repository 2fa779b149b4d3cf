"""Case tables and float64 references for the 3x3 forward / data-gradient convolution (ops.conv3x3,
s2s_conv3x3_nhwc_s), form by form (a helper module of the suite, not a conftest; no HIP calls in here).

A row is  name: ((B, H, W, c0, c1, Cout), operands, plan).

  operands  a string of flags: bias, affine, relu, stats (BatchNorm partial sums; "rows0" = the launch is handed
            stat_rows = 0, the per-tile layout, else the layout it prefers), kwork (a split-K workspace is offered), f32
            (the row is an fp32 row: its plan is the fp32 family's), dgrad (the weight is the data-gradient packing of a
            [c0 + c1, Cout, 3, 3] forward weight and the reference is conv_transpose2d)
  plan      (family, cfg, gx, gy, grid, xsp, xsn, ksplit, stat_rows) as s2s_conv3x3_plan reports it with no switch set
            (CASES), under the row's own switch (SWITCH_CASES) or under S2S_CONV_PERS=2 S2S_CONV_STAGE=0 (PERS_CASES)

tests/test_conv3x3_forms_cpu.py holds the library's plan query to the tables and to the list of forms they must contain.

Operands come in two tiers.  EXACT: x in {-1, 0, 1}, w ternary with a density chosen per row, integer bias and shift,
power-of-two scale -- every product and every partial sum in any order is an integer below 2^24, so fp32 accumulation is
exact and the stored value has one correct answer, the float64 result rounded to nearest even.  REAL: x uniform in
(-1, 1) rounded as the kernel reads it, w scaled so that y is O(1), bias / scale / shift as in test_ops_gpu.py.

References are float64 (F.conv2d / F.conv_transpose2d under cpu_thread_share(), then the epilogue in float64) and come
with their YARDSTICK: the deviation from float64 of torch's fp32 result on the CPU, in the max norm, in L2 and per element
relative to S = conv(|x|, |w|) + |b|, floored at YARD_FLOOR.  Cases are cached and read-only."""
from __future__ import annotations

import functools
from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F

import stepwise_ref as SR

BF, F32 = torch.bfloat16, torch.float32
YARD_FLOOR = 1e-7
FIELDS = ("family", "cfg", "gx", "gy", "grid", "xsp", "xsn", "ksplit", "stat_rows")
STAGE_RESIDENT, STAGE_STREAM, PERS_CARRY, PERS, TAP, SPLIT_F32 = range(6)
# (rows, columns, channels) of a tile: kBf16Cfg / kF32Cfg of conv3x3_mfma.hip; the staged families tile 16 x 32 x 64
BF16_TILES = ((8, 32, 128), (8, 32, 64), (4, 32, 128), (4, 32, 64), (16, 16, 128), (16, 16, 64), (8, 16, 128), (8, 16, 64))
F32_TILES = ((4, 32, 64), (8, 16, 64))
STAGE_TILE = (16, 32, 64)
MAX_FLOP = 6e9

Row = Tuple[Tuple[int, int, int, int, int, int], str, Tuple[int, ...]]

# ---------------------------------------------------------------------------------------------------------------------
# no switch set
# ---------------------------------------------------------------------------------------------------------------------
CASES: Dict[str, Row] = {
    # staged kernel, filter resident (c0 + c1 <= 64): 256 workgroups walk gx * gy >= 512 jobs of 16 x 32 x 64
    "res_stats_xcd":     ((16, 17, 33, 8, 0, 512), "stats", (0, 1, 64, 8, 256, 8, 1, 1, 2048)),    # gx < 256: a walk jumps over channel tiles
    "res_stats_plain":   ((9, 17, 33, 8, 0, 1024), "stats", (0, 1, 36, 16, 256, 0, 1, 1, 2048)),   # gx % 8 != 0
    "res_stats_70":      ((2, 100, 130, 8, 0, 512), "stats", (0, 0, 70, 8, 256, 0, 1, 1, 2048)),
    "res_two_src":       ((300, 4, 33, 32, 8, 72), "stats", (0, 0, 600, 2, 256, 8, 1, 1, 2048)),   # second chunk has 8 of 32 channels
    "res_plain":         ((16, 17, 33, 8, 0, 512), "", (0, 1, 64, 8, 256, 8, 1, 1, 2048)),         # deferred epilogue
    "res_plain_36":      ((9, 17, 33, 8, 0, 1024), "", (0, 1, 36, 16, 256, 0, 1, 1, 2048)),                                           # plain order, deferred epilogue
    "res_plain_dgrad":   ((300, 4, 33, 32, 8, 72), "dgrad", (0, 0, 600, 2, 256, 8, 1, 1, 2048)),
    "res_affine":        ((16, 17, 33, 8, 0, 512), "bias affine relu", (0, 1, 64, 8, 256, 8, 1, 1, 2048)),
    "res_affine_norelu": ((9, 17, 33, 8, 0, 1024), "affine", (0, 1, 36, 16, 256, 0, 1, 1, 2048)),
    # staged kernel, filter streamed (c0 + c1 > 64), one channel tile; every tile has 4 of its 16 rows in the image
    "stream_stats":      ((300, 4, 33, 64, 8, 8), "stats", (1, 1, 600, 1, 256, 8, 1, 1, 2048)),
    "stream_plain":      ((300, 4, 33, 64, 8, 8), "", (1, 1, 600, 1, 256, 8, 1, 1, 2048)),
    "stream_affine":     ((300, 4, 33, 64, 8, 8), "bias affine relu", (1, 1, 600, 1, 256, 8, 1, 1, 2048)),
    "stream_dgrad":      ((257, 4, 33, 96, 0, 40), "dgrad stats", (1, 1, 514, 1, 256, 0, 1, 1, 2048)),
    # persistent per-tap kernel (>= 1024 tiles of cfg 1 or cfg 5, no bias / affine), walks of 2 and 3 tiles
    "pers1_tile_stats":  ((100, 9, 33, 64, 8, 136), "stats", (3, 1, 400, 3, 512, 8, 1, 1, 1600)),
    "pers1_plain":       ((100, 9, 33, 64, 8, 136), "", (3, 1, 400, 3, 512, 8, 1, 1, 1600)),
    "pers5_tile_stats":  ((600, 4, 8, 64, 8, 136), "stats", (3, 5, 600, 3, 512, 8, 1, 1, 2400)),
    "pers5_plain_dgrad": ((600, 4, 8, 64, 8, 136), "dgrad", (3, 5, 600, 3, 512, 8, 1, 1, 2400)),
    "pers1_rows0":       ((600, 4, 33, 64, 8, 8), "stats rows0", (3, 1, 1200, 1, 512, 8, 1, 1, 4800)),     # one channel tile, per-tile rows all the same
    "stream_rows0":      ((300, 4, 33, 64, 8, 8), "stats rows0", (4, 1, 600, 1, 0, 8, 1, 1, 2400)),     # per-tile rows keep a staged shape on the per-tap kernel
    # per-tap kernel, one tile per workgroup: each of the eight tiles with bias + statistics and with bias + affine + relu
    "tap0_stats":        ((40, 9, 70, 8, 0, 200), "bias stats", (4, 0, 240, 2, 0, 8, 1, 1, 480)),
    "tap0_affine":       ((40, 9, 70, 8, 0, 200), "bias affine relu", (4, 0, 240, 2, 0, 8, 1, 1, 480)),
    "tap1_stats":        ((1, 4, 17, 8, 0, 8), "bias stats", (4, 1, 1, 1, 0, 0, 1, 1, 4)),
    "tap1_affine":       ((3, 4, 33, 40, 0, 72), "bias affine relu", (4, 1, 6, 2, 0, 0, 1, 1, 24)),
    "tap2_stats":        ((45, 8, 32, 8, 0, 576), "bias stats", (4, 2, 90, 5, 0, 0, 1, 1, 180)),   # the Cout % 128 sliver
    "tap2_affine":       ((45, 8, 31, 8, 8, 576), "bias affine relu", (4, 2, 90, 5, 0, 0, 1, 1, 180)),
    "tap3_stats":        ((2, 20, 37, 16, 0, 24), "bias stats", (4, 3, 20, 1, 0, 0, 1, 1, 40)),
    "tap3_affine":       ((2, 20, 37, 16, 8, 24), "bias affine relu", (4, 3, 20, 1, 0, 0, 1, 1, 40)),
    "tap4_stats":        ((600, 4, 8, 8, 0, 72), "bias stats", (4, 4, 600, 1, 0, 8, 1, 1, 1200)),
    "tap4_affine":       ((600, 4, 8, 8, 8, 72), "bias affine relu", (4, 4, 600, 1, 0, 8, 1, 1, 1200)),
    "tap5_stats":        ((2, 8, 8, 256, 0, 72), "bias stats", (4, 5, 2, 2, 0, 0, 1, 1, 8)),
    "tap5_affine":       ((2, 8, 8, 40, 0, 72), "bias affine relu", (4, 5, 2, 2, 0, 0, 1, 1, 8)),
    "tap6_stats":        ((45, 16, 16, 8, 0, 576), "bias stats", (4, 6, 90, 5, 0, 0, 1, 1, 180)),  # the sliver, W <= 16
    "tap6_affine":       ((45, 15, 15, 8, 0, 576), "bias affine relu", (4, 6, 90, 5, 0, 0, 1, 1, 180)),
    "tap7_stats":        ((1, 9, 8, 8, 0, 8), "bias stats", (4, 7, 2, 1, 0, 0, 1, 1, 4)),
    "tap7_affine":       ((3, 9, 15, 24, 0, 40), "bias affine relu", (4, 7, 6, 1, 0, 0, 1, 1, 12)),
    # per-tap kernel, every XCD cut xcd_cut() returns
    "cut_8x1":           ((1, 15, 63, 8, 0, 8), "stats", (4, 3, 8, 1, 0, 8, 1, 1, 16)),
    "cut_4x2":           ((1, 7, 63, 8, 0, 72), "bias", (4, 3, 4, 2, 0, 4, 2, 1, 8)),
    "cut_2x4":           ((1, 3, 63, 8, 0, 200), "stats", (4, 1, 2, 4, 0, 2, 4, 1, 8)),
    "cut_1x8":           ((1, 3, 7, 8, 0, 456), "bias affine", (4, 5, 1, 8, 0, 1, 8, 1, 4)),
    # per-tap kernel, split-K: the 32-channel chunks shared by 2 ... 16 workgroups, evenly and not
    "split2":            ((1, 16, 16, 256, 64, 192), "kwork bias", (4, 7, 2, 3, 0, 0, 1, 2, 4)),
    "split2_two_src":    ((1, 16, 16, 264, 88, 192), "kwork", (4, 7, 2, 3, 0, 0, 1, 2, 4)),        # c0 % 32 != 0, 11 chunks
    "split3":            ((1, 8, 17, 416, 0, 8), "kwork bias", (4, 3, 2, 1, 0, 0, 1, 3, 4)),       # 13 chunks: 4 / 4 / 5
    "split4":            ((1, 8, 17, 544, 0, 8), "kwork bias affine relu", (4, 3, 2, 1, 0, 0, 1, 4, 4)),   # 17 chunks
    "split8":            ((2, 8, 8, 1048, 0, 72), "kwork affine relu", (4, 5, 2, 2, 0, 0, 1, 8, 8)),       # 33 chunks
    "split16":           ((1, 8, 17, 2048, 0, 8), "kwork", (4, 3, 2, 1, 0, 0, 1, 16, 4)),
    "split16_dgrad":     ((1, 7, 9, 2040, 0, 16), "kwork dgrad", (4, 5, 1, 1, 0, 0, 1, 16, 4)),
    # relu without a folded affine: relu(conv + bias) in both modes (the per-tap kernel's activation path in bf16)
    "relu_plain":        ((2, 20, 37, 16, 8, 72), "bias relu", (4, 3, 20, 2, 0, 4, 2, 1, 40)),
    "relu_stats":        ((2, 20, 37, 16, 8, 72), "bias relu stats", (4, 3, 20, 2, 0, 4, 2, 1, 40)),
    "relu_split":        ((1, 8, 17, 416, 0, 8), "kwork bias relu", (4, 3, 2, 1, 0, 0, 1, 3, 4)),
    "relu_nobias":       ((16, 17, 33, 8, 0, 512), "relu", (4, 1, 96, 8, 0, 4, 2, 1, 384)),         # a staged shape sent to the tap kernel
    # fp32 parity kernel: one plan per shape (cfg 0: W > 16, cfg 1: W <= 16), one statistics row per tile
    "f32_cfg0_stats":    ((2, 20, 37, 16, 8, 72), "f32 bias stats", (5, 0, 20, 2, 0, 0, 1, 1, 20)),   # the chunk straddles both sources
    "f32_cfg0_affine":   ((2, 20, 37, 16, 8, 72), "f32 bias affine relu", (5, 0, 20, 2, 0, 0, 1, 1, 20)),
    "f32_cfg1_affine":   ((3, 12, 10, 40, 0, 200), "f32 bias affine relu", (5, 1, 6, 4, 0, 0, 1, 1, 6)),
    "f32_cfg1_stats":    ((3, 12, 10, 40, 0, 200), "f32 stats", (5, 1, 6, 4, 0, 0, 1, 1, 6)),
    "f32_relu":          ((3, 12, 10, 40, 0, 200), "f32 bias relu stats", (5, 1, 6, 4, 0, 0, 1, 1, 6)),
    "f32_dgrad":         ((2, 9, 33, 24, 16, 40), "f32 dgrad", (5, 0, 12, 1, 0, 0, 1, 1, 12)),
    # edges: one pixel, one row, one column, H and W one more / one less than each tile size, Cout and cin of 8 and 8 mod
    "one_pixel":         ((1, 1, 1, 8, 0, 8), "bias", (4, 5, 1, 1, 0, 0, 1, 1, 4)),
    "one_row":           ((3, 1, 70, 8, 0, 72), "stats", (4, 1, 9, 2, 0, 0, 1, 1, 36)),
    "one_column":        ((3, 37, 1, 40, 0, 8), "stats", (4, 7, 15, 1, 0, 0, 1, 1, 30)),
    "hw_9x33":           ((2, 9, 33, 8, 0, 72), "bias stats", (4, 3, 12, 2, 0, 4, 2, 1, 24)),
    "hw_7x31":           ((2, 7, 31, 40, 0, 8), "bias", (4, 3, 4, 1, 0, 0, 1, 1, 8)),
    "hw_5x17":           ((2, 5, 17, 8, 0, 8), "stats", (4, 3, 4, 1, 0, 0, 1, 1, 8)),
    "hw_3x15":           ((2, 3, 15, 8, 0, 72), "bias stats", (4, 5, 2, 2, 0, 0, 1, 1, 8)),
    "hw_17x17":          ((2, 17, 17, 40, 0, 72), "stats", (4, 3, 10, 2, 0, 0, 1, 1, 20)),
    "hw_15x16":          ((3, 15, 16, 8, 0, 136), "bias", (4, 7, 6, 3, 0, 0, 1, 1, 12)),
    "hw_17x9":           ((3, 17, 9, 40, 0, 136), "stats", (4, 7, 9, 3, 0, 0, 1, 1, 18)),
}

# rows whose form needs a switch of its own (the plan is asserted in a child process that sets it)
SWITCH_CASES: Dict[str, Tuple[Tuple[int, ...], str, Dict[str, str], Tuple[int, ...]]] = {
    # the staged streaming order with more than one channel tile (the default leaves those launches on the per-tap kernels)
    "stream_gy2_stats":  ((300, 4, 33, 64, 8, 72), "stats", {"S2S_CONV_STAGE": "2"}, (1, 0, 600, 2, 256, 8, 1, 1, 2048)),
    "stream_gy2_plain":  ((300, 4, 33, 64, 8, 72), "", {"S2S_CONV_STAGE": "2"}, (1, 0, 600, 2, 256, 8, 1, 1, 2048)),
    # carried statistics on the persistent kernel: with no switch set every such launch is taken by the staged kernel
    "pers1_carry":       ((600, 4, 33, 64, 8, 8), "stats", {"S2S_CONV_STAGE": "0"}, (2, 1, 1200, 1, 512, 8, 1, 1, 2048)),
}

# ---------------------------------------------------------------------------------------------------------------------
# S2S_CONV_PERS=2 S2S_CONV_STAGE=0: the persistent kernel from two tiles on, which is the only way to its instantiations
# for cfgs 2, 3, 6 and 7.  Per cfg: STATS = 0 (plain), 1 (per tile, gy > 1) and 2 (carried, gy == 1), each with one tile
# per workgroup and with more than 512 tiles.  cfgs 2 and 6 exist only for Cout >= 512 with Cout % 128 in (0, 64], where
# gy >= 5 (nothing is carried) and the tile count stays below 10/9 of cfg 1's / cfg 5's, which is below 448 (no walk).
# ---------------------------------------------------------------------------------------------------------------------
PERS_ENV = {"S2S_CONV_PERS": "2", "S2S_CONV_STAGE": "0"}
_PERS_SHAPES = {   # cfg: (one tile per workgroup, more than 512 tiles: B for Cout = 72 and for Cout = 8)
    1: ((1, 4, 33), (150, 300, 4, 33)), 3: ((1, 8, 17), (50, 100, 9, 33)),
    5: ((2, 8, 8), (300, 600, 4, 8)), 7: ((1, 9, 8), (150, 300, 9, 8)),
}
_PERS_ROWS: Dict[str, Tuple[Tuple[int, ...], str]] = {}
for _cfg, ((_b, _h, _w), (_b72, _b8, _hh, _ww)) in _PERS_SHAPES.items():
    _PERS_ROWS[f"p{_cfg}_one_plain"] = ((_b, _h, _w, 32, 8, 72), "dgrad" if _cfg == 3 else "")
    _PERS_ROWS[f"p{_cfg}_one_tile"] = ((_b, _h, _w, 32, 8, 72), "stats")
    _PERS_ROWS[f"p{_cfg}_one_carry"] = ((_b, _h, _w, 32, 8, 8), "stats")
    _PERS_ROWS[f"p{_cfg}_walk_plain"] = ((_b72, _hh, _ww, 32, 8, 72), "dgrad" if _cfg == 7 else "")
    _PERS_ROWS[f"p{_cfg}_walk_tile"] = ((_b72, _hh, _ww, 32, 8, 72), "stats")
    _PERS_ROWS[f"p{_cfg}_walk_carry"] = ((_b8, _hh, _ww, 32, 8, 8), "stats")
_PERS_ROWS["p2_one_plain"] = ((45, 8, 32, 32, 8, 576), "")
_PERS_ROWS["p2_one_tile"] = ((45, 8, 32, 32, 8, 576), "stats")
_PERS_ROWS["p6_one_plain"] = ((45, 16, 16, 32, 8, 576), "dgrad")
_PERS_ROWS["p6_one_tile"] = ((45, 16, 16, 32, 8, 576), "stats")
PERS_PLANS: Dict[str, Tuple[int, ...]] = {
    "p1_one_plain": (3, 1, 2, 2, 4, 0, 1, 1, 8),
    "p1_one_tile": (3, 1, 2, 2, 4, 0, 1, 1, 8),
    "p1_one_carry": (2, 1, 2, 1, 2, 0, 1, 1, 8),
    "p1_walk_plain": (3, 1, 300, 2, 512, 4, 2, 1, 1200),
    "p1_walk_tile": (3, 1, 300, 2, 512, 4, 2, 1, 1200),
    "p1_walk_carry": (2, 1, 600, 1, 512, 8, 1, 1, 2048),
    "p3_one_plain": (3, 3, 2, 2, 4, 0, 1, 1, 4),
    "p3_one_tile": (3, 3, 2, 2, 4, 0, 1, 1, 4),
    "p3_one_carry": (2, 3, 2, 1, 2, 0, 1, 1, 4),
    "p3_walk_plain": (3, 3, 300, 2, 512, 4, 2, 1, 600),
    "p3_walk_tile": (3, 3, 300, 2, 512, 4, 2, 1, 600),
    "p3_walk_carry": (2, 3, 600, 1, 512, 8, 1, 1, 1024),
    "p5_one_plain": (3, 5, 2, 2, 4, 0, 1, 1, 8),
    "p5_one_tile": (3, 5, 2, 2, 4, 0, 1, 1, 8),
    "p5_one_carry": (2, 5, 2, 1, 2, 0, 1, 1, 8),
    "p5_walk_plain": (3, 5, 300, 2, 512, 4, 2, 1, 1200),
    "p5_walk_tile": (3, 5, 300, 2, 512, 4, 2, 1, 1200),
    "p5_walk_carry": (2, 5, 600, 1, 512, 8, 1, 1, 2048),
    "p7_one_plain": (3, 7, 2, 2, 4, 0, 1, 1, 4),
    "p7_one_tile": (3, 7, 2, 2, 4, 0, 1, 1, 4),
    "p7_one_carry": (2, 7, 2, 1, 2, 0, 1, 1, 4),
    "p7_walk_plain": (3, 7, 300, 2, 512, 4, 2, 1, 600),
    "p7_walk_tile": (3, 7, 300, 2, 512, 4, 2, 1, 600),
    "p7_walk_carry": (2, 7, 600, 1, 512, 8, 1, 1, 1024),
    "p2_one_plain": (3, 2, 90, 5, 450, 0, 1, 1, 180),
    "p2_one_tile": (3, 2, 90, 5, 450, 0, 1, 1, 180),
    "p6_one_plain": (3, 6, 90, 5, 450, 0, 1, 1, 180),
    "p6_one_tile": (3, 6, 90, 5, 450, 0, 1, 1, 180),
}
PERS_CASES: Dict[str, Row] = {k: (v[0], v[1], PERS_PLANS.get(k, ())) for k, v in _PERS_ROWS.items()}


def row(name: str):
    """(shape, flags, env, plan) of a row of any table."""
    if name in CASES:
        s, f, p = CASES[name]
        return s, f.split(), {}, p
    if name in SWITCH_CASES:
        s, f, e, p = SWITCH_CASES[name]
        return s, f.split(), e, p
    s, f, p = PERS_CASES[name]
    return s, f.split(), PERS_ENV, p


def row_dtype(name: str) -> torch.dtype:
    return F32 if "f32" in row(name)[1] else BF


def flop(name: str) -> float:
    B, H, W, c0, c1, cout = row(name)[0]
    return 2.0 * B * H * W * cout * 9 * (c0 + c1)


def plan_query_args(name: str) -> dict:
    """Keyword arguments of ops.conv3x3_plan for the row.  (A bf16 launch with relu and no affine runs on the activation
    path: its plan is that of the same launch with a bias.)"""
    shape, flags, _, _ = row(name)
    relu_only = "relu" in flags and "affine" not in flags
    return {"bias": "bias" in flags or relu_only, "affine": "affine" in flags, "stats": "stats" in flags,
            "stat_rows": 0 if "rows0" in flags else -1, "kwork": "kwork" in flags}


def tile_of(plan: dict, dtype: torch.dtype) -> Tuple[int, int, int]:
    if plan["family"] in (STAGE_RESIDENT, STAGE_STREAM):
        return STAGE_TILE
    return F32_TILES[plan["cfg"]] if dtype == F32 else BF16_TILES[plan["cfg"]]


def stats_form(plan: dict, flags) -> str:
    if "stats" not in flags:
        return "none"
    return "carried" if plan["family"] in (STAGE_RESIDENT, STAGE_STREAM, PERS_CARRY) else "tile"


# ---------------------------------------------------------------------------------------------------------------------
# operands, references, yardsticks
# ---------------------------------------------------------------------------------------------------------------------
def as_read(t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    return SR.bf(t) if dtype == BF else t.float()


def _seed(name) -> int:
    return sum((i + 1) * ord(ch) for i, ch in enumerate(str(name))) % 100003


def exact_density(shape, stats: bool) -> float:
    """Share of non-zero weights in the exact tier.  E[y^2] = 9 cin (2/3) d; a statistics row keeps the sum of y^2 over
    all pixels of a channel below 2^24 with a margin of 4 (the CPU test asserts the sum itself)."""
    B, H, W, c0, c1, _ = shape
    if not stats:
        return 1.0
    return min(1.0, 2.0 ** 22 / (B * H * W * 6.0 * (c0 + c1)))


def _conv(x: torch.Tensor, w: torch.Tensor, dgrad: bool) -> torch.Tensor:
    return F.conv_transpose2d(x, w, None, padding=1) if dgrad else F.conv2d(x, w, None, padding=1)


@functools.lru_cache(maxsize=4)
def case(name: str, dtype: torch.dtype, tier: str) -> dict:
    """x: NCHW fp32 as the kernel reads it; w: the fp32 weight to pack, OIHW of the forward convolution (a dgrad row: of
    the forward convolution whose data gradient the launch is, [c0 + c1, Cout, 3, 3]); b, sc, sh: fp32 or None.
    pre: float64 NCHW before the relu, ref: after it, S: conv(|x|, |w|) + |b| (float64), yard: (max, l2, per element
    relative to S) of torch's fp32 result."""
    shape, flags, _, _ = row(name)
    B, H, W, c0, c1, cout = shape
    cin = c0 + c1
    dgrad = "dgrad" in flags
    assert flop(name) <= MAX_FLOP, name
    g = torch.Generator().manual_seed(_seed((name, tier)))
    wshape = (cin, cout, 3, 3) if dgrad else (cout, cin, 3, 3)
    if tier == "exact":
        x = torch.randint(-1, 2, (B, cin, H, W), generator=g).float()
        d = exact_density(shape, "stats" in flags)
        w = torch.randint(-1, 2, wshape, generator=g).float() * (torch.rand(wshape, generator=g) < d).float()
        b = torch.randint(-3, 4, (cout,), generator=g).float()
        sc = torch.tensor([0.5, 1.0, 2.0, -1.0])[torch.randint(0, 4, (cout,), generator=g)]
        sh = torch.randint(-2, 3, (cout,), generator=g).float()
    else:
        x = as_read(torch.rand((B, cin, H, W), generator=g) * 2 - 1, dtype)
        w = (torch.rand(wshape, generator=g) * 2 - 1) * (3.0 / cin) ** 0.5
        b = torch.rand(cout, generator=g) - 0.5
        sc = torch.rand(cout, generator=g) + 0.5
        sh = torch.rand(cout, generator=g) - 0.5
    b = b if "bias" in flags else None
    if "affine" not in flags:
        sc = sh = None
    wr = as_read(w, dtype)
    v = lambda t: t.reshape(1, cout, 1, 1)                                             # noqa: E731
    with SR.cpu_thread_share():
        acc = _conv(x.double(), wr.double(), dgrad)
        S = _conv(x.double().abs(), wr.double().abs(), dgrad)
        acc32 = acc.float() if tier == "exact" else _conv(x, wr, dgrad)     # (exact tier: no yardstick is used)
    pre, pre32 = acc, acc32
    if b is not None:
        pre, pre32, S = pre + v(b.double()), pre32 + v(b), S + v(b.double().abs())
    if sc is not None:
        pre, pre32 = pre * v(sc.double()) + v(sh.double()), pre32 * v(sc) + v(sh)
    relu = "relu" in flags
    ref = pre.clamp_min(0) if relu else pre
    ref32 = pre32.clamp_min(0) if relu else pre32
    mag = S if sc is None else S * v(sc.double().abs()) + v(sh.double().abs())
    yard = (max(SR.rel_max(ref32, ref), YARD_FLOOR), max(SR.rel_l2(ref32, ref), YARD_FLOOR),
            max(float(((pre32.double() - pre).abs() / mag.clamp_min(1e-30)).max()), YARD_FLOOR))
    return {"x": x, "w": w, "wr": wr, "b": b, "sc": sc, "sh": sh, "pre": pre, "ref": ref, "S": S, "mag": mag, "yard": yard}


def stored(ref: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """The exact tier's one correct stored tensor: the float64 result (exact in fp32) rounded to nearest even."""
    return ref.float().to(dtype)


def stat_sums(y_nchw: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """float64 (sum, sum of squares) per channel of stored values."""
    y = y_nchw.double()
    return y.sum((0, 2, 3)), (y * y).sum((0, 2, 3))


def stat_yardstick(y_nchw: torch.Tensor) -> Tuple[float, float]:
    """What fp32 summation costs on these stored values: torch's fp32 (sum, sum of squares) per channel against float64,
    relative to sum |y| and sum y^2 of the channel, the worst channel, floored."""
    y = y_nchw.float()
    s1, s2 = stat_sums(y)
    a1 = y.double().abs().sum((0, 2, 3)).clamp_min(1e-30)
    e1 = float(((y.sum((0, 2, 3)).double() - s1).abs() / a1).max())
    e2 = float((((y * y).sum((0, 2, 3)).double() - s2).abs() / s2.clamp_min(1e-30)).max())
    return max(e1, YARD_FLOOR), max(e2, YARD_FLOOR)


def worst(got_nchw: torch.Tensor, ref: torch.Tensor, plan: Optional[dict], dtype: torch.dtype) -> str:
    """For a failure message: the worst pixel and channel and the tile of the row's plan they fall in."""
    d = (got_nchw.detach().cpu().double() - ref).abs()
    bad = ~torch.isfinite(d)
    if bool(bad.any()):
        d = bad.double()
        head = f"{int(bad.sum())} non-finite elements, first"
    else:
        head = f"worst |err| {float(d.max()):.3e} (max |ref| {float(ref.abs().max()):.3e})"
    k = int(d.flatten().argmax())
    _, C, H, W = d.shape
    n, c, y, x = k // (C * H * W), k // (H * W) % C, k // W % H, k % W
    per_c = d.amax((0, 2, 3))
    msg = f"{head} at image {n} y {y} x {x} channel {c}; worst channel {int(per_c.argmax())}; {int((d > 0).sum())} of {d.numel()} differ"
    if plan is not None:
        th, tw, bn = tile_of(plan, dtype)
        msg += (f"; tile {th}x{tw}x{bn} row {y // th} column {x // tw} channel tile {c // bn} of family "
                f"{SR.FAMILY_NAMES[plan['family']]} cfg {plan['cfg']} ksplit {plan['ksplit']}")
    return msg
