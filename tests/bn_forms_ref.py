"""Case tables and the float64 host model of the BatchNorm / ReLU / 2x2 max-pool kernels (norm_act.hip), form by form (a
helper module of the suite, not a conftest; no HIP calls in here except the plan query a caller hands in).

  * ``bwd_model``: BN(train) -> ReLU (-> pool) backward as s2s_bn_relu_bwd_phase computes it.  The DECISIONS are the
    kernel's: the ReLU mask from fmaf(x, scale, shift) with the fp32 scale / shift rows -- of the value rounded to the
    storage type for the windowed kernels (WindowGrad::eval), of the unrounded value for the flat ones --, the pool winner
    the first maximum, in (0,0), (0,1), (1,0), (1,1) order, of the stored ReLU output.  Odd H / W: the last row / column
    belongs to a window without a pool output and receives g1 only.  Everything after the decisions (dz, xhat, the sums,
    the means c1 and c2, dx) is evaluated in ``cd``: float64 for the reference, float32 for the yardstick (what plain
    fp32 arithmetic on the CPU costs from the same decisions).  With ``count_total`` / ``other`` it is one shard of a
    SyncBatchNorm step: c1, c2 = local sums / count_total (+ the other shards' vector), dgamma / dbeta the local sums.
  * ``finalize_model``: s2s_bn_finalize_b teacher-forced on the partial buffer: the float64 sum of the given partials.
  * ``plan``: a mirror of host_pcb / red_blocks / finalize_tpc, used only to label the cases and to assert that a case
    reaches the form it was written for; s2s_bn_bwd_blocks gives the real row count.

tests/test_bn_forms_cpu.py holds the model to torch autograd in float64 and the mirror to the library's query.
References are cached per (row, dtype[, kind]) and shared by the tests; treat them as read-only."""
from __future__ import annotations

import functools
from typing import Dict, Optional, Tuple

import torch

import stepwise_ref as SR

BF, F32 = torch.bfloat16, torch.float32
YARD_FLOOR = 1e-7
KINDS = ("g1+gp", "g1", "gp")        # windowed kernels / flat kernels / windowed with g1 null

# (B, H, W, C): pcb, channel groups, pieces in the last group, nb, finalize threads per channel, 16-byte finalize loads
BWD: Dict[Tuple[int, int, int, int], Tuple[int, int, int, int, int, bool]] = {
    (1, 1, 1, 8):        (1, 1, 1, 1, 64, False),       # one pixel, one window
    (2, 5, 7, 8):        (1, 1, 1, 1, 64, False),       # odd H and W
    (1, 2, 2, 16):       (2, 1, 2, 1, 64, False),       # one full window
    (2, 13, 9, 24):      (4, 1, 3, 2, 64, False),       # 3 of 4 pieces
    (3, 12, 10, 40):     (8, 1, 5, 3, 64, False),       # 5 of 8 pieces, scalar finalize
    (2, 9, 11, 72):      (16, 1, 9, 4, 64, True),       # 9 of 16 pieces, 16-byte finalize loads
    (1, 17, 15, 136):    (32, 1, 17, 9, 64, False),     # 17 of 32 pieces
    (1, 7, 9, 264):      (32, 2, 1, 3, 64, False),      # two channel groups, the second holds 1 piece
    (3, 25, 27, 520):    (32, 3, 1, 69, 64, False),     # three channel groups, the last holds 1 piece
    (2, 6, 6, 1024):     (32, 4, 32, 3, 64, False),     # four full channel groups
    (2, 66, 66, 256):    (32, 1, 32, 273, 256, False),  # 256-thread finalize, scalar path
    (2, 64, 68, 256):    (32, 1, 32, 272, 256, True),   # 256-thread finalize, 16-byte path
    (4, 260, 260, 8):    (1, 1, 1, 265, 256, False),    # pcb 1: 256 windows per workgroup row
    (1, 222, 222, 256):  (32, 1, 32, 1536, 256, True),  # nb at its cap: a workgroup walks more than one window
}
CAPPED = (1, 222, 222, 256)
NB_CAP = 1536


def shape_id(s) -> str:
    return "x".join(map(str, s))


# ---------------------------------------------------------------------------------------------------------------------
# plan mirror
# ---------------------------------------------------------------------------------------------------------------------
def host_pcb(C: int) -> int:
    p = 1
    while p < 32 and p * 8 < C:
        p <<= 1
    return p


def red_blocks(B: int, H: int, W: int, C: int) -> int:
    nwin = B * ((H + 1) // 2) * ((W + 1) // 2)
    pcb = host_pcb(C)
    wl = 256 // pcb
    want = max(1, NB_CAP // -(-(C // 8) // pcb))
    return max(1, min(-(-nwin // wl), want))


def finalize_tpc(nblk: int) -> int:
    return 256 if nblk > 256 else 64


def plan(B: int, H: int, W: int, C: int, nb: Optional[int] = None) -> dict:
    """The launch form of s2s_bn_relu_bwd_phase; ``nb`` from s2s_bn_bwd_blocks where the caller has it."""
    pcb = host_pcb(C)
    pieces = C // 8
    groups = -(-pieces // pcb)
    nb = red_blocks(B, H, W, C) if nb is None else nb
    nwin = B * ((H + 1) // 2) * ((W + 1) // 2)
    return {"pcb": pcb, "groups": groups, "last": pieces - (groups - 1) * pcb, "nb": nb, "tpc": finalize_tpc(nb),
            "vec": nb % 4 == 0, "walk": -(-nwin // (nb * (256 // pcb)))}


def plan_row(p: dict) -> Tuple[int, int, int, int, int, bool]:
    return p["pcb"], p["groups"], p["last"], p["nb"], p["tpc"], p["vec"]


# ---------------------------------------------------------------------------------------------------------------------
# error measures
# ---------------------------------------------------------------------------------------------------------------------
def as_read(t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """fp32 values as a kernel of that storage type reads (and stores) them: identity rounding in fp32."""
    return SR.bf(t) if dtype == BF else t.float()


def deviation(a: torch.Tensor, ref: torch.Tensor) -> Tuple[float, float]:
    return SR.rel_max(a, ref), SR.rel_l2(a, ref)


def ratios(err, yard) -> Tuple[float, float]:
    return err[0] / max(yard[0], YARD_FLOOR), err[1] / max(yard[1], YARD_FLOOR)


def f32_ulps(a: torch.Tensor, r: torch.Tensor, mag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """|a - r| in units of the fp32 spacing at |mag| (default |r|)."""
    a, r = a.detach().cpu().double(), r.detach().cpu().double()
    m = (r if mag is None else mag.detach().cpu().double()).abs().clamp_min(2.0 ** -126)
    return (a - r).abs() / torch.exp2(torch.floor(torch.log2(m)) - 23)


# ---------------------------------------------------------------------------------------------------------------------
# backward model
# ---------------------------------------------------------------------------------------------------------------------
def decisions(raw: torch.Tensor, stats: torch.Tensor, dtype: torch.dtype, windowed: bool):
    """(ReLU mask, stored ReLU output) as the kernels take them from the fp32 scale / shift rows."""
    z = SR.fma_f32(raw, stats[2], stats[3])
    y = as_read(z.clamp_min(0.0), dtype)
    return (y > 0) if windowed else (z > 0), y


def _bwd_model(g1, gp, raw, stats, gamma, dtype, cd, count_total, other):
    B, H, W, C = raw.shape
    Hp, Wp = H >> 1, W >> 1
    mask, y = decisions(raw, stats, dtype, gp is not None)
    dz = torch.zeros(raw.shape, dtype=cd) if g1 is None else g1.detach().cpu().to(cd).clone()
    if gp is not None and Hp and Wp:
        win = SR.pool_winner(y[:, :2 * Hp, :2 * Wp])
        dz[:, :2 * Hp, :2 * Wp] += SR.pool_scatter(gp.detach().cpu().to(cd), win)
    dz = torch.where(mask, dz, torch.zeros_like(dz))
    st = stats.detach().cpu().to(cd)
    xh = (raw.detach().cpu().to(cd) - st[0]) * st[1]
    n = B * H * W if count_total is None else count_total
    dbeta = dz.reshape(-1, C).sum(0)
    dgamma = (dz * xh).reshape(-1, C).sum(0)
    c = torch.stack([dbeta, dgamma]) / n
    if other is not None:
        c = c + other.detach().cpu().to(cd).reshape(2, C)
    gak = gamma.detach().cpu().to(cd) * st[1]
    t = xh * c[1]
    dx = gak * (dz - c[0] - t)
    # room for the fp32 evaluation of gak * (dz - c1 - xh * c2) in a bf16-stored dx (see _hold_dx in the GPU test)
    slack = 2.0 ** -22 * gak.abs() * (dz.abs() + c[0].abs() + t.abs())
    return {"dx": dx, "dgamma": dgamma, "dbeta": dbeta, "c1": c[0], "c2": c[1], "slack": slack}


def bwd_model(g1: Optional[torch.Tensor], gp: Optional[torch.Tensor], raw: torch.Tensor, stats: torch.Tensor,
              gamma: torch.Tensor, dtype: torch.dtype, cd: torch.dtype = torch.float64,
              count_total: Optional[int] = None, other: Optional[torch.Tensor] = None) -> dict:
    """``raw``, ``g1`` [B, H, W, C] and ``gp`` [B, H/2, W/2, C] as read; ``stats`` rows mean, invstd, scale, shift (fp32
    as the kernel holds them, or float64 for the comparison with autograd: the decisions round scale and shift to fp32
    either way).  Returns dx, dgamma (sum dz xhat), dbeta (sum dz), c1, c2 and slack in ``cd``.  Large cases are
    evaluated in channel chunks."""
    C = raw.shape[-1]
    step = C if raw.numel() <= (1 << 22) else 32
    outs = []
    with SR.cpu_thread_share():
        for c0 in range(0, C, step):
            s = slice(c0, c0 + step)
            o = None if other is None else other.reshape(2, C)[:, s]
            outs.append(_bwd_model(None if g1 is None else g1[..., s], None if gp is None else gp[..., s], raw[..., s],
                                   stats[:, s], gamma[s], dtype, cd, count_total, o))
    return {k: torch.cat([o[k] for o in outs], -1) for k in outs[0]}


def _seed(name) -> int:
    return sum((i + 1) * ord(ch) for i, ch in enumerate(str(name))) % 100003


def stats_rows(raw: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5,
               dtype: torch.dtype = F32) -> torch.Tensor:
    """[4, C] rows mean, invstd, scale, shift of the stored conv output ``raw``, from float64 statistics."""
    st = SR.bn_stats(raw, eps)
    scale, shift = SR.bn_affine(st, gamma, beta)
    return torch.stack([st["mean"], st["invstd"], scale, shift]).to(dtype)


@functools.lru_cache(maxsize=4)
def bwd_case(shape: Tuple[int, int, int, int], dtype: torch.dtype) -> dict:
    """Operands of one table row: the conv output (per-channel offset and spread), gamma about 1 and beta about 0.3 (so
    the pre-activation has standard deviation about 1, mean about 0.3, and both ReLU branches are populated), gradients
    uniform in +-0.5, all as read; the statistics rows in fp32."""
    B, H, W, C = shape
    g = torch.Generator().manual_seed(_seed(shape))
    spread = 0.5 + 1.5 * torch.rand(C, generator=g)
    offset = torch.rand(C, generator=g) * 2 - 1
    raw = as_read(torch.randn(shape, generator=g) * spread + offset, dtype)
    gamma = 0.75 + 0.5 * torch.rand(C, generator=g)
    beta = 0.2 + 0.2 * torch.rand(C, generator=g)
    g1 = as_read(torch.rand(shape, generator=g) - 0.5, dtype)
    gp = as_read(torch.rand((B, H >> 1, W >> 1, C), generator=g) - 0.5, dtype)
    return {"raw": raw, "g1": g1, "gp": gp, "gamma": gamma, "beta": beta, "stats": stats_rows(raw, gamma, beta)}


def kind_operands(case: dict, kind: str):
    return (case["g1"] if kind != "gp" else None), (case["gp"] if kind != "g1" else None)


@functools.lru_cache(maxsize=12)
def bwd_ref(shape: Tuple[int, int, int, int], dtype: torch.dtype, kind: str) -> dict:
    """The float64 model of one (row, dtype, kind) and the yardsticks {quantity: (max, l2)} of the fp32 evaluation."""
    case = bwd_case(shape, dtype)
    g1, gp = kind_operands(case, kind)
    ref = bwd_model(g1, gp, case["raw"], case["stats"], case["gamma"], dtype)
    f32 = bwd_model(g1, gp, case["raw"], case["stats"], case["gamma"], dtype, cd=F32)
    ref["yard"] = {k: deviation(f32[k], ref[k]) for k in ("dx", "dgamma", "dbeta", "c1", "c2")}
    if dtype != BF:
        ref["slack"] = None            # only a bf16-stored dx is held element by element
    return ref


# ---------------------------------------------------------------------------------------------------------------------
# statistics finalize
# ---------------------------------------------------------------------------------------------------------------------
def finalize_model(part: torch.Tensor, count: int, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5,
                   momentum: float = 0.1, rm: Optional[torch.Tensor] = None, rv: Optional[torch.Tensor] = None,
                   conv_bias: Optional[torch.Tensor] = None) -> dict:
    """bn_finalize_kernel on the partial buffer [2][C][nblk] in float64.  eps and momentum reach the kernel as fp32."""
    eps = float(torch.tensor(eps, dtype=F32))
    m = float(torch.tensor(momentum, dtype=F32))
    s = part.detach().cpu().double().sum(-1)
    mean = s[0] / count
    var = (s[1] / count - mean * mean).clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma.detach().cpu().double() * invstd
    out = {"sums": s, "mean": mean, "var": var, "invstd": invstd, "scale": scale,
           "shift": beta.detach().cpu().double() - mean * scale, "shift_mag": beta.detach().cpu().double().abs() + (mean * scale).abs()}
    if rm is not None:
        new_m = mean if conv_bias is None else mean + conv_bias.detach().cpu().double()
        new_v = var * (count / (count - 1.0)) if count > 1 else var
        old_m, old_v = rm.detach().cpu().double() * (1.0 - m), rv.detach().cpu().double() * (1.0 - m)
        out.update(running_mean=old_m + m * new_m, running_var=old_v + m * new_v,
                   running_mean_mag=old_m.abs() + (m * new_m).abs(), running_var_mag=old_v.abs() + (m * new_v).abs())
    return out


FIN_NBLK = (1, 3, 4, 64, 255, 256, 257, 260, 1536)
FIN_C = (1, 3, 5, 64, 1024)
FIN_COUNT = 1 << 16


@functools.lru_cache(maxsize=None)
def finalize_part(nblk: int, C: int) -> torch.Tensor:
    """A synthetic partial buffer [2][C][nblk] for FIN_COUNT elements.  Every row is quantised to a grid of 2^24 steps of
    its largest entry, so a float64 sum of it is exact in any order: the model and the kernel see the same sums, and a
    difference between them is a dropped, doubled or misplaced partial.  For C >= 3, channel 0 is a constant input whose
    sum of squares was rounded down (a negative variance: the clamp, invstd = 1 / sqrt(eps)) and channel C - 1 has mean
    about 1e3 and a variance of 1e-4 that the fp32 partials cannot resolve; its mean is a multiple of 2^-12, so mean^2
    is exact in float64 and a fused or unfused b/count - mean^2 agree."""
    g = torch.Generator().manual_seed(_seed(("finalize", nblk, C)))
    n = FIN_COUNT / nblk
    mu = torch.rand(C, 1, generator=g) * 2 - 0.7
    sd = 0.3 + torch.rand(C, 1, generator=g)
    p0 = n * (mu + sd * torch.randn(C, nblk, generator=g) / n ** 0.5)
    p1 = n * (mu * mu + sd * sd) * (1 + 0.1 * torch.randn(C, nblk, generator=g) / n ** 0.5)
    part = torch.stack([p0, p1]).double()
    if C >= 3:
        part[0, 0], part[1, 0] = 1.5 * n, 2.25 * n * (1 - 2.0 ** -12)
        k = torch.round(1000.25 * n / 16 + torch.randn(nblk, generator=g).double())
        part[0, C - 1] = 16 * k
        part[1, C - 1] = ((16 * k.sum() / FIN_COUNT) ** 2 + 1e-4) * n
    q = torch.exp2(torch.ceil(torch.log2(part.abs().amax(-1, keepdim=True))) - 23)
    part = (torch.round(part / q) * q).float()
    if C >= 3:
        assert float(part[0, C - 1].double().sum()) % 16 == 0
    return part
