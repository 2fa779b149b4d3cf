"""Row tables, launch-arithmetic predicates and float64 host models of the small fp32 "glue" kernels of a training step
and of the samplers, form by form (a helper module of the suite, not a conftest; CPU only, no HIP calls in here):

  optim.hip     s2s_adam_step / _step_dev / s2s_adam_multi / s2s_adam_ema_step / _ema_step_dev,
                s2s_pack_conv3x3 / _batched, s2s_nchw_to_nhwc / s2s_nhwc_to_nchw
  resample.hip  s2s_pixel_sum
  flow.hip      s2s_time_embedding, s2s_linear_fwd / _bwd, s2s_silu_fwd / _bwd, s2s_cfm_sample, s2s_mse_loss,
                s2s_ode_error_norm, s2s_axpy, s2s_euler_tick, s2s_fill_f32

Models.  Every ``*_ref(..., cd)`` evaluates the operation from the fp32 (or bf16-exact) operands the kernel receives, with
``cd = float64`` for the reference and ``cd = float32`` for the yardstick: what torch's fp32 arithmetic on the CPU costs
for the same quantity (deviations as relative max and L2, floored at 1e-7).  Scalars that reach an
entry point as a C ``float`` are rounded to fp32 first (``f32``); Adam's bias corrections are taken in double from those
``float`` betas, as the entry point forms them.

Launch arithmetic.  The constants of the kernels' launches are mirrored once, below; ``walk`` is the grid-stride loop of
``ew_grid`` / ``ema_grid`` / the 1024-block reductions, and the ``*_form`` predicates say which form of a kernel a row
takes.  tests/test_glue_forms_cpu.py asserts that every table holds every form.

Cases are cached and shared; treat them as read-only."""
from __future__ import annotations

import functools
import math
import struct

import torch
import torch.nn.functional as F

from head_tail_forms_ref import BF, F32, F64, YARD_FLOOR, deviation, ratios, round_to, same_bits, ulp  # noqa: F401

# ---------------------------------------------------------------------------------------------------------------------
# launch constants (optim.hip, flow.hip, resample.hip)
# ---------------------------------------------------------------------------------------------------------------------
THREADS = 256
OPTIM_CAP = 8192               # ew_grid of optim.hip: adam_kernel, pack_conv3x3_kernel, the layout kernels
FLOW_CAP = 4096                # ew_grid of flow.hip: cfm_sample, axpy, fill
EMA_CAP = 2048                 # ema_grid: adam_ema_kernel, over float4
MSE_CAP = 1024                 # MSE_BLOCKS: mse_partial_kernel (over float4), ode_err_partial_kernel
CHUNK = 4096                   # elements a block of adam_multi_kernel owns
PIXSUM_GROUPS, PIXSUM_U = 4, 16     # pixel_sum_kernel: 4 pixel groups, 16 loads in flight
LIN_WAVES, LIN_UNROLL = 16, 4       # linear_bwd_x_kernel: 16 waves split n, four partial sums


def f32(x: float) -> float:
    """The value a C ``float`` parameter receives."""
    return struct.unpack("f", struct.pack("f", float(x)))[0]


def walk(total: int, cap: int) -> dict:
    """A grid-stride loop over ``total`` items: ``min(ceil(total / 256), cap)`` blocks of 256 threads."""
    grid = max(1, min(-(-total // THREADS), cap))
    stride = grid * THREADS
    rounds = -(-total // stride)
    last = total - (rounds - 1) * stride
    return {"grid": grid, "rounds": rounds, "last": last, "strides": rounds > 1, "partial_last": rounds > 1 and last < stride,
            "ragged": total % THREADS != 0}


def _seed(*key) -> int:
    return (sum((i + 1) * ord(ch) for i, ch in enumerate(repr(key))) * 7919) % (2 ** 31)


def _gen(*key) -> torch.Generator:
    return torch.Generator().manual_seed(_seed(*key))


def bf(t: torch.Tensor) -> torch.Tensor:
    return t.to(BF).float()


def with_ties(t: torch.Tensor) -> torch.Tensor:
    """Every third fp32 value moved onto a bf16 rounding tie (low 16 bits 0x8000; the kept bit above is odd or even as it
    falls, so round-to-nearest-even goes both ways)."""
    bits = t.float().contiguous().view(torch.int32).clone().reshape(-1)
    idx = torch.arange(0, bits.numel(), 3)
    bits[idx] = (bits[idx] & ~0xFFFF) | 0x8000
    return bits.view(torch.float32).reshape(t.shape)


# ---------------------------------------------------------------------------------------------------------------------
# Adam family
# ---------------------------------------------------------------------------------------------------------------------
ADAM_STRIDING = 2_097_152 + 1027
# the issue's ten sizes, and 6 (the only one with n & 3 == 2)
ADAM_SIZES = [1, 3, 4, 6, 255, 256, 257, 4095, 4096, 4097, ADAM_STRIDING]
ADAM_SCALARS = {
    "step1": dict(step=1, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, grad_scale=1.0, ema_weight=1.0),
    "step2-wd-gs": dict(step=2, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, grad_scale=0.5,
                        ema_weight=1.0 - 0.999),
    "step1000": dict(step=1000, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-5, grad_scale=1.0,
                     ema_weight=1.0 - 0.999),
    "step1e6": dict(step=10 ** 6, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, grad_scale=1.0,
                    ema_weight=0.75),
}
ADAM_V_STARTS = ("zeros", "positive")
ADAM_MAGNITUDES = (1.0, 1e-4, 1e-8)
ADAM_MULTI = {"one": [4097], "mixed": [1, 4095, 4096, 4097, 7, 12289], "33x1": [1] * 33}


def adam_form(n: int) -> dict:
    return {"plain": walk(n, OPTIM_CAP), "ema": walk(n >> 2, EMA_CAP), "tail": n & 3, "vector": n >> 2 > 0,
            "multi_blocks": -(-n // CHUNK), "multi_ragged": n % CHUNK != 0}


def adam_zero_block(n: int):
    """[z0, z1): g = m = v = 0 there (none below four elements)."""
    return (n // 2, n // 2 + max(1, n // 8)) if n >= 4 else (0, 0)


@functools.lru_cache(maxsize=6)
def adam_case(n: int, v_start: str, salt: int = 0) -> dict:
    """p, g, m, v, ema as fp32 CPU tensors.  Gradient magnitudes 1, 1e-4 and 1e-8 interleaved (with v = 0 at step 1 a
    gradient of 1e-8 makes sqrt(v) / sqrt(bc2) equal to eps: eps is half the denominator), a block of exact zeros."""
    gen = _gen("adam", n, v_start, salt)
    mag = torch.tensor(ADAM_MAGNITUDES, dtype=F32)[(torch.arange(n) + salt) % 3]
    p = torch.rand(n, generator=gen) - 0.5
    g = torch.randn(n, generator=gen) * mag
    if v_start == "positive":
        m = torch.randn(n, generator=gen) * 0.1 * mag
        v = torch.rand(n, generator=gen) * mag * mag
    else:
        m, v = torch.zeros(n), torch.zeros(n)
    ema = p + torch.randn(n, generator=gen) * 0.01
    z0, z1 = adam_zero_block(n)
    g[z0:z1] = 0.0
    m[z0:z1] = 0.0
    v[z0:z1] = 0.0
    return dict(p=p, g=g, m=m, v=v, ema=ema)


def adam_scalars(step, lr, beta1, beta2, eps, weight_decay, grad_scale, ema_weight=1.0) -> dict:
    """The scalars as s2s_adam_step forms them: every float parameter an fp32 value, the bias corrections in double."""
    b1, b2 = f32(beta1), f32(beta2)
    return dict(lr=f32(lr), b1=b1, b2=b2, eps=f32(eps), wd=f32(weight_decay), gs=f32(grad_scale), w=f32(ema_weight),
                bc1=1.0 - math.pow(b1, float(step)), bc2_sqrt=math.sqrt(1.0 - math.pow(b2, float(step))))


def lerp_ref(a: torch.Tensor, b: torch.Tensor, w: float, cd=F64) -> torch.Tensor:
    """torch.lerp's two-branch form (aten/src/ATen/native/Lerp.h)."""
    a, b, w = a.to(cd), b.to(cd), f32(w)
    return a + w * (b - a) if abs(w) < 0.5 else b - (b - a) * (1.0 - w)


def adam_ref(p, g, m, v, s: dict, cd=F64) -> dict:
    """torch.optim.Adam's single-tensor formula with coupled weight decay and a gradient scale; ``s`` = adam_scalars."""
    P, G, M, V = (t.to(cd) for t in (p, g, m, v))
    gi = G * s["gs"]
    if s["wd"] != 0.0:
        gi = gi + s["wd"] * P
    m2 = M + (gi - M) * (1.0 - s["b1"])
    v2 = V * s["b2"] + (1.0 - s["b2"]) * gi * gi
    denom = v2.sqrt() / s["bc2_sqrt"] + s["eps"]
    upd = (s["lr"] / s["bc1"]) * (m2 / denom)
    return dict(p=P - upd, m=m2, v=v2, upd=upd)


def adam_model(case: dict, scalars: dict, cd=F64) -> dict:
    s = adam_scalars(**scalars)
    out = adam_ref(case["p"], case["g"], case["m"], case["v"], s, cd)
    out["ema"] = lerp_ref(case["ema"], out["p"], s["w"], cd)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# weight packing
# ---------------------------------------------------------------------------------------------------------------------
PACK = [(32, 32), (64, 8), (24, 40), (40, 24), (3, 5), (64, 66), (96, 160), (512, 512)]
PACK_WANT_DGRAD = (True, False)
PACK_ORDERS = [[0, 1, 2, 3, 4, 5, 6, 7], [7, 2, 5, 0, 3, 6, 1, 4]]
PACK_NULL_WD = 2                      # position in the first order whose layer is packed without a data-gradient output
PACK_MISALIGNED = "w one float into a 16-byte aligned buffer"


def pack_elems(cout: int, cin: int):
    return 9 * ((cin + 31) // 32) * cout * 32, 9 * ((cout + 31) // 32) * cin * 32


def pack_form(cout: int, cin: int) -> dict:
    nco, nci = (cout + 31) // 32, (cin + 31) // 32
    inside = (cout // 32) * (cin // 32)            # tiles with all 32 x 32 (co, ci) inside the tensor
    vec = (cin * 9) % 4 == 0
    nf, nd = pack_elems(cout, cin)
    return {"tiles": nco * nci, "whole": inside if vec else 0, "element": nco * nci - (inside if vec else 0),
            "inside_unaligned_rows": inside if not vec else 0, "pad_ci": cin % 32 != 0, "pad_co": cout % 32 != 0,
            "single": walk(nf + nd, OPTIM_CAP), "single_fwd_only": walk(nf, OPTIM_CAP)}


@functools.lru_cache(maxsize=16)
def pack_case(cout: int, cin: int) -> torch.Tensor:
    return with_ties(torch.randn(cout, cin, 3, 3, generator=_gen("pack", cout, cin)) * 0.2)


def pack_ref(w: torch.Tensor, dtype):
    """(Wf, Wd) as flat fp32 tensors holding the T-rounded values, by reshape / permute / pad:
    Wf[cin/32][tap][cout][32] and Wd[cout/32][tap'][cin][32] = W[co][ci][8 - tap'], zero beyond Cin / Cout."""
    cout, cin = w.shape[:2]
    nco, nci = (cout + 31) // 32, (cin + 31) // 32
    w9 = round_to(w.reshape(cout, cin, 9).float(), dtype)
    a = F.pad(w9.permute(0, 2, 1), (0, nci * 32 - cin)).reshape(cout, 9, nci, 32).permute(2, 1, 0, 3)
    b = F.pad(w9.flip(2).permute(1, 2, 0), (0, nco * 32 - cout)).reshape(cin, 9, nco, 32).permute(2, 1, 0, 3)
    return a.contiguous().reshape(-1), b.contiguous().reshape(-1)


def pack_gather(w: torch.Tensor, dtype):
    """The same two layouts by a gather with the flat index formula of pack_conv3x3_kernel's documentation."""
    cout, cin = w.shape[:2]
    nf, nd = pack_elems(cout, cin)
    flat = round_to(w.reshape(-1).float(), dtype)
    i = torch.arange(nf)
    k, t = i & 31, i >> 5
    co, t = t % cout, t // cout
    tap, c = t % 9, t // 9
    ci = c * 32 + k
    wf = torch.where(ci < cin, flat[(co * cin + ci.clamp_max(cin - 1)) * 9 + tap], torch.zeros(()))
    j = torch.arange(nd)
    k, t = j & 31, j >> 5
    ci, t = t % cin, t // cin
    tap, c = t % 9, t // 9
    co = c * 32 + k
    wd = torch.where(co < cout, flat[(co.clamp_max(cout - 1) * cin + ci) * 9 + (8 - tap)], torch.zeros(()))
    return wf, wd


# ---------------------------------------------------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------------------------------------------------
LAYOUT = [(1, 8, 1, 1), (2, 16, 5, 7), (3, 24, 1, 13), (1, 8, 1, 2_097_152 + 333)]
LAYOUT_SLICES = [None, (8, 16), (16, 8)]           # dense; (channels before, channels after) of a wider buffer
LAYOUT_ACCUMULATE = (False, True)
LAYOUT_REFUSED = [("C", (1, 12, 2, 2), 16), ("ld", (1, 8, 2, 2), 20)]      # (what, (B, C, H, W), pixel stride)


def layout_form(shape) -> dict:
    B, C, H, W = shape
    return walk(B * (C // 8) * H * W, OPTIM_CAP)


@functools.lru_cache(maxsize=2)
def layout_case(shape) -> dict:
    gen = _gen("layout", shape)
    B, C, H, W = shape
    return dict(x=with_ties(torch.randn(shape, generator=gen)), base=torch.randn(shape, generator=gen))


def nchw_to_nhwc_ref(x: torch.Tensor, dtype) -> torch.Tensor:
    return round_to(x.float(), dtype).permute(0, 2, 3, 1).contiguous()


def nhwc_to_nchw_ref(x: torch.Tensor) -> torch.Tensor:
    return x.float().permute(0, 3, 1, 2).contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# pixel sum
# ---------------------------------------------------------------------------------------------------------------------
PIXSUM_HW = [1, 3, 4, 63, 64, 65, 127, 256, 1000]
PIXSUM_C = [8, 64, 72, 136]
PIXSUM_B = [1, 3]
PIXSUM_LAYOUTS = ("dense", "slice")
PIXSUM_ACCUMULATE = (False, True)


def pixsum_form(HW: int, C: int) -> dict:
    """Passes of the 16-deep unrolled loop and of the tail loop for each of the 4 pixel groups."""
    unrolled, tail = [], []
    for rg in range(PIXSUM_GROUPS):
        p, u, t = rg, 0, 0
        while p + PIXSUM_GROUPS * (PIXSUM_U - 1) < HW:
            p += PIXSUM_GROUPS * PIXSUM_U
            u += 1
        while p < HW:
            p += PIXSUM_GROUPS
            t += 1
        unrolled.append(u)
        tail.append(t)
    took = sum(1 for u in unrolled if u)
    return {"unrolled": unrolled, "tail": tail, "groups": "every" if took == 4 else "some" if took else "none",
            "blocks": -(-C // 64), "ragged_c": C % 64 != 0}


@functools.lru_cache(maxsize=4)
def pixsum_case(B: int, HW: int, C: int, tier: str) -> dict:
    gen = _gen("pixsum", B, HW, C, tier)
    if tier == "exact":
        x = torch.randint(-4, 5, (B, 1, HW, C), generator=gen).float()
        base = torch.randint(-8, 9, (B, C), generator=gen).float()
    else:
        x = bf(torch.randn(B, 1, HW, C, generator=gen) + 0.25)
        base = torch.randn(B, C, generator=gen)
    return dict(x=x, base=base)


def pixel_sum_ref(x: torch.Tensor, base, cd=F64) -> torch.Tensor:
    B, C = x.shape[0], x.shape[-1]
    s = x.to(cd).reshape(B, -1, C).sum(1)
    return s if base is None else base.to(cd) + s


# ---------------------------------------------------------------------------------------------------------------------
# time path
# ---------------------------------------------------------------------------------------------------------------------
TIME_DIMS = [4, 6, 32, 256, 1024]
TIME_B = [1, 5, 600]
# the issue's eight rows, and one with 49 <= N <= 63 (only there do SOME of the 16 waves take the unrolled loop)
LINEAR = [(1, 1, 1), (5, 32, 48), (3, 64, 64), (2, 65, 67), (3, 130, 3), (2, 100, 113), (7, 256, 1024), (1, 1024, 256),
          (2, 40, 56)]
LINEAR_BIAS = (True, False)
LINEAR_BWD_OPTS = [(db, need_dx, acc) for db in (True, False) for need_dx in (True, False) for acc in (False, True)]
SILU_N = [1, 255, 256, 257, 5120]
SILU_SPECIALS = [0.0, 1e-30, -1e-30, 20.0, -20.0, 88.0, -88.0, 104.0, -104.0]
SILU_UNDERFLOW = 2.0 ** -119     # below 2^-126 an fp32 result may be flushed; dh scales that by 1 + |h| < 2^7


def time_case(B: int) -> torch.Tensor:
    t = torch.rand(B, generator=_gen("time", B))
    t[0] = 0.0
    t[-1] = 1.0 if B > 1 else t[-1]
    return t


def time_embedding_ref(t: torch.Tensor, dim: int, cd=F64) -> torch.Tensor:
    half = dim // 2
    step = torch.log(torch.tensor(10000.0, dtype=cd)) / (half - 1)
    freq = torch.exp(torch.arange(half, dtype=cd) * -step)
    ang = t.to(cd).reshape(-1, 1) * freq[None, :]
    return torch.cat([ang.sin(), ang.cos()], dim=-1)


def linear_form(B: int, K: int, N: int) -> dict:
    """linear_bwd_x_kernel: wave wv starts at n = wv and takes the unrolled loop while n + 48 < N."""
    passes = []
    for wv in range(LIN_WAVES):
        n, u = wv, 0
        while n + (LIN_UNROLL - 1) * LIN_WAVES < N:
            n += LIN_UNROLL * LIN_WAVES
            u += 1
        passes.append(u)
    took = sum(1 for u in passes if u)
    return {"passes": passes, "waves": "every" if took == LIN_WAVES else "some" if took else "none",
            "bn_mod4": (B * N) % 4, "k_blocks": -(-K // 64), "k_ragged": K % 64 != 0}


@functools.lru_cache(maxsize=4)
def linear_case(B: int, K: int, N: int, tier: str) -> dict:
    gen = _gen("linear", B, K, N, tier)
    if tier == "exact":
        r = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gen).float()     # noqa: E731
        return dict(x=r(-3, 3, B, K), w=r(-2, 2, N, K), b=r(-4, 4, N), dy=r(-3, 3, B, N), dw0=r(-8, 8, N, K), db0=r(-8, 8, N))
    r = lambda *s: torch.rand(*s, generator=gen) - 0.5                                  # noqa: E731
    return dict(x=torch.rand(B, K, generator=gen), w=r(N, K), b=r(N), dy=r(B, N), dw0=r(N, K), db0=r(N))


def linear_fwd_ref(x, w, b, cd=F64) -> torch.Tensor:
    y = x.to(cd) @ w.to(cd).t()
    return y if b is None else y + b.to(cd)


def linear_bwd_ref(dy, x, w, cd=F64) -> dict:
    dy, x, w = dy.to(cd), x.to(cd), w.to(cd)
    return dict(dx=dy @ w, dw=dy.t() @ x, db=dy.sum(0))


def silu_case(n: int) -> dict:
    gen = _gen("silu", n)
    h = torch.randn(n, generator=gen) * 3
    k = min(n, len(SILU_SPECIALS))
    h[:k] = torch.tensor(SILU_SPECIALS[:k])
    return dict(h=h, da=torch.rand(n, generator=gen) - 0.5, specials=k)


def silu_fwd_ref(h, cd=F64) -> torch.Tensor:
    h = h.to(cd)
    return h / (1.0 + torch.exp(-h))


def silu_bwd_ref(h, da, cd=F64) -> torch.Tensor:
    h = h.to(cd)
    sg = 1.0 / (1.0 + torch.exp(-h))
    return da.to(cd) * sg * (1.0 + h * (1.0 - sg))


# ---------------------------------------------------------------------------------------------------------------------
# probability path and loss
# ---------------------------------------------------------------------------------------------------------------------
CFM_STRIDING = (3, 4 * (1_048_576 + 224) // 3)
CFM = [(B, ps) for B in (1, 3) for ps in (4, 12, 288)] + [CFM_STRIDING]
CFM_CASES = {"sigma0": (0.0, None), "sigma0-nan-eps": (0.0, "nan"), "sigma0.1": (0.1, "eps")}
CFM_REFUSED = [("per_sample % 4", (2, 6), 0), ("misaligned", (2, 8), 1)]       # (what, (B, per_sample), view offset)
MSE_STRIDING = 1_048_576 + 1200
MSE_COUNTS = [4, 864, 4096, MSE_STRIDING]
MSE_GRAD_SCALES = (1.0, 0.25)
MSE_WANT_DV = (True, False)


def cfm_form(B: int, ps: int) -> dict:
    return walk(B * ps // 4, FLOW_CAP)


def cfm_times(B: int):
    """t vectors with exact 0 and 1: one for B = 3, three for B = 1."""
    return [[0.0], [1.0], [0.3125 + 1e-3]] if B == 1 else [[0.0, 1.0, 0.3125 + 1e-3][:B]]


@functools.lru_cache(maxsize=2)
def cfm_case(B: int, ps: int) -> dict:
    gen = _gen("cfm", B, ps)
    r = lambda: torch.rand(B, ps, generator=gen) * 2 - 1                    # noqa: E731
    return dict(x0=r(), x1=r(), eps=torch.randn(B, ps, generator=gen))


def cfm_ref(x0, x1, t, eps, sigma: float, cd=F64):
    tb = t.to(cd).reshape(-1, 1)
    xt = tb * x1.to(cd) + (1.0 - tb) * x0.to(cd)
    if sigma != 0.0:
        xt = xt + f32(sigma) * eps.to(cd)
    return xt, x1.to(cd) - x0.to(cd)


def mse_form(count: int) -> dict:
    return walk(count // 4, MSE_CAP)


def mse_coef(grad_scale: float, count: int) -> float:
    """(float)(2.0 * (double)grad_scale / (double)count), the entry point's expression."""
    return f32(2.0 * f32(grad_scale) / count)


@functools.lru_cache(maxsize=2)
def mse_case(count: int, tier: str) -> dict:
    gen = _gen("mse", count, tier)
    if tier == "exact":
        u = torch.randint(-4, 5, (count,), generator=gen).float()
        d = (torch.randint(0, 2, (count,), generator=gen).float() * 2 - 1) * torch.randint(1, 3, (count,), generator=gen).float()
        return dict(v=u + d, u=u)
    return dict(v=torch.rand(count, generator=gen), u=torch.rand(count, generator=gen) * 2 - 1)


def mse_ref(v, u, grad_scale: float, cd=F64) -> dict:
    d = v.to(cd) - u.to(cd)
    return dict(loss=(d * d).mean(), dv=d * mse_coef(grad_scale, v.numel()))


# ---------------------------------------------------------------------------------------------------------------------
# sampler glue
# ---------------------------------------------------------------------------------------------------------------------
ERR_STRIDING = 262_144 + 513
ERR_N = [1, 255, 257, ERR_STRIDING]
ERR_TOLS = [(1e-5, 1e-5), (0.0, 1e-3), (1e-6, 0.0)]
AXPY_STRIDING = 4_194_304 + 308
AXPY_N = [4, 1020, AXPY_STRIDING]
AXPY_A = [1.0, -1.0, 0.5, 1.0 / 3.0, 0.0]
TICK_N = [1, 255, 256, 257, 1000]
TICK_TABLE = [0.0, 0.25, 1.0 / 3.0, 0.75, 1.0]
FILL_STRIDING = 1_048_576 + 99
FILL_N = [1, 257, FILL_STRIDING]


def err_form(n: int) -> dict:
    return walk(n, MSE_CAP)


def axpy_form(n: int) -> dict:
    return walk(n // 4, FLOW_CAP)


def fill_form(n: int) -> dict:
    return walk(n, FLOW_CAP)


@functools.lru_cache(maxsize=2)
def err_case(n: int) -> dict:
    """|y| bounded away from 0 (0.5 ... 1.5 with either sign), so that atol = 0 leaves every scale positive."""
    gen = _gen("err", n)
    y = lambda: (torch.rand(n, generator=gen) + 0.5) * (torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1)  # noqa: E731
    return dict(e=torch.randn(n, generator=gen) * 1e-5, y0=y(), y1=y())


def err_norm_ref(e, y0, y1, atol: float, rtol: float, cd=F64) -> torch.Tensor:
    sc = f32(atol) + f32(rtol) * torch.maximum(y0.to(cd).abs(), y1.to(cd).abs())
    r = e.to(cd) / sc
    return (r * r).mean().sqrt().reshape(1)


@functools.lru_cache(maxsize=2)
def axpy_case(n: int) -> dict:
    gen = _gen("axpy", n)
    return dict(x=torch.randn(n, generator=gen), y=torch.randn(n, generator=gen))


def axpy_ref(x, y, a: float, cd=F64) -> torch.Tensor:
    return x.to(cd) + f32(a) * y.to(cd)


def within_ulps(got: torch.Tensor, ref64: torch.Tensor, n: float) -> bool:
    """|got - ref| <= n fp32 ulps of the float64 reference, element by element."""
    g = got.detach().cpu().double().reshape(ref64.shape)
    return bool(torch.isfinite(g).all()) and bool(((g - ref64).abs() <= n * ulp(ref64, F32)).all())
