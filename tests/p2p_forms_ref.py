"""Shared reference, inputs and shape tables of the kernel-level tests of the bf16-only pix2pix forms
(test_p2p_forms_cpu.py, test_instnorm_forms_gpu.py, test_p2p_split_forms_gpu.py, test_p2p_conv_plans_gpu.py).

Everything here is plain torch on the CPU in fp64: the reference is torch's own operators under autograd on double
tensors, never a restatement of a kernel's formulas.  The shape tables live here so that the CPU tests can check, through
the library's host-only queries, that every shape reaches the launch plan it is listed for."""
import functools

import torch
import torch.nn.functional as F

EPS = 1e-5
BF16, F32 = torch.bfloat16, torch.float32

# the project's own max-norm relative bounds (conftest.relerr); one bf16 rounding is 2^-9
TOL_OUT = {F32: 1e-4, BF16: 4e-3}            # y, y2 (dx: twice that, as test_instnorm_gpu.py has it)
TOL_AFFINE = 1e-3                            # dgamma / dbeta
TOL_STAT = 1e-5                              # mean: * max(1, max|x|); invstd: relative
YARD_FACTOR = 4.0                            # margin over a measured yardstick, as in test_production_shapes_gpu.py
MIN_ABS_Z = 1e-3                             # precondition on the inputs of every backward comparison


# ----------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------
def _round(t, dtype):
    return t.to(dtype).double()


def decision_free_input(B, C, H, W, dtype, seed, offset=0.4, scale=1.0):
    """[B, C, H, W] in fp64 holding values of ``dtype``: per (sample, channel) the H*W values are shuffled +-pairs with
    magnitudes in [0.25, 2] (an odd count ends in one triple that sums to zero), then * scale + offset, then rounded to
    ``dtype``.  The plane's mean is the offset up to rounding, so no normalised value is near the LeakyReLU's kink."""
    g = torch.Generator().manual_seed(seed)
    n = H * W
    npair = n // 2 if n % 2 == 0 else (n - 3) // 2
    if n < 2:
        raise ValueError("a plane needs at least two pixels")
    m = torch.rand(B, C, npair, generator=g, dtype=torch.float64) * 1.75 + 0.25
    parts = [m, -m]
    if n % 2:
        a = torch.rand(B, C, 2, generator=g, dtype=torch.float64) * 0.75 + 0.25         # a, b in [0.25, 1], a + b <= 2
        parts += [a, -a.sum(-1, keepdim=True)]
    v = torch.cat(parts, -1)
    order = torch.rand(B, C, n, generator=g).argsort(-1)
    v = torch.gather(v, -1, order).reshape(B, C, H, W)
    return _round(v * scale + offset, dtype)


def affine_params(C, seed):
    """gamma with |gamma| in [0.5, 1.5] and both signs present, |beta| <= 0.05 (fp32 values in fp64)."""
    g = torch.Generator().manual_seed(seed)
    gamma = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0).double()
    sign[0], sign[1] = 1.0, -1.0
    beta = (torch.rand(C, generator=g, dtype=torch.float64) - 0.5) * 0.1
    return _round(gamma * sign, F32), _round(beta, F32)


def cotangent(B, C, H, W, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return _round(torch.rand(B, C, H, W, generator=g, dtype=torch.float64) - 0.5, dtype)


def min_abs_preactivation(x, gamma=None, beta=None):
    """min |z| of the fp64 pre-activation z = instance_norm(x) (* gamma + beta): what every backward test asserts to be
    >= MIN_ABS_Z before it launches anything."""
    return float(F.instance_norm(x.double(), weight=gamma, bias=beta, eps=EPS).abs().min())


# ----------------------------------------------------------------------------------------------------------------------
# InstanceNorm -> LeakyReLU in fp64
# ----------------------------------------------------------------------------------------------------------------------
def instnorm_reference(x, gamma, beta, slope, g=None, g2=None):
    """y = leaky_relu(z, slope), y2 = relu(z), z = instance_norm(x, gamma, beta); stats[4][B][C] = mean, 1/std, scale,
    shift.  With ``g`` (wrt y) and optionally ``g2`` (wrt y2): dx, dgamma, dbeta from autograd.  All fp64, NCHW."""
    x = x.double().detach().clone().requires_grad_(g is not None)
    gm = None if gamma is None else gamma.double().detach().clone().requires_grad_(g is not None)
    bt = None if beta is None else beta.double().detach().clone().requires_grad_(g is not None)
    z = F.instance_norm(x, weight=gm, bias=bt, eps=EPS)
    y, y2 = F.leaky_relu(z, slope), F.relu(z)
    xd = x.detach()
    mean = xd.mean((2, 3))
    invstd = (xd.var((2, 3), unbiased=False) + EPS).rsqrt()
    scale = invstd if gm is None else invstd * gm.detach()[None, :]
    shift = -mean * scale if bt is None else bt.detach()[None, :] - mean * scale
    out = {"y": y.detach(), "y2": y2.detach(), "stats": torch.stack([mean, invstd, scale, shift])}
    if g is not None:
        loss = (y * g.double()).sum()
        if g2 is not None:
            loss = loss + (y2 * g2.double()).sum()
        loss.backward()
        out["dx"] = x.grad
        if gm is not None:
            out["dgamma"], out["dbeta"] = gm.grad, bt.grad
    return out


@functools.lru_cache(maxsize=1)             # the largest case holds ~0.3 GB of fp64 tensors
def instnorm_case(B, C, H, W, dtype, seed, offset, scale, affine, slope, with_g2):
    """Inputs and fp64 reference of one case, computed once and shared (callers must not modify what they get)."""
    x = decision_free_input(B, C, H, W, dtype, seed, offset, scale)
    gamma, beta = affine_params(C, seed + 1) if affine else (None, None)
    g = cotangent(B, C, H, W, dtype, seed + 2)
    g2 = cotangent(B, C, H, W, dtype, seed + 3) if with_g2 else None
    return x, gamma, beta, g, g2, instnorm_reference(x, gamma, beta, slope, g, g2)


# ----------------------------------------------------------------------------------------------------------------------
# convolutions in fp64 on rounded operands
# ----------------------------------------------------------------------------------------------------------------------
def conv_operands(B, cin, Hi, Wi, cout, seed, transposed=False):
    """bf16-valued fp64 operands: x [B, cin, Hi, Wi], w (Conv2d [cout, cin, 4, 4] or ConvTranspose2d [cin, cout, 4, 4])
    scaled so that the output is O(1), bias [cout] (fp32-valued)."""
    g = torch.Generator().manual_seed(seed)
    x = _round(torch.randn(B, cin, Hi, Wi, generator=g, dtype=torch.float64), BF16)
    fan = (4.0 if transposed else 16.0) * cin
    ws = (cin, cout, 4, 4) if transposed else (cout, cin, 4, 4)
    w = _round(torch.randn(*ws, generator=g, dtype=torch.float64) / fan ** 0.5, BF16)
    b = _round(torch.randn(cout, generator=g, dtype=torch.float64) * 0.5, F32)
    return x, w, b


def conv_s2_reference(x, w, b):
    return F.conv2d(x.double(), w.double(), None if b is None else b.double(), stride=2, padding=1)


def convT_s2_reference(x, w, b):
    return F.conv_transpose2d(x.double(), w.double(), None if b is None else b.double(), stride=2, padding=1)


# ----------------------------------------------------------------------------------------------------------------------
# shape tables
# ----------------------------------------------------------------------------------------------------------------------
# InstanceNorm, single-launch forms without affine: (dtype, B, C, H, W, with_y2, with_g2, slope).  H*W in {2, 63, 64, 65,
# 1023, 1024} = 1, 2 and all 16 register iterations of in_small_res_kernel and their edges; C in {8, 24, 64, 72, 264} =
# a channel tail inside a 32- and a 64-channel workgroup, one and several workgroups per sample.  Every H*W, every C, both
# y2 settings and both slopes occur with the bf16 backward without g2 (<true,false>), with g2 (<true,true>), and with
# the fp32 kernel; the bf16 forward <false,false> runs in all of the bf16 rows.
IN_SINGLE = [
    (BF16, 2, 8, 1, 2, False, False, 0.2), (BF16, 1, 24, 7, 9, True, False, 0.0), (BF16, 2, 64, 8, 8, False, False, 0.0),
    (BF16, 1, 72, 5, 13, True, False, 0.2), (BF16, 1, 264, 31, 33, False, False, 0.2), (BF16, 2, 72, 32, 32, True, False, 0.0),
    (BF16, 1, 264, 1, 2, True, True, 0.0), (BF16, 2, 72, 7, 9, False, True, 0.2), (BF16, 1, 24, 8, 8, True, True, 0.2),
    (BF16, 2, 8, 5, 13, False, True, 0.0), (BF16, 1, 64, 31, 33, True, True, 0.2), (BF16, 1, 24, 32, 32, False, True, 0.0),
    (F32, 2, 24, 1, 2, True, True, 0.2), (F32, 1, 264, 7, 9, False, False, 0.0), (F32, 1, 8, 8, 8, True, False, 0.2),
    (F32, 2, 64, 5, 13, False, True, 0.0), (F32, 1, 72, 31, 33, True, True, 0.0), (F32, 1, 24, 32, 32, False, False, 0.2),
]
# the switch: 1025 pixels without affine is the first map of the three-launch form
IN_SWITCH = [
    (BF16, 2, 72, 25, 41, True, True, 0.2), (BF16, 1, 24, 25, 41, False, False, 0.0),
    (F32, 1, 72, 25, 41, True, True, 0.0), (F32, 2, 8, 25, 41, False, False, 0.2),
]
# three-launch form with several blocks and more than one, ragged, trip of the grid-stride loop:
# (dtype, B, C, H, W, affine, with_y2, with_g2, slope); the inequality blocks * (256 / pcb) < H*W is asserted from
# s2s_instnorm_blocks by the tests
IN_MULTI = [
    (BF16, 8, 264, 50, 61, False, True, True, 0.2), (F32, 8, 264, 50, 61, False, False, False, 0.0),
    (BF16, 32, 264, 23, 29, True, False, False, 0.0), (F32, 32, 264, 23, 29, True, True, True, 0.2),
    (BF16, 32, 264, 23, 29, True, True, True, 0.2),
]
# three-launch form at a small map (affine given) on the data of a single-launch case: (dtype, B, C, H, W, with_y2, with_g2, slope)
IN_SMALL_AFFINE = [
    (BF16, 2, 72, 8, 8, True, True, 0.2), (BF16, 1, 24, 32, 32, False, False, 0.0), (F32, 2, 72, 7, 9, True, True, 0.2),
]
# conditioning (offset 8, scale 0.5), one per form: (dtype, B, C, H, W, affine)
IN_COND = [
    (BF16, 2, 72, 31, 33, False), (F32, 2, 72, 31, 33, False), (BF16, 2, 72, 50, 61, False), (F32, 2, 72, 50, 61, False),
    (F32, 2, 72, 23, 29, True),
]
IN_COND_OFFSET, IN_COND_SCALE = 8.0, 0.5


def in_pcb(C):
    """Channel pieces of 8 per workgroup of the three-launch form (instnorm.hip)."""
    p = 1
    while p < 32 and p * 8 < C:
        p <<= 1
    return p


def all_instnorm_inputs():
    """(B, C, H, W, dtype, seed, offset, scale, affine) of every backward comparison in the GPU tables."""
    out = []
    for i, (dt, B, C, H, W, _y2, _g2, _s) in enumerate(IN_SINGLE):
        out.append((B, C, H, W, dt, 100 + i, 0.4, 1.0, False))
    for i, (dt, B, C, H, W, _y2, _g2, _s) in enumerate(IN_SWITCH):
        out.append((B, C, H, W, dt, 200 + i, 0.4, 1.0, False))
    for i, (dt, B, C, H, W, aff, _y2, _g2, _s) in enumerate(IN_MULTI):
        out.append((B, C, H, W, dt, 300 + i, 0.4, 1.0, aff))
    for i, (dt, B, C, H, W, _y2, _g2, _s) in enumerate(IN_SMALL_AFFINE):
        out.append((B, C, H, W, dt, 400 + i, 0.4, 1.0, False))
    for i, (dt, B, C, H, W, aff) in enumerate(IN_COND):
        out.append((B, C, H, W, dt, 500 + i, IN_COND_OFFSET, IN_COND_SCALE, aff))
    return out


# Stride-2 convolutions, one case per launch plan: (plan, B, H, W, C, Cin) with H x W the OUTPUT map of the forward
# (s2s_conv4x4s2_plan) and the INPUT map of the transposed form (s2s_convt4x4s2_plan), C the output channels.  Plans 0, 2
# and 4 need >= 448 workgroups of the next-larger tile, which sets their batch.
CONV_FWD_PLANS = [
    (0, 112, 3, 40, 136, 8), (1, 2, 3, 40, 64, 8), (2, 56, 6, 40, 136, 8), (3, 2, 6, 40, 136, 8),
    (4, 112, 3, 6, 512, 8), (5, 2, 3, 6, 72, 8), (6, 3, 4, 8, 72, 16),
]
CONV_T_PLANS = [
    (0, 28, 3, 40, 192, 8), (1, 2, 3, 20, 64, 8), (2, 28, 6, 20, 192, 8), (3, 2, 6, 20, 128, 8),
    (4, 56, 3, 6, 192, 8), (5, 2, 3, 6, 64, 8), (6, 3, 4, 8, 128, 64),
]
# non-flat split-K, one each: (plan, minimal split, B, H, W, C, Cin)
CONV_FWD_SPLIT = [(5, 2, 2, 3, 6, 72, 64)]
CONV_T_SPLIT = [(3, 2, 1, 6, 20, 64, 256)]

# Deferred split-K into the single-launch InstanceNorm: (kind, plan, min split, B, H, W, C, Cin); H x W as above.
#   flat at C <= 64 and C > 64 (the latter with a tail in the 64-channel workgroup), plan 5 at 3 x 6 and plan 1 / 3 at
#   3 x 20 / 6 x 20 non-flat, a split of at least 3.
SPLIT_FWD = [
    ("conv", 6, 2, 2, 4, 8, 64, 16), ("conv", 6, 3, 1, 4, 4, 72, 64), ("conv", 5, 2, 2, 3, 6, 72, 64),
    ("conv", 1, 2, 1, 3, 20, 64, 64), ("conv", 3, 2, 1, 6, 20, 72, 64),
]
SPLIT_T = [
    ("convT", 6, 2, 2, 4, 8, 64, 64), ("convT", 6, 3, 1, 2, 2, 128, 256), ("convT", 5, 2, 1, 3, 6, 64, 256),
    ("convT", 3, 2, 1, 6, 20, 64, 256),
]

# 4x4 weight gradients (ops.convkxk_wgrad, bf16 operands, fp32 result): (name, ks, x_plain, B, H, W, C, Cout) with H x W the
# map of dy; ks = 2 is the stride-2 layer (x plain [B, 2H, 2W, C] or its space-to-depth image), ks = 4 the stride-1 layer
# (x [B, H+1, W+1, C]).  One pixel tile is 8 x 16; split z of S owns tiles z, z + S, ...
WGRAD = [
    ("dma_plain_uneven", 2, True, 1, 19, 100, 64, 512),      # S = 8 over 21 tiles: 3, 3, 3, 3, 3, 2, 2, 2; fold<1>
    ("dma_s2d_uneven", 2, False, 1, 19, 100, 64, 512),       # the same layer from the space-to-depth image
    ("dma_plain_fold4", 2, True, 2, 17, 40, 16, 64),         # S = 18 >= 16, one 64-channel group x 64 rows: fold<4>
    ("flat", 2, True, 17, 8, 8, 32, 72),                     # 1088 pixels of 8 x 8 maps: 9 tiles of the flattened batch
    ("flat_c8", 2, True, 2, 4, 4, 8, 24),                    # C % 16 != 0 keeps a small batch on the flat kernel
    ("small_1tile", 2, True, 2, 8, 8, 16, 72),               # 128 pixels: conv2x2_wgrad_small_kernel, ntiles == 1
    ("small_3tiles", 2, True, 5, 8, 8, 32, 64),              # 320 pixels: ntiles == 3, the last one ragged
    ("rows_uneven", 4, False, 1, 9, 70, 256, 512),           # S = 3 over 10 tiles: 4, 3, 3; fold<1>
    ("rows_fold4", 4, False, 2, 17, 40, 16, 24),             # S = 18 >= 16: fold<4>
]
WGRAD_UNEVEN = {"dma_plain_uneven": (8, 21), "dma_s2d_uneven": (8, 21), "rows_uneven": (3, 10)}     # name: (S, tiles)
WGRAD_FOLD4 = {"dma_plain_fold4": 18, "rows_fold4": 18}                                              # name: S
# layout 0 (tap-major grad[ks*ks][Cout][cin]) through the raw entry point: (ks, B, H, W, cin, Cout)
WGRAD_LAYOUT0 = [(4, 2, 9, 20, 16, 24), (2, 2, 9, 20, 32, 24)]


def wgrad_tiles(B, H, W):
    return B * ((H + 7) // 8) * ((W + 15) // 16)


@functools.lru_cache(maxsize=2)
def wgrad_case(ks, B, H, W, C, Cout, seed):
    """bf16-valued fp64 operands and the fp64 weight gradient [Cout, C, 4, 4] of Conv2d(4, stride 2 (ks = 2) or 1, pad 1)."""
    g = torch.Generator().manual_seed(seed)
    hi, wi = (2 * H, 2 * W) if ks == 2 else (H + 1, W + 1)
    x = _round(torch.randn(B, C, hi, wi, generator=g, dtype=torch.float64), BF16)
    dy = _round(torch.randn(B, Cout, H, W, generator=g, dtype=torch.float64), BF16)
    ref = torch.nn.grad.conv2d_weight(x, (Cout, C, 4, 4), dy, stride=2 if ks == 2 else 1, padding=1)
    return x, dy, ref


# conv_small.hip forward (ops.convsm_fwd): the shapes of test_conv_small_gpu.py plus one whose channel count is no
# multiple of the 64 channels a norm workgroup takes elsewhere.  mode 1: (B, ho, cin, cout, slope), ho x ho the output
# map; mode 2: (B, hi, cin, cout), hi x hi the input map.
CONVSM_FWD = [(16, 4, 512, 512, 0.2), (16, 2, 512, 512, 0.2), (3, 8, 64, 32, 0.2), (5, 4, 128, 48, 0.0), (2, 2, 256, 16, 0.2),
              (3, 4, 64, 80, 0.2)]
CONVSM_T = [(16, 4, 1024, 512), (16, 2, 1024, 512), (16, 1, 512, 512), (5, 2, 64, 32), (3, 1, 128, 16), (3, 2, 64, 80)]
