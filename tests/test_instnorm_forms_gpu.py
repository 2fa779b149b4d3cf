"""Every form of the fused InstanceNorm2d + LeakyReLU (instnorm.hip) at its boundaries, against torch's own operators under
autograd in fp64 on the dtype-rounded inputs (tests/p2p_forms_ref.py):

  * the single-launch forms -- bf16 in_small_res_kernel<false,false>, <true,false>, <true,true> at 1, 2 and all 16 of its
    register iterations, fp32 in_small_kernel -- with and without the second output y2 = relu(z) and the second gradient
    g2, at slope 0.2 and 0.0, with a channel tail inside a 32- and a 64-channel workgroup;
  * the 1024 / 1025-pixel switch to the three-launch form;
  * the three-launch form with several blocks and more than one, ragged, trip of its grid-stride loop, with affine
    parameters of both signs, y2 and g2;
  * the three-launch form on a small map (which it takes when affine parameters are given);
  * a badly conditioned input (level 8, spread 0.5) through each form.

Operands are always channel slices of wider NHWC buffers, each with its own pixel stride; the channels outside the slices
hold a sentinel that must come back unchanged.  The inputs are decision-free: every backward comparison first asserts, on
the CPU, that no fp64 pre-activation is within 1e-3 of the LeakyReLU's kink, so the max-norm bounds on dx never hang on a
knife edge.  Bounds (max-norm relative, conftest.relerr): fp32 1e-4; bf16-stored y / y2 4e-3 (one bf16 rounding is
2^-9); dx twice the output bound; dgamma / dbeta 1e-3; mean 1e-5 * max(1, max|x|), 1/std 1e-5 relative."""
import pytest
import torch
import torch.nn.functional as F

import p2p_forms_ref as R
from conftest import relerr

pytestmark = pytest.mark.gpu
DEV = "cuda"
IN_SMALL_HW = 1024


def _ids(table):
    return ["-".join(str(v).replace("torch.", "") for v in row) for row in table]


class _Sliced:
    """An NHWC operand as channels [lo, lo + C) of a buffer of lo + C + hi channels filled with ``sentinel``."""

    def __init__(self, B, H, W, C, dtype, lo, hi, sentinel, value=None):
        self.lo, self.C, self.sentinel = lo, C, sentinel
        self.buf = torch.full((B, H, W, lo + C + hi), sentinel, dtype=dtype, device=DEV)
        self.view = self.buf[..., lo:lo + C]
        if value is not None:                                  # NCHW fp64 on the CPU, already holding values of dtype
            self.view.copy_(value.permute(0, 2, 3, 1).to(dtype))

    def nchw(self):
        return self.view.double().cpu().permute(0, 3, 1, 2)

    def assert_rest_untouched(self):
        rest = torch.cat([self.buf[..., :self.lo], self.buf[..., self.lo + self.C:]], -1)
        assert bool((rest == self.sentinel).all()), "channels outside the slice were written"


def _launch(dtype, x, gamma, beta, g, g2, slope, with_y2, accumulate_too=True):
    """Forward and backward through the raw entry points, every operand a slice; returns NCHW fp64 CPU tensors."""
    from stain2stain_amd import _native, ops
    L = _native.lib()
    B, C, H, W = x.shape
    xs = _Sliced(B, H, W, C, dtype, 8, 16, 3.0, x)
    ys = _Sliced(B, H, W, C, dtype, 16, 8, -5.0)
    y2s = _Sliced(B, H, W, C, dtype, 24, 8, 7.0) if with_y2 else None
    gs = _Sliced(B, H, W, C, dtype, 0, 8, 2.0, g)
    g2s = _Sliced(B, H, W, C, dtype, 8, 0, -3.0, g2) if g2 is not None else None
    dxs = _Sliced(B, H, W, C, dtype, 8, 8, 9.0)
    gm = None if gamma is None else gamma.float().to(DEV)
    bt = None if beta is None else beta.float().to(DEV)
    nb = L.s2s_instnorm_blocks(B, H, W, C)
    assert nb >= 1
    work = torch.empty(2 * B * C * nb + 2 * B * C, dtype=torch.float32, device=DEV)
    stats = torch.full((4, B, C), float("nan"), dtype=torch.float32, device=DEV)
    px, ldx = ops._nhwc(xs.view)
    py, ldy = ops._nhwc(ys.view)
    p2, ld2 = ops._nhwc(y2s.view) if with_y2 else (0, 8)
    assert ldx != C and ldy != C and (not with_y2 or ld2 != C)
    rc = L.s2s_instnorm_lrelu_fwd2(ops._dt(xs.view), px, ldx, ops._f32(gm), ops._f32(bt), py, ldy, p2, ld2, ops._f32(work),
                                   ops._f32(stats), B, H, W, C, R.EPS, slope, ops._stream())
    assert rc == 0
    out = {"y": ys.nchw(), "stats": stats.double().cpu()}
    if with_y2:
        out["y2"] = y2s.nchw()
    pg, ldg = ops._nhwc(gs.view)
    pg2, ldg2 = ops._nhwc(g2s.view) if g2s is not None else (0, 8)
    pdx, lddx = ops._nhwc(dxs.view)
    assert ldg != C and lddx != C and (g2s is None or ldg2 != C)
    dg = torch.full((C,), 3.0, device=DEV) if gamma is not None else None
    db = torch.full((C,), -3.0, device=DEV) if gamma is not None else None

    def bwd(acc):
        r = L.s2s_instnorm_lrelu_bwd2(ops._dt(xs.view), pg, ldg, pg2, ldg2, px, ldx, ops._f32(stats), pdx, lddx, ops._f32(dg),
                                      ops._f32(db), acc, ops._f32(work), B, H, W, C, R.EPS, slope, ops._stream())
        assert r == 0
    bwd(0)
    out["dx"] = dxs.nchw()
    if gamma is not None:
        out["dgamma"], out["dbeta"] = dg.double().cpu(), db.double().cpu()
        if accumulate_too:
            bwd(1)
            out["dgamma_acc"], out["dbeta_acc"] = dg.double().cpu(), db.double().cpu()
            assert torch.equal(dxs.nchw(), out["dx"])
    for s in (xs, ys, y2s, gs, g2s, dxs):
        if s is not None:
            s.assert_rest_untouched()
    assert torch.equal(xs.nchw(), x.double()) and torch.equal(gs.nchw(), g.double())      # inputs are left alone
    return out


def _elementwise_rel(a, b):
    return float(((a - b).abs() / b.abs()).max())


def _errors(out, ref, x):
    e = {"y": relerr(out["y"], ref["y"]), "dx": relerr(out["dx"], ref["dx"]),
         "mean": float((out["stats"][0] - ref["stats"][0]).abs().max()) / max(1.0, float(x.abs().max())),
         "invstd": _elementwise_rel(out["stats"][1], ref["stats"][1]),
         "scale": _elementwise_rel(out["stats"][2], ref["stats"][2]),
         "shift": float((out["stats"][3] - ref["stats"][3]).abs().max())
         / (max(1.0, float(x.abs().max())) * float(ref["stats"][2].abs().max()))}
    if "y2" in out:
        e["y2"] = relerr(out["y2"], ref["y2"])
    for k in ("dgamma", "dbeta"):
        if k in out:
            e[k] = relerr(out[k], ref[k])
            if k + "_acc" in out:
                e[k + "_acc"] = relerr(out[k + "_acc"], 2 * ref[k])
    return e


def _bounds(dtype):
    t = R.TOL_OUT[dtype]
    return {"y": t, "y2": t, "dx": 2 * t, "mean": R.TOL_STAT, "invstd": R.TOL_STAT, "scale": R.TOL_STAT, "shift": R.TOL_STAT,
            "dgamma": R.TOL_AFFINE, "dbeta": R.TOL_AFFINE, "dgamma_acc": R.TOL_AFFINE, "dbeta_acc": R.TOL_AFFINE}


def _hold(errors, bounds, what):
    print(what, {k: f"{v:.2e}" for k, v in errors.items()})
    bad = {k: (v, bounds[k]) for k, v in errors.items() if not v < bounds[k]}
    assert not bad, f"{what}: (error, bound) {bad}"


def _case(B, C, H, W, dtype, seed, affine, slope, with_g2, offset=0.4, scale=1.0):
    x, gamma, beta, g, g2, ref = R.instnorm_case(B, C, H, W, dtype, seed, offset, scale, affine, slope, with_g2)
    assert R.min_abs_preactivation(x, gamma, beta) >= R.MIN_ABS_Z              # precondition on the inputs, not a tolerance
    return x, gamma, beta, g, g2, ref


@pytest.mark.parametrize("row", list(enumerate(R.IN_SINGLE)), ids=_ids(R.IN_SINGLE))
def test_single_launch_forms(row):
    """The two-pixel maps are the hard ones for dx: dz - mean(dz) is collinear with xhat there, so dx is what a cancellation
    down to eps / (var + eps) leaves (max |dx| 5e-5 in the fp32 case), and an fp32 1/std is not enough for it -- torch's own
    fp32 autograd on the CPU is off by 2.7e-3 of max |dx| in that case, fp64 arithmetic on the fp32-rounded mean and 1/std
    by 1.5e-3.  The fp32 backward therefore takes its statistics again from x in fp64 (in_small_bwd_kernel: 2.8e-8 on an
    MI355X, 2.1e-3 before); bf16 has the 8e-3 of its storage (2.0e-3 measured)."""
    i, (dtype, B, C, H, W, with_y2, with_g2, slope) = row
    assert H * W <= IN_SMALL_HW
    x, gamma, beta, g, g2, ref = _case(B, C, H, W, dtype, 100 + i, False, slope, with_g2)
    out = _launch(dtype, x, None, None, g, g2, slope, with_y2)
    _hold(_errors(out, ref, x), _bounds(dtype), "single-launch")


@pytest.mark.parametrize("row", list(enumerate(R.IN_SWITCH)), ids=_ids(R.IN_SWITCH))
def test_first_map_of_the_three_launch_form(row):
    i, (dtype, B, C, H, W, with_y2, with_g2, slope) = row
    assert H * W == IN_SMALL_HW + 1
    x, gamma, beta, g, g2, ref = _case(B, C, H, W, dtype, 200 + i, False, slope, with_g2)
    out = _launch(dtype, x, None, None, g, g2, slope, with_y2)
    _hold(_errors(out, ref, x), _bounds(dtype), "three-launch at 1025 pixels")


@pytest.mark.parametrize("row", list(enumerate(R.IN_MULTI)), ids=_ids(R.IN_MULTI))
def test_three_launch_form_with_several_blocks_and_trips(row):
    from stain2stain_amd import _native
    i, (dtype, B, C, H, W, affine, with_y2, with_g2, slope) = row
    nb = _native.lib().s2s_instnorm_blocks(B, H, W, C)
    lanes = 256 // R.in_pcb(C)
    assert nb > 1 and nb * lanes < H * W and (H * W) % (nb * lanes) != 0          # > 1 block, > 1 trip, ragged last trip
    x, gamma, beta, g, g2, ref = _case(B, C, H, W, dtype, 300 + i, affine, slope, with_g2)
    if affine:
        assert bool((gamma < 0).any()) and bool((gamma > 0).any())
    out = _launch(dtype, x, gamma, beta, g, g2, slope, with_y2)
    _hold(_errors(out, ref, x), _bounds(dtype), "three-launch, several trips")


@pytest.mark.parametrize("row", list(enumerate(R.IN_SMALL_AFFINE)), ids=_ids(R.IN_SMALL_AFFINE))
def test_three_launch_form_at_a_small_map(row):
    """gamma = 1, beta = 0 sends a small map through the three-launch form; the same data without affine parameters takes
    the single-launch form.  Both are held to the reference; their own difference is only reported."""
    i, (dtype, B, C, H, W, with_y2, with_g2, slope) = row
    assert H * W <= IN_SMALL_HW
    x, _, _, g, g2, ref = _case(B, C, H, W, dtype, 400 + i, False, slope, with_g2)
    one, zero = torch.ones(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    ref3 = R.instnorm_reference(x, one, zero, slope, g, g2)
    assert relerr(ref3["dx"], ref["dx"]) < 1e-12
    three = _launch(dtype, x, one, zero, g, g2, slope, with_y2)
    single = _launch(dtype, x, None, None, g, g2, slope, with_y2)
    _hold(_errors(three, ref3, x), _bounds(dtype), "three-launch at a small map")
    _hold(_errors(single, ref, x), _bounds(dtype), "single-launch on the same data")
    print("three-launch against single-launch:", {k: f"{relerr(three[k], single[k]):.2e}" for k in ("y", "dx", "stats")})


def _fp32_yardstick(x, gamma, beta, g, g2, slope, ref):
    """torch's own fp32 operators on the CPU on the same inputs, against the fp64 reference."""
    x32 = x.float().requires_grad_(True)
    gm = None if gamma is None else gamma.float().requires_grad_(True)
    bt = None if beta is None else beta.float().requires_grad_(True)
    z = F.instance_norm(x32, weight=gm, bias=bt, eps=R.EPS)
    y, y2 = F.leaky_relu(z, slope), F.relu(z)
    ((y * g.float()).sum() + (y2 * g2.float()).sum()).backward()
    xd = x32.detach()
    mean, invstd = xd.mean((2, 3)), (xd.var((2, 3), unbiased=False) + R.EPS).rsqrt()
    scale = invstd if gm is None else invstd * gm.detach()[None]
    shift = -mean * scale if bt is None else bt.detach()[None] - mean * scale
    out = {"y": y.detach().double(), "y2": y2.detach().double(), "dx": x32.grad.double(),
           "stats": torch.stack([mean, invstd, scale, shift]).double()}
    if gm is not None:
        out["dgamma"], out["dbeta"] = gm.grad.double(), bt.grad.double()
    return _errors(out, ref, x)


@pytest.mark.parametrize("row", list(enumerate(R.IN_COND)), ids=_ids(R.IN_COND))
def test_badly_conditioned_input(row):
    """Level 8, spread 0.5: E[x^2] - mean^2 loses about 2^10 of an fp32 sum's 2^24.  The single-launch forms shift their
    sums by the plane's first pixel; the three-launch form takes plain fp32 partial sums per thread and adds those in
    fp64.  Bound per quantity: 4 x what torch's own fp32 F.instance_norm / leaky_relu / autograd on the CPU deviates from
    the fp64 reference on the same inputs (YARD_FACTOR of test_production_shapes_gpu.py), or the bound of the ordinary
    cases, whichever is larger.

    Measured on an MI355X (yardstick -> kernel), 1/std relative error, the quantity the conditioning acts on:
      single-launch bf16 31x33          1.0e-07 -> 3.7e-08        single-launch fp32 31x33          1.0e-07 -> 5.8e-08
      three-launch  bf16 50x61          9.7e-08 -> 3.6e-08        three-launch  fp32 50x61          1.1e-07 -> 2.2e-06
      three-launch  fp32 23x29 affine   9.5e-08 -> 4.2e-06
    so the yardstick never lifts a bound here: 4 x 1e-7 is below the ordinary 1e-5, which the unshifted three-launch form
    keeps with a factor of two to spare (its y and dx follow 1/std: 2.2e-6 and 3.3e-6 against 1e-4 and 2e-4; torch
    6.9e-7 / 1.6e-7 at most).  bf16 values at level 8 are multiples of 2^-5, so the bf16 sums are exact."""
    i, (dtype, B, C, H, W, affine) = row
    x, gamma, beta, g, g2, ref = _case(B, C, H, W, dtype, 500 + i, affine, 0.2, True, R.IN_COND_OFFSET, R.IN_COND_SCALE)
    yard = _fp32_yardstick(x, gamma, beta, g, g2, 0.2, ref)
    print("yardstick (torch fp32 on the CPU)", {k: f"{v:.2e}" for k, v in yard.items()})
    out = _launch(dtype, x, gamma, beta, g, g2, 0.2, True, accumulate_too=False)
    ordinary = _bounds(dtype)
    err = _errors(out, ref, x)
    _hold(err, {k: max(R.YARD_FACTOR * yard[k], ordinary[k]) for k in err}, "conditioning")
