"""The weight-gradient kernels of the CFM / multitask step, every launch form, against float64 (tables, references and
yardsticks: tests/wgrad_forms_ref.py; the forms the tables must contain: tests/test_wgrad_forms_cpu.py):

  * ops.conv3x3_wgrad: conv3x3_wgrad_dma_kernel (bf16) and conv3x3_wgrad_kernel<float> with tile walks of 1 to 6 tiles per
    split, both workgroup orders, both folds;
  * ops.stem_wgrad: more tiles than workgroups, two channel groups, Cout tails, both loops of its fold;
  * ops.head_fwd / ops.head_bwd: head_lanes_kernel with 1 ... 64 lanes per pixel, the one-thread-per-pixel kernels with 4
    and 8 outputs, the block cap of the backward, the refused shapes.

Every row runs in bf16 and in fp32, on poisoned memory (torch.empty filled with NaN, 0xFF in every ops._workspace slab),
with dense operands -- accumulate = False into a buffer of random values, then accumulate = True into another, which
must give prefill + reference -- and once more with every operand that has a pixel stride as a channel slice of a wider
NaN-filled buffer (dy with lddy > Cout, x0 and x1 from two buffers of different strides, the head's x and dx), after which
the channels around the slices must still be NaN.

Bounds.  Hard bounds are the project's own: fp32 outputs (dW, db, the head's v and its fp32 dx) 1e-4 in the max norm
(test_ops_gpu.py) and 1e-4 in L2 (test_stepwise_bf16_gpu.py), the bf16-stored dx of the head 4e-3 / 2.2e-3.  On top of
them the weight gradients (and the head's v) are held to a multiple K of the YARDSTICK: the deviation from float64 of the
same quantity computed by torch on the CPU in fp32 (floored at 1e-7), which is 1e-7 ... 3e-6 here, two decades under the
hard bound.  The kernels sum in another order (splits, the MFMA's tree, the fold), so a small factor is expected; K is 4 x
the largest ratio measured on an MI355X, rounded up to a power of two, and never more than 64.  Largest ratios measured
(max norm / L2), with the row that gave them:

  kernel, dtype        max    L2    row                                              K
  conv3x3 dW, bf16     0.83   0.81  one_split (one workgroup column walks 6 tiles)   4
  conv3x3 dW, fp32     0.89   0.85  one_split                                        4
  stem dW, bf16        0.79   0.57  partial_15 / partial_17x33                       4
  stem dW, fp32        1.13   0.86  partial_15                                       8
  head dW, bf16        1.31   1.05  C 64, Cout 1, 63 pixels / C 72, Cout 1           8
  head dW, fp32        1.37   1.09  C 72, Cout 3, 63 pixels (fallback, 4 outputs)    8
  head v, bf16         3.26   1.98  C 72, Cout 3, 40000 pixels / C 72, Cout 1        16
  head v, fp32         2.77   2.12  C 72, Cout 3, 40000 pixels / C 256, Cout 3       16

(The head's v is a chain of C fused multiply-adds in one order where torch's matmul blocks the sum: the largest factor.)
The bf16-stored dx of the head measured 3.83e-3 in the max norm, 1.73e-3 in L2 over the cases of 500 elements and more,
and 0.500 bf16 ulps for the worst element (see _hold_bf16_dx for the one-pixel cases).

Under S2S_WGRAD_XCD / S2S_WGRAD_BLOCKS (tests/test_env_variants_gpu.py runs the conv3x3 tests of this file in child
processes) the plan is read from the query and printed, and the table's default plan is not asserted."""
import os

import pytest
import torch

import wgrad_forms_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
DTYPES = [BF, F32]
DT_IDS = ["bf16", "fp32"]
TOL_F32 = (1e-4, 1e-4)             # fp32 outputs: max norm, L2
TOL_BF16 = (4e-3, 2.2e-3)          # bf16-stored outputs
NAN = float("nan")
DEFAULT_SWITCHES = not (os.environ.get("S2S_WGRAD_XCD") or os.environ.get("S2S_WGRAD_BLOCKS"))

# K per (kernel, dtype): see the module docstring
K = {("conv3x3", BF): 4, ("conv3x3", F32): 4, ("stem", BF): 4, ("stem", F32): 8,
     ("head_dw", BF): 8, ("head_dw", F32): 8, ("head_v", BF): 16, ("head_v", F32): 16}


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    """torch.empty starts as NaN and every workspace slab as 0xFF (the fixture of tests/test_objects_gpu.py)."""
    from stain2stain_amd import ops
    import torch.utils.deterministic as tud
    prev_det, prev_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    prev_fill = tud.fill_uninitialized_memory
    orig = ops._workspace

    def poisoned(device, numel, tag):
        buf = orig(device, numel, tag)
        buf.view(torch.uint8).fill_(255)
        return buf

    torch.use_deterministic_algorithms(True, warn_only=True)
    tud.fill_uninitialized_memory = True
    try:
        for buf in ops._WORKSPACE.values():
            buf.view(torch.uint8).fill_(255)
        monkeypatch.setattr(ops, "_workspace", poisoned)
        yield orig
    finally:
        torch.use_deterministic_algorithms(prev_det, warn_only=prev_warn)
        tud.fill_uninitialized_memory = prev_fill


def _name(dtype):
    return "bf16" if dtype == BF else "fp32"


def _hold(what, got, ref, tol, yard=None, k=None, detail=None):
    """Print the figures, then assert the hard bound and, where a yardstick is given, the ratio bound."""
    err = R.deviation(got, ref)
    line = f"{what}: max {err[0]:.2e} l2 {err[1]:.2e}"
    rat = None
    if yard is not None:
        rat = R.ratios(err, yard)
        line += f" | yardstick {yard[0]:.2e} {yard[1]:.2e} | ratio {rat[0]:.2f} {rat[1]:.2f} (K {k})"
    print(line)
    more = "" if detail is None else "; " + detail()
    assert err[0] < tol[0] and err[1] < tol[1], f"{line}: over the hard bound {tol}{more}"
    if rat is not None:
        assert rat[0] <= k and rat[1] <= k, f"{line}: over K x yardstick{more}"


def _hold_bf16_dx(what, dx, case, cout):
    """The head's bf16-stored data gradient: 4e-3 in the max norm and, for 500 elements and more, 2.2e-3 in L2.  That L2
    figure is the statistic of one bf16 rounding over many elements (about 1.7e-3); over the 8 ... 256 elements of the
    one-pixel cases a correctly rounded result can be anywhere up to 2^-8 = 3.9e-3 (measured: 2.59e-3 at C = 8, where the
    float64 reference rounded to bf16 deviates by the same 2.59e-3), so those are held element by element instead, and so
    is every other case: dx is one rounding of an fp32 sum of Cout products, |dx - ref| <= (1/2 + 1/64) ulp_bf16(ref)
    plus the rounding of the fp32 sum itself, Cout^2 2^-24 max|dy| max|w|."""
    ref = case["dx"]
    err = R.deviation(dx, ref)
    slack = cout * cout * 2.0 ** -24 * float(case["dy"].abs().max()) * float(case["w"].abs().max())
    d = (dx.detach().cpu().double() - ref).abs()
    mag = ref.abs().clamp_min(2.0 ** -126)
    ulps = float(((d - slack).clamp_min(0) / torch.exp2(torch.floor(torch.log2(mag)) - 7)).max())
    line = f"{what}: max {err[0]:.2e} l2 {err[1]:.2e} worst element {ulps:.3f} bf16 ulps ({ref.numel()} elements)"
    print(line)
    assert err[0] < TOL_BF16[0], line
    assert ref.numel() < 500 or err[1] < TOL_BF16[1], line
    assert ulps <= 0.5 + 1.0 / 64, line


def _prefill(ref, seed):
    """Random values of the reference's own size for the buffer a kernel overwrites or adds to."""
    g = torch.Generator().manual_seed(seed)
    scale = max(float(ref.abs().max()), 1e-3)
    return (torch.rand(ref.shape, generator=g) * 2 - 1).float() * scale


def _nhwc(t_nchw, dtype):
    return t_nchw.permute(0, 2, 3, 1).contiguous().to(DEV, dtype)


def _slice_of_wide(t_nhwc, before, after):
    """The tensor as channels [before, before + C) of a NaN-filled buffer: returns (view, buffer)."""
    B, H, W, C = t_nhwc.shape
    wide = torch.full((B, H, W, before + C + after), NAN, dtype=t_nhwc.dtype, device=t_nhwc.device)
    wide[..., before:before + C] = t_nhwc
    return wide[..., before:before + C], wide


def _guards_intact(wide, before, C):
    return bool(torch.isnan(wide[..., :before]).all()) and bool(torch.isnan(wide[..., before + C:]).all())


# ---------------------------------------------------------------------------------------------------------------------
# 3x3 weight gradient
# ---------------------------------------------------------------------------------------------------------------------
def _conv3x3_plan_line(name, dtype):
    from stain2stain_amd import ops
    (B, H, W, c0, c1, cout), (S, tiles, xcd, fold) = R.CONV3X3[name]
    plan = ops.conv3x3_wgrad_plan(dtype, B, H, W, c0 + c1, cout)
    if DEFAULT_SWITCHES:
        want = {"splits": S, "tiles": tiles, "xcd": xcd if dtype == BF else 0, "fold": fold, "kernel": 0 if dtype == BF else 1}
        assert plan == want, (plan, want)
    walks = sorted({len(w) for w in R.conv3x3_walks(name, plan["splits"])})
    return (f"conv3x3_wgrad {name} {_name(dtype)} S {plan['splits']} tiles {plan['tiles']} walk {'/'.join(map(str, walks))} "
            f"xcd {plan['xcd']} fold {plan['fold']} kernel {plan['kernel']}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name", list(R.CONV3X3))
def test_conv3x3_wgrad_form_dense(name, dtype):
    from stain2stain_amd import ops
    (B, H, W, c0, c1, cout), _ = R.CONV3X3[name]
    case = R.conv3x3_case(name, dtype)
    ref, line = case["ref"], _conv3x3_plan_line(name, dtype)
    xs, dy = _nhwc(case["x"], dtype), _nhwc(case["dy"], dtype)
    x0 = xs[..., :c0].contiguous()
    x1 = xs[..., c0:].contiguous() if c1 else None
    grad = _prefill(ref, 1).to(DEV)
    ops.conv3x3_wgrad(dy, x0, x1, grad, accumulate=False)
    _hold(line + " dense", grad, ref, TOL_F32, case["yard"], K[("conv3x3", dtype)], lambda: R.worst_tap_and_tile(grad, ref))
    pre = _prefill(ref, 2)
    grad = pre.to(DEV)
    ops.conv3x3_wgrad(dy, x0, x1, grad, accumulate=True)
    _hold(line + " dense, accumulated", grad, pre.double() + ref, TOL_F32, detail=lambda: R.worst_tap_and_tile(grad, pre.double() + ref))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name", list(R.CONV3X3))
def test_conv3x3_wgrad_form_strided(name, dtype):
    """dy with lddy > Cout, x0 and x1 from two buffers with different pixel strides, NaN in every channel around them."""
    from stain2stain_amd import ops
    (B, H, W, c0, c1, cout), _ = R.CONV3X3[name]
    case = R.conv3x3_case(name, dtype)
    ref, line = case["ref"], _conv3x3_plan_line(name, dtype)
    xs = _nhwc(case["x"], dtype)
    dy, dy_wide = _slice_of_wide(_nhwc(case["dy"], dtype), 8, 16)
    x0, x0_wide = _slice_of_wide(xs[..., :c0], 16, 8)
    x1, x1_wide = _slice_of_wide(xs[..., c0:], 8, 40) if c1 else (None, None)
    assert dy.stride(2) == cout + 24 and x0.stride(2) == c0 + 24 and (x1 is None or x1.stride(2) == c1 + 48 != x0.stride(2))
    grad = _prefill(ref, 3).to(DEV)
    ops.conv3x3_wgrad(dy, x0, x1, grad, accumulate=False)
    _hold(line + " strided", grad, ref, TOL_F32, case["yard"], K[("conv3x3", dtype)], lambda: R.worst_tap_and_tile(grad, ref))
    assert _guards_intact(dy_wide, 8, cout) and _guards_intact(x0_wide, 16, c0)
    assert x1 is None or _guards_intact(x1_wide, 8, c1)


# ---------------------------------------------------------------------------------------------------------------------
# stem weight / bias gradient
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name", list(R.STEM))
def test_stem_wgrad_form(name, dtype):
    from stain2stain_amd import _native, ops
    (B, H, W, cin, cout), (tiles, blocks, slabs) = R.STEM[name]
    assert _native.lib().s2s_stem_wgrad_blocks(B, H, W) == blocks
    case = R.stem_case(name, dtype)
    ref, ref_db = case["ref"], case["ref_db"]
    line = f"stem_wgrad {name} {_name(dtype)} tiles {tiles} workgroups {blocks} slabs {slabs}"
    x, dyd = case["x"].to(DEV), _nhwc(case["dy"], dtype)
    k = K[("stem", dtype)]
    detail = lambda: R.worst_tap_and_tile(dw, ref)                                      # noqa: E731
    # dense, accumulate = False into random values
    dw, db = _prefill(ref, 4).to(DEV), _prefill(ref_db, 5).to(DEV)
    ops.stem_wgrad(dyd, x, dw, db)
    _hold(line + " dense dW", dw, ref, TOL_F32, case["yard"], k, detail)
    _hold(line + " dense db", db, ref_db, TOL_F32)
    # dense, accumulate = True
    pw, pb = _prefill(ref, 6), _prefill(ref_db, 7)
    dw, db = pw.to(DEV), pb.to(DEV)
    ops.stem_wgrad(dyd, x, dw, db, accumulate=True)
    _hold(line + " dense dW, accumulated", dw, pw.double() + ref, TOL_F32)
    _hold(line + " dense db, accumulated", db, pb.double() + ref_db, TOL_F32)
    # dy as a channel slice of a wider NaN-filled buffer
    dys, dy_wide = _slice_of_wide(dyd, 16, 8)
    dw, db = _prefill(ref, 8).to(DEV), _prefill(ref_db, 9).to(DEV)
    ops.stem_wgrad(dys, x, dw, db)
    _hold(line + " strided dW", dw, ref, TOL_F32, case["yard"], k, detail)
    _hold(line + " strided db", db, ref_db, TOL_F32)
    assert _guards_intact(dy_wide, 16, cout)


# ---------------------------------------------------------------------------------------------------------------------
# head
# ---------------------------------------------------------------------------------------------------------------------
_HEAD_IDS = [f"{c}-{o}" for c, o in R.HEAD]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("C,cout", list(R.HEAD), ids=_HEAD_IDS)
def test_head_fwd_form(C, cout, dtype):
    from stain2stain_amd import ops
    for px in R.head_pixels(C):
        fam = ops.head_family(dtype, *px, C, cout, True)
        assert fam == R.HEAD[(C, cout)]
        case = R.head_case(C, cout, px, dtype)
        line = f"head_fwd C {C} Cout {cout} {_name(dtype)} pixels {px[0] * px[1] * px[2]} family {fam}"
        x, w, b = case["x"].to(DEV, dtype), case["w"].to(DEV), case["b"].to(DEV)
        v = ops.head_fwd(x, w, b)
        _hold(line + " dense v", v, case["v"], TOL_F32, case["yard_v"], K[("head_v", dtype)])
        xs, x_wide = _slice_of_wide(x, 8, 16)
        v = ops.head_fwd(xs, w, b)
        _hold(line + " strided v", v, case["v"], TOL_F32, case["yard_v"], K[("head_v", dtype)])
        assert _guards_intact(x_wide, 8, C)
        v = ops.head_fwd(x, w, None)
        _hold(line + " no bias v", v, case["v"] - case["b"].double().reshape(1, cout, 1, 1), TOL_F32)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("C,cout", list(R.HEAD), ids=_HEAD_IDS)
def test_head_bwd_form(C, cout, dtype):
    from stain2stain_amd import _native, ops
    k = K[("head_dw", dtype)]
    for px in R.head_pixels(C):
        fam = ops.head_family(dtype, *px, C, cout, False)
        assert fam == R.HEAD[(C, cout)]
        case = R.head_case(C, cout, px, dtype)
        nb = _native.lib().s2s_head_wgrad_blocks(*px)
        line = f"head_bwd C {C} Cout {cout} {_name(dtype)} pixels {px[0] * px[1] * px[2]} family {fam} workgroups {nb}"
        x, w, dy = case["x"].to(DEV, dtype), case["w"].to(DEV), case["dy"].to(DEV)
        rdw, rdb = case["dw"], case["db"]
        # dense, accumulate = False into random values
        dw, db = _prefill(rdw, 10).to(DEV), _prefill(rdb, 11).to(DEV)
        dx = ops.head_bwd(dy, x, w, dw, db)
        _hold(line + " dense dW", dw, rdw, TOL_F32, case["yard_dw"], k)
        _hold(line + " dense db", db, rdb, TOL_F32)
        if dtype == BF:
            _hold_bf16_dx(line + " dense dx", dx, case, cout)
        else:
            _hold(line + " dense dx", dx, case["dx"], TOL_F32)
        # dense, accumulate = True
        pw, pb = _prefill(rdw, 12), _prefill(rdb, 13)
        dw, db = pw.to(DEV), pb.to(DEV)
        ops.head_bwd(dy, x, w, dw, db, accumulate=True)
        _hold(line + " dense dW, accumulated", dw, pw.double() + rdw, TOL_F32)
        _hold(line + " dense db, accumulated", db, pb.double() + rdb, TOL_F32)
        # x and dx as channel slices of two wider NaN-filled buffers with different strides; no bias gradient asked
        xs, x_wide = _slice_of_wide(x, 16, 8)
        dxs, dx_wide = _slice_of_wide(torch.full_like(x, NAN), 8, 24)
        dw = _prefill(rdw, 14).to(DEV)
        out = ops.head_bwd(dy, xs, w, dw, None, dx=dxs)
        assert out.data_ptr() == dxs.data_ptr()
        _hold(line + " strided dW", dw, rdw, TOL_F32, case["yard_dw"], k)
        if dtype == BF:
            _hold_bf16_dx(line + " strided dx", dxs, case, cout)
        else:
            _hold(line + " strided dx", dxs, case["dx"], TOL_F32)
        assert _guards_intact(x_wide, 16, C) and _guards_intact(dx_wide, 8, C)           # dx wrote its own slice only


@pytest.mark.parametrize("C,cout,fwd", R.HEAD_REFUSED, ids=[f"{c}-{o}-{'fwd' if f else 'bwd'}" for c, o, f in R.HEAD_REFUSED])
def test_head_refused_shapes_raise_and_launch_nothing(C, cout, fwd):
    """The return path only: valid tensors of the refused shape, the wrapper raises, no output buffer is touched."""
    from stain2stain_amd import ops
    B, H, W = 1, 7, 9
    assert ops.head_family(BF, B, H, W, C, cout, fwd) < 0
    x = torch.zeros((B, H, W, C), dtype=BF, device=DEV)
    w = torch.zeros((cout, C, 1, 1), device=DEV)
    if fwd:
        with pytest.raises(RuntimeError, match="head_conv1x1_fwd failed: invalid shape"):
            ops.head_fwd(x, w, None)
        return
    dw, db = torch.full((cout, C, 1, 1), 5.0, device=DEV), torch.full((cout,), 6.0, device=DEV)
    dx = torch.full((B, H, W, C), 7.0, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError, match="head_conv1x1_bwd failed: invalid shape"):
        ops.head_bwd(torch.zeros((B, cout, H, W), device=DEV), x, w, dw, db, dx=dx)
    torch.cuda.synchronize()
    assert bool((dw == 5.0).all()) and bool((db == 6.0).all()) and bool((dx == 7.0).all())
