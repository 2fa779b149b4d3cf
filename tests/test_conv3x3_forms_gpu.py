"""The 3x3 forward / data-gradient convolution (s2s_conv3x3_nhwc_s, ops.conv3x3), every launch form, against float64
(tables, references and yardsticks: tests/conv3x3_forms_ref.py; the forms the tables must contain and the plans of the
rows: tests/test_conv3x3_forms_cpu.py):

  * conv3x3_stage_kernel, filter resident and streamed: statistics / deferred epilogue / affine, both workgroup orders;
  * conv3x3_pers16_kernel on cfgs 1 and 5, and -- in a child process under S2S_CONV_PERS=2 S2S_CONV_STAGE=0, the only way to
    them -- on cfgs 2, 3, 6 and 7, with STATS 0 / 1 / 2, one tile per workgroup and a walk;
  * conv3x3_dma16_kernel on each of its eight tiles, every XCD cut, split-K with 2, 3, 4, 8 and 16 splits;
  * conv3x3_mfma_kernel<float> on both tiles;  relu without a folded affine in every mode;  data gradients.

Every row runs in two operand tiers on poisoned memory (torch.empty filled with NaN, NaN in the output, the statistics
rows and the split workspace), dense and once more with the output and the sources as channel slices of wider NaN-filled
buffers (ldy > Cout, ld0 != c0, ld1 != c1, guard bands intact afterwards); bf16 rows below 0.3 GFLOP also run in fp32.
With no switch set the row's plan is asserted first; under a switch (tests/test_env_variants_gpu.py runs this file under
its five) the plan is queried and the buffers are sized from it.

EXACT tier (small-integer operands: one correct answer).  y is bit-equal to the rounded exact result; the statistics rows
are finite and their float64 sum equals the sum and the sum of squares of the stored values exactly; a split launch
equals the unsplit one bit for bit; ops.conv3x3, which sizes the buffers itself, gives the same bits.  (A bf16 launch with
relu and no affine may store a zero as -0: the activation path computes 0 * t.  Those rows compare y + 0.)

REAL tier.  Hard bounds, the project's own: bf16 4e-3 in the max norm and 2.2e-3 in L2 from 500 elements on, fp32 1e-4
in both, statistics 2e-4.  Element by element, with Y the row's per-element yardstick (torch's fp32 result against
float64, relative to mag = (conv(|x|, |w|) + |b|) |scale| + |shift|, floored at 1e-7):
    bf16  |y - ref| <= (1/2 + 1/64) ulp_bf16(ref before the relu) + K Y mag  (+ 2 fp32 ulps of mag behind an affine)
    fp32  |y - ref| <= K Y mag                                               (+ the same)
and the statistics against the float64 sums of the kernel's own stored values: K x what torch's fp32 sums of those values
lose (relative to sum |y| and sum y^2 of the channel, floored at 1e-7).  K is 4 x the largest ratio measured on an MI355X,
rounded up to a power of two and never more than 64.  Largest ratios measured, with the row that gave them:

  quantity, dtype     ratio   row                                                   K
  y, bf16             0.22    pers1_tile_stats (what is left beyond the rounding)    1
  y, fp32             2.37    p1_walk_carry (fp32 run of the bf16 row)               16
  statistics, bf16    0.80    p7_one_tile                                            4
  statistics, fp32    1.72    p1_one_carry (fp32 run)                                8

(y in bf16 is what is left beyond the rounding allowance.  The exact tier's values above 256, where bf16 rounds, occur in
the deep rows only, which are the split rows: their unsplit launches hold the per-tap epilogue's rounding mode at ties,
the real tier's (1/2 + 1/64) ulp holds that of the staged and persistent epilogues.)

Run time on an MI355X: the 195 tests of this file take 34 s with no switch set (test_conv3x3_forms_persistent_child 11 to
13 s of it), no test more than 2 s; under a launch variant the file takes 20 to 25 s, and the children of
tests/test_env_variants_gpu.py, which now run it too, take 46 to 50 s each of their 900 s."""
import os
import subprocess
import sys

import pytest
import torch

import conv3x3_forms_ref as R
import stepwise_ref as SR
from test_wgrad_forms_gpu import _guards_intact, _slice_of_wide, poison  # noqa: F401  (poison: autouse here too)

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
TOL = {BF: (4e-3, 2.2e-3), F32: (1e-4, 1e-4)}
TOL_STAT = 2e-4
K = {("y", BF): 1, ("y", F32): 16, ("stat", BF): 4, ("stat", F32): 8}
CHEAP_F32 = 0.3e9
SWITCHES = ("S2S_CONV_STAGE", "S2S_CONV_PERS", "S2S_CONV_XCD")
ENV_NOW = {k: os.environ[k] for k in SWITCHES if os.environ.get(k)}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dn(dtype):
    return "bf16" if dtype == BF else "fp32"


def _nhwc(t_nchw, dtype):
    return t_nchw.permute(0, 2, 3, 1).contiguous().to(DEV, dtype)


def _nchw(y):
    return y.detach().cpu().permute(0, 3, 1, 2).contiguous()


def _plan(name, dtype, ld0, ld1, ldy):
    """The library's plan of the launch; asserted against the table where the row was written for this environment."""
    from stain2stain_amd import ops
    shape, flags, env, want = R.row(name)
    B, H, W, c0, c1, cout = shape
    plan = ops.conv3x3_plan(dtype, B, H, W, c0, c1, cout, ld0=ld0, ld1=ld1, ldy=ldy, **R.plan_query_args(name))
    if env == ENV_NOW and dtype == R.row_dtype(name):
        assert tuple(plan.values()) == tuple(want), (name, plan, want)
    return plan


_KEEP = []


def _launch(name, dtype, c, wp, *, sliced, split=True):
    """One s2s_conv3x3_nhwc_s launch of the row on NaN-filled buffers sized from the plan: (y NCHW on the CPU, float64
    statistics [2, Cout] or None, plan)."""
    from stain2stain_amd import ops
    shape, flags, _, _ = R.row(name)
    B, H, W, c0, c1, cout = shape
    xs = _nhwc(c["x"], dtype)
    guards = []
    if sliced:
        x0, w0 = _slice_of_wide(xs[..., :c0], 16, 8)
        guards.append((w0, 16, c0))
        x1 = None
        if c1:
            x1, w1 = _slice_of_wide(xs[..., c0:], 8, 40)
            guards.append((w1, 8, c1))
        y, wy = _slice_of_wide(torch.full((B, H, W, cout), NAN, dtype=dtype, device=DEV), 8, 16)
        guards.append((wy, 8, cout))
    else:
        x0 = xs[..., :c0].contiguous()
        x1 = xs[..., c0:].contiguous() if c1 else None
        y = torch.full((B, H, W, cout), NAN, dtype=dtype, device=DEV)
    p0, py, p1 = x0.data_ptr(), y.data_ptr(), x1.data_ptr() if c1 else 0
    ld0, ldy, ld1 = (c0 + 24, cout + 24, c1 + 48 if c1 else 8) if sliced else (c0, cout, c1 if c1 else 8)
    assert B * H * W == 1 or (x0.stride(2) == ld0 and y.stride(2) == ldy and (not c1 or x1.stride(2) == ld1))
    plan = _plan(name, dtype, ld0, ld1, ldy)
    stat = torch.full((2, cout, plan["stat_rows"]), NAN, device=DEV) if "stats" in flags else None
    kw = None
    if "kwork" in flags and split and dtype == BF:
        assert plan["ksplit"] > 1 or ENV_NOW
        kw = torch.full((max(plan["ksplit"], 1), B * H * W, cout), NAN, device=DEV)
    dev = {k: (None if c[k] is None else c[k].to(DEV).float().contiguous()) for k in ("b", "sc", "sh")}
    _KEEP[:] = [xs, x0, x1, y, stat, kw, dev, wp]
    rc = ops._L().s2s_conv3x3_nhwc_s(0 if dtype == BF else 1, p0, ld0, c0, p1, ld1, c1, wp.data_ptr(), ops._f32(dev["b"]),
                                     py, ldy, ops._f32(stat), 0 if (stat is None or "rows0" in flags) else plan["stat_rows"],
                                     ops._f32(dev["sc"]), ops._f32(dev["sh"]), int("relu" in flags), ops._f32(kw), B, H, W,
                                     cout, ops._stream())
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()
    for wide, before, C in guards:
        assert _guards_intact(wide, before, C), f"{name}: a guard band was written or read into the result"
    sums = None
    if stat is not None:
        assert bool(torch.isfinite(stat).all()), f"{name}: {int((~torch.isfinite(stat)).sum())} statistics entries unwritten or non-finite"
        sums = stat.double().sum(-1).cpu()
    return _nchw(y), sums, plan


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def _check_exact(name, dtype, c, y, sums, plan, what):
    _, flags, _, _ = R.row(name)
    want = R.stored(c["ref"], dtype)
    if dtype == BF and "relu" in flags and "affine" not in flags:
        y = y + 0                                              # -0 -> +0 (see the module docstring)
    assert torch.equal(_bits(y), _bits(want)), f"{name} {_dn(dtype)} {what}: " + R.worst(y, want.double(), plan, dtype)
    if sums is not None:
        s1, s2 = R.stat_sums(y)
        assert torch.equal(sums[0], s1) and torch.equal(sums[1], s2), \
            (f"{name} {_dn(dtype)} {what}: statistics differ from the stored values in channels "
             f"{((sums[0] != s1) | (sums[1] != s2)).nonzero().flatten().tolist()[:8]}: "
             f"sum {(sums[0] - s1).abs().max():.1f} sum of squares {(sums[1] - s2).abs().max():.1f}")


def _check_real(name, dtype, c, y, sums, plan, what):
    _, flags, _, _ = R.row(name)
    ref, pre, mag, yard = c["ref"], c["pre"], c["mag"], c["yard"]
    assert bool(torch.isfinite(y).all()), f"{name} {_dn(dtype)} {what}: " + R.worst(y, ref, plan, dtype)
    err = (SR.rel_max(y, ref), SR.rel_l2(y, ref))
    d = (y.double() - ref).abs()
    free = torch.zeros_like(d)
    if dtype == BF:
        free = (0.5 + 1.0 / 64) * torch.exp2(torch.floor(torch.log2(pre.abs().clamp_min(2.0 ** -126))) - 7)
    if "affine" in flags:
        free = free + 2 * torch.exp2(torch.floor(torch.log2(mag.clamp_min(2.0 ** -126))) - 23)
    ratio = float(((d - free).clamp_min(0) / (yard[2] * mag.clamp_min(1e-30))).max())
    k = K[("y", dtype)]
    line = (f"{name} {_dn(dtype)} {what}: max {err[0]:.2e} l2 {err[1]:.2e} | yardstick {yard[0]:.2e} {yard[1]:.2e} "
            f"per element {yard[2]:.2e} | RATIO y {_dn(dtype)} {ratio:.3f} (K {k})")
    print(line)
    detail = lambda: R.worst(y, ref, plan, dtype)                                       # noqa: E731
    tol = TOL[dtype]
    assert err[0] < tol[0] and (ref.numel() < 500 or err[1] < tol[1]), f"{line}: over the hard bound {tol}; {detail()}"
    assert ratio <= k, f"{line}: over the per-element bound; {detail()}"
    if sums is not None:
        s1, s2 = R.stat_sums(y)
        ys = R.stat_yardstick(y)
        a1 = y.double().abs().sum((0, 2, 3)).clamp_min(1e-30)
        r1 = float(((sums[0] - s1).abs() / a1).max()) / ys[0]
        r2 = float(((sums[1] - s2).abs() / s2.clamp_min(1e-30)).max()) / ys[1]
        ks = K[("stat", dtype)]
        e1, e2 = SR.rel_max(sums[0], s1), SR.rel_max(sums[1], s2)
        sline = (f"{name} {_dn(dtype)} {what} statistics: sum {e1:.2e} squares {e2:.2e} | yardstick {ys[0]:.2e} {ys[1]:.2e} "
                 f"| RATIO stat {_dn(dtype)} {max(r1, r2):.3f} (K {ks})")
        print(sline)
        assert e1 < TOL_STAT and e2 < TOL_STAT, sline
        assert r1 <= ks and r2 <= ks, sline


def _pack(c, dtype, flags):
    from stain2stain_amd import ops
    wf, wd = ops.pack_conv3x3(c["w"].to(DEV), dtype)
    return wd if "dgrad" in flags else wf


def _run_row(name, tier):
    from stain2stain_amd import ops
    shape, flags, _, _ = R.row(name)
    B, H, W, c0, c1, cout = shape
    dtypes = [R.row_dtype(name)]
    if dtypes[0] == BF and R.flop(name) < CHEAP_F32:
        dtypes.append(F32)                                     # the fp32 family has its own plan: only the result is held
    check = _check_exact if tier == "exact" else _check_real
    for dtype in dtypes:
        c = R.case(name, dtype, tier)
        wp = _pack(c, dtype, flags)
        y, sums, plan = _launch(name, dtype, c, wp, sliced=False)
        check(name, dtype, c, y, sums, plan, "dense")
        ys, sums_s, _ = _launch(name, dtype, c, wp, sliced=True)
        check(name, dtype, c, ys, sums_s, plan, "sliced")
        if tier != "exact":
            continue
        if "kwork" in flags and dtype == BF:
            yu, _, _ = _launch(name, dtype, c, wp, sliced=False, split=False)
            assert torch.equal(_bits(yu), _bits(y)), f"{name}: split and unsplit launches differ: " + R.worst(y, yu.double(), plan, dtype)
        if "rows0" not in flags:                               # the wrapper sizes statistics and workspace itself
            xs = _nhwc(c["x"], dtype)
            dev = {k: (None if c[k] is None else c[k].to(DEV)) for k in ("b", "sc", "sh")}
            yw, stat = ops.conv3x3(xs[..., :c0], xs[..., c0:] if c1 else None, wp, dev["b"], cout, want_stats="stats" in flags,
                                   scale=dev["sc"], shift=dev["sh"], relu="relu" in flags)
            torch.cuda.synchronize()
            check(name, dtype, c, _nchw(yw), None if stat is None else stat.double().sum(-1).cpu(), plan, "ops.conv3x3")


TIERS = ["exact", "real"]


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", list(R.CASES) + list(R.SWITCH_CASES))
def test_conv3x3_form(name, tier):
    _run_row(name, tier)


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", list(R.PERS_CASES))
def test_conv3x3_pers_table_row(name, tier):
    """The rows written for S2S_CONV_PERS=2 S2S_CONV_STAGE=0 (test_conv3x3_forms_persistent_child runs them there, plans
    asserted); in any other environment they run on whatever the plan says."""
    _run_row(name, tier)


def test_conv3x3_forms_persistent_child():
    """conv3x3_pers16_kernel on cfgs 1, 2, 3, 5, 6 and 7 with STATS 0 / 1 / 2: the switches are read once per process, so
    the persistent table runs in a fresh child.  (Under a launch switch -- tests/test_env_variants_gpu.py -- this process
    is itself such a child and starts none.)"""
    if ENV_NOW or os.environ.get("S2S_WGRAD_XCD") or os.environ.get("S2S_WGRAD_BLOCKS"):
        return
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", os.path.abspath(__file__),
                          "-k", "pers_table_row"], capture_output=True, text=True, timeout=600, cwd=ROOT,
                         env={**os.environ, **R.PERS_ENV})
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-1500:]
    assert f"{len(R.PERS_CASES) * len(TIERS)} passed" in out.stdout and "failed" not in out.stdout, out.stdout[-500:]
