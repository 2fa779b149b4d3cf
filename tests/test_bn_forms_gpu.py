"""The BatchNorm / ReLU / 2x2 max-pool kernels (norm_act.hip), every launch form, against float64 (tables, the host model
and the yardsticks: tests/bn_forms_ref.py; the model against autograd and the plan mirror against the library:
tests/test_bn_forms_cpu.py):

  * backward, ops.bn_relu_bwd -> s2s_bn_relu_bwd / s2s_bn_relu_bwd_phase (and the C ABI itself where the wrapper cannot
    express the call: a dx with lddx > C, a pool gradient of an image without a pool output): every pcb from 1 to 32 with
    partly used piece slots, one to four channel groups with a last group of one piece, nb from 1 to its cap (a workgroup
    walking several windows), the 64- and the 256-thread finalize on their scalar and 16-byte paths, odd H and W; each row
    with g1 + gp (windowed kernels), g1 only (flat kernels) and gp only (windowed, g1 null); accumulate; every operand as
    a channel slice of a wider NaN-filled buffer; the SyncBatchNorm phases with one and with two shards; determinism;
    the refused calls;
  * forward: ops.bn_finalize (s2s_bn_finalize_b) and ops.bn_partial_sums on synthetic partial buffers of 1 ... 1536 rows
    and 1 ... 1024 channels and on a real staged-convolution buffer, ops.bn_eval_prepare, ops.bn_relu_apply with and
    without the fused pool, dense and sliced, ops.maxpool2.

Every row runs in bf16 and in fp32 on poisoned memory (torch.empty filled with NaN, 0xFF in every ops._workspace slab).
The decisions (ReLU mask, pool winner) of the model are the kernel's own (teacher-forced, bn_forms_ref.decisions), so
the comparison is linear and tight.  The launch plan has no S2S_* switch: the form of every row is asserted.

Bounds.  Hard bounds are the project's own: fp32 outputs 1e-4 in the max norm and in L2, bf16-stored tensors 4e-3 /
2.2e-3, statistics 1e-5.  On top of them:

  * activation <= 1 ulp of the storage type from the model; the fused pool equal to the 2x2 maximum of the kernel's own
    stored activation; maxpool2 equal to torch's amax;
  * finalize, from the roundings in bn_finalize_kernel: mean, invstd <= 1 fp32 ulp, scale <= 2, shift <= 4 ulps of
    |beta| + |mean scale|, running statistics <= 4 ulps of |(1 - m) old| + |m new|, bn_partial_sums <= 1 ulp,
    bn_eval_prepare 1e-6 relative;
  * bf16 dx element by element: |dx - ref| <= (1/2 + 1/64) ulp_bf16(ref) + 2^-22 |gak| (|dz| + |c1| + |xh c2|), the
    second term for the fp32 evaluation of gak (dz - c1 - xh c2); cases of 500 elements and more also 2.2e-3 in L2.
    That slack covers the evaluation and nothing else, so ref is evaluated (in float64) with the fp32 means c1, c2 the
    apply pass read from the workspace, which are themselves held to the float64 model: see _hold_dx;
  * fp32 dx, and dgamma, dbeta, c1, c2 in both modes: K x YARDSTICK, the yardstick being the deviation from the float64
    model of the same quantity computed by torch on the CPU in fp32 from the same decisions (floored at 1e-7); dgamma and
    dbeta normalised by their max norm over the channels.  K is 4 x the largest ratio measured on an MI355X, rounded up
    to a power of two, never more than 64.  Largest ratios measured (max norm / L2) and the row that gave them:

  quantity, dtype      max    L2    row                                              K
  dx, fp32             1.03   0.74  2x6x6x1024 g1+gp / 1x2x2x16 gp                   8
  dgamma, bf16         3.58   3.34  2x13x9x24 gp / 4x260x260x8 g1+gp                 16
  dgamma, fp32         1.15   0.81  2x5x7x8 g1                                       8
  dbeta, bf16          0.50   0.40  2x66x66x256 g1 / 4x260x260x8 g1+gp               2
  dbeta, fp32          0.70   0.49  1x7x9x264 gp / 3x12x10x40 g1                     4
  c1, bf16             0.47   0.33  3x25x27x520 gp / 3x12x10x40 gp                   2
  c1, fp32             0.67   0.47  1x7x9x264 gp / 1x7x9x264 g1+gp                   4
  c2, bf16             3.28   3.44  2x13x9x24 gp / 4x260x260x8 g1+gp                 16
  c2, fp32             0.93   0.71  1x2x2x16 g1 / 2x5x7x8 g1                         4

(No ratio is over 16.  The yardsticks are 1e-7 ... 2e-7, mostly the floor; the bf16 kernels add their sum dz xhat in fp32,
the fp32 kernels in double.)  The bf16-stored dx measured 3.53e-3 in the max norm, 1.80e-3 in L2 over the cases of 500
elements and more, and 0.500 bf16 ulps for the worst element of every case with the kernel's means -- with the model's own
means up to 31.9 ulps (3x25x27x520) and 87.9 in its two-shard form.  Finalize: mean, invstd 0.50 ulps, scale 1.34, shift
2.21, running mean 2.86, running variance 1.33; bn_partial_sums 0.50; bn_eval_prepare 1.4e-7; activation 0 ulps.

Not reachable, so not tested: s2s_bn_relu_bwd_phase sets dbias_conv = nullptr before it launches (the conv-bias gradient
of a train-mode BatchNorm is identically zero and is written as such), so the dxsum_part partial sums of the two apply
kernels, colsum_finalize_kernel and prereduce never run from the C ABI.  The fused tail's reduction stays with
tests/test_tail_fused_gpu.py, the fused up-sampling loads with tests/test_upsample_bn_fused_gpu.py, the apply kernel's
grid cap with tests/test_production_shapes_gpu.py.

Run time of this file on an MI355X: 7.4 s (167 tests; the slowest, the capped row in bf16, 1.7 s)."""
import pytest
import torch

import bn_forms_ref as R
import stepwise_ref as SR
from test_wgrad_forms_gpu import _guards_intact, _slice_of_wide, poison  # noqa: F401  (poison: autouse fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
DTYPES = [BF, F32]
DT_IDS = ["bf16", "fp32"]
TOL_F32 = (1e-4, 1e-4)
TOL_BF16 = (4e-3, 2.2e-3)
TOL_STAT = 1e-5
NAN = float("nan")
ROWS = list(R.BWD)
SMALL_ROWS = [s for s in ROWS if s != R.CAPPED]
SLICE_ROWS = [(2, 13, 9, 24), (1, 7, 9, 264), (2, 66, 66, 256)]      # pcb 4, two channel groups, nb > 256

# K per (quantity, dtype): see the module docstring
K = {("dx", F32): 8, ("dgamma", BF): 16, ("dgamma", F32): 8, ("dbeta", BF): 2, ("dbeta", F32): 4,
     ("c1", BF): 2, ("c1", F32): 4, ("c2", BF): 16, ("c2", F32): 4}


def _name(dtype):
    return "bf16" if dtype == BF else "fp32"


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def _rand(n, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(n, generator=g) * 2 - 1) * scale).float()


def _hold(what, got, ref, tol, yard=None, k=None):
    """Print the figures, then assert the hard bound and, where a yardstick is given, the ratio bound."""
    err = R.deviation(got, ref)
    line = f"{what}: max {err[0]:.2e} l2 {err[1]:.2e}"
    rat = None
    if yard is not None:
        rat = R.ratios(err, yard)
        line += f" | yardstick {yard[0]:.2e} {yard[1]:.2e} | ratio {rat[0]:.2f} {rat[1]:.2f} (K {k})"
    print(line)
    assert err[0] < tol[0] and err[1] < tol[1], f"{line}: over the hard bound {tol}"
    if rat is not None:
        assert rat[0] <= k and rat[1] <= k, f"{line}: over K x yardstick"


def _worst_bf16_ulps(dx, r, slack):
    d = (dx.detach().cpu().double() - r).abs()
    mag = r.abs().clamp_min(2.0 ** -126)
    return float(((d - slack).clamp_min(0) / torch.exp2(torch.floor(torch.log2(mag)) - 7)).max())


def _hold_dx(what, dx, ref, dtype, case, means, yard=None):
    """fp32: hard bound and K x yardstick against the float64 model.  bf16: 4e-3 in the max norm, 2.2e-3 in L2 from 500
    elements on (the statistic of one bf16 rounding over many elements) against the float64 model, and element by
    element: within (1/2 + 1/64) bf16 ulps plus the slack of the fp32 evaluation of gak (dz - c1 - xh c2)
    (bn_forms_ref._bwd_model) of that expression in float64 WITH THE MEANS THE APPLY PASS READ, ``means`` = the kernel's
    fp32 (c1, c2) from its workspace.  The slack is for the evaluation alone (which needs 3.96 of its 4 units of 2^-24 in
    torch's fp32 on the CPU); the means' own rounding, held to the float64 model by _hold_sums, enters dx times |xhat| and
    where dz - c1 - xh c2 cancels it is many bf16 ulps of the result: against the pure model the CPU's fp32 evaluation
    itself is 51 ulps out at the (3, 25, 27, 520) row.  The figure against the pure model is printed."""
    if dtype == F32:
        _hold(what, dx, ref["dx"], TOL_F32, yard, K[("dx", F32)] if yard is not None else None)
        return
    r = ref["dx"]
    err = R.deviation(dx, r)
    st = case["stats"].double()
    xh = (case["raw"].double() - st[0]) * st[1]
    c1, c2 = (m.detach().cpu().double() for m in means)
    forced = r + (case["gamma"].double() * st[1]) * ((ref["c1"] - c1) + xh * (ref["c2"] - c2))
    ulps, pure = _worst_bf16_ulps(dx, forced, ref["slack"]), _worst_bf16_ulps(dx, r, ref["slack"])
    line = (f"{what}: max {err[0]:.2e} l2 {err[1]:.2e} worst element {ulps:.3f} bf16 ulps ({pure:.3f} with the model's "
            f"own means; {r.numel()} elements)")
    print(line)
    assert bool(torch.isfinite(dx).all()), line
    assert err[0] < TOL_BF16[0], line
    assert r.numel() < 500 or err[1] < TOL_BF16[1], line
    assert ulps <= 0.5 + 1.0 / 64, line


def _hold_sums(what, got, ref, dtype, yard=True):
    """dgamma, dbeta, c1, c2 (dict of GPU tensors) against the model."""
    for q in ("dgamma", "dbeta", "c1", "c2"):
        if q in got:
            _hold(f"{what} {q}", got[q], ref[q], TOL_F32, ref["yard"][q] if yard else None, K[(q, dtype)] if yard else None)


# ---------------------------------------------------------------------------------------------------------------------
# launching the backward
# ---------------------------------------------------------------------------------------------------------------------
def _operands(shape, dtype):
    case = R.bwd_case(shape, dtype)
    d = {k: case[k].to(DEV, dtype) for k in ("raw", "g1", "gp")}
    d.update(gamma=case["gamma"].to(DEV), stats=case["stats"].to(DEV))
    return d


def _abi(dtype, g1, gp, x, stats, gamma, dgamma, dbeta, dbias, accumulate, dx, shape, count_total=None, phases=(3,),
         exchange=None):
    """s2s_bn_relu_bwd_phase itself; operands may be channel slices, dx included.  A pool gradient without elements (an
    image of one row or column) is passed as a valid pointer nothing is read from.  Returns (status, work)."""
    from stain2stain_amd import ops
    L = ops._L()
    B, H, W, C = shape
    nb = L.s2s_bn_bwd_blocks(B, H, W, C)
    work = torch.empty((4 * nb * C + 2 * C,), dtype=F32, device=DEV)
    p1, ld1 = (0, 8) if g1 is None else ops._nhwc(g1)
    p2, ld2 = (0, 8) if gp is None else ((work.data_ptr(), C) if gp.numel() == 0 else ops._nhwc(gp))
    px, ldx = ops._nhwc(x)
    pdx, lddx = ops._nhwc(dx)
    n = B * H * W if count_total is None else count_total
    rc = 0
    for phase in phases:
        rc = L.s2s_bn_relu_bwd_phase(ops._dt(x), p1, ld1, p2, ld2, stats[2].data_ptr(), stats[3].data_ptr(), px, ldx,
                                     stats[0].data_ptr(), stats[1].data_ptr(), gamma.data_ptr(), dgamma.data_ptr(),
                                     dbeta.data_ptr(), 0 if dbias is None else dbias.data_ptr(), int(accumulate), pdx, lddx,
                                     work.data_ptr(), B, H, W, C, n, phase, ops._stream())
        if rc:
            break
        if phase == 1 and exchange is not None:
            exchange(work[4 * nb * C:])
    return rc, work


def _run(d, kind, shape, *, accumulate=False, exchange=None, count_total=None, seed=1, x=None):
    """One backward through ops.bn_relu_bwd (through the ABI where the pool gradient has no elements).  dgamma / dbeta
    start as random values, dbias_conv as NaN (as random values when accumulating).  Returns a dict of GPU tensors."""
    from stain2stain_amd import ops
    C = shape[3]
    x = d["raw"] if x is None else x
    g1 = d["g1"] if kind != "gp" else None
    gp = d["gp"] if kind != "g1" else None
    pre = {"dgamma": _rand(C, seed), "dbeta": _rand(C, seed + 1), "dbias": _rand(C, seed + 2)}
    out = {k: v.to(DEV) for k, v in pre.items()}
    if not accumulate:
        out["dbias"].fill_(NAN)
    if gp is not None and gp.numel() == 0:
        dx = torch.empty(shape, dtype=x.dtype, device=DEV)
        rc, _ = _abi(x.dtype, g1, gp, x, d["stats"], d["gamma"], out["dgamma"], out["dbeta"], out["dbias"], accumulate, dx,
                     shape, count_total, (3,) if exchange is None else (1, 2), exchange)
        assert rc == 0
    else:
        dx = ops.bn_relu_bwd(g1, gp, x, d["stats"], d["gamma"], out["dgamma"], out["dbeta"], out["dbias"],
                             accumulate=accumulate, exchange=exchange, count_total=count_total)
    out.update(dx=dx, pre=pre)
    return out


def _assert_form(shape):
    from stain2stain_amd import ops
    nb = ops._L().s2s_bn_bwd_blocks(*shape)
    p = R.plan(*shape, nb=nb)
    assert nb == R.red_blocks(*shape) and R.plan_row(p) == R.BWD[shape], (p, R.BWD[shape])
    return (f"bn_relu_bwd {R.shape_id(shape)} pcb {p['pcb']} groups {p['groups']} (last {p['last']}) nb {nb} "
            f"finalize {p['tpc']}{' 16B' if p['vec'] else ' scalar'} walk {p['walk']}")


# ---------------------------------------------------------------------------------------------------------------------
# backward: every row, three kinds, two dtypes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", ROWS, ids=R.shape_id)
def test_bwd_form(shape, dtype):
    """One call (phases = 3), then the same in two phases with an exchange that only records c1 and c2: the same bits,
    which is also the determinism of the launch (there is no atomic in the file)."""
    form = _assert_form(shape)
    case, d = R.bwd_case(shape, dtype), _operands(shape, dtype)
    C = shape[3]
    for kind in (R.KINDS[:2] if shape == R.CAPPED else R.KINDS):
        ref = R.bwd_ref(shape, dtype, kind)
        line = f"{form} {_name(dtype)} {kind}"
        out = _run(d, kind, shape)
        assert bool((out["dbias"] == 0).all()), line + ": dbias_conv is not exactly zero"
        rec = {}
        two = _run(d, kind, shape, exchange=lambda v: rec.update(c=v.clone()), count_total=shape[0] * shape[1] * shape[2])
        out.update(c1=rec["c"][:C], c2=rec["c"][C:])
        _hold_dx(line + " dx", out["dx"], ref, dtype, case, (out["c1"], out["c2"]), ref["yard"]["dx"])
        _hold_sums(line, out, ref, dtype)
        for q in ("dx", "dgamma", "dbeta", "dbias"):
            assert _same_bits(out[q], two[q]), f"{line}: {q} of the two-phase form differs from the one-call form"


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("shape", SLICE_ROWS, ids=R.shape_id)
def test_bwd_accumulate_and_repeat(shape, kind, dtype):
    """accumulate = True gives prefill + reference, the dx of the plain call, and leaves dbias_conv alone; the same call
    twice gives the same bits."""
    d = _operands(shape, dtype)
    ref = R.bwd_ref(shape, dtype, kind)
    line = f"{_assert_form(shape)} {_name(dtype)} {kind} accumulated"
    out = _run(d, kind, shape, accumulate=True, seed=20)
    again = _run(d, kind, shape, accumulate=True, seed=20)
    assert _same_bits(out["dx"], _run(d, kind, shape, seed=20)["dx"]), line + ": dx differs from the plain call's"
    for q in ("dgamma", "dbeta"):
        _hold(f"{line} {q}", out[q], out["pre"][q].double() + ref[q], TOL_F32)
    assert bool(torch.equal(out["dbias"].cpu(), out["pre"]["dbias"])), line + ": dbias_conv was touched"
    for q in ("dx", "dgamma", "dbeta"):
        assert _same_bits(out[q], again[q]), f"{line}: {q} differs between two identical calls"


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("shape", SLICE_ROWS, ids=R.shape_id)
def test_bwd_channel_slices(shape, kind, dtype):
    """x, g1, gp and dx each a channel slice of a wider NaN-filled buffer with its own stride (lddx > C: the C ABI): the
    bits of the dense run, and NaN still in every channel around the slices."""
    C = shape[3]
    d = _operands(shape, dtype)
    line = f"{_assert_form(shape)} {_name(dtype)} {kind} sliced"
    dense = _run(d, kind, shape, seed=30)
    xs, x_wide = _slice_of_wide(d["raw"], 8, 16)
    g1s, g1_wide = _slice_of_wide(d["g1"], 16, 16)
    gps, gp_wide = _slice_of_wide(d["gp"], 8, 32)
    dxs, dx_wide = _slice_of_wide(torch.full(shape, NAN, dtype=dtype, device=DEV), 24, 24)
    assert len({xs.stride(2), g1s.stride(2), gps.stride(2), dxs.stride(2), C}) == 5
    dgamma, dbeta = _rand(C, 30).to(DEV), _rand(C, 31).to(DEV)
    dbias = torch.full((C,), NAN, device=DEV)
    rc, _ = _abi(dtype, g1s if kind != "gp" else None, gps if kind != "g1" else None, xs, d["stats"], d["gamma"], dgamma,
                 dbeta, dbias, False, dxs, shape)
    assert rc == 0
    assert _same_bits(dxs, dense["dx"]) and _same_bits(dgamma, dense["dgamma"]) and _same_bits(dbeta, dense["dbeta"]), line
    assert bool((dbias == 0).all())
    assert _guards_intact(dx_wide, 24, C), line + ": dx wrote outside its slice"
    assert _guards_intact(x_wide, 8, C) and _guards_intact(g1_wide, 16, C) and _guards_intact(gp_wide, 8, C)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("shape", [(3, 12, 10, 40), (3, 25, 27, 520)], ids=R.shape_id)
def test_bwd_two_shards(shape, kind, dtype):
    """SyncBatchNorm: shards of 1 and 2 samples, each with count_total of the whole batch and an exchange that adds the
    other shard's recorded [2C] vector.  dx of each shard is the full-batch model's rows, dgamma and dbeta are the
    shard-local sums, c1 and c2 after the exchange the full batch's."""
    B, H, W, C = shape
    n = B * H * W
    case, d, full = R.bwd_case(shape, dtype), _operands(shape, dtype), R.bwd_ref(shape, dtype, kind)
    shards = [slice(0, 1), slice(1, 3)]

    def cut(src, s):
        return {k: (v[s] if k in ("raw", "g1", "gp") else v) for k, v in src.items()}

    vec = []
    for s in shards:                                   # phase 1 of each shard: its [2C] vector of local sums / n
        rec = {}
        _run(cut(d, s), kind, (s.stop - s.start, H, W, C), exchange=lambda v: rec.update(c=v.clone()), count_total=n)
        vec.append(rec["c"])
    for i, s in enumerate(shards):
        sub, cs = (s.stop - s.start, H, W, C), cut(case, s)
        g1, gp = R.kind_operands(cs, kind)
        local = R.bwd_model(g1, gp, cs["raw"], cs["stats"], cs["gamma"], dtype, count_total=n)
        line = f"bn_relu_bwd {R.shape_id(shape)} {_name(dtype)} {kind} shard {i} of 2"
        _hold(line + " c1 (local)", vec[i][:C], local["c1"], TOL_F32)
        _hold(line + " c2 (local)", vec[i][C:], local["c2"], TOL_F32)
        rec = {}

        def exchange(v, other=vec[1 - i], rec=rec):
            v.add_(other)
            rec.update(c=v.clone())

        out = _run(cut(d, s), kind, sub, exchange=exchange, count_total=n, seed=40 + i)
        rows = {"dx": full["dx"][s], "slack": full["slack"][s] if dtype == BF else None, "c1": full["c1"], "c2": full["c2"]}
        _hold_dx(line + " dx", out["dx"], rows, dtype, cs, (rec["c"][:C], rec["c"][C:]))
        _hold(line + " dgamma", out["dgamma"], local["dgamma"], TOL_F32)
        _hold(line + " dbeta", out["dbeta"], local["dbeta"], TOL_F32)
        _hold(line + " c1", rec["c"][:C], full["c1"], TOL_F32)
        _hold(line + " c2", rec["c"][C:], full["c2"], TOL_F32)
        assert bool((out["dbias"] == 0).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_bwd_relu_mask_below_the_smallest_bf16(dtype):
    """A pre-activation of 2^-140: positive in fp32, zero once stored in bf16 (whose smallest subnormal is 2^-133).  The
    windowed kernels take the ReLU mask from the value as the forward STORED it (WindowGrad::eval: the activation the
    next layer saw is 0, and so is its gradient), the flat kernels from the unrounded fmaf(x, scale, shift) > 0.  Pinned
    as written: in bf16 the pixel passes its gradient through the flat kernels and not through the windowed ones; in
    fp32 both pass it.  No value of a real step is that small, so the two never disagree there."""
    shape = (1, 2, 2, 8)
    case = dict(R.bwd_case(shape, dtype))
    raw, stats = case["raw"].clone(), case["stats"].clone()
    raw[0, 1, 0, 3] = 2.0 ** -70
    stats[:, 3] = torch.tensor([0.0, 1.0, 2.0 ** -70, 0.0])           # mean, invstd, scale, shift of channel 3
    raw[0, 0, 0, 3], raw[0, 0, 1, 3], raw[0, 1, 1, 3] = 1.0, 2.0, 0.5  # the window's other pixels: (0, 1) wins the pool
    z = SR.fma_f32(raw, stats[2], stats[3])
    assert float(z[0, 1, 0, 3]) == 2.0 ** -140 and float(R.as_read(z, BF)[0, 1, 0, 3]) == 0.0
    d = {"raw": raw.to(DEV, dtype), "g1": case["g1"].to(DEV, dtype), "gp": case["gp"].to(DEV, dtype),
         "gamma": case["gamma"].to(DEV), "stats": stats.to(DEV)}
    g = float(case["g1"][0, 1, 0, 3])
    assert abs(g) > 1e-3
    for kind in ("g1+gp", "g1"):
        g1, gp = R.kind_operands(case, kind)
        ref = R.bwd_model(g1, gp, raw, stats, case["gamma"], dtype)
        rec = {}
        out = _run(d, kind, shape, exchange=lambda v: rec.update(c=v.clone()), count_total=4)
        line = f"2^-140 pre-activation {_name(dtype)} {kind}"
        _hold(line + " dbeta", out["dbeta"], ref["dbeta"], TOL_F32)
        _hold_dx(line + " dx", out["dx"], ref, dtype, {"raw": raw, "stats": stats, "gamma": case["gamma"]},
                 (rec["c"][:8], rec["c"][8:]))
        # the pixel's own share of dbeta[3], against the model with that pixel's gradient removed
        g1z = g1.clone()
        g1z[0, 1, 0, 3] = 0.0
        without = R.bwd_model(g1z, gp, raw, stats, case["gamma"], dtype)
        share = float(out["dbeta"][3]) - float(without["dbeta"][3])
        passes = not (dtype == BF and kind == "g1+gp")
        print(f"{line}: share of dbeta {share:.6f}, g1 there {g:.6f}, passes {passes}")
        assert abs(share - (g if passes else 0.0)) < 1e-5


def test_bwd_refused_calls_launch_nothing():
    """What tests/test_native_cpu.py does not pin: count_total below the local count, phases outside 1 ... 3, C or an ld
    that is no multiple of 8, both gradients null.  Valid tensors; the status is returned and no output is touched."""
    shape = (2, 4, 6, 16)
    B, H, W, C = shape
    x = torch.zeros((B, H, W, 24), dtype=BF, device=DEV)
    g1 = torch.zeros((B, H, W, 24), dtype=BF, device=DEV)
    gp = torch.zeros((B, H // 2, W // 2, 24), dtype=BF, device=DEV)
    stats, gamma = torch.ones((4, C), device=DEV), torch.ones(C, device=DEV)

    def call(g1v=g1[..., :C], gpv=gp[..., :C], xv=x[..., :C], dx_ld=24, sh=shape, **kw):
        dgamma, dbeta, dbias = (torch.full((C,), v, device=DEV) for v in (5.0, 6.0, 7.0))
        dxw = torch.full((B, H, W, dx_ld), 8.0, dtype=BF, device=DEV)
        rc, work = _abi(BF, g1v, gpv, xv, stats, gamma, dgamma, dbeta, dbias, False, dxw[..., :C] if dx_ld > C else dxw,
                        sh, **kw)
        torch.cuda.synchronize()
        assert bool((dgamma == 5).all()) and bool((dbeta == 6).all()) and bool((dbias == 7).all()) and bool((dxw == 8).all())
        assert bool(work.isnan().all())
        return rc

    n = B * H * W
    assert call(count_total=n - 1) == -1
    assert call(phases=(0,)) == -1 and call(phases=(4,)) == -1 and call(phases=(-1,)) == -1
    assert call(g1v=None, gpv=None) == -5
    assert call(sh=(B, H, W, 12)) == -1                                # C % 8
    x20 = torch.zeros((B, H, W, 20), dtype=BF, device=DEV)
    assert call(xv=x20[..., :C]) == -1                                 # ldx % 8
    assert call(g1v=x20[..., :C]) == -1                                # ldg1 % 8
    gp20 = torch.zeros((B, H // 2, W // 2, 20), dtype=BF, device=DEV)
    assert call(gpv=gp20[..., :C]) == -1                               # ldgp % 8
    assert call(dx_ld=20) == -1                                        # lddx % 8
    # ... and the same call with nothing wrong is accepted
    dgamma, dbeta = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    dx = torch.empty((B, H, W, 24), dtype=BF, device=DEV)[..., :C]
    rc, _ = _abi(BF, g1[..., :C], gp[..., :C], x[..., :C], stats, gamma, dgamma, dbeta, None, False, dx, shape)
    assert rc == 0 and not bool(dx.isnan().any()) and not bool(dgamma.isnan().any())


# ---------------------------------------------------------------------------------------------------------------------
# forward: statistics
# ---------------------------------------------------------------------------------------------------------------------
FIN_OPTIONS = [
    {"running": True, "nbt": True, "momentum": 0.1, "eps": 1e-5, "bias": True},
    {"running": False, "nbt": False, "momentum": 0.1, "eps": 1e-3, "bias": False},
    {"running": True, "nbt": False, "momentum": 0.01, "eps": 1e-3, "bias": False},
    {"running": False, "nbt": True, "momentum": 0.01, "eps": 1e-5, "bias": False},
]


def _guarded(values):
    """A contiguous fp32 vector in the middle of a NaN-filled buffer: (view, buffer)."""
    buf = torch.full((values.numel() + 16,), NAN, device=DEV)
    buf[8:8 + values.numel()] = values.to(DEV)
    return buf[8:8 + values.numel()], buf


def _hold_finalize(line, out, f, rm=None, rv=None):
    got = {"mean": out[0], "invstd": out[1], "scale": out[2], "shift": out[3]}
    limit = {"mean": 1, "invstd": 1, "scale": 2, "shift": 4, "running_mean": 4, "running_var": 4}
    if rm is not None:
        got.update(running_mean=rm, running_var=rv)
    for q, t in got.items():
        ulps = R.f32_ulps(t, f[q], f.get(q + "_mag"))
        rel = SR.rel_max(t, f[q])
        print(f"{line} {q}: {float(ulps.max()):.3f} fp32 ulps (limit {limit[q]}), max norm {rel:.2e}")
        assert bool(torch.isfinite(t).all()) and rel < TOL_STAT, (line, q)
        assert float(ulps.max()) <= limit[q], (line, q, int(ulps.argmax()))


@pytest.mark.parametrize("C", R.FIN_C)
@pytest.mark.parametrize("nblk", R.FIN_NBLK)
def test_finalize_and_partial_sums(nblk, C):
    from stain2stain_amd import ops
    part = R.finalize_part(nblk, C)
    pd = part.to(DEV)
    g = torch.Generator().manual_seed(nblk * 7 + C)
    gamma, beta = 0.5 + torch.rand(C, generator=g), torch.rand(C, generator=g) - 0.5
    rm0, rv0, cb = torch.rand(C, generator=g) - 0.5, 0.5 + torch.rand(C, generator=g), torch.rand(C, generator=g) - 0.5
    tpc, vec = R.finalize_tpc(nblk), nblk % 4 == 0
    for o in FIN_OPTIONS:
        line = f"bn_finalize nblk {nblk} C {C} finalize {tpc}{' 16B' if vec else ' scalar'} {o}"
        rm, rm_buf = _guarded(rm0) if o["running"] else (None, None)
        rv, rv_buf = _guarded(rv0) if o["running"] else (None, None)
        nbt = torch.full((), 41, dtype=torch.int64, device=DEV) if o["nbt"] else None
        bias = cb if o["bias"] else None
        out = ops.bn_finalize(pd, R.FIN_COUNT, gamma.to(DEV), beta.to(DEV), rm, rv, nbt, momentum=o["momentum"],
                              eps=o["eps"], conv_bias=None if bias is None else bias.to(DEV))
        f = R.finalize_model(part, R.FIN_COUNT, gamma, beta, o["eps"], o["momentum"], rm0 if o["running"] else None,
                             rv0 if o["running"] else None, bias)
        _hold_finalize(line, out, f, rm, rv)
        assert nbt is None or int(nbt) == 42
        if o["running"]:
            assert bool(rm_buf[:8].isnan().all()) and bool(rm_buf[8 + C:].isnan().all())
            assert bool(rv_buf[:8].isnan().all()) and bool(rv_buf[8 + C:].isnan().all())
        if C >= 3:                                     # the constant channel: variance clamped at 0
            assert float(f["var"][0]) == 0.0
            assert float(R.f32_ulps(out[1][0], torch.tensor(float(torch.tensor(o["eps"])) ** -0.5, dtype=torch.float64))) <= 1
    sums = ops.bn_partial_sums(pd)
    ulps = float(R.f32_ulps(sums, R.finalize_model(part, 1, gamma, beta)["sums"]).max())
    print(f"bn_partial_sums nblk {nblk} C {C}: {ulps:.3f} fp32 ulps")
    assert ulps <= 1
    # what SyncBatchNorm does with them: a one-row buffer finalizes to the same statistics (within the roundings of sums)
    out = ops.bn_finalize(sums.view(2, C, 1), R.FIN_COUNT, gamma.to(DEV), beta.to(DEV), None, None, None)
    f = R.finalize_model(sums.view(2, C, 1), R.FIN_COUNT, gamma, beta)
    _hold_finalize(f"bn_finalize of bn_partial_sums nblk {nblk} C {C}", out, f)


def test_finalize_count_one():
    """One element per channel: the variance is 0 (or the rounding of x^2 - x^2, clamped), and the unbiased variance of
    the running statistics is the variance itself, not a division by zero."""
    from stain2stain_amd import ops
    C = 5
    x = _rand(C, 3, 2.0)
    part = torch.stack([x, x * x]).reshape(2, C, 1)
    gamma, beta, rm0, rv0 = 0.5 + _rand(C, 4).abs(), _rand(C, 5), _rand(C, 6), 0.5 + _rand(C, 7).abs()
    rm, _ = _guarded(rm0)
    rv, _ = _guarded(rv0)
    out = ops.bn_finalize(part.to(DEV), 1, gamma.to(DEV), beta.to(DEV), rm, rv, None)
    f = R.finalize_model(part, 1, gamma, beta, 1e-5, 0.1, rm0, rv0)
    _hold_finalize("bn_finalize count 1", out, f, rm, rv)
    assert float(f["var"].max()) < 1e-6


def test_finalize_real_staged_conv_buffer():
    """The partial buffer of a staged convolution (2048 rows: the 256-thread finalize on 16-byte loads), finalized
    against float64 statistics of the stored output."""
    import os
    from stain2stain_amd import ops
    from test_ops_gpu import STAGE_CASES
    B, H, W, c0, c1, cout, stats, level = STAGE_CASES[-1]
    assert (c0, c1, stats, level) == (8, 0, True, 1)
    g = torch.Generator().manual_seed(21)
    x = (torch.rand(B, H, W, c0, generator=g) * 2 - 1).to(DEV, BF)
    w = (torch.rand(cout, c0, 3, 3, generator=g) * 2 - 1) * 0.1
    wf, _ = ops.pack_conv3x3(w.to(DEV), BF)
    staged = ops._L().s2s_conv3x3_staged(0, B, H, W, cout, c0, 0, c0, 8, cout, 1)
    y, part = ops.conv3x3(x, None, wf, None, cout, want_stats=True)
    print(f"staged {staged}, partial buffer {tuple(part.shape)}")
    if int(os.environ.get("S2S_CONV_STAGE", "1")) >= 1:
        assert staged and part.shape[2] == 2048 and R.finalize_tpc(part.shape[2]) == 256
    gamma, beta, cb = 0.5 + _rand(cout, 1).abs(), _rand(cout, 2), _rand(cout, 3)
    rm0, rv0 = _rand(cout, 4), 0.5 + _rand(cout, 5).abs()
    rm, rv = rm0.to(DEV), rv0.to(DEV)
    n = B * H * W
    out = ops.bn_finalize(part, n, gamma.to(DEV), beta.to(DEV), rm, rv, None, conv_bias=cb.to(DEV))
    st = SR.bn_stats(y)
    scale, shift = SR.bn_affine(st, gamma, beta)
    erm, erv = SR.bn_running(rm0, rv0, st, 0.1, cb)
    for q, got, ref in (("mean", out[0], st["mean"]), ("invstd", out[1], st["invstd"]), ("scale", out[2], scale),
                        ("shift", out[3], shift), ("running_mean", rm, erm), ("running_var", rv, erv)):
        rel = SR.rel_max(got, ref)
        print(f"bn_finalize of a staged conv {q}: max norm {rel:.2e}")
        assert rel < TOL_STAT, q
    # and teacher-forced on the buffer itself, to the ulp
    _hold_finalize("bn_finalize of a staged conv, on its buffer", out,
                   R.finalize_model(part, n, gamma, beta, 1e-5, 0.1, rm0, rv0, cb), rm, rv)


@pytest.mark.parametrize("C", [1, 5, 256, 257, 1024])
def test_eval_prepare(C):
    from stain2stain_amd import ops
    gamma, beta, rmean, rvar = 0.5 + _rand(C, 1).abs(), _rand(C, 2), _rand(C, 3, 2.0), 0.05 + _rand(C, 4).abs()
    for eps in (1e-5, 1e-3):
        out = ops.bn_eval_prepare(gamma.to(DEV), beta.to(DEV), rmean.to(DEV), rvar.to(DEV), eps)
        sc = gamma.double() / torch.sqrt(rvar.double() + float(torch.tensor(eps)))
        sh = beta.double() - rmean.double() * sc
        e_sc = float(((out[0].cpu().double() - sc).abs() / sc.abs()).max())
        e_sh = float(((out[1].cpu().double() - sh).abs() / (beta.double().abs() + (rmean.double() * sc).abs())).max())
        print(f"bn_eval_prepare C {C} eps {eps}: scale {e_sc:.2e} shift {e_sh:.2e}")
        assert e_sc <= 1e-6 and e_sh <= 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# forward: apply (+ pool), stand-alone pool
# ---------------------------------------------------------------------------------------------------------------------
def _pool_of(act):
    B, H, W, C = act.shape
    Hp, Wp = H >> 1, W >> 1
    return act[:, :2 * Hp, :2 * Wp].reshape(B, Hp, 2, Wp, 2, C).amax((2, 4))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", SMALL_ROWS, ids=R.shape_id)
def test_apply_form(shape, dtype):
    from stain2stain_amd import ops
    B, H, W, C = shape
    Hp, Wp = H >> 1, W >> 1
    case = R.bwd_case(shape, dtype)
    x, scale, shift = case["raw"].to(DEV, dtype), case["stats"][2].to(DEV), case["stats"][3].to(DEV)
    _, stored = R.decisions(case["raw"], case["stats"], dtype, True)
    line = f"bn_relu_apply {R.shape_id(shape)} {_name(dtype)}"
    act, pool = ops.bn_relu_apply(x, scale, shift, want_pool=True)
    ulps = SR.bf16_ulps(act, stored) if dtype == BF else R.f32_ulps(act, stored)
    print(f"{line}: worst element {float(ulps.max()):.3f} ulps, {int((stored > 0).sum())} of {stored.numel()} positive")
    assert float(ulps.max()) <= 1 and bool((act >= 0).all())
    assert 0.2 < float((stored > 0).float().mean()) < 0.9 or stored.numel() < 100       # both ReLU branches
    assert tuple(pool.shape) == (B, Hp, Wp, C) and bool(torch.equal(pool, _pool_of(act))), line + ": fused pool"
    alone, none = ops.bn_relu_apply(x, scale, shift)
    assert none is None and _same_bits(alone, act), line + ": without the pool"
    # out= and pool= as channel slices of NaN-filled buffers, x as one too
    xs, x_wide = _slice_of_wide(x, 16, 8)
    outs, out_wide = _slice_of_wide(torch.full(shape, NAN, dtype=dtype, device=DEV), 8, 32)
    pools, pool_wide = _slice_of_wide(torch.full((B, Hp, Wp, C), NAN, dtype=dtype, device=DEV), 24, 8)
    got, gotp = ops.bn_relu_apply(xs, scale, shift, out=outs, pool=pools if pools.numel() else None)
    assert got.data_ptr() == outs.data_ptr() and _same_bits(outs, act), line + ": sliced"
    assert _guards_intact(out_wide, 8, C) and _guards_intact(x_wide, 16, C)
    if pools.numel():
        assert _same_bits(pools, pool) and _guards_intact(pool_wide, 24, C), line + ": sliced pool"


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", [(2, 5, 7, 8), (2, 13, 9, 24), (1, 7, 9, 264), (2, 6, 6, 1024), (2, 66, 66, 256)],
                         ids=R.shape_id)
def test_maxpool2_form(shape, dtype):
    """Negative and mixed inputs (the fused pool only ever sees ReLU outputs), dense and as a channel slice."""
    from stain2stain_amd import ops
    for name, offset in (("negative", -3.0), ("mixed", 0.0)):
        x = (_rand(shape, 50, 1.0) + offset).to(DEV, dtype)
        assert name == "mixed" or bool((x < 0).all())
        pool = ops.maxpool2(x)
        assert bool(torch.equal(pool, _pool_of(x))), f"maxpool2 {shape} {_name(dtype)} {name}"
        xs, x_wide = _slice_of_wide(x, 8, 16)
        assert _same_bits(ops.maxpool2(xs), pool) and _guards_intact(x_wide, 8, shape[3])
