"""tests/bn_forms_ref.py is right: its float64 model of the BatchNorm / ReLU / max-pool backward and of the statistics
finalize against torch autograd and nn.BatchNorm2d in float64, its two-shard SyncBatchNorm form against the full batch,
and its mirror of the launch plan against the library's own query (a host function: no GPU).

Inputs are drawn so that the model's decisions and autograd's cannot differ: every pre-activation is at least 1e-3 from
zero, and the positive stored values of every pool window are distinct (values the ReLU kills are stored as 0, tie
there, and carry no gradient either way).  Bound: 1e-12 relative."""
import pytest
import torch
import torch.nn.functional as F

import bn_forms_ref as R
import stepwise_ref as SR

BF, F32 = R.BF, R.F32
TOL = 1e-12
EPS = 1e-5


def _draw(shape, dtype, seed):
    """raw (float64, exactly representable in the storage type), gamma, beta (float64) and the float64 statistics rows."""
    B, H, W, C = shape
    g = torch.Generator().manual_seed(seed)
    raw = R.as_read(torch.randn(shape, generator=g) * 1.5 + 0.2, dtype).double()
    gamma = (0.75 + 0.5 * torch.rand(C, generator=g)).double()
    beta = (0.2 + 0.2 * torch.rand(C, generator=g)).double()
    Hp, Wp = H >> 1, W >> 1
    for _ in range(200):
        stats = R.stats_rows(raw, gamma, beta, EPS, torch.float64)
        z = SR.fma_f32(raw, stats[2], stats[3])
        bad = z.abs() < 1e-3
        if Hp and Wp:
            y = R.as_read(z.clamp_min(0), dtype)[:, :2 * Hp, :2 * Wp]
            q = y.reshape(B, Hp, 2, Wp, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, 4, C)
            dup = torch.zeros(q.shape, dtype=torch.bool)
            for i in range(4):
                for j in range(i + 1, 4):
                    same = (q[:, :, :, i] == q[:, :, :, j]) & (q[:, :, :, i] > 0)
                    dup[:, :, :, j] |= same
            bad[:, :2 * Hp, :2 * Wp] |= dup.reshape(B, Hp, Wp, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * Hp, 2 * Wp, C)
        if not bool(bad.any()):
            return raw, gamma, beta, stats
        redraw = R.as_read(torch.randn(shape, generator=g) * 1.5 + 0.2, dtype).double()
        raw = torch.where(bad, redraw, raw)
    raise AssertionError("no decision-safe draw")


def _autograd(raw, gamma, beta, g1, gp):
    x = raw.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    ga, be = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = F.relu(F.batch_norm(x, None, None, ga, be, training=True, eps=EPS))
    loss = y.sum() * 0.0
    if g1 is not None:
        loss = loss + (y * g1.permute(0, 3, 1, 2)).sum()
    if gp is not None:
        loss = loss + (F.max_pool2d(y, 2) * gp.permute(0, 3, 1, 2)).sum()
    loss.backward()
    return x.grad.permute(0, 2, 3, 1), ga.grad, be.grad


def _rel(a, r):
    return float((a - r).abs().max() / max(float(r.abs().max()), 1e-30))


SHAPES = [(3, 6, 8, 16), (3, 5, 7, 8), (2, 4, 5, 8), (2, 7, 6, 24)]


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=R.shape_id)
def test_backward_model_equals_autograd(shape, dtype, kind):
    B, H, W, C = shape
    raw, gamma, beta, stats = _draw(shape, dtype, R._seed(shape) + (dtype == BF))
    g = torch.Generator().manual_seed(5)
    g1 = (torch.rand(shape, generator=g) - 0.5).double() if kind != "gp" else None
    gp = (torch.rand((B, H >> 1, W >> 1, C), generator=g) - 0.5).double() if kind != "g1" else None
    m = R.bwd_model(g1, gp, raw, stats, gamma, dtype)
    dx, dgamma, dbeta = _autograd(raw, gamma, beta, g1, gp)
    n = B * H * W
    errs = {"dx": _rel(m["dx"], dx), "dgamma": _rel(m["dgamma"], dgamma), "dbeta": _rel(m["dbeta"], dbeta),
            "c1": _rel(m["c1"], dbeta / n), "c2": _rel(m["c2"], dgamma / n)}
    print(shape, dtype, kind, errs)
    assert max(errs.values()) < TOL, errs
    assert int((m["dx"] != 0).sum()) > 0 and m["dx"].dtype == torch.float64


def test_backward_model_equals_the_stepwise_reference():
    """On even sizes in bf16 the model is stepwise_ref.bn_relu_bwd, up to that one's fp32 xhat and g1 + gp."""
    shape = (2, 6, 8, 16)
    case = R.bwd_case(shape, BF)
    m = R.bwd_model(case["g1"], case["gp"], case["raw"], case["stats"], case["gamma"], BF)
    draw, dgamma, dbeta = SR.bn_relu_bwd(case["g1"], case["gp"], case["raw"], case["stats"], case["gamma"])
    assert _rel(m["dx"], draw) < 1e-6 and _rel(m["dgamma"], dgamma) < 1e-6 and _rel(m["dbeta"], dbeta) < 1e-6


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
def test_odd_edges_receive_g1_only(dtype):
    """The last row and column of an odd image have no pool output: changing gp changes nothing there but through the
    means, and with g1 null their dz is zero."""
    shape = (2, 5, 7, 8)
    case = R.bwd_case(shape, dtype)
    m = R.bwd_model(None, case["gp"], case["raw"], case["stats"], case["gamma"], dtype)
    gak = case["gamma"].double() * case["stats"][1].double()
    xh = (case["raw"].double() - case["stats"][0].double()) * case["stats"][1].double()
    dz = m["dx"] / gak + m["c1"] + xh * m["c2"]
    assert float(dz[:, 4].abs().max()) < 1e-12 and float(dz[:, :, 6].abs().max()) < 1e-12
    assert float(dz[:, :4, :6].abs().max()) > 0.1


@pytest.mark.parametrize("kind", R.KINDS)
def test_two_shard_sync_model_equals_the_full_batch(kind):
    shape = (3, 5, 6, 16)
    raw, gamma, beta, stats = _draw(shape, F32, 11)
    g = torch.Generator().manual_seed(6)
    g1 = (torch.rand(shape, generator=g) - 0.5).double() if kind != "gp" else None
    gp = (torch.rand((3, 2, 3, 16), generator=g) - 0.5).double() if kind != "g1" else None
    full = R.bwd_model(g1, gp, raw, stats, gamma, F32)
    n = 3 * 5 * 6
    cut = lambda t, s: None if t is None else t[s]                                      # noqa: E731
    shards = [slice(0, 1), slice(1, 3)]
    first = [R.bwd_model(cut(g1, s), cut(gp, s), raw[s], stats, gamma, F32, count_total=n) for s in shards]
    vec = [torch.cat([f["c1"], f["c2"]]) for f in first]
    for i, s in enumerate(shards):
        m = R.bwd_model(cut(g1, s), cut(gp, s), raw[s], stats, gamma, F32, count_total=n, other=vec[1 - i])
        assert _rel(m["dx"], full["dx"][s]) < TOL
        assert _rel(m["c1"], full["c1"]) < TOL and _rel(m["c2"], full["c2"]) < TOL
    assert _rel(first[0]["dgamma"] + first[1]["dgamma"], full["dgamma"]) < TOL
    assert _rel(first[0]["dbeta"] + first[1]["dbeta"], full["dbeta"]) < TOL
    dx, _, _ = _autograd(raw, gamma, beta, g1, gp)
    assert _rel(full["dx"], dx) < TOL


@pytest.mark.parametrize("momentum", [0.1, 0.01])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
def test_finalize_model_equals_batchnorm2d(bias, momentum):
    B, C, H, W = 3, 5, 6, 7
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(B, C, H, W, generator=g) * 1.3 + 0.4).double()
    cb = (torch.rand(C, generator=g) - 0.5).double() if bias else None
    # the model takes eps and momentum as the fp32 values the kernel receives: the module gets those
    bn = torch.nn.BatchNorm2d(C, eps=float(torch.tensor(1e-3, dtype=F32)),
                              momentum=float(torch.tensor(momentum, dtype=F32))).double()
    with torch.no_grad():
        bn.weight.copy_(0.5 + torch.rand(C, generator=g))
        bn.bias.copy_(torch.rand(C, generator=g) - 0.5)
        bn.running_mean.copy_(torch.rand(C, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(C, generator=g))
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    y = bn(x if cb is None else x + cb[None, :, None, None]).detach()
    # the partial buffer of the convolution WITHOUT its bias, in three uneven pieces
    xs = x.permute(1, 0, 2, 3).reshape(C, -1)
    cuts = [(0, 40), (40, 41), (41, xs.shape[1])]
    part = torch.stack([torch.stack([xs[:, a:b].sum(1) for a, b in cuts], 1),
                        torch.stack([(xs[:, a:b] ** 2).sum(1) for a, b in cuts], 1)])
    f = R.finalize_model(part, B * H * W, bn.weight.detach(), bn.bias.detach(), 1e-3, momentum, rm, rv, cb)
    assert _rel(f["running_mean"], bn.running_mean) < TOL and _rel(f["running_var"], bn.running_var) < TOL
    act = x * f["scale"][None, :, None, None] + f["shift"][None, :, None, None]
    assert _rel(act, y) < TOL
    var = x.var((0, 2, 3), unbiased=False)
    assert _rel(f["mean"], x.mean((0, 2, 3))) < TOL and _rel(f["invstd"], 1 / torch.sqrt(var + bn.eps)) < TOL


def test_finalize_model_count_one_and_clamp():
    part = torch.tensor([[[1.5]], [[2.25 * (1 - 2.0 ** -12)]]])
    one = torch.ones(1)
    f = R.finalize_model(part, 1, one, one, 1e-5, 0.1, 0 * one, one)
    eps = float(torch.tensor(1e-5, dtype=F32))
    assert float(f["var"]) == 0.0 and abs(float(f["invstd"]) * eps ** 0.5 - 1.0) < TOL
    assert abs(float(f["running_var"]) - 0.9) < 1e-7          # unbiased = var when count = 1 (no division by zero)
    part = R.finalize_part(260, 5)
    f = R.finalize_model(part, R.FIN_COUNT, torch.ones(5), torch.ones(5))
    assert float(f["var"][0]) == 0.0 and abs(float(f["mean"][4]) - 1000.25) < 0.01
    assert float(f["mean"][4]) * 4096 == round(float(f["mean"][4]) * 4096)


@pytest.mark.parametrize("shape", list(R.BWD), ids=R.shape_id)
def test_plan_mirror_agrees_with_the_library(shape):
    """Every table row reaches the form it names, by the mirror and by s2s_bn_bwd_blocks."""
    from stain2stain_amd import _native
    nb = _native.lib().s2s_bn_bwd_blocks(*shape)
    assert nb == R.red_blocks(*shape)
    p = R.plan(*shape, nb=nb)
    assert R.plan_row(p) == R.BWD[shape], (p, R.BWD[shape])
    assert (p["walk"] > 1) == (shape == R.CAPPED) and (nb == R.NB_CAP) == (shape == R.CAPPED)


def test_plan_mirror_on_a_sweep():
    from stain2stain_amd import _native
    lib = _native.lib()
    for C in (8, 16, 24, 64, 136, 256, 264, 520, 1024, 2048):
        for B, H, W in ((1, 1, 1), (2, 5, 7), (3, 33, 31), (2, 128, 130), (16, 256, 256)):
            assert lib.s2s_bn_bwd_blocks(B, H, W, C) == R.red_blocks(B, H, W, C), (B, H, W, C)


def test_table_covers_the_forms():
    rows = list(R.BWD.values())
    assert {r[0] for r in rows} == {1, 2, 4, 8, 16, 32}                                  # every pcb
    assert {r[1] for r in rows} == {1, 2, 3, 4}                                          # channel groups
    assert {(r[4], r[5]) for r in rows} == {(64, False), (64, True), (256, False), (256, True)}
    assert any(r[1] > 1 and r[2] == 1 for r in rows) and any(r[2] < r[0] and r[1] == 1 for r in rows)
    assert any(s[1] % 2 and s[2] % 2 for s in R.BWD)
