"""The EMA kernels of optim.hip against torch: the fused Adam + EMA leaves p, m, v bit-equal to the plain Adam and lerps
within 1 ulp of torch.lerp; weight 1.0 copies exactly; the device-scalar form equals the argument form; the multi-tensor
lerp matches torch._foreach_lerp_ with an empty tensor in the table and an integer buffer copied."""
import pytest
import torch

from stain2stain_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [1, 7, 8, 1000003]


def _adam_inputs(n, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    p = torch.randn(n, device=DEV, generator=g)
    grad = torch.randn(n, device=DEV, generator=g)
    m = torch.randn(n, device=DEV, generator=g) * 0.1
    v = torch.rand(n, device=DEV, generator=g) * 0.01
    e = p + torch.randn(n, device=DEV, generator=g) * 0.05
    return p, grad, m, v, e


def _within_1ulp(got, ref):
    up = torch.nextafter(ref, torch.full_like(ref, float("inf")))
    down = torch.nextafter(ref, torch.full_like(ref, float("-inf")))
    return bool(((got == ref) | (got == up) | (got == down)).all())


ARGS = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, grad_scale=0.5)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("w", [0.1, 0.7])
def test_adam_ema_matches_adam_bitwise_and_lerp_within_1ulp(n, w):
    p, g, m, v, e = _adam_inputs(n, n)
    p1, m1, v1 = p.clone(), m.clone(), v.clone()
    ops.adam_step_(p1, g, m1, v1, 3, **ARGS)
    p2, m2, v2, e2 = p.clone(), m.clone(), v.clone(), e.clone()
    ops.adam_ema_step_(p2, g, m2, v2, e2, 3, **ARGS, ema_weight=w)
    assert torch.equal(p1, p2) and torch.equal(m1, m2) and torch.equal(v1, v2)
    ref = torch.lerp(e, p1, w)
    assert _within_1ulp(e2, ref)
    assert not torch.equal(e2, e)


@pytest.mark.parametrize("n", SIZES)
def test_weight_one_copies_exactly(n):
    p, g, m, v, e = _adam_inputs(n, 10 + n)
    ops.adam_ema_step_(p, g, m, v, e, 1, **ARGS, ema_weight=1.0)
    assert torch.equal(e, p)


@pytest.mark.parametrize("n", SIZES)
def test_device_scalar_form_is_bit_equal_to_argument_form(n):
    p, g, m, v, e = _adam_inputs(n, 20 + n)
    a = [t.clone() for t in (p, m, v, e)]
    ops.adam_ema_step_(a[0], g, a[1], a[2], a[3], 5, **ARGS, ema_weight=0.25)
    hyper = torch.tensor(ops.adam_hyper(5, ARGS["lr"], ARGS["beta1"], ARGS["beta2"], ARGS["eps"],
                                        ARGS["weight_decay"], ARGS["grad_scale"]), dtype=torch.float32, device=DEV)
    slot = ops.EmaWeightSlot(DEV)
    slot.push(0.25)
    b = [t.clone() for t in (p, m, v, e)]
    ops.adam_ema_step_dev_(b[0], g, b[1], b[2], b[3], hyper, slot.dev)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # and the device form's p, m, v equal the plain device-scalar Adam's
    c = [t.clone() for t in (p, m, v)]
    ops.adam_step_dev_(c[0], g, c[1], c[2], hyper)
    for x, y in zip(c, b):
        assert torch.equal(x, y)


def test_misaligned_or_mismatched_operands_raise():
    p, g, m, v, e = _adam_inputs(64, 3)
    with pytest.raises(RuntimeError, match="aligned"):
        ops.adam_ema_step_(p[1:], g[1:], m[1:], v[1:], e[1:], 1, 1e-3, ema_weight=0.5)
    with pytest.raises(RuntimeError, match="same number"):
        ops.adam_ema_step_(p, g, m, v, e[:32], 1, 1e-3, ema_weight=0.5)
    with pytest.raises(RuntimeError):
        ops.EmaTable([(e.cpu(), p.cpu())])


@pytest.mark.parametrize("w", [1.0, 0.3, 0.7])
def test_ema_multi_matches_foreach_lerp(w):
    gen = torch.Generator(device=DEV).manual_seed(7)
    shapes = [1, 7, 0, 8, 1000003]
    dst = [torch.randn(n, device=DEV, generator=gen) for n in shapes]
    src = [torch.randn(n, device=DEV, generator=gen) for n in shapes]
    # an fp32 view that is not 16-byte aligned (the scalar path) and an int64 buffer (copied)
    base_d = torch.randn(4099, device=DEV, generator=gen)
    base_s = torch.randn(4099, device=DEV, generator=gen)
    dst.append(base_d[1:])
    src.append(base_s[1:])
    nbt_d = torch.tensor([5], dtype=torch.int64, device=DEV)
    nbt_s = torch.tensor([9], dtype=torch.int64, device=DEV)
    ref = [d.clone() for d in dst]
    torch._foreach_lerp_([r for r in ref if r.numel()], [s for s in src if s.numel()], w)
    guard = base_d[:1].clone()
    table = ops.EmaTable(list(zip(dst, src)) + [(nbt_d, nbt_s)])
    assert table.total == 1 + 1 + 0 + 1 + 245 + 2 + 1
    slot = ops.EmaWeightSlot(DEV)
    slot.push(w)
    ops.ema_multi_(table, slot.dev)
    for d, r in zip(dst, ref):
        if w == 1.0:
            assert torch.equal(d, r)
        else:
            assert _within_1ulp(d, r)
    assert int(nbt_d) == 9
    assert torch.equal(base_d[:1], guard)                  # nothing outside the view was written
    # deterministic: the same launch on the same inputs gives the same bits
    again = [r.clone() for r in ref]
    d2 = [x.clone() for x in again]
    table2 = ops.EmaTable(list(zip(d2, src)))
    ops.ema_multi_(table2, slot.dev)
    table3 = ops.EmaTable(list(zip(again, src)))
    ops.ema_multi_(table3, slot.dev)
    for x, y in zip(d2, again):
        assert torch.equal(x, y)


def test_ema_multi_copy_flag_copies_fp32_bits():
    a = torch.randn(4097, device=DEV)
    b = torch.randn(4097, device=DEV)
    slot = ops.EmaWeightSlot(DEV)
    slot.push(0.5)
    ops.ema_multi_(ops.EmaTable([(a, b)], copy=[True]), slot.dev)
    assert torch.equal(a, b)
