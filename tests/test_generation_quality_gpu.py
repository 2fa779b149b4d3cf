"""generation_quality and the trainers' evaluate_generation: the metrics of a sampler's output against its target, the
epoch accumulation, and no effect on training (bit-equal to a twin that never evaluated: loss, parameters, running
statistics, Adam state, packed weights, module modes; eager and beside a captured training step; live and EMA network)."""
import pytest
import torch

from stain2stain_amd import (CFMTrainer, EvalAccumulator, FlowMatchingDecoder, FlowUNet, MultiTaskTrainer,
                             SegmentationDecoder, SharedEncoder, euler_generate, fixed_step_generate, generation_quality,
                             image_quality, ops)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("psnr", "ssim", "mae", "mse")


def _data(B, H, seed, C=3):
    g = torch.Generator().manual_seed(seed)
    x0 = (torch.rand(B, C, H, H, generator=g) * 2 - 1).to(DEV)
    x1 = (x0.cpu() * 0.6 + 0.4 * (torch.rand(B, C, H, H, generator=g) * 2 - 1)).to(DEV)
    t = torch.rand(B, generator=g).to(DEV)
    return x0, x1, t


def _net(precision="bf16"):
    torch.manual_seed(1984)
    return FlowUNet(3, [16, 32], 3, 32, precision=precision).to(DEV)


@pytest.mark.parametrize("graph", [False, True])
def test_generation_quality_scores_the_samplers_output(graph):
    net = _net().eval()
    sampler = lambda x: euler_generate(net, x, 4, graph=graph)
    acc = EvalAccumulator()
    means, weights = [], []
    for B, seed in ((4, 1), (2, 2), (4, 3)):
        x0, x1, _ = _data(B, 64, seed)
        got = generation_quality(sampler, x0, x1, accumulator=acc)
        want = image_quality(sampler(x0), x1)
        assert sorted(got) == sorted(KEYS)
        for k in KEYS:
            assert tuple(got[k].shape) == (B,) and got[k].dtype == torch.float32 and got[k].is_cuda
            assert torch.equal(got[k], want[k]), k
        assert torch.isfinite(got["psnr"]).all() and (got["ssim"] < 1).all()
        means.append({k: got[k].mean().double() for k in KEYS})
        weights.append(B)
    epoch = acc.compute()
    for k in KEYS:
        want = sum(w * m[k] for w, m in zip(weights, means)) / sum(weights)
        assert abs(float(epoch[k]) - float(want)) <= 1e-6 * abs(float(want)), k
    # metric arguments pass through; a tuple-returning sampler is scored on its image
    x0, x1, _ = _data(2, 64, 4)
    a = generation_quality(lambda x: (sampler(x), None), x0, x1, quantize=False, window=7)
    b = image_quality(sampler(x0), x1, quantize=False, window=7)
    assert all(torch.equal(a[k], b[k]) for k in KEYS)
    g = getattr(net, "_s2s_euler_graph", None)
    if g is not None:
        g.close()


def _cfm(graph, ema=True):
    net = _net().train()
    return net, CFMTrainer(net, lr=1e-3, graph=graph, ema_decay=0.9 if ema else None)


def _state(mods, fp):
    s = {f"b{i}.{k}": v.detach().clone() for i, m in enumerate(mods) for k, v in m.state_dict().items()}
    s.update(p=fp.p.clone(), g=fp.g.clone(), m=fp.m.clone(), v=fp.v.clone())
    return s


def _packed(blocks, dtype):
    return [cb._pack[dtype][0].clone() for pair in blocks for cb in pair if dtype in cb._pack]


def _modes(mods):
    return [m.training for top in mods for m in top.modules()]


@pytest.mark.parametrize("graph", [False, True])
def test_cfm_evaluate_generation_leaves_training_bit_equal(graph):
    netA, A = _cfm(graph)
    netB, B = _cfm(graph)
    dtype = netA.encoder.compute_dtype
    blocks = lambda n: list(n.encoder._blocks) + list(n.flow_decoder.up_blocks)
    batches = [_data(4, 64, 10 + i) for i in range(4)]
    gx0, gx1, _ = _data(3, 64, 99)
    la, lb = [], []
    for i, (x0, x1, t) in enumerate(batches):
        la.append(A.step(x0, x1, t).clone())
        lb.append(B.step(x0, x1, t).clone())
        if i in (1, 2):                     # after the eager warm-up and after the capture of graph=True
            pa, sa, ma, steps = _packed(blocks(netA), dtype), _state([netA], A.fp), _modes([netA]), A.step_count
            ema_before = {k: v.clone() for k, v in A.ema_state_dict().items()}
            acc = EvalAccumulator()
            outs = [A.evaluate_generation(gx0, gx1, num_steps=3, accumulator=acc),
                    A.evaluate_generation(gx0, gx1, num_steps=3, graph=True),
                    A.evaluate_generation(gx0, gx1, num_steps=2, method="rk4", graph=True, use_ema=True),
                    A.evaluate_generation(gx0, gx1, num_steps=3, use_ema=True, quantize=False),
                    A.evaluate_generation(gx0, gx1, num_steps=3, graph=True, use_ema=True, quantize=False)]
            for o in outs:
                assert sorted(o) == sorted(KEYS) and all(tuple(v.shape) == (3,) for v in o.values())
                assert all(torch.isfinite(v).all() for v in o.values())
            assert all(torch.equal(outs[0][k], outs[1][k]) for k in KEYS)      # the captured step = the eager step
            assert all(torch.equal(outs[3][k], outs[4][k]) for k in KEYS)
            assert abs(float(acc.compute()["ssim"]) - float(outs[0]["ssim"].mean())) <= 1e-6
            # the live network's result is what the public sampler gives on the eval-mode network
            # (the engine forward with training=False is the kernel sequence of the eval-mode module: bit-equal, so
            #  a wrong BatchNorm mode cannot hide)
            want = image_quality(euler_generate(netA, gx0, 3), gx1)
            print("live vs module path:", {k: float((outs[0][k] - want[k]).abs().max()) for k in KEYS})
            assert all(torch.equal(outs[0][k], want[k]) for k in KEYS)
            want = image_quality(fixed_step_generate(A.ema_model(), gx0, 2, "rk4"), gx1)
            print("ema vs module path:", {k: float((outs[2][k] - want[k]).abs().max()) for k in KEYS})
            assert all(torch.equal(outs[2][k], want[k]) for k in KEYS)
            # nothing moved
            assert all(torch.equal(sa[k], v) for k, v in _state([netA], A.fp).items())
            assert all(torch.equal(a, b) for a, b in zip(pa, _packed(blocks(netA), dtype)))
            assert ma == _modes([netA]) and A.step_count == steps
            assert all(torch.equal(v, A.ema_state_dict()[k]) for k, v in ema_before.items())
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(la, lb))
    sa, sb = _state([netA], A.fp), _state([netB], B.fp)
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    ea, eb = A.ema_state_dict(), B.ema_state_dict()
    assert all(torch.equal(ea[k], eb[k]) for k in ea)
    assert A.step_count == B.step_count
    owner = id(A._eval_owner)
    assert any(key[3] == owner for key in ops._WORKSPACE)
    holders = A._generation.holders()
    captures = [g for h in holders for g in vars(h).values()]
    assert len(holders) == 2 and len(captures) >= 3 and all(g.graph is not None for g in captures)
    A.close()
    assert all(g.graph is None for g in captures) and not any(vars(h) for h in holders)
    assert not A._generation.holders() and not any(key[3] == owner for key in ops._WORKSPACE)
    B.close()


def test_cfm_evaluate_generation_without_ema_and_right_after_construction():
    net, tr = _cfm(False, ema=False)
    x0, x1, _ = _data(2, 64, 5)
    out = tr.evaluate_generation(x0, x1, num_steps=2)
    assert sorted(out) == sorted(KEYS) and tr.step_count == 0 and net.training
    with pytest.raises(RuntimeError):
        tr.evaluate_generation(x0, x1, num_steps=2, use_ema=True)
    with pytest.raises(ValueError):
        tr.evaluate_generation(x0, x1, num_steps=2, method="rk5")
    # dopri5 runs the per-sample controller: a sample's score does not depend on its batch mates
    both = tr.evaluate_generation(x0, x1, method="dopri5")
    one = tr.evaluate_generation(x0[1:], x1[1:], method="dopri5")
    graphed = tr.evaluate_generation(x0, x1, method="dopri5", graph=True)
    assert all(torch.isfinite(both[k]).all() and torch.equal(both[k][1:], one[k]) for k in KEYS)
    assert all(torch.equal(both[k], graphed[k]) for k in KEYS)
    tr.close()


def _multitask(precision="bf16"):
    torch.manual_seed(1984)
    enc = SharedEncoder(3, [16, 32], precision=precision)
    fdec = FlowMatchingDecoder(32, [16], 3, 32, precision=precision)
    sdec = SegmentationDecoder(32, [16], 1, precision=precision)
    return tuple(m.to(DEV).train() for m in (enc, fdec, sdec))


def test_multitask_evaluate_generation_leaves_training_bit_equal():
    netsA, netsB = _multitask(), _multitask()
    A = MultiTaskTrainer(*netsA, time_emb_dim=32, lr=1e-3, ema_decay=0.9)
    B = MultiTaskTrainer(*netsB, time_emb_dim=32, lr=1e-3, ema_decay=0.9)
    g = torch.Generator().manual_seed(5)
    mask = lambda b, h: (torch.rand(b, 1, h, h, generator=g) < 0.3).float().to(DEV)
    batches = [(*_data(4, 64, 20 + i), mask(4, 64)) for i in range(3)]
    gx0, gx1, _ = _data(3, 64, 98)
    la, lb = [], []
    for i, (x0, x1, t, m) in enumerate(batches):
        la.append(A.step(x0, x1, m, t).clone())
        lb.append(B.step(x0, x1, m, t).clone())
        if i in (0, 1):
            sa, ma = _state(netsA, A.fp), _modes(netsA)
            acc = EvalAccumulator()
            eager = A.evaluate_generation(gx0, gx1, num_steps=3, accumulator=acc)
            graphed = A.evaluate_generation(gx0, gx1, num_steps=3, graph=True)
            ema = A.evaluate_generation(gx0, gx1, num_steps=2, method="heun", graph=True, use_ema=True)
            assert all(torch.equal(eager[k], graphed[k]) for k in KEYS)
            assert all(tuple(v.shape) == (3,) and torch.isfinite(v).all() for v in ema.values())
            assert sorted(acc.compute()) == sorted(KEYS)
            # the flow head's image, as the module path forms it (encoder -> time embedding -> flow decoder)
            enc, fdec, _ = netsA
            for mod in netsA:
                mod.eval()
            temb = lambda t: ops.time_embedding(t, 32)
            want = image_quality(euler_generate(lambda t, x: fdec(*enc(x), temb(t)), gx0, 3), gx1)
            for mod in netsA:
                mod.train()
            assert all(torch.equal(eager[k], want[k]) for k in KEYS)
            assert all(torch.equal(sa[k], v) for k, v in _state(netsA, A.fp).items())
            assert ma == _modes(netsA)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(la, lb))
    sa, sb = _state(netsA, A.fp), _state(netsB, B.fp)
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    ea, eb = A.ema_state_dict(), B.ema_state_dict()
    assert all(torch.equal(ea[k], eb[k]) for k in ea)
    owner = id(A._eval_owner)
    captures = [g for h in A._generation.holders() for g in vars(h).values()]
    assert captures
    A.close()
    assert all(g.graph is None for g in captures)
    assert not A._generation.holders() and not any(key[3] == owner for key in ops._WORKSPACE)
    B.close()
