"""The trainers' ``lazy_up`` switch (engine.LazyAct): the activations that only an up-sampling reads -- the bottleneck and
the second conv of every Up block but the last -- are not stored, the up-sampling applies BatchNorm + ReLU to its loads.
Elementwise and rounded as ``bn_relu_apply`` rounds, so a run with the switch on is the run with it off BIT FOR BIT:
losses and every ``state_dict`` entry after three optimisation steps from one seed, eagerly and as a captured graph, in
bf16 and fp32.  ``ops.profile_start`` must show ``bn_relu_apply`` launched fewer times per step, by the number of lazy
layers (the CFM step: the bottleneck and every Up block but the last; the multitask step keeps its encoder passes whole,
so there: every Up block but the last of either decoder), and the inspecting call (``want_v`` /
``want_outputs``) must keep every launch.  The kernel itself is held by tests/test_upsample_bn_fused_gpu.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEPS = 3


def _batch(nb, size, seed=5):
    g = torch.Generator().manual_seed(seed)
    x0 = (torch.rand(nb, 3, size, size, generator=g) * 2 - 1).to(DEV)
    x1 = (torch.rand(nb, 3, size, size, generator=g) * 2 - 1).to(DEV)
    return x0, x1, torch.rand(STEPS, nb, generator=g).to(DEV)


def _applies(ops):
    return sum(1 for p in ops.profile_stop() if p[0].split("@")[0] == "bn_relu_apply")


def _same(a, b):
    assert a[0] == b[0], (a[0], b[0])
    assert set(a[1]) == set(b[1])
    for k, v in b[1].items():
        assert torch.equal(a[1][k], v), k


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("features,size", [([8, 16, 24], 24), ([64, 128], 16)], ids=["odd3", "c64"])
def test_cfm_trainer_lazy_up_is_bit_equal(features, size, prec):
    from stain2stain_amd import CFMTrainer, FlowUNet, ops
    x0, x1, t = _batch(2, size)
    n_lazy = len(features) - 1            # the bottleneck and len(features) - 2 Up blocks
    runs, applies, inspect = {}, {}, {}
    for lazy, graph in ((False, False), (True, False), (True, True)):
        torch.manual_seed(1984)
        net = FlowUNet(3, features, 3, 32, precision=prec).to(DEV).train()
        tr = CFMTrainer(net, lr=1e-3, weight_decay=1e-5, graph=graph)
        assert tr.lazy_up is True         # the default
        tr.lazy_up = lazy
        losses = []
        for s in range(STEPS):
            if not graph and s == STEPS - 1:     # (a profiled step runs eagerly: counted on the eager trainers only)
                ops.profile_start(("bn_relu_apply",))
            losses.append(float(tr.step(x0, x1, t[s])))
            if not graph and s == STEPS - 1:
                applies[lazy] = _applies(ops)
        torch.cuda.synchronize()
        runs[lazy, graph] = (losses, {k: v.detach().cpu().clone() for k, v in net.state_dict().items()})
        if not graph:                     # the inspecting call keeps every activation (the fused tail's too)
            ops.profile_start(("bn_relu_apply",))
            tr.forward_backward(x0, x1, t[0], want_v=True)
            inspect[lazy] = _applies(ops)
        if graph:
            assert tr._captured is not None
        tr.close()
    print("losses", runs[False, False][0], "bn_relu_apply launches per step", applies)
    assert applies[False] - applies[True] == n_lazy, applies
    assert inspect[True] == inspect[False] == applies[False] + 1, inspect      # (+ 1: the tail layer's own launch)
    _same(runs[True, False], runs[False, False])
    _same(runs[True, True], runs[False, False])
    assert all(l == l for l in runs[True, False][0])


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("features,size", [([8, 16], 32), ([8, 16, 24], 24)], ids=["two", "odd3"])
def test_multitask_trainer_lazy_up_is_bit_equal(features, size, prec):
    """The multitask step keeps both encoder passes' bottleneck (the step-wise suite reads every encoder layer's activation
    from it), so its lazy layers are the decoders' alone: none with one Up block per decoder, one per decoder with two."""
    from stain2stain_amd import FlowMatchingDecoder, MultiTaskTrainer, SegmentationDecoder, SharedEncoder, ops
    x0, x1, t = _batch(2, size)
    mask = (torch.rand(2, 1, size, size, generator=torch.Generator().manual_seed(9)) > 0.5).float().to(DEV)
    dfeat = features[:-1][::-1]
    runs, applies, inspect = {}, {}, {}
    for lazy in (False, True):
        torch.manual_seed(1984)
        enc = SharedEncoder(3, features, precision=prec).to(DEV).train()
        fdec = FlowMatchingDecoder(features[-1], dfeat, 3, 32, precision=prec).to(DEV).train()
        sdec = SegmentationDecoder(features[-1], dfeat, 1, precision=prec).to(DEV).train()
        tr = MultiTaskTrainer(enc, fdec, sdec, time_emb_dim=32, lr=1e-3, weight_decay=1e-5)
        assert tr.lazy_up is True
        tr.lazy_up = lazy
        losses = []
        for s in range(STEPS):
            if s == STEPS - 1:
                ops.profile_start(("bn_relu_apply",))
            losses.append(float(tr.step(x0, x1, mask, t[s])))
            if s == STEPS - 1:
                applies[lazy] = _applies(ops)
        torch.cuda.synchronize()
        runs[lazy] = (losses, {f"{i}.{k}": v.detach().cpu().clone() for i, m in enumerate((enc, fdec, sdec))
                               for k, v in m.state_dict().items()})
        ops.profile_start(("bn_relu_apply",))
        tr.forward_backward(x0, x1, mask, t[0], want_outputs=True)
        inspect[lazy] = _applies(ops)
        tr.close()
    print("losses", runs[False][0], "bn_relu_apply launches per step", applies)
    assert applies[False] - applies[True] == 2 * (len(features) - 2), applies     # every Up block but the last, per decoder
    assert inspect[True] == inspect[False] == applies[False] + 1, inspect      # (+ 1: the flow decoder's tail layer)
    _same(runs[True], runs[False])
