"""The drop-in FusedEMA (modules + FusedAdam under autograd) against torch.optim.swa_utils.AveragedModel: step-by-step
numbers, state-dict keys and interchange, a forward of the averaged copy that follows the average (packed operands,
folded BatchNorm constants), and the GPU-only contract."""
import copy

import pytest
import torch
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

from stain2stain_amd import FlowUNet, FusedAdam, FusedEMA, checkpoint, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DECAY = 0.9


def _batch(step, B=2, H=64):
    g = torch.Generator().manual_seed(200 + step)
    x0 = (torch.rand(B, 3, H, H, generator=g) * 2 - 1).to(DEV)
    x1 = (torch.rand(B, 3, H, H, generator=g) * 2 - 1).to(DEV)
    t = torch.rand(B, generator=g).to(DEV)
    return x0, x1, t


def _train_step(net, opt, step):
    x0, x1, t = _batch(step)
    xt, ut = ops.cfm_sample(x0, x1, t)
    loss = ((net(t, xt) - ut) ** 2).mean()
    loss.backward()
    opt.step()
    opt.zero_grad(set_to_none=True)


def _net(precision):
    torch.manual_seed(1984)
    return FlowUNet(3, [16, 32], 3, 32, precision=precision).to(DEV).train()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_fused_ema_matches_averaged_model_step_by_step(precision):
    net = _net(precision)
    opt = FusedAdam(net.parameters(), lr=1e-2)
    ema = FusedEMA(net, DECAY)
    ref = AveragedModel(net, multi_avg_fn=get_ema_multi_avg_fn(DECAY), use_buffers=True)
    for s in range(5):
        _train_step(net, opt, s)
        ema.update_parameters(net)
        ref.update_parameters(net)
        ours, want = ema.state_dict(), ref.state_dict()
        assert list(ours) == list(want)
        for k, v in want.items():
            if v.is_floating_point():
                assert float((ours[k] - v).abs().max()) <= 1e-6, k
        assert int(ours["n_averaged"]) == int(want["n_averaged"]) == s + 1
        for k, v in net.state_dict().items():              # integer buffers: copied from the live network
            if not v.is_floating_point():
                assert torch.equal(ours["module." + k], v), k
    diff = max(float((a - b).detach().abs().max()) for a, b in zip(ema.module.parameters(), net.parameters()))
    assert diff > 1e-3
    # the descriptor table is built once for an unchanged set of tensors
    table = ema._table
    ema.update_parameters(net)
    assert ema._table is table


def test_averaged_copy_forward_follows_the_average():
    net = _net("bf16")
    opt = FusedAdam(net.parameters(), lr=1e-2)
    ema = FusedEMA(net, DECAY)
    x0, _, t = _batch(40)
    ema.eval()
    for s in range(4):
        _train_step(net, opt, s)
        ema.update_parameters(net)
        with torch.no_grad():
            got = ema(t, x0)                       # forward delegates to .module (its caches warm from step 1 on)
        fresh = FlowUNet(3, [16, 32], 3, 32, precision="bf16").to(DEV)
        checkpoint.load_weights(fresh, ema.state_dict(), strip_prefix="module.")
        with torch.no_grad():
            want = fresh.eval()(t, x0)
        assert torch.equal(got, want), s


def test_state_dict_interchanges_with_averaged_model():
    net = _net("fp32")
    opt = FusedAdam(net.parameters(), lr=1e-2)
    ema = FusedEMA(net, DECAY)
    ref = AveragedModel(net, multi_avg_fn=get_ema_multi_avg_fn(DECAY), use_buffers=True)
    for s in range(2):
        _train_step(net, opt, s)
        ema.update_parameters(net)
        ref.update_parameters(net)
    assert list(ema.state_dict()) == list(ref.state_dict())
    # AveragedModel -> FusedEMA: a loaded n_averaged > 0 means the next update averages (does not copy)
    ema2 = FusedEMA(copy.deepcopy(net), DECAY)
    ema2.load_state_dict(ref.state_dict())
    ref2 = AveragedModel(copy.deepcopy(net), multi_avg_fn=get_ema_multi_avg_fn(DECAY), use_buffers=True)
    ref2.load_state_dict(ema.state_dict())                 # FusedEMA -> AveragedModel
    _train_step(net, opt, 2)
    ema2.update_parameters(net)
    ref2.update_parameters(net)
    for k, v in ref2.state_dict().items():
        if v.is_floating_point():
            assert float((ema2.state_dict()[k] - v).abs().max()) <= 1e-6, k
    assert int(ema2.n_averaged) == 3


def test_cpu_modules_raise():
    with pytest.raises(RuntimeError, match="GPU"):
        FusedEMA(FlowUNet(3, [16, 32], 3, 32), DECAY)
    net = _net("fp32")
    ema = FusedEMA(net, DECAY)
    with pytest.raises(RuntimeError, match="GPU"):
        ema.update_parameters(copy.deepcopy(net).cpu())
