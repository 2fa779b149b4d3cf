"""The fused trainers' EMA of the weights (ema_decay=) against torch.optim.swa_utils.AveragedModel, twins without EMA,
graph=True against eager, state round trips, and sampling / evaluation of the averaged network after further steps
(its packed operands and folded BatchNorm constants must follow the average)."""
import copy

import pytest
import torch
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

from stain2stain_amd import (CFMTrainer, FlowMatchingDecoder, FlowUNet, MultiTaskTrainer, SegmentationDecoder,
                             SharedEncoder, checkpoint, euler_generate)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DECAY, LR, STEPS = 0.9, 1e-2, 5


def _data(step, B=2, H=64):
    g = torch.Generator().manual_seed(100 + step)
    x0 = (torch.rand(B, 3, H, H, generator=g) * 2 - 1).to(DEV)
    x1 = (torch.rand(B, 3, H, H, generator=g) * 2 - 1).to(DEV)
    t = torch.rand(B, generator=g).to(DEV)
    return x0, x1, t


def _net(precision="bf16"):
    torch.manual_seed(1984)
    return FlowUNet(3, [16, 32], 3, 32, precision=precision).to(DEV).train()


def _cfm(precision="bf16", graph=False, ema=True):
    net = _net(precision)
    return net, CFMTrainer(net, lr=LR, graph=graph, ema_decay=DECAY if ema else None)


def _compare_to_averaged(ours, ref, tol=1e-6):
    assert list(ours) == list(ref)
    for k, v in ref.items():
        o = ours[k].to(v.device)
        if v.is_floating_point():
            assert float((o - v).abs().max()) <= tol, k
        elif k != "n_averaged" and not k.endswith("num_batches_tracked"):
            assert torch.equal(o, v), k
    assert int(ours["n_averaged"]) == int(ref["n_averaged"])


def test_cfm_ema_matches_averaged_model_every_step():
    net, tr = _cfm("fp32")
    ref = AveragedModel(copy.deepcopy(net).cpu(), multi_avg_fn=get_ema_multi_avg_fn(DECAY), use_buffers=True)
    live_cpu = FlowUNet(3, [16, 32], 3, 32, precision="fp32")
    for s in range(STEPS):
        tr.step(*_data(s))
        live_cpu.load_state_dict({k: v.cpu() for k, v in net.state_dict().items()})
        ref.update_parameters(live_cpu)
        ours = tr.ema_state_dict()
        _compare_to_averaged(ours, ref.state_dict())
        for k, v in net.state_dict().items():     # integer buffers: copied from the live network
            if not v.is_floating_point():
                assert torch.equal(ours["module." + k].cpu(), v.cpu()), k
    diff = max(float((a - b).abs().max()) for a, b in zip(tr.ema_model().parameters(), net.parameters()))
    assert diff > 1e-3                             # the average really lags the live weights
    tr.close()


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_live_state_bit_equal_to_twin_without_ema(precision):
    net_a, a = _cfm(precision, ema=True)
    net_b, b = _cfm(precision, ema=False)
    for s in range(STEPS):
        la, lb = a.step(*_data(s)), b.step(*_data(s))
        assert torch.equal(la, lb)
    for x, y in ((a.fp.p, b.fp.p), (a.fp.m, b.fp.m), (a.fp.v, b.fp.v)):
        assert torch.equal(x, y)
    for (k, x), y in zip(net_a.state_dict().items(), net_b.state_dict().values()):
        assert torch.equal(x, y), k
    a.close()
    b.close()


def test_graph_step_bit_equal_to_eager_with_ema():
    net_e, e = _cfm("bf16", graph=False)
    net_g, g = _cfm("bf16", graph=True)
    for s in range(STEPS):
        assert torch.equal(e.step(*_data(s)), g.step(*_data(s)))
    assert g._captured is not None
    for x, y in ((e.fp.p, g.fp.p), (e.fp.m, g.fp.m), (e.fp.v, g.fp.v), (e.fp.ema, g.fp.ema)):
        assert torch.equal(x, y)
    se, sg = e.ema_state_dict(), g.ema_state_dict()
    for k in se:
        assert torch.equal(se[k], sg[k]), k
    # a changed decay and a loaded state take effect without a recapture
    graph = g._captured
    g.fp.ema_decay = e.fp.ema_decay = 0.5
    g.load_ema_state_dict(se)
    e.load_ema_state_dict(se)
    assert torch.equal(e.step(*_data(9)), g.step(*_data(9)))
    assert g._captured is graph and torch.equal(e.fp.ema, g.fp.ema)
    e.close()
    g.close()


def test_ema_state_round_trips_through_averaged_model_and_resumes_bit_equal():
    net_a, a = _cfm("bf16")
    net_b, b = _cfm("bf16")
    for s in range(STEPS):
        a.step(*_data(s))
        if s < 3:
            b.step(*_data(s))
    sd = b.ema_state_dict()
    avg = AveragedModel(copy.deepcopy(net_b), multi_avg_fn=get_ema_multi_avg_fn(DECAY), use_buffers=True)
    avg.load_state_dict(sd)
    back = avg.state_dict()
    assert list(back) == list(sd)
    b.load_ema_state_dict(back)
    for k, v in b.ema_state_dict().items():
        assert torch.equal(v, sd[k]), k
    # resume in a fresh trainer from the weights, the optimiser state and the EMA state
    torch.manual_seed(5)
    net_c = FlowUNet(3, [16, 32], 3, 32, precision="bf16")
    net_c.load_state_dict({k: v.cpu() for k, v in net_b.state_dict().items()})
    c = CFMTrainer(net_c.to(DEV).train(), lr=LR, ema_decay=DECAY)
    c.load_optimizer_state_dict(b.optimizer_state_dict())
    c.load_ema_state_dict(sd)
    for s in range(3, STEPS):
        c.step(*_data(s))
    for x, y in ((a.fp.p, c.fp.p), (a.fp.m, c.fp.m), (a.fp.v, c.fp.v), (a.fp.ema, c.fp.ema)):
        assert torch.equal(x, y)
    sa, sc = a.ema_state_dict(), c.ema_state_dict()
    for k in sa:
        assert torch.equal(sa[k], sc[k]), k
    for x in (a, b, c):
        x.close()


def _fresh_from(state):
    net = FlowUNet(3, [16, 32], 3, 32, precision="bf16").to(DEV)
    rec = checkpoint.load_weights(net, state, strip_prefix="module.")
    assert not rec.missing_keys and not rec.unexpected_keys
    return net.eval()


def test_sampling_and_evaluate_follow_the_average():
    net, tr = _cfm("bf16")
    src = _data(50, B=1)[0]
    em = None
    for s in range(STEPS):
        tr.step(*_data(s))
        if s + 1 not in (3, 5):
            continue
        if em is None:
            em = tr.ema_model()
        assert tr.ema_model() is em and not em.training
        fresh = _fresh_from(tr.ema_state_dict())
        want = euler_generate(fresh, src, 8)
        assert torch.equal(euler_generate(em, src, 8), want)
        assert torch.equal(euler_generate(em, src, 8, graph=True), want)
        # evaluate(use_ema=True) against evaluate on the fresh network (a trainer that never stepped)
        x0, x1, t = _data(60)
        other = CFMTrainer(fresh.train(), lr=LR)
        assert torch.equal(tr.evaluate(x0, x1, t, use_ema=True)["loss"], other.evaluate(x0, x1, t)["loss"])
        other.close()
    assert not torch.equal(tr.evaluate(*_data(60), use_ema=True)["loss"], tr.evaluate(*_data(60))["loss"])
    tr.close()


def _mt_parts(precision, seed=7):
    torch.manual_seed(seed)
    enc = SharedEncoder(3, [16, 32], precision=precision).to(DEV).train()
    fdec = FlowMatchingDecoder(32, [16], 3, 32, precision=precision).to(DEV).train()
    sdec = SegmentationDecoder(32, [16], 1, precision=precision).to(DEV).train()
    return enc, fdec, sdec


def _mt_data(step, B=2, H=64):
    x0, x1, t = _data(step, B, H)
    g = torch.Generator().manual_seed(300 + step)
    mask = (torch.rand(B, 1, H, H, generator=g) > 0.5).float().to(DEV)
    return x0, x1, mask, t


def test_multitask_ema_matches_averaged_model_and_twin():
    parts = _mt_parts("fp32")
    tr = MultiTaskTrainer(*parts, time_emb_dim=32, lr=LR, ema_decay=DECAY)
    twin_parts = _mt_parts("fp32")
    twin = MultiTaskTrainer(*twin_parts, time_emb_dim=32, lr=LR)
    names = ("encoder", "flow_decoder", "seg_decoder")
    live = torch.nn.ModuleDict(dict(zip(names, parts)))
    ref = AveragedModel(copy.deepcopy(live).cpu(), multi_avg_fn=get_ema_multi_avg_fn(DECAY), use_buffers=True)
    live_cpu = copy.deepcopy(live).cpu()
    for s in range(STEPS):
        la, lb = tr.step(*_mt_data(s)), twin.step(*_mt_data(s))
        assert torch.equal(la, lb)
        live_cpu.load_state_dict({k: v.cpu() for k, v in live.state_dict().items()})
        ref.update_parameters(live_cpu)
        _compare_to_averaged(tr.ema_state_dict(), ref.state_dict())
    for x, y in ((tr.fp.p, twin.fp.p), (tr.fp.m, twin.fp.m), (tr.fp.v, twin.fp.v)):
        assert torch.equal(x, y)
    enc, fdec, sdec = tr.ema_model()
    assert not enc.training and fdec is not parts[1]
    # the averaged networks evaluate as fresh copies loaded from the EMA state
    fresh = _mt_parts("fp32", seed=11)
    mods = torch.nn.ModuleDict(dict(zip(names, fresh)))
    checkpoint.load_weights(mods, tr.ema_state_dict(), strip_prefix="module.")
    other = MultiTaskTrainer(*fresh, time_emb_dim=32, lr=LR)
    batch = _mt_data(70)
    got, want = tr.evaluate(*batch, use_ema=True), other.evaluate(*batch)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    for x in (tr, twin, other):
        x.close()


def test_without_ema_the_ema_methods_raise():
    net, tr = _cfm("bf16", ema=False)
    with pytest.raises(RuntimeError, match="ema_decay"):
        tr.ema_model()
    with pytest.raises(ValueError):
        CFMTrainer(_net(), ema_decay=1.5)
    tr.close()
