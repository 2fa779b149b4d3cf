"""EMA of the weights, host side: exports, host-side validation of the new entry points (no launch), decay checks, and the
AveragedModel state-dict layout with its integer buffers."""
import ctypes
import inspect

import pytest
import torch
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn


def test_new_symbols_are_exported():
    import stain2stain_amd as s
    from stain2stain_amd import _native
    assert "FusedEMA" in s.__all__ and s.FusedEMA is s.ema.FusedEMA
    for cls in (s.CFMTrainer, s.MultiTaskTrainer):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["ema_decay"].default is None and sig["ema_buffers"].default is True
        assert hasattr(cls, "ema_model") and hasattr(cls, "ema_state_dict") and hasattr(cls, "load_ema_state_dict")
        assert inspect.signature(cls.evaluate).parameters["use_ema"].default is False
    assert inspect.signature(s.checkpoint.save_checkpoint).parameters["ema_state"].default is None
    for name in ("s2s_adam_ema_step", "s2s_adam_ema_step_dev", "s2s_ema_multi_blocks", "s2s_ema_multi"):
        assert name in _native.declared_symbols()


def test_entry_points_return_status_codes_without_a_gpu():
    from stain2stain_amd import _native
    lib = _native.lib()
    a = ctypes.c_void_p(4096)                   # never dereferenced: every call below is refused before a launch
    odd = ctypes.c_void_p(4096 + 4)
    step = lambda p, g, m, v, e, n, st: lib.s2s_adam_ema_step(p, g, m, v, e, n, st, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0,
                                                              0.1, None)
    assert step(None, a, a, a, a, 8, 1) == -5
    assert step(a, a, a, a, None, 8, 1) == -5
    assert step(a, a, a, a, a, 0, 1) == -1
    assert step(a, a, a, a, a, 8, 0) == -1
    assert step(a, a, a, a, odd, 8, 1) == -2
    assert step(odd, a, a, a, a, 8, 1) == -2
    dev = lambda p, e, n, h, w: lib.s2s_adam_ema_step_dev(p, a, a, a, e, n, h, w, None)
    assert dev(a, a, 8, None, a) == -5
    assert dev(a, a, 8, a, None) == -5
    assert dev(a, a, -3, a, a) == -1
    assert dev(a, odd, 8, a, a) == -2
    # blocks: an empty tensor owns none (it must not shift the map), negative sizes are refused
    assert [lib.s2s_ema_multi_blocks(n) for n in (0, 1, 4096, 4097, 1000003)] == [0, 1, 1, 2, 245]
    assert lib.s2s_ema_multi_blocks(-1) == -1
    assert lib.s2s_ema_multi(None, 1, 1, a, None) == -5
    assert lib.s2s_ema_multi(a, 1, 1, None, None) == -5
    assert lib.s2s_ema_multi(a, 0, 1, a, None) == -1
    assert lib.s2s_ema_multi(a, 1, -1, a, None) == -1
    assert lib.s2s_ema_multi(a, 1, 1 << 31, a, None) == -1
    assert lib.s2s_ema_multi(a, 2, 0, a, None) == 0          # only empty tensors: nothing to launch


@pytest.mark.parametrize("decay", [-0.1, 1.5, float("inf")])
def test_decay_outside_unit_interval_raises_like_torch(decay):
    from stain2stain_amd import FlowUNet, FusedEMA, ops
    with pytest.raises(ValueError):
        get_ema_multi_avg_fn(decay)
    with pytest.raises(ValueError):
        ops.check_ema_decay(decay)
    with pytest.raises(ValueError):           # checked before anything else, on any device
        FusedEMA(FlowUNet(3, [16, 32], 3, 32), decay)


def test_decay_bounds_and_weights():
    from stain2stain_amd import ops
    assert ops.check_ema_decay(0) == 0.0 and ops.check_ema_decay(1) == 1.0
    assert ops.ema_weight(0, 0.9) == 1.0                 # the first update copies
    assert ops.ema_weight(1, 0.9) == 1 - 0.9 and ops.ema_weight(7, 0.999) == 1 - 0.999


def test_fused_ema_refuses_cpu_modules():
    from stain2stain_amd import FlowUNet, FusedEMA
    with pytest.raises(RuntimeError, match="GPU"):
        FusedEMA(FlowUNet(3, [16, 32], 3, 32), 0.9)


def _bump_batchnorm(net):
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.num_batches_tracked += 3
                m.running_mean.uniform_(-1, 1)


def test_state_dict_layout_matches_averaged_model_with_integer_buffers(tmp_path):
    from stain2stain_amd import FlowUNet, checkpoint
    from stain2stain_amd.ema import averaged_state_dict, split_averaged_state_dict
    torch.manual_seed(0)
    net = FlowUNet(3, [16, 32], 3, 32)
    _bump_batchnorm(net)
    ref = AveragedModel(net, multi_avg_fn=get_ema_multi_avg_fn(0.9), use_buffers=True)
    ref.update_parameters(net)            # (one update: a copy; later ones truncate the lerped count, see ema.py)
    sd = averaged_state_dict(ref.module.state_dict(), 1)
    assert list(sd) == list(ref.state_dict())                    # same keys, same order
    assert sd["n_averaged"].dtype == torch.int64 and sd["n_averaged"].dim() == 0 and int(sd["n_averaged"]) == 1
    ints = [k for k in sd if k.endswith("num_batches_tracked")]
    assert ints and all(sd[k].dtype == torch.int64 and int(sd[k]) == 3 for k in ints)
    # this project's state loads into AveragedModel, and back
    other = AveragedModel(FlowUNet(3, [16, 32], 3, 32), multi_avg_fn=get_ema_multi_avg_fn(0.9), use_buffers=True)
    other.load_state_dict(sd)
    for k, v in other.state_dict().items():
        assert v.dtype == sd[k].dtype and torch.equal(v, sd[k]), k
    n, inner = split_averaged_state_dict(ref.state_dict(), list(net.state_dict()))
    assert n == 1 and set(inner) == set(net.state_dict())
    assert all(inner[k].dtype == torch.int64 for k in inner if k.endswith("num_batches_tracked"))
    bad = dict(sd)
    bad.pop(ints[0])
    with pytest.raises(ValueError, match="missing"):
        split_averaged_state_dict(bad, list(net.state_dict()))
    with pytest.raises(ValueError, match="unexpected"):
        split_averaged_state_dict({**sd, "module.extra": torch.zeros(1)}, list(net.state_dict()))
    # a checkpoint carries it; load_weights puts it into a bare network, skipping n_averaged
    path = str(tmp_path / "ema.ckpt")
    checkpoint.save_checkpoint(path, net, ema_state=sd)
    ck = checkpoint.read_checkpoint(path)
    assert set(ck["ema_state_dict"]) == set(sd)
    bare = FlowUNet(3, [16, 32], 3, 32)
    rec = checkpoint.load_weights(bare, ck["ema_state_dict"], strip_prefix="module.")
    assert not rec.missing_keys and not rec.unexpected_keys
    for k, v in bare.state_dict().items():
        assert torch.equal(v, sd["module." + k]), k
    # without ema_state the checkpoint is what it was
    assert "ema_state_dict" not in checkpoint.save_checkpoint(str(tmp_path / "plain.ckpt"), net)
