"""The fused tail (ops.tail_fwd_loss / ops.tail_bwd_apply: last BatchNorm + ReLU, head, MSE loss and their backward in
two passes over the last conv output) against the chain it replaces,

    bn_relu_apply -> head_loss_fused -> bn_relu_bwd,

on the same inputs, both measured against an fp64 CPU evaluation of that chain which rounds the activation and the head's
data gradient to the storage type T where the chain stores them.  Per output the fused path's maximum error may be at
most twice the chain's (for the T-typed ``d raw`` plus one ulp of T per element).  The fused passes also round at the
chain's points and sum in the chain's order, so beyond that bound every output has to equal the chain's bit for bit.
Every buffer the ops allocate starts out as NaN (tests/test_unwritten_memory_gpu.py's poison).

Then the trainers: ``fuse_tail`` on and off from the same seed, three optimisation steps, held to the bound
tests/test_e2e_gpu.py holds the fused trainer to against its golden steps (1e-3 of the loss; 1e-3 of each tensor's
maximum plus Adam's sign slack of ``slack * lr * steps`` on the parameters).  Four networks, batch 2: features [8, 16] on
32 x 32 tiles; the default first-level width (64 channels into the head, the headline's tail kernels) as [64, 128] on
16 x 16 tiles; all five default levels on 16 x 16 tiles; and a first level of 128 channels, [128, 256] on 16 x 16 tiles,
whose chain head_loss_fused refused until its limits were applied to the one-thread-per-pixel kernel alone.  (The last leaves a 1 x 1 bottleneck whose BatchNorm
normalises two values per channel: there a one-ulp change of one weight alone moves the third step's loss by 1e-4 of its
value, and a fused tail that summed in another order than the chain moved it by 1e-2.  It passes because the fused
results are the chain's bit for bit.)

Every form of the tail kernels (all seven widths, both output-loop instantiations, odd and even round counts) against
float64: tests/test_head_tail_forms_gpu.py, DESIGN.md 3.29."""
import itertools

import pytest
import torch

import stepwise_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-3                  # tests/test_e2e_gpu.py

SIZES = [(1, 5, 7), (2, 16, 16), (3, 33, 18)]      # 35 pixels: less than one workgroup's 256 / (C / 8) at C = 8 and 16
CHANNELS = [8, 16, 64]
# cout, head bias, want_v, accumulate, raw a strided view
OPTIONS = [(3, True, True, False, False), (3, False, False, True, True), (1, True, False, False, True),
           (1, False, True, True, False), (3, True, True, True, True), (3, False, False, False, False)]
CASES = []
for _di, _dt in enumerate((torch.bfloat16, torch.float32)):
    for _i, (_size, _C) in enumerate(itertools.product(SIZES, CHANNELS)):
        CASES.append((_dt, _size, _C) + OPTIONS[(_i + 2 * _di) % len(OPTIONS)])


def _case_id(c):
    dt, (B, H, W), C, cout, bias, want_v, acc, strided = c
    return (f"{'bf16' if dt == torch.bfloat16 else 'fp32'}-{B}x{H}x{W}-C{C}-o{cout}" + ("-bias" if bias else "")
            + ("-v" if want_v else "") + ("-acc" if acc else "") + ("-ld" if strided else ""))


@pytest.fixture(autouse=True)
def poison():
    import torch.utils.deterministic as tud
    prev_det, prev_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    prev_fill = tud.fill_uninitialized_memory
    torch.use_deterministic_algorithms(True, warn_only=True)
    tud.fill_uninitialized_memory = True
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev_det, warn_only=prev_warn)
        tud.fill_uninitialized_memory = prev_fill


def _round(x, dt):
    """fp64 / fp32 -> the storage type T and back (fp32 values)."""
    return x.float().to(dt).float()


def _ulp(ref, dt):
    bits = 7 if dt == torch.bfloat16 else 23
    return torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - bits)


def _reference(raw, stats, gamma, w, b, u, dt):
    """The chain in fp64 from the stored inputs; the activation and d act rounded to T where the chain stores them."""
    stats = stats.detach().cpu().float()
    raw = raw.detach().cpu().float()
    cout = w.shape[0]
    z = R.fma_f32(raw, stats[2], stats[3])
    act = _round(z.clamp_min(0.0), dt).double()
    wm = w.detach().cpu().double().reshape(cout, -1)
    v = act @ wm.t()
    if b is not None:
        v = v + b.detach().cpu().double()
    d = v - u.detach().cpu().double().permute(0, 2, 3, 1)
    loss = (d * d).mean()
    g = d * (2.0 / d.numel())
    dact = _round(g @ wm, dt)
    dz = torch.where(z > 0, dact, torch.zeros_like(dact)).double()
    xh = ((raw - stats[0]) * stats[1]).double()
    C = raw.shape[-1]
    n = raw.numel() // C
    dbeta = dz.reshape(-1, C).sum(0)
    dgamma = (dz * xh).reshape(-1, C).sum(0)
    draw = (gamma.detach().cpu().double() * stats[1].double()) * (dz - dbeta / n - xh * (dgamma / n))
    return dict(v=v.permute(0, 3, 1, 2), loss=loss, g=g.permute(0, 3, 1, 2), draw=draw,
                dw=torch.einsum("bhwo,bhwc->oc", g, act), db=g.sum((0, 1, 2)), dgamma=dgamma, dbeta=dbeta,
                dbias=torch.zeros(C, dtype=torch.float64))


@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_fused_tail_against_the_chain(case):
    from stain2stain_amd import ops
    dt, (B, H, W), C, cout, has_bias, want_v, acc, strided = case
    gen = torch.Generator().manual_seed(1984 + 7 * C + H)
    ld = C + 8 if strided else C
    buf = torch.full((B, H, W, ld), float("nan"), dtype=dt, device=DEV)
    raw = buf[..., :C]
    # per-channel offsets and spreads: some channels mostly off, some mostly on
    x = torch.randn(B, H, W, C, generator=gen) * (0.5 + torch.rand(C, generator=gen)) + torch.randn(C, generator=gen)
    raw.copy_(x.to(DEV))
    gamma = (torch.rand(C, generator=gen) + 0.5).to(DEV)
    beta = (torch.rand(C, generator=gen) - 0.5).to(DEV)
    w = ((torch.rand(cout, C, 1, 1, generator=gen) * 2 - 1) * 0.3).to(DEV)
    b = ((torch.rand(cout, generator=gen) * 2 - 1) * 0.1).to(DEV) if has_bias else None
    u = (torch.rand(B, cout, H, W, generator=gen) * 2 - 1).to(DEV)
    # statistics as the conv epilogue leaves them: one partial row
    r64 = raw.double().reshape(-1, C)
    stat = torch.stack([r64.sum(0), (r64 * r64).sum(0)]).float().reshape(2, C, 1).contiguous()
    stats = ops.bn_finalize(stat, B * H * W, gamma, beta, None, None, None)

    def grads():
        # accumulate: onto known finite values; otherwise the kernels must overwrite NaN
        fill = (lambda *s: torch.rand(*s, generator=gen).to(DEV) - 0.5) if acc else \
            (lambda *s: torch.full(s, float("nan"), device=DEV))
        return dict(dw=fill(cout, C, 1, 1), db=fill(cout) if has_bias else None, dgamma=fill(C), dbeta=fill(C),
                    dbias=fill(C))
    base = grads()
    old = {k: None if t is None else t.clone() for k, t in base.items()}
    new = {k: None if t is None else t.clone() for k, t in base.items()}

    # the chain
    act, _ = ops.bn_relu_apply(raw, stats[2], stats[3])
    loss_o, dact, v_o = ops.head_loss_fused(act, w, b, u, old["dw"], old["db"], want_v=True, accumulate=acc)
    draw_o = ops.bn_relu_bwd(dact, None, raw, stats, gamma, old["dgamma"], old["dbeta"], old["dbias"], accumulate=acc)
    g_o = (v_o - u) * (2.0 / u.numel())     # the chain has no g tensor; its v gives it to fp32 rounding
    # the fused pair
    loss_n, g_n, v_n, work = ops.tail_fwd_loss(raw, stats, w, b, u, new["dw"], new["db"], new["dgamma"], new["dbeta"],
                                               new["dbias"], want_v=want_v, accumulate=acc)
    draw_n = ops.tail_bwd_apply(raw, stats, w, g_n, gamma, work)
    torch.cuda.synchronize()
    assert (v_n is not None) == want_v
    assert draw_n.shape == raw.shape and draw_n.dtype == dt and g_n.shape == u.shape

    ref = _reference(raw, stats, gamma, w, b, u, dt)
    if acc:
        for k in ("dw", "db", "dgamma", "dbeta", "dbias"):
            if base[k] is not None:
                ref[k] = ref[k] + base[k].detach().cpu().double().reshape(ref[k].shape)
    got_old = dict(v=v_o, loss=loss_o, g=g_o, draw=draw_o, dw=old["dw"], db=old["db"], dgamma=old["dgamma"],
                   dbeta=old["dbeta"], dbias=old["dbias"])
    got_new = dict(v=v_n, loss=loss_n, g=g_n, draw=draw_n, dw=new["dw"], db=new["db"], dgamma=new["dgamma"],
                   dbeta=new["dbeta"], dbias=new["dbias"])
    bad = []
    for k, r in ref.items():
        if got_new[k] is None:      # v not asked for, no head bias
            continue
        o = got_old[k].detach().cpu().double().reshape(r.shape)
        n = got_new[k].detach().cpu().double().reshape(r.shape)
        assert bool(torch.isfinite(n).all()), k
        e_old, e_new = float((o - r).abs().max()), float((n - r).abs().max())
        print(f"{_case_id(case)} {k}: chain {e_old:.3e} fused {e_new:.3e}")
        if acc and k == "dbias":
            # the conv-bias gradient is exactly zero: accumulating leaves the buffer as it was
            ok = torch.equal(new["dbias"], base["dbias"])
        elif k == "draw":
            ok = bool(((n - r).abs() <= 2.0 * e_old + _ulp(r, dt)).all())
        else:
            ok = e_new <= 2.0 * e_old
        if not ok:
            bad.append(f"{k}: chain {e_old:.3e} fused {e_new:.3e}")
    assert not bad, bad
    # every sum is taken in the chain's own order (pass A on head_loss_fused's grid, the BatchNorm sums on
    # bn_relu_bwd's): the fused results are the chain's bit for bit, which is what keeps a training run on its path
    differ = [k for k in ref if got_new[k] is not None and k != "g"
              and not torch.equal(got_new[k].reshape(-1), got_old[k].reshape(-1))]
    assert not differ, differ


def _tiny_batch(nb, size, seed=5):
    g = torch.Generator().manual_seed(seed)
    x0 = (torch.rand(nb, 3, size, size, generator=g) * 2 - 1).to(DEV)
    x1 = (torch.rand(nb, 3, size, size, generator=g) * 2 - 1).to(DEV)
    return x0, x1, torch.rand(3, nb, generator=g).to(DEV)


def _check_params(got, ref, lr, steps):
    for k, r in ref.items():
        if k.endswith("num_batches_tracked"):
            assert int(got[k]) == int(r), k
            continue
        slack = 1.0 if k.endswith(("double_conv.0.bias", "double_conv.3.bias")) else 0.05
        err = float((got[k].float() - r.float()).abs().max())
        assert err <= TOL * float(r.abs().max()) + slack * lr * steps, (k, err)


@pytest.mark.parametrize("features,size", [([8, 16], 32), ([64, 128], 16), (None, 16), ([128, 256], 16)],
                         ids=["tiny", "c64", "default16", "c128"])
def test_cfm_trainer_fused_tail_equals_the_chain(features, size):
    from stain2stain_amd import CFMTrainer, FlowUNet, ops
    lr, steps = 1e-4, 3
    x0, x1, t = _tiny_batch(2, size)
    runs = {}
    for fuse in (False, True):
        torch.manual_seed(1984)
        net = (FlowUNet(3, features, 3, 32, precision="fp32") if features else FlowUNet(precision="fp32")).to(DEV).train()
        tr = CFMTrainer(net, lr=lr, weight_decay=1e-5)
        assert tr.fuse_tail is True       # the default
        tr.fuse_tail = fuse
        ops.profile_start(("tail_fwd_loss", "tail_bwd_apply", "head_loss_fused"))
        losses = [float(tr.step(x0, x1, t[s])) for s in range(steps)]
        names = sorted({p[0].split("@")[0] for p in ops.profile_stop()})
        assert names == (["tail_bwd_apply", "tail_fwd_loss"] if fuse else ["head_loss_fused"]), names
        torch.cuda.synchronize()
        runs[fuse] = (losses, {k: v.detach().cpu().clone() for k, v in net.state_dict().items()})
        tr.close()
    print("losses", runs[False][0], runs[True][0])
    for a, b in zip(runs[True][0], runs[False][0]):
        assert abs(a - b) <= TOL * abs(b), (a, b)
    _check_params(runs[True][1], runs[False][1], lr, steps)


def test_multitask_trainer_fused_tail_equals_the_chain():
    from stain2stain_amd import FlowMatchingDecoder, MultiTaskTrainer, SegmentationDecoder, SharedEncoder
    lr, steps = 1e-4, 3
    x0, x1, t = _tiny_batch(2, 32)
    mask = (torch.rand(2, 1, 32, 32, generator=torch.Generator().manual_seed(9)) > 0.5).float().to(DEV)
    runs = {}
    for fuse in (False, True):
        torch.manual_seed(1984)
        enc = SharedEncoder(3, [8, 16], precision="fp32").to(DEV).train()
        fdec = FlowMatchingDecoder(16, [8], 3, 32, precision="fp32").to(DEV).train()
        sdec = SegmentationDecoder(16, [8], 1, precision="fp32").to(DEV).train()
        tr = MultiTaskTrainer(enc, fdec, sdec, time_emb_dim=32, lr=lr, weight_decay=1e-5)
        assert tr.fuse_tail is True
        tr.fuse_tail = fuse
        losses = [float(tr.step(x0, x1, mask, t[s])) for s in range(steps)]
        torch.cuda.synchronize()
        state = {f"{i}.{k}": v.detach().cpu().clone() for i, m in enumerate((enc, fdec, sdec))
                 for k, v in m.state_dict().items()}
        runs[fuse] = (losses, state)
    print("losses", runs[False][0], runs[True][0])
    for a, b in zip(runs[True][0], runs[False][0]):
        assert abs(a - b) <= TOL * abs(b), (a, b)
    _check_params(runs[True][1], runs[False][1], lr, steps)
