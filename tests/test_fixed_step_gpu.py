"""Fixed-step Runge-Kutta samplers on the GPU (``fixed_step_integrate`` / ``fixed_step_generate``, csrc/ode.hip,
DESIGN.md 3.13): bit-equal to the ``clone`` + ``ops.axpy_`` chain, parity with the CPU oracle network under a tableau
typed out here, the observed order on an ODE with a known solution, captured == eager, independent of batch mates,
Euler untouched, reachable from every module face and the region sampler, correct on poisoned outputs."""
import numpy as np
import pytest
import torch

from conftest import load_golden, relerr, sub

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-3                                   # the project's fp32 statement (tests/test_e2e_gpu.py)
NAMES = ("euler", "midpoint", "heun", "rk4", "rk4_38")

# name -> (c, A rows, b), typed from the issue's table and deliberately NOT imported from the package
LITERAL = {
    "euler": ((0.0,), ((),), (1.0,)),
    "midpoint": ((0.0, 1 / 2), ((), (1 / 2,)), (0.0, 1.0)),
    "heun": ((0.0, 1.0), ((), (1.0,)), (1 / 2, 1 / 2)),
    "rk4": ((0.0, 1 / 2, 1 / 2, 1.0), ((), (1 / 2,), (0.0, 1 / 2), (0.0, 0.0, 1.0)), (1 / 6, 1 / 3, 1 / 3, 1 / 6)),
    "rk4_38": ((0.0, 1 / 3, 2 / 3, 1.0), ((), (1 / 3,), (-1 / 3, 1.0), (1.0, -1.0, 1.0)), (1 / 8, 3 / 8, 3 / 8, 1 / 8)),
}


def tiny_net(precision="fp32"):
    from stain2stain_amd import FlowUNet
    G = load_golden("tiny_step.npz")
    net = FlowUNet(3, [16, 32], 3, 32, precision=precision)
    net.load_state_dict(sub(G, "step1/after/"))
    return net.to(DEV).eval()


def tiles(B, seed, h=16, w=None):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 3, h, w or h, generator=g) * 2 - 1).to(DEV)


def chain_integrate(f, x, n, name):
    """The solve restated from kernels that predate the fused ones: a copy of x and one ``ops.axpy_`` per non-zero
    coefficient ``float(h * a)``, ascending j; node times ``k * h + c_i * h`` rounded once by ``torch.full``."""
    from stain2stain_amd import ops
    c, A, b = LITERAL[name]
    h = 1.0 / n
    for k in range(n):
        ks = []
        for i in range(len(c)):
            xi = x.clone()
            for j, a in enumerate(A[i]):
                if a != 0.0:
                    ops.axpy_(xi, ks[j], float(h * a))
            t = torch.full((x.shape[0],), k * h + c[i] * h, device=x.device, dtype=torch.float32)
            ks.append(f(t, xi).contiguous())
        for j, w in enumerate(b):
            if w != 0.0:
                ops.axpy_(x, ks[j], float(h * w))
    return x


# ---- 1. bit-equal to the axpy chain ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 16, 16), (3, 20, 36), (1, 8, 8)])     # 3*20*36 = 2160 floats: two blocks and a tail
@pytest.mark.parametrize("name", NAMES)
def test_bit_equal_to_the_clone_axpy_chain(name, shape):
    from stain2stain_amd import fixed_step_integrate
    net = tiny_net()
    B, h, w = shape
    x = tiles(B, 21, h, w)
    with torch.no_grad():
        want = chain_integrate(net, x.clone(), 3, name)
        y = x.clone()
        got = fixed_step_integrate(net, y, 3, name)
    assert got is y                                               # advanced in place and returned
    assert torch.equal(got, want), (name, shape, float((got - want).abs().max()))
    assert not torch.equal(got, x)


# ---- 2. parity with the oracle network ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_parity_with_the_oracle_network(name, golden_tiny):
    from oracle import unet_oracle as O
    from stain2stain_amd import fixed_step_generate
    G = golden_tiny
    P = sub(G, "step1/after/")
    net = tiny_net()
    n = 8
    x0 = G["euler/x_start"].float()
    c, A, b = LITERAL[name]
    h = 1.0 / n
    x = x0.clone()
    with torch.no_grad():
        for k in range(n):
            ks = []
            for i in range(len(c)):
                xi = x.clone()
                for j, a in enumerate(A[i]):
                    if a != 0.0:
                        xi = xi + (h * a) * ks[j]
                ks.append(O.flow_forward(torch.full((x.shape[0],), k * h + c[i] * h), xi, P, training=False))
            for j, w in enumerate(b):
                if w != 0.0:
                    x = x + (h * w) * ks[j]
    got = fixed_step_generate(net, x0.to(DEV), n, name)
    err = relerr(got, x)
    print(f"fixed-step parity {name}: rel err {err:.3e}")
    assert err < TOL, (name, err)


# ---- 3. observed order ----------------------------------------------------------------------------------------------
def _field(t, x):
    t = t.view(-1, 1, 1, 1)
    return (torch.cos(2.0 * t) * x - 0.5 * torch.sin(t) * x * x).contiguous()


def _exact(x0):
    """x(1) by classical RK4 in float64 with 4096 steps on the CPU."""
    x = x0.double().numpy().copy()
    f = lambda t, y: np.cos(2.0 * t) * y - 0.5 * np.sin(t) * y * y
    n = 4096
    h = 1.0 / n
    for k in range(n):
        t = k * h
        k1 = f(t, x)
        k2 = f(t + h / 2, x + h / 2 * k1)
        k3 = f(t + h / 2, x + h / 2 * k2)
        k4 = f(t + h, x + h * k3)
        x = x + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
    return x


ORDER_BOUNDS = {"euler": (0.9, 1.3), "midpoint": (1.9, 2.7), "heun": (1.9, 2.7), "rk4": (3.8, 4.7), "rk4_38": (3.8, 4.7)}


@pytest.mark.parametrize("name", NAMES)
def test_observed_order(name):
    from stain2stain_amd import fixed_step_integrate
    g = torch.Generator().manual_seed(5)
    x0 = 0.5 + torch.rand(4, 3, 8, 8, generator=g)
    want = _exact(x0)

    def err(n):
        got = fixed_step_integrate(_field, x0.to(DEV).clone(), n, name).double().cpu().numpy()
        return float(np.sqrt(np.mean((got - want) ** 2)))

    lo, hi = ORDER_BOUNDS[name]
    for n in ((4,) if lo > 3 else (4, 8)):           # 4th order at 16 steps sits at the fp32 floor
        e1, e2 = err(n), err(2 * n)
        p = float(np.log2(e1 / e2))
        print(f"observed order {name} n={n}: e_n {e1:.3e} e_2n {e2:.3e} p {p:.3f}")
        assert lo <= p <= hi, (name, n, p)


# ---- 4. graph equals eager ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", NAMES[1:])
def test_graph_equals_eager_and_repeats(name, precision):
    from stain2stain_amd import fixed_step_generate
    net = tiny_net(precision)
    x = tiles(3, 41)
    try:
        eager = fixed_step_generate(net, x, 3, name)
        a = fixed_step_generate(net, x, 3, name, graph=True)
        g0 = net._s2s_rk_graph
        b = fixed_step_generate(net, x, 3, name, graph=True)          # the counter is reset: same bits again
        assert torch.equal(a, eager) and torch.equal(b, eager), (name, precision)
        assert net._s2s_rk_graph is g0                                # cache hit
        assert not net.training
    finally:
        g = getattr(net, "_s2s_rk_graph", None)
        if g is not None:
            g.close()
    assert getattr(net, "_s2s_rk_graph", None) is None


def test_graph_cache_is_rebuilt_and_the_old_graph_closed():
    from stain2stain_amd import fixed_step_generate
    net = tiny_net()
    net.train()
    x = tiles(2, 43)
    a = fixed_step_generate(net, x, 3, "rk4", graph=True)
    assert net.training                                               # mode restored
    g0 = net._s2s_rk_graph
    b = fixed_step_generate(net, x, 3, "rk4_38", graph=True)          # another method
    g1 = net._s2s_rk_graph
    assert g1 is not g0 and g0.graph is None and torch.equal(b, fixed_step_generate(net, x, 3, "rk4_38"))
    c = fixed_step_generate(net, x, 4, "rk4_38", graph=True)          # another step count
    g2 = net._s2s_rk_graph
    assert g2 is not g1 and g1.graph is None and torch.equal(c, fixed_step_generate(net, x, 4, "rk4_38"))
    one = fixed_step_generate(net, x[:1], 4, "rk4_38", graph=True)    # another batch shape
    g3 = net._s2s_rk_graph
    assert g3 is not g2 and g2.graph is None and torch.equal(one, c[:1])
    with torch.no_grad():
        net.flow_decoder.outc.bias.add_(0.25)                         # new parameters
    d = fixed_step_generate(net, x[:1], 4, "rk4_38", graph=True)
    g4 = net._s2s_rk_graph
    assert g4 is not g3 and g3.graph is None
    assert not torch.equal(d, one) and torch.equal(d, fixed_step_generate(net, x[:1], 4, "rk4_38"))
    assert not torch.equal(a, b)
    g4.close()
    assert getattr(net, "_s2s_rk_graph", None) is None and g4.graph is None
    with pytest.raises(RuntimeError):
        g4.solve(x[:1])


# ---- 5. batch-mate independence -------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["rk4", "midpoint"])
def test_tiles_do_not_depend_on_their_batch_mates(name, precision):
    from stain2stain_amd import FlowUNet, fixed_step_generate
    torch.manual_seed(11)
    net = FlowUNet(3, [16, 32], 3, 32, precision=precision).to(DEV).eval()
    x = tiles(8, 5, 32)
    a = fixed_step_generate(net, x[:6], 3, name)
    order = [3, 6, 1, 5, 7, 0]                 # tiles 0, 1, 3, 5 shared, at new positions; 2, 4 replaced by 6, 7
    b = fixed_step_generate(net, x[order], 3, name)
    for pos, i in enumerate(order):
        if i < 6:
            assert torch.equal(b[pos], a[i]), (name, precision, i)


# ---- 6. Euler is untouched ------------------------------------------------------------------------------------------
def test_euler_delegates_to_the_existing_path(golden_tiny):
    from stain2stain_amd import euler_generate, euler_integrate, fixed_step_generate, fixed_step_integrate
    net = tiny_net()
    x = golden_tiny["euler/x_start"].to(DEV)
    n = int(golden_tiny["euler/n_steps"])
    want = euler_generate(net, x, n)
    assert relerr(want, golden_tiny["euler/x_end"]) < TOL
    assert torch.equal(fixed_step_generate(net, x, n, "euler"), want)
    assert torch.equal(fixed_step_generate(net, x, n, method="euler", graph=True), want)
    assert torch.equal(euler_generate(net, x, n, graph=True), want)
    assert getattr(net, "_s2s_rk_graph", None) is None               # the Euler graph, not a new one
    with torch.no_grad():
        assert torch.equal(fixed_step_integrate(net, x.clone(), n, "euler"), euler_integrate(net, x.clone(), n))
    net._s2s_euler_graph.close()


# ---- 7. module faces ------------------------------------------------------------------------------------------------
def test_every_module_face():
    from stain2stain_amd import (ClassConditionalFlowMatchingModule, ClassConditionalFlowUNet,
                                 ConditionalFlowMatchingModule, FlowMatchingDecoder, FlowUNet,
                                 MaskConditionedFlowMatchingModule, MultiTaskFlowMatchingModule, SegmentationDecoder,
                                 SharedEncoder, SolverConfig, fixed_step_integrate)
    x = tiles(2, 13)
    net = tiny_net()
    mod = ConditionalFlowMatchingModule(net, solver=SolverConfig())
    mod.train()
    with torch.no_grad():
        want = fixed_step_integrate(net.eval(), x.clone(), 4, "rk4")
        want_mid = fixed_step_integrate(net, x.clone(), 4, "midpoint")
    mod.train()
    assert torch.equal(mod.generate(x, 4, method="rk4"), want) and not mod.training      # left in eval mode
    assert torch.equal(mod.generate(x, 4, method="rk4", graph=True), want)
    assert not torch.equal(want, want_mid)
    mid = ConditionalFlowMatchingModule(net, solver=SolverConfig(solver="midpoint"))
    assert torch.equal(mid.generate(x, 4), want_mid)
    assert torch.equal(mid.generate(x, 4, method="rk4"), want)                           # method= wins
    with pytest.raises(ValueError):
        mid.generate(x, 4, per_sample=True)
    with pytest.raises(ValueError):
        mod.generate(x, 4, method="rk4", per_sample=True)

    torch.manual_seed(3)
    mask = (torch.rand(2, 1, 16, 16, device=DEV) > 0.5).float()
    mnet = FlowUNet(4, [16, 32], 3, 32, precision="fp32").to(DEV)
    mm = MaskConditionedFlowMatchingModule(mnet, solver=SolverConfig())
    got = mm.generate(x, mask, 4, method="rk4")
    with torch.no_grad():
        ref = fixed_step_integrate(lambda t, y: mnet(t, torch.cat([y, mask], dim=1)), x.clone(), 4, "rk4")
    assert torch.equal(got, ref) and not mm.training

    cnet = ClassConditionalFlowUNet(3, [16, 32], 3, 32, num_classes=3, precision="fp32").to(DEV)
    cm = ClassConditionalFlowMatchingModule(cnet, solver=SolverConfig())
    got = cm.generate(x, 2, 4, method="rk4")
    y = torch.tensor([2, 2], device=DEV)
    with torch.no_grad():
        ref = fixed_step_integrate(lambda t, z: cnet(t, z, y=y), x.clone(), 4, "rk4")
    assert torch.equal(got, ref) and not cm.training

    enc = SharedEncoder(3, [16, 32], precision="fp32")
    fdec = FlowMatchingDecoder(32, [16], 3, 32, precision="fp32")
    sdec = SegmentationDecoder(32, [16], 1, precision="fp32")
    mt = MultiTaskFlowMatchingModule(enc, fdec, sdec, time_emb_dim=32, solver=SolverConfig()).to(DEV)
    img, pm = mt.generate(x, 4, method="rk4")
    with torch.no_grad():
        ref = fixed_step_integrate(mt.forward_flow, x.clone(), 4, "rk4")
    assert torch.equal(img, ref) and pm.shape == (2, 1, 16, 16) and not mt.training


# ---- 8. region ------------------------------------------------------------------------------------------------------
def _gather_ref(img, origins, T):
    norm = lambda u8: (u8.astype(np.float32) / np.float32(255.0) - np.float32(0.5)) / np.float32(0.5)
    return np.stack([norm(img[y:y + T, x:x + T]).transpose(2, 0, 1) for y, x in origins])


def test_exact_tiling_matches_the_sampler_on_the_crops():
    from stain2stain_amd import FlowUNet, fixed_step_generate, translate_region
    from stain2stain_amd.region import plan_tiles
    torch.manual_seed(1984)
    net = FlowUNet(3, [16, 32, 64], 3, 32, precision="bf16").to(DEV)
    H, W, T, batch, steps = 96, 64, 32, 4, 4
    g = torch.Generator().manual_seed(5)
    img = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
    sampler = lambda x: fixed_step_generate(net, x, steps, "rk4", graph=True)
    u8, f = translate_region(img.to(DEV), sampler, tile=T, overlap=0, batch=batch, return_float=True)
    plan = plan_tiles(H, W, T, 0)
    crops = torch.from_numpy(_gather_ref(img.numpy(), plan.tolist(), T)).to(DEV)
    outs = []
    for p0 in range(0, crops.shape[0], batch):
        b = crops[p0:p0 + batch]
        if b.shape[0] < batch:
            b = torch.cat([b, b[-1:].expand(batch - b.shape[0], -1, -1, -1)])
        outs.append(sampler(b)[:min(batch, crops.shape[0] - p0)])
    ref = torch.cat(outs).cpu().numpy()
    net._s2s_rk_graph.close()
    side = np.zeros((H, W, 3), np.float32)
    for v, (y, x) in zip(ref, plan.tolist()):
        side[y:y + T, x:x + T] = v.transpose(1, 2, 0)
    assert np.array_equal(f.cpu().numpy(), side)
    want_u8 = np.clip((side * np.float32(0.5) + np.float32(0.5)) * np.float32(255.0), 0, 255).astype(np.uint8)
    assert np.array_equal(u8.cpu().numpy(), want_u8)


def test_multitask_sampler_takes_the_new_methods():
    from stain2stain_amd import (FlowMatchingDecoder, MultiTaskFlowMatchingModule, SegmentationDecoder, SharedEncoder,
                                 SolverConfig, fixed_step_integrate, multitask_sampler, translate_region)
    torch.manual_seed(7)
    enc = SharedEncoder(3, [16, 32], precision="fp32")
    fdec = FlowMatchingDecoder(32, [16], 3, 32, precision="fp32")
    sdec = SegmentationDecoder(32, [16], 1, precision="fp32")
    mt = MultiTaskFlowMatchingModule(enc, fdec, sdec, time_emb_dim=32, solver=SolverConfig()).to(DEV)
    x = tiles(2, 17)
    with torch.no_grad():
        want = fixed_step_integrate(mt.eval().forward_flow, x.clone(), 4, "rk4")
    for graph in (False, True):
        img, probs = multitask_sampler(mt, 4, graph=graph, method="rk4")(x)
        assert torch.equal(img, want) and probs.shape == (2, 1, 16, 16) and probs.dtype == torch.float32
        assert float(probs.detach().min()) >= 0.0 and float(probs.detach().max()) <= 1.0
    g = torch.Generator().manual_seed(4)
    region = (torch.rand(40, 56, 3, generator=g) * 255).to(torch.uint8).to(DEV)
    outs = []
    for graph in (False, True):
        u8, probs = translate_region(region, multitask_sampler(mt, 4, graph=graph, method="rk4"), tile=32, overlap=8,
                                     batch=4)
        assert u8.shape == (40, 56, 3) and probs.shape == (40, 56, 1)
        outs.append(u8)
    assert torch.equal(outs[0], outs[1])


# ---- 9. poisoned outputs and the wrappers' checks -------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 16, 16), (3, 3, 20, 36), (5, 4)])
def test_stage_and_combine_write_everything_on_poisoned_outputs(shape):
    from stain2stain_amd import ops
    g = torch.Generator().manual_seed(9)
    B = shape[0]
    x = torch.randn(*shape, generator=g).to(DEV)
    ks = [torch.randn(*shape, generator=g).to(DEV) for _ in range(4)]
    cs = [0.25, -0.125, 0.3, 0.7]
    table = torch.arange(12, dtype=torch.float32, device=DEV) * 0.0625
    for step in (0, 2):
        counter = torch.full((1,), step, dtype=torch.int32, device=DEV)
        for nk in (0, 1, 2, 3):
            out = torch.full_like(x, float("nan"))
            t = torch.full((B,), float("nan"), device=DEV)
            ops.rk_stage_(x, list(zip(cs[:nk], ks[:nk])), out, t, table, counter, 4, nk)
            want = x.clone()
            for c, k in zip(cs[:nk], ks[:nk]):
                ops.axpy_(want, k, c)
            assert not out.isnan().any() and torch.equal(out, want), (shape, nk)
            assert torch.equal(t, table[step * 4 + nk].expand(B)), (shape, nk)
            assert int(counter) == step                               # a stage launch only reads the counter
        t = torch.full((B,), float("nan"), device=DEV)
        ops.rk_stage_(x, [], None, t, table, counter, 4, 0)           # the node time alone
        assert torch.equal(t, table[step * 4].expand(B))
        for nk in (1, 2, 3, 4):
            y, want = x.clone(), x.clone()
            ops.rk_combine_(y, list(zip(cs[:nk], ks[:nk])), counter)
            for c, k in zip(cs[:nk], ks[:nk]):
                ops.axpy_(want, k, c)
            assert torch.equal(y, want), (shape, nk)
        assert int(counter) == step + 4                               # one tick per combine launch


def test_wrappers_refuse_bad_operands_before_any_launch():
    from stain2stain_amd import fixed_step_integrate, ops
    x = torch.zeros(2, 3, 4, 4, device=DEV)
    k = torch.ones_like(x)
    out = torch.empty_like(x)
    t = torch.zeros(2, device=DEV)
    table = torch.zeros(8, device=DEV)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    ok = lambda: ops.rk_stage_(x, [(0.5, k)], out, t, table, counter, 2, 1)
    ok()
    bad_stage = [
        lambda: ops.rk_stage_(x.cpu(), [(0.5, k)], out, t, table, counter, 2, 1),                   # not on the GPU
        lambda: ops.rk_stage_(x.double(), [(0.5, k)], out, t, table, counter, 2, 1),                # dtype
        lambda: ops.rk_stage_(x.transpose(2, 3), [(0.5, k)], out, t, table, counter, 2, 1),         # contiguity
        lambda: ops.rk_stage_(x, [(0.5, k[:, :, :, :3])], out, t, table, counter, 2, 1),            # k's shape
        lambda: ops.rk_stage_(x[:, :, :3, :3].contiguous(), [], None, t, table, counter, 2, 0),     # n % 4
        lambda: ops.rk_stage_(x, [(0.5, k)], x, t, table, counter, 2, 1),                           # in place
        lambda: ops.rk_stage_(x, [(0.5, k)], None, t, table, counter, 2, 1),                        # terms, no output
        lambda: ops.rk_stage_(x, [(0.5, k)] * 4, out, t, table, counter, 2, 1),                     # too many terms
        lambda: ops.rk_stage_(x, [(0.5, k)], out, t, table, counter, 2, 2),                         # stage >= stages
        lambda: ops.rk_stage_(x, [(0.5, k)], out, t[:1], table, counter, 2, 1),                     # t_out's shape
        lambda: ops.rk_stage_(x, [(0.5, k)], out, t, table, counter.long(), 2, 1),                  # counter dtype
        lambda: ops.rk_combine_(x, [], counter),
        lambda: ops.rk_combine_(x, [(0.5, k)] * 5, counter),
        lambda: ops.rk_combine_(x, [(0.5, x)], counter),
        lambda: ops.rk_combine_(x, [(0.5, k.half())], counter),
    ]
    for i, call in enumerate(bad_stage):
        with pytest.raises(RuntimeError):
            call()
    flat = torch.zeros(2 * 48 + 1, device=DEV)[1:].view(2, 3, 4, 4)      # 4-byte offset: contiguous, misaligned
    with pytest.raises(RuntimeError, match="aligned"):
        ops.rk_stage_(flat, [(0.5, k)], out, t, table, counter, 2, 1)
    with pytest.raises(RuntimeError, match="aligned"):
        ops.rk_combine_(flat, [(0.5, k)], counter)
    f = lambda tt, xx: xx.clone()
    with pytest.raises(RuntimeError):
        fixed_step_integrate(f, torch.zeros(2, 3, 4, 4), 2, "rk4")       # host tensor
    with pytest.raises(RuntimeError):
        fixed_step_integrate(f, torch.zeros(2, 3, 3, 3, device=DEV), 2, "rk4")
    with pytest.raises(ValueError):
        fixed_step_integrate(f, x, 0, "rk4")
    assert int(counter) == 0 and float(x.abs().max()) == 0.0
