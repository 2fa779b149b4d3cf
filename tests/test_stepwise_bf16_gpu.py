"""The bf16 steps layer by layer, teacher-forced: a real step runs once under ``stepwise_ref.Recorder``, which keeps what
every layer received and produced, and each layer is then checked against a plain CPU reference fed with THOSE bf16
inputs.  ReLU masks and pool winners come from the step's own tensors, so the backward is linear and every layer can be
held to the per-op tolerances (tests/test_ops_gpu.py) inside the real trainer at the headline configuration -- where the
end-to-end comparison with the parity mode (test_production_shapes_gpu.py) can only bound a chaotic divergence.

What is checked, per layer: the conv output against the conv of the recorded inputs with the bf16-rounded master weight;
the statistics rows against fp64 statistics of the stored output; the running statistics (late conv bias, unbiased
variance) against their values before the call; the activation to 1 bf16 ulp; the pooled activation bit-equal; which
tensor each launch read (routing identities); the head, loss and time path; the BatchNorm backward from the recorded
incoming gradients; the final conv weight gradient (side stream) against the weight gradient of the recorded ``draw``;
the data gradient; the up-sampling backward and the split of the concat gradient; the conv launch families.

Tolerances (upper limits, from the per-op suite): 4e-3 max-norm relative for bf16-stored tensors, 1e-4 for fp32 outputs
(statistics, parameter gradients), 1e-5 for the loss; plus an L2-relative bound per tensor (2.2e-3 bf16, 1e-4 fp32) that
catches widespread small errors a max-norm bound lets through.  Measured on an MI355X: bf16-stored tensors 2.9e-3 ..
3.7e-3 max-norm and 1.66e-3 .. 1.73e-3 in L2 (the statistics of one bf16 rounding: half an ulp is 2^-9 .. 2^-8 of the
value), fp32 outputs <= 8.7e-6 (conv weight gradients; statistics, running statistics, BatchNorm and head gradients
<= 2.1e-7), the loss 2.4e-9, the activation 0 ulps.  The file runs in about a minute.  Forward and data gradients are
compared on samples {0, B-1} (a convolution treats samples independently); batch-coupled quantities on the whole batch.
S2S_TEST_REPORT=1 prints every measured margin."""
import os
import time

import pytest
import torch

import stepwise_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, SIZE = 16, 256                      # the headline configuration (BASELINE.json): batch 16, 256x256, default widths
NLEV = 5
TOL_BF, TOL_F32, TOL_LOSS = 4e-3, 1e-4, 1e-5
L2_BF, L2_F32 = 2.2e-3, 1e-4
# the 3x3 launch families the headline step runs (conv3x3_mfma.hip's plan at these shapes, default environment)
HEADLINE_FAMILIES = {"kStageResident", "kStageStream", "kTap"}


class Checks:
    """Collects every measured margin of one test; ``done()`` prints them (S2S_TEST_REPORT) and fails with the list of
    all violations, so one run shows the whole picture."""

    def __init__(self, title):
        self.title, self.rows, self.bad = title, [], []
        self.t0 = time.time()

    def le(self, cat, what, value, bound):
        self.rows.append((cat, what, value, bound))
        if not value <= bound:          # (NaN fails)
            self.bad.append(f"{cat} {what}: {value:.3e} > {bound:.1e}")

    def true(self, cat, what, ok):
        self.rows.append((cat, what, 0.0 if ok else 1.0, 0.0))
        if not ok:
            self.bad.append(f"{cat} {what}")

    def bf(self, cat, what, got, ref):
        self.le(cat + " max", what, R.rel_max(got, ref), TOL_BF)
        self.le(cat + " L2", what, R.rel_l2(got, ref), L2_BF)

    def f32(self, cat, what, got, ref, tol=TOL_F32):
        self.le(cat + " max", what, R.rel_max(got, ref), tol)
        self.le(cat + " L2", what, R.rel_l2(got, ref), max(tol, L2_F32))

    def done(self):
        if os.environ.get("S2S_TEST_REPORT"):
            print(f"\n== {self.title}: {time.time() - self.t0:.1f} s")
            worst = {}
            for cat, what, v, b in self.rows:
                if b > 0:
                    print(f"  {cat:28s} {v:.3e} (bound {b:.0e})  {what}")
                    if v > worst.get(cat, (-1.0, ""))[0]:
                        worst[cat] = (v, what)
            for cat, (v, what) in sorted(worst.items()):
                print(f"  largest {cat:20s} {v:.3e}  {what}")
        assert not self.bad, "\n".join(self.bad)


def enc_name(l, j):
    return ("inc.double_conv" if l == 0 else f"downs.{l - 1}.maxpool_conv.1.double_conv") + (".0" if j == 0 else ".3")


def dec_name(i, j):
    return f"ups.{i}.conv.double_conv" + (".0" if j == 0 else ".3")


def same(a, b):
    return a is None and b is None or (a is not None and b is not None and a.shape == b.shape and torch.equal(a, b))


def _batch(nb, seed=1984):
    g = torch.Generator().manual_seed(seed)
    x0 = (torch.rand(nb, 3, SIZE, SIZE, generator=g) * 2 - 1).to(DEV)
    x1 = (torch.rand(nb, 3, SIZE, SIZE, generator=g) * 2 - 1).to(DEV)
    return x0, x1, torch.rand(nb, generator=g).to(DEV)


def _grads(mods):
    return {f"{i}.{n}": p.grad.detach().clone() for i, m in enumerate(mods) for n, p in m.named_parameters()}


# ---------------------------------------------------------------------------------------------------------------------
# per-layer checks shared by the trainers
# ---------------------------------------------------------------------------------------------------------------------
def _sel(nb):
    return [0, nb - 1]


def check_train_forward(ck, r, nb):
    """One recorded training-mode conv + BN + ReLU (+ pool) layer."""
    cb, name = r["cb"], r["name"]
    sel = _sel(nb)
    w = R.bf(cb.conv.weight.detach().cpu())
    x = R.stem_image(r["x0"][sel]) if r["stem"] else \
        R.cat_input(r["x0"][sel], None if r["x1"] is None else r["x1"][sel])
    ck.bf("fwd raw", name, R.to_nchw(r["raw"][sel]), R.conv3x3(x, w))           # bf16 mode: no bias in the conv
    st = R.bn_stats(r["raw"])
    k = r["stats"].detach().cpu().double()
    gamma, beta = cb.bn.weight.detach(), cb.bn.bias.detach()
    scale, shift = R.bn_affine(st, gamma, beta)
    ck.f32("stats mean", name, k[0], st["mean"])
    ck.f32("stats invstd", name, k[1], st["invstd"])
    ck.f32("stats scale", name, k[2], scale)
    ck.f32("stats shift", name, k[3], shift)
    rm, rv = R.bn_running(r["rm0"], r["rv0"], st, cb.bn.momentum, cb.conv.bias)
    ck.f32("running_mean", name, r["rm1"], rm)
    ck.f32("running_var", name, r["rv1"], rv)
    ck.true("num_batches_tracked", name, int(r["nbt1"]) == int(r["nbt0"]) + 1)
    _, ys = R.bn_relu_apply(r["raw"], r["stats"][2], r["stats"][3])
    ck.le("act ulps", name, float(R.bf16_ulps(r["act"].float(), ys).max()), 1.0)
    if r["pooled"] is not None:
        a = r["act"]
        n, H, W, C = a.shape
        ck.true("pooled bit-equal", name, torch.equal(r["pooled"], a.view(n, H // 2, 2, W // 2, 2, C).amax((2, 4))))


def check_bn_backward(ck, rec, b):
    """BatchNorm + ReLU (+ pool) backward of one recorded layer, from its recorded incoming gradients.  Returns the fp64
    (dgamma, dbeta) and the conv weight gradient of the recorded ``draw`` (fp32 CPU)."""
    f = rec.fwd_of(b)
    cb, name = b["cb"], b["name"]
    draw_ref, dgam, dbet = R.bn_relu_bwd(b["g1"], b["gp"], f["raw"], f["stats"], cb.bn.weight)
    ck.bf("bwd draw", name, b["draw"], draw_ref)
    del draw_ref
    x = R.stem_image(f["x0"]) if b["stem"] else R.cat_input(f["x0"], f["x1"])
    wg = R.conv3x3_wgrad(x, R.to_nchw(b["draw"]))
    return dgam, dbet, wg


def check_dgrad(ck, b, nb):
    cb, name = b["cb"], b["name"]
    if not b["need_dx"]:
        ck.true("dx absent", name, b["dx"] is None)
        return
    sel = _sel(nb)
    ref = R.conv3x3_dgrad(R.to_nchw(b["draw"][sel]), R.bf(cb.conv.weight.detach().cpu()))
    ck.bf("bwd dx", name, R.to_nchw(b["dx"][sel]), ref)


# ---------------------------------------------------------------------------------------------------------------------
# a. CFMTrainer, bf16, headline configuration
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cfm():
    from stain2stain_amd import CFMTrainer, FlowUNet
    torch.manual_seed(1984)
    net = FlowUNet(precision="bf16").to(DEV).train()
    tr = CFMTrainer(net, lr=1e-4, weight_decay=1e-5)
    assert tr.overlap_wgrad
    x0, x1, t = _batch(B)
    buffers0 = {k: v.clone() for k, v in net.named_buffers()}
    torch.cuda.synchronize()
    t0 = time.time()
    with R.Recorder() as rec:
        loss, v = tr.forward_backward(x0, x1, t)
    torch.cuda.synchronize()
    out = dict(net=net, tr=tr, rec=rec, loss=loss.clone(), v=v.clone(), grads=_grads([net]), buffers0=buffers0,
               buffers1={k: v_.clone() for k, v_ in net.named_buffers()}, x0=x0, x1=x1, t=t, step_s=time.time() - t0)
    yield out
    tr.close()


def test_cfm_forward_layers(cfm):
    rec = cfm["rec"]
    ck = Checks("CFM bf16 forward, per layer")
    with R.cpu_thread_share():
        assert len(rec.calls["fwd"]) == 2 * NLEV + 2 * (NLEV - 1)
        for r in rec.calls["fwd"]:
            assert r["training"]
            check_train_forward(ck, r, B)
    ck.done()


def test_cfm_routing(cfm):
    """Which tensor every launch read: identities between the recorded tensors (bit-equal clones)."""
    rec = cfm["rec"]
    ck = Checks("CFM bf16 routing")
    L = NLEV - 1
    fw, bw = rec.fwd, rec.bwd
    xt = rec.calls["cfm_sample"][0]["out"][0]
    ck.true("route", "stem input is xt", same(fw(enc_name(0, 0))["x0"], xt))
    for l in range(NLEV):
        ck.true("route", f"enc {l} conv2 <- conv1 act", same(fw(enc_name(l, 1))["x0"], fw(enc_name(l, 0))["act"]))
        if l < L:
            ck.true("route", f"enc {l + 1} conv1 <- pool {l}", same(fw(enc_name(l + 1, 0))["x0"], fw(enc_name(l, 1))["pooled"]))
        else:
            ck.true("route", "bottleneck not pooled", fw(enc_name(l, 1))["pooled"] is None)
    tbias = rec.calls["linear_fwd"][2]["out"]
    ups = rec.calls["upsample2x_fwd"]
    assert len(ups) == L
    for i in range(L):
        low, _, bias = ups[i]["args"]
        up = ups[i]["after"][1]
        ck.true("route", f"ups {i} low", same(low, fw(enc_name(L, 1))["act"] if i == 0 else fw(dec_name(i - 1, 1))["act"]))
        ck.true("route", f"ups {i} time bias", same(bias, tbias if i == 0 else None))
        c1 = fw(dec_name(i, 0))
        ck.true("route", f"dec {i} conv1 x0 = skip", same(c1["x0"], fw(enc_name(L - 1 - i, 1))["act"]))
        ck.true("route", f"dec {i} conv1 x1 = up", same(c1["x1"], up))
        ck.true("route", f"dec {i} conv2 <- conv1 act", same(fw(dec_name(i, 1))["x0"], c1["act"]))
    head = rec.calls["head_loss_fused"][0]
    ck.true("route", "head input", same(head["args"][0], fw(dec_name(L - 1, 1))["act"]))
    ck.true("route", "head target is ut", same(head["args"][3], rec.calls["cfm_sample"][0]["out"][1]))
    # backward
    g_head = head["out"][1]
    ck.true("route", "dec 3 conv2 <- g_head", same(bw(dec_name(L - 1, 1))["g1"], g_head) and bw(dec_name(L - 1, 1))["gp"] is None)
    ubw = rec.calls["upsample2x_bwd"]
    assert len(ubw) == L
    for i in range(L - 1, -1, -1):
        c1, c2 = bw(dec_name(i, 0)), bw(dec_name(i, 1))
        ck.true("route", f"dec {i} conv1 <- conv2 dx", same(c1["g1"], c2["dx"]) and c1["gp"] is None)
        cs = fw(dec_name(i, 0))["x0"].shape[3]
        u = ubw[L - 1 - i]
        ck.true("route", f"ups {i} bwd <- dcat[cs:]", same(u["args"][0], c1["dx"][..., cs:]))
        if i > 0:
            ck.true("route", f"dec {i - 1} conv2 <- ups {i} bwd", same(bw(dec_name(i - 1, 1))["g1"], u["out"]))
        l = L - 1 - i
        ck.true("route", f"enc {l} conv2 <- dskip {i}", same(bw(enc_name(l, 1))["g1"], c1["dx"][..., :cs]))
        ck.true("route", f"enc {l} conv2 <- gpool", same(bw(enc_name(l, 1))["gp"], bw(enc_name(l + 1, 0))["dx"]))
    ck.true("route", "bottleneck <- ups 0 bwd", same(bw(enc_name(L, 1))["g1"], ubw[L - 1]["out"]) and bw(enc_name(L, 1))["gp"] is None)
    ck.true("route", "time path <- ups 0 bwd", same(rec.calls["pixel_sum"][0]["args"][0], ubw[L - 1]["out"]))
    for l in range(NLEV):
        ck.true("route", f"enc {l} conv1 <- conv2 dx", same(bw(enc_name(l, 0))["g1"], bw(enc_name(l, 1))["dx"]))
    ck.true("route", "stem has no dx", bw(enc_name(0, 0))["dx"] is None)
    ck.done()


def test_cfm_head_loss_time_path_and_glue(cfm):
    rec, net = cfm["rec"], cfm["net"]
    dec = net.flow_decoder
    ck = Checks("CFM bf16 head, loss, time path, glue")
    sel = _sel(B)
    with R.cpu_thread_share():
        xt, ut = R.cfm_sample(cfm["x0"], cfm["x1"], cfm["t"])
        s = rec.calls["cfm_sample"][0]["out"]
        ck.f32("cfm_sample", "xt", s[0], xt, 1e-6)
        ck.f32("cfm_sample", "ut", s[1], ut, 1e-6)
        temb = rec.calls["time_embedding"][0]["out"]
        ck.f32("time embedding", "t_emb", temb, R.time_embedding(cfm["t"], net.time_embedding.dim))
        tb, _ = R.time_path(temb, dec)
        ck.f32("time bias", "time_proj out", rec.calls["linear_fwd"][2]["out"], tb)
        for i, u in enumerate(rec.calls["upsample2x_fwd"]):
            low, _, bias = u["args"]
            ck.bf("up", f"ups {i}", u["after"][1][sel], R.upsample2x(low[sel], None if bias is None else bias[sel]))
        h = rec.calls["head_loss_fused"][0]
        x, w, b, u = h["args"][:4]
        loss, v, dx, dw, db = R.head_loss(x, w, b, u)
        ck.le("loss", "mse", abs(float(h["out"][0]) - float(loss)) / abs(float(loss)), TOL_LOSS)
        ck.le("loss", "trainer's loss", abs(float(cfm["loss"]) - float(loss)) / abs(float(loss)), TOL_LOSS)
        ck.f32("head v", "v", cfm["v"], v)
        ck.bf("head g_head", "g_head", h["out"][1], dx)
        ck.f32("head grad", "outc.weight", cfm["grads"]["0.flow_decoder.outc.weight"], dw)
        ck.f32("head grad", "outc.bias", cfm["grads"]["0.flow_decoder.outc.bias"], db)
    ck.done()


def test_cfm_backward_layers(cfm):
    rec, net, grads = cfm["rec"], cfm["net"], cfm["grads"]
    ck = Checks("CFM bf16 backward, per layer")
    pname = {id(p): n for n, p in net.named_parameters()}
    with R.cpu_thread_share():
        assert len(rec.calls["bwd"]) == 2 * NLEV + 2 * (NLEV - 1)
        for b in rec.calls["bwd"]:
            cb = b["cb"]
            ck.true("accumulate off", b["name"], not b["accumulate"])
            dgam, dbet, wg = check_bn_backward(ck, rec, b)
            ck.f32("bwd dgamma", b["name"], grads["0." + pname[id(cb.bn.weight)]], dgam)
            ck.f32("bwd dbeta", b["name"], grads["0." + pname[id(cb.bn.bias)]], dbet)
            ck.f32("bwd wgrad", b["name"], grads["0." + pname[id(cb.conv.weight)]], wg)
            check_dgrad(ck, b, B)
        L = NLEV - 1
        for i, u in enumerate(rec.calls["upsample2x_bwd"]):
            dy, hin, win = u["args"]
            sel = _sel(B)
            ck.bf("up bwd", f"call {i}", u["out"][sel], R.upsample2x_bwd(dy[sel], hin, win))
        dbott = rec.calls["upsample2x_bwd"][L - 1]["out"]
        dtb = R.pixel_sum(dbott)
        ck.f32("pixel_sum", "dtb", rec.calls["pixel_sum"][0]["out"], dtb)
        _, tg = R.time_path(rec.calls["time_embedding"][0]["out"], net.flow_decoder, dtb)
        for n, g in tg.items():
            ck.f32("time grad", n, grads["0.flow_decoder." + n], g)
    ck.done()


def test_cfm_launch_families(cfm):
    """The set of 3x3 conv families the headline step launches (forward with statistics, data gradients): a change of
    launch plan shows up here and has to be re-pinned deliberately."""
    fams = cfm["rec"].families()
    if os.environ.get("S2S_TEST_REPORT"):
        for k, v in sorted(fams.items()):
            print(f"{k}: {sorted(v)}")
    plan_env = [k for k in ("S2S_CONV_STAGE", "S2S_CONV_PERS", "S2S_CONV_XCD") if k in os.environ]
    assert set(fams) == HEADLINE_FAMILIES or plan_env, (sorted(fams), plan_env)
    # every forward (with statistics) and every data gradient is one launch of a known family
    for r in cfm["rec"].calls["fwd"]:
        assert len(r["families"]) == 1, r["name"]
    for b in cfm["rec"].calls["bwd"]:
        assert len(b["families"]) == (1 if b["need_dx"] else 0), b["name"]


def test_cfm_instrumentation_changes_nothing(cfm):
    """The same step again from the same state, without the recorder: loss, velocity, every gradient and every running
    statistic bit-equal to the recorded step."""
    net, tr = cfm["net"], cfm["tr"]
    with torch.no_grad():
        for k, v in net.named_buffers():
            v.copy_(cfm["buffers0"][k])
    loss, v = tr.forward_backward(cfm["x0"], cfm["x1"], cfm["t"])
    torch.cuda.synchronize()
    assert torch.equal(loss, cfm["loss"]) and torch.equal(v, cfm["v"])
    g = _grads([net])
    bad = [k for k in g if not torch.equal(g[k], cfm["grads"][k])]
    assert not bad, bad
    bad = [k for k, b in net.named_buffers() if not torch.equal(b, cfm["buffers1"][k])]
    assert not bad, bad
    if os.environ.get("S2S_TEST_REPORT"):
        print(f"recorded step {cfm['step_s']:.1f} s")


# ---------------------------------------------------------------------------------------------------------------------
# b. MultiTaskTrainer, bf16: the shared encoder's gradients are the sum of its two passes
# ---------------------------------------------------------------------------------------------------------------------
def test_multitask_encoder_gradients_sum_two_passes():
    from stain2stain_amd import FlowMatchingDecoder, MultiTaskTrainer, SegmentationDecoder, SharedEncoder
    nb = 4
    torch.manual_seed(1984)
    enc = SharedEncoder(3, precision="bf16").to(DEV).train()
    fdec = FlowMatchingDecoder(1024, [512, 256, 128, 64], 3, 256, precision="bf16").to(DEV).train()
    sdec = SegmentationDecoder(1024, [512, 256, 128, 64], 1, precision="bf16").to(DEV).train()
    tr = MultiTaskTrainer(enc, fdec, sdec, time_emb_dim=256)
    x0, x1, t = _batch(nb, 7)
    g = torch.Generator().manual_seed(8)
    mask = (torch.rand(nb, 1, SIZE, SIZE, generator=g) > 0.5).float().to(DEV)
    with R.Recorder() as rec:
        tr.forward_backward(x0, x1, mask, t)
    torch.cuda.synchronize()
    grads = _grads([enc])
    pname = {id(p): n for n, p in enc.named_parameters()}
    ck = Checks("multitask bf16: shared encoder, two passes")
    xt = rec.calls["cfm_sample"][0]["out"][0]
    ck.true("route", "pass 1 reads xt", same(rec.fwd(enc_name(0, 0), 0)["x0"], xt))
    ck.true("route", "pass 2 reads the source", same(rec.fwd(enc_name(0, 0), 1)["x0"], x0))
    with R.cpu_thread_share():
        for l in range(NLEV):
            for j in (0, 1):
                name = enc_name(l, j)
                for k in (0, 1):
                    check_train_forward(ck, rec.fwd(name, k), nb)
                # backward: the source pass (second forward) first, then the xt pass accumulating onto it
                b2, b1 = rec.bwd(name, 0), rec.bwd(name, 1)
                ck.true("accumulate", name, (b2["accumulate"], b1["accumulate"]) == (False, True))
                ck.true("pass order", name, rec.fwd_of(b2) is rec.fwd(name, 1) and rec.fwd_of(b1) is rec.fwd(name, 0))
                dg2, db2, w2 = check_bn_backward(ck, rec, b2)
                dg1, db1, w1 = check_bn_backward(ck, rec, b1)
                check_dgrad(ck, b2, nb)
                check_dgrad(ck, b1, nb)
                cb = b1["cb"]
                ck.f32("sum dgamma", name, grads["0." + pname[id(cb.bn.weight)]], dg1 + dg2)
                ck.f32("sum dbeta", name, grads["0." + pname[id(cb.bn.bias)]], db1 + db2)
                ck.f32("sum wgrad", name, grads["0." + pname[id(cb.conv.weight)]], w1 + w2)
    ck.done()


# ---------------------------------------------------------------------------------------------------------------------
# c. eval-mode sampler, bf16: one Euler step
# ---------------------------------------------------------------------------------------------------------------------
def test_euler_step_eval_bf16():
    """euler_generate(net, x, 1) with non-trivial running statistics: every conv with the folded BatchNorm + ReLU
    epilogue (``cb.eval_affine()``), the bf16 stem-as-conv, the head and the state update."""
    from stain2stain_amd import FlowUNet, euler_generate
    nb = 2
    torch.manual_seed(1984)
    net = FlowUNet(precision="bf16").to(DEV)
    g = torch.Generator(device=DEV).manual_seed(5)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                C = m.num_features
                m.running_mean.copy_((torch.rand(C, device=DEV, generator=g) - 0.5) * 0.2)
                m.running_var.copy_(torch.rand(C, device=DEV, generator=g) * 0.5 + 0.1)
                m.weight.copy_(torch.rand(C, device=DEV, generator=g) + 0.5)
                m.bias.copy_(torch.rand(C, device=DEV, generator=g) - 0.3)
    x, _, _ = _batch(nb, 11)
    with R.Recorder() as rec:
        out = euler_generate(net, x, 1)
    torch.cuda.synchronize()
    ck = Checks("eval sampler bf16, one Euler step")
    sel = _sel(nb)
    L = NLEV - 1
    fw = rec.fwd
    with R.cpu_thread_share():
        assert len(rec.calls["fwd"]) == 2 * NLEV + 2 * (NLEV - 1)
        for r in rec.calls["fwd"]:
            cb, name = r["cb"], r["name"]
            assert not r["training"]
            sc, sh = R.eval_affine(cb.bn)
            ck.f32("eval affine", name + " scale", r["ss"][0], sc, 1e-5)
            ck.f32("eval affine", name + " shift", r["ss"][1], sh, 1e-5)
            xin = R.stem_image(r["x0"][sel]) if r["stem"] else \
                R.cat_input(r["x0"][sel], None if r["x1"] is None else r["x1"][sel])
            z = R.conv3x3(xin, R.bf(cb.conv.weight.detach().cpu()), cb.conv.bias.detach()).double()
            ref = (z * r["ss"][0].cpu().double()[None, :, None, None] + r["ss"][1].cpu().double()[None, :, None, None])
            ck.bf("eval act", name, R.to_nchw(r["act"][sel]), ref.clamp_min(0))
            if r["pooled"] is not None:
                a = r["act"]
                n, H, W, C = a.shape
                ck.true("pooled bit-equal", name, torch.equal(r["pooled"], a.view(n, H // 2, 2, W // 2, 2, C).amax((2, 4))))
        ck.true("route", "stem input is the state", same(fw(enc_name(0, 0))["x0"], x))
        for l in range(NLEV):
            ck.true("route", f"enc {l} conv2 <- conv1", same(fw(enc_name(l, 1))["x0"], fw(enc_name(l, 0))["act"]))
            if l < L:
                ck.true("route", f"enc {l + 1} <- pool", same(fw(enc_name(l + 1, 0))["x0"], fw(enc_name(l, 1))["pooled"]))
        temb = rec.calls["time_embedding"][0]["out"]
        ck.f32("time embedding", "t = 0", temb, R.time_embedding(torch.zeros(nb), net.time_embedding.dim))
        tb, _ = R.time_path(temb, net.flow_decoder)
        ck.f32("time bias", "time_proj out", rec.calls["linear_fwd"][2]["out"], tb)
        for i, u in enumerate(rec.calls["upsample2x_fwd"]):
            low, _, bias = u["args"]
            ck.true("route", f"ups {i} low", same(low, fw(enc_name(L, 1))["act"] if i == 0 else fw(dec_name(i - 1, 1))["act"]))
            ck.true("route", f"dec {i} skip / up", same(fw(dec_name(i, 0))["x0"], fw(enc_name(L - 1 - i, 1))["act"])
                    and same(fw(dec_name(i, 0))["x1"], u["after"][1]))
            ck.bf("up", f"ups {i}", u["after"][1][sel], R.upsample2x(low[sel], None if bias is None else bias[sel]))
        h = rec.calls["head_fwd"][0]
        ck.true("route", "head input", same(h["args"][0], fw(dec_name(L - 1, 1))["act"]))
        ck.f32("head v", "v", h["out"], R.head_fwd(*h["args"]))
        a = rec.calls["axpy_"][0]
        xs, v, dt = a["args"]
        ck.true("route", "update reads v", same(v, h["out"]) and same(xs, x))
        ck.f32("euler update", "x + dt v", a["after"][0], xs.cpu().double() + dt * v.cpu().double(), 1e-6)
        ck.true("route", "result is the updated state", same(out, a["after"][0]))
    ck.done()
