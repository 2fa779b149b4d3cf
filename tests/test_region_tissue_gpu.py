"""Tissue-aware region translation (stain2stain_amd.region, csrc/region.hip) on the GPU: the tissue counts are bit-exact
against numpy; with every tile kept the result is bit-equal to the call without the keywords; with none kept the
sampler never runs and the region comes back byte for byte; mixed masks copy the uncovered pixels and blend the rest as
a float64 restatement in plan order says."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---- numpy / float64 restatements (as in test_region_gpu.py) ---------------------------------------------------------
def _norm(u8):
    return (u8.astype(np.float32) / np.float32(255.0) - np.float32(0.5)) / np.float32(0.5)


def _gather_ref(img, origins, T):
    H, W, _ = img.shape
    pad = np.pad(img, ((0, max(0, T - H)), (0, max(0, T - W)), (0, 0)), mode="reflect")
    return np.stack([_norm(pad[y:y + T, x:x + T]).transpose(2, 0, 1) for y, x in origins])


def _axis_w(T, overlap):
    i = np.arange(T, dtype=np.float64)
    if overlap == 0:
        return np.ones(T)
    return np.minimum(1.0, np.minimum((i + 0.5) / overlap, (T - i - 0.5) / overlap))


def _check_u8(got, ref64, where):
    pre = np.clip((ref64 * 0.5 + 0.5) * 255.0, 0, 255)
    want = np.trunc(pre).astype(np.int64)
    diff = np.abs(got.astype(np.int64) - want)[where]
    near = (np.abs(pre - np.round(pre)) <= 1e-3)[where]
    assert diff.max() <= 1 and not np.any((diff > 0) & ~near)


def _img(H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)


def _counts_ref(img, plan, T, white, black):
    tis = (img.min(2).astype(np.int64) < white) & (img.max(2).astype(np.int64) >= black)
    counts = [int(tis[y:y + T, x:x + T].sum()) for y, x in plan]
    areas = [int(tis[y:y + T, x:x + T].size) for y, x in plan]
    return counts, areas


def _edge_img(H, W, white, black, seed):
    """Random bytes, a third of the pixels made of the values either side of both thresholds."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    edge = np.array([min(255, max(0, v)) for v in (white - 1, white, black - 1, black, 255)], dtype=np.uint8)
    planted = edge[rng.integers(0, len(edge), (H, W, 3))]
    return torch.from_numpy(np.where(rng.random((H, W, 1)) < 0.34, planted, img))


class _Pointwise:
    """A cheap pointwise sampler that records its inputs and outputs; ``cm`` probability channels as a tuple."""

    def __init__(self, cm=0):
        self.cm, self.inputs, self.outputs, self.probs = cm, [], [], []
        if cm:
            self.mask_channels = cm

    def __call__(self, x):
        self.inputs.append(x.clone())
        out = x * 0.5 + 0.1
        self.outputs.append(out.clone())
        if not self.cm:
            return out
        p = (x[:, :self.cm] * 0.25 + 0.5).contiguous()
        self.probs.append(p.clone())
        return out, p


# ---- counts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("white,black", [(220, 0), (200, 30), (256, 255), (1, 0)])
@pytest.mark.parametrize("H,W,T,overlap", [(37, 45, 64, 0), (133, 71, 32, 5), (1, 100, 16, 4)])
def test_counts_bit_exact(H, W, T, overlap, white, black):
    from stain2stain_amd import ops, tissue_counts
    from stain2stain_amd.region import plan_tiles
    img = _edge_img(H, W, white, black, H + white)
    plan = plan_tiles(H, W, T, overlap)
    want, want_areas = _counts_ref(img.numpy(), plan.tolist(), T, white, black)
    counts, areas = tissue_counts(img.to(DEV), T, overlap, white=white, black=black)
    assert counts.is_cuda and counts.dtype == torch.int32 and not areas.is_cuda
    assert counts.tolist() == want and areas.tolist() == want_areas
    assert 0 < sum(want) < sum(want_areas) or white in (1, 256)
    # a poisoned counts buffer: every entry is written
    buf = torch.full((plan.shape[0],), 0x7F7F7F7F, dtype=torch.int32, device=DEV)
    ops.region_tissue_count(img.to(DEV), 0, H, W, plan.to(DEV), T, white, black, buf)
    assert buf.tolist() == want
    # the host image, streamed one tile row per band
    hc, ha = tissue_counts(img, T, overlap, white=white, black=black)
    assert hc.is_cuda and hc.tolist() == want and ha.tolist() == want_areas


@pytest.mark.parametrize("y0,x0", [(13, 7), (4, 8)])          # misaligned and 4-byte aligned row starts
def test_counts_crop_view(y0, x0):
    from stain2stain_amd import tissue_counts
    from stain2stain_amd.region import plan_tiles
    big = _edge_img(260, 320, 220, 10, 2)
    H, W, T, ov = 181, 229, 32, 6
    view = big[y0:y0 + H, x0:x0 + W]
    plan = plan_tiles(H, W, T, ov)
    want, want_areas = _counts_ref(view.numpy(), plan.tolist(), T, 220, 10)
    for im in (big.to(DEV)[y0:y0 + H, x0:x0 + W], view):
        counts, areas = tissue_counts(im, T, ov, white=220, black=10)
        assert counts.tolist() == want and areas.tolist() == want_areas


def test_count_outside_the_band_is_flagged():
    from stain2stain_amd import ops
    from stain2stain_amd.region import plan_tiles
    img = _img(100, 40, 3).to(DEV)
    plan = plan_tiles(100, 40, 32, 0)
    buf = torch.zeros((plan.shape[0],), dtype=torch.int32, device=DEV)
    ops.region_tissue_count(img[32:64], 32, 100, 40, plan.to(DEV), 32, 256, 0, buf)
    inside = [(32 <= y and y + 32 <= 64) for y, _ in plan.tolist()]
    assert buf.tolist() == [32 * min(32, 40 - x) if ok else -1 for ok, (_, x) in zip(inside, plan.tolist())]


# ---- every tile kept: the call without the keywords, bit for bit -----------------------------------------------------
@pytest.mark.parametrize("H,W,T,overlap,batch", [(150, 130, 32, 8, 4), (37, 45, 64, 16, 3)])
@pytest.mark.parametrize("cm,on_gpu", [(0, True), (2, True), (2, False)], ids=["0", "2", "2-host"])
def test_all_kept_equals_the_plain_call(H, W, T, overlap, batch, cm, on_gpu):
    from stain2stain_amd import translate_region
    from stain2stain_amd.region import plan_tiles
    img = _img(H, W, 3).to(DEV) if on_gpu else _img(H, W, 3)      # a host image: both staging directions
    kw = dict(tile=T, overlap=overlap, batch=batch, return_float=True)
    s0 = _Pointwise(cm)
    plain = translate_region(img, s0, **kw)
    assert translate_region.last_stats["kept"] == plan_tiles(H, W, T, overlap).shape[0]
    assert translate_region.last_stats["skipped"] == 0
    assert translate_region.last_stats["sampler_calls"] == len(s0.inputs)
    N = plan_tiles(H, W, T, overlap).shape[0]
    for extra in (dict(keep=torch.ones(N, dtype=torch.bool)), dict(min_tissue=0.0)):
        s1 = _Pointwise(cm)
        got = translate_region(img, s1, **kw, **extra)
        assert len(got) == len(plain) == (3 if cm else 2)
        for a, b in zip(got, plain):
            assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)
        assert len(s1.inputs) == len(s0.inputs)
        assert all(torch.equal(a, b) for a, b in zip(s1.inputs, s0.inputs))
        st = translate_region.last_stats
        assert (st["kept"], st["skipped"], st["sampler_calls"]) == (N, 0, len(s0.inputs))


# ---- nothing kept: the region itself ---------------------------------------------------------------------------------
@pytest.mark.parametrize("on_gpu", [True, False])
def test_nothing_kept_copies_the_region(on_gpu):
    from stain2stain_amd import translate_region
    from stain2stain_amd.region import plan_tiles
    H, W, T, ov = 150, 130, 32, 8
    img = _img(H, W, 4)
    assert len(np.unique(img.numpy())) == 256               # the 63 byte values a float round trip loses are there
    N = plan_tiles(H, W, T, ov).shape[0]
    calls = []

    def sampler(x):
        calls.append(1)
        return x.clone()

    u8, probs, f = translate_region(img.to(DEV) if on_gpu else img, sampler, tile=T, overlap=ov, batch=4,
                                    keep=torch.zeros(N, dtype=torch.bool), mask_channels=2, return_float=True)
    assert not calls
    assert u8.is_cuda == on_gpu and torch.equal(u8.cpu(), img)
    assert probs.shape == (H, W, 2) and probs.dtype == torch.float32 and not probs.any()
    assert np.array_equal(f.cpu().numpy(), _norm(img.numpy()))
    st = translate_region.last_stats
    assert (st["kept"], st["skipped"], st["sampler_calls"], st["channels"]) == (0, N, 0, 5)
    # min_tissue on a region without tissue
    white = torch.full((70, 50, 3), 240, dtype=torch.uint8, device=DEV)
    out = translate_region(white, sampler, tile=T, overlap=ov, batch=4, min_tissue=0.01)
    assert not calls and torch.equal(out, white)


# ---- mixed masks -----------------------------------------------------------------------------------------------------
def _keep_pattern(name, plan, T):
    ys = sorted({y for y, _ in plan})
    xs = sorted({x for _, x in plan})
    if name == "checkerboard":
        return [(ys.index(y) + xs.index(x)) % 2 == 0 for y, x in plan]
    if name == "corner":
        return [(y, x) == (ys[-1], xs[-1]) for y, x in plan]
    if name == "row":                                        # a fully skipped tile row in the middle
        return [y != ys[len(ys) // 2] for y, x in plan]
    raise KeyError(name)


def _mixed_ref(img, plan, kept, outs, H, W, T, overlap, C):
    """float64 restatement in plan order: kept tiles bring their sampler output, skipped tiles the normalised source
    and probability 0.  Returns (blend [H, W, C], kept weight [H, W])."""
    w2 = np.outer(_axis_w(T, overlap), _axis_w(T, overlap))
    src = np.zeros((H, W, C))
    src[..., :3] = _norm(img).astype(np.float64)
    acc, ws, wk = np.zeros((H, W, C)), np.zeros((H, W)), np.zeros((H, W))
    it = iter(outs)
    for (y, x), k in zip(plan, kept):
        h, w = min(T, H - y), min(T, W - x)
        if k:
            acc[y:y + h, x:x + w] += w2[:h, :w, None] * next(it).astype(np.float64).transpose(1, 2, 0)[:h, :w]
            wk[y:y + h, x:x + w] += w2[:h, :w]
        else:
            acc[y:y + h, x:x + w] += w2[:h, :w, None] * src[y:y + h, x:x + w]
        ws[y:y + h, x:x + w] += w2[:h, :w]
    return acc / ws[..., None], wk


@pytest.mark.parametrize("pattern", ["checkerboard", "corner", "row"])
@pytest.mark.parametrize("H,W,T,overlap,batch,cm,on_gpu", [(150, 130, 32, 8, 4, 0, True), (150, 130, 32, 8, 4, 2, False),
                                                          (100, 90, 32, 0, 3, 2, True)])
def test_mixed_masks(pattern, H, W, T, overlap, batch, cm, on_gpu):
    from stain2stain_amd import plan_region_batches, translate_region
    from stain2stain_amd.region import band_rows_for, plan_tiles
    img = _img(H, W, 5)
    plan_t = plan_tiles(H, W, T, overlap)
    plan = [tuple(p) for p in plan_t.tolist()]
    kept = _keep_pattern(pattern, plan, T)
    keep = torch.tensor(kept, dtype=torch.bool)
    s = _Pointwise(cm)
    res = translate_region(img.to(DEV) if on_gpu else img, s, tile=T, overlap=overlap, batch=batch, keep=keep,
                           return_float=True)
    u8, f = res[0].cpu().numpy(), res[-1].cpu().numpy()
    # the sampler's calls: exactly `batch` tiles, the gather of each range's kept origins in plan order, padded
    ranges = plan_region_batches(plan_t, keep, batch, band_rows_for(H, W, T, overlap, batch), T)
    with_kept = [[p for p in range(p0, p1) if kept[p]] for p0, p1 in ranges]
    with_kept = [ks for ks in with_kept if ks]
    st = translate_region.last_stats
    assert st["sampler_calls"] == len(with_kept) == len(s.inputs)
    assert (st["kept"], st["skipped"]) == (sum(kept), len(kept) - sum(kept))
    outs = []
    for x, o, ks in zip(s.inputs, s.outputs, with_kept):
        assert x.shape == (batch, 3, T, T)
        want = _gather_ref(img.numpy(), [plan[p] for p in ks + [ks[-1]] * (batch - len(ks))], T)
        assert np.array_equal(x.cpu().numpy(), want)
        outs += list(o[:len(ks)].cpu().numpy())
    if cm:
        pr = [q for p, ks in zip(s.probs, with_kept) for q in p[:len(ks)].cpu().numpy()]
        outs = [np.concatenate([a, b]) for a, b in zip(outs, pr)]
    ref, wk = _mixed_ref(img.numpy(), plan, kept, outs, H, W, T, overlap, 3 + cm)
    bare = wk == 0
    assert bare.any() and (~bare).any()
    # pixels no kept tile covers: the source bytes, the normalised source, probability 0
    assert np.array_equal(u8[bare], img.numpy()[bare])
    assert np.array_equal(f[bare], _norm(img.numpy())[bare])
    assert np.abs(f - ref[..., :3]).max() <= 1e-6
    _check_u8(u8, ref[..., :3], ~bare)
    if cm:
        probs = res[1].cpu().numpy()
        assert probs.shape == (H, W, cm) and not probs[bare].any()
        assert np.abs(probs - ref[..., 3:]).max() <= 1e-6


# ---- min_tissue end to end -------------------------------------------------------------------------------------------
def test_min_tissue_end_to_end():
    from stain2stain_amd import translate_region
    from stain2stain_amd.region import plan_tiles
    H, W, T, ov, batch, white, frac = 150, 130, 32, 8, 4, 215, 0.1
    g = torch.Generator().manual_seed(6)
    img = torch.randint(white, 256, (H, W, 3), generator=g, dtype=torch.uint8)          # glass
    img[40:95, 30:80] = torch.randint(0, 256, (55, 50, 3), generator=g, dtype=torch.uint8)   # a textured blob
    plan = plan_tiles(H, W, T, ov).tolist()
    counts, areas = _counts_ref(img.numpy(), plan, T, white, 0)
    kept = [c >= frac * a for c, a in zip(counts, areas)]
    assert 0 < sum(kept) < len(kept)
    run = lambda im: translate_region(im, _Pointwise(), tile=T, overlap=ov, batch=batch, min_tissue=frac, white=white,
                                      return_float=True)
    big = torch.zeros((H + 9, W + 11, 3), dtype=torch.uint8, device=DEV)
    big[5:5 + H, 7:7 + W] = img.to(DEV)
    du8, df = run(big[5:5 + H, 7:7 + W])                     # a pitched view
    st = translate_region.last_stats
    assert (st["kept"], st["skipped"]) == (sum(kept), len(kept) - sum(kept))
    assert 0 < st["sampler_calls"] < -(-len(kept) // batch)
    hu8, hf = run(img)
    assert not hu8.is_cuda and torch.equal(hu8, du8.cpu()) and torch.equal(hf, df.cpu())
    assert translate_region.last_stats == st
    au8, af = run(big[5:5 + H, 7:7 + W])
    assert torch.equal(au8, du8) and torch.equal(af, df)
    cover = np.zeros((H, W), bool)
    for (y, x), k in zip(plan, kept):
        if k:
            cover[y:y + T, x:x + T] = True
    assert np.array_equal(du8.cpu().numpy()[~cover], img.numpy()[~cover])


# ---- the ring --------------------------------------------------------------------------------------------------------
def test_ring_is_independent_of_height_with_skipped_rows():
    from stain2stain_amd import translate_region
    from stain2stain_amd.region import plan_tiles
    W, T, ov, batch = 150, 64, 16, 5
    full = _img(1100, W, 7)
    res, stats = [], []
    for H in (1100, 700):
        plan = plan_tiles(H, W, T, ov)
        keep = ~((plan[:, 0] >= 190) & (plan[:, 0] < 400))   # the middle tile rows are skipped
        assert 0 < int(keep.sum()) < plan.shape[0]
        res.append(translate_region(full[:H].to(DEV), _Pointwise(), tile=T, overlap=ov, batch=batch, keep=keep,
                                    return_float=True))
        stats.append(translate_region.last_stats)
    assert stats[0]["band_rows"] == stats[1]["band_rows"] < 700
    assert stats[0]["accumulator_bytes"] == stats[1]["accumulator_bytes"]
    assert stats[0]["accumulator_bytes"] <= stats[0]["band_rows"] * W * (3 + 1 + 1) * 4
    shared = 560                                             # both plans agree on every tile touching these rows
    assert torch.equal(res[0][0][:shared], res[1][0][:shared]) and torch.equal(res[0][1][:shared], res[1][1][:shared])
    assert torch.equal(res[0][0][260:380], full[260:380].to(DEV))


# ---- the real network ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_kept_tiles_match_euler_generate(precision):
    from stain2stain_amd import FlowUNet, euler_generate, translate_region
    from stain2stain_amd.region import plan_tiles
    torch.manual_seed(1984)
    net = FlowUNet(3, [16, 32], 3, 32, precision=precision).to(DEV)
    H, W, T, batch, steps = 96, 64, 32, 2, 2
    img = _img(H, W, 8)
    plan = plan_tiles(H, W, T, 0).tolist()
    kept = [True, False, False, False, True, True]           # ranges (0, 4) with one kept tile, padded, and (4, 6)
    u8, f = translate_region(img.to(DEV), lambda x: euler_generate(net, x, steps, graph=True), tile=T, overlap=0,
                             batch=batch, keep=torch.tensor(kept), return_float=True)
    assert translate_region.last_stats["sampler_calls"] == 2
    tiles = torch.from_numpy(_gather_ref(img.numpy(), plan, T)).to(DEV)
    want = _norm(img.numpy())
    a = euler_generate(net, tiles[[0, 0]], steps, graph=True)[0]
    b = euler_generate(net, tiles[[4, 5]], steps, graph=True)
    for v, (y, x) in zip((a, b[0], b[1]), (plan[0], plan[4], plan[5])):
        want[y:y + T, x:x + T] = v.permute(1, 2, 0).cpu().numpy()
    assert np.array_equal(f.cpu().numpy(), want)
    skipped = np.ones((H, W), bool)
    for p in (0, 4, 5):
        skipped[plan[p][0]:plan[p][0] + T, plan[p][1]:plan[p][1] + T] = False
    assert np.array_equal(u8.cpu().numpy()[skipped], img.numpy()[skipped])


@pytest.mark.parametrize("num_classes", [None, 3])
def test_multitask_sampler_carries_mask_channels(num_classes):
    from stain2stain_amd import (FlowMatchingDecoder, MultiTaskFlowMatchingModule, SegmentationDecoder, SharedEncoder,
                                 SolverConfig, multitask_sampler, translate_region)
    torch.manual_seed(1984)
    Cm = 1 if num_classes is None else num_classes
    enc = SharedEncoder(3, [16, 32], precision="fp32")
    fdec = FlowMatchingDecoder(32, [16], 3, 32, precision="fp32")
    sdec = SegmentationDecoder(32, [16], Cm, precision="fp32")
    mod = MultiTaskFlowMatchingModule(enc, fdec, sdec, time_emb_dim=32, num_classes=num_classes,
                                      solver=SolverConfig("euler")).to(DEV)
    sampler = multitask_sampler(mod, 2)
    assert sampler.mask_channels == Cm
    img = _img(64, 32, 9).to(DEV)
    u8, probs = translate_region(img, sampler, tile=32, overlap=0, batch=2, keep=torch.tensor([False, True]))
    assert probs.shape == (64, 32, Cm) and not probs[:32].any() and probs[32:].any()
    assert torch.equal(u8[:32], img[:32])


# ---- rejections ------------------------------------------------------------------------------------------------------
def test_rejections():
    from stain2stain_amd import tissue_counts, translate_region
    from stain2stain_amd.region import plan_tiles
    img = _img(70, 40, 11).to(DEV)
    N = plan_tiles(70, 40, 32, 8).shape[0]
    ident = lambda x: x.clone()
    kw = dict(tile=32, overlap=8, batch=2)
    ok = torch.ones(N, dtype=torch.bool)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            translate_region(img, ident, min_tissue=bad, **kw)
    with pytest.raises(ValueError):
        translate_region(img, ident, min_tissue=0.5, keep=ok, **kw)
    with pytest.raises(ValueError):
        translate_region(img, ident, keep=torch.ones(N + 1, dtype=torch.bool), **kw)
    with pytest.raises(ValueError):
        translate_region(img, ident, keep=torch.ones(N, dtype=torch.uint8), **kw)
    with pytest.raises(TypeError):
        translate_region(img, ident, keep=[True] * N, **kw)
    for w, b in ((0, 0), (257, 0), (220, -1), (220, 256)):
        with pytest.raises(ValueError):
            translate_region(img, ident, min_tissue=0.5, white=w, black=b, **kw)
        with pytest.raises(ValueError):
            tissue_counts(img, 32, 8, white=w, black=b)
    with pytest.raises(ValueError):
        tissue_counts(img.float(), 32, 8)
    with pytest.raises(ValueError):
        translate_region(img, ident, keep=ok, mask_channels=6, **kw)
    # the declared layout against the sampler's output
    with pytest.raises(ValueError, match="changed its output channels"):
        translate_region(img, ident, keep=ok, mask_channels=2, **kw)
    with pytest.raises(ValueError, match="changed its output channels"):
        translate_region(img, lambda x: (x.clone(), x[:, :2].contiguous()), keep=ok, **kw)
    with pytest.raises(ValueError, match="changed its output channels"):
        translate_region(img, lambda x: (x.clone(), x[:, :2].contiguous()), keep=ok, mask_channels=1, **kw)
