"""The stain-quantification kernels (csrc/stain_quant.hip) against the float32 restatement of tests/stain_quant_ref.py, on
poisoned memory (every ``torch.empty`` and every ``ops._workspace`` slab starts as NaN / 0xFF, as in
tests/test_image_metrics_gpu.py).

Tolerances: tissue and positive counts and the separated concentrations are exact (the restatement
rounds operation by operation as the kernels do); od_sum 1e-10 relative (the same fp32 terms, added in fp64 in another
order: n terms of one sign give at most n * 2^-53 relative, 7e-12 at 256 x 256); burden, mean_od, Dice, IoU and the
burden error are one fp32 rounding of a double quotient: 2^-23 relative (2^-24 for the rounding, the rest for the
restatement's own double arithmetic), absolute 2^-24 for |burden_pred - burden_target|, whose operands are below 1."""
import numpy as np
import pytest
import torch

import stain_quant_ref as R
from stain2stain_amd import (region_stain_agreement, region_stain_map, stain_agreement, stain_quantify, stain_separate)
from stain2stain_amd.stain_quant import unmix_matrix

pytestmark = pytest.mark.gpu
DEV = "cuda"
THR = (0.2, 0.15, 0.1)
F32 = 2.0 ** -23
PAIR_KEYS = ("burden_pred", "burden_target", "burden_abs_err", "dice", "iou")


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    from stain2stain_amd import ops
    import torch.utils.deterministic as tud
    prev_det, prev_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    prev_fill = tud.fill_uninitialized_memory
    orig = ops._workspace

    def poisoned(device, numel, tag):
        buf = orig(device, numel, tag)
        buf.view(torch.uint8).fill_(255)
        return buf

    torch.use_deterministic_algorithms(True, warn_only=True)
    tud.fill_uninitialized_memory = True
    try:
        for buf in ops._WORKSPACE.values():
            buf.view(torch.uint8).fill_(255)
        monkeypatch.setattr(ops, "_workspace", poisoned)
        yield
    finally:
        torch.use_deterministic_algorithms(prev_det, warn_only=prev_warn)
        tud.fill_uninitialized_memory = prev_fill


def _stained(B, H, W, seed, plaque=0.08):
    """uint8 [B, H, W, 3]: haematoxylin background with DAB blobs, glass patches, black specks and noise."""
    rng = np.random.default_rng(seed)
    conc = np.zeros((B, H, W, 3))
    conc[..., 0] = rng.uniform(0.05, 0.5, size=(B, H, W))
    conc[..., 1] = np.where(rng.random((B, H, W)) < plaque, rng.uniform(0.1, 1.2, size=(B, H, W)), 0.02)
    img = R.synthesise(conc, "hdab").astype(np.int32) + rng.integers(-3, 4, size=(B, H, W, 3))
    img = np.clip(img, 0, 255).astype(np.uint8)
    glass = rng.random((B, H, W)) < 0.2
    img[glass] = rng.integers(225, 256, size=(int(glass.sum()), 3), dtype=np.uint8)
    img[rng.random((B, H, W)) < 0.01] = 0
    return img


def _network(u8, seed):
    """uint8 [B, H, W, 3] -> fp32 [B, 3, H, W] in the network's range with a sub-level jitter (the quantiser has work)."""
    rng = np.random.default_rng(seed)
    lv = u8.astype(np.float64).transpose(0, 3, 1, 2) + rng.random(u8.transpose(0, 3, 1, 2).shape) * 0.98
    return np.ascontiguousarray((lv / 127.5 - 1.0).astype(np.float32))


def _crop_view(u8):
    """The batch as a crop view of a larger GPU array: odd row pitch, unaligned base."""
    B, H, W, _ = u8.shape
    big = torch.full((B, H + 5, W + 6, 3), 77, dtype=torch.uint8, device=DEV)
    view = big[:, 2:2 + H, 3:3 + W]
    view.copy_(torch.from_numpy(u8))
    assert (3 * (W + 6)) % 4 != 0 or view.data_ptr() % 4 != 0 or W % 4 != 0
    return view


def _close(got, want, tol, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    err = np.where(want == 0, np.abs(got), err)
    print(f"{what}: max rel err {err.max():.3e} (tolerance {tol:.1e})")
    assert got.shape == want.shape and (err <= tol).all(), what


def _check_single(got, ref, what):
    got = {k: v.cpu().numpy() for k, v in got.items()}
    assert got["tissue"].dtype == np.int64 and got["positive"].dtype == np.int64
    assert got["od_sum"].dtype == np.float64 and got["burden"].dtype == np.float32 and got["mean_od"].dtype == np.float32
    assert np.array_equal(got["tissue"], ref["tissue"]), what
    assert np.array_equal(got["positive"], ref["positive"]), what
    _close(got["od_sum"], ref["od_sum"], 1e-10, what + " od_sum")
    _close(got["burden"], ref["burden"], F32, what + " burden")
    _close(got["mean_od"], ref["mean_od"], F32, what + " mean_od")


def _check_pair(got, ref, what):
    got = {k: v.cpu().numpy() for k, v in got.items()}
    assert sorted(got) == sorted(PAIR_KEYS)
    for k in PAIR_KEYS:
        assert got[k].dtype == np.float32
        if k == "burden_abs_err":
            err = np.abs(got[k].astype(np.float64) - ref[k]).max()
            print(f"{what} {k}: max abs err {err:.3e}")
            assert err <= 2.0 ** -24, what
        else:
            _close(got[k], ref[k], F32, f"{what} {k}")


SHAPES = [(1, 1, 1, False), (3, 37, 53, True), (2, 64, 64, False), (1, 256, 256, False)]


@pytest.mark.parametrize("B,H,W,crop", SHAPES)
@pytest.mark.parametrize("stains", ["hdab", "hed"])
def test_parity_uint8(B, H, W, crop, stains):
    m32 = unmix_matrix(stains).numpy()
    a, b = _stained(B, H, W, 100 + H), _stained(B, H, W, 200 + H, plaque=0.12)
    b[:, : H // 2] = a[:, : H // 2]                                        # the masks overlap
    ga, gb = (_crop_view(a), _crop_view(b)) if crop else (torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV))
    _check_single(stain_quantify(ga, stains=stains, thresholds=THR), R.quantify32(a, m32, THR), f"u8 {B}x{H}x{W}")
    _check_single(stain_quantify(ga, stains=stains, thresholds=THR, white=256, black=40),
                  R.quantify32(a, m32, THR, 256, 40), f"u8 {B}x{H}x{W} white 256 black 40")
    for stain in (0, 1):
        _check_pair(stain_agreement(ga, gb, stain=stain, stains=stains, thresholds=THR),
                    R.agreement32(a, b, m32, THR, stain), f"u8 pair {B}x{H}x{W} stain {stain}")
    sep = stain_separate(ga, stains=stains).cpu().numpy()
    assert np.array_equal(sep, R.concentrations32(a, m32).transpose(0, 3, 1, 2))


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (3, 37, 53), (2, 64, 64), (1, 256, 256)])
def test_parity_fp32(B, H, W):
    m32 = unmix_matrix("hdab").numpy()
    a, b = _stained(B, H, W, 300 + H), _stained(B, H, W, 400 + H, plaque=0.12)
    xa, xb = _network(a, 1), _network(b, 2)
    xa.reshape(-1)[:: 7] += 3.0                                            # out of range: the clamp has work
    xb.reshape(-1)[:: 11] -= 3.0
    qa, qb = R.nchw_to_u8(xa), R.nchw_to_u8(xb)
    ga, gb = torch.from_numpy(xa).to(DEV), torch.from_numpy(xb).to(DEV)
    _check_single(stain_quantify(ga, thresholds=THR), R.quantify32(qa, m32, THR), f"f32 {B}x{H}x{W}")
    _check_pair(stain_agreement(ga, gb, thresholds=THR), R.agreement32(qa, qb, m32, THR), f"f32 pair {B}x{H}x{W}")
    assert np.array_equal(stain_separate(ga).cpu().numpy(), R.concentrations32(qa, m32).transpose(0, 3, 1, 2))
    # a channels-last tensor is the same image
    again = stain_quantify(ga.contiguous(memory_format=torch.channels_last), thresholds=THR)
    assert torch.equal(again["positive"], stain_quantify(ga, thresholds=THR)["positive"])


def test_special_images():
    white = torch.full((2, 33, 47, 3), 255, dtype=torch.uint8, device=DEV)
    q = stain_quantify(white)
    assert (q["tissue"] == 0).all() and (q["positive"] == 0).all() and (q["burden"] == 0).all()
    assert (q["od_sum"] == 0).all() and (q["mean_od"] == 0).all()
    a = stain_agreement(white, white.clone())
    assert (a["dice"] == 1).all() and (a["iou"] == 1).all() and (a["burden_abs_err"] == 0).all()
    zero = torch.zeros((1, 33, 47, 3), dtype=torch.uint8, device=DEV)       # u = 0 takes the entry of u = 1
    m32 = unmix_matrix("hdab").numpy()
    _check_single(stain_quantify(zero), R.quantify32(zero.cpu().numpy(), m32, (0.2, 0.2, 0.2)), "zero bytes")
    assert int(stain_quantify(zero)["tissue"][0]) == 33 * 47
    assert int(stain_quantify(zero, black=1)["tissue"][0]) == 0
    # tissue, no positives: a faint haematoxylin tile against itself and against another faint tile
    faint = torch.from_numpy(np.broadcast_to(R.synthesise([0.1, 0.0, 0.0], "hdab"), (1, 20, 24, 3)).copy()).to(DEV)
    q = stain_quantify(faint)
    assert int(q["tissue"][0]) == 480 and int(q["positive"][0, 1]) == 0 and float(q["burden"][0, 1]) == 0
    a = stain_agreement(faint, faint.clone())
    assert float(a["dice"][0]) == 1 and float(a["iou"][0]) == 1
    # identical non-empty masks
    img = torch.from_numpy(_stained(2, 40, 44, 9)).to(DEV)
    a = stain_agreement(img, img.clone(), thresholds=THR)
    assert (a["burden_pred"] > 0).all() and (a["dice"] == 1).all() and (a["iou"] == 1).all()
    assert (a["burden_abs_err"] == 0).all()


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_a_sample_does_not_see_its_batch_mates_and_runs_repeat(kind):
    a, b = _stained(4, 64, 80, 31), _stained(4, 64, 80, 32)
    if kind == "f32":
        a, b = _network(a, 3), _network(b, 4)
    ga, gb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    q1, q2 = stain_quantify(ga, thresholds=THR), stain_quantify(ga, thresholds=THR)
    p1, p2 = stain_agreement(ga, gb, thresholds=THR), stain_agreement(ga, gb, thresholds=THR)
    assert all(torch.equal(q1[k], q2[k]) for k in q1) and all(torch.equal(p1[k], p2[k]) for k in p1)
    for n in (0, 3):
        qs = stain_quantify(ga[n:n + 1], thresholds=THR)
        ps = stain_agreement(ga[n:n + 1], gb[n:n + 1], thresholds=THR)
        assert all(torch.equal(qs[k][0], q1[k][n]) for k in q1), n
        assert all(torch.equal(ps[k][0], p1[k][n]) for k in p1), n


def test_region_stain_map():
    H, W, cell = 301, 203, 64
    region = _stained(1, H, W, 41)[0]
    m32 = unmix_matrix("hdab").numpy()
    want_t, want_p = R.cell_counts32(region, m32, THR, cell, stain=1)
    host = torch.from_numpy(region)
    big = torch.zeros((H + 2, W + 3, 3), dtype=torch.uint8, device=DEV)
    gpu = big[1:1 + H, 2:2 + W]                                            # a crop view: odd pitch, unaligned base
    gpu.copy_(host)
    base = region_stain_map(gpu, cell=cell, thresholds=THR)
    assert tuple(base["tissue"].shape) == (5, 4) and base["tissue"].dtype == torch.int64
    assert np.array_equal(base["tissue"].cpu().numpy(), want_t)
    assert np.array_equal(base["positive"].cpu().numpy(), want_p)
    _close(base["burden"].cpu().numpy(), want_p / np.maximum(want_t, 1), F32, "cell burden")
    for src in (gpu, host):
        for band_rows in (16, 50, 128):
            got = region_stain_map(src, cell=cell, band_rows=band_rows, thresholds=THR)
            assert all(torch.equal(got[k], base[k]) for k in base), (src.is_cuda, band_rows)
            assert region_stain_map.last_stats["bands"] > 1
    got = region_stain_map(host, cell=cell, thresholds=THR)
    assert all(torch.equal(got[k], base[k]) for k in base)
    whole = stain_quantify(gpu[None], thresholds=THR)
    assert int(base["tissue"].sum()) == int(whole["tissue"][0])
    assert int(base["positive"].sum()) == int(whole["positive"][0, 1])
    other = region_stain_map(gpu, cell=cell, thresholds=THR, stain=0)
    assert int(other["positive"].sum()) == int(whole["positive"][0, 0])
    one = region_stain_map(gpu, cell=1000, thresholds=THR)                # a cell larger than the region: one owner
    assert tuple(one["tissue"].shape) == (1, 1) and int(one["tissue"]) == int(whole["tissue"][0])


def test_region_stain_agreement():
    H, W = 301, 203
    a, b = _stained(1, H, W, 51)[0], _stained(1, H, W, 52, plaque=0.12)[0]
    b[:150] = a[:150]
    m32 = unmix_matrix("hdab").numpy()
    ref = R.agreement32(a[None], b[None], m32, THR)
    ga, hb = torch.from_numpy(a).to(DEV), torch.from_numpy(b)
    base = region_stain_agreement(ga, torch.from_numpy(b).to(DEV), thresholds=THR)
    assert all(tuple(v.shape) == () for v in base.values())
    _check_pair({k: v[None] for k, v in base.items()}, ref, "region pair")
    for band_rows in (16, 100):
        got = region_stain_agreement(ga, hb, band_rows=band_rows, thresholds=THR)      # one on the GPU, one on the host
        assert all(torch.equal(got[k], base[k]) for k in base), band_rows
    cells = region_stain_agreement(ga, hb, cell=64, thresholds=THR)
    assert tuple(cells["dice"].shape) == (5, 4)
    sub = R.agreement32(a[None, 64:128, 128:192], b[None, 64:128, 128:192], m32, THR)
    _check_pair({k: v[1, 2][None] for k, v in cells.items()}, sub, "one cell of the pair")
    edge = R.agreement32(a[None, 256:, 192:], b[None, 256:, 192:], m32, THR)
    _check_pair({k: v[4, 3][None] for k, v in cells.items()}, edge, "the ragged corner cell")


def test_stain_agreement_in_a_captured_graph():
    a, b = _stained(2, 64, 64, 61), _stained(2, 64, 64, 62)
    ga, gb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    eager = stain_agreement(ga, gb, thresholds=THR)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                  # one stream, one chain of two kernels: no parallel branches
        out = stain_agreement(ga, gb, thresholds=THR)
    for v in out.values():
        v.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(out[k], eager[k]) for k in eager)
    gb.copy_(ga)                                   # the graph reads its inputs at replay
    graph.replay()
    torch.cuda.synchronize()
    assert (out["dice"] == 1).all() and (out["burden_abs_err"] == 0).all()
    del graph


def test_evaluate_generation_with_stain():
    from stain2stain_amd import CFMTrainer, EvalAccumulator, FlowUNet, generation_quality
    torch.manual_seed(1984)
    net = FlowUNet(3, [16, 32], 3, 32, precision="bf16").to("cuda:0").train()
    tr = CFMTrainer(net, lr=1e-3)
    g = torch.Generator().manual_seed(5)
    x0 = (torch.rand(2, 3, 64, 64, generator=g) * 2 - 1).to("cuda:0")
    x1 = torch.from_numpy(_network(_stained(2, 64, 64, 71), 5)).to("cuda:0")
    try:
        plain = tr.evaluate_generation(x0, x1, num_steps=2)
        assert sorted(plain) == ["mae", "mse", "psnr", "ssim"]
        acc = EvalAccumulator()
        got = tr.evaluate_generation(x0, x1, num_steps=2, accumulator=acc, stain={"thresholds": THR})
        assert sorted(got) == ["mae", "mse", "psnr", "ssim", "stain/burden_abs_err", "stain/dice", "stain/iou"]
        for k in plain:
            assert torch.equal(got[k], plain[k]), k
        pred = None

        def sampler(x):
            nonlocal pred
            from stain2stain_amd import samplers
            pred = samplers.solve(tr._generation.velocity(False, net.encoder, net.flow_decoder, net.time_embedding.dim)[0],
                                  samplers._prep_source(x), "euler", 2)
            return pred

        with torch.no_grad():
            via = generation_quality(sampler, x0, x1, stain={"thresholds": THR})
            want = stain_agreement(pred, x1, thresholds=THR)
        for k in ("burden_abs_err", "dice", "iou"):
            assert tuple(got["stain/" + k].shape) == (2,) and torch.equal(got["stain/" + k], want[k]), k
            assert torch.equal(via["stain/" + k], want[k]), k
        epoch = acc.compute()
        assert sorted(epoch) == sorted(got)
        assert abs(float(epoch["stain/dice"]) - float(got["stain/dice"].mean())) <= 1e-6
    finally:
        tr.close()
