"""The grey-morphology and background-subtraction kernels (csrc/grey_morph.hip) against the numpy / scipy restatement of
tests/background_ref.py, on poisoned memory (every ``torch.empty`` and every ``ops._workspace`` slab starts as NaN / 0xFF,
as in tests/test_stain_calibrate_gpu.py).

Tolerances: none.  Minima, maxima, sums and differences on the integer 1/1024 OD grid are integers, the
burdens and means one double quotient of exact integers each, which the restatement forms with the same operations:
everything is compared for equality.  The one fp32 number, the object burden of ``stain_objects_corrected``, is one
rounding of the same double quotient and is compared for equality too."""
import functools

import numpy as np
import pytest
import torch

import background_ref as G
import stain_quant_ref as R
from stain2stain_amd import (concentration_bins, grey_morphology, label_components, mask_morphology,
                             region_stain_quantify_corrected, stain_agreement_corrected, stain_background,
                             stain_histogram, stain_objects_corrected, stain_quantify, stain_quantify_corrected,
                             stain_thresholds)
from stain2stain_amd.stain_quant import unmix_matrix

pytestmark = pytest.mark.gpu
DEV = "cuda"
SMALL = [(1, 1), (1, 9), (5, 1), (23, 31)]
LARGE = [(63, 65), (129, 131), (70, 300)]
RADII = (0, 1, 1.5, 2, 3.5, 4, 5, 7.5, 8, 16, 17)
RADIUS_BEYOND = 40
J = 205


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


def _m32():
    return unmix_matrix("hdab").numpy()


def _same(got, want, what):
    """Equality of a tensor and the restatement's array, dtype and shape included."""
    got, want = got.cpu().numpy(), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), what


def _crop_view(a):
    """[B, H, W(, 3)] as a crop view of a larger GPU array: odd row pitch, unaligned base."""
    a = torch.from_numpy(np.ascontiguousarray(a))
    B, H, W = a.shape[:3]
    big = torch.full((B, H + 5, W + 7) + tuple(a.shape[3:]), 77, dtype=a.dtype, device=DEV)
    view = big[:, 2:2 + H, 3:3 + W]
    view.copy_(a)
    return view


@functools.lru_cache(maxsize=None)
def _tiles(B, H, W, seed):
    """uint8 [B, H, W, 3]: haematoxylin, a DAB haze that varies over the tile, DAB blobs on it, noise, glass, specks."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    conc = np.zeros((B, H, W, 3))
    conc[..., 0] = rng.uniform(0.05, 0.5, size=(B, H, W))
    for n in range(B):
        haze = 0.05 + 0.35 * x / max(W - 1, 1) + 0.1 * np.sin(y / 9.0 + n)
        blobs = G.discs(H, W, [(int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(1, 6)))
                               for _ in range(12)])
        conc[n, ..., 1] = haze + 0.4 * blobs + rng.normal(0, 0.02, size=(H, W))
    img = R.synthesise(np.maximum(conc, 0), "hdab").astype(np.int32) + rng.integers(-2, 3, size=(B, H, W, 3))
    img = np.clip(img, 0, 255).astype(np.uint8)
    glass = rng.random((B, H, W)) < 0.1
    img[glass] = rng.integers(225, 256, size=(int(glass.sum()), 3), dtype=np.uint8)
    img[rng.random((B, H, W)) < 0.01] = 0
    return img


def _network(u8, seed):
    """uint8 [B, H, W, 3] -> fp32 [B, 3, H, W] in the network's range with a sub-level jitter and out-of-range values."""
    rng = np.random.default_rng(seed)
    lv = u8.astype(np.float64).transpose(0, 3, 1, 2) + rng.random(u8.transpose(0, 3, 1, 2).shape) * 0.98
    x = np.ascontiguousarray((lv / 127.5 - 1.0).astype(np.float32))
    x.reshape(-1)[::7] += 3.0
    return x


# ---- 1. grey_morphology against the restatement ------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SMALL + LARGE)
def test_grey_morphology_parity(H, W):
    for dtype, tdtype in ((np.uint8, torch.uint8), (np.int16, torch.int16)):
        names, x = G.stack(H, W, dtype, seed=3 * H + W)
        gx = torch.from_numpy(x).to(DEV)
        for kind in G.FOOTPRINTS:
            for r in RADII + ((RADIUS_BEYOND,) if (H, W) in SMALL else ()):
                ref = G.all_ops(x, r, kind)
                for op in G.OPS:
                    got = grey_morphology(gx, op, r, kind)
                    assert got.dtype == tdtype and got.is_cuda
                    if not torch.equal(got.cpu(), torch.from_numpy(ref[op])):
                        bad = [names[i] for i in range(len(names)) if not np.array_equal(got[i].cpu().numpy(), ref[op][i])]
                        raise AssertionError((dtype.__name__, kind, r, op, bad))


def test_one_high_pixel_dilates_to_the_footprint():
    x = np.zeros((41, 45), np.int16)
    x[20, 22] = 4095
    for kind in G.FOOTPRINTS:
        for r in (0, 1.5, 4, 7.5, 16):
            F = G.footprint(r, kind)
            R_ = F.shape[0] // 2
            want = np.zeros((41, 45), bool)
            want[20 - R_:21 + R_, 22 - R_:23 + R_] = F
            got = grey_morphology(torch.from_numpy(x).to(DEV), "dilate", r, kind)
            assert np.array_equal(got.cpu().numpy() == 4095, want), (kind, r)


@pytest.mark.parametrize("H,W", [(23, 31), (70, 300)])
def test_grey_morphology_forms(H, W):
    """Batch mates, a row-strided crop view, a host input, no batch dimension."""
    for dtype in (np.uint8, np.int16):
        top = 255 if dtype == np.uint8 else 4095
        _, x = G.stack(H, W, dtype, seed=H)
        trio = np.stack([np.zeros((H, W), dtype), x[0], np.full((H, W), top, dtype)])
        for r, kind in ((5, "disc"), (17, "disc"), (8, "square")):
            refs = G.all_ops(x, r, kind)
            for op in ("open", "dilate", "tophat", "bothat"):
                what = (dtype.__name__, r, kind, op)
                ref = refs[op]
                got = grey_morphology(torch.from_numpy(trio).to(DEV), op, r, kind)        # nothing bleeds across samples
                _same(got[1], ref[0], what)
                flat = top if op in ("open", "dilate") else 0
                assert (got[0] == 0).all() and (got[2] == flat).all(), what
                view = _crop_view(x)
                assert not view.is_contiguous()
                _same(grey_morphology(view, op, r, kind), ref, what)
                assert (view.cpu().numpy() == x).all(), what                             # the input is not written
                host = grey_morphology(torch.from_numpy(x), op, r, kind)
                assert not host.is_cuda
                _same(host, ref, what)
                _same(grey_morphology(torch.from_numpy(x[0]).to(DEV), op, r, kind), ref[0], what)
                _same(grey_morphology(view[1], op, r, kind), ref[1], what)


def test_binary_masks_equal_mask_morphology():
    """Two independent kernels: the span gather here, the exact distance transform there."""
    rng = np.random.default_rng(11)
    for H, W in ((23, 31), (63, 65)):
        masks = np.stack([G.discs(H, W, [(H // 2, W // 2, min(H, W) // 3), (2, 3, 4), (H - 1, W - 5, 6)]),
                          rng.random((H, W)) < 0.5, rng.random((H, W)) < 0.97, np.zeros((H, W), bool),
                          np.ones((H, W), bool)]).astype(np.uint8)
        gm = torch.from_numpy(masks).to(DEV)
        for r in (0, 1, 1.5, 2, 3.5, 5, 7.5, 16):
            for op in ("erode", "dilate", "open", "close"):
                assert torch.equal(grey_morphology(gm, op, r), mask_morphology(gm, op, r)), (H, W, r, op)


# ---- 2. the bins --------------------------------------------------------------------------------------------------------
def test_concentration_bins():
    u8 = _tiles(2, 37, 53, 1)
    m32 = _m32()
    for stain in (0, 1, 2):
        _same(concentration_bins(_crop_view(u8), stain=stain), G.bins(u8, m32, stain), f"u8 {stain}")
    x = _network(u8, 2)
    seen = R.nchw_to_u8(x)
    _same(concentration_bins(torch.from_numpy(x).to(DEV)), G.bins(seen, m32, 1), "f32")
    got = concentration_bins(torch.from_numpy(u8).to(DEV))
    assert got.dtype == torch.int16 and int(got.min()) >= 0 and int(got.max()) <= 4095


# ---- 3. nothing subtracted: today's numbers -----------------------------------------------------------------------------
def test_radius_none_reduces_to_stain_quantify():
    u8 = _tiles(3, 37, 53, 3)
    for tiles in (torch.from_numpy(u8).to(DEV), torch.from_numpy(_network(u8, 4)).to(DEV)):
        for stain in (0, 1):
            for j in (1, 100, J, 4095):
                q = stain_quantify_corrected(tiles, None, j / 1024, stain=stain)
                base = stain_quantify(tiles, thresholds=(j / 1024,) * 3)
                assert torch.equal(q["positive"], base["positive"][:, stain]) and torch.equal(q["tissue"], base["tissue"])
            h = stain_histogram(tiles)
            assert torch.equal(q["hist"][:, stain], h["hist"][:, stain])
            others = [k for k in range(3) if k != stain]
            assert (q["hist"][:, others] == 0).all()
            assert torch.equal(q["sum_t"], (h["hist"][:, stain] * torch.arange(4096, device=DEV)).sum(1))


# ---- 4. the corrected numbers against the restatement -------------------------------------------------------------------
KEYS = ("tissue", "positive", "sum_t", "burden", "mean_t", "hist")


def _check_corrected(q, ref, what, maps=True):
    for k in KEYS + (("mask", "corrected") if maps else ()):
        _same(q[k], ref[k], f"{what} {k}")


@pytest.mark.parametrize("radius", [5, 17])
@pytest.mark.parametrize("smooth", [0, 2])
def test_corrected_parity(radius, smooth):
    m32 = _m32()
    u8 = _tiles(3, 70, 90, 5)
    what = f"r {radius} s {smooth}"
    ref = G.corrected(u8, m32, radius, J, smooth=smooth)
    g = _crop_view(u8)
    q = stain_quantify_corrected(g, radius, J / 1024, smooth=smooth, return_mask=True, return_corrected=True)
    _check_corrected(q, ref, what)
    assert q["stain"] == 1 and q["threshold_bin"] == J
    _same(stain_background(g, radius, smooth=smooth), ref["bg"], what + " background")
    # the suffix sums of the histogram are the positive counts at every threshold
    pos = stain_thresholds(q)["positive"][:, 1]
    for j in (1, 50, J, 400, 4095):
        _same(pos[:, j], G.corrected(u8, m32, radius, j, smooth=smooth)["positive"], f"{what} suffix {j}")
    _same(pos[:, J], ref["positive"], what + " suffix")
    # one owner over the batch = the sum of the samples; out= accumulates
    p = stain_quantify_corrected(g, radius, J / 1024, smooth=smooth, pool=True)
    _check_corrected(p, G.corrected(u8, m32, radius, J, smooth=smooth, pool=True), what + " pool", maps=False)
    for k in ("tissue", "positive", "sum_t", "hist"):
        assert torch.equal(p[k], q[k].sum(0, keepdim=True)), k
    twice = stain_quantify_corrected(g, radius, J / 1024, smooth=smooth, pool=True, out=p)
    assert twice is p
    for k in ("tissue", "positive", "sum_t", "hist"):
        assert torch.equal(p[k], 2 * q[k].sum(0, keepdim=True)), k
    _same(p["burden"], G.corrected(u8, m32, radius, J, smooth=smooth, pool=True)["burden"], what + " burden after out=")
    with pytest.raises(ValueError):
        stain_quantify_corrected(g, radius, 100 / 1024, smooth=smooth, pool=True, out=p)
    with pytest.raises(ValueError):
        stain_quantify_corrected(g, radius, J / 1024, smooth=smooth, out=p)                # B owners into one


def test_corrected_other_forms():
    """fp32 tiles, the square, another stain and tissue rule, a single pixel."""
    m32 = _m32()
    u8 = _tiles(2, 37, 53, 6)
    x = _network(u8, 7)
    q = stain_quantify_corrected(torch.from_numpy(x).to(DEV), 5, J / 1024, return_mask=True, return_corrected=True)
    _check_corrected(q, G.corrected(R.nchw_to_u8(x), m32, 5, J), "f32")
    g = torch.from_numpy(u8).to(DEV)
    q = stain_quantify_corrected(g, 4.5, 60 / 1024, stain=0, smooth=1, footprint="square", white=200, black=10,
                                 return_mask=True, return_corrected=True)
    _check_corrected(q, G.corrected(u8, m32, 4.5, 60, stain=0, smooth=1, kind="square", white=200, black=10), "square")
    one = u8[:1, :1, :1]
    q = stain_quantify_corrected(torch.from_numpy(one.copy()).to(DEV), 128, J / 1024, return_mask=True,
                                 return_corrected=True)
    _check_corrected(q, G.corrected(one, m32, 128, J), "1 x 1")


# ---- 5. objects and agreement -------------------------------------------------------------------------------------------
def test_objects_corrected():
    m32 = _m32()
    u8 = _tiles(2, 70, 90, 8)
    ref = G.corrected(u8, m32, 9, 150)
    mpp, min_area = 0.5, 20
    got = stain_objects_corrected(torch.from_numpy(u8).to(DEV), 9, 150 / 1024, min_area=min_area, connectivity=8,
                                  max_objects=16, mpp=mpp, return_labels=True)
    lab = label_components(torch.from_numpy(ref["mask"] & 1).to(DEV), connectivity=8, min_area=min_area, max_objects=16)
    assert int(lab["count"].sum()) > 0
    for k in ("count", "largest", "size_hist", "labels", "area", "bbox", "centroid"):
        assert torch.equal(got[k], lab[k]), k
    assert torch.equal(got["positive"], lab["kept_pixels"])
    _same(got["tissue"], ref["tissue"], "tissue")
    kept, tissue = lab["kept_pixels"].cpu().numpy(), ref["tissue"]
    _same(got["burden"], (kept.astype(np.float64) / np.maximum(tissue, 1).astype(np.float64)).astype(np.float32), "burden")
    mm2 = tissue.astype(np.float64) * (mpp * mpp * 1e-6)
    count = lab["count"].cpu().numpy().astype(np.float64)
    _same(got["per_mm2"], np.where(tissue > 0, count / np.where(tissue > 0, mm2, 1.0), 0.0), "per_mm2")
    # min_area = 1 keeps every positive pixel
    every = stain_objects_corrected(torch.from_numpy(u8).to(DEV), 9, 150 / 1024)
    _same(every["positive"], ref["positive"], "positive")


def test_agreement_corrected():
    m32 = _m32()
    a, b = _tiles(3, 37, 53, 9).copy(), _tiles(3, 37, 53, 10).copy()
    b[:, :18] = a[:, :18]                                                  # the masks overlap
    a[2], b[2] = 255, 250                                                  # glass: both masks empty
    ref = G.agreement(a, b, m32, 5, 100)
    assert ref["dice"][2] == 1.0 and ref["iou"][2] == 1.0 and 0.0 < ref["dice"][0] < 1.0
    got = stain_agreement_corrected(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), 5, 100 / 1024)
    assert sorted(got) == sorted(ref)
    for k in ref:
        _same(got[k], ref[k], k)
    xa, xb = _network(a, 1), _network(b, 2)
    ref = G.agreement(R.nchw_to_u8(xa), R.nchw_to_u8(xb), m32, 5, 100, smooth=0)
    got = stain_agreement_corrected(torch.from_numpy(xa).to(DEV), torch.from_numpy(xb).to(DEV), 5, 100 / 1024, smooth=0)
    for k in ref:
        _same(got[k], ref[k], "f32 " + k)


# ---- 6. regions ---------------------------------------------------------------------------------------------------------
def test_region_equals_batch_for_every_banding():
    m32 = _m32()
    H, W = 150, 140
    region = _tiles(1, H, W, 12)[0]
    ref = G.corrected(region[None], m32, 9, J, smooth=1)
    g = torch.from_numpy(region.copy()).to(DEV)
    whole = stain_quantify_corrected(g[None], 9, J / 1024, smooth=1, return_mask=True, return_corrected=True)
    _check_corrected(whole, ref, "batch")
    pitched = _crop_view(region[None])[0]
    for src, name in ((g, "gpu"), (pitched, "gpu view"), (torch.from_numpy(region.copy()), "host")):
        for band_rows in (1, 7, 20, H, None):
            r = region_stain_quantify_corrected(src, 9, J / 1024, band_rows=band_rows, smooth=1, return_mask=True,
                                                return_corrected=True)
            what = f"{name} band_rows {band_rows}"
            for k in KEYS:
                assert torch.equal(r[k], whole[k]), (what, k)
            assert torch.equal(r["mask"], whole["mask"][0]) and torch.equal(r["corrected"], whole["corrected"][0]), what
            stats = region_stain_quantify_corrected.last_stats
            nb = 1 if band_rows is None else -(-H // band_rows)
            assert stats["bands"] == nb and stats["band_rows"] <= (band_rows or H) + 2 * (2 * 9 + 1), what
    r = region_stain_quantify_corrected(g, None, J / 1024, band_rows=7)
    assert torch.equal(r["positive"], stain_quantify(g[None], thresholds=(J / 1024,) * 3)["positive"][:, 1])


# ---- 7. what it is for --------------------------------------------------------------------------------------------------
def test_haze_and_blobs():
    """A linear haze of 0..600 (in 1/1024 OD) across 160 columns with five blobs of +400 and radius 4 on it.  A global
    threshold of 200 / 1024 calls the high half of the haze positive; after a top-hat of radius 8 the positive mask is
    exactly the blobs (away from the image edges, where the opening underestimates a rising background)."""
    H, W, r = 64, 160, 8
    centres = [(14, 20), (40, 45), (22, 80), (48, 118), (30, 140)]
    blobs = G.discs(H, W, [(cy, cx, 4) for cy, cx in centres])
    x = np.mgrid[0:H, 0:W][1]
    conc = np.zeros((1, H, W, 3))
    conc[..., 0] = 0.3
    conc[0, ..., 1] = (600.0 * x / (W - 1) + 400.0 * blobs) / 1024.0
    u8 = R.synthesise(conc, "hdab")
    assert R.tissue(u8).all()
    g = torch.from_numpy(u8).to(DEV)
    thr = 200 / 1024
    ref = G.corrected(u8, _m32(), r, 200, smooth=0)
    q = stain_quantify_corrected(g, r, thr, smooth=0, return_mask=True)
    _same(q["mask"], ref["mask"], "mask")
    pos = (q["mask"][0] & 1).bool().cpu().numpy()
    inner = (slice(r + 1, H - r - 1), slice(r + 1, W - r - 1))
    assert np.array_equal(pos[inner], blobs[inner]) and blobs[inner].sum() == blobs.sum() == 5 * 49
    raw = stain_quantify_corrected(g, None, thr, return_mask=True)
    raw_pos = (raw["mask"][0] & 1).bool().cpu().numpy()
    assert raw_pos[:, W // 2:].all() and not raw_pos[:, :40][~blobs[:, :40]].any()
    assert int(raw["positive"][0]) > 20 * int(q["positive"][0]) > 0
