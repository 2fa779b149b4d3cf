"""Seeded component selection (s2s_objects_label_seeded, csrc/objects.hip) and the dual-threshold mask (csrc/hysteresis.hip)
against the scipy / numpy restatement of tests/hysteresis_ref.py, on poisoned memory (every ``torch.empty`` and every
``ops._workspace`` slab starts as NaN / 0xFF, as in tests/test_background_gpu.py).

Tolerances: none.  Labels, counts and masks are integers; the burdens, Dice and IoU are one double
quotient of exact integers each, which the restatement forms with the same operations: everything is compared for
equality.  The shapes straddle the 32 x 64 local tile and the 64-lane wave."""
import functools

import numpy as np
import pytest
import torch

import background_ref as G
import hysteresis_ref as Y
import objects_ref as O
import stain_calibrate_ref as C
import stain_quant_ref as R
from stain2stain_amd import (clear_border, hysteresis, hysteresis_mask, hysteresis_thresholds, label_components,
                             object_features, reconstruct_mask, region_stain_objects_hysteresis, select_components,
                             stain_agreement_hysteresis, stain_objects, stain_objects_corrected,
                             stain_objects_hysteresis, stain_quantify_corrected, stain_thresholds)
from stain2stain_amd.stain_quant import unmix_matrix

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 1), (1, 70), (33, 65), (70, 130), (97, 200)]
PS = (0.3, 0.55, 0.62, 0.9)
TABLE = ("area", "bbox", "centroid")


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


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(got, want, what):
    """Equality of a tensor and the restatement's array, dtype and shape included."""
    got, want = got.cpu().numpy(), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), what


def _check(got, ref, what):
    assert sorted(got) == sorted(ref), (what, sorted(got), sorted(ref))
    for k in ref:
        _same(got[k], ref[k], f"{what}: {k}")


def _crop_view(a, top=2, left=3, extra=(5, 7)):
    """[B, H, W(, 3)] as a crop view of a larger GPU array: odd row pitch, unaligned base."""
    a = torch.from_numpy(np.ascontiguousarray(a))
    B, H, W = a.shape[:3]
    big = torch.full((B, H + extra[0], W + extra[1]) + tuple(a.shape[3:]), 77, dtype=a.dtype, device=DEV)
    view = big[:, top:top + H, left:left + W]
    view.copy_(a)
    return view


def _select_one(mask, marker, what, **kw):
    """select_components of one [H, W] pair against the restatement; returns the result."""
    got = select_components(_g(mask), _g(marker), return_mask=True, **kw)
    _check(got, Y.select(mask, marker, **kw), what)
    return got


# ---- 1. parity on Bernoulli masks ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SHAPES)
def test_select_parity(H, W):
    masks = np.stack([O.bernoulli((H, W), p, seed=H * W + int(100 * p)) for p in PS])
    markers = np.stack([O.bernoulli((H, W), 0.01, seed=H + W + int(100 * p)) for p in PS])
    markers[0].flat[np.flatnonzero(masks[0])[:1]] = 1                     # at least one seed that counts
    for conn in (4, 8):
        ref = Y.select_batch(masks, markers, connectivity=conn, max_objects=3)
        got = select_components(_g(masks), _g(markers), connectivity=conn, max_objects=3, return_mask=True)
        _check(got, ref, f"{H}x{W} conn {conn}")
        for n in range(len(PS)):
            assert np.array_equal(ref["mask"][n] != 0, Y.propagation(masks[n], markers[n], conn))
        _same(reconstruct_mask(_g(masks), _g(markers), conn), ref["mask"], "reconstruct")
        got_b = reconstruct_mask(_g(masks).bool(), _g(markers).bool(), conn)
        assert got_b.dtype == torch.bool and np.array_equal(got_b.cpu().numpy(), ref["mask"] != 0)
        want = np.stack([Y.clear_border(m, conn) for m in masks])
        _same(clear_border(_g(masks), conn), want.astype(np.uint8), "clear_border")
        _same(clear_border(_g(masks[1]).bool(), conn), want[1], "clear_border [H, W] bool")


# ---- 2. patterns --------------------------------------------------------------------------------------------------------
def test_patterns():
    H, W = 70, 130
    snake = O.serpentine(H, W)
    ys, xs = np.nonzero(snake)
    far = np.zeros_like(snake)
    far[ys[-1], xs[-1]] = 1                                              # one seed, at the end farthest from the root
    for conn in (4, 8):
        got = _select_one(snake, far, f"serpentine {conn}", connectivity=conn)
        assert int(got["count"]) == 1 and int(got["seed_pixels"]) == 1 and int(got["kept_pixels"]) == int(snake.sum())
        assert np.array_equal(got["mask"].cpu().numpy(), snake)
    board = O.checkerboard(33, 65)
    one = np.zeros_like(board)
    one[0, 0] = 1
    assert int(_select_one(board, one, "checkerboard 8", connectivity=8)["kept_pixels"]) == int(board.sum())
    g4 = _select_one(board, one, "checkerboard 4", connectivity=4)
    assert int(g4["kept_pixels"]) == 1 and int(g4["candidates"]) == int(board.sum())
    for d, corner in zip(O.diagonals(70), ((69, 69), (69, 0))):
        seed = np.zeros_like(d)
        seed[corner] = 1
        assert int(_select_one(d, seed, "diagonal 8", connectivity=8)["kept_pixels"]) == 70
        assert int(_select_one(d, seed, "diagonal 4", connectivity=4)["kept_pixels"]) == 1
    mask = O.bernoulli((H, W), 0.55, seed=7)
    seam = np.zeros_like(mask)                                           # seeds only on the pixels next to a tile seam
    seam[31::32], seam[32::32], seam[:, 63::64], seam[:, 64::64] = 1, 1, 1, 1
    for conn in (4, 8):
        _select_one(mask, seam, f"seam seeds {conn}", connectivity=conn)
    out = _select_one(mask, 1 - mask, "seeds outside the mask")
    assert int(out["count"]) == 0 and int(out["seed_pixels"]) == 0 and int(out["seeded"]) == 0
    assert not out["mask"].any() and not out["labels"].any() and int(out["candidates"]) > 0
    y, x = np.mgrid[0:H, 0:W]
    ring = lambda cy, cx: (((y - cy) ** 2 + (x - cx) ** 2 <= 100) & ((y - cy) ** 2 + (x - cx) ** 2 > 25))
    rings = (ring(20, 30) | ring(45, 90)).astype(np.uint8)
    hole = np.zeros_like(rings)
    hole[20, 30] = 1                                                     # inside the first ring's hole: selects nothing
    hole[45, 98] = 1                                                     # on the second ring
    got = _select_one(rings, hole, "marker in a hole")
    assert int(got["count"]) == 1 and int(got["seed_pixels"]) == 1 and not got["mask"][20, 30 - 8]


# ---- 3. batch mates, views, bits ----------------------------------------------------------------------------------------
def test_batch_mates():
    H, W = 70, 130
    mask = O.bernoulli((H, W), 0.55, seed=11)
    markers = np.stack([np.ones_like(mask), np.zeros_like(mask), O.bernoulli((H, W), 0.01, seed=12)])
    masks = np.stack([mask] * 3)
    kw = dict(connectivity=8, min_area=2, max_objects=9)
    got = select_components(_g(masks), _g(markers), return_mask=True, **kw)
    _check(got, Y.select_batch(masks, markers, **kw), "batch")
    for n in range(3):
        single = select_components(_g(mask), _g(markers[n]), return_mask=True, **kw)
        for k in got:
            assert torch.equal(single[k], got[k][n]), (n, k)
    assert int(got["count"][1]) == 0 and int(got["seeded"][0]) == int(got["candidates"][0])


def test_views_and_bits():
    H, W = 70, 130
    masks = np.stack([O.bernoulli((H, W), p, seed=20 + i) for i, p in enumerate((0.55, 0.62))])
    markers = np.stack([O.bernoulli((H, W), 0.02, seed=30 + i) for i in range(2)])
    ref = Y.select_batch(masks, markers, connectivity=8, max_objects=4)
    vm, vk = _crop_view(masks), _crop_view(markers, top=1, left=6, extra=(3, 9))
    assert not vm.is_contiguous() and not vk.is_contiguous() and vm.stride(1) % 2 == 1 and vk.stride(1) % 2 == 1
    got = select_components(vm, vk, connectivity=8, max_objects=4, return_mask=True)
    _check(got, ref, "views")
    assert (vm.cpu().numpy() == masks).all() and (vk.cpu().numpy() == markers).all()       # the inputs are not written
    _check(select_components(vm[1], vk[1], connectivity=8, max_objects=4, return_mask=True),
           {k: v[1] for k, v in ref.items()}, "[H, W] views")
    # mask and marker in one buffer under different bits (the C ABI as the hysteresis calls use it)
    byte = _g(masks | (markers << 2) | 8)
    res = hysteresis._select(byte.data_ptr(), W, H * W, 1, byte.data_ptr(), W, H * W, 4, 1, False, 2, H, W, byte.device, 8,
                             1, 4, True, "test")
    _check(res, ref, "one buffer")


# ---- 4. options ---------------------------------------------------------------------------------------------------------
def test_options():
    H, W = 70, 130
    mask = O.bernoulli((H, W), 0.55, seed=41)
    marker = O.bernoulli((H, W), 0.05, seed=42)
    lab, n = O.flood_label(mask, 8)
    top = int(np.bincount(lab[(marker != 0) & (mask != 0)], minlength=n + 1)[1:].max())
    assert top >= 3
    for min_seed in (1, 2, top, top + 1):
        for invert in (False, True):
            _select_one(mask, marker, f"min_seed {min_seed} invert {invert}", min_seed=min_seed, invert=invert,
                        max_objects=2)
    assert int(_select_one(mask, marker, "above the largest", min_seed=top + 1)["count"]) == 0
    for min_area in (2, 5, 40):
        _select_one(mask, marker, f"min_area {min_area}", min_seed=2, min_area=min_area, max_objects=3)
        _select_one(mask, marker, f"min_area {min_area} invert", invert=True, min_area=min_area, connectivity=4)


# ---- 5. reductions to label_components ----------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SHAPES)
def test_reduces_to_label_components(H, W):
    masks = _g(np.stack([O.bernoulli((H, W), p, seed=H + 3 * W + int(100 * p)) for p in PS] + [np.ones((H, W), np.uint8)]))
    zero = torch.zeros_like(masks)
    for conn in (4, 8):
        for min_area in (1, 3):
            base = label_components(masks, connectivity=conn, min_area=min_area, max_objects=5)
            a = select_components(masks, masks, connectivity=conn, min_area=min_area, max_objects=5)
            b = select_components(masks, zero, connectivity=conn, min_area=min_area, max_objects=5, invert=True)
            for k in base:
                assert torch.equal(a[k], base[k]) and torch.equal(b[k], base[k]), (conn, min_area, k)
            assert torch.equal(a["seeded"], a["candidates"]) and int(b["seeded"].sum()) == 0
            assert torch.equal(a["seed_pixels"], (masks != 0).sum((1, 2)))


# ---- 6. the dual mask and hysteresis_mask -------------------------------------------------------------------------------
def test_hysteresis_mask_and_counts():
    rng = np.random.default_rng(5)
    B, H, W = 3, 70, 130
    t = np.clip(rng.normal(150, 90, size=(B, H, W)), 0, 4000).astype(np.int16)
    tis = rng.random((B, H, W)) < 0.9
    for j_low, j_high in ((128, 320), (200, 200), (1, 4000), (250, 4095)):
        for conn in (4, 8):
            want = Y.hysteresis(t, tis, j_low, j_high, conn)
            got = hysteresis_mask(_g(t), j_low / 1024, j_high / 1024, tissue=_g(tis), connectivity=conn)
            _same(got, want, f"{j_low} {j_high} {conn}")
        _same(hysteresis_mask(_g(t), j_low / 1024, j_high / 1024), Y.hysteresis(t, None, j_low, j_high), "no tissue")
    assert not hysteresis_mask(_g(t), 250 / 1024, 4095 / 1024).any()                # high above the maximum: empty
    _same(hysteresis_mask(_g(t[0]), 128 / 1024, 320 / 1024, tissue=_g(tis[0].astype(np.uint8)), min_seed=2),
          Y.hysteresis(t[:1], tis[:1], 128, 320, min_seed=2)[0], "[H, W], min_seed 2")
    # the kernel itself: the byte, the counts, pool and reset
    gt, gtis = _g(t), _g(tis.astype(np.uint8))
    byte, counts = Y.dual(t, tis, 128, 320)
    for pool in (False, True):
        c = torch.empty((1 if pool else B, 3), dtype=torch.int64, device=DEV)
        m = torch.empty((B, H, W), dtype=torch.uint8, device=DEV)
        hysteresis._dual_mask(gt.data_ptr(), gtis.data_ptr(), B, H, W, 0, H, 128, 320, pool, 1, c, m.data_ptr(), H * W, "t")
        _same(m, byte, "byte")
        _same(c, counts.sum(0, keepdims=True) if pool else counts, f"counts pool {pool}")
        hysteresis._dual_mask(gt.data_ptr(), gtis.data_ptr(), B, H, W, 0, H, 128, 320, pool, 0, c, m.data_ptr(), H * W, "t")
        _same(c, 2 * (counts.sum(0, keepdims=True) if pool else counts), f"counts added, pool {pool}")
    # a window of rows: only those are written and counted
    c = torch.empty((B, 3), dtype=torch.int64, device=DEV)
    m = torch.full((B, 20, W), 99, dtype=torch.uint8, device=DEV)
    hysteresis._dual_mask(gt.data_ptr(), gtis.data_ptr(), B, H, W, 13, 7, 128, 320, False, 1, c, m.data_ptr(), 20 * W, "t")
    wb, wc = Y.dual(t[:, 13:20], tis[:, 13:20], 128, 320)
    _same(m[:, :7], wb, "window byte")
    _same(c, wc, "window counts")
    assert (m[:, 7:] == 99).all()


def test_plaques_with_halo_and_speckle():
    """The case the feature exists for (tests/test_hysteresis_cpu.py states it on the restatement)."""
    t, halo = Y.plaques()
    got = hysteresis_mask(_g(t), 128 / 1024, 320 / 1024)
    assert np.array_equal(got.cpu().numpy() != 0, halo) and int(got.sum()) == 1012
    assert int(label_components(got)["count"]) == 4
    low = label_components(_g((t >= 128).astype(np.uint8)))
    assert int(low["kept_pixels"]) == 1259 and int(low["count"]) == 233
    assert int(hysteresis_mask(_g(t), 320 / 1024, 320 / 1024).sum()) == 116


# ---- 7. stains ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tiles(B, H, W, seed):
    """uint8 [B, H, W, 3]: haematoxylin, a DAB haze that varies over the tile, blobs with a halo and a core, noise, glass."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    conc = np.zeros((B, H, W, 3))
    conc[..., 0] = rng.uniform(0.05, 0.5, size=(B, H, W))
    for n in range(B):
        haze = 0.05 + 0.2 * x / max(W - 1, 1) + 0.05 * np.sin(y / 9.0 + n)
        spots = [(int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(2, 7))) for _ in range(10)]
        halo = G.discs(H, W, spots)
        core = G.discs(H, W, [(cy, cx, 1) for cy, cx, _ in spots[::2]])          # every other blob has no core
        conc[n, ..., 1] = haze + 0.2 * halo + 0.4 * core + rng.normal(0, 0.03, size=(H, W))
    img = R.synthesise(np.maximum(conc, 0), "hdab").astype(np.int32) + rng.integers(-2, 3, size=(B, H, W, 3))
    img = np.clip(img, 0, 255).astype(np.uint8)
    glass = rng.random((B, H, W)) < 0.1
    img[glass] = rng.integers(225, 256, size=(int(glass.sum()), 3), dtype=np.uint8)
    return img


def _network(u8, seed):
    """uint8 [B, H, W, 3] -> fp32 [B, 3, H, W] in the network's range with a sub-level jitter and out-of-range values."""
    rng = np.random.default_rng(seed)
    lv = u8.astype(np.float64).transpose(0, 3, 1, 2) + rng.random(u8.transpose(0, 3, 1, 2).shape) * 0.98
    x = np.ascontiguousarray((lv / 127.5 - 1.0).astype(np.float32))
    x.reshape(-1)[::7] += 3.0
    return x


STAIN_KEYS = ("count", "tissue", "positive", "burden", "largest", "size_hist", "labels", "mask", "weak", "strong",
              "candidates", "seeded")


def _check_stain(got, ref, what, table=False):
    for k in STAIN_KEYS + (TABLE if table else ()):
        _same(got[k], ref[k], f"{what}: {k}")


@pytest.mark.parametrize("radius,smooth", [(None, 2), (5, 0), (5, 2), (17, 0), (17, 2)])
def test_stain_objects_hysteresis(radius, smooth):
    m32 = _m32()
    u8 = _tiles(3, 70, 90, 5)
    g = _crop_view(u8)
    J_LOW, J_HIGH = (200, 420) if radius is None else (100, 320)
    what = f"r {radius} s {smooth}"
    ref = Y.stain_objects(u8, m32, J_LOW, J_HIGH, radius, smooth=smooth, min_area=2, max_objects=4)
    assert 0 < ref["seeded"].sum() < ref["candidates"].sum() and (ref["strong"] > 0).all()
    got = stain_objects_hysteresis(g, J_LOW / 1024, J_HIGH / 1024, radius=radius, smooth=smooth, min_area=2,
                                   max_objects=4, mpp=0.5, return_labels=True, return_mask=True)
    _check_stain(got, ref, what, table=True)
    tissue = ref["tissue"]
    mm2 = tissue.astype(np.float64) * (0.5 * 0.5 * 1e-6)
    _same(got["per_mm2"], np.where(tissue > 0, ref["count"].astype(np.float64) / np.where(tissue > 0, mm2, 1.0), 0.0),
          what + " per_mm2")
    lean = stain_objects_hysteresis(g, J_LOW / 1024, J_HIGH / 1024, radius=radius, smooth=smooth)
    assert "labels" not in lean and "mask" not in lean and "per_mm2" not in lean and "area" not in lean
    # weak and strong are the positive counts of the two single thresholds: suffix sums of the corrected histogram
    q = stain_quantify_corrected(g, radius, J_LOW / 1024, smooth=smooth)
    assert torch.equal(got["weak"], q["hist"][:, 1, J_LOW:].sum(1)) and torch.equal(got["weak"], q["positive"])
    assert torch.equal(got["strong"], q["hist"][:, 1, J_HIGH:].sum(1)) and torch.equal(got["tissue"], q["tissue"])
    # low == high: the single threshold of stain_objects / stain_objects_corrected
    for j in (J_LOW, J_HIGH):
        h = stain_objects_hysteresis(g, j / 1024, j / 1024, radius=radius, smooth=smooth, min_area=3, max_objects=4,
                                     return_labels=True)
        if radius is None:
            s = stain_objects(g, thresholds=(j / 1024,) * 3, min_area=3, max_objects=4, return_labels=True)
        else:
            s = stain_objects_corrected(g, radius, j / 1024, smooth=smooth, min_area=3, max_objects=4, return_labels=True)
        for k in ("labels", "count", "tissue", "positive", "largest", "size_hist") + TABLE:
            assert torch.equal(h[k], s[k]), (what, j, k)
        assert torch.equal(h["weak"], h["strong"]) and torch.equal(h["seeded"], h["candidates"])
    # high above the maximum: empty
    top = int(Y.stain_t(u8, m32, radius, smooth=smooth)[0].max())
    if top < 4095:
        e = stain_objects_hysteresis(g, J_LOW / 1024, 4095 / 1024, radius=radius, smooth=smooth, return_labels=True)
        assert not e["labels"].any() and not e["count"].any() and not e["positive"].any() and not e["strong"].any()
        assert torch.equal(e["weak"], got["weak"]) and (e["burden"] == 0).all()
    # the labels feed the per-object measurements unchanged
    f = object_features(got["labels"], max_objects=4)
    assert torch.equal(f["area"].long(), got["area"].long())


def test_stain_other_forms():
    """fp32 tiles; another stain, tissue rule, footprint, connectivity and min_seed."""
    m32 = _m32()
    u8 = _tiles(2, 37, 53, 6)
    x = _network(u8, 7)
    got = stain_objects_hysteresis(_g(x), 100 / 1024, 320 / 1024, radius=5, return_labels=True, return_mask=True)
    _check_stain(got, Y.stain_objects(R.nchw_to_u8(x), m32, 100, 320, 5), "f32")
    got = stain_objects_hysteresis(_g(x), 200 / 1024, 420 / 1024, return_labels=True, return_mask=True)
    _check_stain(got, Y.stain_objects(R.nchw_to_u8(x), m32, 200, 420), "f32, no radius")
    got = stain_objects_hysteresis(_g(u8), 150 / 1024, 300 / 1024, radius=4.5, smooth=1, footprint="square", stain=0,
                                   white=200, black=10, connectivity=4, min_seed=2, return_labels=True, return_mask=True)
    ref = Y.stain_objects(u8, m32, 150, 300, 4.5, stain=0, smooth=1, kind="square", white=200, black=10, connectivity=4,
                          min_seed=2)
    assert ref["candidates"].sum() > 0
    _check_stain(got, ref, "stain 0")


def test_agreement_hysteresis():
    m32 = _m32()
    a, b = _tiles(3, 37, 53, 9).copy(), _tiles(3, 37, 53, 10).copy()
    b[:, :18] = a[:, :18]                                                  # the masks overlap
    a[2], b[2] = 255, 250                                                  # glass: both masks empty
    for radius, lo, hi in ((None, 200, 420), (5, 100, 320)):
        ref = Y.agreement(a, b, m32, lo, hi, radius)
        assert ref["dice"][2] == 1.0 and ref["iou"][2] == 1.0 and 0.0 < ref["dice"][0] < 1.0
        got = stain_agreement_hysteresis(_g(a), _g(b), lo / 1024, hi / 1024, radius=radius)
        _check(got, ref, f"agreement r {radius}")
    xa, xb = _network(a, 1), _network(b, 2)
    ref = Y.agreement(R.nchw_to_u8(xa), R.nchw_to_u8(xb), m32, 100, 320, 5, smooth=0, connectivity=4)
    got = stain_agreement_hysteresis(_g(xa), _g(xb), 100 / 1024, 320 / 1024, radius=5, smooth=0, connectivity=4)
    _check(got, ref, "agreement f32")


# ---- 8. regions ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _region():
    """uint8 [150, 140, 3] with a blob whose core (rows 15..19) lies in the band [0, 20) and whose halo reaches row 25."""
    H, W = 150, 140
    base = _tiles(1, H, W, 12)[0].copy()
    y, x = np.mgrid[0:H, 0:W]
    d2 = (y - 17) ** 2 + (x - 60) ** 2
    conc = np.zeros((H, W, 3))
    conc[..., 0] = 0.3
    conc[..., 1] = 0.1 + 0.25 * (d2 <= 64) + 0.5 * (d2 <= 4)
    blob = R.synthesise(conc, "hdab")
    near = d2 <= 144
    base[near] = blob[near]
    return base


def test_region_equals_batch_for_every_banding():
    H, W = 150, 140
    region = _region()
    lo, hi = 100 / 1024, 320 / 1024
    kw = dict(radius=9, smooth=1, min_area=2, max_objects=6, return_labels=True, return_mask=True)
    ref = Y.stain_objects(region[None], _m32(), 100, 320, 9, smooth=1, min_area=2, max_objects=6)
    lab = ref["labels"][0]
    strong = (Y.dual(*Y.stain_t(region[None], _m32(), 9, smooth=1), 100, 320)[0][0] & 4) != 0
    assert lab[17, 60] > 0 and lab[17, 60] == lab[24, 60] and strong[17, 60]
    assert not strong[20:][lab[20:] == lab[17, 60]].any()                 # every seed of that object lies above row 20
    g = _g(region)
    whole = stain_objects_hysteresis(g[None], lo, hi, **kw)
    _check_stain(whole, ref, "batch", table=True)
    pitched = _crop_view(region[None])[0]
    for src, name in ((g, "gpu"), (pitched, "gpu view"), (torch.from_numpy(region.copy()), "host")):
        for band_rows in (1, 7, 20, H, None):
            r = region_stain_objects_hysteresis(src, lo, hi, band_rows=band_rows, **kw)
            assert sorted(r) == sorted(whole)
            for k in whole:
                assert torch.equal(r[k], whole[k][0]), (name, band_rows, k)
    none = region_stain_objects_hysteresis(g, 200 / 1024, 420 / 1024, band_rows=7, return_labels=True)
    base = stain_objects_hysteresis(g[None], 200 / 1024, 420 / 1024, return_labels=True)
    for k in base:
        assert torch.equal(none[k], base[k][0]), k


# ---- 9. the pair of thresholds ------------------------------------------------------------------------------------------
def test_hysteresis_thresholds_from_a_histogram():
    t, _ = Y.plaques()
    rng = np.random.default_rng(3)
    t = (t + rng.integers(0, 30, size=t.shape)).astype(np.int16)
    hist = np.zeros((1, 3, 4096), np.int64)
    hist[0, 1] = np.bincount(t.ravel(), minlength=4096)
    hist[0, 0] = np.bincount(np.minimum(t.ravel() * 3, 4095), minlength=4096)
    (jo, vo), (jt, vt) = C.otsu(hist[0, 1]), C.triangle(hist[0, 1])
    assert vo and vt and jo >= 1 and jt >= 1
    th = stain_thresholds({"hist": _g(hist), "tissue": _g(np.array([t.size], np.int64))})
    low, high = hysteresis_thresholds(th)
    assert (low, high) == (jt / 1024, max(jo, jt) / 1024)
    assert hysteresis_thresholds(th, low="otsu", high="triangle") == (jo / 1024, max(jo, jt) / 1024)
    lo, hi = sorted((jo, jt))
    assert lo < hi                                                        # one of the two orders has to raise high to low
    (jo0, _), (jt0, _) = C.otsu(hist[0, 0]), C.triangle(hist[0, 0])
    assert hysteresis_thresholds(th, stain=0) == (jt0 / 1024, max(jo0, jt0) / 1024)
    with pytest.raises(ValueError):
        hysteresis_thresholds(th, stain=2)                                # an empty histogram: no rule answers
    assert hysteresis_thresholds(th, stain=2, fallback=(lo / 1024, hi / 1024)) == (lo / 1024, hi / 1024)
    got = hysteresis_mask(_g(t), low, high)                               # the two floats are on the grid
    _same(got, Y.hysteresis(t[None], None, jt, max(jo, jt))[0], "mask at the calibrated pair")
