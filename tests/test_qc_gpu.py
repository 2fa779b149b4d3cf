"""Tile quality control (csrc/qc.hip) against the numpy int64 restatement of tests/qc_ref.py, on poisoned
memory (every ``torch.empty`` and every workspace starts as 0xFF, as in tests/test_region_warp_gpu.py).  GPU inputs are
crop views with an odd row pitch and an unaligned base inside a guard band of a constant byte, plus an aligned
contiguous copy, so both load paths run and a wrong index shows as a wrong count.

What must hold.  The eight counts are integers and bit-equal to the restatement, for host and GPU input and for every
banding; the fp64 values are within 1e-12 relative of the fp64 quotients of those integers (the same IEEE operations on
the same integers: in practice they are equal)."""
import functools

import numpy as np
import pytest
import torch

import qc_ref as Q
from stain2stain_amd import qc_keep, region_qc, region_qc_map, tile_qc, translate_region, window_sums

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 77
DERIVED = ("focus", "tissue_frac", "ink_frac", "dark_frac", "mean_luma")


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


def _t(arr):
    """A host tensor that owns a copy of ``arr`` (the shared references are read-only)."""
    return torch.from_numpy(np.array(arr))


def _view(arr):
    """A uint8 region [H, W, 3] or batch [B, H, W, 3] as a crop view of a larger GPU array of GUARD bytes: odd row pitch,
    unaligned base.  Returns (view, the larger array)."""
    lead = arr.shape[:-3]
    H, W = arr.shape[-3:-1]
    pad = next(p for p in (6, 7, 8, 9) if ((W + p) * 3) % 4 != 0 and ((2 * (W + p) + 3) * 3) % 4 != 0)
    big = torch.full(lead + (H + 5, W + pad, 3), GUARD, dtype=torch.uint8, device=DEV)
    view = big[..., 2:2 + H, 3:3 + W, :]
    view.copy_(_t(arr))
    assert view.stride(-3) % 4 != 0 and view.data_ptr() % 4 != 0
    return view, big


def _guard_intact(big, arr):
    H, W = arr.shape[-3:-1]
    g = big.clone()
    g[..., 2:2 + H, 3:3 + W, :] = GUARD
    return bool((g == GUARD).all()) and np.array_equal(big[..., 2:2 + H, 3:3 + W, :].cpu().numpy(), arr)


def _check(got, want, what):
    """counts bit-equal; the fp64 values within 1e-12 relative of the quotients of the exact integers; no NaN."""
    counts = got["counts"].cpu().numpy()
    assert got["counts"].dtype == torch.int64 and counts.shape == want["counts"].shape, what
    bad = np.argwhere(counts != want["counts"])
    assert bad.size == 0, (what, bad[:4].tolist(), counts[tuple(bad[0][:-1])].tolist(),
                           want["counts"][tuple(bad[0][:-1])].tolist())
    for k in DERIVED:
        v = got[k].cpu().numpy()
        assert got[k].dtype == torch.float64 and v.shape == want[k].shape and np.isfinite(v).all(), (what, k)
        assert (np.abs(v - want[k]) <= 1e-12 * np.abs(want[k])).all(), (what, k, v.tolist(), want[k].tolist())


def _both_layouts(arr):
    """(name, GPU tensor, guard array or None): the crop view and the aligned contiguous copy."""
    view, big = _view(arr)
    return (("view", view, big), ("contiguous", _t(arr).to(DEV), None))


# ---- tiles ----------------------------------------------------------------------------------------------------------------
# 37 x 45; every W in 1..9 at H = 5 (the four-pixel quad, the image's border columns); H around the chunk height of 16
# rows; W around the chunk width of 256 columns (the halo pixel of lanes 0 and 63) and two chunks plus one column
TILE_SHAPES = ([(37, 45)] + [(5, w) for w in range(1, 10)] + [(h, 21) for h in (1, 2, 3, 15, 16, 17, 33)]
               + [(4, w) for w in (255, 256, 257, 513)])


@pytest.mark.parametrize("H,W", TILE_SHAPES)
def test_tiles_equal_the_restatement(H, W):
    rng = np.random.default_rng(H * 1000 + W)
    batch = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    batch[1] = np.minimum(batch[1], 240) // 2 + 100            # one sample with glass and little contrast
    want = Q.tiles(batch)
    if H < 3 or W < 3:
        assert (want["counts"][:, 1] == 0).all() and (want["focus"] == 0).all()
    for name, g, big in _both_layouts(batch):
        got = tile_qc(g)
        _check(got, want, (H, W, name))
        assert torch.equal(tile_qc(g)["counts"], got["counts"])                     # two identical runs
        for b in range(3):                                                          # alone and with batch mates
            assert torch.equal(tile_qc(g[b:b + 1])["counts"], got["counts"][b:b + 1]), (H, W, name, b)
        assert big is None or _guard_intact(big, batch)


def test_every_threshold_at_equality():
    thr = dict(white=200, black=30, ink_chroma=35, dark=70)
    px = [(199, 220, 210), (200, 220, 210),                    # mn = white - 1, white
          (29, 10, 5), (30, 10, 5),                            # mx = black - 1, black
          (50, 100, 66), (50, 100, 65), (66, 100, 50), (65, 100, 50),      # G - max(R, B) = 34, 35
          (50, 50, 84), (50, 50, 85), (50, 49, 85), (50, 49, 84),          # B - R = 34, 35 with G = R; G = R - 1
          (69, 40, 40), (70, 40, 40), (40, 40, 69), (40, 70, 40)]          # mx = dark - 1, dark
    flags = Q.pixel_maps(np.array([px], np.uint8), **thr)[0]
    assert flags[:, 0].tolist() == [1, 0, 0, 1] + [1] * 12
    assert flags[:, 5].tolist() == [0] * 4 + [0, 1, 0, 1] + [0] * 8
    assert flags[:, 6].tolist() == [0] * 8 + [0, 1, 0, 0] + [0] * 4
    assert flags[:, 7].tolist() == [0, 0, 0, 1] + [0] * 8 + [1, 0, 1, 0]
    rng = np.random.default_rng(8)
    tile = np.array(px, np.uint8)[rng.integers(0, len(px), (2, 19, 23))]
    tile[0, :2, :16] = np.array(px, np.uint8)                   # every crafted pixel at least once, on the border too
    for kw in (thr, dict(white=256, black=255, ink_chroma=1, dark=256), dict(white=1, black=0, ink_chroma=255, dark=0)):
        want = Q.tiles(tile, **kw)
        for name, g, big in _both_layouts(tile):
            _check(tile_qc(g, **kw), want, (kw, name))
    assert Q.tiles(tile, **thr)["counts"][:, 5:].min() > 0


@pytest.mark.parametrize("H,W", [(96, 96), (20, 1100)])
def test_checkerboard_needs_64_bit_sums(H, W):
    """L = +-1020 on every inner pixel: 96 x 96 passes 2^32 over six chunk rows, 20 x 1100 within one chunk row, and a
    single chunk of 16 x 256 holds 4.2e9 > 2^32 already: a 32-bit sum at wave, chunk or owner level shows."""
    yy, xx = np.mgrid[:H, :W]
    board = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[None, :, :, None], 3, -1)
    want = Q.tiles(board, white=256)
    assert want["counts"][0, 3] == (H - 2) * (W - 2) * 1020 ** 2 > 2 ** 32 and want["counts"][0, 0] == H * W
    for name, g, big in _both_layouts(board):
        _check(tile_qc(g, white=256), want, (H, W, name))
        assert big is None or _guard_intact(big, board)


# ---- regions ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _region():
    img = Q.synthetic_he(70, 90, seed=3)
    rng = np.random.default_rng(4)
    img[40:, 60:] = rng.integers(0, 256, (30, 30, 3), dtype=np.uint8)          # every class of pixel, across cell borders
    img[:20, 70:] = 245                                                        # glass
    img.setflags(write=False)
    return img


@pytest.mark.parametrize("cell", [32, 128])
def test_cell_map_equals_the_restatement_for_every_banding(cell):
    img = _region()
    want = Q.cell_map(img, cell)
    g, big = _view(img)
    got = region_qc_map(g, cell)
    assert tuple(got["counts"].shape) == (-(-70 // cell), -(-90 // cell), 8)
    _check(got, want, cell)
    assert region_qc_map.last_stats["bands"] == 1
    assert torch.equal(region_qc_map(g, cell)["counts"], got["counts"])            # two identical runs
    for band_rows in (1, 7, 70, None):
        _check(region_qc_map(g, cell, band_rows=band_rows), want, (cell, "gpu", band_rows))
        host = region_qc_map(_t(img), cell, band_rows=band_rows)
        assert host["counts"].is_cuda
        _check(host, want, (cell, "host", band_rows))
    assert region_qc_map.last_stats["bands"] == 1 and region_qc_map.last_stats["band_bytes"] == 70 * 90 * 3
    assert _guard_intact(big, img)
    # neighbours are taken across cell borders: the cells add up to the region scored as one tile
    whole = tile_qc(g[None])
    assert torch.equal(got["counts"].reshape(-1, 8).sum(0), whole["counts"][0])
    if cell == 32:
        sums = window_sums(got["counts"], win=2, stride=1)
        assert sums.is_cuda and np.array_equal(sums.cpu().numpy(), Q.window_sums(want["counts"], 2, 1))
        assert torch.equal(window_sums(got["counts"], win=3)[0, 0], whole["counts"][0])


@pytest.mark.parametrize("tile,overlap", [(32, 8), (128, 32)])
def test_plan_tiles_equal_the_restatement_for_every_banding(tile, overlap):
    img = _region()
    want = Q.region(img, tile, overlap)
    g, big = _view(img)
    got = region_qc(g, tile, overlap)
    assert tuple(got["counts"].shape) == (len(Q.plan(70, 90, tile, overlap)), 8)
    _check(got, want, tile)
    assert torch.equal(region_qc(g, tile, overlap)["counts"], got["counts"])
    for band_rows in (1, 7, 70, None):
        _check(region_qc(g, tile, overlap, band_rows=band_rows), want, (tile, "gpu", band_rows))
        _check(region_qc(_t(img), tile, overlap, band_rows=band_rows), want, (tile, "host", band_rows))
    _check(region_qc(_t(img).to(DEV), tile, overlap, white=200, black=20, ink_chroma=10, dark=120),
           Q.region(img, tile, overlap, white=200, black=20, ink_chroma=10, dark=120), (tile, "thresholds"))
    assert _guard_intact(big, img)


def test_windows_are_clipped_on_all_four_sides():
    """The entry points take any origins: windows that stick out of the image on every side, across two chunk columns,
    windows that miss it, and origins at the ends of int32."""
    from stain2stain_amd import ops
    rng = np.random.default_rng(12)
    wide = rng.integers(0, 256, (20, 300, 3), dtype=np.uint8)
    cases = ((_region(), 32, 40, [(-5, -7), (60, 80), (-20, 30), (10, -300), (50, -3), (-100, -100), (0, 0), (69, 89),
                                  (2 ** 31 - 40, 5), (-2 ** 31, -2 ** 31), (3, 2 ** 31 - 1)]),
             (wide, 24, 290, [(-3, -10), (5, 40), (-23, 299), (19, -289), (-8, -289), (20, 0)]))
    L = ops._L()
    for img, win_h, win_w, origins in cases:
        H, W = img.shape[:2]
        want = Q.windows(img, origins, win_h, win_w)
        assert (want["area"] == 0).any() and (want["area"] == 1).any() and want["counts"][:, 1].max() > 0
        n, nchunk = len(origins), L.s2s_qc_chunks(win_h, win_w)
        o = torch.tensor(origins, dtype=torch.int32, device=DEV)
        for name, g, big in _both_layouts(img):
            slab = torch.empty((n * nchunk, 8), dtype=torch.int64, device=DEV)
            counts = torch.empty((n, 8), dtype=torch.int64, device=DEV)
            derived = torch.empty((n, 5), dtype=torch.float64, device=DEV)
            assert L.s2s_qc_windows_u8(g.data_ptr(), g.stride(0), g.stride(0) * H, 1, 0, H, H, W, o.data_ptr(), n, win_h,
                                       win_w, 0, H, 220, 0, 40, 60, slab.data_ptr(), ops._stream()) == 0
            assert L.s2s_qc_finalize(slab.data_ptr(), n, nchunk, 0, o.data_ptr(), n, H, W, win_h, win_w,
                                     counts.data_ptr(), derived.data_ptr(), ops._stream()) == 0
            _check(dict({"counts": counts}, **{k: derived[:, i] for i, k in enumerate(DERIVED)}), want, (name, win_w))
            assert big is None or _guard_intact(big, img)


# ---- keep ---------------------------------------------------------------------------------------------------------------
def test_qc_keep_equals_the_restatement():
    img = _region()
    q = region_qc(_t(img).to(DEV), 32, 8)
    want = Q.region(img, 32, 8)
    for kw in ({}, {"min_focus": 4000.0}, {"min_focus_rel": 0.5}, {"min_focus_rel": 1.0, "min_tissue": 0.5},
               {"max_ink": 1.0, "max_dark": 0.05, "min_focus_rel": 0.9}):
        got = qc_keep(q, **kw)
        assert got.dtype == torch.bool and got.is_cuda and tuple(got.shape) == (12,)
        assert got.cpu().numpy().tolist() == Q.keep(want, **kw).tolist(), kw
    assert 0 < int(qc_keep(q, min_focus_rel=1.0).sum()) < 12
    m = region_qc_map(_t(img).to(DEV), 32)
    assert np.array_equal(qc_keep(m, min_focus_rel=0.5).cpu().numpy(), Q.keep(Q.cell_map(img, 32), min_focus_rel=0.5))
    glass = tile_qc(torch.full((2, 9, 9, 3), 250, dtype=torch.uint8, device=DEV))
    assert glass["counts"].tolist() == [[0] * 8] * 2 and glass["focus"].tolist() == [0.0, 0.0]
    assert qc_keep(glass, min_focus_rel=0.5).tolist() == [False, False]
    assert qc_keep(glass, min_focus_rel=0.5, min_tissue=0.0).tolist() == [True, True]     # the relative test drops nothing


@functools.lru_cache(maxsize=None)
def _slide():
    """64 x 96, tiles of 32 with overlap 8: 3 x 4 tiles at rows 0, 24, 32 and columns 0, 24, 48, 64.  Tile 0 is painted
    marker green where no other tile covers it; tile 3 (top right) is blurred over the 24 columns it shares least."""
    img = Q.synthetic_he(64, 96, seed=21)
    img[:24, :24] = (30, 150, 60)
    img[:32, 72:] = np.clip(np.round(Q.gaussian_blur(img[:32, 72:], 2.0)), 0, 255).astype(np.uint8)
    img.setflags(write=False)
    return img


def test_marked_and_blurred_tiles_skip_the_sampler():
    img = _slide()
    want = Q.keep(Q.region(img, 32, 8), min_focus_rel=0.5)
    assert want.tolist() == [False, True, True, False] + [True] * 8
    g, big = _view(img)
    q = region_qc(g, 32, 8)
    _check(q, Q.region(img, 32, 8), "slide")
    keep = qc_keep(q, min_focus_rel=0.5)
    assert keep.is_cuda and keep.cpu().numpy().tolist() == want.tolist()
    assert float(q["ink_frac"][0]) > 0.5 and float(q["ink_frac"][1:].max()) == 0.0
    out = translate_region(g, lambda x: x, tile=32, overlap=8, keep=keep)
    assert tuple(out.shape) == (64, 96, 3) and out.dtype == torch.uint8
    assert translate_region.last_stats["kept"] == 10 and translate_region.last_stats["skipped"] == 2
    got = out.cpu().numpy()
    assert np.array_equal(got[:24, :24], img[:24, :24])          # covered by tile 0 alone
    assert np.array_equal(got[:24, 80:], img[:24, 80:])          # covered by tile 3 alone
    assert _guard_intact(big, img)


# ---- no hidden synchronisation ------------------------------------------------------------------------------------------
def test_quality_control_does_not_synchronise():
    img = _region()
    g = _view(img)[0]
    batch = torch.stack([g[:32, :32], g[30:62, 40:72]])
    first = (tile_qc(batch), region_qc(g, 32, 8), region_qc_map(g, 32))       # the library is loaded from here on
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        t = tile_qc(batch)
        r = region_qc(g, 32, 8)
        rb = region_qc(g, 32, 8, band_rows=7)
        m = region_qc_map(g, 32, band_rows=16)
        keep = qc_keep(r, min_focus=100.0, min_focus_rel=0.5)
        keep_map = qc_keep(m, min_focus_rel=0.5)
        sums = window_sums(m["counts"], win=2, stride=1)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    for a, b in zip((t, r, m), first):
        assert torch.equal(a["counts"], b["counts"])
    assert torch.equal(rb["counts"], r["counts"])
    assert keep.cpu().numpy().tolist() == Q.keep(Q.region(img, 32, 8), min_focus=100.0, min_focus_rel=0.5).tolist()
    assert tuple(keep_map.shape) == (3, 3) and tuple(sums.shape) == (2, 2, 8)
