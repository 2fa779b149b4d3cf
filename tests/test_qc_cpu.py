"""Tile quality control (stain2stain_amd/qc.py, csrc/qc.hip) without a GPU: the boundary (exports, the
source list, the declared symbols, status codes, the wrappers' errors), ``window_sums`` against brute force, and the
properties of the numpy restatement in tests/qc_ref.py that the GPU tests compare the kernels with."""
import ctypes

import numpy as np
import pytest
import torch

import qc_ref as Q
import stain2stain_amd
from stain2stain_amd import _native, qc


# ---- the boundary ------------------------------------------------------------------------------------------------------
def test_names_are_exported_and_the_source_is_built():
    for name in ("tile_qc", "region_qc", "region_qc_map", "qc_keep", "window_sums"):
        assert name in stain2stain_amd.__all__ and getattr(stain2stain_amd, name) is getattr(qc, name), name
    assert "qc.hip" in _native.SOURCES
    assert {"s2s_qc_windows_u8", "s2s_qc_finalize", "s2s_qc_chunks"} <= set(_native.declared_symbols())
    assert qc.COUNT_KEYS == Q.KEYS
    defaults = (220, 0, qc.DEFAULT_INK_CHROMA, qc.DEFAULT_DARK)
    assert defaults == tuple(Q.DEFAULTS[k] for k in ("white", "black", "ink_chroma", "dark"))


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _native.lib()
    ok = ctypes.c_void_p(4096)

    def win(img=ok, origins=ok, slab=ok, pitch=300, stride=300 * 70, B=1, band_top=0, band_h=70, H=70, W=100, n=6,
            win_h=32, win_w=32, row0=0, row1=70, white=220, black=0, ink=40, dark=60):
        return lib.s2s_qc_windows_u8(img, pitch, stride, B, band_top, band_h, H, W, origins, n, win_h, win_w, row0, row1,
                                     white, black, ink, dark, slab, None)

    assert win(img=None) == -5 and win(origins=None) == -5 and win(slab=None) == -5
    assert win(B=0) == -1 and win(B=65536) == -1 and win(n=0) == -1
    assert win(H=0, band_h=1, row1=1) == -1 and win(W=0) == -1 and win(win_h=0) == -1 and win(win_w=0) == -1
    assert win(win_h=(1 << 30) + 1) == -1 and win(H=(1 << 30) + 1) == -1
    assert win(pitch=299) == -1 and win(B=2, stride=300 * 70 - 1) == -1
    # thresholds at one past either end of their ranges
    assert win(white=0) == -1 and win(white=257) == -1 and win(black=-1) == -1 and win(black=256) == -1
    assert win(ink=0) == -1 and win(ink=256) == -1 and win(dark=-1) == -1 and win(dark=257) == -1
    # the rows of the launch, and the rows present: [row0 - 1, row1] where they exist
    assert win(row0=-1) == -1 and win(row0=10, row1=10) == -1 and win(row1=71) == -1
    assert win(band_top=-1) == -1 and win(band_h=0) == -1 and win(band_h=71) == -1
    assert win(row0=20, row1=30, band_top=20, band_h=11) == -1            # needs row 19
    assert win(row0=20, row1=30, band_top=19, band_h=11) == -1            # needs row 30
    assert win(row0=0, row1=30, band_top=0, band_h=30) == -1 and win(row0=20, row1=70, band_top=20, band_h=50) == -1
    assert win(n=1 << 30, win_h=1 << 20, win_w=1 << 20) == -1             # more chunks than a grid holds

    def fin(slab=ok, origins=ok, counts=ok, derived=ok, owners=6, nchunk=2, accumulate=0, n=3, H=70, W=100, win_h=32,
            win_w=32):
        return lib.s2s_qc_finalize(slab, owners, nchunk, accumulate, origins, n, H, W, win_h, win_w, counts, derived, None)

    for k in ("slab", "origins", "counts", "derived"):
        assert fin(**{k: None}) == -5, k
    assert fin(owners=0) == -1 and fin(owners=1 << 31) == -1 and fin(nchunk=0) == -1
    assert fin(n=0) == -1 and fin(n=4) == -1                              # owners = samples x windows
    assert fin(H=0) == -1 and fin(W=0) == -1 and fin(win_h=0) == -1 and fin(win_w=(1 << 30) + 1) == -1
    assert lib.s2s_qc_chunks(0, 5) == -1 and lib.s2s_qc_chunks(5, (1 << 30) + 1) == -1
    assert lib.s2s_qc_chunks(1, 1) == 1 and lib.s2s_qc_chunks(qc.CHUNK_ROWS, 256) == 1
    assert lib.s2s_qc_chunks(qc.CHUNK_ROWS + 1, 257) == 4 and lib.s2s_qc_chunks(256, 256) == 16


def test_wrappers_refuse_bad_arguments():
    tiles = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    region = torch.zeros((8, 8, 3), dtype=torch.uint8)
    with pytest.raises(TypeError, match="tile_qc: tiles must be a torch.Tensor"):
        qc.tile_qc(np.zeros((1, 8, 8, 3), np.uint8))
    with pytest.raises(ValueError, match="tile_qc: tiles must be uint8"):
        qc.tile_qc(tiles.float())
    with pytest.raises(ValueError, match=r"\[B, H, W, 3\]"):
        qc.tile_qc(region)
    with pytest.raises(ValueError, match=r"\[B, H, W, 3\]"):
        qc.tile_qc(tiles[:0])
    with pytest.raises(RuntimeError, match="tile_qc needs GPU tensors"):
        qc.tile_qc(tiles)
    for kw, msg in (({"white": 0}, "white must lie in 1..256"), ({"black": 256}, "black must lie in 0..255"),
                    ({"ink_chroma": 0}, "ink_chroma must lie in 1..255"), ({"ink_chroma": 256}, "ink_chroma must lie"),
                    ({"dark": -1}, "dark must lie in 0..256"), ({"dark": 257}, "dark must lie in 0..256")):
        for call in (lambda: qc.tile_qc(tiles, **kw), lambda: qc.region_qc(region, 4, 1, **kw),
                     lambda: qc.region_qc_map(region, 4, **kw)):
            with pytest.raises(ValueError, match=msg):
                call()
    with pytest.raises(TypeError):
        qc.tile_qc(tiles, ink_chroma=40.0)
    with pytest.raises(TypeError, match="region_qc: the region must be a torch.Tensor"):
        qc.region_qc(None)
    with pytest.raises(ValueError, match="region_qc: the region must be uint8"):
        qc.region_qc(region.float())
    with pytest.raises(ValueError, match=r"region_qc_map: the region must be a non-empty \[H, W, 3\]"):
        qc.region_qc_map(tiles)
    with pytest.raises(ValueError, match="pixels within a row must be contiguous"):
        qc.region_qc_map(torch.zeros((8, 16, 3), dtype=torch.uint8)[:, ::2])
    with pytest.raises(ValueError, match="overlap must lie in"):
        qc.region_qc(region, 4, 4)
    with pytest.raises(ValueError, match="cell must be positive"):
        qc.region_qc_map(region, 0)
    with pytest.raises(ValueError, match="band_rows must be at least 1"):
        qc.plan_qc_bands(8, 0)
    assert qc.plan_qc_bands(8) == [(0, 8)] and qc.plan_qc_bands(8, 3) == [(0, 3), (3, 6), (6, 8)]
    assert qc.plan_qc_bands(8, 100) == [(0, 8)]


def test_qc_keep_and_window_sums_refuse_bad_arguments():
    q = {k: torch.zeros(3, dtype=torch.float64) for k in ("focus", "tissue_frac", "ink_frac", "dark_frac")}
    with pytest.raises(TypeError, match="qc_keep: q must be the dict"):
        qc.qc_keep(torch.zeros(3))
    with pytest.raises(TypeError, match="qc_keep: q must be the dict"):
        qc.qc_keep({"focus": q["focus"]})
    for kw in ({"min_tissue": -0.1}, {"max_ink": 1.5}, {"max_dark": float("nan")}):
        with pytest.raises(ValueError, match=r"must lie in \[0, 1\]"):
            qc.qc_keep(q, **kw)
    for kw in ({"min_focus": -1.0}, {"min_focus_rel": float("nan")}):
        with pytest.raises(ValueError, match="must be None or a number >= 0"):
            qc.qc_keep(q, **kw)
    m = torch.zeros((3, 4, 8), dtype=torch.int64)
    with pytest.raises(TypeError, match="window_sums: counts must be a torch.Tensor"):
        qc.window_sums(m.numpy())
    with pytest.raises(ValueError, match="non-empty int64"):
        qc.window_sums(m.int())
    with pytest.raises(ValueError, match="non-empty int64"):
        qc.window_sums(m[0, 0])
    with pytest.raises(ValueError, match="win must lie in 1..3"):
        qc.window_sums(m, win=4)
    with pytest.raises(ValueError, match="win must lie in 1..3"):
        qc.window_sums(m, win=0)
    with pytest.raises(ValueError, match="stride must be at least 1"):
        qc.window_sums(m, stride=0)


# ---- plain torch: window_sums and qc_keep run on the host too -----------------------------------------------------------
def test_window_sums_equal_brute_force():
    rng = np.random.default_rng(3)
    for shape in ((5, 7, 8), (4, 4, 8), (1, 6), (3, 5, 2, 2)):
        m = rng.integers(-2 ** 40, 2 ** 40, shape)
        G = min(shape[:2])
        for win, stride in {(1, 1), (min(2, G), 1), (min(2, G), 2), (min(3, G), 2), (G, 1), (G, 3), (1, 4)}:
            got = qc.window_sums(torch.from_numpy(m), win=win, stride=stride)
            want = Q.window_sums(m, win, stride)
            assert got.dtype == torch.int64 and tuple(got.shape) == want.shape, (shape, win, stride)
            assert np.array_equal(got.numpy(), want), (shape, win, stride)
    m = rng.integers(0, 100, (4, 4, 8))
    assert np.array_equal(qc.window_sums(torch.from_numpy(m), win=4).numpy()[0, 0], m.reshape(16, 8).sum(0))


def test_qc_keep_equals_the_restatement_on_the_host():
    rng = np.random.default_rng(5)
    for n, glass in ((1, 0.0), (6, 0.3), (7, 0.5), (12, 1.0)):
        q = {"focus": rng.uniform(0, 100, n), "tissue_frac": np.where(rng.random(n) < glass, 0.0, rng.uniform(0, 1, n)),
             "ink_frac": rng.uniform(0, 0.02, n), "dark_frac": rng.uniform(0, 1, n)}
        tq = {k: torch.from_numpy(v) for k, v in q.items()}
        for kw in ({}, {"min_focus": 30.0}, {"min_focus_rel": 0.5}, {"min_focus_rel": 1.0, "min_tissue": 0.5},
                   {"min_focus": 10.0, "min_focus_rel": 2.0, "max_ink": 1.0, "max_dark": 1.0}):
            got = qc.qc_keep(tq, **kw)
            assert got.dtype == torch.bool and np.array_equal(got.numpy(), Q.keep(q, **kw)), (n, glass, kw)
    # no tile passes the tissue test: the relative test drops nothing (and nothing is kept anyway)
    none = {k: torch.zeros(4, dtype=torch.float64) for k in ("focus", "tissue_frac", "ink_frac", "dark_frac")}
    assert not qc.qc_keep(none, min_focus_rel=0.5).any()
    assert qc.qc_keep(none, min_focus_rel=0.5, min_tissue=0.0).all()


# ---- the restatement's own properties ------------------------------------------------------------------------------------
def test_hand_computed_pixels():
    img = np.full((3, 3, 3), 100, np.uint8)
    img[1, 1] = (200, 10, 30)                                   # Y = (15400 + 1500 + 870 + 128) >> 8 = 69
    m = Q.pixel_maps(img)
    assert Q.luma(img)[1, 1] == 69 and Q.luma(img)[0, 0] == 100
    assert m[1, 1].tolist() == [1, 1, 124, 124 * 124, 69, 0, 0, 0]
    assert m[..., 1].sum() == 1 and m[0, 1].tolist() == [1, 0, 0, 0, 100, 0, 0, 0]
    px = np.array([[[10, 60, 20], [10, 59, 20], [10, 10, 50], [10, 9, 50], [10, 10, 49], [59, 0, 0], [60, 0, 0],
                    [219, 230, 240], [220, 230, 240]]], np.uint8)
    m = Q.pixel_maps(px)[0]
    assert m[:, 5].tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 0]      # green: G - max(R, B) >= 40
    assert m[:, 6].tolist() == [0, 0, 1, 0, 0, 0, 0, 0, 0]      # blue: B - R >= 40 and G >= R
    assert m[:, 7].tolist() == [0, 1, 1, 1, 1, 1, 0, 0, 0]      # dark: mx < 60
    assert m[:, 0].tolist() == [1, 1, 1, 1, 1, 1, 1, 1, 0]      # tissue: mn < 220
    assert Q.pixel_maps(px, black=60)[0][:, 0].tolist() == [1, 0, 0, 0, 0, 0, 1, 1, 0]


def test_cell_counts_add_up_to_the_image():
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (70, 90, 3), dtype=np.uint8)
    whole = Q.tiles(img[None])
    assert whole["counts"][0, 1] > 0 and whole["area"].tolist() == [6300]
    for cell in (32, 17, 128):
        m = Q.cell_map(img, cell)
        assert np.array_equal(m["counts"].reshape(-1, 8).sum(0), whole["counts"][0]), cell
        assert m["area"].sum() == 6300
    m = Q.cell_map(img, 32)
    assert np.array_equal(Q.window_sums(m["counts"], 3, 1)[0, 0], whole["counts"][0])
    # focus pixels are those of the image: cutting a cell out and scoring it alone loses its border
    alone = Q.tiles(img[None, :32, :32])["counts"][0]
    assert alone[0] == m["counts"][0, 0, 0] and alone[1] < m["counts"][0, 0, 1]
    # a plan tile larger than the region is the region
    assert np.array_equal(Q.region(img, 128, 32)["counts"], whole["counts"])
    assert len(Q.plan(70, 90, 32, 8)) == 12 and Q.plan(70, 90, 32, 8)[-1] == (38, 58)


def test_no_stain_mixture_is_ink():
    colours = Q.stain_palette(200_000, seed=2001)
    m = Q.pixel_maps(colours[None], white=256)
    assert m[..., 0].sum() == 200_000
    assert int(m[..., 5].sum()) == 0 and int(m[..., 6].sum()) == 0
    marker = np.array([[[20, 140, 40], [30, 60, 160], [25, 25, 30]]], np.uint8)     # green, blue, black marker
    m = Q.pixel_maps(marker)[0]
    assert m[:, 5].tolist() == [1, 0, 0] and m[:, 6].tolist() == [0, 1, 0] and m[:, 7].tolist() == [0, 0, 1]


def test_focus_falls_with_blur():
    focus = []
    for sigma in (0.0, 1.0, 2.0, 4.0):
        tile = Q.synthetic_he(96, 96, seed=11, sigma=sigma)
        q = Q.tiles(tile[None])
        assert q["tissue_frac"][0] > 0.9 and q["ink_frac"][0] == 0.0
        focus.append(float(q["focus"][0]))
    print("focus over blur sigma 0, 1, 2, 4:", [round(f, 1) for f in focus])
    assert all(a > b for a, b in zip(focus, focus[1:])), focus
    assert focus[0] > 10 * focus[1]
