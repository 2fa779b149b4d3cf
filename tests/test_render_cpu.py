"""Result rendering (stain2stain_amd/render.py, csrc/render.hip) without a GPU: the boundary (exports,
the source list, the declared symbols, the status codes of every entry point before any HIP call, the wrappers' errors),
the palette and colour maps, and the properties of the numpy restatement in tests/render_ref.py that the GPU tests
compare the kernels with."""
import ctypes

import numpy as np
import pytest
import torch

import morphology_ref
import render_ref as R
import stain2stain_amd
from stain2stain_amd import _native, render

NAMES = ("render_classes", "render_heat", "compare_regions", "downsample_region", "render_region", "compose_panels",
         "default_palette", "colormap")
SYMBOLS = {"s2s_render_classes_u8", "s2s_render_labels_u8", "s2s_render_heat_u8", "s2s_render_compare_u8",
           "s2s_box_down_u8"}
NULL, SHAPE = -5, -1


# ---- the boundary ------------------------------------------------------------------------------------------------------
def test_names_are_exported_and_the_source_is_built():
    for name in NAMES:
        assert name in stain2stain_amd.__all__ and getattr(stain2stain_amd, name) is getattr(render, name), name
    assert "render.hip" in _native.SOURCES
    assert SYMBOLS <= set(_native.declared_symbols())
    assert render.QMAX == R.QMAX == 255 * 256


def test_palette_and_colour_maps_equal_the_restatement():
    pal = render.default_palette()
    assert pal.dtype == torch.uint8 and tuple(pal.shape) == (256, 3) and not pal.is_cuda
    assert np.array_equal(pal.numpy(), R.palette())
    assert pal[0].tolist() == [0, 0, 0] and pal[1].tolist() == [230, 25, 75] and pal[8].tolist() == [240, 50, 230]
    assert pal[9].tolist() == pal[1].tolist() and pal[255].tolist() == list(R.PALETTE8[254 % 8])
    for name, anchors in R.ANCHORS.items():
        lut = render.colormap(name)
        assert lut.dtype == torch.uint8 and tuple(lut.shape) == (256, 3)
        assert np.array_equal(lut.numpy(), R.colormap(name)), name
        for i, c in anchors:                                    # the maps hit their anchors
            assert lut[i].tolist() == list(c), (name, i)
    assert render.colormap("gray")[:, 0].tolist() == list(range(256))
    assert render.colormap("heat")[42].tolist() == [126, 0, 0]          # (255 * 42 + 42) // 85
    with pytest.raises(ValueError, match="colormap: name must be one of"):
        render.colormap("jet")


@pytest.mark.parametrize("labels", [False, True])
def test_class_entry_points_refuse_bad_arguments_without_a_gpu(labels):
    lib = _native.lib()
    ok = ctypes.c_void_p(4096)
    fn = lib.s2s_render_labels_u8 if labels else lib.s2s_render_classes_u8
    mrow = 400 if labels else 100

    def call(base=ok, mask=ok, pal=ok, fa=ok, out=ok, bpitch=300, mpitch=None, m0=0, mrows=70, r=1, ea=256, rgb=-1, H=70,
             W=100, row0=0, rows=70, opitch=300):
        return fn(base, bpitch, mask, mrow if mpitch is None else mpitch, m0, mrows, pal, fa, r, ea, rgb, H, W, row0, rows,
                  out, opitch, None)

    for k in ("base", "mask", "pal", "fa", "out"):
        assert call(**{k: None}) == NULL, k
    assert call(H=0, rows=0) == SHAPE and call(W=0) == SHAPE
    assert call(H=(1 << 30) + 1) == SHAPE and call(W=(1 << 30) + 1, bpitch=1 << 40, opitch=1 << 40, mpitch=1 << 40) == SHAPE
    assert call(r=-1) == SHAPE and call(r=5) == SHAPE and call(ea=-1) == SHAPE and call(ea=257) == SHAPE
    assert call(rgb=-2) == SHAPE and call(rgb=1 << 24) == SHAPE
    assert call(bpitch=299) == SHAPE and call(opitch=299) == SHAPE and call(mpitch=mrow - 1) == SHAPE
    if labels:
        assert call(mpitch=402) == SHAPE                                   # label rows are whole dwords
    # rows outside the region
    assert call(row0=-1) == SHAPE and call(rows=0) == SHAPE and call(rows=71) == SHAPE and call(row0=70, rows=1) == SHAPE
    assert call(m0=-1) == SHAPE and call(mrows=0) == SHAPE and call(mrows=71) == SHAPE
    # the mask rows present must cover [row0 - r, row0 + rows + r) where the region has them
    band = dict(row0=20, rows=10, r=2)
    assert call(m0=19, mrows=13, **band) == SHAPE                          # misses row 18
    assert call(m0=18, mrows=13, **band) == SHAPE                          # misses row 31
    assert call(m0=20, mrows=10, r=1, row0=20, rows=10) == SHAPE
    assert call(row0=0, rows=30, m0=0, mrows=30) == SHAPE and call(row0=40, rows=30, m0=40, mrows=30) == SHAPE


def test_heat_entry_point_refuses_bad_arguments_without_a_gpu():
    lib = _native.lib()
    ok = ctypes.c_void_p(4096)

    def call(base=ok, Q=ok, lut=ok, out=ok, bpitch=300, Gy=3, Gx=4, cell=32, alpha=128, mi=0, smooth=1, H=70, W=100, row0=0,
             rows=70, opitch=300):
        return lib.s2s_render_heat_u8(base, bpitch, Q, Gy, Gx, cell, lut, alpha, mi, smooth, H, W, row0, rows, out, opitch,
                                      None)

    for k in ("base", "Q", "lut", "out"):
        assert call(**{k: None}) == NULL, k
    assert call(H=0, rows=0) == SHAPE and call(W=0) == SHAPE and call(H=(1 << 30) + 1) == SHAPE
    assert call(W=(1 << 30) + 1, bpitch=1 << 40, opitch=1 << 40) == SHAPE
    assert call(cell=0) == SHAPE and call(cell=(1 << 14) + 1, Gy=1, Gx=1) == SHAPE
    assert call(alpha=-1) == SHAPE and call(alpha=257) == SHAPE and call(mi=-1) == SHAPE and call(mi=257) == SHAPE
    assert call(smooth=-1) == SHAPE and call(smooth=2) == SHAPE
    assert call(bpitch=299) == SHAPE and call(opitch=299) == SHAPE
    assert call(row0=-1) == SHAPE and call(rows=0) == SHAPE and call(rows=71) == SHAPE and call(row0=70, rows=1) == SHAPE
    # 70 x 100 at cell 32: Gy in {2, 3}, Gx in {3, 4}
    assert call(Gy=1) == SHAPE and call(Gy=4) == SHAPE and call(Gx=2) == SHAPE and call(Gx=5) == SHAPE
    assert call(Gy=0, cell=128, Gx=1) == SHAPE                            # H // cell = 0 is no grid
    assert call(H=1 << 20, W=1 << 20, cell=1 << 11, Gy=512, Gx=512, rows=1, bpitch=1 << 22, opitch=1 << 22) == SHAPE


def test_compare_entry_point_refuses_bad_arguments_without_a_gpu():
    lib = _native.lib()
    ok = ctypes.c_void_p(4096)

    def call(a=ok, b=ok, out=ok, ap=300, bp=300, mode=0, cell=64, alpha=128, gain=4, H=70, W=100, row0=0, rows=70, op=300):
        return lib.s2s_render_compare_u8(a, ap, b, bp, mode, cell, alpha, gain, H, W, row0, rows, out, op, None)

    for k in ("a", "b", "out"):
        assert call(**{k: None}) == NULL, k
    assert call(H=0, rows=0) == SHAPE and call(W=0) == SHAPE and call(H=(1 << 30) + 1) == SHAPE
    assert call(W=(1 << 30) + 1, ap=1 << 40, bp=1 << 40, op=1 << 40) == SHAPE
    assert call(mode=-1) == SHAPE and call(mode=3) == SHAPE and call(cell=0) == SHAPE and call(cell=(1 << 30) + 1) == SHAPE
    assert call(alpha=-1) == SHAPE and call(alpha=257) == SHAPE and call(gain=0) == SHAPE and call(gain=256) == SHAPE
    assert call(ap=299) == SHAPE and call(bp=299) == SHAPE and call(op=299) == SHAPE
    assert call(row0=-1) == SHAPE and call(rows=0) == SHAPE and call(rows=71) == SHAPE and call(row0=70, rows=1) == SHAPE


def test_thumbnail_entry_point_refuses_bad_arguments_without_a_gpu():
    lib = _native.lib()
    ok = ctypes.c_void_p(4096)

    def call(src=ok, out=ok, sp=300, s0=0, srows=70, H=70, W=100, C=3, f=16, row0=0, rows=5, op=21):
        return lib.s2s_box_down_u8(src, sp, s0, srows, H, W, C, f, row0, rows, out, op, None)

    assert call(src=None) == NULL and call(out=None) == NULL
    assert call(C=0) == SHAPE and call(C=2) == SHAPE and call(C=4) == SHAPE
    assert call(H=0, srows=0) == SHAPE and call(W=0) == SHAPE and call(H=(1 << 30) + 1) == SHAPE
    assert call(W=(1 << 30) + 1, sp=1 << 40, op=1 << 40) == SHAPE
    assert call(f=0) == SHAPE and call(f=257, rows=1) == SHAPE
    assert call(sp=299) == SHAPE and call(op=20) == SHAPE and call(C=1, sp=99, op=7) == SHAPE and call(C=1, sp=100, op=6) == SHAPE
    # output rows outside the ceil(70 / 16) = 5 rows of the result
    assert call(row0=-1) == SHAPE and call(rows=0) == SHAPE and call(rows=6) == SHAPE and call(row0=5, rows=1) == SHAPE
    assert call(s0=-1) == SHAPE and call(srows=0) == SHAPE and call(srows=71) == SHAPE
    # output rows [1, 3) read input rows [16, 48)
    assert call(row0=1, rows=2, s0=17, srows=40) == SHAPE and call(row0=1, rows=2, s0=16, srows=31) == SHAPE
    assert call(row0=4, rows=1, s0=64, srows=5) == SHAPE                   # the ragged last block ends at row 70


def test_wrappers_refuse_bad_arguments():
    region = torch.zeros((8, 12, 3), dtype=torch.uint8)
    mask = torch.zeros((8, 12), dtype=torch.uint8)
    vals = torch.zeros((2, 3))
    with pytest.raises(TypeError, match="render_classes: the region must be a torch.Tensor"):
        render.render_classes(np.zeros((8, 12, 3), np.uint8), mask)
    with pytest.raises(ValueError, match="render_classes: the region must be uint8"):
        render.render_classes(region.float(), mask)
    with pytest.raises(ValueError, match=r"render_classes: the region must be a non-empty \[H, W, 3\]"):
        render.render_classes(mask, mask)
    with pytest.raises(TypeError, match="render_classes: the mask must be a torch.Tensor"):
        render.render_classes(region, None)
    with pytest.raises(ValueError, match="render_classes: the mask must be uint8 or bool classes or int32 labels"):
        render.render_classes(region, mask.long())
    with pytest.raises(ValueError, match=r"render_classes: the mask must be \[8, 12\]"):
        render.render_classes(region, mask[:, :11])
    with pytest.raises(ValueError, match="render_classes: the mask's pixels within a row must be contiguous"):
        render.render_classes(region, torch.zeros((8, 24), dtype=torch.uint8)[:, ::2])
    for kw, msg in (({"alpha": -1}, "alpha must lie in 0..256"), ({"alpha": 257}, "alpha must lie in 0..256"),
                    ({"outline": -1}, "outline must lie in 0..4"), ({"outline": 5}, "outline must lie in 0..4"),
                    ({"outline_alpha": 257}, "outline_alpha must lie in 0..256"),
                    ({"outline_rgb": (0, 0, 256)}, "outline_rgb must be three integers"),
                    ({"outline_rgb": (0, 0)}, "outline_rgb must be three integers"),
                    ({"band_rows": 0}, "band_rows must be positive")):
        with pytest.raises(ValueError, match="render_classes: " + msg):
            render.render_classes(region, mask, **kw)
    with pytest.raises(TypeError):
        render.render_classes(region, mask, alpha=96.0)
    with pytest.raises(TypeError, match="render_classes: out must be a torch.Tensor"):
        render.render_classes(region, mask, out=0)
    with pytest.raises(ValueError, match="render_classes: out must be uint8"):
        render.render_classes(region, mask, out=torch.zeros((8, 11, 3), dtype=torch.uint8))
    big = torch.zeros((9, 12, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="render_classes: out may be the region itself but must not overlap it in part"):
        render.render_classes(big[:8], mask, out=big[1:])
    # everything about the tables is checked before the device is asked for
    for call in (lambda: render.render_classes(region, mask), lambda: render.render_heat(region, vals, 4),
                 lambda: render.compare_regions(region, region), lambda: render.downsample_region(region, 2)):
        if not torch.cuda.is_available():
            with pytest.raises(RuntimeError, match="needs a GPU"):
                call()

    with pytest.raises(TypeError, match="render_heat: values must be a torch.Tensor"):
        render.render_heat(region, [[0.0]], 4)
    with pytest.raises(ValueError, match=r"render_heat: values must be a real or integer \[Gy, Gx\] map"):
        render.render_heat(region, torch.zeros(3), 4)
    with pytest.raises(ValueError, match="render_heat: values must be a real or integer"):
        render.render_heat(region, torch.zeros((2, 3), dtype=torch.bool), 4)
    with pytest.raises(ValueError, match="render_heat: cell must lie in 1..16384"):
        render.render_heat(region, vals, 0)
    with pytest.raises(ValueError, match="render_heat: cell must lie in 1..16384"):
        render.render_heat(region, torch.zeros((1, 1)), (1 << 14) + 1)
    with pytest.raises(ValueError, match=r"render_heat: Gy must be 8 // 4 or ceil\(8 / 4\)"):
        render.render_heat(region, torch.zeros((3, 3)), 4)
    with pytest.raises(ValueError, match=r"render_heat: Gx must be 12 // 5 or ceil\(12 / 5\)"):
        render.render_heat(region, torch.zeros((2, 4)), 5)
    with pytest.raises(ValueError, match="render_heat: Gy must be"):
        render.render_heat(region, torch.zeros((0, 1)), 16)
    for kw, msg in (({"hi": 0.0}, "hi must be a finite number above lo"), ({"lo": 2.0}, "hi must be a finite number above"),
                    ({"hi": float("nan")}, "hi must be a finite number above lo"),
                    ({"alpha": 257}, "alpha must lie in 0..256"), ({"min_index": -1}, "min_index must lie in 0..256"),
                    ({"min_index": 257}, "min_index must lie in 0..256"), ({"lut": "jet"}, "name must be one of"),
                    ({"lut": torch.zeros((255, 3), dtype=torch.uint8)}, r"lut must be uint8 \[256, 3\]"),
                    ({"quantized": True}, "a quantized map must be int32")):
        with pytest.raises(ValueError, match=msg):
            render.render_heat(region, vals, 4, **kw)

    with pytest.raises(ValueError, match="compare_regions: the regions must have one shape"):
        render.compare_regions(region, region[:7])
    with pytest.raises(TypeError, match="compare_regions: the region must be a torch.Tensor"):
        render.compare_regions(region, None)
    for kw, msg in (({"mode": "xor"}, "mode must be one of"), ({"cell": 0}, "cell must lie in 1.."),
                    ({"alpha": -1}, "alpha must lie in 0..256"), ({"gain": 0}, "gain must lie in 1..255"),
                    ({"gain": 256}, "gain must lie in 1..255")):
        with pytest.raises(ValueError, match="compare_regions: " + msg):
            render.compare_regions(region, region, **kw)

    with pytest.raises(ValueError, match="downsample_region: factor must lie in 1..256"):
        render.downsample_region(region, 0)
    with pytest.raises(ValueError, match="downsample_region: factor must lie in 1..256"):
        render.downsample_region(mask, 257)
    with pytest.raises(TypeError):
        render.downsample_region(region, 2.0)
    with pytest.raises(ValueError, match="downsample_region: the region must be a non-empty"):
        render.downsample_region(torch.zeros((2, 8, 12, 3), dtype=torch.uint8), 2)

    with pytest.raises(ValueError, match="render_region: at least one layer"):
        render.render_region(region, [])
    with pytest.raises(ValueError, match="render_region: layer 0 must be"):
        render.render_region(region, [("glyphs", mask)])
    with pytest.raises(ValueError, match=r"render_region: layer 0 \('heat'\) takes 2 argument"):
        render.render_region(region, [("heat", vals)])
    with pytest.raises(ValueError, match="render_region: layer 0 must not set out or band_rows"):
        render.render_region(region, [("classes", mask, {"out": region})])
    with pytest.raises(ValueError, match="render_classes: outline must lie in 0..4"):
        render.render_region(region, [("classes", mask, {"outline": 9})])


def test_compose_panels_runs_on_the_host_and_equals_the_restatement():
    rng = np.random.default_rng(2)
    for shape in ((5, 7, 3), (4, 6)):
        ims = [rng.integers(0, 256, shape, dtype=np.uint8) for _ in range(5)]
        for kw in ({}, {"cols": 2}, {"cols": 3, "gap": 0, "fill": 7}, {"cols": 9, "gap": 1}, {"cols": 1, "gap": 2, "fill": 0}):
            got = render.compose_panels([torch.from_numpy(i) for i in ims], **kw)
            assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), R.compose(ims, **kw)), (shape, kw)
    three = render.compose_panels([torch.zeros((4, 5, 3), dtype=torch.uint8)] * 3)
    assert tuple(three.shape) == (4, 3 * 5 + 2 * 8, 3) and int(three[0, 5, 0]) == 255
    with pytest.raises(ValueError, match="compose_panels: at least one image"):
        render.compose_panels([])
    with pytest.raises(TypeError, match="compose_panels: every image must be a torch.Tensor"):
        render.compose_panels([np.zeros((4, 4, 3), np.uint8)])
    with pytest.raises(ValueError, match="compose_panels: the images must share"):
        render.compose_panels([torch.zeros((4, 4, 3), dtype=torch.uint8), torch.zeros((4, 5, 3), dtype=torch.uint8)])
    with pytest.raises(ValueError, match="compose_panels: an image must be a non-empty uint8"):
        render.compose_panels([torch.zeros((4, 4, 3))])
    with pytest.raises(ValueError, match="compose_panels: fill must lie in 0..255"):
        render.compose_panels([torch.zeros((4, 4, 3), dtype=torch.uint8)], fill=256)


def test_quantisation_equals_the_restatement_on_the_host():
    step = 1.5 / R.QMAX
    v = np.array([[0.25 + step * k for k in (0, 1, 2, 32640, 65279, 65280)],
                  [np.nan, -1.0, 0.25 - step, 1.75 + step, np.inf, -np.inf]])
    got = render.quantize_map(torch.from_numpy(v), 0.25, 1.75)
    want = R.quantize(v, 0.25, 1.75)
    assert got.dtype == torch.int32 and np.array_equal(got.numpy(), want)
    assert want[0].tolist() == [0, 1, 2, 32640, 65279, 65280] and want[1].tolist() == [0, 0, 0, 65280, 65280, 0]
    counts = np.arange(12, dtype=np.int64).reshape(3, 4) * 1000
    assert np.array_equal(render.quantize_map(torch.from_numpy(counts), 0, 11000).numpy(), R.quantize(counts, 0, 11000))


# ---- the restatement's own properties ------------------------------------------------------------------------------------
def test_mix_returns_its_ends_exactly():
    b, c = np.meshgrid(np.arange(256), np.arange(256))
    assert np.array_equal(R.mix(b, c, 0), b) and np.array_equal(R.mix(b, c, 256), c)
    assert R.mix(10, 20, 128) == 15 and R.mix(0, 255, 128) == 128 and R.mix(255, 0, 1) == 254
    assert R.mix(b, c, 77).min() >= 0 and R.mix(b, c, 77).max() <= 255


def test_alpha_ends_of_the_class_overlay():
    base = R.random_region(20, 23, 1)
    rng = np.random.default_rng(1)
    mask = rng.integers(0, 4, (20, 23)).astype(np.uint8)
    assert np.array_equal(R.render_classes(base, mask, alpha=0, r=0), base)
    assert np.array_equal(R.render_classes(base, mask, alpha=0, r=2, edge_alpha=0), base)
    full = R.render_classes(base, mask, alpha=256, r=0)
    assert np.array_equal(full[mask > 0], R.palette()[mask[mask > 0]]) and np.array_equal(full[mask == 0], base[mask == 0])
    # background pixels are copied unchanged whatever the outline does
    assert np.array_equal(R.render_classes(base, mask, r=4)[mask == 0], base[mask == 0])
    fixed = R.render_classes(base, mask, r=1, edge_rgb=(1, 2, 3))
    assert (fixed[R.edges(mask, 1)] == (1, 2, 3)).all()


def test_outline_one_on_a_binary_mask_is_the_mask_boundary():
    for name, m in morphology_ref.patterns(33, 35, seed=3):
        assert np.array_equal(R.edges(m, 1).astype(np.uint8), morphology_ref.boundary(m)), name
    m = np.ones((5, 6), np.uint8)
    assert R.edges(m, 1).sum() == 5 * 6 - 3 * 4 and R.edges(m, 2).sum() == 5 * 6 - 1 * 2 and R.edges(m, 4).all()
    assert not R.edges(m, 0).any()
    dot = np.zeros((9, 9), np.uint8)
    dot[4, 4] = 1
    assert R.edges(dot, 3).sum() == 1                                      # only foreground pixels are edges


def test_touching_labels_of_one_colour_keep_separate_outlines():
    lab = np.zeros((8, 12), np.int32)
    lab[1:7, 1:6] = 1
    lab[1:7, 6:11] = 256                                                   # ((256 - 1) mod 255) + 1 = 1: the same colour
    ident, k = R.identity_and_index(lab)
    assert k[3, 3] == k[3, 8] == 1 and ident[3, 3] != ident[3, 8]
    e = R.edges(ident, 1)
    assert e[3, 5] and e[3, 6] and not e[3, 3] and not e[3, 8]             # both sides of the contact
    assert not R.edges(k, 1)[3, 5]                                         # comparing colours would lose it
    ident, k = R.identity_and_index(np.array([[-5, 0, 255, 256, 2 ** 31 - 1, -2 ** 31]], np.int32))
    assert ident.tolist() == [[0, 0, 255, 256, 2 ** 31 - 1, 0]]
    assert k.tolist() == [[0, 0, 255, 1, (2 ** 31 - 2) % 255 + 1, 0]]


def test_heat_properties():
    base = R.random_region(70, 90, 5)
    lut = R.colormap("heat")
    for G in ((3, 3), (2, 2), (2, 3)):
        Q = np.full(G, 30000, np.int32)                                    # a constant map: one colour either way
        flat = R.render_heat(base, Q, 32, lut, alpha=256, smooth=False)
        assert (flat == lut[(30000 + 128) >> 8]).all()
        assert np.array_equal(R.render_heat(base, Q, 32, lut, alpha=256, smooth=True), flat)
    one = np.array([[R.QMAX]], np.int32)                                   # a one-node map
    for smooth in (False, True):
        assert (R.render_heat(base[:40], one, 40, lut, alpha=256, smooth=smooth) == 255).all()
        assert np.array_equal(R.render_heat(base, np.zeros((3, 3), np.int32), 32, lut, alpha=0, smooth=smooth), base)
    rng = np.random.default_rng(6)
    Q = rng.integers(0, R.QMAX + 1, (3, 3)).astype(np.int32)
    idx = R.heat_index(Q, 70, 90, 32, True)
    assert idx.min() >= 0 and idx.max() <= 255
    # the nodes are the cell centres, which lie between pixels 15 and 16: up to pixel 15 the first node alone counts
    assert (idx[:16, :16] == (Q[0, 0] + 128) >> 8).all()
    d = (31 * (31 * int(Q[0, 0]) + 33 * int(Q[0, 1])) + 33 * (31 * int(Q[1, 0]) + 33 * int(Q[1, 1])) + 2048) // 4096
    assert idx[32, 32] == (d + 128) >> 8                                   # u = 33: weights 31 and 33 of span 64
    # with the H // cell grid the ragged remainder lies beyond the last centre and takes the last node
    idx2 = R.heat_index(Q[:2, :2], 70, 90, 32, True)
    assert (idx2[48:, 48:] == (Q[1, 1] + 128) >> 8).all() and (idx2[:16, 48:] == (Q[0, 1] + 128) >> 8).all()
    cut = int(np.median(idx))
    got = R.render_heat(base, Q, 32, lut, alpha=200, min_index=cut, smooth=True)
    assert np.array_equal(got[idx < cut], base[idx < cut]) and (idx < cut).any() and (idx >= cut).any()
    assert np.array_equal(R.render_heat(base, Q, 32, lut, min_index=256), base)
    # anything a map may hold is clamped, not wrapped
    wild = np.array([[-2 ** 31, 2 ** 31 - 1], [70000, -1]], np.int32)
    for smooth in (False, True):
        idx = R.heat_index(wild, 64, 64, 32, smooth)
        assert idx.min() == 0 and idx.max() == 255


def test_compare_properties():
    a, b = R.random_region(20, 30, 7), R.random_region(20, 30, 8)
    assert np.array_equal(R.compare(a, b, "checker", cell=30), a)
    assert np.array_equal(R.compare(a, b, "checker", cell=64), a)
    c1 = R.compare(a, b, "checker", cell=1)
    assert np.array_equal(c1[0, 0], a[0, 0]) and np.array_equal(c1[0, 1], b[0, 1]) and np.array_equal(c1[1, 1], a[1, 1])
    assert not R.compare(a, a, "difference", gain=255).any()
    assert np.array_equal(R.compare(a, b, "blend", alpha=0), a) and np.array_equal(R.compare(a, b, "blend", alpha=256), b)
    d = R.compare(a, b, "difference", gain=255)
    assert set(np.unique(d)) <= {0, 255}
    assert np.array_equal(R.compare(a, b, "difference", gain=1), np.abs(a.astype(int) - b.astype(int)).astype(np.uint8))


def test_thumbnail_properties():
    img = R.random_region(24, 36, 9)
    mask = (np.random.default_rng(9).random((24, 36)) < 0.05).astype(np.uint8) * 3
    assert np.array_equal(R.box_down(img, 1), img) and np.array_equal(R.box_down(mask, 1), mask)
    for f in (2, 3, 4, 12):
        s = img.astype(np.int64).reshape(24 // f, f, 36 // f, f, 3).sum((1, 3))
        assert np.array_equal(R.box_down(img, f), ((2 * s + f * f) // (2 * f * f)).astype(np.uint8)), f      # round half up
        assert np.array_equal(R.box_down(mask, f), mask.reshape(24 // f, f, 36 // f, f).max((1, 3))), f
    # a ragged block averages its own pixels
    t = R.box_down(img, 16)
    assert t.shape == (2, 3, 3)
    own = img[16:, 32:].astype(np.int64).reshape(-1, 3)
    assert np.array_equal(t[1, 2], (2 * own.sum(0) + 32) // 64)
    half = np.array([[[0, 1, 255]], [[1, 2, 255]]], np.uint8)              # means 0.5, 1.5, 255 round to 1, 2, 255
    assert R.box_down(half, 2)[0, 0].tolist() == [1, 2, 255]
    assert R.box_down(img, 256).shape == (1, 1, 3)
    for arr in (img, mask):
        for f in (1, 2, 3, 5, 16, 256):
            assert np.array_equal(R.box_down_fast(arr, f), R.box_down(arr, f)), f
