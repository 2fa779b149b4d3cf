"""Result rendering (csrc/render.hip) against the numpy int64 restatement of tests/render_ref.py, on
poisoned memory (every ``torch.empty`` and every workspace starts as 0xFF, as in tests/test_qc_gpu.py).  Every GPU input
is given two ways: as a crop view with an odd row pitch and an unaligned base inside a guard band of a constant byte, and
as an aligned contiguous copy, so the dword and the byte paths of every load and store run; the guard bytes are checked
after every call.

What must hold.  Everything is integer arithmetic: every result is bit-equal to the restatement, for host and GPU input
and for every banding, and two runs give identical bytes."""
import functools

import numpy as np
import pytest
import torch

import render_ref as R
import stain_quant_ref
from stain2stain_amd import (colormap, compare_regions, compose_panels, default_palette, downsample_region,
                             region_stain_map, render_classes, render_heat, render_region, stain_objects)
from stain2stain_amd.render import quantize_map

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 77
# 1 x 1, a row and a column; odd sizes; 70 x 90 (ragged at cell 32); 40 x 100 (one node row at cell 40); 260 x 515: a row
# spans two waves and ends in a lane with three pixels, and the rows span more than one workgroup
SHAPES = [(1, 1), (1, 9), (9, 1), (33, 35), (70, 90), (40, 100), (260, 515)]
CELLS = {(1, 1): 1, (1, 9): 4, (9, 1): 4, (33, 35): 8, (70, 90): 32, (40, 100): 40, (260, 515): 64}


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


class Guarded:
    """``arr`` ([H, W, 3] or [H, W], uint8 / bool / int32) as a crop view of a larger GPU array of guard values: odd row
    pitch in bytes, and for byte arrays an unaligned base."""

    def __init__(self, arr):
        self.arr = np.array(arr)
        H, W = arr.shape[:2]
        C = 3 if arr.ndim == 3 else 1
        item = self.arr.dtype.itemsize
        pad = next(p for p in (6, 7, 8, 9) if item > 1 or (((W + p) * C) % 4 != 0 and ((2 * (W + p) + 3) * C) % 4 != 0))
        if item > 1 and (W + pad) % 2 == 0:
            pad += 1                                            # an odd pitch in elements
        self.guard = GUARD if self.arr.dtype != np.bool_ else True
        self.big = torch.full((H + 5, W + pad) + arr.shape[2:], self.guard, dtype=_t(self.arr[:1]).dtype, device=DEV)
        self.view = self.big[2:2 + H, 3:3 + W]
        self.view.copy_(_t(self.arr))
        if item == 1:
            assert self.view.stride(0) * item % 4 != 0 and self.view.data_ptr() % 4 != 0
        else:
            assert self.view.stride(0) % 2 == 1

    def border_intact(self):
        H, W = self.arr.shape[:2]
        g = self.big.clone()
        g[2:2 + H, 3:3 + W] = self.guard
        return bool((g == self.guard).all())

    def intact(self):
        H, W = self.arr.shape[:2]
        return self.border_intact() and np.array_equal(self.big[2:2 + H, 3:3 + W].cpu().numpy(), self.arr)


def _layouts(*arrays):
    """(name, GPU tensors, guards): every array as a crop view, then every array as an aligned contiguous copy."""
    guards = [Guarded(a) for a in arrays]
    return (("view", [g.view for g in guards], guards), ("contiguous", [_t(a).to(DEV) for a in arrays], []))


def _same(got, want, what):
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape, (what, tuple(got.shape), want.shape)
    g = got.cpu().numpy()
    bad = np.argwhere(g != want)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), g[tuple(bad[0])], want[tuple(bad[0])])


@functools.lru_cache(maxsize=None)
def _region(H, W, seed=0):
    img = R.random_region(H, W, 100 * H + W + seed)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _class_mask(H, W):
    """uint8 [H, W]: blobs of 3 x 3 pixels over all 256 classes with a third background, and single-pixel specks."""
    rng = np.random.default_rng(7 * H + W)
    coarse = rng.integers(0, 256, (-(-H // 3), -(-W // 3))) * (rng.random((-(-H // 3), -(-W // 3))) > 0.33)
    m = np.kron(coarse, np.ones((3, 3), np.int64))[:H, :W]
    m = np.where(rng.random((H, W)) < 0.08, rng.integers(0, 256, (H, W)), m).astype(np.uint8)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _labels(H, W):
    lab = R.random_labels(H, W, 11 * H + W)
    lab.setflags(write=False)
    return lab


def _alphas(seed):
    fa = np.random.default_rng(seed).integers(0, 257, 256)
    fa[[3, 17]] = (0, 256)
    return fa


# ---- classes and labels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SHAPES)
def test_class_overlay_equals_the_restatement(H, W):
    base, mask, fa = _region(H, W), _class_mask(H, W), _alphas(H + W)
    pal = np.random.default_rng(3).integers(0, 256, (256, 3), dtype=np.uint8)
    want = {r: R.render_classes(base, mask, pal, fa, r=r, edge_alpha=200) for r in range(5)}      # r = 4 > H for H = 1
    want_fixed = R.render_classes(base, mask, pal, fa, r=2, edge_alpha=256, edge_rgb=(9, 200, 31))
    want_default = R.render_classes(base, mask)
    for name, (g, m), guards in _layouts(base, mask):
        for r in range(5):
            got = render_classes(g, m, palette=_t(pal), class_alpha=fa.tolist(), outline=r, outline_alpha=200)
            _same(got, want[r], (H, W, name, r))
            assert got.is_contiguous() and all(x.intact() for x in guards), (name, r)
        got = render_classes(g, m, palette=_t(pal).to(DEV), class_alpha=_t(fa.astype(np.int32)).to(DEV), outline=2,
                             outline_rgb=(9, 200, 31))
        _same(got, want_fixed, (H, W, name, "fixed edge colour, device tables"))
        assert torch.equal(render_classes(g, m, palette=_t(pal), class_alpha=_t(fa), outline=2, outline_rgb=(9, 200, 31)),
                           got)                                                              # two identical runs
        _same(render_classes(g, m), want_default, (H, W, name, "defaults"))
        assert all(x.intact() for x in guards), name
    if H > 1 and W > 1:
        assert any((want[r] != want[r + 1]).any() for r in range(4)) and (want[0] != base).any()


@pytest.mark.parametrize("H,W", SHAPES)
def test_label_overlay_equals_the_restatement(H, W):
    base, lab = _region(H, W), _labels(H, W)
    if H * W >= 6:
        lab = lab.copy()
        lab.reshape(-1)[:6] = (-5, 0, 255, 256, 2 ** 31 - 1, -2 ** 31)
    for name, (g, m), guards in _layouts(base, lab):
        for r in (0, 1, 3, 4):
            got = render_classes(g, m, alpha=160, outline=r, outline_alpha=256)
            _same(got, R.render_classes(base, lab, alpha=160, r=r), (H, W, name, r))
            assert all(x.intact() for x in guards), (name, r)
    # a bool mask is classes 0 and 1
    fg = lab > 0
    for name, (g, m), guards in _layouts(base, fg):
        assert m.dtype == torch.bool
        _same(render_classes(g, m, outline=1, outline_rgb=(255, 255, 255)),
              R.render_classes(base, fg.astype(np.uint8), r=1, edge_rgb=(255, 255, 255)), (H, W, name, "bool"))
        assert all(x.intact() for x in guards), name


def test_touching_parts_of_one_colour_keep_their_outlines_on_the_gpu():
    base = _region(33, 35)
    lab = np.zeros((33, 35), np.int32)
    lab[4:20, 3:15] = 1
    lab[4:20, 15:30] = 256                                                  # the same colour index as label 1
    lab[20:30, 3:30] = 2 ** 31 - 1
    want = R.render_classes(base, lab, alpha=0, r=1, edge_rgb=(0, 255, 0))
    got = render_classes(_t(base).to(DEV), _t(lab).to(DEV), alpha=0, outline=1, outline_rgb=(0, 255, 0))
    _same(got, want, "touching")
    assert got[10, 14].tolist() == [0, 255, 0] and got[10, 15].tolist() == [0, 255, 0]
    assert got[10, 8].tolist() == base[10, 8].tolist()


@pytest.mark.parametrize("H,W", [(33, 35), (260, 515)])
def test_overlays_run_in_place(H, W):
    base, mask, lab = _region(H, W), _class_mask(H, W), _labels(H, W)
    Q = np.random.default_rng(H).integers(0, R.QMAX + 1, (-(-H // CELLS[H, W]), -(-W // CELLS[H, W]))).astype(np.int32)
    lut = R.colormap("blue_red")
    sparse = np.where(mask > 200, mask, 0).astype(np.uint8)                 # most lanes change nothing and write nothing
    steps = ((lambda g, out: render_classes(g, _t(mask).to(DEV), outline=2, out=out), R.render_classes(base, mask, r=2)),
             (lambda g, out: render_classes(g, _t(sparse).to(DEV), alpha=256, outline=0, out=out),
              R.render_classes(base, sparse, alpha=256, r=0)),
             (lambda g, out: render_classes(g, _t(lab).to(DEV), outline=4, out=out), R.render_classes(base, lab, r=4)),
             (lambda g, out: render_heat(g, _t(Q).to(DEV), CELLS[H, W], quantized=True, lut="blue_red", min_index=128,
                                         out=out), R.render_heat(base, Q, CELLS[H, W], lut, min_index=128)))
    for call, want in steps:
        for layout in ("view", "contiguous"):
            guard = Guarded(base)
            g = guard.view if layout == "view" else _t(base).to(DEV)
            got = call(g, g)
            assert got.data_ptr() == g.data_ptr() and got.stride() == g.stride()
            _same(got.contiguous(), want, (H, W, layout))
            assert layout == "contiguous" or guard.border_intact()
        # into a buffer of the caller's that is not the region
        guard, other = Guarded(base), Guarded(np.zeros_like(base))
        got = call(guard.view, other.view)
        _same(got.contiguous(), want, (H, W, "other"))
        assert guard.intact() and other.border_intact()
    big = torch.zeros((H + 1, W, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="must not overlap it in part"):
        render_classes(big[:H], _t(mask).to(DEV), out=big[1:])


# ---- heat -------------------------------------------------------------------------------------------------------------
def _grids(H, W, cell):
    """Both grid conventions: (H // cell, W // cell) where that is a grid, and (ceil(H / cell), ceil(W / cell))."""
    lo, hi = (max(H // cell, 1), max(W // cell, 1)), (-(-H // cell), -(-W // cell))
    if H // cell < 1:
        lo = (hi[0], lo[1])
    if W // cell < 1:
        lo = (lo[0], hi[1])
    return sorted({lo, hi})


@pytest.mark.parametrize("H,W", SHAPES)
def test_heat_overlay_equals_the_restatement(H, W):
    base, cell = _region(H, W), CELLS[H, W]
    grids = _grids(H, W, cell)
    assert grids == {(1, 1): [(1, 1)], (1, 9): [(1, 2), (1, 3)], (9, 1): [(2, 1), (3, 1)], (33, 35): [(4, 4), (5, 5)],
                     (70, 90): [(2, 2), (3, 3)], (40, 100): [(1, 2), (1, 3)], (260, 515): [(4, 8), (5, 9)]}[H, W]
    lut = np.random.default_rng(5).integers(0, 256, (256, 3), dtype=np.uint8)
    rng = np.random.default_rng(H + 3 * W)
    for Gy, Gx in grids:
        Q = rng.integers(0, R.QMAX + 1, (Gy, Gx)).astype(np.int32)
        Q.reshape(-1)[0] = R.QMAX
        Q.reshape(-1)[-1] = 0
        want = {(smooth, mi): R.render_heat(base, Q, cell, lut, alpha=180, min_index=mi, smooth=smooth)
                for smooth in (False, True) for mi in (0, 1, 256)}
        want_heat = {smooth: R.render_heat(base, Q, cell, R.colormap("heat"), alpha=256, min_index=100, smooth=smooth)
                     for smooth in (False, True)}
        assert np.array_equal(want[True, 256], base)
        for name, (g,), guards in _layouts(base):
            q = _t(Q).to(DEV)
            for smooth in (False, True):
                for min_index in (0, 1, 256):
                    got = render_heat(g, q, cell, quantized=True, lut=_t(lut), alpha=180, min_index=min_index,
                                      smooth=smooth)
                    _same(got, want[smooth, min_index], (H, W, Gy, Gx, name, smooth, min_index))
                    assert all(x.intact() for x in guards)
                got = render_heat(g, q, cell, quantized=True, lut="heat", alpha=256, min_index=100, smooth=smooth)
                _same(got, want_heat[smooth], (H, W, Gy, Gx, name, smooth, "heat"))
                assert torch.equal(render_heat(g, q, cell, quantized=True, lut="heat", alpha=256, min_index=100,
                                               smooth=smooth), got)


def test_heat_clamps_whatever_the_map_holds():
    """Nodes beyond 0 .. 65280, up to the ends of int32: the blend leaves the float64 range and takes the int64 path."""
    base = _region(70, 90)
    rng = np.random.default_rng(9)
    Q = rng.integers(-2 ** 31, 2 ** 31, (3, 3)).astype(np.int32)
    Q[0, 0], Q[0, 1], Q[1, 1], Q[2, 2] = -2 ** 31, 2 ** 31 - 1, 70000, -1
    near = rng.integers(-(1 << 20) - 2, (1 << 20) + 3, (3, 3)).astype(np.int32)     # around the float64 / int64 switch
    near[0, 0], near[1, 1] = 1 << 20, (1 << 20) + 1
    lut = R.colormap("gray")
    for M in (Q, near):
        for smooth in (False, True):
            for name, (g,), guards in _layouts(base):
                got = render_heat(g, _t(M).to(DEV), 32, quantized=True, lut="gray", alpha=256, smooth=smooth)
                _same(got, R.render_heat(base, M, 32, lut, alpha=256, smooth=smooth), (name, smooth))
    # the largest cell: span^2 = 2^30
    tall = R.random_region(3, 33000, 5)
    M = np.array([[0, R.QMAX]], np.int32)
    got = render_heat(_t(tall).to(DEV), _t(M).to(DEV), 1 << 14, quantized=True, lut="gray", alpha=256)
    _same(got, R.render_heat(tall, M, 1 << 14, lut, alpha=256), "cell 2^14")


def test_heat_quantisation_equals_the_restatement():
    base = _region(70, 90)
    lo, hi = -1.0, 254.0                                                    # a step of exactly 1 / 256
    ks = np.array([[0, 1, 127], [128, 129, 32640], [65279, 65280, 40000]], np.float64)
    v = lo + ks / 256.0
    want_q = R.quantize(v, lo, hi)
    assert np.array_equal(want_q, ks.astype(np.int32))
    odd = np.array([[np.nan, lo - 3.0, hi + 1.0], [np.inf, -np.inf, lo], [hi, 0.3, 100.7]], np.float64)
    lut = R.colormap("heat")
    for vals, dtype in ((v, torch.float64), (v, torch.float32), (odd, torch.float64), (odd, torch.float32)):
        tv = _t(vals).to(dtype)
        q = R.quantize(tv.numpy(), lo, hi)
        assert np.array_equal(quantize_map(tv.to(DEV), lo, hi).cpu().numpy(), q)
        for smooth in (False, True):
            got = render_heat(_t(base).to(DEV), tv.to(DEV), 32, lo=lo, hi=hi, smooth=smooth)
            _same(got, R.render_heat(base, q, 32, lut, smooth=smooth), (dtype, smooth))
    assert R.quantize(odd, lo, hi).tolist() == [[0, 0, 65280], [65280, 0, 0], [65280, 333, 26035]]
    counts = _t(np.arange(9, dtype=np.int64).reshape(3, 3) * 1000)           # an integer map, and a host map
    _same(render_heat(_t(base).to(DEV), counts, 32, lo=0, hi=8000),
          R.render_heat(base, R.quantize(counts.numpy(), 0, 8000), 32, lut), "int64 host map")


# ---- compare ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SHAPES)
def test_comparisons_equal_the_restatement(H, W):
    a, b = _region(H, W), _region(H, W, seed=1)
    b = np.where(np.random.default_rng(H).random((H, W, 1)) < 0.5, a, b)    # half the pixels agree
    cases = ([("checker", {"cell": c}) for c in (1, 7, 64)] + [("blend", {"alpha": al}) for al in (0, 77, 256)]
             + [("difference", {"gain": gn}) for gn in (1, 4, 255)])
    for name, (ga, gb), guards in _layouts(a, b):
        for mode, kw in cases:
            got = compare_regions(ga, gb, mode, **kw)
            _same(got, R.compare(a, b, mode, **kw), (H, W, name, mode, kw))
            assert all(x.intact() for x in guards)
        assert torch.equal(compare_regions(ga, gb, "checker", cell=7), compare_regions(ga, gb, "checker", cell=7))
    _same(compare_regions(_t(a).to(DEV), _t(b).to(DEV)), R.compare(a, b, "checker", cell=64), "defaults")


# ---- thumbnails -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SHAPES)
def test_thumbnails_equal_the_restatement(H, W):
    img = _region(H, W)
    mask = np.where(np.random.default_rng(W).random((H, W)) < 0.02, _class_mask(H, W), 0).astype(np.uint8)
    for arr in (img, mask):
        for name, (g,), guards in _layouts(arr):
            for f in (1, 2, 3, 16, 256):
                got = downsample_region(g, f)
                _same(got, R.box_down_fast(arr, f), (H, W, arr.ndim, name, f))
                assert got.is_contiguous() and all(x.intact() for x in guards)
            assert torch.equal(downsample_region(g, 3), downsample_region(g, 3))


def test_thumbnail_of_saturated_blocks():
    """255 everywhere: the largest sum, 255 * 65536, and its rounding."""
    img = np.full((300, 520, 3), 255, np.uint8)
    img[256:, :, 1] = 254
    _same(downsample_region(_t(img).to(DEV), 256), R.box_down_fast(img, 256), "saturated")
    assert R.box_down_fast(img, 256)[0, 0].tolist() == [255, 255, 255]


# ---- banding: host against GPU input ------------------------------------------------------------------------------------
@pytest.mark.parametrize("band_rows", [1, 7, 70, None])
def test_every_call_is_independent_of_banding_and_of_where_the_region_lives(band_rows):
    H, W = 70, 90
    base, other, mask, lab = _region(H, W), _region(H, W, seed=1), _class_mask(H, W), _labels(H, W)
    Q = np.random.default_rng(1).integers(0, R.QMAX + 1, (3, 3)).astype(np.int32)
    vals = np.random.default_rng(2).random((2, 2)).astype(np.float32)
    kw = {"band_rows": band_rows}
    calls = (
        ("classes", lambda x: render_classes(x(base), x(mask), outline=4, **kw), R.render_classes(base, mask, r=4)),
        ("labels", lambda x: render_classes(x(base), x(lab), outline=3, outline_rgb=(1, 2, 3), **kw),
         R.render_classes(base, lab, r=3, edge_rgb=(1, 2, 3))),
        ("bool", lambda x: render_classes(x(base), x(lab > 0), **kw), R.render_classes(base, (lab > 0).astype(np.uint8))),
        ("heat", lambda x: render_heat(x(base), x(Q), 32, quantized=True, **kw),
         R.render_heat(base, Q, 32, R.colormap("heat"))),
        ("heat, flat, real map", lambda x: render_heat(x(base), x(vals), 32, smooth=False, lut="gray", **kw),
         R.render_heat(base, R.quantize(vals), 32, R.colormap("gray"), smooth=False)),
        ("checker", lambda x: compare_regions(x(base), x(other), "checker", cell=7, **kw),
         R.compare(base, other, "checker", cell=7)),
        ("blend", lambda x: compare_regions(x(base), x(other), "blend", alpha=99, **kw),
         R.compare(base, other, "blend", alpha=99)),
        ("difference", lambda x: compare_regions(x(base), x(other), "difference", **kw),
         R.compare(base, other, "difference")),
        ("thumbnail 3", lambda x: downsample_region(x(base), 3, **kw), R.box_down_fast(base, 3)),
        ("thumbnail 16", lambda x: downsample_region(x(base), 16, **kw), R.box_down_fast(base, 16)),
        ("mask thumbnail", lambda x: downsample_region(x(mask), 3, **kw), R.box_down_fast(mask, 3)),
        ("layers", lambda x: render_region(x(base), [("classes", x(mask)), ("heat", x(Q), 32, {"quantized": True}),
                                                      ("classes", x(lab), {"alpha": 0, "outline": 2})], **kw),
         R.render_classes(R.render_heat(R.render_classes(base, mask), Q, 32, R.colormap("heat")), lab, alpha=0, r=2)),
    )
    for what, call, want in calls:
        on_gpu = call(lambda a: _t(a).to(DEV))
        assert on_gpu.is_cuda
        _same(on_gpu, want, (what, "gpu", band_rows))
        on_host = call(_t)
        assert not on_host.is_cuda
        _same(on_host, want, (what, "host", band_rows))
    # a host region given as a strided view, and a host out
    wide = torch.zeros((H, W + 5, 3), dtype=torch.uint8)
    wide[:, 2:2 + W] = _t(base)
    out = torch.zeros((H, W, 3), dtype=torch.uint8)
    assert render_classes(wide[:, 2:2 + W], _t(mask), out=out, **kw) is out
    _same(out, R.render_classes(base, mask), ("host view", band_rows))


# ---- composition --------------------------------------------------------------------------------------------------------
def test_render_region_equals_its_layers_chained():
    H, W = 70, 90
    base, mask, lab = _region(H, W), _class_mask(H, W), _labels(H, W)
    vals = np.random.default_rng(4).random((3, 3))
    guard = Guarded(base)
    m, l, v = _t(mask).to(DEV), _t(lab).to(DEV), _t(vals).to(DEV)
    got = render_region(guard.view, [("heat", v, 32, {"alpha": 100, "lut": "blue_red"}),
                                     ("classes", m, {"alpha": 40, "outline": 0}),
                                     ("classes", l, {"alpha": 0, "outline": 2, "outline_rgb": (0, 0, 0)})])
    assert guard.intact() and got.data_ptr() != guard.view.data_ptr()       # the region itself is never written
    one = render_heat(guard.view, v, 32, alpha=100, lut="blue_red")
    two = render_classes(one, m, alpha=40, outline=0)
    three = render_classes(two, l, alpha=0, outline=2, outline_rgb=(0, 0, 0))
    assert torch.equal(got, three)
    want = R.render_heat(base, R.quantize(vals), 32, R.colormap("blue_red"), alpha=100)
    want = R.render_classes(R.render_classes(want, mask, alpha=40, r=0), lab, alpha=0, r=2, edge_rgb=(0, 0, 0))
    _same(got, want, "three layers")
    _same(render_region(guard.view, [("classes", m)]), R.render_classes(base, mask), "one layer, no options")


def test_compose_panels_equals_the_restatement_on_the_gpu():
    ims = [_region(33, 35, seed=s) for s in range(5)]
    views = [Guarded(i) for i in ims]
    for kw in ({}, {"cols": 2}, {"cols": 3, "gap": 0, "fill": 7}, {"cols": 1, "gap": 3, "fill": 0}):
        got = compose_panels([g.view for g in views], **kw)
        assert got.is_cuda
        _same(got, R.compose(ims, **kw), kw)
    masks = [_class_mask(33, 35), _class_mask(33, 35)[::-1].copy()]
    _same(compose_panels([_t(m).to(DEV) for m in masks], gap=2), R.compose(masks, gap=2), "masks")
    assert all(g.intact() for g in views)


# ---- end to end -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hdab_tile():
    """uint8 [96, 128, 3]: haematoxylin background with DAB discs, as tests/test_objects_gpu.py builds its tiles."""
    H, W = 96, 128
    rng = np.random.default_rng(31)
    yy, xx = np.mgrid[0:H, 0:W]
    conc = np.zeros((H, W, 3))
    conc[..., 0] = rng.uniform(0.05, 0.5, size=(H, W))
    conc[..., 1] = 0.02
    for _ in range(12):
        cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(2.0, 9.0)
        conc[..., 1][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = rng.uniform(0.5, 1.2)
    img = stain_quant_ref.synthesise(conc, "hdab")
    img = np.clip(img.astype(np.int32) + rng.integers(-3, 4, size=(H, W, 3)), 0, 255).astype(np.uint8)
    img.setflags(write=False)
    return img


def test_objects_and_burden_of_a_stained_tile_end_in_a_picture():
    img = _hdab_tile()
    guard = Guarded(img)
    g = guard.view
    objs = stain_objects(g[None], thresholds=(0.2, 0.15, 0.1), return_labels=True)
    labels = objs["labels"][0]
    burden = region_stain_map(g, cell=32)["burden"]
    assert labels.dtype == torch.int32 and tuple(burden.shape) == (3, 4) and int(objs["count"][0]) >= 3
    layers = [("heat", burden, 32, {"hi": 0.5, "alpha": 96, "min_index": 1}),
              ("classes", labels, {"alpha": 64, "outline": 1, "outline_rgb": (0, 0, 0)})]
    got = render_region(g, layers)
    want = R.render_heat(img, R.quantize(burden.cpu().numpy(), 0.0, 0.5), 32, R.colormap("heat"), alpha=96, min_index=1)
    want = R.render_classes(want, labels.cpu().numpy(), alpha=64, r=1, edge_rgb=(0, 0, 0))
    _same(got, want, "end to end")
    assert guard.intact() and (want != img).any()
    thumb = downsample_region(got, 4)
    _same(thumb, R.box_down_fast(want, 4), "thumbnail of the picture")
    panel = compose_panels([downsample_region(g, 4), thumb])
    _same(panel, R.compose([R.box_down_fast(img, 4), R.box_down_fast(want, 4)]), "panel")
    _same(render_region(_t(img), [(k, a.cpu(), *rest) for k, a, *rest in layers], band_rows=20), want, "host, banded")


# ---- no hidden synchronisation ------------------------------------------------------------------------------------------
def test_rendering_does_not_synchronise():
    H, W = 70, 90
    base, other, mask, lab = _region(H, W), _region(H, W, seed=1), _class_mask(H, W), _labels(H, W)
    guard = Guarded(base)
    g, o, m, l = guard.view, _t(other).to(DEV), _t(mask).to(DEV), _t(lab).to(DEV)
    vals = _t(np.random.default_rng(4).random((3, 3))).to(DEV)
    pal = default_palette()

    def everything():
        a = render_classes(g, m, palette=pal, class_alpha=[0] + [50] * 255, outline=2)
        b = render_classes(g, l, outline=1, outline_rgb=(255, 255, 255), band_rows=16)
        c = render_heat(g, vals, 32, lo=0.1, hi=0.9, lut=colormap("blue_red"))
        d = render_heat(g, vals, 32, smooth=False, min_index=30)
        e = [compare_regions(g, o, mode, band_rows=33) for mode in ("checker", "blend", "difference")]
        f = downsample_region(g, 4)
        h = downsample_region(m, 4)
        i = render_region(g, [("classes", m), ("heat", vals, 32), ("classes", l, {"alpha": 0})])
        j = render_classes(a, m, out=a)
        return [a, b, c, d, *e, f, h, i, j, compose_panels([f, f, f], cols=2)]

    first = [t.clone() for t in everything()]                   # the library and the tables are loaded from here on
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = everything()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    assert guard.intact()
