"""The dense region alignment (csrc/warp.hip) against the numpy restatement of tests/region_warp_ref.py,
on poisoned memory (every ``torch.empty`` starts as NaN / 0xFF, as in tests/test_registration_gpu.py).  GPU inputs are
crop views with an odd row pitch and an unaligned base inside a guard band of a constant byte, so a wrong index shows as
a wrong value.

What must hold.  Everything is integer arithmetic: warped bytes, fields, ``kept`` and the statistics are bit-equal to the
restatement, for host and GPU input and for every banding."""
import functools

import numpy as np
import pytest
import torch

import region_warp_ref as Wr
from stain2stain_amd import clean_shift_field, register_region, shift_tiles, warp_region

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 77


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


def _view(arr):
    """A uint8 region [H, W, 3] or mask [H, W] as a crop view of a larger GPU array of GUARD bytes: odd row pitch,
    unaligned base.  Returns (view, the larger array)."""
    H, W = arr.shape[:2]
    c = 3 if arr.ndim == 3 else 1
    pad = next(p for p in (6, 7, 8, 9) if ((W + p) * c) % 4 != 0)
    big = torch.full((H + 5, W + pad) + arr.shape[2:], GUARD, dtype=torch.uint8, device=DEV)
    view = big[2:2 + H, 3:3 + W]
    view.copy_(_t(arr))
    assert view.stride(0) % 4 != 0 and view.data_ptr() % 4 != 0
    return view, big


def _t(arr):
    """A host tensor that owns a copy of ``arr`` (the shared references are read-only)."""
    return torch.from_numpy(np.array(arr))


def _guard_intact(big, arr):
    H, W = arr.shape[:2]
    g = big.clone()
    g[2:2 + H, 3:3 + W] = GUARD
    return bool((g == GUARD).all()) and np.array_equal(big[2:2 + H, 3:3 + W].cpu().numpy(), arr)


# name: (H, W, cell): 2 x 2 nodes with ragged edges; 3 x 3 nodes; Gy = 1; one node
SHAPES = {"ragged_2x2": (70, 90, 32), "grid_3x3": (96, 100, 32), "one_row": (40, 100, 40), "one_node": (33, 35, 33)}
# name: (max_shift, the range of the random field in 1/16 px): the whole clamp range, so that taps leave every border
# (max_shift 70 turns whole rows into fill), and values far beyond the clamp
FIELDS = {"small": (3, 48), "large": (70, 1120), "beyond": (3, 2 ** 31 - 1)}


@functools.lru_cache(maxsize=None)
def _warp_case(shape, kind):
    H, W, cell = SHAPES[shape]
    ms, rng_max = FIELDS[kind]
    rng = np.random.default_rng(sorted(SHAPES).index(shape) * 10 + sorted(FIELDS).index(kind))
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    mask = rng.integers(0, 256, (H, W), dtype=np.uint8)
    D = rng.integers(-rng_max, rng_max + 1, (H // cell, W // cell, 2)).astype(np.int32)
    if kind == "beyond":
        D.reshape(-1)[0] = -2 ** 31
    if kind == "large" and D.shape[0] >= 2:
        D[0, :, 0] = -rng_max                                  # every row above the first node centre reads 70 rows up
    want_img, want_mask = Wr.warp(img, D, cell, ms, 255), Wr.warp(mask, D, cell, ms, 0)
    for a in (img, mask, D, want_img, want_mask):
        a.setflags(write=False)
    return img, mask, D, ms, want_img, want_mask


@pytest.mark.parametrize("kind", list(FIELDS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_warp_equals_the_restatement(shape, kind):
    cell = SHAPES[shape][2]
    img, mask, D, ms, want_img, want_mask = _warp_case(shape, kind)
    field = _t(D).to(DEV)
    if kind == "large" and D.shape[0] >= 2:
        assert (want_img[:cell // 2] == 255).all() and (want_mask[:cell // 2] == 0).all()     # whole rows of fill
    for arr, want, fill in ((img, want_img, 255), (mask, want_mask, 0)):
        g, big = _view(arr)
        out = warp_region(g, field, cell, max_shift=ms, fill=fill)
        assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous() and tuple(out.shape) == arr.shape
        got = out.cpu().numpy()
        bad = np.argwhere(got != want)
        assert bad.size == 0, (shape, kind, arr.ndim, len(bad), bad[:4].tolist())
        assert torch.equal(warp_region(g, field, cell, max_shift=ms, fill=fill), out)             # two identical runs
        assert torch.equal(warp_region(_t(arr).to(DEV), field, cell, max_shift=ms, fill=fill), out)
        assert _guard_intact(big, arr)


@pytest.mark.parametrize("shape", ["ragged_2x2", "one_node"])
def test_banding_and_host_input_do_not_change_a_byte(shape):
    H, W, cell = SHAPES[shape]
    img, mask, D, ms, want_img, want_mask = _warp_case(shape, "large")
    field = _t(D).to(DEV)
    for arr, want, fill in ((img, want_img, 255), (mask, want_mask, 0)):
        g, big = _view(arr)
        host = _t(arr)
        for band_rows in (1, 7, H, None):
            dev_out = warp_region(g, field, cell, max_shift=ms, fill=fill, band_rows=band_rows)
            host_out = warp_region(host, field, cell, max_shift=ms, fill=fill, band_rows=band_rows)
            assert dev_out.is_cuda and not host_out.is_cuda and host_out.is_contiguous()
            assert np.array_equal(dev_out.cpu().numpy(), want), (shape, band_rows)
            assert np.array_equal(host_out.numpy(), want), (shape, band_rows)
        assert _guard_intact(big, arr)
    # a small halo: bands of 7 rows with 4 rows of halo, the source band moves with the output band
    img, mask, D, ms, want_img, _ = _warp_case(shape, "small")
    out = warp_region(_t(img), _t(D).to(DEV), cell, max_shift=ms, band_rows=7)
    assert np.array_equal(out.numpy(), want_img)


def test_constant_field_equals_shift_tiles():
    H, W, cell = SHAPES["grid_3x3"]
    img, mask, _, _, _, _ = _warp_case("grid_3x3", "small")
    for dy, dx in ((0, 0), (3, -5), (-11, 7), (64, 0), (0, -64)):
        field = torch.tensor([16 * dy, 16 * dx], dtype=torch.int32, device=DEV).repeat(H // cell, W // cell, 1)
        sh = torch.tensor([[dy, dx]], dtype=torch.int32, device=DEV)
        for arr, fill in ((img, 255), (mask, 3)):
            g, _ = _view(arr)
            out = warp_region(g, field, cell, fill=fill)
            assert torch.equal(out, shift_tiles(g[None], sh, fill)[0]), (dy, dx, arr.ndim)
            assert np.array_equal(out.cpu().numpy(), Wr.shifted(arr, dy, dx, fill))


# ---- cleaning ----------------------------------------------------------------------------------------------------------
def _check_clean(shift, rel, what, **kw):
    want_field, want_kept, want_stats = Wr.clean(shift, rel, **kw)
    pad = torch.full((shift.shape[0] + 2, shift.shape[1] + 2, 2), 10 ** 6, dtype=torch.int32, device=DEV)
    pad[1:-1, 1:-1] = torch.from_numpy(shift).to(DEV)                      # a non-contiguous shift
    for s in (pad[1:-1, 1:-1], torch.from_numpy(shift).to(DEV)):
        got = clean_shift_field(s, reliable=torch.from_numpy(rel).to(DEV), **kw)
        assert got["field"].dtype == torch.int32 and got["kept"].dtype == torch.uint8 and got["stats"].dtype == torch.int32
        assert np.array_equal(got["kept"].cpu().numpy(), want_kept), what
        assert got["stats"].tolist() == want_stats.tolist(), (what, got["stats"].tolist(), want_stats.tolist())
        assert np.array_equal(got["field"].cpu().numpy(), want_field), what
    return want_field, want_kept, want_stats


@pytest.mark.parametrize("Gy,Gx", [(1, 1), (1, 7), (5, 6), (17, 33)])
def test_clean_equals_the_restatement_on_random_masks(Gy, Gx):
    rng = np.random.default_rng(Gy * 100 + Gx)
    for density in (0.9, 0.5, 0.08):
        shift = rng.integers(-3, 4, (Gy, Gx, 2)).astype(np.int32)
        wild = rng.random((Gy, Gx)) < 0.15
        shift[wild] = rng.integers(-80, 81, (int(wild.sum()), 2))           # outliers, some beyond max_shift = 64
        rel = (rng.random((Gy, Gx)) < density).astype(np.uint8)
        for max_dev in (0, 2):
            _check_clean(shift, rel, (Gy, Gx, density, max_dev), max_dev=max_dev)


def test_clean_corner_outlier_and_empty_cases():
    shift = np.zeros((17, 33, 2), np.int32)
    shift[0, 0] = (3, -4)
    rel = np.zeros((17, 33), np.uint8)
    rel[0, 0] = 1
    field, kept, stats = _check_clean(shift, rel, "corner")
    assert stats.tolist() == [1, 32] and (field == [48, -64]).all()
    rng = np.random.default_rng(11)
    shift = rng.integers(-2, 3, (5, 6, 2)).astype(np.int32)
    shift[2, 3] = (30, 30)
    field, kept, stats = _check_clean(shift, np.ones((5, 6), np.uint8), "outlier", max_dev=4)
    assert kept[2, 3] == 0 and stats.tolist() == [29, 1] and np.abs(field[2, 3]).max() <= 32
    field, kept, stats = _check_clean(shift, np.zeros((5, 6), np.uint8), "empty")
    assert not field.any() and not kept.any() and stats.tolist() == [0, 0]
    extreme = np.full((5, 6, 2), -2 ** 31, np.int32)                       # no shift within max_shift: nothing is kept
    extreme[1, 1] = (2 ** 31 - 1, 0)
    _check_clean(extreme, np.ones((5, 6), np.uint8), "extreme")


def test_clean_takes_the_field_dict_as_it_comes():
    rng = np.random.default_rng(4)
    shift = rng.integers(-2, 3, (5, 6, 2)).astype(np.int32)
    valid = (rng.random((5, 6)) < 0.8).astype(np.int32)
    score, margin = rng.uniform(0.3, 1.0, (5, 6)), rng.uniform(0.0, 0.3, (5, 6))
    rel = Wr.reliable(valid, score, margin, shift, 0.5, 0.05, 64)
    assert 0 < rel.sum() < 30
    want = Wr.clean(shift, rel)
    d = {"shift": torch.from_numpy(shift).to(DEV), "valid": torch.from_numpy(valid).to(DEV),
         "score": torch.from_numpy(score).to(DEV), "margin": torch.from_numpy(margin).to(DEV)}
    got = clean_shift_field(d)
    for k, w in zip(("field", "kept", "stats"), want):
        assert np.array_equal(got[k].cpu().numpy(), w), k


# ---- end to end ----------------------------------------------------------------------------------------------------------
def test_register_region_aligns_the_glass_pair():
    src, tgt = Wr.glass_pair()
    mask = np.random.default_rng(6).integers(0, 4, (128, 192), dtype=np.uint8)
    (gs, bs), (gt, bt), (gm, bm) = _view(src), _view(tgt), _view(mask)
    want, want_mask = Wr.shifted(tgt, 3, -5, 255), Wr.shifted(mask, 3, -5, 0)
    dev = register_region(gs, gt, 64, masks=[gm], radius=6)
    host = register_region(torch.from_numpy(src), torch.from_numpy(tgt), 64, masks=[torch.from_numpy(mask)], radius=6,
                           band_rows=50)
    for out, on_gpu in ((dev, True), (host, False)):
        assert out["aligned"].is_cuda == on_gpu and out["masks"][0].is_cuda == on_gpu
        assert np.array_equal(out["aligned"].cpu().numpy(), want)
        assert len(out["masks"]) == 1 and np.array_equal(out["masks"][0].cpu().numpy(), want_mask)
        assert out["field"].is_cuda and (out["field"].cpu().numpy() == [48, -80]).all()     # the glass cell was filled
        assert out["kept"].tolist() == [[1, 1, 1], [1, 0, 1]] and out["stats"].tolist() == [5, 1]
        assert tuple(out["score"].shape) == (2, 3) and out["score"].dtype == torch.float64
        assert float(out["score"][1, 1]) == 0.0 and float(out["score"].sum()) > 4.5
    assert _guard_intact(bs, src) and _guard_intact(bt, tgt) and _guard_intact(bm, mask)


# ---- no hidden synchronisation ----------------------------------------------------------------------------------------------
def test_region_alignment_does_not_synchronise():
    src, tgt = Wr.glass_pair()
    mask = np.zeros((128, 192), np.uint8)
    gs, gt, gm = _view(src)[0], _view(tgt)[0], _view(mask)[0]
    register_region(gs, gt, 64, masks=[gm], radius=6)           # the library is loaded from here on
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = register_region(gs, gt, 64, masks=[gm], radius=6)
        cleaned = clean_shift_field(out["field"] // 16, reliable=out["kept"])
        again = warp_region(gt, cleaned["field"], 64, band_rows=40)
        moved = warp_region(gm, cleaned["field"], 64, fill=0)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert torch.equal(again, out["aligned"]) and torch.equal(moved, out["masks"][0])
    assert out["stats"].tolist() == [5, 1] and cleaned["stats"].tolist() == [5, 1]
