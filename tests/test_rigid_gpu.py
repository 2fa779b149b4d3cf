"""The rigid pre-alignment (csrc/rigid.hip) against the numpy restatement of tests/rigid_ref.py, on
poisoned memory (every ``torch.empty`` starts as NaN / 0xFF, as in tests/test_region_warp_gpu.py).  GPU inputs are crop
views with an odd row pitch and an unaligned base inside a guard band of a constant byte, so a wrong index shows as a
wrong value.

What must hold.  Everything is integer arithmetic: overview maps, warped bytes, shifts, transforms and fields are
bit-equal to the restatement, for host and GPU input and for every banding, and the guard bytes stay intact.  Scores
agree as in tests/test_registration_gpu.py: within 1e-12 relative (an absolute 1e-15 where the value is 0); the picks are
exact because the restatement's best score leads by more than 1e-3 (tests/test_rigid_cpu.py checks that)."""
import functools

import numpy as np
import pytest
import torch

import region_warp_ref as Wr
import registration_ref as R
import rigid_ref as G
from stain2stain_amd import (align_regions, register_rigid, rigid_warp, rotation_table, shift_tiles, structure_map,
                             structure_overview, warp_region)

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 77
ONE = 1 << 24


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
    """A uint8 region [H, W, 3] or map [H, W] as a crop view of a larger GPU array of GUARD bytes: odd row pitch,
    unaligned base.  Returns (view, the larger array)."""
    H, W = arr.shape[:2]
    c = 3 if arr.ndim == 3 else 1
    pad = next(p for p in (6, 7, 8, 9) if ((W + p) * c) % 4 != 0)
    big = torch.full((H + 5, W + pad) + arr.shape[2:], GUARD, dtype=torch.uint8, device=DEV)
    view = big[2:2 + H, 3:3 + W]
    view.copy_(_t(arr))
    assert view.stride(0) % 4 != 0 and view.data_ptr() % 4 != 0
    return view, big


def _guard_intact(big, arr):
    H, W = arr.shape[:2]
    g = big.clone()
    g[2:2 + H, 3:3 + W] = GUARD
    return bool((g == GUARD).all()) and np.array_equal(big[2:2 + H, 3:3 + W].cpu().numpy(), arr)


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want)
    bound = np.where(want == 0.0, 1e-15, 1e-12 * np.abs(want))
    print(f"{what}: largest error {err.max():.3e} (largest bound {bound.max():.3e})")
    assert got.shape == want.shape and (err <= bound).all(), what


def _same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    bad = np.argwhere(got != want)
    assert got.shape == want.shape and bad.size == 0, (what, len(bad), bad[:4].tolist())


# ---- overview maps -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _region(H, W):
    rng = np.random.default_rng(H * 1000 + W)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    img[: H // 2, : W // 3] //= 3                              # a darker part: structure bytes over their whole range
    img.setflags(write=False)
    return img


@pytest.mark.parametrize("H,W", [(70, 90), (131, 67)])
def test_overview_equals_the_restatement_and_structure_map(H, W):
    img = _region(H, W)
    g, big = _view(img)
    for stains in ("hed", "hdab"):
        w = R.weights(stains, 0)
        for ds in (1, 2, 4, 8, 16, 32, 64):
            want = G.overview(img, w, ds)
            out = structure_overview(g, ds, stains=stains)
            assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous()
            _same(out, want, (H, W, stains, ds))
            assert torch.equal(structure_overview(_t(img).to(DEV), ds, stains=stains), out)
            if ds <= 4:
                assert torch.equal(structure_map(g[None], stains, 0, ds)[0], out), (stains, ds)
        assert want.shape == (H // 64, W // 64) and len(np.unique(G.overview(img, w, 8))) > 4
    assert _guard_intact(big, img)


@pytest.mark.parametrize("H,W", [(70, 90), (131, 67)])
def test_overview_banding_and_host_input_do_not_change_a_byte(H, W):
    img = _region(H, W)
    g, big = _view(img)
    w = R.weights("hed", 0)
    for ds in (1, 4, 16):
        want = G.overview(img, w, ds)
        for band_rows in (ds, 3 * ds, H, None):
            dev_out = structure_overview(g, ds, band_rows=band_rows)
            host_out = structure_overview(_t(img), ds, band_rows=band_rows)
            assert dev_out.is_cuda and host_out.is_cuda
            _same(dev_out, want, (ds, band_rows, "gpu"))
            _same(host_out, want, (ds, band_rows, "host"))
    assert _guard_intact(big, img)


# ---- the warp ----------------------------------------------------------------------------------------------------------
SHAPES = [(33, 33), (20, 31), (70, 90), (40, 100)]
FORMS = ("image", "mask_nearest", "mask_bilinear")


@functools.lru_cache(maxsize=None)
def _arrays(H, W):
    rng = np.random.default_rng(H * 100 + W)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    mask = rng.integers(0, 256, (H, W), dtype=np.uint8)
    img.setflags(write=False)
    mask.setflags(write=False)
    return img, mask


def _forms(H, W):
    """(name, array, nearest as the wrapper takes it, fill) of the three forms."""
    img, mask = _arrays(H, W)
    return (("image", img, None, 255), ("mask_nearest", mask, None, 3), ("mask_bilinear", mask, False, 0))


def _transforms(H, W):
    """name -> six numbers: rotations with sub-pixel shifts, shifts that leave whole rows of fill, centres outside
    the region, and all six numbers at and beyond their clamps."""
    tab = dict(zip((0.3, -7.0, 31.0, 90.0, 180.0), rotation_table([0.3, -7.0, 31.0, 90.0, 180.0]).tolist()))
    out = {}
    for a, (c, s) in tab.items():
        out[f"rot{a}"] = (c, s, 0, 0, H - 1, W - 1)
        out[f"rot{a}_sub"] = (c, s, 16 * 2 + 5, -(16 * 3 + 9), H - 1, W - 1)
    c, s = tab[0.3]
    out["rows_of_fill"] = (c, s, 16 * (H - 3), 7, H - 1, W - 1)
    out["rows_of_fill_up"] = (ONE, 0, -16 * (H - 2) - 3, 0, H - 1, W - 1)
    c, s = tab[-7.0]
    out["centre_outside"] = (c, s, 16 * 5, -16 * 20, -40, 6 * W)
    out["centre_far"] = (tab[0.3][0], tab[0.3][1], 0, 0, 2 * H + 50, -3 * W)
    out["at_clamps"] = (ONE, ONE, 1 << 36, -(1 << 36), ONE, -ONE)
    out["beyond_clamps"] = (1 << 40, -(1 << 40), 1 << 50, (1 << 63) - 1, -(1 << 63), 1 << 30)
    out["cos_beyond"] = (1 << 30, 0, 0, 0, H - 1, W - 1)
    out["sin_beyond"] = (0, -(1 << 62), 16, -16, H - 1, W - 1)
    out["shift_at_clamp"] = (ONE, 0, -(1 << 36), 1 << 36, 0, 0)
    return out


@functools.lru_cache(maxsize=None)
def _want(H, W, name, form):
    arr, nearest, fill = next((a, n, f) for k, a, n, f in _forms(H, W) if k == form)
    want = G.warp(arr, _transforms(H, W)[name], nearest=nearest, fill=fill)
    want.setflags(write=False)
    return want


def _run(g, T, **kw):
    return rigid_warp(g, torch.tensor(T, dtype=torch.int64), **kw)


@pytest.mark.parametrize("H,W", SHAPES)
def test_the_four_identities(H, W):
    for form, arr, nearest, fill in _forms(H, W):
        g, big = _view(arr)
        kw = dict(nearest=nearest, fill=fill)
        _same(_run(g, (ONE, 0, 0, 0, H - 1, W - 1), **kw), arr, (form, "copy"))
        _same(_run(g, (-ONE, 0, 0, 0, H - 1, W - 1), **kw), arr[::-1, ::-1], (form, "flip"))
        for dy, dx in ((3, -5), (-7, 2), (H, 0), (0, -W), (1, 1)):
            out = _run(g, (ONE, 0, 16 * dy, 16 * dx, H - 1, W - 1), **kw)
            sh = torch.tensor([[dy, dx]], dtype=torch.int32, device=DEV)
            assert torch.equal(out, shift_tiles(g[None], sh, fill)[0]), (form, dy, dx)
            _same(out, Wr.shifted(arr, dy, dx, fill), (form, dy, dx))
        if H == W:
            _same(_run(g, (0, ONE, 0, 0, H - 1, H - 1), **kw), np.rot90(arr, -1), (form, "quarter turn"))
        assert _guard_intact(big, arr)


@pytest.mark.parametrize("H,W", SHAPES)
def test_warp_equals_the_restatement(H, W):
    names = list(_transforms(H, W))
    for form, arr, nearest, fill in _forms(H, W):
        g, big = _view(arr)
        plain = _t(arr).to(DEV)
        for name in names:
            want = _want(H, W, name, form)
            T = torch.tensor(_transforms(H, W)[name], dtype=torch.int64)
            out = rigid_warp(g, T, nearest=nearest, fill=fill)
            assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous() and tuple(out.shape) == arr.shape
            _same(out, want, (form, name))
            assert torch.equal(rigid_warp(g, T, nearest=nearest, fill=fill), out)                  # two identical runs
            assert torch.equal(rigid_warp(plain, T.to(DEV), nearest=nearest, fill=fill), out)      # a device transform
        assert (_want(H, W, "rows_of_fill", form)[5:] == fill).all()                               # whole rows of fill
        assert (_want(H, W, "rows_of_fill_up", form)[:H - 3] == fill).all()
        assert (_want(H, W, "rows_of_fill", form)[:2] != fill).any()
        assert (_want(H, W, "at_clamps", form) == fill).all()
        assert np.array_equal(_want(H, W, "cos_beyond", form), arr)
        assert _guard_intact(big, arr)


@pytest.mark.parametrize("H,W", [(33, 33), (70, 90)])
def test_a_batch_of_five_transforms_is_one_launch(H, W):
    names = ["rot0.3_sub", "rot-7.0", "rot31.0_sub", "centre_outside", "beyond_clamps"]
    T5 = torch.tensor([_transforms(H, W)[n] for n in names], dtype=torch.int64)
    for form, arr, nearest, fill in _forms(H, W):
        g, big = _view(arr)
        for T in (T5, T5.to(DEV)):
            out = rigid_warp(g, T, nearest=nearest, fill=fill)
            assert tuple(out.shape) == (5,) + arr.shape and out.is_contiguous()
            for k, name in enumerate(names):
                _same(out[k], _want(H, W, name, form), (form, name))
        _same(rigid_warp(g, T5[:1], nearest=nearest, fill=fill)[0], _want(H, W, names[0], form), form)
        _same(rigid_warp(g, T5, nearest=nearest, fill=fill, band_rows=7)[3], _want(H, W, names[3], form), form)
        assert _guard_intact(big, arr)


@functools.lru_cache(maxsize=None)
def _field_case():
    H, W, cell = 70, 90, 32
    rng = np.random.default_rng(32)
    D = rng.integers(-16 * 9, 16 * 9 + 1, (H // cell, W // cell, 2)).astype(np.int32)     # beyond max_shift 6 too
    D.setflags(write=False)
    return H, W, cell, D, 6


def test_identity_transform_with_a_field_is_warp_region():
    H, W, cell, D, ms = _field_case()
    field = _t(D).to(DEV)
    T = torch.tensor([ONE, 0, 0, 0, H - 1, W - 1], dtype=torch.int64)
    for form, arr, nearest, fill in _forms(H, W)[:2]:
        g, big = _view(arr)
        out = rigid_warp(g, T, field=field, cell=cell, max_shift=ms, fill=fill)
        assert torch.equal(out, warp_region(g, field, cell, max_shift=ms, fill=fill)), form
        _same(out, Wr.warp(arr, D, cell, ms, fill), form)
        assert _guard_intact(big, arr)
    wild = D.copy()
    wild.reshape(-1)[:3] = (2 ** 31 - 1, -2 ** 31, 10 ** 9)                               # any values: the clamp holds
    img = _arrays(H, W)[0]
    _same(rigid_warp(_t(img).to(DEV), T, field=_t(wild).to(DEV), cell=cell, max_shift=ms), Wr.warp(img, wild, cell, ms), "wild")


@pytest.mark.parametrize("name", ["rot0.3_sub", "rot-7.0", "rot90.0_sub", "centre_outside", "beyond_clamps"])
def test_a_rigid_transform_plus_a_field(name):
    H, W, cell, D, ms = _field_case()
    field = _t(D).to(DEV)
    stack = torch.full(tuple(D.shape[:2]) + (3, 2), 10 ** 6, dtype=torch.int32, device=DEV)
    strided = stack[:, :, 1, :]                                # a non-contiguous field: the call works on a copy of it
    strided.copy_(field)
    assert not strided.is_contiguous()
    six = _transforms(H, W)[name]
    T = torch.tensor(six, dtype=torch.int64)
    for form, arr, nearest, fill in _forms(H, W):
        g, big = _view(arr)
        want = G.warp(arr, six, D, cell, ms, nearest=nearest, fill=fill)
        kw = dict(cell=cell, max_shift=ms, nearest=nearest, fill=fill)
        for band_rows in (None, 7):
            _same(rigid_warp(g, T, field=field, band_rows=band_rows, **kw), want, (form, name, band_rows))
            _same(rigid_warp(g, T, field=strided, band_rows=band_rows, **kw), want, (form, name, band_rows, "strided"))
        for f, what in ((field, "host"), (strided, "host, strided")):
            host = rigid_warp(_t(arr), T, field=f, band_rows=7, **kw)
            assert not host.is_cuda
            _same(host, want, (form, name, what))
        assert _guard_intact(big, arr)
    assert (stack[:, :, 0] == 10 ** 6).all() and (stack[:, :, 2] == 10 ** 6).all() and torch.equal(strided, field)


@pytest.mark.parametrize("H,W", [(20, 31), (70, 90)])
def test_warp_banding_and_host_input_do_not_change_a_byte(H, W):
    for form, arr, nearest, fill in _forms(H, W):
        g, big = _view(arr)
        host = _t(arr)
        for name in ("rot0.3_sub", "rot31.0_sub", "rot90.0", "rot180.0_sub", "rows_of_fill", "centre_outside", "at_clamps"):
            want = _want(H, W, name, form)
            T = torch.tensor(_transforms(H, W)[name], dtype=torch.int64)
            for band_rows in (1, 7, H, None):
                dev_out = rigid_warp(g, T, nearest=nearest, fill=fill, band_rows=band_rows)
                host_out = rigid_warp(host, T, nearest=nearest, fill=fill, band_rows=band_rows)
                assert dev_out.is_cuda and not host_out.is_cuda and host_out.is_contiguous()
                _same(dev_out, want, (form, name, band_rows, "gpu"))
                _same(host_out, want, (form, name, band_rows, "host"))
            _same(rigid_warp(host, T.to(DEV), nearest=nearest, fill=fill, band_rows=7), want, (form, name, "device T"))
        assert _guard_intact(big, arr)


# ---- the search --------------------------------------------------------------------------------------------------------
RIGID_KW = {"downsample": G.SEARCH["ds"], "radius": G.SEARCH["radius"], "angles": G.SEARCH_ANGLES}


@functools.lru_cache(maxsize=None)
def _table():
    return rotation_table(G.SEARCH_ANGLES).tolist()


@functools.lru_cache(maxsize=None)
def _plant(n):
    angle, shift = G.PLANTS[n]
    src, tgt = G.planted(rotation_table([angle])[0].tolist(), shift)
    return src, tgt, G.register(src, tgt, _table(), G.SEARCH_ANGLES, **G.SEARCH)


def _check_rigid(got, want, what):
    for k, dt in (("transform", torch.int64), ("angle_index", torch.int32), ("shift", torch.int32),
                  ("shifts", torch.int32), ("valid", torch.int32)):
        assert got[k].dtype == dt and got[k].is_cuda, (what, k)
        _same(got[k], np.asarray(want[k]), (what, k))
    for k in ("angle", "score", "margin", "angle_margin", "scores"):
        assert got[k].dtype == torch.float64 and got[k].is_cuda, (what, k)
        _close(got[k].cpu().numpy(), want[k], f"{what} {k}")
    assert tuple(got["transform"].shape) == (6,) and tuple(got["shift"].shape) == (2,) and got["score"].dim() == 0


@pytest.mark.parametrize("n", range(len(G.PLANTS)))
def test_register_rigid_recovers_the_planted_pair(n):
    src, tgt, want = _plant(n)
    (gs, bs), (gt, bt) = _view(src), _view(tgt)
    got = register_rigid(gs, gt, **RIGID_KW)
    _check_rigid(got, want, f"plant {n}")
    assert int(got["angle_index"]) == G.SEARCH_ANGLES.index(G.PLANTS[n][0]) and int(got["valid"]) == 1
    a, b, bk = want["maps"]
    _same(structure_overview(gs, 2), a, "a")
    _same(structure_overview(gt, 2, stains="hdab"), b, "b")
    Tk = torch.tensor(G.overview_transforms(_table(), *a.shape), dtype=torch.int64)
    _same(rigid_warp(_view(b)[0], Tk, nearest=False, fill=0), bk, "b_k")
    host = register_rigid(_t(src), _t(tgt), **RIGID_KW)
    _check_rigid(host, want, f"plant {n} host")
    assert _guard_intact(bs, src) and _guard_intact(bt, tgt)


def test_a_flat_source_is_invalid_and_gives_the_identity():
    src, tgt, _ = _plant(0)
    flat = np.full_like(src, 255)
    want = G.register(flat, tgt, _table(), G.SEARCH_ANGLES, **G.SEARCH)
    got = register_rigid(_view(flat)[0], _view(tgt)[0], **RIGID_KW)
    _check_rigid(got, want, "flat")
    assert int(got["valid"]) == 0 and got["transform"].tolist() == [ONE, 0, 0, 0, 191, 191]
    assert int(got["angle_index"]) == -1 and float(got["score"]) == 0.0 and got["shift"].tolist() == [0, 0]


# ---- the composition ---------------------------------------------------------------------------------------------------
ALIGN_KW = {"radius": 6}


@functools.lru_cache(maxsize=None)
def _align_case():
    src, tgt, _ = _plant(0)
    mask = np.random.default_rng(6).integers(0, 4, tgt.shape[:2], dtype=np.uint8)
    mask.setflags(write=False)
    return src, tgt, mask, G.align(src, tgt, _table(), G.SEARCH_ANGLES, 64, masks=[mask], rigid=G.SEARCH, **ALIGN_KW)


def test_align_regions_equals_the_restatements_chain():
    src, tgt, mask, want = _align_case()
    (gs, bs), (gt, bt), (gm, bm) = _view(src), _view(tgt), _view(mask)
    dev = align_regions(gs, gt, 64, masks=[gm], rigid=RIGID_KW, **ALIGN_KW)
    host = align_regions(_t(src), _t(tgt), 64, masks=[_t(mask)], rigid=RIGID_KW, band_rows=50, **ALIGN_KW)
    for out, on_gpu in ((dev, True), (host, False)):
        assert out["aligned"].is_cuda == on_gpu and out["masks"][0].is_cuda == on_gpu and len(out["masks"]) == 1
        _same(out["transform"], want["transform"], "transform")
        _same(out["field"], want["field"], "field")
        _same(out["kept"], want["kept"], "kept")
        assert out["stats"].tolist() == want["stats"].tolist()
        _same(out["aligned"], want["aligned"], "aligned")
        _same(out["masks"][0], want["masks"][0], "mask")
        _close(out["score"].cpu().numpy(), want["score"], "cell scores")
        _close(out["rigid_score"].cpu().numpy(), want["rigid_score"], "rigid score")
        assert float(out["angle"]) == want["angle"] == 3.0 and int(out["rigid_valid"]) == 1
    _same(rigid_warp(gt, dev["transform"]), want["intermediate"], "intermediate")
    assert _guard_intact(bs, src) and _guard_intact(bt, tgt) and _guard_intact(bm, mask)


# ---- no hidden synchronisation -----------------------------------------------------------------------------------------
def test_rigid_alignment_does_not_synchronise():
    src, tgt, mask, want = _align_case()
    gs, gt, gm = _view(src)[0], _view(tgt)[0], _view(mask)[0]
    align_regions(gs, gt, 64, masks=[gm], rigid=RIGID_KW, **ALIGN_KW)       # the library is loaded from here on
    T5 = torch.tensor([_transforms(192, 192)[n] for n in ("rot0.3_sub", "rot-7.0")], dtype=torch.int64)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        rg = register_rigid(gs, gt, **RIGID_KW)
        mid = rigid_warp(gt, rg["transform"], band_rows=40)
        two = rigid_warp(gm, T5, fill=0)
        out = align_regions(gs, gt, 64, masks=[gm], rigid=RIGID_KW, **ALIGN_KW)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    _same(rg["transform"], want["transform"], "transform")
    _same(mid, want["intermediate"], "intermediate")
    _same(out["aligned"], want["aligned"], "aligned")
    _same(out["masks"][0], want["masks"][0], "mask")
    assert tuple(two.shape) == (2, 192, 192)
