"""The paired tile registration (csrc/registration.hip) against the numpy restatement of
tests/registration_ref.py, on poisoned memory (every ``torch.empty`` starts as NaN / 0xFF, as in
tests/test_augment_gpu.py).  The inputs are crop views with an odd row pitch and an unaligned base inside a guard band
of a constant byte, so a wrong index shows as a wrong value.

What must hold.  Structure maps, ``tsum`` and ``sums`` are integers: bit-equal.  ``shift`` and ``valid`` are exact: the
restatement's best score leads its second best by more than 1e-3 on every case (tests/test_registration_cpu.py checks
that on the restatement alone), far more than the last bits in which two correctly rounded ``sqrt`` and ``/`` may
differ.  Scores agree within 1e-12 relative (an absolute 1e-15 where the value is 0): one float64 division and one
square root on equal integers."""
import functools

import numpy as np
import pytest
import torch

import registration_ref as R
import stain_quant_ref as Q
from stain2stain_amd import (image_quality, overlap_boxes, region_shift_field, register_pairs, registered_quality,
                             shift_tiles, structure_map)

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
    """A uint8 batch [B, H, W, 3] or [B, H, W] as a crop view of a larger GPU array of GUARD bytes: odd row pitch,
    unaligned base.  Returns (view, the larger array)."""
    B, H, W = arr.shape[:3]
    pad = 6 if (W + 6) % 4 != 0 else 7
    big = torch.full((B, H + 5, W + pad) + arr.shape[3:], GUARD, dtype=torch.uint8, device=DEV)
    view = big[:, 2:2 + H, 3:3 + W]
    view.copy_(torch.from_numpy(np.ascontiguousarray(arr)))
    assert view.stride(1) % 4 != 0 and view.data_ptr() % 4 != 0
    return view, big


def _guard_intact(big, arr):
    B, H, W = arr.shape[:3]
    g = big.clone()
    g[:, 2:2 + H, 3:3 + W] = GUARD
    return bool((g == GUARD).all()) and np.array_equal(big[:, 2:2 + H, 3:3 + W].cpu().numpy(), arr)


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want)
    bound = np.where(want == 0.0, 1e-15, 1e-12 * np.abs(want))
    print(f"{what}: largest error {err.max():.3e} (largest bound {bound.max():.3e})")
    assert got.shape == want.shape and (err <= bound).all(), what


def _check_level(got, want, what):
    """A register_pairs(return_surface=True) result against the restatement's level."""
    for k in ("tsum", "sums"):
        assert got[k].dtype == torch.int64 and np.array_equal(got[k].cpu().numpy(), want[k]), (what, k)
    assert got["shift"].dtype == torch.int32 and np.array_equal(got["shift"].cpu().numpy(), want["shift"]), what
    assert got["valid"].dtype == torch.int32 and np.array_equal(got["valid"].cpu().numpy(), want["valid"]), what
    for k in ("score", "score_center", "margin", "scores"):
        assert got[k].dtype == torch.float64
        _close(got[k].cpu().numpy(), want[k], f"{what} {k}")


@functools.lru_cache(maxsize=None)
def _case(name):
    src, tgt, planted, kw = R.case(name)
    return src, tgt, planted, kw, R.register(src, tgt, **kw)


# ---- the table -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_table_case(name):
    src, tgt, planted, kw, want = _case(name)
    (gs, bs), (gt, bt) = _view(src), _view(tgt)
    ds = kw["downsample"]
    for g, img, stains in ((gs, src, "hed"), (gt, tgt, "hdab")):
        m = structure_map(g, stains, downsample=ds)
        ref = R.structure(img, R.weights(stains), ds)
        assert m.dtype == torch.uint8 and m.is_contiguous() and tuple(m.shape) == ref.shape
        assert np.array_equal(m.cpu().numpy(), ref), (name, stains)
        assert ref.min() < 10 and ref.max() > 60             # the maps are not flat
    got = register_pairs(gs, gt, return_surface=True, **kw)
    _check_level(got, want, name)
    assert np.array_equal(got["shift"].cpu().numpy(), planted)
    again = register_pairs(gs, gt, return_surface=True, **kw)
    assert all(torch.equal(got[k], again[k]) for k in got)
    # contiguous, aligned input: the same integers
    flat = register_pairs(torch.from_numpy(src).to(DEV), torch.from_numpy(tgt).to(DEV), return_surface=True, **kw)
    assert all(torch.equal(got[k], flat[k]) for k in got)
    assert _guard_intact(bs, src) and _guard_intact(bt, tgt)


def test_two_level_without_refinement_returns_the_coarse_level():
    src, tgt, planted, kw, _ = _case("two_level")
    kw = dict(kw, refine=False)
    want = R.register(src, tgt, **kw)
    got = register_pairs(_view(src)[0], _view(tgt)[0], return_surface=True, **kw)
    _check_level(got, want, "coarse only")
    assert (np.abs(want["shift"] - planted) <= 2).all() and (want["shift"] % 4 == 0).all()


def test_fp32_input_goes_through_the_save_conversion():
    src, tgt, planted, kw, _ = _case("aligned")
    fs, ft = ((torch.from_numpy(x).permute(0, 3, 1, 2).float() / 255.0 - 0.5) / 0.5 for x in (src, tgt))
    qs, qt = Q.nchw_to_u8(fs.numpy()), Q.nchw_to_u8(ft.numpy())
    want = R.register(qs, qt, **kw)
    got = register_pairs(fs.to(DEV), ft.to(DEV), return_surface=True, **kw)
    _check_level(got, want, "fp32")
    assert np.array_equal(structure_map(fs.to(DEV), "hed").cpu().numpy(), R.structure(qs, R.weights("hed")))


# ---- ties, degenerate input, centres ------------------------------------------------------------------------------------
def test_ties_are_broken_by_the_total_order():
    """A target that is periodic with period 4 in x and in y: windows 4 apart hold identical bytes, so identical sums and
    identical scores.  The pick is the one the total order names."""
    rng = np.random.default_rng(3)
    cell = Q.synthesise(rng.uniform(0, 1.2, (4, 4, 3)) * [1.0, 1.0, 0.0], "hdab")
    img = np.tile(cell, (12, 13, 1))[None].repeat(3, 0)       # [3, 48, 52, 3]
    center = np.array([[2, 2], [0, 0], [-2, 1]], np.int32)
    want = R.register(img, img, radius=5, center=center, src_stains="hdab", tgt_stains="hdab")
    for s in range(3):
        assert (want["scores"][s] == want["scores"][s].max()).sum() >= 4         # there are ties to break
    assert want["shift"].tolist() == [[0, 0], [0, 0], [-4, 0]]
    g, _ = _view(img)
    got = register_pairs(g, g, radius=5, center=torch.from_numpy(center).to(DEV), src_stains="hdab", tgt_stains="hdab",
                         return_surface=True)
    _check_level(got, want, "ties")
    sc = got["scores"].cpu().numpy()
    assert (sc[:, 1, 1] == sc[:, 5, 5]).all() and (sc[:, 1, 5] == sc[:, 5, 9]).all()    # identical, not merely close


def test_flat_tiles_are_invalid():
    src, tgt, _, _, _ = _case("aligned")
    flat = np.full_like(src[:1], 200)
    s = np.concatenate([flat, src[1:2], src[2:]])
    t = np.concatenate([tgt[:1], np.full_like(tgt[:1], 230), tgt[2:]])
    want = R.register(s, t, radius=8)
    assert want["valid"].tolist() == [0, 1, 1] and want["shift"].tolist()[:2] == [[0, 0], [0, 0]]
    got = register_pairs(_view(s)[0], _view(t)[0], radius=8, return_surface=True)
    _check_level(got, want, "flat")
    assert got["score"][:2].tolist() == [0.0, 0.0] and got["margin"][:2].tolist() == [0.0, 0.0]
    assert got["score_center"][:2].tolist() == [0.0, 0.0] and got["shift"][:2].tolist() == [[0, 0], [0, 0]]


def test_device_centres_never_move_a_read_outside_the_maps():
    src, tgt, planted, _, _ = _case("corners")
    center = np.array([[1000, -1000], [-2147483648, 2147483647], [1, -1]], np.int32)
    want = R.register(src, tgt, radius=5, center=center)
    assert want["valid"].tolist() == [0, 0, 1]
    assert want["shift"].tolist() == [[1000, -1000], [-2147483648, 2147483647], [0, 0]]
    (gs, bs), (gt, bt) = _view(src), _view(tgt)
    got = register_pairs(gs, gt, radius=5, center=torch.from_numpy(center).to(DEV), return_surface=True)
    _check_level(got, want, "centres")
    assert not got["sums"][:2].any() and not got["tsum"][:2].any()
    assert _guard_intact(bs, src) and _guard_intact(bt, tgt)
    # a centre next to the largest that leaves a template: 70 x 90 at R = 5 has two rows left at |cy| = 29
    edge = np.array([[29, 0], [-29, 39], [30, 0]], np.int32)
    want = R.register(src, tgt, radius=5, center=edge)
    assert want["tsum"][:, 0].tolist() == [2 * 80, 2 * 2, 0]
    got = register_pairs(gs, gt, radius=5, center=torch.from_numpy(edge).to(DEV), return_surface=True)
    _check_level(got, want, "edge centres")


def test_radius_zero_is_one_score_per_pair():
    src, tgt, _, _, _ = _case("aligned")
    want = R.register(src, tgt, radius=0)
    got = register_pairs(_view(src)[0], _view(tgt)[0], radius=0, return_surface=True)
    _check_level(got, want, "R = 0")
    assert tuple(got["scores"].shape) == (3, 1, 1) and torch.equal(got["score"], got["score_center"])
    assert got["shift"].tolist() == [[0, 0]] * 3 and got["margin"].tolist() == [0.0] * 3


def test_wide_template_takes_more_than_one_chunk_and_band():
    """300 template columns (two column chunks of the sums kernel, the second 44 wide) by 40 rows (two bands)."""
    rng = np.random.default_rng(8)
    a = rng.integers(0, 256, (2, 46, 306, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (2, 46, 306, 3), dtype=np.uint8)
    want = R.register(a, b, radius=3)
    got = register_pairs(_view(a)[0], _view(b)[0], radius=3, return_surface=True)
    _check_level(got, want, "wide")


# ---- shift_tiles, overlap_boxes -------------------------------------------------------------------------------------------
def _shifted(img, shift, fill):
    out = np.full_like(img, fill)
    H, W = img.shape[1:3]
    for n, (dy, dx) in enumerate(shift):
        ys = [y for y in range(H) if 0 <= y + dy < H]
        xs = [x for x in range(W) if 0 <= x + dx < W]
        if ys and xs:
            out[n, ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] = img[n, ys[0] + dy:ys[-1] + 1 + dy, xs[0] + dx:xs[-1] + 1 + dx]
    return out


def test_shift_tiles_and_overlap_boxes():
    rng = np.random.default_rng(2)
    shift = [[0, 0], [3, -2], [-7, 11], [37, 0], [0, -41], [36, 40], [-2147483648, 2147483647], [1, 1]]
    img = rng.integers(0, 256, (8, 37, 41, 3), dtype=np.uint8)
    mask = rng.integers(0, 256, (8, 37, 41), dtype=np.uint8)
    sh = torch.tensor(shift, dtype=torch.int32, device=DEV)
    for arr, fill in ((img, 255), (mask, 0), (img, 9)):
        g, big = _view(arr)
        out = shift_tiles(g, sh, fill)
        assert out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == arr.shape
        assert np.array_equal(out.cpu().numpy(), _shifted(arr, shift, fill))
        assert torch.equal(shift_tiles(torch.from_numpy(arr).to(DEV), sh, fill), out)     # aligned input
        assert _guard_intact(big, arr)
    boxes = overlap_boxes(sh, 37, 41)
    assert boxes.is_cuda and torch.equal(boxes.cpu(), overlap_boxes(sh.cpu(), 37, 41))
    assert boxes[1].tolist() == [0, 2, 34, 39] and boxes[3].tolist()[2] == 0 and boxes[5].tolist()[2:] == [1, 1]
    for bad in (sh[:4], sh.long(), sh.cpu()):
        with pytest.raises(ValueError, match="shift"):
            shift_tiles(_view(img)[0], bad)
    with pytest.raises(ValueError, match="fill"):
        shift_tiles(_view(img)[0], sh, 256)


# ---- registered_quality, region_shift_field ---------------------------------------------------------------------------------
def test_registered_quality_scores_the_aligned_pair():
    rng = np.random.default_rng(12)
    H, W, r = 64, 72, 8
    big = np.stack([R.pair(H + 16, W + 16, 50 + n, 0, 0)[1] for n in range(2)])
    gen = big[:, 8:8 + H, 8:8 + W].astype(np.int32) + rng.integers(-6, 7, (2, H, W, 3))
    gen = np.clip(gen, 0, 255).astype(np.uint8)
    tgt = big[:, 5:5 + H, 10:10 + W]                           # tgt[y + 3, x - 2] is the tissue at gen[y, x]
    g, t = _view(gen)[0], _view(tgt)[0]
    got = registered_quality(g, t, radius=r)
    assert got["shift"].tolist() == [[3, -2], [3, -2]] and (got["score"] > 0.9).all()
    hand = image_quality(g[:, r:H - r, r:W - r], t[:, r + 3:H - r + 3, r - 2:W - r - 2])
    for k in ("psnr", "ssim", "mae", "mse"):
        assert torch.equal(got[k], hand[k]), k
    plain = image_quality(g, t)
    assert (got["psnr"] > plain["psnr"] + 3.0).all() and (got["ssim"] > plain["ssim"]).all()
    with pytest.raises(ValueError, match="quantize"):
        registered_quality(g, t, radius=r, quantize=False)


def test_region_shift_field_recovers_a_shift_per_cell():
    cell, planted = 64, [[(2, -3), (-4, 1), (0, 5)], [(5, 5), (-1, -6), (3, 0)]]
    src = np.full((2 * cell + 9, 3 * cell + 5, 3), 255, np.uint8)             # a ragged edge that is not searched
    tgt = np.full_like(src, 255)
    want = np.zeros((2, 3, 2), np.int32)
    for gy in range(2):
        for gx in range(3):
            s, t = R.pair(cell, cell, 70 + 3 * gy + gx, *planted[gy][gx])
            sl = (slice(gy * cell, (gy + 1) * cell), slice(gx * cell, (gx + 1) * cell))
            src[sl], tgt[sl] = s, t
            ref = R.register(s[None], t[None], radius=8)
            assert R.runner_up_gap(ref["scores"][0], 8) > 1e-3
            want[gy, gx] = ref["shift"][0]
    assert want.tolist() == [[list(p) for p in row] for row in planted]
    host = region_shift_field(torch.from_numpy(src), torch.from_numpy(tgt), cell=cell, radius=8)
    gs = torch.full((src.shape[0] + 3, src.shape[1] + 2, 3), GUARD, dtype=torch.uint8, device=DEV)
    gt = gs.clone()
    gs[1:-2, 1:-1], gt[1:-2, 1:-1] = torch.from_numpy(src).to(DEV), torch.from_numpy(tgt).to(DEV)
    dev = region_shift_field(gs[1:-2, 1:-1], gt[1:-2, 1:-1], cell=cell, radius=8)
    mixed = region_shift_field(gs[1:-2, 1:-1], torch.from_numpy(tgt), cell=cell, radius=8)
    for out in (host, dev, mixed):
        assert tuple(out["shift"].shape) == (2, 3, 2) and out["shift"].is_cuda
        assert np.array_equal(out["shift"].cpu().numpy(), want) and bool(out["valid"].all())
        assert tuple(out["score"].shape) == (2, 3) and (out["margin"] > 1e-3).all()
        assert all(torch.equal(out[k], host[k]) for k in host)


# ---- no hidden synchronisation ----------------------------------------------------------------------------------------------
def test_registration_does_not_synchronise():
    src, tgt, _, kw, _ = _case("two_level")
    gs, gt = _view(src)[0], _view(tgt)[0]
    out = register_pairs(gs, gt, **kw)                          # the library is loaded from here on
    shift_tiles(gt, out["shift"])
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = register_pairs(gs, gt, return_surface=True, **kw)
        moved = shift_tiles(gt, out["shift"])
        boxes = overlap_boxes(out["shift"], 96, 100)
        m = structure_map(gs, downsample=2)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert out["shift"].tolist() == [[-13, 9]] * 3 and int(moved.sum()) > 0 and int(m.sum()) > 0
    assert boxes.tolist() == [[13, 0, 83, 91]] * 3
