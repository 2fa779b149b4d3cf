"""The fused paired augmentation (csrc/augment.hip) against the numpy restatement of tests/augment_ref.py, on poisoned
memory (every ``torch.empty`` starts as NaN / 0xFF, as in tests/test_stain_norm_gpu.py).  The inputs are crop views with
an odd row pitch and an unaligned base inside a guard band of a constant byte, so a wrong index shows as a wrong value.

Tolerances.  The geometry, the mask, the byte path, identity maps and ``white`` are exact: bit for bit.
Jittered bytes follow the rule of section 3.18: the kernel evaluates in fp32 what the restatement evaluates in float64
from the same fp32 constants, a few 1e-4 levels apart, so the bytes are equal wherever the restatement's unrounded level
lies more than 1e-3 from a half-integer and at most one level apart elsewhere.  The share of pixels with a channel in that
band is a condition on the input, computed from the restatement alone: below 1.5 % for images of 1 500 pixels or more (a
numpy run on 1 961 to 41 200 pixel images gave 0.6 % on average and at most 0.97 % over 40 draws); smaller cases are
not capped."""
import random

import numpy as np
import pytest
import torch

import augment_ref as A
from stain2stain_amd import (PairedAugmenter, fit_stains, paired_augment, sample_d4_params, sample_stain_jitter,
                             stain_augment, stain_jitter_maps)
from stain2stain_amd.data import paired_crop_flip_normalize

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 77
IDENT = [[1.0, 1.0, 1.0, 0.0, 0.0, 0.0]]


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
    unaligned base."""
    B, H, W = arr.shape[:3]
    pad = 6 if (W + 6) % 4 != 0 else 7
    big = torch.full((B, H + 5, W + pad) + arr.shape[3:], GUARD, dtype=torch.uint8, device=DEV)
    view = big[:, 2:2 + H, 3:3 + W]
    view.copy_(torch.from_numpy(np.ascontiguousarray(arr)))
    assert view.stride(1) % 4 != 0 and view.data_ptr() % 4 != 0
    return view


def _params(rows):
    return torch.tensor(rows, dtype=torch.int32)


@pytest.fixture(scope="module")
def he():
    """Three 70 x 90 synthetic H&E pairs and a class mask of random bytes, their GPU views, and a fitted basis."""
    rng = np.random.default_rng(5)
    src = np.stack([A.synthetic_he(70, 90, 31 + n)[0] for n in range(3)])
    tgt = np.stack([A.synthetic_he(70, 90, 41 + n)[0] for n in range(3)])
    mask = rng.integers(0, 256, (3, 70, 90), dtype=np.uint8)
    fit = fit_stains(torch.from_numpy(A.synthetic_he(96, 96, 1)[0]).to(DEV))
    return {"src": src, "tgt": tgt, "mask": mask, "gsrc": _view(src), "gtgt": _view(tgt), "gmask": _view(mask),
            "fitted": fit.vectors}


# the far corners of the 70 x 90 images at S = 64: top = H - S = 6, left = W - S = 26
P4 = [[6, 26, 1, 0], [0, 0, 0, 1], [3, 11, 1, 1]]
P5 = [[6, 26, 1, 0, 1], [0, 26, 0, 1, 0], [6, 0, 1, 1, 1]]


def _check_bytes(got, want, raw, what):
    band = A.half_band(raw)
    share = band.any(-1).mean()
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    pixels = band[..., 0].size
    print(f"{what}: {int((diff != 0).sum())} of {diff.size} bytes differ, {share:.2%} of {pixels} pixels are exempt")
    if pixels >= 1500:
        assert share < 0.015, what                                 # a condition on the input, from the restatement alone
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert (diff[~band] == 0).all() and diff.max() <= 1, what


# ---- exact: the byte path and the geometry -----------------------------------------------------------------------------
def test_without_maps_equals_paired_crop_flip_normalize(he):
    p = _params(P4)
    old_s, old_t = paired_crop_flip_normalize(torch.from_numpy(he["src"]).to(DEV), torch.from_numpy(he["tgt"]).to(DEV),
                                              p, 64)
    out = paired_augment(he["gsrc"], he["gtgt"], p, 64)
    assert len(out) == 2
    for got, old in zip(out, (old_s, old_t)):
        assert got.dtype == torch.float32 and tuple(got.shape) == (3, 3, 64, 64) and got.is_contiguous()
        assert torch.equal(got, old)
    # and on aligned, contiguous input (the dword loads)
    out = paired_augment(torch.from_numpy(he["src"]).to(DEV), torch.from_numpy(he["tgt"]).to(DEV), p, 64)
    assert torch.equal(out[0], old_s) and torch.equal(out[1], old_t)


@pytest.mark.parametrize("S,H,W", [(1, 4, 6), (5, 8, 11), (31, 34, 37), (33, 33, 33), (64, 70, 90)])
def test_all_eight_symmetries(S, H, W):
    rng = np.random.default_rng(S)
    src = rng.integers(0, 256, (8, H, W, 3), dtype=np.uint8)
    tgt = rng.integers(0, 256, (8, H, W, 3), dtype=np.uint8)
    mask = rng.integers(0, 256, (8, H, W), dtype=np.uint8)
    rows = [[(H - S) if n % 3 == 0 else int(rng.integers(0, H - S + 1)),
             (W - S) if n % 3 != 1 else int(rng.integers(0, W - S + 1)), h, v, t] for n, (h, v, t) in enumerate(A.SYMMETRIES)]
    p = _params(rows)
    s, t, m, s8, t8 = paired_augment(_view(src), _view(tgt), p, S, mask_u8=_view(mask), mask_dtype=torch.uint8,
                                     return_u8=True)
    want_s, want_t, want_m = (A.augment(x, rows, S)[0] for x in (src, tgt, mask))
    assert np.array_equal(s8.cpu().numpy(), want_s) and np.array_equal(t8.cpu().numpy(), want_t)
    assert tuple(m.shape) == (8, 1, S, S) and np.array_equal(m[:, 0].cpu().numpy(), want_m)
    assert np.array_equal(s.cpu().numpy(), A.network(want_s)) and np.array_equal(t.cpu().numpy(), A.network(want_t))
    # contiguous, aligned input takes the dword loads: the same values
    again = paired_augment(torch.from_numpy(src).to(DEV), torch.from_numpy(tgt).to(DEV), p, S,
                           mask_u8=torch.from_numpy(mask).to(DEV), mask_dtype=torch.uint8, return_u8=True)
    for a, b in zip(again, (s, t, m, s8, t8)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8, torch.int64])
def test_mask_dtypes(he, dtype):
    out = paired_augment(he["gsrc"], he["gtgt"], _params(P5), 64, mask_u8=he["gmask"], mask_dtype=dtype)
    assert len(out) == 3
    m = out[2]
    assert m.dtype == dtype and tuple(m.shape) == (3, 1, 64, 64) and m.is_contiguous()
    want = A.augment(he["mask"], P5, 64)[0]
    assert want.min() == 0 and want.max() == 255
    assert np.array_equal(m[:, 0].cpu().numpy(), want.astype(m[:, 0].cpu().numpy().dtype))
    assert np.array_equal(out[0].cpu().numpy(), A.network(A.augment(he["src"], P5, 64)[0]))


@pytest.mark.parametrize("S,H,W", [(5, 8, 11), (33, 33, 33)])
def test_identity_maps_return_the_bytes(S, H, W):
    rng = np.random.default_rng(100 + S)
    src = rng.integers(0, 256, (8, H, W, 3), dtype=np.uint8)
    tgt = rng.integers(0, 256, (8, H, W, 3), dtype=np.uint8)
    src[:, ::3, ::2] = 0                                           # 0 takes the table entry of 1
    rows = [[H - S, W - S, h, v, t] for h, v, t in A.SYMMETRIES]
    ms, mt = stain_jitter_maps(IDENT * 8, "hed"), stain_jitter_maps(IDENT * 8, "hdab")
    s, t, s8, t8 = paired_augment(_view(src), _view(tgt), _params(rows), S, src_map=ms, tgt_map=mt, return_u8=True)
    want_s, want_t = (np.maximum(A.augment(x, rows, S)[0], 1) for x in (src, tgt))
    assert (want_s == 1).any()
    assert np.array_equal(s8.cpu().numpy(), want_s) and np.array_equal(t8.cpu().numpy(), want_t)
    assert np.array_equal(s.cpu().numpy(), A.network(want_s)) and np.array_equal(t.cpu().numpy(), A.network(want_t))


# ---- jittered bytes: the rule of section 3.18 ----------------------------------------------------------------------------
@pytest.mark.parametrize("sigmas", [(0.05, 0.01), (0.2, 0.05)])
def test_jittered_bytes_against_the_float64_restatement(he, sigmas):
    rng = random.Random(2018)
    js, jt = sample_stain_jitter(3, *sigmas, rng), sample_stain_jitter(3, *sigmas, rng)
    ms, mt = stain_jitter_maps(js, "hed"), stain_jitter_maps(jt, "hdab")
    s, t, s8, t8 = paired_augment(he["gsrc"], he["gtgt"], _params(P5), 64, src_map=ms, tgt_map=mt, return_u8=True)
    for name, img, maps, got8, got in (("source", he["src"], ms, s8, s), ("target", he["tgt"], mt, t8, t)):
        want, raw = A.augment(img, P5, 64, maps.numpy())
        assert (want != A.augment(img, P5, 64)[0]).mean() > 0.05                  # the jitter does move the bytes
        _check_bytes(got8.cpu().numpy(), want, raw, f"{name} {sigmas}")
        assert got8.is_contiguous() and tuple(got8.shape) == (3, 64, 64, 3)
        assert np.array_equal(got.cpu().numpy(), A.network(got8.cpu().numpy()))   # the fp32 outputs are those bytes
    # two runs give the same result
    again = paired_augment(he["gsrc"], he["gtgt"], _params(P5), 64, src_map=ms, tgt_map=mt, return_u8=True)
    for a, b in zip(again, (s, t, s8, t8)):
        assert torch.equal(a, b)
    # a map on one image kind leaves the other on the byte path
    only = paired_augment(he["gsrc"], he["gtgt"], _params(P5), 64, src_map=ms, return_u8=True)
    assert torch.equal(only[2], s8) and np.array_equal(only[3].cpu().numpy(), A.augment(he["tgt"], P5, 64)[0])


def test_white_keeps_glass(he):
    js = sample_stain_jitter(3, 0.2, 0.05, random.Random(9))
    ms, mt = stain_jitter_maps(js, "hed"), stain_jitter_maps(js, "hdab")
    kw = {"src_map": ms, "tgt_map": mt, "return_u8": True}
    plain = paired_augment(he["gsrc"], he["gtgt"], _params(P5), 64, **kw)
    gated = paired_augment(he["gsrc"], he["gtgt"], _params(P5), 64, white=230, **kw)
    for k, img in ((2, he["src"]), (3, he["tgt"])):
        geo = A.augment(img, P5, 64)[0]
        glass = geo.min(-1) >= 230
        assert 0.05 < glass.mean() < 0.6
        g, pl = gated[k].cpu().numpy(), plain[k].cpu().numpy()
        assert np.array_equal(g[glass], geo[glass]) and np.array_equal(g[~glass], pl[~glass])
        assert (pl[glass] != geo[glass]).any()
        assert np.array_equal(gated[k - 2].cpu().numpy(), A.network(g))
    # white = 0 keeps every pixel, white = None none
    kept = paired_augment(he["gsrc"], he["gtgt"], _params(P5), 64, white=0, **kw)
    assert np.array_equal(kept[2].cpu().numpy(), A.augment(he["src"], P5, 64)[0])


def test_a_sample_does_not_depend_on_its_batch_mates(he):
    j = sample_stain_jitter(3, 0.2, 0.05, random.Random(4))
    bases = ["hed", "hdab", he["fitted"]]
    maps = stain_jitter_maps(j, bases)
    assert not torch.equal(maps[0], stain_jitter_maps(j[:1], "hdab")[0])
    p = _params(P5)
    full = paired_augment(he["gsrc"], he["gtgt"], p, 64, mask_u8=he["gmask"], src_map=maps, tgt_map=maps.flip(0),
                          white=235, return_u8=True)
    for n in range(3):
        one = paired_augment(he["gsrc"][n:n + 1], he["gtgt"][n:n + 1], p[n:n + 1], 64, mask_u8=he["gmask"][n:n + 1],
                             src_map=stain_jitter_maps(j[n:n + 1], bases[n]), tgt_map=maps.flip(0)[n:n + 1].contiguous(),
                             white=235, return_u8=True)
        for a, b in zip(one, full):
            assert torch.equal(a[0], b[n]), n


# ---- stain_augment ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,seed", [(33, 7, 14), (40, 1030, 13)])
def test_stain_augment(H, W, seed):
    img = np.stack([A.synthetic_he(H, W, seed)[0], A.synthetic_he(H, W, seed + 50)[0]])
    maps = stain_jitter_maps(sample_stain_jitter(2, 0.2, 0.05, random.Random(seed)), ["hed", "hdab"])
    g = _view(img)
    out = stain_augment(g, maps)
    net = stain_augment(g, maps, network_input=True)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (2, H, W, 3) and out.is_contiguous()
    assert net.dtype == torch.float32 and tuple(net.shape) == (2, 3, H, W) and net.is_contiguous()
    want, raw = zip(*(A.mapped(img[n], maps[n].numpy()) for n in range(2)))
    _check_bytes(out.cpu().numpy(), np.stack(want), np.stack(raw), f"stain_augment {H}x{W}")
    assert np.array_equal(net.cpu().numpy(), A.network(out.cpu().numpy()))
    assert torch.equal(stain_augment(torch.from_numpy(img).to(DEV), maps), out)    # aligned input: the dword path
    # white, and the identity
    gated = stain_augment(g, maps, white=235).cpu().numpy()
    glass = img.min(-1) >= 235
    assert glass.any() and np.array_equal(gated[glass], img[glass])
    assert np.array_equal(gated[~glass], out.cpu().numpy()[~glass])
    ident = stain_augment(g, stain_jitter_maps(IDENT * 2, "hed"))
    assert np.array_equal(ident.cpu().numpy(), np.maximum(img, 1))


def test_stain_augment_equals_paired_augment_with_the_identity_geometry(he):
    j = sample_stain_jitter(3, 0.2, 0.05, random.Random(6))
    maps = stain_jitter_maps(j, "hed")
    sq_s, sq_t = he["gsrc"][:, 1:66, 20:85], he["gtgt"][:, 1:66, 20:85]            # 65 x 65 views: S = H = W
    zero = torch.zeros((3, 5), dtype=torch.int32)
    s, t, s8, t8 = paired_augment(sq_s, sq_t, zero, 65, src_map=maps, tgt_map=maps, white=240, return_u8=True)
    assert torch.equal(stain_augment(sq_s, maps, white=240), s8) and torch.equal(stain_augment(sq_t, maps, white=240), t8)
    assert torch.equal(stain_augment(sq_s, maps, white=240, network_input=True), s)


# ---- the augmenter ------------------------------------------------------------------------------------------------------
def test_paired_augmenter_equals_the_explicit_calls(he):
    aug = PairedAugmenter(64, 0.2, 0.05, src_stains="hed", tgt_stains="hdab", white=230, rng=random.Random(11))
    got = aug(he["gsrc"], he["gtgt"], he["gmask"])
    rng = random.Random(11)
    p = sample_d4_params(3, (70, 90), 64, rng)
    js, jt = sample_stain_jitter(3, 0.2, 0.05, rng), sample_stain_jitter(3, 0.2, 0.05, rng)
    want = paired_augment(he["gsrc"], he["gtgt"], p, 64, mask_u8=he["gmask"], src_map=stain_jitter_maps(js, "hed"),
                          tgt_map=stain_jitter_maps(jt, "hdab"), white=230)
    assert len(got) == 3 and all(torch.equal(a, b) for a, b in zip(got, want))
    # the defaults: the target's colours are untouched, no mask
    aug = PairedAugmenter(64, rng=random.Random(12), transpose=False)
    s, t = aug(he["gsrc"], he["gtgt"])
    rng = random.Random(12)
    p = sample_d4_params(3, (70, 90), 64, rng, transpose=False)
    js = sample_stain_jitter(3, 0.05, 0.01, rng)
    ws, wt = paired_augment(he["gsrc"], he["gtgt"], p, 64, src_map=stain_jitter_maps(js, "hed"))
    assert torch.equal(s, ws) and torch.equal(t, wt)
    assert np.array_equal(t.cpu().numpy(), A.network(A.augment(he["tgt"], p.tolist(), 64)[0]))


# ---- no hidden synchronisation ------------------------------------------------------------------------------------------
def test_augment_does_not_synchronise(he):
    maps = stain_jitter_maps(sample_stain_jitter(3, rng=random.Random(1)), "hed")
    kw = {"mask_u8": he["gmask"], "src_map": maps, "tgt_map": maps, "white": 230, "return_u8": True}
    paired_augment(he["gsrc"], he["gtgt"], _params(P5), 64, **kw)                   # the library is loaded from here on
    stain_augment(he["gsrc"], maps)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = paired_augment(he["gsrc"], he["gtgt"], _params(P5), 64, **kw)
        b = stain_augment(he["gsrc"], maps, white=230)
        c = stain_augment(he["gsrc"], maps, network_input=True)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert torch.isfinite(a[0]).all() and int(b.sum()) > 0 and torch.isfinite(c).all()


# ---- error paths ---------------------------------------------------------------------------------------------------------
def test_paired_augment_rejects(he):
    s, t, m = he["gsrc"], he["gtgt"], he["gmask"]
    p = _params(P5)
    maps = stain_jitter_maps(IDENT * 3, "hed")

    def call(src=s, tgt=t, params=p, size=64, **kw):
        return paired_augment(src, tgt, params, size, **kw)

    for bad, name in ((s.float(), "src_u8"), (s[0], "src_u8"), (s[..., :2], "src_u8"), (s[:, :, ::2], "src_u8")):
        with pytest.raises(ValueError, match=name):
            call(src=bad)
    with pytest.raises(ValueError, match="tgt_u8"):
        call(tgt=t[:, :69])
    with pytest.raises(ValueError, match="tgt_u8"):
        call(tgt=t.int())
    with pytest.raises(TypeError, match="tgt_u8"):
        call(tgt=None)
    for bad in (m[:, :69], m.float(), m[..., None], m[:, :, ::2], m.cpu()):
        with pytest.raises(ValueError, match="mask_u8"):
            call(mask_u8=bad)
    for bad in (p.to(DEV), p.long(), p[:, :3], torch.zeros((3, 6), dtype=torch.int32), p[:2], p.reshape(-1),
                _params([[7, 0, 0, 0, 0]] * 3), _params([[0, 27, 0, 0, 0]] * 3), _params([[-1, 0, 0, 0, 0]] * 3),
                _params([[0, -1, 0, 0, 0]] * 3), _params([[0, 0, 2, 0, 0]] * 3), _params([[0, 0, 0, -1, 0]] * 3),
                _params([[0, 0, 0, 0, 2]] * 3)):
        with pytest.raises(ValueError, match="params"):
            call(params=bad)
    with pytest.raises(TypeError, match="params"):
        call(params=P5)
    for name in ("src_map", "tgt_map"):
        nan = maps.clone()
        nan[1, 3] = float("nan")
        for bad in (maps[:2], maps[:, :9], maps.double(), nan, maps.to(DEV)):
            with pytest.raises(ValueError, match=name):
                call(**{name: bad})
        with pytest.raises(TypeError, match=name):
            call(**{name: maps.numpy()})
    for bad in (-1, 256):
        with pytest.raises(ValueError, match="white"):
            call(src_map=maps, white=bad)
    with pytest.raises(TypeError):
        call(src_map=maps, white=200.5)
    for bad in (torch.float16, torch.int32, torch.bool):
        with pytest.raises(ValueError, match="mask_dtype"):
            call(mask_u8=m, mask_dtype=bad)
    for bad in (0, 71, -4):
        with pytest.raises(ValueError, match="size"):
            call(size=bad)
    with pytest.raises(ValueError, match="maps"):
        stain_augment(s, maps[:2])
    with pytest.raises(TypeError, match="maps"):
        stain_augment(s, None)
    with pytest.raises(ValueError, match="tiles_u8"):
        stain_augment(s.float(), maps)
    with pytest.raises(ValueError, match="white"):
        stain_augment(s, maps, white=300)
