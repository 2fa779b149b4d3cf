"""Fused paired augmentation without a GPU: the exports, the status codes of the two entry points (returned before any HIP
call), the folding of a jitter into the OD map against the float64 restatement (tests/augment_ref.py), the identity map,
the samplers and the eight symmetries of the restatement's geometry."""
import ctypes
import random

import numpy as np
import pytest
import torch

import augment_ref as A

NEW_SYMBOLS = ["s2s_paired_augment", "s2s_stain_augment_u8"]
NAMES = ["paired_augment", "stain_augment", "stain_jitter_maps", "sample_d4_params", "sample_stain_jitter",
         "PairedAugmenter"]


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


# ---- exports ----------------------------------------------------------------------------------------------------------
def test_exports():
    import stain2stain_amd
    from stain2stain_amd import _native, augment
    for name in NAMES:
        assert name in stain2stain_amd.__all__ and getattr(stain2stain_amd, name) is getattr(augment, name), name
    assert "augment.hip" in _native.SOURCES
    declared = _native.declared_symbols()
    lib = _native.lib()
    for sym in NEW_SYMBOLS:
        assert sym in declared and hasattr(lib, sym), sym


# ---- status codes of the entry points: returned before any HIP call ---------------------------------------------------
def test_entry_points_return_status_codes():
    from stain2stain_amd import _native
    lib = _native.lib()
    X = 4096                                      # a non-null pointer that is never dereferenced: every call below fails first
    od = (ctypes.c_float * 256)()

    def pa(src=X, sp=96, si=96 * 32, tgt=X, tp=96, ti=96 * 32, mask=0, mp=32, mi=32 * 32, B=1, Hs=32, Ws=32, S=16, params=X,
           cols=4, smap=0, tmap=0, od=od, white=-1, out_s=X, out_t=X, out_m=0, kind=0, u8s=0, u8t=0):
        return lib.s2s_paired_augment(src, sp, si, tgt, tp, ti, mask, mp, mi, B, Hs, Ws, S, params, cols, smap, tmap, od,
                                      white, out_s, out_t, out_m, kind, u8s, u8t, None)

    for name in ("src", "tgt", "params", "out_s", "out_t"):
        assert pa(**{name: 0}) == -5, name
    assert pa(smap=X, od=None) == -5 and pa(tmap=X, od=None) == -5
    assert pa(mask=X) == -5 and pa(mask=X, kind=1) == -5 and pa(kind=2, out_m=X) == -5 and pa(out_m=X) == -5
    assert pa(mask=X, out_m=X, kind=4) == -3 and pa(kind=-1) == -3
    assert pa(B=0) == -1 and pa(B=65536) == -1 and pa(S=0) == -1 and pa(S=33) == -1 and pa(Hs=15) == -1 and pa(Ws=15) == -1
    assert pa(cols=3) == -1 and pa(cols=6) == -1 and pa(white=-2) == -1 and pa(white=256) == -1
    assert pa(sp=95) == -1 and pa(tp=95) == -1 and pa(B=2, si=96 * 31) == -1 and pa(B=2, ti=96 * 31) == -1
    assert pa(mask=X, out_m=X, kind=1, mp=31) == -1 and pa(B=2, mask=X, out_m=X, kind=3, mi=32 * 31) == -1
    assert pa(S=32769, Hs=40000, Ws=40000, sp=120000, tp=120000) == -1

    def sa(img=X, pitch=96, stride=96 * 32, B=1, H=32, W=32, maps=X, od=od, white=-1, out=X, op=96, oi=96 * 32, f32=0):
        return lib.s2s_stain_augment_u8(img, pitch, stride, B, H, W, maps, od, white, out, op, oi, f32, None)

    assert sa(img=0) == -5 and sa(maps=0) == -5 and sa(od=None) == -5 and sa(out=0) == -5
    assert sa(B=0) == -1 and sa(B=65536) == -1 and sa(H=0) == -1 and sa(W=-1) == -1 and sa(pitch=95) == -1
    assert sa(B=2, stride=96 * 31) == -1 and sa(white=-2) == -1 and sa(white=256) == -1
    assert sa(op=95) == -1 and sa(B=2, oi=96 * 31) == -1
    assert sa(op=0, oi=0, f32=1, img=0) == -5                      # fp32 out ignores the output pitch: the null comes first


# ---- folding a jitter into a map ---------------------------------------------------------------------------------------
def _jitter(B, seed, sa=0.2, sb=0.05):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(1 - sa, 1 + sa, (B, 3)), rng.uniform(-sb, sb, (B, 3))], axis=1)


def test_stain_jitter_maps_against_fold():
    from stain2stain_amd import stain_jitter_maps
    custom = np.array([[0.5626, 0.7201, 0.4062], [0.2159, 0.8012, 0.5581]])          # a [2, 3] basis, not unit length
    j = _jitter(5, 3)
    for stains in ("hed", "hdab", custom, torch.from_numpy(custom), custom.tolist()):
        got = stain_jitter_maps(torch.from_numpy(j), stains)
        assert got.dtype == torch.float32 and tuple(got.shape) == (5, 12) and not got.is_cuda
        for n in range(5):
            want = A.fold(j[n], stains.numpy() if isinstance(stains, torch.Tensor) else stains)
            assert (np.abs(got[n].numpy().astype(np.float64) - want) <= _ulp32(want)).all(), (stains, n)
    # one basis per sample: a list of names and arrays, and a [B, 2, 3] batch
    per = ["hed", "hdab", custom, "hed", custom * 2.0]
    got = stain_jitter_maps(j, per)
    for n in range(5):
        want = A.fold(j[n], per[n])
        assert (np.abs(got[n].numpy().astype(np.float64) - want) <= _ulp32(want)).all(), n
    batch = np.stack([custom, custom[::-1], custom, custom, custom[::-1]])
    got = stain_jitter_maps(j, batch)
    for n in range(5):
        want = A.fold(j[n], batch[n])
        assert (np.abs(got[n].numpy().astype(np.float64) - want) <= _ulp32(want)).all(), n
    assert not torch.equal(got[0], got[1])
    # a plain list of six-number rows works as well
    assert torch.equal(stain_jitter_maps(j.tolist(), "hed"), stain_jitter_maps(j, "hed"))


def test_stain_jitter_maps_rejects():
    from stain2stain_amd import stain_jitter_maps
    j = _jitter(2, 4)
    with pytest.raises(ValueError):
        stain_jitter_maps(j, [[1.0, 2.0, 3.0], [2.0, 4.0, 6.0]])                     # parallel vectors: singular
    with pytest.raises(ValueError):
        stain_jitter_maps(j, [[0.0, 0.0, 0.0], [0.2, 0.8, 0.5]])
    with pytest.raises(ValueError):
        stain_jitter_maps(j, "he")
    for bad in (np.nan, np.inf, -np.inf):
        k = j.copy()
        k[1, 4] = bad
        with pytest.raises(ValueError):
            stain_jitter_maps(k, "hed")
    for shape in ((2, 5), (6,), (2, 6, 1), (0, 6)):
        with pytest.raises(ValueError):
            stain_jitter_maps(np.ones(shape), "hed")
    with pytest.raises(ValueError):
        stain_jitter_maps(j, ["hed", "hdab", "hed"])                                # three bases for two samples


@pytest.mark.parametrize("stains", ["hed", "hdab"])
def test_identity_map(stains):
    from stain2stain_amd import stain_jitter_maps
    ident = np.array([[1.0, 1.0, 1.0, 0.0, 0.0, 0.0]])
    got = stain_jitter_maps(ident, stains)[0].numpy()
    assert np.abs(got[:9].astype(np.float64).reshape(3, 3) - np.eye(3)).max() <= 1e-16
    # the restatement's inv(M) @ diag(1) @ M is the identity up to the rounding of two float64 3 x 3 products of entries
    # below 2 in magnitude: 2 * 3 * 4 * 2^-53 (numpy gives 0.96e-16 for "hed" and 1.41e-16 for "hdab" after the fp32
    # rounding, which makes the diagonal exact)
    ref = A.fold(ident[0], stains).astype(np.float32)
    assert np.abs(ref[:9].astype(np.float64).reshape(3, 3) - np.eye(3)).max() <= 24 * 2.0 ** -53
    for m in (got, ref):
        assert (m[9:] == 0).all()
        grid = np.stack(np.meshgrid(np.arange(256), np.arange(0, 256, 5), np.arange(0, 256, 3), indexing="ij"), -1)
        grid = grid.reshape(-1, 3).astype(np.uint8)
        got32, raw32 = A.apply32(grid, m[:9], m[9:])
        got64, raw64 = A.apply64(grid, m[:9], m[9:])
        want = np.maximum(grid, 1)                                                   # 0 takes the entry of 1
        assert np.array_equal(got32, want) and np.array_equal(got64, want)
        assert np.abs(raw64 - want).max() <= 1.6e-5


# ---- samplers ---------------------------------------------------------------------------------------------------------
def test_sample_d4_params():
    from stain2stain_amd import sample_d4_params
    from stain2stain_amd.data import sample_crop_flip_params
    p = sample_d4_params(64, (70, 90), 64, random.Random(7))
    assert p.dtype == torch.int32 and tuple(p.shape) == (64, 5) and not p.is_cuda
    assert torch.equal(p[:, :4], sample_crop_flip_params(64, (70, 90), 64, random.Random(7)))
    assert int(p[:, 0].min()) >= 0 and int(p[:, 0].max()) <= 6 and int(p[:, 1].min()) >= 0 and int(p[:, 1].max()) <= 26
    assert set(p[:, 2:].reshape(-1).tolist()) == {0, 1}
    # the draw order: every row of sample_crop_flip_params first, then one random() per sample
    rng = random.Random(7)
    sample_crop_flip_params(64, (70, 90), 64, rng)
    assert p[:, 4].tolist() == [int(rng.random() > 0.5) for _ in range(64)]
    assert {tuple(r) for r in p[:, 2:].tolist()} == {(h, v, t) for h, v, t in A.SYMMETRIES}      # all eight appear
    q = sample_d4_params(64, (70, 90), 64, random.Random(7), transpose=False)
    assert torch.equal(q[:, :4], p[:, :4]) and (q[:, 4] == 0).all()
    rng2 = random.Random(7)
    sample_d4_params(4, (70, 90), 64, rng2, transpose=False)
    rng3 = random.Random(7)
    sample_crop_flip_params(4, (70, 90), 64, rng3)
    assert rng2.random() == rng3.random()                                            # no draw for an unused column
    with pytest.raises(ValueError):
        sample_d4_params(2, (60, 90), 64)


def test_sample_stain_jitter():
    from stain2stain_amd import sample_stain_jitter
    j = sample_stain_jitter(200, rng=random.Random(3))
    assert j.dtype == torch.float64 and tuple(j.shape) == (200, 6) and not j.is_cuda
    assert float(j[:, :3].min()) >= 0.95 and float(j[:, :3].max()) <= 1.05
    assert float(j[:, 3:].min()) >= -0.01 and float(j[:, 3:].max()) <= 0.01
    assert float(j[:, :3].max() - j[:, :3].min()) > 0.09 and float(j[:, 3:].max() - j[:, 3:].min()) > 0.018
    rng = random.Random(5)
    want = []
    for _ in range(3):
        a = [rng.uniform(0.8, 1.2) for _ in range(3)]
        want.append(a + [rng.uniform(-0.05, 0.05) for _ in range(3)])
    assert sample_stain_jitter(3, 0.2, 0.05, random.Random(5)).tolist() == want
    assert sample_stain_jitter(2, 0.0, 0.0, random.Random(1)).tolist() == [[1.0, 1.0, 1.0, 0.0, 0.0, 0.0]] * 2
    for kw in ({"sigma_alpha": -0.1}, {"sigma_beta": float("nan")}, {"sigma_alpha": float("inf")}):
        with pytest.raises(ValueError):
            sample_stain_jitter(2, **kw)
    with pytest.raises(ValueError):
        sample_stain_jitter(0)
    assert "convention" in sample_stain_jitter.__doc__


def test_the_eight_symmetries_are_distinct():
    img = np.arange(5 * 5 * 3, dtype=np.uint8).reshape(5, 5, 3)                       # no symmetry of its own
    seen = {A.geometry(img, 0, 0, h, v, t, 5).tobytes() for h, v, t in A.SYMMETRIES}
    assert len(A.SYMMETRIES) == 8 and len(seen) == 8
    # the definition, index by index
    big = np.random.default_rng(0).integers(0, 256, (9, 11, 3), dtype=np.uint8)
    for h, v, t in A.SYMMETRIES:
        out = A.geometry(big, 2, 3, h, v, t, 6)
        for y in range(6):
            for x in range(6):
                a, b = (x, y) if t else (y, x)
                assert (out[y, x] == big[2 + (5 - a if v else a), 3 + (5 - b if h else b)]).all()
    # the rotations are among them: rot90 = transpose, then a vertical flip of the result = hflip, then transpose
    assert np.array_equal(np.rot90(img), A.geometry(img, 0, 0, 1, 0, 1, 5))
    assert np.array_equal(np.rot90(img, 2), A.geometry(img, 0, 0, 1, 1, 0, 5))
    assert np.array_equal(np.rot90(img, 3), A.geometry(img, 0, 0, 0, 1, 1, 5))


# ---- argument checks that need no GPU --------------------------------------------------------------------------------
def test_wrappers_reject_host_tensors_and_bad_types():
    from stain2stain_amd import PairedAugmenter, paired_augment, stain_augment
    u = torch.zeros((2, 16, 16, 3), dtype=torch.uint8)
    p = torch.zeros((2, 4), dtype=torch.int32)
    with pytest.raises(ValueError, match="GPU"):
        paired_augment(u, u, p, 8)
    with pytest.raises(TypeError, match="src_u8"):
        paired_augment(u.numpy(), u, p, 8)
    with pytest.raises(ValueError, match="src_u8"):
        paired_augment(u.float(), u, p, 8)
    with pytest.raises(ValueError, match="GPU"):
        stain_augment(u, torch.zeros((2, 12)))
    with pytest.raises(TypeError):
        stain_augment(None, torch.zeros((2, 12)))
    for kw in ({"sigma_alpha": -1.0}, {"src_stains": "he"}, {"white": 256}, {"size": 0}):
        with pytest.raises(ValueError):
            PairedAugmenter(**{"size": 8, **kw})
