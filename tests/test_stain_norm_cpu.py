"""Macenko stain normalisation without a GPU: the numpy restatement (tests/stain_norm_ref.py) against the method as
published, the host arithmetic between the passes, the status codes of the new entry points and the argument checks the
wrappers make before they touch the device.

The bound of the textbook comparison.  The restatement reads the stain directions off a histogram of the diamond angle
s = y / (|x| + |y|) with NB = 4096 bins over [-1, 1].  With phi = atan2(y, x) and x > 0, s = tan(phi) / (1 + |tan(phi)|),
so dphi/ds = (1 + |tan phi|)^2 / (1 + tan^2 phi) <= 2: one bin of width 2 / NB is at most 9.8e-4 rad, and a second bin
covers the two rank conventions (the bin's centre against np.percentile's order statistic).  2e-3 rad per vector, on an
image that keeps at least 5000 pixels so that neighbouring order statistics are closer than a bin."""
import ctypes

import numpy as np
import pytest
import torch

import stain_norm_ref as R

NEW_SYMBOLS = ["s2s_stain_moments_slots", "s2s_stain_moments_u8", "s2s_stain_moments_finalize",
               "s2s_stain_angle_hist_u8", "s2s_stain_conc_hist_u8", "s2s_stain_normalize_u8"]


def _angle(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    c = abs(a @ b) / (np.linalg.norm(a) * np.linalg.norm(b))
    return float(np.arctan2(np.sqrt(max(0.0, 1.0 - c * c)), c))


# ---- the restatement against the published method --------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2])
def test_restatement_against_textbook_macenko(seed):
    img, true = R.synthetic_he(96, 96, seed)
    fit = R.fit(img)
    book, kept = R.textbook(img)
    assert fit["pixels"] >= 5000                  # the bound's premise: a dense histogram
    assert fit["pixels"] == kept == int(R.kept(img).sum())        # the byte rule is the published OD rule
    for k in range(2):
        a = _angle(fit["vectors"][k], book[k])
        print(f"seed {seed} vector {k}: {a:.2e} rad from the textbook, {_angle(fit['vectors'][k], true[k]):.2e} from truth")
        assert a <= 2e-3
    assert fit["vectors"][0][0] > fit["vectors"][1][0]
    assert np.abs(np.linalg.norm(fit["vectors"], axis=1) - 1).max() < 1e-12


# ---- host arithmetic -------------------------------------------------------------------------------------------------
def test_u_beta_and_q_table():
    from stain2stain_amd import stain_norm as N
    assert N.u_beta(0.15) == 219 == R.u_beta(0.15)
    assert N.u_beta(0.0) == 255 and N.u_beta(1.0) == 93 and N.u_beta(50.0) == 0
    assert 255 * np.exp(-0.15) >= 219 and -np.log(220 / 255.0) < 0.15 <= -np.log(219 / 255.0)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            N.u_beta(bad)
    q = N.q_table()
    assert q.dtype == torch.int32 and np.array_equal(q.numpy().astype(np.int64), R.q_table())
    assert int(q[255]) == 0 and int(q[0]) == int(q[1]) == round(float(np.float32(np.log10(255.0))) * 4096)
    assert N.NB == R.NB == 4096 and N.CONC_MAX == R.CONC_MAX == 4.0


def test_rank_rule():
    from stain2stain_amd.stain_norm import max_conc_from_histograms, rank_bin
    h = np.zeros(4096, np.int64)
    h[[10, 20, 30]] = (1, 98, 1)                                  # 100 pixels
    assert rank_bin(h, 1.0) == 10 and rank_bin(h, 1.5) == 20 and rank_bin(h, 99.0) == 20 and rank_bin(h, 99.5) == 30
    assert rank_bin(h, 100.0) == 30 and rank_bin(h, 1e-9) == 10   # rank = max(1, ceil(.)): never below the first pixel
    for p in (0.5, 1.0, 37.0, 99.0, 100.0):
        assert rank_bin(h, p) == R.rank_bin(h, p)
    one = np.zeros(4096, np.int64)
    one[7] = 1
    assert rank_bin(one, 1.0) == rank_bin(one, 99.0) == 7
    with pytest.raises(ValueError):
        rank_bin(np.zeros(4096, np.int64), 50.0)
    mc = max_conc_from_histograms(np.stack([h, one]), 99.0)
    assert mc.dtype == torch.float64 and mc.tolist() == [21 * 4.0 / 4096, 8 * 4.0 / 4096]      # upper bin edges
    assert np.array_equal(mc.numpy(), R.max_conc(np.stack([h, one]), 99.0))
    for bad in (0.0, 100.5, float("nan")):
        with pytest.raises(ValueError):
            max_conc_from_histograms(np.stack([h, one]), bad)


def test_plane_sign_conventions_and_agreement_with_an_independent_eigh():
    from stain2stain_amd.stain_norm import plane_from_moments
    for seed in (1, 2, 3):
        img, _ = R.synthetic_he(64, 80, seed)
        mom = R.moments(img)
        pl = plane_from_moments(torch.tensor(mom, dtype=torch.int64))
        assert pl.dtype == torch.float32 and tuple(pl.shape) == (3, 2)
        pl = pl.numpy().astype(np.float64)
        assert pl[:, 0].sum() > 0 and pl[np.abs(pl[:, 1]).argmax(), 1] > 0
        want, w = R.plane(mom)
        assert w[1] > 0 and np.abs(pl - want).max() <= 1e-6
        # an eigen-decomposition of the covariance of the OD samples themselves, not of the moments
        q = R.q_table()[img][R.kept(img)].reshape(-1, 3) / 4096.0
        ww, vv = np.linalg.eigh(np.cov(q.T, bias=True))
        for j, col in enumerate((2, 1)):
            v = vv[:, col] * np.sign(vv[:, col] @ pl[:, j])
            assert np.abs(v - pl[:, j]).max() <= 1e-6


def test_vectors_from_histogram_orders_haematoxylin_first():
    from stain2stain_amd.stain_norm import vectors_from_histogram
    img, _ = R.synthetic_he(64, 80, 4)
    pl, _ = R.plane(R.moments(img))
    hist = R.angle_hist(img, pl)
    assert int(hist.sum()) == int(R.kept(img).sum())
    vec = vectors_from_histogram(torch.from_numpy(hist), torch.from_numpy(pl), 1.0)
    assert vec.dtype == torch.float64 and tuple(vec.shape) == (2, 3)
    assert np.abs(vec.numpy() - R.vectors(hist, pl, 1.0)).max() <= 1e-15
    assert float(vec[0, 0]) > float(vec[1, 0])
    # the rule is the R component, whichever end of the angle range it comes from: mirror the plane's second axis
    flipped = pl * np.array([1.0, -1.0], dtype=np.float32)
    vec2 = vectors_from_histogram(torch.from_numpy(hist[::-1].copy()), torch.from_numpy(flipped), 1.0)
    assert float(vec2[0, 0]) > float(vec2[1, 0])
    # bins k <-> NB - 1 - k under s -> -s: the same two directions, up to the bin the rank rule may move by
    assert max(_angle(vec2[k].numpy(), vec[k].numpy()) for k in range(2)) <= 2e-3
    for bad in (0.0, 50.0, -1.0):
        with pytest.raises(ValueError):
            vectors_from_histogram(torch.from_numpy(hist), torch.from_numpy(pl), bad)


def test_blank_and_single_colour_images_raise():
    from stain2stain_amd.stain_norm import plane_from_moments
    blank = np.full((32, 32, 3), 255, np.uint8)
    assert R.moments(blank)[0] == 0
    with pytest.raises(ValueError, match="pixels"):
        plane_from_moments(R.moments(blank))
    single = np.broadcast_to(np.array([120, 60, 140], np.uint8), (32, 32, 3))
    assert R.moments(single)[0] == 1024
    with pytest.raises(ValueError, match="plane"):
        plane_from_moments(R.moments(single))
    two = np.array(single)
    two[:16] = (90, 40, 110)                                      # two colours span a line, not a plane
    with pytest.raises(ValueError, match="plane"):
        plane_from_moments(R.moments(two))
    few = np.array(blank)
    few[0, :15] = np.random.default_rng(0).integers(20, 200, size=(15, 3))
    assert R.moments(few)[0] == 15
    with pytest.raises(ValueError, match="pixels"):
        plane_from_moments(R.moments(few))
    with pytest.raises(ValueError):
        plane_from_moments([1, 2, 3])


def test_fitted_vectors_are_a_stain_basis():
    """fit.vectors plugs into stain_quant's stains= unchanged; the 3 x 3 inverse's first two rows are the two-stain
    least-squares solution Macenko uses (the residual is orthogonal to both)."""
    from stain2stain_amd import stain_matrix
    from stain2stain_amd.stain_quant import unmix_matrix
    img, _ = R.synthetic_he(64, 64, 5)
    vec = R.fit(img)["vectors"]
    M = stain_matrix(torch.from_numpy(vec)).numpy()
    assert np.abs(M[:2] - vec).max() < 1e-15 and abs(M[2] @ vec[0]) < 1e-15 and abs(M[2] @ vec[1]) < 1e-15
    m32 = unmix_matrix(torch.from_numpy(vec)).numpy()
    assert np.abs(m32.astype(np.float64) - R.unmix32(vec)).max() <= 2.0 ** -22 * np.abs(m32).max()
    lstsq = np.linalg.pinv(vec)                                   # od [.., 3] @ pinv [3, 2] = the least-squares c
    assert np.abs(np.linalg.inv(M)[:, :2] - lstsq).max() < 1e-12


# ---- status codes of the entry points: returned before any HIP call ---------------------------------------------------
def test_entry_points_return_status_codes():
    from stain2stain_amd import _native
    lib = _native.lib()
    od, co, qt = (ctypes.c_float * 256)(), (ctypes.c_float * 17)(), (ctypes.c_int * 256)()
    X = 4096                                      # a non-null pointer that is never dereferenced: every call below fails first

    assert lib.s2s_stain_moments_slots(1, 16, 1024) == 1 and lib.s2s_stain_moments_slots(2, 17, 1025) == 8
    assert lib.s2s_stain_moments_slots(0, 16, 16) == -1 and lib.s2s_stain_moments_slots(1, 0, 16) == -1
    assert lib.s2s_stain_moments_slots(1, 16, -1) == -1

    def mom(img=X, pitch=96, B=1, band_top=0, band_h=32, H=32, W=32, qt=qt, ub=219, black=0, part=X):
        return lib.s2s_stain_moments_u8(img, pitch, pitch * band_h, B, band_top, band_h, H, W, qt, ub, black, part, None)

    assert mom(img=0) == -5 and mom(part=0) == -5 and mom(qt=None) == -5
    assert mom(W=0) == -1 and mom(W=-4) == -1 and mom(H=0) == -1 and mom(B=0) == -1 and mom(pitch=95) == -1
    assert mom(band_top=-16) == -1 and mom(band_top=32, band_h=16) == -1 and mom(band_h=48) == -1 and mom(band_h=0) == -1
    assert mom(band_top=8, band_h=24) == -1 and mom(band_h=8) == -1       # not whole chunk rows
    assert mom(ub=256) == -1 and mom(ub=-1) == -1 and mom(black=256) == -1 and mom(black=-1) == -1

    fin = lib.s2s_stain_moments_finalize
    assert fin(0, 1, X, None) == -5 and fin(X, 1, 0, None) == -5 and fin(X, 0, X, None) == -1 and fin(X, -3, X, None) == -1

    for fn in (lib.s2s_stain_angle_hist_u8, lib.s2s_stain_conc_hist_u8):
        def hist(img=X, pitch=96, B=1, band_top=0, band_h=32, H=32, W=32, od=od, co=co, ub=219, black=0, out=X):
            return fn(img, pitch, pitch * band_h, B, band_top, band_h, H, W, od, co, ub, black, 1, out, None)

        assert hist(img=0) == -5 and hist(out=0) == -5 and hist(od=None) == -5 and hist(co=None) == -5
        assert hist(W=0) == -1 and hist(W=-4) == -1 and hist(H=0) == -1 and hist(B=0) == -1 and hist(pitch=95) == -1
        assert hist(band_top=-1) == -1 and hist(band_top=20, band_h=13) == -1 and hist(band_h=33) == -1
        assert hist(band_h=0) == -1 and hist(ub=256) == -1 and hist(black=-1) == -1

    def app(img=X, pitch=96, B=1, H=32, W=32, od=od, co=co, out=X, out_pitch=96, f32=0):
        return lib.s2s_stain_normalize_u8(img, pitch, pitch * H, B, H, W, od, co, out, out_pitch, out_pitch * H, f32, None)

    assert app(img=0) == -5 and app(out=0) == -5 and app(od=None) == -5 and app(co=None) == -5
    assert app(W=0) == -1 and app(W=-4) == -1 and app(H=0) == -1 and app(B=0) == -1 and app(pitch=95) == -1
    assert app(out_pitch=95) == -1
    assert lib.s2s_stain_normalize_u8(X, 96, 96 * 31, 2, 32, 32, od, co, X, 96, 96 * 32, 0, None) == -1
    assert lib.s2s_stain_normalize_u8(X, 96, 96 * 32, 2, 32, 32, od, co, X, 96, 96 * 31, 0, None) == -1


# ---- exports, the header and the wrappers' argument checks ------------------------------------------------------------
def test_exports_and_header():
    import stain2stain_amd as S
    from stain2stain_amd import _native
    for name in ("fit_stains", "stain_normalize", "normalize_region", "StainFit", "REFERENCE_HE"):
        assert name in S.__all__ and hasattr(S, name), name
    declared = _native.declared_symbols()
    lib = _native.lib()
    for sym in NEW_SYMBOLS:
        assert sym in declared and hasattr(lib, sym), sym
    assert "stain_norm.hip" in _native.SOURCES
    ref = S.REFERENCE_HE
    assert isinstance(ref, S.StainFit)
    assert np.array_equal(ref.vectors.numpy(), R.REF_VECTORS) and np.abs(ref.max_conc.numpy() - R.REF_MAX_CONC).max() < 1e-15
    assert np.abs(np.linalg.norm(R.REF_VECTORS, axis=1) - 1).max() < 1e-4
    S.stain_matrix(ref.vectors)                                   # a valid basis for stain_quant


def test_wrappers_reject():
    from stain2stain_amd import REFERENCE_HE, fit_stains, normalize_region, stain_normalize
    from stain2stain_amd.stain_norm import angle_histogram, concentration_histogram, moments
    r = torch.zeros((40, 40, 3), dtype=torch.uint8)
    b = torch.zeros((2, 16, 16, 3), dtype=torch.uint8)
    for fn in (fit_stains, moments, normalize_region):
        with pytest.raises(TypeError):
            fn(r.numpy())
        with pytest.raises(ValueError):
            fn(r.float())
        with pytest.raises(ValueError):
            fn(r[..., :2])
        with pytest.raises(ValueError):
            fn(r[:, ::2])                                         # pixels not contiguous within a row
        with pytest.raises(ValueError):
            fn(torch.zeros((0, 40, 3), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="GPU"):
        fit_stains(b)                                             # a host batch: there is no CPU path
    with pytest.raises(RuntimeError, match="GPU"):
        stain_normalize(b, REFERENCE_HE)
    with pytest.raises(ValueError):
        stain_normalize(r, REFERENCE_HE)                          # a region goes through normalize_region
    with pytest.raises(TypeError):
        stain_normalize(None)
    for kw in ({"alpha": 0.0}, {"alpha": 50.0}, {"beta": -1.0}, {"conc_percentile": 0.0}, {"conc_percentile": 101.0},
               {"black": 256}, {"black": -1}):
        with pytest.raises(ValueError):
            fit_stains(r, **kw)
    with pytest.raises(ValueError):
        angle_histogram(r, torch.zeros((2, 3)))
    with pytest.raises(ValueError):
        concentration_histogram(r, [[1.0, 2.0, 3.0], [2.0, 4.0, 6.0]])     # parallel vectors: no basis
    with pytest.raises(TypeError):
        normalize_region(r, fit="hdab")
    with pytest.raises(ValueError):
        normalize_region(r, REFERENCE_HE, band_rows=8)
