"""Stain quantification without a GPU: the stain bases, the float32 restatement (tests/stain_quant_ref.py) against a plain
float64 evaluation of the definition, the band planner, the status codes of the new entry points and the argument checks
the wrappers make before they touch the device.

The uint8 quantisation bound of the recovery test.  A synthesised channel is I = 255 * 10^(-od) rounded to the nearest
integer u, so u lies in [I - 0.5, I + 0.5] and the optical density read back, -log10(u / 255), is off by
|log10(u / I)| <= -log10(1 - 0.5 / I) =: d(I) (the lower end is the wider one; it needs I > 0.5, the test keeps every
channel at I >= 16).  Concentrations are linear in the densities, c_k = sum_ch od_ch m_ch,k, so
|c_k - c_k(true)| <= sum_ch |m_ch,k| d(I_ch): the bound is per pixel and per stain, from the pixel's own intensities.
The float32 restatement adds its rounding: the table entry, m and the product are each rounded once (relative 2^-24
each) and the two sums round partial sums no larger than S_k = sum_ch |od_ch m_ch,k|: at most 5 * 2^-24 * S_k to first
order, 6 * 2^-24 * S_k covers the second-order terms."""
import ctypes

import numpy as np
import pytest
import torch

import stain_quant_ref as R

THR = (0.2, 0.2, 0.2)


# ---- the stain bases -------------------------------------------------------------------------------------------------
def test_named_bases():
    from stain2stain_amd import stain_matrix
    from stain2stain_amd.stain_quant import unmix_matrix
    for name, rows in (("hdab", [[0.650, 0.704, 0.286], [0.268, 0.570, 0.776]]),
                       ("hed", [[0.65, 0.70, 0.29], [0.07, 0.99, 0.11], [0.27, 0.57, 0.78]])):
        M = stain_matrix(name)
        assert M.dtype == torch.float64 and tuple(M.shape) == (3, 3) and not M.is_cuda
        M = M.numpy()
        assert np.abs(np.linalg.norm(M, axis=1) - 1.0).max() < 1e-15
        for k, r in enumerate(rows):
            r = np.array(r)
            assert np.abs(M[k] - r / np.linalg.norm(r)).max() < 1e-15, (name, k)
        assert np.abs(M - R.stain_matrix(name)).max() < 1e-15
        # the nine kernel arguments: the double inverse, rounded to fp32 once
        m32 = unmix_matrix(name)
        assert m32.dtype == torch.float32
        inv = np.linalg.inv(M)
        assert np.abs(m32.numpy().astype(np.float64) - inv).max() <= 2.0 ** -24 * np.abs(inv).max() + 1e-14
    M = stain_matrix("hdab").numpy()
    assert abs(M[2] @ M[0]) < 1e-15 and abs(M[2] @ M[1]) < 1e-15          # the residual is orthogonal to H and DAB


def test_custom_bases_and_rejects():
    from stain2stain_amd import stain_matrix
    a = stain_matrix([[2.0, 0.0, 0.0], [0.0, 3.0, 0.0]]).numpy()
    assert np.array_equal(a, np.eye(3))
    b = stain_matrix(np.array([[0.65, 0.70, 0.29], [0.07, 0.99, 0.11], [0.27, 0.57, 0.78]])).numpy()
    assert np.abs(b - stain_matrix("hed").numpy()).max() == 0
    assert np.abs(stain_matrix(torch.tensor(R.HDAB)).numpy() - stain_matrix("hdab").numpy()).max() == 0
    for bad in ([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0]],                       # parallel
                [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 1.0, 0.0]],      # coplanar
                [[0.0, 0.0, 0.0], [0.0, 1.0, 0.0]],                       # a zero row
                [[1.0, 0.0, 0.0]], [[1.0, 0.0], [0.0, 1.0]], [[float("nan"), 0.0, 1.0], [0.0, 1.0, 0.0]], "he"):
        with pytest.raises(ValueError):
            stain_matrix(bad)


def test_od_table():
    from stain2stain_amd.stain_quant import od_table
    t = od_table()
    assert t.dtype == torch.float32 and tuple(t.shape) == (256,)
    assert np.array_equal(t.numpy(), R.od_table32())
    assert t[0] == t[1] and float(t[255]) == 0.0 and abs(float(t[1]) - np.log10(255.0)) < 1e-6
    assert (t[1:-1] > t[2:]).all()


# ---- the float32 restatement against the float64 evaluation -----------------------------------------------------------
def _synthetic(stains, H, W, seed):
    """Concentrations whose three channels all stay at I >= 16, and the image synthesised from them."""
    rng = np.random.default_rng(seed)
    M = R.stain_matrix(stains)
    conc = rng.uniform(0.0, 0.6, size=(H, W, 3))
    conc[..., 2] *= 0.0 if (M[2] < 0).any() else 0.1        # a residual with negative entries would push I above 255
    od = conc @ M
    assert od.min() >= 0.0 and od.max() < np.log10(255.0 / 16.0)
    return conc, R.synthesise(conc, stains)


def _random_u8(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(H, W, 3), dtype=np.uint8)


@pytest.mark.parametrize("stains", ["hdab", "hed"])
@pytest.mark.parametrize("kind,seed", [("synthetic", 11), ("synthetic", 12), ("random", 21), ("random", 22)])
def test_float32_restatement_against_float64(stains, kind, seed):
    from stain2stain_amd.stain_quant import unmix_matrix
    H, W = 96, 80
    img = _synthetic(stains, H, W, seed)[1] if kind == "synthetic" else _random_u8(H, W, seed)
    m64, m32 = R.unmix64(stains), unmix_matrix(stains).numpy()
    c64, c32 = R.concentrations64(img, m64), R.concentrations32(img, m32)
    thr = np.asarray(THR, dtype=np.float32).astype(np.float64)
    near = np.abs(c64 - thr) < 1e-5
    # a condition on the inputs, from the float64 evaluation alone: at most 0.1 % of the pixels sit that near a threshold
    assert near.any(-1).mean() <= 1e-3, (stains, kind, seed)
    p64, p32 = R.positive64(img, m64, THR), R.positive32(img, m32, THR)
    differ = p64 != p32
    assert not (differ & ~near).any(), (stains, kind, seed)
    assert np.abs(c32.astype(np.float64) - c64).max() < 1e-5


@pytest.mark.parametrize("stains", ["hdab", "hed"])
def test_synthesised_concentrations_are_recovered_to_the_quantisation_bound(stains):
    from stain2stain_amd.stain_quant import unmix_matrix
    conc, img = _synthetic(stains, 64, 72, 5)
    assert img.min() >= 16
    m64, m32 = R.unmix64(stains), unmix_matrix(stains).numpy()
    I = 255.0 * 10.0 ** (-(conc @ R.stain_matrix(stains)))                 # the unrounded intensities
    d = -np.log10(1.0 - 0.5 / I)                                           # per channel
    bound = d @ np.abs(m64)                                                # [H, W, 3]: sum_ch |m_ch,k| d_ch
    e64 = np.abs(R.concentrations64(img, m64) - conc)
    assert (e64 <= bound + 1e-12).all()
    S = R.od_table64()[img] @ np.abs(m64)
    e32 = np.abs(R.concentrations32(img, m32).astype(np.float64) - conc)
    assert (e32 <= bound + 6 * 2.0 ** -24 * S + 1e-12).all()
    print(f"{stains}: worst float64 error {e64.max():.3e} at a bound of {bound.max():.3e}")


def test_quantify_and_agreement_restatement_closed_forms():
    m32 = np.linalg.inv(R.stain_matrix("hdab")).astype(np.float32)
    white = np.full((1, 8, 8, 3), 255, np.uint8)
    q = R.quantify32(white, m32, THR)
    assert q["tissue"][0] == 0 and (q["positive"] == 0).all() and (q["burden"] == 0).all()
    a = R.agreement32(white, white, m32, THR)
    assert a["dice"][0] == 1 and a["iou"][0] == 1 and a["burden_abs_err"][0] == 0
    brown = np.broadcast_to(R.synthesise([0.0, 1.0, 0.0], "hdab"), (1, 8, 8, 3)).copy()
    q = R.quantify32(brown, m32, THR)
    assert q["tissue"][0] == 64 and q["positive"][0, 1] == 64 and q["positive"][0, 0] == 0 and q["burden"][0, 1] == 1
    half = brown.copy()
    half[:, :4] = 255
    a = R.agreement32(half, brown, m32, THR)
    assert a["dice"][0] == pytest.approx(2 * 32 / 96) and a["iou"][0] == 0.5 and a["burden_abs_err"][0] == 0
    x = torch.tensor([-1.5, -1.0, -0.999, 0.0, 0.003, 0.5, 0.999, 1.0, 2.0])
    assert np.array_equal(R.quantise(x.numpy()), ((x * 0.5 + 0.5) * 255).clamp(0, 255).to(torch.uint8).numpy())


# ---- the band planner ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [1, 15, 16, 17, 64, 301, 1000])
@pytest.mark.parametrize("cell", [1, 16, 40, 64, 256])
@pytest.mark.parametrize("band_rows", [None, 16, 17, 50, 64, 100, 4096])
def test_plan_stain_bands_covers_every_row_once(H, cell, band_rows):
    from stain2stain_amd.stain_quant import CHUNK_ROWS, plan_stain_bands
    cell = min(cell, H)
    bands = plan_stain_bands(H, cell, band_rows)
    ncy = -(-cell // CHUNK_ROWS)
    total = -(-H // cell) * ncy
    seen = [0] * H
    nxt = 0
    for g0, ng, r0, r1 in bands:
        assert g0 == nxt and ng >= 1 and 0 <= r0 <= r1 <= H
        nxt = g0 + ng
        if band_rows is not None:
            assert r1 - r0 <= band_rows
        for g in range(g0, g0 + ng):
            gy, cy = divmod(g, ncy)
            top = gy * cell + cy * CHUNK_ROWS
            bottom = min(top + CHUNK_ROWS, (gy + 1) * cell, H)
            for r in range(top, bottom):
                assert r0 <= r < r1
                seen[r] += 1
    assert nxt == total and seen == [1] * H
    if band_rows is None:
        assert len(bands) == 1


def test_plan_stain_bands_rejects():
    from stain2stain_amd.stain_quant import plan_stain_bands
    for args in ((0, 16), (16, 0), (64, 16, 15)):
        with pytest.raises(ValueError):
            plan_stain_bands(*args)


# ---- status codes of the entry points: returned before any HIP call ---------------------------------------------------
def test_entry_points_return_status_codes():
    from stain2stain_amd import _native
    lib = _native.lib()
    od, um = (ctypes.c_float * 256)(), (ctypes.c_float * 12)()
    X = 4096                                      # a non-null pointer that is never dereferenced: every call below fails first
    assert lib.s2s_stain_quant_chunks(0, 16) == -1 and lib.s2s_stain_quant_chunks(16, -1) == -1
    assert lib.s2s_stain_quant_chunks(16, 1024) == 1 and lib.s2s_stain_quant_chunks(17, 1025) == 4

    def u8(a=X, pitch=96, b=0, paired=0, B=1, band_top=0, band_h=32, H=32, W=32, ch=32, cw=32, g0=0, ng=2, od=od, um=um,
           white=220, black=0, stain=1, part=X):
        return lib.s2s_stain_quant_u8(a, pitch, pitch * band_h, b, pitch, pitch * band_h, paired, B, band_top, band_h, H, W,
                                      ch, cw, g0, ng, od, um, white, black, stain, part, None)

    assert u8(a=0) == -5 and u8(part=0) == -5 and u8(od=None) == -5 and u8(um=None) == -5
    assert u8(paired=1, b=0) == -5
    assert u8(B=0) == -1 and u8(B=-2) == -1 and u8(H=0) == -1 and u8(W=-1) == -1
    assert u8(ch=0) == -1 and u8(cw=0) == -1 and u8(ch=-64) == -1
    assert u8(pitch=95) == -1 and u8(ng=0) == -1 and u8(g0=-1) == -1 and u8(ng=3) == -1
    assert u8(band_h=16) == -1 and u8(band_top=1, band_h=31) == -1 and u8(band_h=0) == -1 and u8(band_h=33) == -1
    assert u8(white=0) == -1 and u8(white=257) == -1 and u8(black=256) == -1 and u8(stain=3) == -1 and u8(stain=-1) == -1

    def f32(a=X, b=0, paired=0, B=1, H=8, W=8, od=od, um=um, part=X):
        return lib.s2s_stain_quant_f32(a, b, paired, B, H, W, od, um, 220, 0, 1, part, None)

    assert f32(a=0) == -5 and f32(part=0) == -5 and f32(paired=1) == -5 and f32(od=None) == -5 and f32(um=None) == -5
    assert f32(B=0) == -1 and f32(H=0) == -1 and f32(W=-3) == -1

    fin = lib.s2s_stain_quant_finalize
    assert fin(0, 1, 1, 0, X, X, X, None) == -5 and fin(X, 1, 1, 0, 0, X, X, None) == -5
    assert fin(X, 1, 1, 0, X, 0, X, None) == -5 and fin(X, 1, 1, 1, X, 0, 0, None) == -5
    assert fin(X, 0, 1, 0, X, X, X, None) == -1 and fin(X, 1, 0, 0, X, X, X, None) == -1 and fin(X, -1, 1, 1, X, 0, X, None) == -1

    sep = lib.s2s_stain_separate
    assert sep(0, 0, 96, 96 * 32, 1, 32, 32, od, um, X, None) == -5 and sep(X, 0, 96, 96 * 32, 1, 32, 32, od, um, 0, None) == -5
    assert sep(X, 0, 96, 96 * 32, 1, 32, 32, None, um, X, None) == -5
    assert sep(X, 0, 96, 96 * 32, 0, 32, 32, od, um, X, None) == -1 and sep(X, 0, 96, 96 * 32, 1, 0, 32, od, um, X, None) == -1
    assert sep(X, 0, 95, 96 * 32, 1, 32, 32, od, um, X, None) == -1 and sep(X, 1, 31, 3 * 32 * 32, 1, 32, 32, od, um, X, None) == -1
    assert sep(X, 0, 96, 96 * 31, 2, 32, 32, od, um, X, None) == -1


# ---- argument checks that need no GPU --------------------------------------------------------------------------------
def test_wrappers_reject():
    from stain2stain_amd import stain_agreement, stain_quantify, stain_separate
    u = torch.zeros((2, 16, 16, 3), dtype=torch.uint8)
    f = torch.zeros((2, 3, 16, 16))
    for fn in (stain_quantify, stain_separate):
        with pytest.raises(RuntimeError, match="GPU"):
            fn(u)                                                         # CPU tensors: there is no CPU path
        with pytest.raises(RuntimeError, match="GPU"):
            fn(f)
        with pytest.raises(ValueError):
            fn(torch.zeros((2, 16, 16, 4), dtype=torch.uint8))            # C != 3
        with pytest.raises(ValueError):
            fn(torch.zeros((2, 4, 16, 16)))
        with pytest.raises(ValueError):
            fn(torch.zeros((16, 16, 3), dtype=torch.uint8))
        with pytest.raises(ValueError):
            fn(f.double())
        with pytest.raises(ValueError):
            fn(torch.zeros((0, 16, 16, 3), dtype=torch.uint8))
        with pytest.raises(TypeError):
            fn(u.numpy())
        with pytest.raises(ValueError):
            fn(u, stains="he")
    for bad in ((0.1, 0.2), (0.1, 0.2, 0.3, 0.4), 0.2, (0.1, float("nan"), 0.2)):
        with pytest.raises(ValueError):
            stain_quantify(u, thresholds=bad)
        with pytest.raises(ValueError):
            stain_agreement(u, u.clone(), thresholds=bad)
    with pytest.raises(ValueError):
        stain_quantify(u, white=0)
    with pytest.raises(ValueError):
        stain_quantify(u, black=256)
    with pytest.raises(RuntimeError, match="GPU"):
        stain_agreement(u, u.clone())
    with pytest.raises(RuntimeError, match="GPU"):
        stain_agreement(f, f.clone())
    with pytest.raises(ValueError):
        stain_agreement(u, u[:, :15])
    with pytest.raises(ValueError):
        stain_agreement(u, f)
    with pytest.raises(ValueError):
        stain_agreement(u, u.clone(), stain=3)
    with pytest.raises(TypeError):
        stain_agreement(u, None)


def test_region_wrappers_reject():
    from stain2stain_amd import region_stain_agreement, region_stain_map
    r = torch.zeros((40, 40, 3), dtype=torch.uint8)
    with pytest.raises(ValueError):
        region_stain_map(r.float())
    with pytest.raises(ValueError):
        region_stain_map(r[..., :2])
    with pytest.raises(ValueError):
        region_stain_map(r[:, ::2])                                       # pixels not contiguous within a row
    with pytest.raises(ValueError):
        region_stain_map(r, cell=0)
    with pytest.raises(ValueError):
        region_stain_map(r, cell=-8)
    with pytest.raises(ValueError):
        region_stain_map(r, stain=5)
    with pytest.raises(ValueError):
        region_stain_map(r, thresholds=(0.1,))
    with pytest.raises(TypeError):
        region_stain_map(None)
    with pytest.raises(ValueError):
        region_stain_agreement(r, r[:39])
    with pytest.raises(ValueError):
        region_stain_agreement(r, r.clone(), cell=0)
    with pytest.raises(TypeError):
        region_stain_agreement(r, None)


def test_generation_quality_rejects_a_bad_stain_argument():
    from stain2stain_amd.stain_quant import agreement_values
    a = torch.zeros((1, 3, 16, 16))
    with pytest.raises(TypeError):
        agreement_values(a, a, "hdab")
