"""The stain-normalisation kernels (csrc/stain_norm.hip) against the numpy restatement of tests/stain_norm_ref.py, on
poisoned memory (every ``torch.empty`` and every ``ops._workspace`` slab starts as NaN / 0xFF, as in
tests/test_stain_quant_gpu.py).

Tolerances.  The moments and every histogram count are integers and must be equal.  The histograms are
teacher-forced: the restatement gets the ``plane`` / ``vectors`` the implementation produced, so a last-bit difference
between two host eigen-solvers cannot move a bin.  End to end: ``plane`` 1e-6 against an independent eigh; ``vectors``
2e-3 rad against the restatement run on its own (two bins of the angle histogram, dphi/ds <= 2: test_stain_norm_cpu.py);
``max_conc`` two bins, 2 * CONC_MAX / NB.  Apply: the kernel evaluates in fp32 what the restatement evaluates in float64
from the same fp32 constants; its error is a few ulp of 255, about 1e-4 levels, so the bytes are equal wherever the
restatement's unrounded level lies more than 1e-3 from a half-integer and at most one level apart elsewhere; fewer than
1 % of the pixels may lie in that band (a 2e-3-wide window per level), which the restatement alone decides."""
import numpy as np
import pytest
import torch

import stain_norm_ref as R
import stain_quant_ref as Q
from stain2stain_amd import REFERENCE_HE, StainFit, fit_stains, normalize_region, stain_normalize, stain_quantify
from stain2stain_amd.stain_norm import (CONC_MAX, NB, angle_histogram, concentration_histogram, moments,
                                        plane_from_moments, vectors_from_histogram)
from stain2stain_amd.stain_quant import unmix_matrix

pytestmark = pytest.mark.gpu
DEV = "cuda"


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


def _crop_view(u8):
    """The batch as a crop view of a larger GPU array: odd row pitch, unaligned base."""
    B, H, W, _ = u8.shape
    big = torch.full((B, H + 5, W + 6, 3), 77, dtype=torch.uint8, device=DEV)
    view = big[:, 2:2 + H, 3:3 + W]
    view.copy_(torch.from_numpy(u8))
    assert (3 * (W + 6)) % 4 != 0 and view.data_ptr() % 4 != 0
    return view


# name -> (numpy image, the GPU tensor the kernels read): the shapes that can break the kernels
def _batch():
    img = np.stack([R.synthetic_he(37, 53, 11)[0], R.synthetic_he(37, 53, 12)[0]])
    return img, _crop_view(img)


def _region(H, W, seed):
    img = R.synthetic_he(H, W, seed)[0]
    return img, torch.from_numpy(img).to(DEV)


CASES = {"batch 2x37x53 crop view": _batch,
         "region 40x1030": lambda: _region(40, 1030, 13),          # two chunk columns, a ragged last chunk row
         "region 33x7": lambda: _region(33, 7, 14)}


@pytest.fixture(scope="module")
def slide():
    """One 96 x 96 image, its restatement fit (computed once) and the implementation's fit."""
    img = R.synthetic_he(96, 96, 1)[0]
    return {"img": img, "ref": R.fit(img), "fit": fit_stains(torch.from_numpy(img).to(DEV))}


def _sources(img, gpu):
    """(what, tensor, band_rows) over which a result must not change."""
    if gpu.dim() == 4:
        return [("gpu batch", gpu, None)]
    host = torch.from_numpy(img)
    return [(f"{'gpu' if t.is_cuda else 'host'} band_rows {b}", t, b) for t in (gpu, host) for b in (None, 16, 32)]


def _angle(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    c = abs(a @ b) / (np.linalg.norm(a) * np.linalg.norm(b))
    return float(np.arctan2(np.sqrt(max(0.0, 1.0 - c * c)), c))


@pytest.mark.parametrize("case", list(CASES))
def test_moments_are_exact_and_independent_of_the_banding(case):
    img, gpu = CASES[case]()
    want = R.moments(img)
    assert want[0] == int(R.kept(img).sum()) > 16
    for what, t, band_rows in _sources(img, gpu):
        got = moments(t, band_rows=band_rows)
        assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == (10,)
        assert got.cpu().tolist() == want, (case, what)
    dark = R.moments(img, beta=0.4, black=60)                      # another cut-off and the speck rule
    assert moments(gpu, beta=0.4, black=60).cpu().tolist() == dark and dark[0] < want[0]


@pytest.mark.parametrize("case", list(CASES))
def test_histograms_teacher_forced(case):
    img, gpu = CASES[case]()
    kept = int(R.kept(img).sum())
    plane = plane_from_moments(moments(gpu).cpu())
    want = R.angle_hist(img, plane.numpy())
    vectors = None
    for what, t, band_rows in _sources(img, gpu):
        got = angle_histogram(t, plane, band_rows=band_rows)
        assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == (NB,)
        got = got.cpu().numpy()
        assert int(got.sum()) == kept and np.array_equal(got, want), (case, what, int(np.abs(got - want).sum()))
        vectors = vectors_from_histogram(got, plane)
    m32 = unmix_matrix(vectors).numpy()
    want_c = R.conc_hist(img, m32)
    for what, t, band_rows in _sources(img, gpu):
        got = concentration_histogram(t, vectors, band_rows=band_rows)
        assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == (2, NB)
        got = got.cpu().numpy()
        assert got.sum(1).tolist() == [kept, kept], (case, what)
        assert np.array_equal(got, want_c), (case, what, int(np.abs(got - want_c).sum()))
    assert want_c[:, 1:-1].sum() > 0                               # the clamps are not all there is


def test_fit_stains_end_to_end(slide):
    img, ref = slide["img"], slide["ref"]
    gpu = torch.from_numpy(img).to(DEV)
    fit = fit_stains(gpu)
    assert isinstance(fit, StainFit) and fit.pixels == ref["pixels"] >= 5000
    assert fit.vectors.dtype == torch.float64 and tuple(fit.vectors.shape) == (2, 3) and not fit.vectors.is_cuda
    assert fit.plane.dtype == torch.float32 and tuple(fit.plane.shape) == (3, 2)
    assert (fit.alpha, fit.beta, fit.conc_percentile) == (1.0, 0.15, 99.0)
    # plane: an eigen-decomposition of the covariance of the kept OD samples, independent of the moments
    q = R.q_table()[img][R.kept(img)].reshape(-1, 3) / 4096.0
    _, vv = np.linalg.eigh(np.cov(q.T, bias=True))
    pl = fit.plane.numpy().astype(np.float64)
    for j, col in enumerate((2, 1)):
        v = vv[:, col] * np.sign(vv[:, col] @ pl[:, j])
        assert np.abs(v - pl[:, j]).max() <= 1e-6, j
    assert pl[:, 0].sum() > 0 and pl[np.abs(pl[:, 1]).argmax(), 1] > 0
    for k in range(2):
        a = _angle(fit.vectors[k].numpy(), ref["vectors"][k])
        print(f"vector {k}: {a:.2e} rad from the restatement")
        assert a <= 2e-3
    err = np.abs(fit.max_conc.numpy() - ref["max_conc"])
    print(f"max_conc {fit.max_conc.tolist()} against {ref['max_conc'].tolist()}")
    assert (err <= 2 * CONC_MAX / NB + 1e-12).all()
    assert float(fit.vectors[0, 0]) > float(fit.vectors[1, 0])
    # a fit does not depend on where the image lives, on the banding, on the run; a batch is pooled
    for t, band_rows in ((gpu, 16), (torch.from_numpy(img), None), (torch.from_numpy(img), 32), (gpu, None)):
        again = fit_stains(t, band_rows=band_rows)
        assert torch.equal(again.vectors, fit.vectors) and torch.equal(again.max_conc, fit.max_conc)
        assert torch.equal(again.plane, fit.plane) and again.pixels == fit.pixels
    halves = torch.stack([gpu[:48], gpu[48:]])
    pooled = fit_stains(halves)
    assert torch.equal(pooled.vectors, fit.vectors) and torch.equal(pooled.max_conc, fit.max_conc)


def test_fit_stains_rejects_images_without_a_stain_plane():
    blank = torch.full((40, 40, 3), 255, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="pixels"):
        fit_stains(blank)
    single = torch.tensor([120, 60, 140], dtype=torch.uint8, device=DEV).expand(40, 40, 3).contiguous()
    with pytest.raises(ValueError, match="plane"):
        fit_stains(single)
    with pytest.raises(ValueError, match="pixels"):
        fit_stains(single.cpu(), black=200)


def _apply_args(fit, reference):
    scale = (reference.max_conc.numpy() / fit.max_conc.numpy()).astype(np.float32)
    return unmix_matrix(fit.vectors).numpy(), scale, reference.vectors.numpy().astype(np.float32)


def _check_bytes(got, img, fit, reference, what):
    want, raw = R.apply64(img, *_apply_args(fit, reference))
    frac = raw - np.floor(raw)
    exempt = np.abs(frac - 0.5) <= 1e-3
    share = exempt.any(-1).mean()
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print(f"{what}: {int((diff != 0).sum())} of {diff.size} bytes differ, {share:.2%} of the pixels are exempt")
    assert share < 0.01, what                                      # a condition on the input, from the restatement alone
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert (diff[~exempt] == 0).all() and diff.max() <= 1, what
    return want


@pytest.mark.parametrize("case", list(CASES))
def test_apply_against_the_float64_restatement(case, slide):
    img, gpu = CASES[case]()
    fit = slide["fit"]
    if gpu.dim() == 4:
        out = stain_normalize(gpu, fit)
        net = stain_normalize(gpu, fit, network_input=True)
    else:
        out = normalize_region(gpu, fit)
        net = stain_normalize(gpu[None], fit, network_input=True)
        assert torch.equal(stain_normalize(gpu[None], fit)[0], out)
    assert out.dtype == torch.uint8 and tuple(out.shape) == tuple(img.shape) and out.is_cuda and out.is_contiguous()
    _check_bytes(out.cpu().numpy(), img, fit, REFERENCE_HE, case)
    batch = out if out.dim() == 4 else out[None]
    assert net.dtype == torch.float32 and tuple(net.shape) == (batch.shape[0], 3, *batch.shape[1:3])
    assert torch.isfinite(net).all()
    # what to_tensor + Normalize(0.5, 0.5) give after saving and reloading: evaluated on the host, where x / 255 is a
    # division (on the GPU torch multiplies by fp32(1 / 255), which differs in the last bit for 111 of the 256 bytes)
    assert torch.equal(net.cpu(), ((batch.cpu().float() / 255 - 0.5) / 0.5).permute(0, 3, 1, 2))
    assert np.array_equal(net.cpu().numpy(), R.network(batch.cpu().numpy()))
    aligned = torch.from_numpy(img).to(DEV).reshape(batch.shape)
    assert torch.equal(stain_normalize(aligned, fit), batch)       # the dword loads and stores give the same bytes


def test_apply_keeps_glass_white_and_maps_a_slide_onto_another(slide):
    fit = slide["fit"]
    glass = torch.full((1, 8, 12, 3), 255, dtype=torch.uint8, device=DEV)
    assert (stain_normalize(glass, fit) == 255).all()
    assert (stain_normalize(glass, fit, network_input=True) == 1).all()
    zero = torch.zeros((1, 5, 9, 3), dtype=torch.uint8, device=DEV)                # u = 0 takes the entry of u = 1
    _check_bytes(stain_normalize(zero, fit).cpu().numpy(), zero.cpu().numpy(), fit, REFERENCE_HE, "zero bytes")
    # any StainFit is a reference: slide B in slide A's colours
    other = R.synthetic_he(64, 72, 21)[0]
    g = torch.from_numpy(other).to(DEV)
    fit_b = fit_stains(g)
    out = normalize_region(g, fit_b, reference=fit)
    _check_bytes(out.cpu().numpy(), other, fit_b, fit, "slide B onto slide A")
    # fit=None fits on the input itself
    assert torch.equal(normalize_region(g), normalize_region(g, fit_b))
    assert torch.equal(stain_normalize(g[None]), stain_normalize(g[None], fit_b))
    # the identity: a slide normalised to itself moves by the rounding of the colour model alone
    same = normalize_region(g, fit_b, reference=fit_b)
    _check_bytes(same.cpu().numpy(), other, fit_b, fit_b, "slide B onto itself")


@pytest.mark.parametrize("shape,seed", [((40, 1030), 13), ((33, 7), 14)])
def test_normalize_region_host_equals_gpu(shape, seed, slide):
    img = R.synthetic_he(*shape, seed)[0]
    host = torch.from_numpy(img)
    big = torch.zeros((shape[0] + 2, shape[1] + 3, 3), dtype=torch.uint8, device=DEV)
    gpu = big[1:1 + shape[0], 2:2 + shape[1]]                      # a crop view: odd pitch, unaligned base
    gpu.copy_(host)
    base = normalize_region(gpu, slide["fit"])
    for band_rows in (16, 32):
        got = normalize_region(host, slide["fit"], band_rows=band_rows)
        assert not got.is_cuda and got.dtype == torch.uint8 and torch.equal(got, base.cpu()), band_rows
        assert torch.equal(normalize_region(gpu, slide["fit"], band_rows=band_rows), base)
    assert torch.equal(normalize_region(host, slide["fit"]), base.cpu())


def test_fitted_vectors_plug_into_stain_quantify(slide):
    img, fit = slide["img"], slide["fit"]
    thr = (0.2, 0.15, 0.1)
    got = stain_quantify(torch.from_numpy(img).to(DEV)[None], stains=fit.vectors, thresholds=thr)
    want = Q.quantify32(img[None], unmix_matrix(fit.vectors).numpy(), thr)
    assert np.array_equal(got["tissue"].cpu().numpy(), want["tissue"])
    assert np.array_equal(got["positive"].cpu().numpy(), want["positive"])
    assert want["positive"][0, 0] > 0 and want["positive"][0, 1] > 0
    assert np.abs(got["burden"].cpu().numpy() - want["burden"]).max() <= 2.0 ** -23
