"""The layout and device functions every whole-region call shares (stain2stain_amd._regionio), on host tensors: what a
region or a batch may look like in memory, which pitch and stride the kernels are given, and what is refused."""
import pytest
import torch

from stain2stain_amd._regionio import DEFAULT_HOST_BAND, batch_layout, check_region, gpu_device, gpu_rows

H, W = 21, 17


def _big():
    return torch.arange(40 * 32 * 3, dtype=torch.int64).remainder(251).to(torch.uint8).reshape(40, 32, 3)


def _planar():
    """[H, W, 3] over channel planes: what a [3, H, W] image permuted to channels-last looks like."""
    return _big().permute(2, 0, 1).contiguous().permute(1, 2, 0)


# ---- check_region ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("y0,x0", [(5, 3), (4, 8)])           # misaligned and 4-byte aligned row starts
def test_region_contiguous_and_crop_views(y0, x0):
    big = _big()
    assert check_region(big, "t") == (40, 32, 3)
    view = big[y0:y0 + H, x0:x0 + W]
    assert not view.is_contiguous() and (view.data_ptr() - big.data_ptr()) % 4 == (0 if x0 == 8 else 1)
    assert check_region(view, "t") == (H, W, 3)
    assert check_region(view, "t", mask_ok=True) == (H, W, 3)


def test_region_of_one_row_or_one_column():
    big = _big()
    assert check_region(big[7:8, 3:20], "t") == (1, 17, 3)
    assert check_region(big[3:20, 7:8], "t") == (17, 1, 3)            # one pixel a row: its column stride is free
    assert check_region(big[3:20:2, 7:8], "t") == (9, 1, 3)
    assert check_region(big[3:20, 7:8, 0], "t", mask_ok=True) == (17, 1, 1)


def test_mask_only_when_asked_for():
    mask = _big()[..., 0].contiguous()
    assert check_region(mask, "t", mask_ok=True) == (40, 32, 1)
    assert check_region(mask[3:20, 5:9], "t", mask_ok=True) == (17, 4, 1)
    with pytest.raises(ValueError, match=r"t: the region must be a non-empty \[H, W, 3\] RGB image"):
        check_region(mask, "t")
    with pytest.raises(ValueError, match="pixels within a row must be contiguous"):
        check_region(_big()[..., 0], "t", mask_ok=True)                # a channel of an image: column stride 3
    with pytest.raises(ValueError, match="image or .* mask"):
        check_region(_big()[None], "t", mask_ok=True)


def test_region_rejects():
    big = _big()
    with pytest.raises(TypeError, match="t: the region must be a torch.Tensor"):
        check_region(big.numpy(), "t")
    with pytest.raises(ValueError, match="t: the region must be uint8"):
        check_region(big.float(), "t")
    for bad in (big[..., :2], big[None], big[0], big[:0], big[:, :0]):  # channels, rank, empty
        with pytest.raises(ValueError, match="non-empty"):
            check_region(bad, "t")
    for bad in (_planar(), big[:, ::2], big.transpose(0, 1)):         # channel planes, every other pixel, columns
        with pytest.raises(ValueError, match="t: pixels within a row must be contiguous"):
            check_region(bad, "t")
    # host rows may overlap: a host region is copied row by row, only a GPU view's pitch goes to a kernel
    assert check_region(big.as_strided((8, 10, 3), (12, 3, 1)), "t") == (8, 10, 3)


# ---- gpu_rows --------------------------------------------------------------------------------------------------------
def test_rows_checks_come_before_the_device():
    big = _big()
    with pytest.raises(RuntimeError, match="rows overlap"):
        gpu_rows(big.as_strided((8, 10, 3), (29, 3, 1)))                # pitch 29 < 3 * 10
    with pytest.raises(RuntimeError, match="rows overlap"):
        gpu_rows(big[..., 0].contiguous().as_strided((8, 10), (9, 1)))
    with pytest.raises(RuntimeError, match="contiguous within a row"):
        gpu_rows(_planar())
    with pytest.raises(RuntimeError, match="expected a uint8"):
        gpu_rows(big.float())
    with pytest.raises(RuntimeError, match="expected a uint8"):
        gpu_rows(big[..., :2])
    for ok in (big, big[5:26, 3:20], big[7:8], big[..., 0].contiguous()):
        with pytest.raises(RuntimeError, match="not on the GPU"):
            gpu_rows(ok)                                                # a sound view is refused only for where it lives


# ---- batch_layout ----------------------------------------------------------------------------------------------------
def test_batch_pitch_and_stride():
    big = _big().reshape(4, 10, 32, 3)
    t, pitch, stride = batch_layout(big, "t")
    assert t is big and (pitch, stride) == (96, 960)
    for x0 in (3, 8):                                                   # misaligned and 4-byte aligned starts
        view = big[1:3, 2:9, x0:x0 + 17]
        t, pitch, stride = batch_layout(view, "t")
        assert t is view and t.data_ptr() == view.data_ptr() and (pitch, stride) == (96, 960)
    masks = big[..., 1].contiguous()
    assert batch_layout(masks[:, 2:9, 3:20], "t")[1:] == (32, 320)


def test_batch_edge_rules():
    big = _big().reshape(4, 10, 32, 3)
    one_row = big[:, 4:5, 3:20]                                         # H == 1: the pitch is C * W, not the view's
    assert batch_layout(one_row, "t")[1:] == (51, 960)
    one_sample = big[2:3, 2:9, 3:20]                                    # B == 1: the stride is pitch * H
    assert batch_layout(one_sample, "t")[1:] == (96, 96 * 7)
    both = big[2:3, 4:5, 3:20]
    assert batch_layout(both, "t")[1:] == (51, 51)
    one_column = big[:, :, 5:6]                                         # W == 1: the column stride is free
    assert batch_layout(one_column, "t")[1:] == (96, 960)
    assert batch_layout(big[:, :, 5:6, 0], "t")[1:] == (96, 960)


def test_batch_overlap_is_rejected():
    flat = _big().reshape(-1)
    with pytest.raises(ValueError, match="t: the rows or samples of src_u8 overlap"):
        batch_layout(flat.as_strided((2, 8, 10, 3), (400, 29, 3, 1)), "t", "src_u8")      # pitch < 3 * W
    with pytest.raises(ValueError, match="overlap"):
        batch_layout(flat.as_strided((2, 8, 10, 3), (200, 30, 3, 1)), "t")               # stride < pitch * H
    with pytest.raises(ValueError, match="overlap"):
        batch_layout(flat.as_strided((2, 8, 10), (40, 9, 1)), "t")
    assert batch_layout(flat.as_strided((2, 8, 10, 3), (240, 30, 3, 1)), "t")[1:] == (30, 240)


def test_batch_interleaved_samples():
    """The cells of one cell row of a region: sample stride 3 * cell, far below pitch * H."""
    region = _big()                                                      # 40 x 32: a row of four 8 x 8 cells
    band = region[8:16]
    cells = band.as_strided((4, 8, 8, 3), (24, 96, 3, 1))
    with pytest.raises(ValueError, match="overlap"):
        batch_layout(cells, "t")
    t, pitch, stride = batch_layout(cells, "t", interleave=True)
    assert t is cells and (pitch, stride) == (96, 24)
    assert torch.equal(cells[2], region[8:16, 16:24])
    with pytest.raises(ValueError, match="overlap"):                     # rows still must not overlap
        batch_layout(band.as_strided((4, 8, 8, 3), (24, 23, 3, 1)), "t", interleave=True)
    with pytest.raises(ValueError, match="overlap"):                     # and a stride of 0 repeats a sample
        batch_layout(band.as_strided((4, 8, 8, 3), (0, 96, 3, 1)), "t", interleave=True)


@pytest.mark.parametrize("kind", ["planar", "transposed", "strided", "mask_transposed"])
def test_batch_non_contiguous_pixels_copied_or_rejected(kind):
    big = _big().reshape(4, 10, 32, 3)
    view = {"planar": big.permute(3, 0, 1, 2).contiguous().permute(1, 2, 3, 0), "transposed": big.transpose(1, 2),
            "strided": big[:, :, ::2],
            "mask_transposed": big[..., 0].contiguous().transpose(1, 2)}[kind]
    with pytest.raises(ValueError, match="t: the pixels of tiles_u8 must be contiguous within a row"):
        batch_layout(view, "t", "tiles_u8")
    t, pitch, stride = batch_layout(view, "t", copy=True)
    B, h, w = view.shape[:3]
    c = 3 if view.dim() == 4 else 1
    assert t is not view and t.is_contiguous() and torch.equal(t, view) and (pitch, stride) == (c * w, c * w * h)


# ---- gpu_device ------------------------------------------------------------------------------------------------------
def test_default_band():
    assert DEFAULT_HOST_BAND == 512


def test_device_of_host_tensors():
    a = torch.zeros((4, 4, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match=r"some_call needs GPU tensors \(there is no CPU path\)"):
        gpu_device("some_call", a, host_ok=False)
    if torch.cuda.is_available():
        assert gpu_device("some_call", a, a) == torch.device("cuda", torch.cuda.current_device())
    else:
        with pytest.raises(RuntimeError, match=r"some_call needs a GPU \(there is no CPU path\)"):
            gpu_device("some_call", a, a)


def test_device_rules_on_stand_ins():
    """No second GPU is needed to state the rules: the function looks at ``is_cuda`` and ``device`` alone."""
    class T:
        def __init__(self, device):
            self.device = torch.device(device)
            self.is_cuda = self.device.type == "cuda"

    assert gpu_device("c", T("cpu"), T("cuda:1")) == torch.device("cuda:1")            # any GPU tensor decides
    assert gpu_device("c", T("cuda:1"), T("cuda:1"), host_ok=False) == torch.device("cuda:1")
    with pytest.raises(RuntimeError, match="c: the tensors are on different devices"):
        gpu_device("c", T("cuda:0"), T("cpu"), T("cuda:1"))
    with pytest.raises(ValueError, match="different devices"):
        gpu_device("c", T("cuda:0"), T("cuda:1"), mismatch=ValueError)
    with pytest.raises(RuntimeError, match="needs GPU tensors"):
        gpu_device("c", T("cuda:0"), T("cpu"), host_ok=False)
