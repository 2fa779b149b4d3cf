"""The pinned-band streaming every whole-region call shares (stain2stain_amd._regionio) on the GPU: a host region goes up
through a ``BandSource`` and comes back through a ``BandSink`` byte for byte, whatever its pitch, its kind and the
banding; a GPU region is read in place."""
import pytest
import torch

from stain2stain_amd._regionio import BandSink, BandSource, gpu_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, BAND = 37, 45, 8                                          # bands of 8 rows, the last one ragged: 5 rows


def _slide(channels=True):
    g = torch.Generator().manual_seed(11)
    return torch.randint(0, 256, (60, 64, 3) if channels else (60, 64), generator=g, dtype=torch.uint8)


def _round_trip(region, band, f_channels=None):
    """Every band of ``region`` up through a source, copied on the device, and down through a sink."""
    h = region.shape[0]
    dev = torch.device(DEV)
    src = BandSource(region, band, dev)
    sink = BandSink(region.shape, band, f_channels)
    out = torch.empty((band,) + tuple(region.shape[1:]), dtype=torch.uint8, device=dev)
    out_f = torch.empty((band, region.shape[1], f_channels), dtype=torch.float32, device=dev) if f_channels else None
    sizes = []
    for r0 in range(0, h, band):
        r1 = min(r0 + band, h)
        rows = src.rows(r0, r1)
        assert rows.is_cuda and tuple(rows.shape) == (r1 - r0,) + tuple(region.shape[1:])
        ptr, pitch = gpu_rows(rows)
        assert ptr == rows.data_ptr() and pitch == rows[0].numel()
        out[:r1 - r0].copy_(rows)
        if f_channels:                                          # channel c of row r, column x: a value of its own
            y = torch.arange(r0, r1, device=dev, dtype=torch.float32)[:, None, None]
            x = torch.arange(region.shape[1], device=dev, dtype=torch.float32)[None, :, None]
            c = torch.arange(f_channels, device=dev, dtype=torch.float32)[None, None, :]
            out_f[:r1 - r0].copy_(y * 1000.0 + x + c / 8.0)
        sink.put(out, r0, r1, out_f)
        sizes.append(r1 - r0)
    return src, sink.close(), sizes


@pytest.mark.parametrize("channels", [True, False], ids=["image", "mask"])
def test_host_crop_view_round_trip(channels):
    region = _slide(channels)[13:13 + H, 7:7 + W]               # padded rows, a misaligned start
    assert not region.is_contiguous()
    src, (u8, f), sizes = _round_trip(region, BAND)
    assert sizes == [8, 8, 8, 8, 5]
    assert not src.on_gpu and src.band_bytes == BAND * W * (3 if channels else 1)
    assert f is None and not u8.is_cuda and u8.dtype == torch.uint8 and u8.is_contiguous()
    assert tuple(u8.shape) == tuple(region.shape) and torch.equal(u8, region)


def test_fp32_side_result_of_five_channels():
    region = _slide()[4:4 + H, 8:8 + W]
    _, (u8, f), _ = _round_trip(region, BAND, f_channels=5)
    assert torch.equal(u8, region)
    assert not f.is_cuda and f.dtype == torch.float32 and tuple(f.shape) == (H, W, 5)
    y = torch.arange(H, dtype=torch.float32)[:, None, None]
    x = torch.arange(W, dtype=torch.float32)[None, :, None]
    c = torch.arange(5, dtype=torch.float32)[None, None, :]
    assert torch.equal(f, y * 1000.0 + x + c / 8.0)             # small integers and eighths: exact in fp32


def test_gpu_region_is_read_in_place():
    region = _slide().to(DEV)[13:13 + H, 7:7 + W]
    src = BandSource(region, BAND, torch.device(DEV))
    assert src.on_gpu and src.band_bytes == 0 and not hasattr(src, "band") and not hasattr(src, "stage")
    rows = src.rows(16, 24)
    assert rows.data_ptr() == region[16:24].data_ptr() and rows.stride() == region.stride()
    assert src.rows(0, H).data_ptr() == region.data_ptr()
    assert gpu_rows(rows) == (region[16:24].data_ptr(), 64 * 3)


def test_one_band_taller_than_the_region():
    region = _slide()[20:23, 5:5 + W]                           # H = 3 in a band of 8
    src, (u8, f), sizes = _round_trip(region, BAND)
    assert sizes == [3] and src.band_bytes == BAND * W * 3
    assert tuple(u8.shape) == (3, W, 3) and torch.equal(u8, region)
