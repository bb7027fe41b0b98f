"""capi.frame_table: what the Python wrapper of orbx_extract_batch hands to the library, checked without a GPU (list typing, residency,
row strides from numpy and torch views)."""
import numpy as np
import pytest
import torch

from orb_slam_amd import capi


class _FakeDeviceTensor:
    """stands in for a CUDA tensor (is_cuda) on a machine without a GPU; frame_table only reads its layout"""

    def __init__(self, h, w, row_stride, addr):
        self.is_cuda, self.dtype, self.shape = True, torch.uint8, (h, w)
        self._rs, self._addr = row_stride, addr

    def dim(self):
        return 2

    def stride(self, i):
        return (self._rs, 1)[i]

    def data_ptr(self):
        return self._addr


def test_symbol_is_bound():
    assert "orbx_extract_batch" in capi.EXPORTS and hasattr(capi.ORBextractor, "extract_batch")
    assert (capi.FRAMES_ON_DEVICE, capi.FRAMES_ON_HOST) == (0, 1)


def test_numpy_views_keep_their_row_stride_and_base():
    big = np.zeros((3, 48, 100), dtype=np.uint8)
    views = [big[f, :, 5:69] for f in range(3)]
    where, ptrs, strides, w, h, keep = capi.frame_table(views)
    assert where == capi.FRAMES_ON_HOST and (w, h) == (64, 48)
    assert list(strides) == [100] * 3
    assert [int(p) for p in ptrs] == [big.ctypes.data + f * 48 * 100 + 5 for f in range(3)]
    assert ptrs.dtype == np.uint64 and strides.dtype == np.int64


def test_numpy_with_non_contiguous_rows_is_copied():
    a = np.arange(40 * 64, dtype=np.uint8).reshape(40, 64)
    col = a[:, ::2]                                          # stride(1) == 2: not a pitched frame
    where, ptrs, strides, w, h, keep = capi.frame_table([col])
    assert (w, h) == (32, 40) and strides[0] == 32 and np.array_equal(keep[0], col)
    assert int(ptrs[0]) == keep[0].ctypes.data


def test_cpu_tensors_are_host_frames():
    t = torch.zeros((30, 80), dtype=torch.uint8)
    v = t[:, 10:60]
    where, ptrs, strides, w, h, _ = capi.frame_table([t, t])
    assert where == capi.FRAMES_ON_HOST and (w, h) == (80, 30) and list(strides) == [80, 80]
    with pytest.raises(ValueError):                          # sizes differ
        capi.frame_table([t, v])
    where, ptrs, strides, w, h, _ = capi.frame_table([v, v])
    assert where == capi.FRAMES_ON_HOST and (w, h) == (50, 30) and list(strides) == [80, 80] and int(ptrs[0]) == v.data_ptr()


def test_cpu_tensor_with_non_contiguous_rows_is_copied_like_numpy():
    t = torch.arange(40 * 64, dtype=torch.int32).to(torch.uint8).reshape(40, 64)
    col = t[:, ::2]
    where, ptrs, strides, w, h, keep = capi.frame_table([col])
    assert where == capi.FRAMES_ON_HOST and (w, h) == (32, 40) and strides[0] == 32
    assert torch.equal(keep[0], col) and int(ptrs[0]) == keep[0].data_ptr()


def test_device_tensors_give_the_device_form():
    frames = [_FakeDeviceTensor(48, 64, 64 + 16 * f, 4096 * (f + 1)) for f in range(3)]
    where, ptrs, strides, w, h, _ = capi.frame_table(frames)
    assert where == capi.FRAMES_ON_DEVICE and (w, h) == (64, 48)
    assert list(strides) == [64, 80, 96] and [int(p) for p in ptrs] == [4096, 8192, 12288]


def test_mixed_residency_and_bad_frames_raise():
    dev = _FakeDeviceTensor(48, 64, 64, 4096)
    with pytest.raises(ValueError):
        capi.frame_table([dev, np.zeros((48, 64), np.uint8)])
    with pytest.raises(ValueError):
        capi.frame_table([])
    with pytest.raises(ValueError):
        capi.frame_table([np.zeros((48, 64), np.int16)])
    with pytest.raises(ValueError):
        capi.frame_table([np.zeros((2, 48, 64), np.uint8)])
    bad = _FakeDeviceTensor(48, 64, 64, 4096)
    bad.stride = lambda i: (128, 2)[i]
    with pytest.raises(ValueError):
        capi.frame_table([bad])
