"""CPU: the marshalling helpers every ctypes call shares (generativedensification_amd/_marshal.py) on CPU tensors and
plain integers: strides, optional pointers and the 256-byte workspace arithmetic."""
import ctypes as C

import pytest
import torch

from generativedensification_amd import _marshal as M


def test_strides_of_a_non_contiguous_tensor():
    t = torch.zeros(2, 3, 5, 7).permute(0, 2, 3, 1)[:, ::2]      # strides (105, 14, 1, 35)
    assert not t.is_contiguous() and t.stride() == (105, 14, 1, 35)
    s = M.strides(t)
    assert isinstance(s, C.c_int64 * 4) and list(s) == [105, 14, 1, 35]
    s3 = M.strides(t, 3)
    assert isinstance(s3, C.c_int64 * 3) and list(s3) == [105, 14, 1]


def test_ptr_of_none_and_of_a_tensor():
    assert M.ptr(None) is None
    t = torch.zeros(1)
    p = M.ptr(t)
    assert isinstance(p, C.c_void_p) and p.value == t.data_ptr()
    empty = M.ptr(torch.zeros(0))
    assert isinstance(empty, C.c_void_p)      # only None maps to None


def test_ptr_or_none_if_empty():
    assert M.ptr_or_none_if_empty(None) is None
    assert M.ptr_or_none_if_empty(torch.zeros(0)) is None
    t = torch.zeros(1)
    p = M.ptr_or_none_if_empty(t)
    assert isinstance(p, C.c_void_p) and p.value == t.data_ptr()


@pytest.mark.parametrize("k", [1, 7, 1 << 30, (1 << 40) + 3])
@pytest.mark.parametrize("off", [0, 1, 255])
def test_aligned_base(k, off):
    a, nbytes = 256 * k + off, 4096
    base, usable = M.aligned_base(a, nbytes)
    assert base % 256 == 0
    assert 0 <= base - a < 256
    assert usable == nbytes - (base - a)


def test_workspace_on_the_cpu():
    nbytes = 1000
    ws, base, usable = M.workspace(nbytes, "cpu")
    assert ws.dtype == torch.uint8 and ws.numel() == nbytes
    assert base % 256 == 0
    assert 0 <= base - ws.data_ptr() < 256
    assert usable == nbytes - (base - ws.data_ptr())


def test_rasterizer_binds_the_shared_helpers_by_name():
    from generativedensification_amd import rasterizer as R

    assert R._ptr is M.ptr_or_none_if_empty and R._stream is M.stream
