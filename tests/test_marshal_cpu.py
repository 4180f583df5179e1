"""CPU: the marshalling helpers every ctypes call shares (generativedensification_amd/_marshal.py) on CPU tensors and
plain integers: strides, optional pointers, the 256-byte workspace arithmetic, and the argument checks and row layouts
of the row kernels' wrappers."""
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


def test_one_dtype_map_serves_every_module():
    from generativedensification_amd import _lib as L
    from generativedensification_amd import attention, segment, serattn, sparse_conv

    assert M.DTYPES == {torch.float16: 0, torch.bfloat16: 1, torch.float32: 2}
    assert L.GDR_NORM_DTYPES is L.GDR_DTYPES and L.GDR_SUBM_DTYPES is L.GDR_DTYPES
    assert L.GDR_SEG_DTYPES == {**L.GDR_DTYPES, "i64": 3}
    assert (L.GDR_ATTN_F16, L.GDR_ATTN_BF16, L.GDR_ATTN_F32) == tuple(L.GDR_DTYPES[k] for k in ("f16", "bf16", "f32"))
    assert serattn._DTYPES is M.DTYPES and sparse_conv._DTYPES is M.DTYPES
    assert attention._DTYPES == {torch.float16: 0, torch.bfloat16: 1}
    assert segment._DTYPES == {**M.DTYPES, torch.int64: 3}


def _aligned_rows(n, c, dtype=torch.float32):
    """(n, c) zeros whose base is 16-byte aligned, whatever the allocator returns"""
    buf = torch.zeros(n * c + 16, dtype=dtype)
    off = (-buf.data_ptr() % 16) // buf.element_size()
    return buf[off:off + n * c].view(n, c)


def test_rows2d_keeps_a_strided_view_whose_rows_are_aligned():
    t = _aligned_rows(6, 32)[:, :24]                # row stride 32, 24 channels
    assert not t.is_contiguous() and t.stride() == (32, 1) and t.data_ptr() % 16 == 0
    assert M.rows2d(t) is t and M.stride0(t) == 32
    empty = t[:0]
    assert M.rows2d(empty) is empty


@pytest.mark.parametrize("make", [
    lambda: _aligned_rows(6, 32).view(-1)[4:4 + 5 * 32].view(5, 32)[:, 1:17],         # an odd base: 4-byte, not 16-byte aligned
    lambda: _aligned_rows(6, 36)[:, :32],                                              # a row stride that is no multiple of 8
    lambda: _aligned_rows(32, 6).t(),                                                  # channels that are not unit-stride
    lambda: _aligned_rows(6, 32).expand(2, 6, 32)[0].as_strided((6, 32), (8, 1)),      # a row stride below the row
], ids=["odd-base", "stride-not-8", "channel-stride", "stride-below-row"])
def test_rows2d_copies_what_the_kernels_cannot_read(make):
    t = make()
    r = M.rows2d(t)
    assert r is not t and r.is_contiguous() and torch.equal(r, t) and M.stride0(r) == t.shape[1]


def test_stride0_of_a_one_row_tensor():
    """torch reports any stride for one row: the kernels get the least they accept"""
    assert M.stride0(torch.zeros(1, 32)) == 32 and M.stride0(torch.zeros(1, 4)) == 8
    assert M.stride0(torch.zeros(1, 12)) == 12 and M.stride0(torch.zeros(1, 12), pad=True) == 16
    assert M.stride0(torch.zeros(1, 32).as_strided((1, 32), (7, 1))) == 32
    assert M.stride0(_aligned_rows(2, 32)[:, :24]) == 32


def test_rows2d_pads_a_copy_of_rows_that_are_no_multiple_of_8():
    t = _aligned_rows(5, 13)[:, :12]                # stride 13: must be copied; 12 channels need a stride of 16
    r = M.rows2d(t, pad=True)
    assert r.shape == (5, 12) and r.stride() == (16, 1) and r.data_ptr() % 16 == 0 and torch.equal(r, t)
    assert M.stride0(r, pad=True) == 16
    assert M.rows2d(t).stride() == (12, 1)          # without `pad`: the dense copy of the other modules
    u = _aligned_rows(5, 16)[:, :12]
    assert M.rows2d(u, pad=True) is u


def test_check_float_dtype_and_rank_messages():
    M.check_float("x", torch.zeros(2, 3, dtype=torch.bfloat16))
    M.check_float("x", torch.zeros(2, 3, dtype=torch.float16), 2)
    with pytest.raises(TypeError, match=r"^x must be a tensor, not list$"):
        M.check_float("x", [1.0])
    with pytest.raises(TypeError, match=r"^feat must be float32, float16 or bfloat16, not torch\.float64$"):
        M.check_float("feat", torch.zeros(2, 3, dtype=torch.float64))
    with pytest.raises(TypeError, match=r"^feat must be float32, float16 or bfloat16, not torch\.int64$"):
        M.check_float("feat", torch.zeros(2, 3, dtype=torch.int64), 2)
    with pytest.raises(ValueError, match=r"^feat must have 2 dimensions, got \(2, 3, 4\)$"):
        M.check_float("feat", torch.zeros(2, 3, 4), 2)
    with pytest.raises(ValueError, match=r"^frequencies must have 1 dimension, got \(2, 3\)$"):
        M.check_float("frequencies", torch.zeros(2, 3), 1)


def test_check_devices_raises_the_modules_own_sentence_on_cpu_tensors():
    text = "the HIP row normalisations run on ROCm/HIP tensors only (no CPU fallback)"
    with pytest.raises(RuntimeError) as e:
        M.check_devices((("feat", torch.zeros(2, 8)), ("scale", torch.zeros(1, 8))), text)
    assert str(e.value) == text


def test_dense_aligned_passes_none_and_copies_an_odd_base():
    assert M.dense_aligned(None) is None
    t = _aligned_rows(4, 8)
    assert M.dense_aligned(t) is t
    odd = _aligned_rows(5, 8).view(-1)[1:33].view(4, 8)
    r = M.dense_aligned(odd)
    assert odd.data_ptr() % 16 and r.data_ptr() % 16 == 0 and r.is_contiguous() and torch.equal(r, odd)
