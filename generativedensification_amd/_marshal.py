"""What every ctypes call into libgdr_hip.so marshals the same way: the current stream, tensor strides, optional device
pointers and the 256-byte aligned workspace.  Imported as `M`; a new module takes these from here."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L

raw_stream = torch._C._cuda_getCurrentRawStream   # (torch.cuda.current_stream() builds a Stream object: 9 us per call)


def stream():
    """The current device's current stream (= torch.cuda.current_stream().cuda_stream) as a c_void_p."""
    return C.c_void_p(raw_stream(torch.cuda.current_device()))


def strides(t: torch.Tensor, dims=None):
    """The first `dims` element strides of `t` (all of them by default) as a c_int64 array."""
    s = t.stride() if dims is None else t.stride()[:dims]
    return (C.c_int64 * len(s))(*s)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def ptr_or_none_if_empty(t):
    return None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())


def aligned_base(addr: int, nbytes: int):
    """(base, usable): `addr` rounded up to 256 bytes and what is left of `nbytes` behind it."""
    base = (addr + 255) & ~255
    return base, nbytes - (base - addr)


def workspace(nbytes: int, dev):
    """A uint8 workspace of `nbytes` on `dev` as (tensor, base, usable bytes); keep the tensor alive through the call."""
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return (ws, *aligned_base(ws.data_ptr(), nbytes))


# torch dtype -> storage type code (include/gdr.h GDR_F16 / GDR_BF16 / GDR_F32): the one map; a module that takes fewer
# types, or more, derives its own from this
DTYPES = {torch.float16: L.GDR_DTYPES["f16"], torch.bfloat16: L.GDR_DTYPES["bf16"], torch.float32: L.GDR_DTYPES["f32"]}


def check_float(name, t, dims=None):
    """`t` is a tensor of a dtype in DTYPES, with `dims` dimensions where that is given."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a tensor, not {type(t).__name__}")
    if t.dtype not in DTYPES:
        raise TypeError(f"{name} must be float32, float16 or bfloat16, not {t.dtype}")
    if dims is not None and t.dim() != dims:
        raise ValueError(f"{name} must have {dims} dimension{'s' if dims > 1 else ''}, got {tuple(t.shape)}")


def check_devices(named, no_cpu_text):
    """Every (name, tensor) of `named` is on the GPU (else `no_cpu_text`, the module's own sentence) and on the first one's."""
    for name, t in named:
        if not t.is_cuda:
            raise RuntimeError(no_cpu_text)
    dev = named[0][1].device
    for name, t in named:
        if t.device != dev:
            raise RuntimeError(f"{name} must live on {named[0][0]}'s device ({dev}), not {t.device}")


def up8(c):
    return (c + 7) // 8 * 8


def rows2d(t, pad=False):
    """t (rows, C) as the kernels read rows (host_util.h bad_rows): unit channel stride, a 16-byte aligned base, a row stride
    that is a multiple of 8 and covers the row; itself where it is so already, one copy otherwise.  `pad`: the caller's C may
    be no multiple of 8 (viewattn.py, H heads of 4), where only a copy with a padded stride has aligned rows."""
    N, C = t.shape
    if N and (t.stride(1) != 1 or t.stride(0) % 8 or t.stride(0) < C or t.data_ptr() % 16):
        if not pad or C % 8 == 0:
            return t.contiguous()
        buf = torch.empty(N, up8(C), dtype=t.dtype, device=t.device)[:, :C]
        buf.copy_(t)
        return buf
    return t


def stride0(t, pad=False):
    """The row stride to pass for rows2d's `t`.  torch reports any stride for a one-row tensor, so that one gets the least
    the kernels accept: max(C, 8), or C rounded up to 8 for a caller with `pad`."""
    if t.shape[0] > 1:
        return t.stride(0)
    return up8(t.shape[1]) if pad else max(t.shape[1], 8)


def queried_workspace(query, name, dev, *args):
    """A workspace of the `query(*args)` bytes a gdr_*_workspace_bytes function `name` asks for, with the slack to align its
    base; a 0 answer is the library's refusal and raises its text."""
    nbytes = query(*args)
    if nbytes == 0:
        L.check(-1, name)
    return workspace(nbytes + 256, dev)


def dense(t):
    """`t` (or None) contiguous: itself where it is so already"""
    return t if t is None or t.is_contiguous() else t.contiguous()


def dense_aligned(rows):
    """`rows` (or None) dense from a 16-byte aligned base: itself where it is so already, one copy otherwise"""
    if rows is not None and rows.numel() and (not rows.is_contiguous() or rows.data_ptr() % 16):
        rows = rows.contiguous()
        if rows.data_ptr() % 16:
            rows = rows.clone()
    return rows


def f32_contiguous(name, t, shape, dev=None):
    """`t` as the kernels read it: a float32 tensor of `shape` (None = any extent) on `dev`, contiguous.  Shapes are
    refused with a ValueError, other dtypes and devices with a TypeError / RuntimeError, before any launch."""
    if not isinstance(t, torch.Tensor) or t.dim() != len(shape) or any(w is not None and s != w for s, w in zip(t.shape, shape)):
        want = "(" + ", ".join("*" if w is None else str(w) for w in shape) + ")"
        raise ValueError(f"{name} must be a {want} tensor, got {tuple(getattr(t, 'shape', ()))}")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, not {t.dtype}")
    if dev is not None and t.device != dev:
        raise RuntimeError(f"{name} is on {t.device}, the other tensors on {dev}")
    return t.contiguous()


def rays_and_view(rays, viewmatrix, H, W, dev):
    """rays (H,W,6) and the 4x4 view matrix as float32 contiguous tensors on `dev` (cameras keep them in any float type and
    on any device, so these two are converted, not refused)."""
    if not isinstance(rays, torch.Tensor) or tuple(rays.shape) != (H, W, 6):
        raise ValueError(f"rays must be a ({H}, {W}, 6) tensor, got {tuple(getattr(rays, 'shape', ()))}")
    if not isinstance(viewmatrix, torch.Tensor) or tuple(viewmatrix.shape) != (4, 4):
        raise ValueError(f"viewmatrix must be a (4, 4) tensor, got {tuple(getattr(viewmatrix, 'shape', ()))}")
    return (rays.to(device=dev, dtype=torch.float32).contiguous(), viewmatrix.to(device=dev, dtype=torch.float32).contiguous())
