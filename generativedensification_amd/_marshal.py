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


# torch dtype -> the storage type code of the row kernels (GDR_NORM_F16 / BF16 / F32)
NORM_DTYPES = {torch.float16: L.GDR_NORM_DTYPES["f16"], torch.bfloat16: L.GDR_NORM_DTYPES["bf16"],
               torch.float32: L.GDR_NORM_DTYPES["f32"]}


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
    """`rows` dense from a 16-byte aligned base: itself where it is so already, one copy otherwise"""
    if rows.numel() and (not rows.is_contiguous() or rows.data_ptr() % 16):
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
