"""What every ctypes call into libgdr_hip.so marshals the same way: the current stream, tensor strides, optional device
pointers and the 256-byte aligned workspace.  Imported as `M`; a new module takes these from here."""
from __future__ import annotations

import ctypes as C

import torch

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
