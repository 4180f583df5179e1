"""Dense 3x3x3 convolution of channels-last volumes on the MI355X (csrc/conv3d.hip, include/gdr.h gdr_conv3d_*): the
`nn.Conv3d(C, C, 3, padding=1, bias=False)` at the tail of the reference's `GroupAttBlock` (lightning/network.py), on volumes
stored `channels_last_3d`, where a voxel is one contiguous C-element row: what the fused norms of groupattn.py produce and
consume.

    conv3d(x, weight, bias=None, add_input=False)   = F.conv3d(x, weight, bias, padding=1)  [+ x, in the same launch]
    conv3d_of(module, x, add_input=False)           the same with an nn.Conv3d's parameters; refuses other settings
    in_envelope(B, Cin, Cout, D, H, W)              whether the kernels serve this shape

x is (B, Cin, D, H, W), weight (Cout, Cin, 3, 3, 3) in nn.Conv3d's own layout, bias (Cout,) or None; the result is
(B, Cout, D, H, W) with dense channels_last_3d strides.  Stride 1, zero padding 1, dilation 1, groups 1, cross-correlation.
`add_input=True` needs Cin == Cout and returns x + conv(x): the sum is formed in the kernel's epilogue on the float32
accumulator and rounded once.

Layout: a dense channels_last_3d x with a 16-byte aligned base is read in place (a stride of a size-1 axis is never looked
at); anything else (NCDHW-contiguous, a channel slice, an unaligned base) is made so with one copy.
Dtypes: x is float32, float16 or bfloat16 and its dtype is the compute dtype; weight and bias may each be any of the three
and are rounded to the compute dtype by the pack kernel (what autocast's cast does, without a tensor of the rounded
parameter); sums are float32; the result and grad_x have x's dtype; grad_weight and grad_bias come back in the parameters'
dtypes, rounded once from the float32 sums.
Autocast: like torch's conv3d, under an enabled CUDA autocast a float32 x is first cast to the autocast dtype; the Function
itself runs with autocast disabled.
Autograd: once differentiable; only x and weight are saved; a gradient nobody needs is not computed (a frozen weight
launches no weight gradient).  grad_x is the same product kernel on grad_out with the weight transposed and tap-mirrored,
and with `add_input` the grad_out row is added in that kernel's epilogue.
The kernels use no atomics (two calls are bitwise equal) and never synchronise with the host.  GPU tensors only (no CPU
fallback).  Wrong dtypes raise TypeError, shapes outside the envelope ValueError, all before any launch.  Envelope: Cin and
Cout multiples of 8 in 8..MAX_CHANNELS, D, H, W >= 1, B D H W <= MAX_ROWS.  B = 0 or an empty axis returns an empty tensor
without loading the library.  Non-finite inputs are memory-safe and otherwise unspecified.
"""
from __future__ import annotations

import torch

from . import _lib as L
from . import _marshal as M

__all__ = ["conv3d", "conv3d_of", "covers", "in_envelope", "MAX_CHANNELS", "MAX_ROWS", "BRICK"]

MAX_CHANNELS = L.GDR_CONV3D_MAX_CHANNELS
MAX_ROWS = (1 << 31) - 1
BRICK = L.GDR_CONV3D_BRICK          # voxels (D, H, W) of one workgroup of the product kernel

_DTYPES = M.DTYPES
_NO_CPU = "the HIP convolution runs on ROCm/HIP tensors only (no CPU fallback)"


def in_envelope(B, Cin, Cout, D, H, W):
    """whether the kernels serve this shape"""
    return (all(8 <= c <= MAX_CHANNELS and c % 8 == 0 for c in (Cin, Cout)) and B >= 0 and min(D, H, W) >= 1
            and B * D * H * W <= MAX_ROWS)


def _rows(x):
    """x (B, C, D, H, W) as its (B, D, H, W, C) rows, dense from a 16-byte aligned base: a view of a channels_last_3d x (the
    strides of size-1 axes do not count), one copy of anything else"""
    return M.dense_aligned(x.permute(0, 2, 3, 4, 1))


def _workspace(lib, what, dt, voxels, cin, cout, dev):
    return M.queried_workspace(lib.gdr_conv3d_workspace_bytes, "gdr_conv3d_workspace_bytes", dev, what, dt, voxels, cin, cout)


def _product(lib, rows, dt, weight, mirrored, bias, addend, out, dev):
    """out rows = [bias +] [addend +] the convolution of `rows` with `weight` (mirrored: its transposed, tap-mirrored form)"""
    B, D, H, W, ca = rows.shape
    cb = out.shape[-1]
    cout, cin = weight.shape[:2]
    ws, base, _ = _workspace(lib, L.GDR_CONV3D_WS_PACKED, dt, 0, cin, cout, dev)
    L.check(lib.gdr_conv3d_pack_weight(weight.data_ptr(), _DTYPES[weight.dtype], cin, cout, int(mirrored), base, dt, M.stream()),
            "gdr_conv3d_pack_weight")
    L.check(lib.gdr_conv3d_forward(rows.data_ptr(), dt, base, M.ptr(bias), _DTYPES[bias.dtype] if bias is not None else dt,
                                   M.ptr(addend), B, D, H, W, ca, cb, out.data_ptr(), M.stream()), "gdr_conv3d_forward")


class _Conv3d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, add_input):
        dev = x.device
        rows = _rows(x)
        B, D, H, W, cin = rows.shape
        cout = weight.shape[0]
        w, b = M.dense(weight), M.dense(bias)
        with torch.cuda.device(dev):
            out = torch.empty(B, D, H, W, cout, dtype=x.dtype, device=dev)
            if out.numel():
                _product(L.load(), rows, _DTYPES[x.dtype], w, False, b, rows if add_input else None, out, dev)
        ctx.save_for_backward(rows, w)
        ctx.add_input = add_input
        ctx.bias = None if bias is None else (bias.dtype, bias.shape)
        return out.permute(0, 4, 1, 2, 3)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        rows, w = ctx.saved_tensors
        B, D, H, W, cin = rows.shape
        cout, dev, dt = w.shape[0], rows.device, _DTYPES[rows.dtype]
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.bias is not None and ctx.needs_input_grad[2]
        if grad_out.dtype != rows.dtype:
            grad_out = grad_out.to(rows.dtype)
        g = _rows(grad_out)
        n = B * D * H * W
        grad_x = grad_w = grad_b = None
        with torch.cuda.device(dev):
            lib = L.load() if n else None
            if need_x:
                grad_rows = torch.empty_like(rows)
                if n:
                    _product(lib, g, dt, w, True, None, g if ctx.add_input else None, grad_rows, dev)
                grad_x = grad_rows.permute(0, 4, 1, 2, 3)
            if need_w:
                grad_w = torch.zeros_like(w) if not n else torch.empty_like(w)
                if n:
                    ws, base, usable = _workspace(lib, L.GDR_CONV3D_WS_GRAD_WEIGHT, dt, n, cin, cout, dev)
                    L.check(lib.gdr_conv3d_grad_weight(rows.data_ptr(), g.data_ptr(), dt, B, D, H, W, cin, cout, base, usable,
                                                       grad_w.data_ptr(), _DTYPES[w.dtype], M.stream()), "gdr_conv3d_grad_weight")
            if need_b:
                b_dtype, b_shape = ctx.bias
                grad_b = (torch.zeros if not n else torch.empty)(b_shape, dtype=b_dtype, device=dev)
                if n:
                    ws, base, usable = _workspace(lib, L.GDR_CONV3D_WS_GRAD_BIAS, dt, n, cin, cout, dev)
                    L.check(lib.gdr_conv3d_grad_bias(g.data_ptr(), dt, n, cout, base, usable, grad_b.data_ptr(), _DTYPES[b_dtype],
                                                     M.stream()), "gdr_conv3d_grad_bias")
        return grad_x, grad_w, grad_b, None


def _check(x, weight, bias, add_input):
    for name, t in (("x", x), ("weight", weight)) + ((("bias", bias),) if bias is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, not {type(t).__name__}")
        if t.dtype not in _DTYPES:
            raise TypeError(f"{name} must be float32, float16 or bfloat16, not {t.dtype}")
    if x.dim() != 5:
        raise ValueError(f"x is (B, Cin, D, H, W), got {tuple(x.shape)}")
    B, cin, D, H, W = x.shape
    if weight.dim() != 5 or weight.shape[1:] != (cin, 3, 3, 3):
        raise ValueError(f"x {tuple(x.shape)} needs a weight (Cout, {cin}, 3, 3, 3), got {tuple(weight.shape)}")
    cout = weight.shape[0]
    if bias is not None and bias.shape != (cout,):
        raise ValueError(f"bias must have {cout} elements, got {tuple(bias.shape)}")
    for name, c in (("Cin", cin), ("Cout", cout)):
        if c < 8 or c > MAX_CHANNELS or c % 8:
            raise ValueError(f"{name} = {c} is outside the envelope: a multiple of 8 in 8..{MAX_CHANNELS}")
    if B * D * H * W > MAX_ROWS:
        raise ValueError("more than 2^31 - 1 voxels")
    if add_input and cin != cout:
        raise ValueError(f"add_input needs Cin == Cout, got {cin} and {cout}")
    named = [("x", x), ("weight", weight)] + ([("bias", bias)] if bias is not None else [])
    for name, t in named:
        if not t.is_cuda:
            raise RuntimeError(_NO_CPU)
    for name, t in named:
        if t.device != x.device:
            raise RuntimeError(f"{name} must live on x's device ({x.device}), not {t.device}")


def conv3d(x, weight, bias=None, add_input=False):
    """x (B, Cin, D, H, W), weight (Cout, Cin, 3, 3, 3), bias (Cout,) or None -> F.conv3d(x, weight, bias, padding=1) as a
    (B, Cout, D, H, W) tensor of x's dtype with channels_last_3d strides; add_input: x + that, rounded once."""
    add_input = bool(add_input)
    _check(x, weight, bias, add_input)
    if x.dtype == torch.float32 and torch.is_autocast_enabled("cuda"):
        x = x.to(torch.get_autocast_dtype("cuda"))
    with torch.autocast("cuda", enabled=False):
        return _Conv3d.apply(x, weight, bias, add_input)


def _triple(v):
    return (v,) * 3 if isinstance(v, int) else tuple(v)


def covers(module):
    """whether `module` is an nn.Conv3d with the one set of settings the kernels implement"""
    return (isinstance(module, torch.nn.Conv3d) and _triple(module.kernel_size) == (3, 3, 3) and _triple(module.stride) == (1, 1, 1)
            and not isinstance(module.padding, str) and _triple(module.padding) == (1, 1, 1) and _triple(module.dilation) == (1, 1, 1)
            and module.groups == 1 and module.padding_mode == "zeros")


def conv3d_of(module, x, add_input=False):
    """`module(x)` (or x + module(x)) for an nn.Conv3d(Cin, Cout, 3, padding=1) through the HIP kernels; any other kernel size,
    stride, padding, dilation, groups or padding mode raises NotImplementedError."""
    if not covers(module):
        raise NotImplementedError("the HIP convolution covers nn.Conv3d with kernel_size 3, stride 1, padding 1, dilation 1, groups 1 "
                                  f"and padding_mode 'zeros' only, got {module!r}")
    return conv3d(x, module.weight, module.bias, add_input)
