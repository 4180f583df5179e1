"""Fused row normalisations of the point decoder on the MI355X (csrc/norm.hip, include/gdr.h gdr_norm_*): the torch glue that
sits between the decoder's kernels, as one launch each.

`ada_layer_norm(feat, scale, offset)` is the reference's `AdaLayerNorm` (lightning/point_decoder/layers/normalization.py)
behind its `affine`: `gather_csr(scale, [0, offset]) * layer_norm(feat)`, rows at or behind `offset[-1]` zero.  `AdaLayerNorm`
mirrors the class, and `ada_layer_norm_forward` is a forward to bind onto the reference's own class, which has to stay
because `PointSequential` dispatches on it: `normalization.AdaLayerNorm.forward = ada_layer_norm_forward`.

`pe_concat_layer_norm(x, feat, frequencies, upscale_factor)` is the input of `UpscaleModule.delta_f`:
`layer_norm(cat([positional_encoding(frequencies, x), feat.repeat_interleave(S, 0)], -1))` without affine.

Both compute in fp32 from f32 / f16 / bf16 inputs (each input's dtype is independent), have a backward that recomputes the
row statistics, use no atomics (two calls are bitwise equal) and never synchronise with the host: `offset` and `frequencies`
are read on the device only.  The result has the dtype the torch composition returns: float32 under autocast (layer_norm is
on autocast's float32 list), the promotion of the input dtypes otherwise; gradients come back in the dtypes of the inputs.
GPU tensors only (no CPU fallback).  Envelope: C a multiple of 8 in 8..1024, 1 <= B <= 1024, 1 <= F <= 16, 1 <= S <= 16, N and
P * S below 2^31; N = 0 / P = 0 return empty tensors without a launch.  The result of `pe_concat_layer_norm` has unit channel
stride and a row stride rounded up to a multiple of 8.
"""
from __future__ import annotations

import torch
from torch import nn

from . import _lib as L
from . import _marshal as M

__all__ = ["ada_layer_norm", "AdaLayerNorm", "ada_layer_norm_forward", "pe_concat_layer_norm", "MAX_CHANNELS", "MAX_SEGMENTS",
           "MAX_FREQS", "MAX_UPSCALE"]

MAX_CHANNELS, MAX_SEGMENTS = L.GDR_NORM_MAX_CHANNELS, L.GDR_NORM_MAX_SEGMENTS
MAX_FREQS, MAX_UPSCALE = L.GDR_NORM_MAX_FREQS, L.GDR_NORM_MAX_UPSCALE
MAX_ROWS = (1 << 31) - 1

_DTYPES = M.DTYPES
_NO_CPU = "the HIP row normalisations run on ROCm/HIP tensors only (no CPU fallback)"


# ---- argument checks ------------------------------------------------------------------------------------------------------

def _check_channels(C):
    if C < 8 or C > MAX_CHANNELS or C % 8:
        raise ValueError(f"{C} channels are outside the envelope: a multiple of 8 in 8..{MAX_CHANNELS}")


def _result_dtype(*dtypes):
    """What the torch composition returns: float32 under autocast (layer_norm runs in float32 there and the product with it
    promotes), the promotion of the inputs otherwise."""
    if torch.is_autocast_enabled("cuda"):
        return torch.float32
    res = dtypes[0]
    for d in dtypes[1:]:
        res = torch.promote_types(res, d)
    return res


# ---- A: AdaLayerNorm ------------------------------------------------------------------------------------------------------

class _AdaLayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, scale, offset, eps, out_dtype):
        N, C = feat.shape
        B, dev = scale.shape[0], feat.device
        feat, scale = M.rows2d(feat), M.rows2d(scale)
        with torch.cuda.device(dev):
            out = torch.empty(N, C, dtype=out_dtype, device=dev)
            if N:
                L.check(L.load().gdr_norm_ada_forward(feat.data_ptr(), M.stride0(feat), _DTYPES[feat.dtype], scale.data_ptr(),
                                                      M.stride0(scale), _DTYPES[scale.dtype], offset.data_ptr(), N, B, C, eps,
                                                      out.data_ptr(), _DTYPES[out_dtype], M.stream()), "gdr_norm_ada_forward")
        ctx.save_for_backward(feat, scale, offset)
        ctx.eps = eps
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        feat, scale, offset = ctx.saved_tensors
        N, C = feat.shape
        B, dev = scale.shape[0], feat.device
        grad_out = M.rows2d(grad_out)
        lib = L.load()
        with torch.cuda.device(dev):
            grad_feat = torch.empty(N, C, dtype=feat.dtype, device=dev)
            grad_scale = torch.empty(B, C, dtype=scale.dtype, device=dev)
            nbytes = lib.gdr_norm_ada_backward_bytes(N, B, C)
            if nbytes == 0:
                L.check(-1, "gdr_norm_ada_backward_bytes")
            ws, base, usable = M.workspace(nbytes, dev)
            L.check(lib.gdr_norm_ada_backward(M.ptr_or_none_if_empty(grad_out), M.stride0(grad_out), _DTYPES[grad_out.dtype],
                                              M.ptr_or_none_if_empty(feat), M.stride0(feat), _DTYPES[feat.dtype], scale.data_ptr(),
                                              M.stride0(scale), _DTYPES[scale.dtype], offset.data_ptr(), N, B, C, ctx.eps, base,
                                              usable, M.ptr_or_none_if_empty(grad_feat), grad_scale.data_ptr(), M.stream()),
                    "gdr_norm_ada_backward")
        return grad_feat, grad_scale, None, None, None


def ada_layer_norm(feat, scale, offset, eps=1e-5):
    """feat (N, C), scale (B, C), offset (B,) integer segment ends on the device -> (N, C):
    out[i] = scale[b] * layer_norm(feat[i]) for offset[b - 1] <= i < offset[b]; rows at or behind offset[-1] are zero."""
    M.check_float("feat", feat, 2)
    M.check_float("scale", scale, 2)
    if not isinstance(offset, torch.Tensor):
        raise TypeError(f"offset must be a tensor, not {type(offset).__name__}")
    if offset.dtype.is_floating_point or offset.dtype.is_complex or offset.dtype == torch.bool:
        raise TypeError(f"offset must be an integer tensor, not {offset.dtype}")
    N, C = feat.shape
    B = scale.shape[0]
    if offset.dim() != 1 or offset.shape[0] != B or scale.shape[1] != C:
        raise ValueError(f"feat {tuple(feat.shape)} needs scale (B, {C}) and offset (B,), got {tuple(scale.shape)} and "
                         f"{tuple(offset.shape)}")
    if not 1 <= B <= MAX_SEGMENTS:
        raise ValueError(f"{B} segments are outside the envelope 1..{MAX_SEGMENTS}")
    _check_channels(C)
    if N > MAX_ROWS:
        raise ValueError("more than 2^31 - 1 rows")
    M.check_devices((("feat", feat), ("scale", scale), ("offset", offset)), _NO_CPU)
    return _AdaLayerNorm.apply(feat, scale, offset.long().contiguous(), float(eps), _result_dtype(feat.dtype, scale.dtype))


def ada_layer_norm_forward(self, feat, global_feat, offset):
    """The forward of an AdaLayerNorm: reads only `self.affine` and `self.eps`.  Bind it onto the reference's class with
    `normalization.AdaLayerNorm.forward = ada_layer_norm_forward`."""
    return ada_layer_norm(feat, self.affine(global_feat), offset, self.eps)


class AdaLayerNorm(nn.Module):
    """Mirror of the reference's AdaLayerNorm: the one child `affine`, no other parameters."""

    def __init__(self, normalized_shape, w_shape, eps=1e-5):
        super().__init__()
        self.normalized_shape = normalized_shape
        self.eps = eps
        self.affine = nn.Linear(w_shape, normalized_shape)

    forward = ada_layer_norm_forward

    def extra_repr(self):
        return f"{self.normalized_shape}, eps={self.eps}"


# ---- B: the input of UpscaleModule.delta_f --------------------------------------------------------------------------------

class _PeConcatLayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, feat, frequencies, S, eps, out_dtype):
        P, C = feat.shape
        F, dev = frequencies.shape[0], feat.device
        W = 6 * F + C
        x, feat, frequencies = x.contiguous(), M.rows2d(feat), frequencies.contiguous()
        with torch.cuda.device(dev):
            buf = torch.empty(P * S, (W + 7) // 8 * 8, dtype=out_dtype, device=dev)
            if P:
                L.check(L.load().gdr_norm_pe_forward(x.data_ptr(), _DTYPES[x.dtype], feat.data_ptr(), M.stride0(feat),
                                                     _DTYPES[feat.dtype], frequencies.data_ptr(), _DTYPES[frequencies.dtype], P, S,
                                                     C, F, eps, buf.data_ptr(), buf.shape[1], _DTYPES[out_dtype], M.stream()),
                        "gdr_norm_pe_forward")
        ctx.save_for_backward(x, feat, frequencies)
        ctx.S, ctx.eps = S, eps
        return buf[:, :W]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, feat, frequencies = ctx.saved_tensors
        P, C = feat.shape
        F, dev = frequencies.shape[0], feat.device
        need_x, need_feat = ctx.needs_input_grad[:2]
        if grad_out.shape[0] and (grad_out.stride(1) != 1 or grad_out.stride(0) % 2 or grad_out.stride(0) < grad_out.shape[1]
                                  or grad_out.data_ptr() % (2 * grad_out.element_size())):
            grad_out = grad_out.contiguous()       # (a dense row of 6F + C elements is even)
        with torch.cuda.device(dev):
            grad_x = torch.empty(P * ctx.S, 3, dtype=x.dtype, device=dev) if need_x else None
            grad_feat = torch.empty(P, C, dtype=feat.dtype, device=dev) if need_feat else None
            if P and (need_x or need_feat):
                L.check(L.load().gdr_norm_pe_backward(grad_out.data_ptr(), grad_out.stride(0), _DTYPES[grad_out.dtype],
                                                      x.data_ptr(), _DTYPES[x.dtype], feat.data_ptr(), M.stride0(feat),
                                                      _DTYPES[feat.dtype], frequencies.data_ptr(), _DTYPES[frequencies.dtype], P,
                                                      ctx.S, C, F, ctx.eps, M.ptr(grad_x), M.ptr(grad_feat), M.stream()),
                        "gdr_norm_pe_backward")
        return grad_x, grad_feat, None, None, None, None


def pe_concat_layer_norm(x, feat, frequencies, upscale_factor, eps=1e-5):
    """x (P * S, 3), feat (P, C), frequencies (F,) on the device, S = upscale_factor -> (P * S, 6 F + C): layer_norm without
    affine of [sin(f_k x[r, j]) at 3k + j, cos(...) at 3F + 3k + j, feat[r // S]]."""
    M.check_float("x", x, 2)
    M.check_float("feat", feat, 2)
    M.check_float("frequencies", frequencies, 1)
    S = int(upscale_factor)
    F = frequencies.shape[0]
    if F == 0:
        raise NotImplementedError("frequencies is empty: the raw-coordinate variant (n_frequencies = 0) is not implemented")
    if not 1 <= F <= MAX_FREQS:
        raise ValueError(f"{F} frequencies are outside the envelope 1..{MAX_FREQS}")
    if not 1 <= S <= MAX_UPSCALE:
        raise ValueError(f"upscale_factor {S} is outside the envelope 1..{MAX_UPSCALE}")
    P, C = feat.shape
    _check_channels(C)
    if x.shape != (P * S, 3):
        raise ValueError(f"x must be ({P} * {S}, 3) for feat {tuple(feat.shape)}, got {tuple(x.shape)}")
    if P * S > MAX_ROWS:
        raise ValueError("more than 2^31 - 1 rows")
    M.check_devices((("feat", feat), ("x", x), ("frequencies", frequencies)), _NO_CPU)
    out_dtype = _result_dtype(frequencies.dtype, x.dtype, feat.dtype)
    return _PeConcatLayerNorm.apply(x, feat, frequencies, S, float(eps), out_dtype)
