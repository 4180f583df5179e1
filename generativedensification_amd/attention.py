"""Variable-length packed-QKV attention for short sequences on the MI355X (csrc/attn.hip, include/gdr.h gdr_attn_*): what
the reference's point decoder calls through `flash_attn.flash_attn_varlen_qkvpacked_func` in every SerializedAttention
block (lightning/point_decoder/autoencoder.py, patches of 48 tokens, head dimension 8).  The `flash_attn` package of this
repository re-exports these functions.  The semantics are restated in the header of csrc/attn.hip.

Envelope (anything else raises before a kernel is launched): fp16 or bf16 on a ROCm device, head dimension 8, 16, 32 or 64,
max_seqlen <= 256, no dropout / causal mask / window / softcap / alibi.  Rows at or beyond cu_seqlens[-1] are zero in the
output and in the gradient (upstream leaves them undefined).  Nothing here synchronises with the host: `batch` is
cu_seqlens.numel() - 1, `max_seqlen` the caller's int, and cu_seqlens is only ever read on the device — a sequence longer
than max_seqlen is cut there, its further rows are not written.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from . import _marshal as M

__all__ = ["attn_varlen_qkvpacked", "attn_qkvpacked", "MAX_SEQLEN", "HEAD_DIMS"]

MAX_SEQLEN = L.GDR_ATTN_MAX_SEQLEN
HEAD_DIMS = L.GDR_ATTN_HEAD_DIMS
_DTYPES = {d: M.DTYPES[d] for d in (torch.float16, torch.bfloat16)}     # the dense kernels take no float32


class _AttnFunction(torch.autograd.Function):
    """qkv (total, 3, H, D) fp16 / bf16 on the GPU (any strides) -> out (total, H, D); cu_seqlens int32 (batch + 1) or
    None with `args.fixed_len`."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")     # autocast off inside; the caller's half dtype is kept
    def forward(ctx, qkv, cu_seqlens, args):
        lib = L.load()
        dev = qkv.device
        with torch.cuda.device(dev):
            out = torch.empty(args.total, args.H, args.D, dtype=qkv.dtype, device=dev)
            lse = torch.empty(args.H, args.total, dtype=torch.float32, device=dev)
            st = M.stream()
            L.check(lib.gdr_attn_forward(C.byref(args), qkv.data_ptr(), M.strides(qkv),
                                         None if cu_seqlens is None else cu_seqlens.data_ptr(), out.data_ptr(),
                                         lse.data_ptr(), st), "gdr_attn_forward")
        ctx.save_for_backward(qkv, cu_seqlens, out, lse)
        ctx.args = args
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, dout):
        lib = L.load()
        qkv, cu_seqlens, out, lse = ctx.saved_tensors
        args, dev = ctx.args, qkv.device
        dout = dout.to(qkv.dtype)
        with torch.cuda.device(dev):
            dqkv = torch.empty(args.total, 3, args.H, args.D, dtype=qkv.dtype, device=dev)
            st = M.stream()
            L.check(lib.gdr_attn_backward(C.byref(args), dout.data_ptr(), M.strides(dout), qkv.data_ptr(), M.strides(qkv),
                                          None if cu_seqlens is None else cu_seqlens.data_ptr(), out.data_ptr(),
                                          lse.data_ptr(), dqkv.data_ptr(), st), "gdr_attn_backward")
        return dqkv, None, None


def _args(qkv: torch.Tensor, batch: int, max_seqlen: int, fixed_len: int, softmax_scale) -> L.GdrAttnArgs:
    if qkv.dim() != 4 or qkv.shape[1] != 3:
        raise ValueError(f"qkv must be (total, 3, nheads, headdim), got {tuple(qkv.shape)}")
    if qkv.dtype not in _DTYPES:
        raise RuntimeError(f"the HIP attention takes fp16 or bf16 only, not {qkv.dtype}")
    total, _, H, D = qkv.shape
    if D not in HEAD_DIMS:
        raise ValueError(f"head dimension {D} is outside the HIP attention's envelope {HEAD_DIMS}")
    max_seqlen = int(max_seqlen)
    if not 1 <= max_seqlen <= MAX_SEQLEN:
        raise ValueError(f"max_seqlen {max_seqlen} is outside the HIP attention's envelope 1..{MAX_SEQLEN}")
    if not qkv.is_cuda:
        raise RuntimeError("the HIP attention runs on ROCm/HIP tensors only (no CPU fallback)")
    a = L.GdrAttnArgs()
    a.total, a.batch, a.H, a.D = total, batch, H, D
    a.max_seqlen, a.fixed_len, a.dtype = max_seqlen, fixed_len, _DTYPES[qkv.dtype]
    a.scale = float(D ** -0.5 if softmax_scale is None else softmax_scale)
    return a


def attn_varlen_qkvpacked(qkv, cu_seqlens, max_seqlen, softmax_scale=None):
    """softmax(scale Q K^T) V per sequence [cu_seqlens[b], cu_seqlens[b + 1]) and head: (total, 3, H, D) -> (total, H, D)."""
    if cu_seqlens.dtype != torch.int32 or cu_seqlens.dim() != 1 or cu_seqlens.numel() < 1:
        raise ValueError("cu_seqlens must be a 1-D int32 tensor of batch + 1 boundaries")
    a = _args(qkv, cu_seqlens.numel() - 1, max_seqlen, 0, softmax_scale)
    if cu_seqlens.device != qkv.device:
        raise RuntimeError("cu_seqlens must live on qkv's device")
    return _AttnFunction.apply(qkv, cu_seqlens.contiguous(), a)


def attn_qkvpacked(qkv, softmax_scale=None):
    """(B, L, 3, H, D) -> (B, L, H, D): the same kernel with the boundaries b * L implied."""
    if qkv.dim() != 5:
        raise ValueError(f"qkv must be (batch, seqlen, 3, nheads, headdim), got {tuple(qkv.shape)}")
    B, Lq = qkv.shape[:2]
    flat = qkv.reshape(B * Lq, *qkv.shape[2:])
    a = _args(flat, B, max(Lq, 1), Lq, softmax_scale)
    return _AttnFunction.apply(flat, None, a).reshape(B, Lq, *qkv.shape[3:])
