"""Tiled MFMA attention for fixed-length batches of long sequences on the MI355X (csrc/attn_tiled.hip, include/gdr.h
gdr_attn_tiled_*), and a mirror of timm's `Attention.forward` that runs it: what the reference's image encoder
(lightning/network.py DinoWrapper, a timm ViT-B/16 or ViT-S/16 on 512 x 512 images: 1025 tokens, head dimension 64) runs in
each of its layers, forward and backward.  The semantics are restated in the header of csrc/attn_tiled.hip.

Envelope (anything else raises before a kernel is launched): fp16 or bf16 on a ROCm device, head dimension 64,
1 <= L <= 16384, B * H * L < 2^31, no mask, no dropout.  The kernels read q, k and v through their batch / token / head
strides, so the three slices of timm's (B, L, 3, H, D) projection are read in place and the packed gradient is written in
place.  The one requirement on memory is on rows: unit channel stride and 16-byte alignment (a 16-byte aligned base, every
other stride a multiple of 8 elements).  A tensor that does not meet it is COPIED to a dense one first (q, k, v, and the
upstream gradient alike); results do not depend on which path was taken.  Nothing here synchronises with the host.

Binding:  timm.models.vision_transformer.Attention.forward = vitattn.vit_attention_forward
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn.functional as F

from . import _lib as L
from . import _marshal as M

__all__ = ["attn_tiled_qkvpacked", "attn_tiled", "vit_attention_forward", "covers", "VITATTN_BACKEND", "MAX_SEQLEN",
           "HEAD_DIM"]

MAX_SEQLEN = L.GDR_ATTN_TILED_MAX_SEQLEN
HEAD_DIM = L.GDR_ATTN_TILED_HEAD_DIM
_DTYPES = {d: M.DTYPES[d] for d in (torch.float16, torch.bfloat16)}

# "hip": vit_attention_forward takes the fused path wherever covers() holds; "torch": it always runs timm's own lines.
# The shipped value follows from scripts/bench_vitattn.py: "hip" only if the bound module's
# forward + backward at dim 768 under bf16 autocast is faster than torch's with the ranges of the repeated runs apart.
VITATTN_BACKEND = "hip"      # 964 against 1065 us there, the ranges apart


def _strides(t):
    """(batch, token, head, channel) element strides; a dimension of one element has no stride to speak of: 0"""
    return (C.c_int64 * 4)(*(s if n > 1 else 0 for s, n in zip(t.stride(), t.shape[:3])), t.stride(3))


def _rows(t):
    """`t` (B, L, H, D) as the kernels read rows: itself where its rows are unit-stride and 16-byte aligned, one dense copy
    otherwise"""
    if t.stride(3) != 1 or t.data_ptr() % 16 or any(s % 8 for s, n in zip(t.stride()[:3], t.shape[:3]) if n > 1):
        t = t.contiguous()
        if t.data_ptr() % 16:
            t = t.clone()
    return t


class _TiledFunction(torch.autograd.Function):
    """(qkv (B, L, 3, H, D), None, None) or (q, k, v) of (B, L, H, D) each -> out (B, L, H, D)"""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")     # autocast off inside; the caller's half dtype is kept
    def forward(ctx, a, k, v, args):
        lib = L.load()
        packed = k is None
        q, k, v = (_rows(t) for t in (a.unbind(2) if packed else (a, k, v)))
        dev = q.device
        with torch.cuda.device(dev):
            out = torch.empty(args.B, args.L, args.H, args.D, dtype=q.dtype, device=dev)
            lse = torch.empty(args.B, args.H, args.L, dtype=torch.float32, device=dev)
            # what out's rounding drops, for the backward's delta: kept only if a backward can follow
            out_lo = torch.empty_like(out) if any(ctx.needs_input_grad[:3]) else None
            L.check(lib.gdr_attn_tiled_forward(C.byref(args), q.data_ptr(), _strides(q), k.data_ptr(), _strides(k),
                                               v.data_ptr(), _strides(v), out.data_ptr(), M.ptr(out_lo), lse.data_ptr(),
                                               M.stream()), "gdr_attn_tiled_forward")
        ctx.save_for_backward(q, k, v, out, lse, out_lo)
        ctx.args, ctx.packed = args, packed
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, dout):
        lib = L.load()
        q, k, v, out, lse, out_lo = ctx.saved_tensors
        args, dev = ctx.args, q.device
        dout = _rows(dout.to(q.dtype))
        with torch.cuda.device(dev):
            if ctx.packed:      # one packed gradient, written in place through its three slices
                dqkv = torch.empty(args.B, args.L, 3, args.H, args.D, dtype=q.dtype, device=dev)
                dq, dk, dv = dqkv.unbind(2)
            else:
                dq, dk, dv = (torch.empty(args.B, args.L, args.H, args.D, dtype=q.dtype, device=dev) for _ in range(3))
            scratch = torch.empty(args.B * args.H * args.L, dtype=torch.float32, device=dev)
            L.check(lib.gdr_attn_tiled_backward(C.byref(args), dout.data_ptr(), _strides(dout), q.data_ptr(), _strides(q),
                                                k.data_ptr(), _strides(k), v.data_ptr(), _strides(v), out.data_ptr(),
                                                M.ptr(out_lo), lse.data_ptr(), dq.data_ptr(), _strides(dq), dk.data_ptr(), _strides(dk),
                                                dv.data_ptr(), _strides(dv), scratch.data_ptr(), M.stream()),
                    "gdr_attn_tiled_backward")
        return (dqkv, None, None, None) if ctx.packed else (dq, dk, dv, None)


def _args(name, t, softmax_scale) -> L.GdrAttnTiledArgs:
    """the arguments of one (B, L, H, D) operand `t`, or the refusal that names it"""
    if t.dtype not in _DTYPES:
        raise RuntimeError(f"the tiled HIP attention takes fp16 or bf16 only, {name} is {t.dtype}")
    B, Lq, H, D = t.shape
    if D != HEAD_DIM:
        raise ValueError(f"{name}: head dimension {D} is outside the tiled HIP attention's envelope ({HEAD_DIM})")
    if not 1 <= Lq <= MAX_SEQLEN:
        raise ValueError(f"{name}: sequence length {Lq} is outside the tiled HIP attention's envelope 1..{MAX_SEQLEN}")
    if B < 1 or H < 1:
        raise ValueError(f"{name}: batch and nheads must be at least 1, got {tuple(t.shape)}")
    if B * H * Lq >= 1 << 31:
        raise ValueError(f"{name}: batch * nheads * seqlen = {B * H * Lq} must be below 2^31")
    scale = float(D ** -0.5 if softmax_scale is None else softmax_scale)
    if scale != scale or scale in (float("inf"), float("-inf")):
        raise ValueError("softmax_scale must be finite")
    if not t.is_cuda:
        raise RuntimeError("the tiled HIP attention runs on ROCm/HIP tensors only (no CPU fallback)")
    a = L.GdrAttnTiledArgs()
    a.B, a.L, a.H, a.D, a.dtype, a.scale = B, Lq, H, D, _DTYPES[t.dtype], scale
    return a


def attn_tiled_qkvpacked(qkv, softmax_scale=None):
    """softmax(scale Q K^T) V per image and head: qkv (B, L, 3, H, 64) -> (B, L, H, 64).  The gradient is one packed
    (B, L, 3, H, 64) tensor.  qkv is read in place if its rows are unit-stride and 16-byte aligned, copied otherwise."""
    if not isinstance(qkv, torch.Tensor) or qkv.dim() != 5 or qkv.shape[2] != 3:
        raise ValueError(f"qkv must be (batch, seqlen, 3, nheads, headdim), got {tuple(getattr(qkv, 'shape', ()))}")
    return _TiledFunction.apply(qkv, None, None, _args("qkv", qkv[:, :, 0], softmax_scale))


def attn_tiled(q, k, v, softmax_scale=None):
    """The same for three (B, L, H, 64) tensors with any batch / token / head strides; three gradients."""
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise ValueError(f"{name} must be (batch, seqlen, nheads, headdim), got {tuple(getattr(t, 'shape', ()))}")
    for name, t in (("k", k), ("v", v)):
        if t.shape != q.shape:
            raise ValueError(f"{name} must have q's shape {tuple(q.shape)}, got {tuple(t.shape)}")
        if t.dtype != q.dtype:
            raise RuntimeError(f"{name} must have q's dtype {q.dtype}, not {t.dtype}")
    a = _args("q", q, softmax_scale)
    M.check_devices([("q", q), ("k", k), ("v", v)], "the tiled HIP attention runs on ROCm/HIP tensors only (no CPU fallback)")
    return _TiledFunction.apply(q, k, v, a)


def _projected_dtype(x):
    """the dtype `self.qkv(x)` comes out in"""
    if x.is_cuda and torch.is_autocast_enabled():
        return torch.get_autocast_dtype("cuda")
    return x.dtype


def covers(self, x, attn_mask=None) -> bool:
    """Whether vit_attention_forward(self, x, attn_mask) takes the fused path: a GPU tensor whose projection comes out in fp16
    or bf16 (under autocast, or a half model), head_dim 64, Identity q_norm / k_norm, no mask, no active dropout, a sequence
    inside the envelope, and VITATTN_BACKEND == "hip"."""
    if VITATTN_BACKEND != "hip" or attn_mask is not None or not x.is_cuda or x.dim() != 3:
        return False
    if self.head_dim != HEAD_DIM or not 1 <= x.shape[1] <= MAX_SEQLEN or x.shape[0] < 1:
        return False
    if not isinstance(self.q_norm, torch.nn.Identity) or not isinstance(self.k_norm, torch.nn.Identity):
        return False
    if self.attn_drop.p != 0 and self.training:
        return False
    return _projected_dtype(x) in _DTYPES


def vit_attention_forward(self, x, attn_mask=None):
    """timm's Attention.forward over its public attributes (num_heads, head_dim, scale, qkv, q_norm, k_norm, attn_drop, proj,
    proj_drop).  Where covers() holds, the projection is viewed as (B, N, 3, H, D) and goes to the kernels as it is, and their
    (B, N, H, D) result is viewed as (B, N, C): no permute, no copy.  Otherwise these are timm's own lines."""
    B, N, C_ = x.shape
    if covers(self, x, attn_mask):
        qkv = self.qkv(x).view(B, N, 3, self.num_heads, self.head_dim)
        x = attn_tiled_qkvpacked(qkv, self.scale).view(B, N, C_)
    else:
        qkv = self.qkv(x).reshape(B, N, 3, self.num_heads, self.head_dim).permute(2, 0, 3, 1, 4)
        q, k, v = qkv.unbind(0)
        q, k = self.q_norm(q), self.k_norm(k)
        x = F.scaled_dot_product_attention(q, k, v, attn_mask=attn_mask, scale=self.scale,
                                           dropout_p=self.attn_drop.p if self.training else 0.0)
        x = x.transpose(1, 2).reshape(B, N, C_)
    x = self.proj(x)
    return self.proj_drop(x)
