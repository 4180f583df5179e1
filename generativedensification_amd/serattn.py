"""The patch attention of the point decoder's SerializedAttention with its two gathers, both casts and the scatter-accumulate
of its backward inside the attention kernels, on the MI355X (csrc/attn.hip, include/gdr.h gdr_attn_gather_*; reference
lightning/point_decoder/autoencoder.py, SerializedAttention.forward).  `self.qkv`, `self.proj` and `self.proj_drop` stay torch's.

`serialized_attention(qkv, order, inverse, cu_seqlens, num_heads, patch_size, softmax_scale=None) -> (N, C)` in qkv's dtype is
the reference's flash branch,

    attn(qkv[order].half().reshape(-1, 3, H, D), cu_seqlens).reshape(-1, C).to(qkv.dtype)[inverse],      C = H D,

and its autograd, in one launch each way.  qkv (N, 3 C) f32, bf16 or f16; order (Tp,) int64 = serialized_order[i][pad], the
point each padded slot holds; inverse (N,) int64 = unpad[serialized_inverse[i]], the slot that is each point's own; cu_seqlens
int32 over the Tp slots.  Every element is rounded to fp16 as `.half()` rounds it, the arithmetic is the fp16 path of
`attention.attn_varlen_qkvpacked` (the forward is bitwise what the line above gives over that function), the result is rounded
to fp16 and then to qkv's dtype.  No (Tp, .) tensor exists but the (H, Tp) f32 log-sum-exp the backward reads (with f32 / bf16
qkv it also keeps the (N, C) f32 result before its roundings, for delta); under no_grad not even that.  The gradient of a point
that the padding holds twice is the f32 sum of its two contributions, rounded once (to fp16, then to qkv's dtype; the reference
accumulates in qkv's dtype); each row of dqkv is stored exactly once, without atomics: two calls are bitwise equal.

Precondition (values, not memory safety): `order[inverse[i]] == i` for every i, and a slot that is not its point's own sits one
sequence behind the own slot at the same position — the layout of the reference's padding, of `serialization.patch_tables`
and of tests/attn_ref.py padded_patches.  Any other tables are read safely (entries out of range are skipped on the device,
cu_seqlens is clamped) and give unspecified values.  No table is read on the host; nothing here synchronises with it.

Envelope (anything else raises before a launch): GPU tensors only (RuntimeError, "no CPU fallback"); qkv f32 / f16 / bf16,
order and inverse int64, cu_seqlens int32 (TypeError); D = C / H in {8, 16, 32, 64}, 1 <= patch_size <= 256, N and Tp below
2^31, Tp >= N (ValueError).  Rows are read in place when dense from a 16-byte aligned base, and made so with one copy
otherwise.  Autocast is switched off inside.  N = 0 returns an empty tensor without loading the library.

`serialized_attention_forward` is a forward to bind onto the reference's class
(`autoencoder.SerializedAttention.forward = serattn.serialized_attention_forward`): under SERATTN_BACKEND = "hip", wherever
`covers` and `in_envelope` hold, qkv Linear, serialized_attention, proj, proj_drop; anywhere else the reference's lines over this
repository's `flash_attn` drop-in.  Either way the three tables come from the point (`pad`, `unpad`, `cu_seqlens_key`) and are
built by `serialization.patch_tables` and cached there when absent.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from . import _marshal as M

__all__ = ["serialized_attention", "serialized_attention_forward", "covers", "in_envelope", "SERATTN_BACKEND"]

# the path of the bound forward: "hip" (the fused call wherever it covers the module and the shape) or "torch" (the
# reference's lines over the flash_attn drop-in).  "hip" is the default by the project's rule: forward + backward its median
# was lower and the ranges did not overlap at both base-config shapes (scripts/bench_serattn.py, BASELINE §4-serattn: under
# bf16 autocast 354 us against 503 us at 12 000 x 160, 459 us against 706 us at 19 200 x 256).
SERATTN_BACKEND = "hip"

MAX_SEQLEN = L.GDR_ATTN_MAX_SEQLEN
HEAD_DIMS = L.GDR_ATTN_HEAD_DIMS
MAX_ROWS = (1 << 31) - 1
_DTYPES = M.DTYPES


def in_envelope(N, C, H, patch, Tp=None):
    """whether the kernels serve N points of C channels in H heads, patches of `patch`, Tp padded slots (default: N)"""
    Tp = N if Tp is None else Tp
    return (H >= 1 and C >= 1 and C % H == 0 and C // H in HEAD_DIMS and 1 <= patch <= MAX_SEQLEN and 0 <= N <= MAX_ROWS
            and N <= Tp <= MAX_ROWS)


class _SerAttn(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")     # autocast off inside; qkv keeps the dtype it came in
    def forward(ctx, qkv, order, inverse, cu_seqlens, args, keep):
        lib = L.load()
        dev, Cc = qkv.device, args.H * args.D
        qkv = M.dense_aligned(qkv)
        with torch.cuda.device(dev):
            out = torch.empty(args.N, Cc, dtype=qkv.dtype, device=dev)
            # what the backward reads: the per-slot log-sum-exp, and for its delta the result: the f16 one itself (bitwise the
            # backward of the gathered call), else the f32 result before its two roundings
            lse = torch.empty(args.H, args.Tp, dtype=torch.float32, device=dev) if keep else None
            full = torch.empty(args.N, Cc, dtype=torch.float32, device=dev) if keep and qkv.dtype != torch.float16 else None
            L.check(lib.gdr_attn_gather_forward(C.byref(args), qkv.data_ptr(), order.data_ptr(), inverse.data_ptr(),
                                                cu_seqlens.data_ptr(), out.data_ptr(), M.ptr(full), M.ptr(lse), M.stream()),
                    "gdr_attn_gather_forward")
        if keep:
            ctx.save_for_backward(qkv, order, inverse, cu_seqlens, out if full is None else full, lse)
            ctx.args = args
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, dout):
        lib = L.load()
        qkv, order, inverse, cu_seqlens, out, lse = ctx.saved_tensors
        args, dev = ctx.args, qkv.device
        dout = M.dense_aligned(dout.to(qkv.dtype))
        with torch.cuda.device(dev):
            dqkv = torch.empty_like(qkv)
            L.check(lib.gdr_attn_gather_backward(C.byref(args), dout.data_ptr(), qkv.data_ptr(), order.data_ptr(),
                                                 inverse.data_ptr(), cu_seqlens.data_ptr(), out.data_ptr(), _DTYPES[out.dtype],
                                                 lse.data_ptr(), dqkv.data_ptr(), M.stream()), "gdr_attn_gather_backward")
        return dqkv, None, None, None, None, None


def _check_table(name, t, dtype, numel=None):
    if not isinstance(t, torch.Tensor) or t.dim() != 1 or (numel is not None and t.numel() != numel):
        want = "" if numel is None else f" of {numel} entries"
        raise ValueError(f"{name} must be a 1-D tensor{want}, got {tuple(getattr(t, 'shape', ()))}")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, not {t.dtype}")


def serialized_attention(qkv, order, inverse, cu_seqlens, num_heads, patch_size, softmax_scale=None):
    """qkv (N, 3 C), order (Tp,) int64, inverse (N,) int64, cu_seqlens int32 -> (N, C) in qkv's dtype: the reference's gather,
    `.half()`, patch attention, cast back and gather by `inverse` (module docstring)."""
    if not isinstance(qkv, torch.Tensor) or qkv.dim() != 2 or qkv.shape[1] % 3:
        raise ValueError(f"qkv must be (N, 3 C), got {tuple(getattr(qkv, 'shape', ()))}")
    N, Cc = qkv.shape[0], qkv.shape[1] // 3
    H, patch = int(num_heads), int(patch_size)
    _check_table("order", order, torch.int64)
    _check_table("inverse", inverse, torch.int64, N)
    _check_table("cu_seqlens", cu_seqlens, torch.int32)
    if qkv.dtype not in _DTYPES:
        raise TypeError(f"qkv must be float32, float16 or bfloat16, not {qkv.dtype}")
    if isinstance(softmax_scale, torch.Tensor):
        raise TypeError("softmax_scale must be a Python number (a tensor would have to be read back)")
    Tp = order.numel()
    if cu_seqlens.numel() < 1:
        raise ValueError("cu_seqlens must hold batch + 1 boundaries")
    if not in_envelope(N, Cc, H, patch, Tp):
        raise ValueError(f"N {N}, C {Cc}, H {H}, patch {patch}, Tp {Tp} are outside the envelope: C / H in {HEAD_DIMS}, "
                         f"1 <= patch <= {MAX_SEQLEN}, N <= Tp < 2^31")
    if not qkv.is_cuda:
        raise RuntimeError("the HIP serialized attention runs on ROCm/HIP tensors only (no CPU fallback)")
    if any(t.device != qkv.device for t in (order, inverse, cu_seqlens)):
        raise RuntimeError("order, inverse and cu_seqlens must live on qkv's device")
    if N == 0:
        return qkv.new_empty((0, Cc))
    a = L.GdrAttnGatherArgs()
    a.N, a.Tp, a.batch, a.H, a.D = N, Tp, cu_seqlens.numel() - 1, H, Cc // H
    a.max_seqlen, a.dtype = patch, _DTYPES[qkv.dtype]
    a.scale = float((Cc // H) ** -0.5 if softmax_scale is None else softmax_scale)
    keep = torch.is_grad_enabled() and qkv.requires_grad
    return _SerAttn.apply(qkv, order.contiguous(), inverse.contiguous(), cu_seqlens.contiguous(), a, keep)


# ---- the module forward ---------------------------------------------------------------------------------------------------

def covers(module):
    """whether `module` takes the branch that is fused: flash attention without relative position encoding, and no attention
    dropout to draw (attn_drop is 0, or the module is not training)"""
    if not getattr(module, "enable_flash", False) or getattr(module, "enable_rpe", False):
        return False
    drop = getattr(module, "attn_drop", None)
    return isinstance(drop, (int, float)) and (drop == 0 or not module.training)


def _tables(point, patch):
    """pad, unpad and cu_seqlens under the reference's keys, built in one launch and cached in the point when absent"""
    keys = ("pad", "unpad", "cu_seqlens_key")
    if any(k not in point.keys() for k in keys):
        from . import serialization

        for k, t in zip(keys, serialization.patch_tables(point.offset, patch)):
            point[k] = t
    return tuple(point[k] for k in keys)


def _bincount(offset):
    return torch.diff(offset, prepend=offset.new_zeros(1))


def _reference_attention(self, point, qkv, order, cu_seqlens):
    """the reference's lines between the two gathers: qkv (Tp, 3 C) in slot order -> feat (Tp, C)"""
    H, K, Cc = self.num_heads, self.patch_size, self.channels
    if self.enable_flash:
        import flash_attn

        feat = flash_attn.flash_attn_varlen_qkvpacked_func(
            qkv.half().reshape(-1, 3, H, Cc // H), cu_seqlens, max_seqlen=K, dropout_p=self.attn_drop if self.training else 0,
            softmax_scale=self.scale).reshape(-1, Cc)
        return feat.to(qkv.dtype)
    q, k, v = qkv.reshape(-1, K, 3, H, Cc // H).permute(2, 0, 3, 1, 4).unbind(dim=0)       # (N', H, K, D) each
    if self.upcast_attention:
        q, k = q.float(), k.float()
    attn = (q * self.scale) @ k.transpose(-2, -1)
    if self.enable_rpe:
        key = f"rel_pos_{self.order_index}"
        if key not in point.keys():
            with torch.no_grad():
                grid = point.grid_coord[order].reshape(-1, K, 3)
                point[key] = grid.unsqueeze(2) - grid.unsqueeze(1)
        attn = attn + self.rpe(point[key])
    if self.upcast_softmax:
        attn = attn.float()
    attn = self.attn_drop(self.softmax(attn)).to(qkv.dtype)
    return (attn @ v).transpose(1, 2).reshape(-1, Cc)


def _serves(self, qkv, order):
    if not qkv.is_cuda or qkv.dim() != 2 or qkv.dtype not in _DTYPES or isinstance(self.scale, torch.Tensor):
        return False
    return qkv.shape[1] == 3 * self.channels and in_envelope(qkv.shape[0], self.channels, self.num_heads, self.patch_size,
                                                             order.numel())


def serialized_attention_forward(self, point):
    """SerializedAttention.forward of the reference.  Reads self.qkv, proj, proj_drop, num_heads, channels, patch_size, scale,
    order_index, enable_flash, enable_rpe, attn_drop (and what the non-flash branch reads); reads point.feat, offset,
    serialized_order, serialized_inverse and the three tables; assigns point.feat."""
    if SERATTN_BACKEND not in ("torch", "hip"):
        raise ValueError(f"serattn.SERATTN_BACKEND must be 'torch' or 'hip', not {SERATTN_BACKEND!r}")
    if not self.enable_flash:
        self.patch_size = min(_bincount(point.offset).min().tolist(), self.patch_size_max)
    pad, unpad, cu_seqlens = _tables(point, self.patch_size)
    order = point.serialized_order[self.order_index][pad]
    inverse = unpad[point.serialized_inverse[self.order_index]]
    qkv = self.qkv(point.feat)
    if SERATTN_BACKEND == "hip" and covers(self) and _serves(self, qkv, order):
        feat = serialized_attention(qkv, order, inverse, cu_seqlens, self.num_heads, self.patch_size, self.scale)
    else:
        feat = _reference_attention(self, point, qkv[order], order, cu_seqlens)[inverse]
    feat = self.proj(feat)
    feat = self.proj_drop(feat)
    point.feat = feat
    return point
