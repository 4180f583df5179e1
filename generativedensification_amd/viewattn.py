"""Per-point view cross attention of the fine decoder on the MI355X (csrc/viewattn.hip, include/gdr.h gdr_viewattn_*): the
reference's `Decoder.forward_fine` (lightning/network.py) runs `nn.MultiheadAttention(embed 80, 16 heads, kdim = vdim = 8)` with
one query per point over the V = 2..4 view features of that point.  Because the key / value width (8) is close to the head
width (5), the attention folds, with the per-head slices Wq_h (d, E), Wk_h, Wv_h (d, Ck), Wo[:, h] (E, d):

    A  = stack_h(Wk_h^T Wq_h)  (H Ck, E)      t = x A^T + a_bias                         (N, H, Ck)
                                              s[n, h, v] = scale <t[n, h], cond[n, v]>,  p = softmax_v(s)
                                              u[n, h]    = sum_v p[n, h, v] cond[n, v]   (N, H, Ck)
    Bm = cat_h(Wo[:, h] Wv_h)  (E, H Ck)      out = u Bm^T + b_bias                      (N, E)

The q bias becomes a_bias = stack_h(Wk_h^T bq_h); the k bias adds a constant over v to s and drops out of the softmax; the v
bias and the out bias become b_bias = Wo bv + bo because sum_v p = 1.  No projected key or value is materialised: the core
(s, p, u) holds no weights and is one HIP launch each way, and every weight gradient flows through the two small
differentiable products that build A and Bm.

`view_attention_pool(t, cond, scale)` is the core; `fold_attention_weights(mha)` the fold (pure torch, works on CPU modules);
`single_query_cross_attention(mha, x, cond)` equals `mha(x[:, None], cond, cond, need_weights=False)[0][:, 0]`;
`decoder_forward_fine` is a forward to bind: `network.Decoder.forward_fine = viewattn.decoder_forward_fine`.

The core computes in fp32 from f32 / f16 / bf16 inputs (each input's dtype is independent), recomputes p in the backward
(nothing but the inputs is saved), uses no atomics (two calls are bitwise equal) and never synchronises with the host.  The
result has t's dtype; gradients come back in the dtypes of the inputs.  GPU tensors only (no CPU fallback).  Envelope: Ck 4, 8
or 16, 1 <= H <= 64, 1 <= V <= 16, N <= 2^27; N = 0 returns an empty tensor without loading the library.  Non-finite inputs are
memory-safe and otherwise unspecified.  The product with A and the core always run in fp32 with autocast disabled; the
product with Bm runs under the ambient autocast like any F.linear.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _lib as L
from . import _marshal as M

__all__ = ["view_attention_pool", "fold_attention_weights", "single_query_cross_attention", "decoder_forward_fine",
           "MAX_HEADS", "MAX_VIEWS", "MAX_ROWS", "KEY_WIDTHS"]

MAX_HEADS, MAX_VIEWS = 64, 16          # include/gdr.h GDR_VIEWATTN_MAX_HEADS / GDR_VIEWATTN_MAX_VIEWS
MAX_ROWS = 1 << 27
KEY_WIDTHS = (4, 8, 16)

_DTYPES = M.DTYPES
_NO_CPU = "the HIP view attention runs on ROCm/HIP tensors only (no CPU fallback)"


# ---- the core -------------------------------------------------------------------------------------------------------------

# rows of H heads of Ck = 4 are no multiple of 8 wide: copies of them get a padded stride (M.rows2d's and M.stride0's `pad`)
def _rows(t):
    return M.rows2d(t, pad=True)


def _stride0(t):
    return M.stride0(t, pad=True)


class _ViewAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, cond, H, Ck, V, scale):
        N, dev = t.shape[0], t.device
        t, cond = _rows(t), _rows(cond)
        with torch.cuda.device(dev):
            out = torch.empty(N, M.up8(H * Ck), dtype=t.dtype, device=dev)[:, :H * Ck]
            if N:
                L.check(L.load().gdr_viewattn_forward(t.data_ptr(), _stride0(t), _DTYPES[t.dtype], cond.data_ptr(), _stride0(cond),
                                                      _DTYPES[cond.dtype], N, H, Ck, V, scale, out.data_ptr(), _stride0(out),
                                                      _DTYPES[out.dtype], M.stream()), "gdr_viewattn_forward")
        ctx.save_for_backward(t, cond)
        ctx.shape = (H, Ck, V, scale)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        t, cond = ctx.saved_tensors
        H, Ck, V, scale = ctx.shape
        N, dev = t.shape[0], t.device
        if grad_out.dtype not in _DTYPES:
            grad_out = grad_out.to(t.dtype)
        grad_out = _rows(grad_out)
        with torch.cuda.device(dev):
            grad_t = torch.empty(N, H * Ck, dtype=t.dtype, device=dev)
            grad_cond = torch.empty(N, V * Ck, dtype=cond.dtype, device=dev)
            if N:
                L.check(L.load().gdr_viewattn_backward(grad_out.data_ptr(), _stride0(grad_out), _DTYPES[grad_out.dtype], t.data_ptr(),
                                                       _stride0(t), _DTYPES[t.dtype], cond.data_ptr(), _stride0(cond),
                                                       _DTYPES[cond.dtype], N, H, Ck, V, scale, grad_t.data_ptr(),
                                                       grad_cond.data_ptr(), M.stream()), "gdr_viewattn_backward")
        return grad_t, grad_cond, None, None, None, None


def view_attention_pool(t, cond, scale, num_heads=None):
    """t (N, H, Ck), or (N, H * Ck) with `num_heads=H`; cond (N, V, Ck) -> u (N, H, Ck) of t's dtype:
    u[n, h] = sum_v softmax_v(scale * <t[n, h], cond[n, v]>) * cond[n, v]."""
    M.check_float("t", t)
    M.check_float("cond", cond)
    if cond.dim() != 3:
        raise ValueError(f"cond must be (N, V, Ck), got {tuple(cond.shape)}")
    N, V, Ck = cond.shape
    if t.dim() == 3 and num_heads is None:
        H = t.shape[1]
    elif t.dim() == 2 and num_heads is not None:
        H = int(num_heads)
    else:
        raise ValueError(f"t must be (N, H, Ck), or (N, H * Ck) together with num_heads, got {tuple(t.shape)} and "
                         f"num_heads={num_heads}")
    if Ck not in KEY_WIDTHS:
        raise ValueError(f"a key width of {Ck} is outside the envelope {KEY_WIDTHS}")
    if not 1 <= H <= MAX_HEADS:
        raise ValueError(f"{H} heads are outside the envelope 1..{MAX_HEADS}")
    if not 1 <= V <= MAX_VIEWS:
        raise ValueError(f"{V} views are outside the envelope 1..{MAX_VIEWS}")
    if t.shape[0] != N or t.numel() != N * H * Ck or (t.dim() == 3 and t.shape[2] != Ck):
        raise ValueError(f"cond {tuple(cond.shape)} needs t ({N}, {H}, {Ck}) or ({N}, {H * Ck}), got {tuple(t.shape)}")
    if N > MAX_ROWS:
        raise ValueError("more than 2^27 rows")
    scale = float(scale)
    if scale != scale:
        raise ValueError("scale is NaN")
    for name, x in (("t", t), ("cond", cond)):
        if not x.is_cuda:
            raise RuntimeError(_NO_CPU)
    if cond.device != t.device:
        raise RuntimeError(f"cond must live on t's device ({t.device}), not {cond.device}")
    if not cond.is_contiguous():          # (the reference's einsum('lcb->blc', ...) hands a view with strides (1, 8 N, N))
        cond = cond.contiguous()
    out = _ViewAttention.apply(t.reshape(N, H * Ck), cond.view(N, V * Ck), H, Ck, V, scale)
    return out.view(N, H, Ck)


# ---- the fold -------------------------------------------------------------------------------------------------------------

def fold_attention_weights(mha):
    """(A (H Ck, E), a_bias (H Ck,) or None, Bm (E, H Ck), b_bias (E,) or None, scale) of an nn.MultiheadAttention, in fp32
    (or the module's wider dtype) with autocast disabled; differentiable with respect to every parameter of the module."""
    if not isinstance(mha, torch.nn.MultiheadAttention):
        raise TypeError(f"mha must be an nn.MultiheadAttention, not {type(mha).__name__}")
    if not mha.batch_first:
        raise NotImplementedError("the fold covers batch_first=True only")
    if mha.bias_k is not None or mha.bias_v is not None:
        raise NotImplementedError("add_bias_kv appends a learned key / value: the fold does not cover it")
    if mha.add_zero_attn:
        raise NotImplementedError("add_zero_attn appends a zero key: the fold does not cover it")
    if mha.dropout > 0 and mha.training:
        raise NotImplementedError("attention dropout in training mode: the fold does not cover it")
    E, H, d = mha.embed_dim, mha.num_heads, mha.head_dim
    dev_type = mha.out_proj.weight.device.type
    with torch.autocast(dev_type, enabled=False):
        def wide(w):
            return w if w.dtype == torch.float64 else w.float()

        if mha._qkv_same_embed_dim:
            wq, wk, wv = wide(mha.in_proj_weight).chunk(3)
        else:
            wq, wk, wv = wide(mha.q_proj_weight), wide(mha.k_proj_weight), wide(mha.v_proj_weight)
        wo = wide(mha.out_proj.weight)
        Ck = wk.shape[1]
        if wv.shape[1] != Ck:
            raise NotImplementedError(f"kdim {Ck} != vdim {wv.shape[1]}: keys and values must be the same tensor")
        wq_h, wk_h, wv_h = wq.view(H, d, E), wk.view(H, d, Ck), wv.view(H, d, Ck)
        wo_h = wo.view(E, H, d)
        A = torch.einsum("hdc,hde->hce", wk_h, wq_h).reshape(H * Ck, E)
        Bm = torch.einsum("ehd,hdc->ehc", wo_h, wv_h).reshape(E, H * Ck)
        a_bias = b_bias = None
        if mha.in_proj_bias is not None:
            bq, _, bv = wide(mha.in_proj_bias).chunk(3)
            a_bias = torch.einsum("hdc,hd->hc", wk_h, bq.view(H, d)).reshape(H * Ck)
            b_bias = wo @ bv
        if mha.out_proj.bias is not None:
            bo = wide(mha.out_proj.bias)
            b_bias = bo if b_bias is None else b_bias + bo
    return A, a_bias, Bm, b_bias, float(d) ** -0.5


def _pooled(mha, x, cond):
    """(u (N, H Ck) fp32, Bm, b_bias): everything of the attention before the product with Bm, in fp32 without autocast"""
    if x.dim() != 2 or cond.dim() != 3 or cond.shape[0] != x.shape[0]:
        raise ValueError(f"x must be (N, E) and cond (N, V, Ck), got {tuple(x.shape)} and {tuple(cond.shape)}")
    A, a_bias, Bm, b_bias, scale = fold_attention_weights(mha)
    if x.shape[1] != A.shape[1] or cond.shape[2] * mha.num_heads != A.shape[0]:
        raise ValueError(f"the module takes x (N, {A.shape[1]}) and cond (N, V, {A.shape[0] // mha.num_heads}), got "
                         f"{tuple(x.shape)} and {tuple(cond.shape)}")
    with torch.autocast(x.device.type, enabled=False):
        t = F.linear(x.to(A.dtype) if x.dtype != torch.float64 else x, A, a_bias)
        if t.dtype == torch.float64:
            raise TypeError("the HIP view attention computes in float32: float64 inputs are not supported")
        u = view_attention_pool(t, cond, scale, num_heads=mha.num_heads)
    return u.view(x.shape[0], -1), Bm, b_bias


def single_query_cross_attention(mha, x, cond):
    """x (N, E), cond (N, V, Ck) -> (N, E): `mha(x[:, None], cond, cond, need_weights=False)[0][:, 0]` in the folded form."""
    u, Bm, b_bias = _pooled(mha, x, cond)
    out = F.linear(u, Bm, b_bias)
    return out if torch.is_autocast_enabled(x.device.type) else out.to(x.dtype)


def decoder_forward_fine(self, volume_feat, point_feats):
    """The forward_fine of the reference's Decoder: volume_feat (N, E), point_feats (N, V, Ck) -> ((N, 1, feature_dim),
    (N, 1, rest)) float32.  Reads only `self.norm`, `self.cross_att`, `self.mlp_fine` (0 Linear, 1 ReLU, 2 Linear) and
    `self.feature_dim`; Bm is folded into the first Linear.  Bind it with `network.Decoder.forward_fine = decoder_forward_fine`."""
    u, Bm, b_bias = _pooled(self.cross_att, self.norm(volume_feat), point_feats)
    first = self.mlp_fine[0]
    with torch.autocast(u.device.type, enabled=False):
        w1 = first.weight.float()
        weight = w1 @ Bm
        bias = None if first.bias is None else first.bias.float()
        if b_bias is not None:
            bias = w1 @ b_bias if bias is None else w1 @ b_bias + bias
    hidden = F.linear(u, weight, bias)
    if not torch.is_autocast_enabled(u.device.type):
        hidden = hidden.to(first.weight.dtype)         # (a decoder held in 16 bits: the last Linear takes its own dtype)
    y = self.mlp_fine[2](self.mlp_fine[1](hidden)).float()[:, None]
    return y.split([self.feature_dim, y.shape[-1] - self.feature_dim], dim=-1)
