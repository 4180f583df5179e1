"""Group cross attention of the volume transformer on the MI355X (csrc/groupattn.hip, include/gdr.h gdr_groupattn_*): the
reference's `GroupAttBlock` (lightning/network.py) cuts a (B, C, D, H, W) volume into patches of bs^3 voxels, normalises them,
lets the Lq = bs^3 queries of a patch attend to the Lk image tokens of that patch through `nn.MultiheadAttention(C, heads,
kdim = vdim = cond width)`, runs an MLP, normalises again and carries the patches back into the volume for a Conv3d.

    group_cross_attention(q, k, v, scale, num_heads)    the core: q (M, Lq, E), k / v (M, Lk, E) -> (M, Lq, E), E = H Dh
        s[m, h, i, j] = scale <q[m, i, h], k[m, j, h]>,  p = softmax_j(s),  out[m, i, h] = sum_j p[m, h, i, j] v[m, j, h]
    patchify_layer_norm(vol, bs, weight, bias, eps)     -> (patches, layer_norm(patches)), patches (B G, bs^3, C) in the
                                                        reference's order: one launch instead of two copies and a norm
    layer_norm_unpatchify(patches, vol_shape, bs, ...)  -> layer_norm(patches) as a (B, C, D, H, W) channels-last volume
    grouped_cross_attention(mha, x, cond)               = mha(x, cond, cond, need_weights=False)[0]
    group_att_block_forward                             a forward to bind: network.GroupAttBlock.forward = group_att_block_forward

The key width (the image feature width) is far from the head width, so the projections stay torch products (every weight
gradient flows through them): q from x, and k and v as the two halves of ONE product of cond with cat(Wk, Wv), which the core
reads through row strides without a copy.  Patch order: group g = (gd Gh + gh) Gw + gw, in-patch l = (z bs + y) bs + x, patch
row (b G + g) bs^3 + l is voxel (gd bs + z, gh bs + y, gw bs + x); with the volume stored channels_last_3d both directions
are permutations of whole C-element rows.

The kernels compute in fp32 from f32 / f16 / bf16 inputs (each input's dtype is independent), save nothing but their inputs
for the backward, use no atomics (two calls are bitwise equal) and never synchronise with the host.  The core's result has q's
dtype; a norm's result has `out_dtype`, by default torch's rule for layer_norm (float32 under autocast, else the input's);
gradients come back in the dtypes of the inputs.  GPU tensors only (no CPU fallback).  Envelope of the core: Dh 8, 16 or 32,
1 <= H <= 64, 1 <= Lq, Lk <= 64, M <= 2^24; of the norms: C a multiple of 8 in 8..1024, 1 <= bs <= 8, rows below 2^31.  M = 0 /
no rows return empty tensors without loading the library.  Non-finite inputs are memory-safe and otherwise unspecified.
Outside the core's envelope `grouped_cross_attention` runs F.scaled_dot_product_attention on the same projected tensors and
warns once.  Under autocast the bound forward keeps the patches, both fused norms' results and its own result in the autocast
dtype, as the reference's path does through its two einsums, and it hands the convolution an NCDHW copy of the channels-last
volume because that is the faster of torch's convolutions (BASELINE §4-groupattn).  `CONV_BACKEND = "hip"` hands
the channels-last volume to conv3d.py's kernels instead; the default "torch" is the path above, bit for bit.
"""
from __future__ import annotations

import warnings

import torch
import torch.nn.functional as F

from . import _lib as L
from . import _marshal as M
from . import conv3d as C3

__all__ = ["group_cross_attention", "patchify_layer_norm", "layer_norm_unpatchify", "project_qkv", "grouped_cross_attention",
           "group_att_block_forward", "in_envelope", "MAX_HEADS", "MAX_QUERIES", "MAX_KEYS", "MAX_GROUPS", "HEAD_WIDTHS",
           "MAX_CHANNELS", "MAX_BLOCK", "MAX_ROWS"]

MAX_HEADS, MAX_QUERIES, MAX_KEYS = L.GDR_GROUPATTN_MAX_HEADS, L.GDR_GROUPATTN_MAX_QUERIES, L.GDR_GROUPATTN_MAX_KEYS
MAX_GROUPS = 1 << 24
HEAD_WIDTHS = (8, 16, 32)
MAX_CHANNELS, MAX_BLOCK = L.GDR_NORM_MAX_CHANNELS, L.GDR_GROUPATTN_MAX_BLOCK
MAX_ROWS = (1 << 31) - 1

# the convolution at the tail of group_att_block_forward: "torch" = the module's own nn.Conv3d on an NCDHW copy of the volume (the
# default); "hip" = conv3d.conv3d_of on the channels-last volume itself, the residual added in its epilogue, wherever the module
# and the shape lie inside that kernel's envelope (INTEGRATION §15 has the measured recommendation per mode)
CONV_BACKEND = "torch"

_DTYPES = M.DTYPES
_F32 = _DTYPES[torch.float32]
_NO_CPU = "the HIP group attention runs on ROCm/HIP tensors only (no CPU fallback)"


def _dt(t):
    return _F32 if t is None else _DTYPES[t.dtype]


# ---- the core -------------------------------------------------------------------------------------------------------------

def _rows(t):
    """t (M, L, E) as the kernels read its M L rows: (t or a copy, row stride).  Unit channel stride, a 16-byte aligned base,
    one row stride over both leading axes that is a multiple of 8 and covers the row; a layout that does not fit is copied."""
    m, l, e = t.shape
    s = t.stride(1) if l > 1 else (t.stride(0) if m > 1 else e)
    if t.numel() and (t.stride(2) != 1 or s % 8 or s < e or t.data_ptr() % 16 or (m > 1 and l > 1 and t.stride(0) != l * s)):
        t, s = t.contiguous(), e
    return t, s


class _GroupAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, H, scale):
        m, lq, e = q.shape
        lk, dev = k.shape[1], q.device
        (q, qs), (k, ks), (v, vs) = _rows(q), _rows(k), _rows(v)
        with torch.cuda.device(dev):
            out = torch.empty(m, lq, e, dtype=q.dtype, device=dev)
            if m:
                L.check(L.load().gdr_groupattn_forward(q.data_ptr(), qs, _DTYPES[q.dtype], k.data_ptr(), ks, _DTYPES[k.dtype],
                                                       v.data_ptr(), vs, _DTYPES[v.dtype], m, lq, lk, H, e // H, scale,
                                                       out.data_ptr(), _DTYPES[out.dtype], M.stream()), "gdr_groupattn_forward")
        ctx.save_for_backward(q, k, v)
        ctx.shape = (H, scale)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        q, k, v = ctx.saved_tensors
        H, scale = ctx.shape
        m, lq, e = q.shape
        lk, dev = k.shape[1], q.device
        if grad_out.dtype not in _DTYPES:
            grad_out = grad_out.to(q.dtype)
        (q, qs), (k, ks), (v, vs), (grad_out, gs) = _rows(q), _rows(k), _rows(v), _rows(grad_out)
        with torch.cuda.device(dev):
            grad_q = torch.empty(m, lq, e, dtype=q.dtype, device=dev)
            grad_k = torch.empty(m, lk, e, dtype=k.dtype, device=dev)
            grad_v = torch.empty(m, lk, e, dtype=v.dtype, device=dev)
            if m:
                L.check(L.load().gdr_groupattn_backward(grad_out.data_ptr(), gs, _DTYPES[grad_out.dtype], q.data_ptr(), qs,
                                                        _DTYPES[q.dtype], k.data_ptr(), ks, _DTYPES[k.dtype], v.data_ptr(), vs,
                                                        _DTYPES[v.dtype], m, lq, lk, H, e // H, scale, grad_q.data_ptr(),
                                                        grad_k.data_ptr(), grad_v.data_ptr(), M.stream()), "gdr_groupattn_backward")
        return grad_q, grad_k, grad_v, None, None


def in_envelope(m, lq, lk, heads, head_width):
    """whether the core serves this shape"""
    return (head_width in HEAD_WIDTHS and 1 <= heads <= MAX_HEADS and 1 <= lq <= MAX_QUERIES and 1 <= lk <= MAX_KEYS
            and m <= MAX_GROUPS)


def group_cross_attention(q, k, v, scale, num_heads):
    """q (M, Lq, E), k and v (M, Lk, E), E = num_heads * Dh -> (M, Lq, E) of q's dtype: per group m and head h,
    softmax_j(scale <q[m, i, h], k[m, j, h]>) applied to v[m, :, h]."""
    for name, t in (("q", q), ("k", k), ("v", v)):
        M.check_float(name, t, 3)
    H = int(num_heads)
    m, lq, e = q.shape
    lk = k.shape[1]
    if k.shape != (m, lk, e) or v.shape != (m, lk, e):
        raise ValueError(f"q {tuple(q.shape)} needs k and v ({m}, Lk, {e}), got {tuple(k.shape)} and {tuple(v.shape)}")
    if not 1 <= H <= MAX_HEADS:
        raise ValueError(f"{H} heads are outside the envelope 1..{MAX_HEADS}")
    if e % H or e // H not in HEAD_WIDTHS:
        raise ValueError(f"a width of {e} over {H} heads is outside the envelope: head widths {HEAD_WIDTHS}")
    if not 1 <= lq <= MAX_QUERIES:
        raise ValueError(f"{lq} queries per group are outside the envelope 1..{MAX_QUERIES}")
    if not 1 <= lk <= MAX_KEYS:
        raise ValueError(f"{lk} keys per group are outside the envelope 1..{MAX_KEYS}")
    if m > MAX_GROUPS:
        raise ValueError("more than 2^24 groups")
    scale = float(scale)
    if scale != scale:
        raise ValueError("scale is NaN")
    M.check_devices((("q", q), ("k", k), ("v", v)), _NO_CPU)
    return _GroupAttention.apply(q, k, v, H, scale)


# ---- the two permuting LayerNorms -----------------------------------------------------------------------------------------

def _norm_out_dtype(x, out_dtype):
    if out_dtype is None:
        return torch.float32 if torch.is_autocast_enabled("cuda") else x.dtype
    if out_dtype not in _DTYPES:
        raise TypeError(f"out_dtype must be float32, float16 or bfloat16, not {out_dtype}")
    return out_dtype


def _check_affine(weight, bias, C):
    for name, t in (("weight", weight), ("bias", bias)):
        if t is not None:
            M.check_float(name, t, 1)
            if t.shape[0] != C:
                raise ValueError(f"{name} must have {C} elements, got {tuple(t.shape)}")


def _check_volume(shape, bs):
    """(B, C, D, H, W) -> rows"""
    if len(shape) != 5:
        raise ValueError(f"a volume is (B, C, D, H, W), got {tuple(shape)}")
    B, C, D, H, W = (int(s) for s in shape)
    if not 1 <= bs <= MAX_BLOCK:
        raise ValueError(f"block_size {bs} is outside the envelope 1..{MAX_BLOCK}")
    if C < 8 or C > MAX_CHANNELS or C % 8:
        raise ValueError(f"{C} channels are outside the envelope: a multiple of 8 in 8..{MAX_CHANNELS}")
    if min(D, H, W) < 1 or D % bs or H % bs or W % bs:
        raise ValueError(f"D, H and W must be positive multiples of block_size {bs}, got {(D, H, W)}")
    if B * D * H * W > MAX_ROWS:
        raise ValueError("more than 2^31 - 1 rows")
    return B * D * H * W


_dense = M.dense_aligned


def _affine_grads(ctx, weight, bias, which):
    need_w, need_b = weight is not None and ctx.needs_input_grad[which], bias is not None and ctx.needs_input_grad[which + 1]
    grad_w = torch.empty_like(weight, memory_format=torch.contiguous_format) if need_w else None
    grad_b = torch.empty_like(bias, memory_format=torch.contiguous_format) if need_b else None
    return grad_w, grad_b


def _workspace(lib, rows, C, dev):
    nbytes = lib.gdr_groupattn_norm_backward_bytes(rows, C)
    if nbytes == 0:
        L.check(-1, "gdr_groupattn_norm_backward_bytes")
    return M.workspace(nbytes, dev)


class _PatchifyLayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vol, weight, bias, bs, eps, patches_dtype, out_dtype):
        B, C, D, H, W = vol.shape
        dev = vol.device
        rows = _dense(vol.permute(0, 2, 3, 4, 1))        # (B, D, H, W, C): free for a channels_last_3d volume, one copy else
        weight, bias = _dense(weight), _dense(bias)
        G, b3 = (D // bs) * (H // bs) * (W // bs), bs ** 3
        with torch.cuda.device(dev):
            patches = torch.empty(B * G, b3, C, dtype=patches_dtype, device=dev)
            normed = torch.empty(B * G, b3, C, dtype=out_dtype, device=dev)
            if patches.numel():
                L.check(L.load().gdr_groupattn_patchify_norm_forward(rows.data_ptr(), _DTYPES[vol.dtype], M.ptr(weight), _dt(weight),
                                                                     M.ptr(bias), _dt(bias), B, D, H, W, C, bs, eps,
                                                                     patches.data_ptr(), _DTYPES[patches_dtype], normed.data_ptr(),
                                                                     _DTYPES[out_dtype], M.stream()),
                        "gdr_groupattn_patchify_norm_forward")
        ctx.save_for_backward(rows, weight, bias)
        ctx.bs, ctx.eps, ctx.patches_dtype = bs, eps, patches_dtype
        ctx.set_materialize_grads(False)
        return patches, normed

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_patches, grad_normed):
        rows, weight, bias = ctx.saved_tensors
        B, D, H, W, C = rows.shape
        dev = rows.device
        grad_patches, grad_normed = _dense(grad_patches), _dense(grad_normed)
        lib = L.load() if rows.numel() or weight is not None or bias is not None else None
        with torch.cuda.device(dev):
            grad_rows = torch.empty_like(rows)
            grad_w, grad_b = _affine_grads(ctx, weight, bias, 1)
            if lib is not None:
                ws, base, usable = _workspace(lib, rows.numel() // C, C, dev)
                L.check(lib.gdr_groupattn_patchify_norm_backward(M.ptr_or_none_if_empty(grad_normed), _dt(grad_normed),
                                                                 M.ptr_or_none_if_empty(grad_patches), _dt(grad_patches),
                                                                 M.ptr_or_none_if_empty(rows), _DTYPES[rows.dtype],
                                                                 _DTYPES[ctx.patches_dtype], M.ptr(weight), _dt(weight), _dt(bias), B,
                                                                 D, H, W, C, ctx.bs, ctx.eps, base, usable,
                                                                 M.ptr_or_none_if_empty(grad_rows), M.ptr(grad_w), M.ptr(grad_b),
                                                                 M.stream()), "gdr_groupattn_patchify_norm_backward")
        return grad_rows.permute(0, 4, 1, 2, 3), grad_w, grad_b, None, None, None, None


def patchify_layer_norm(vol, block_size, weight=None, bias=None, eps=1e-5, out_dtype=None, patches_dtype=None):
    """vol (B, C, D, H, W) -> (patches, normed), both (B G, bs^3, C): the rows of vol in the reference's patch order (vol's
    dtype and the same bits; rounded to patches_dtype where one is given) and F.layer_norm(patches) over C (out_dtype; by
    default float32 under autocast, else vol's dtype).  A vol that is not channels_last_3d is made so with one copy."""
    M.check_float("vol", vol)
    bs = int(block_size)
    _check_volume(vol.shape, bs)
    _check_affine(weight, bias, vol.shape[1])
    out_dtype = _norm_out_dtype(vol, out_dtype)
    if patches_dtype is None:
        patches_dtype = vol.dtype
    elif patches_dtype not in _DTYPES:
        raise TypeError(f"patches_dtype must be float32, float16 or bfloat16, not {patches_dtype}")
    M.check_devices([("vol", vol)] + [(n, t) for n, t in (("weight", weight), ("bias", bias)) if t is not None], _NO_CPU)
    return _PatchifyLayerNorm.apply(vol, weight, bias, bs, float(eps), patches_dtype, out_dtype)


class _LayerNormUnpatchify(torch.autograd.Function):
    @staticmethod
    def forward(ctx, patches, weight, bias, shape, bs, eps, out_dtype):
        B, C, D, H, W = shape
        dev = patches.device
        patches, weight, bias = _dense(patches), _dense(weight), _dense(bias)
        with torch.cuda.device(dev):
            vol = torch.empty(B, D, H, W, C, dtype=out_dtype, device=dev)
            if vol.numel():
                L.check(L.load().gdr_groupattn_norm_unpatchify_forward(patches.data_ptr(), _DTYPES[patches.dtype], M.ptr(weight),
                                                                       _dt(weight), M.ptr(bias), _dt(bias), B, D, H, W, C, bs, eps,
                                                                       vol.data_ptr(), _DTYPES[out_dtype], M.stream()),
                        "gdr_groupattn_norm_unpatchify_forward")
        ctx.save_for_backward(patches, weight, bias)
        ctx.shape, ctx.bs, ctx.eps = shape, bs, eps
        return vol.permute(0, 4, 1, 2, 3)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_vol):
        patches, weight, bias = ctx.saved_tensors
        B, C, D, H, W = ctx.shape
        dev = patches.device
        if grad_vol.dtype not in _DTYPES:
            grad_vol = grad_vol.to(patches.dtype)
        grad_rows = _dense(grad_vol.permute(0, 2, 3, 4, 1))
        lib = L.load() if patches.numel() or weight is not None or bias is not None else None
        with torch.cuda.device(dev):
            grad_patches = torch.empty_like(patches)
            grad_w, grad_b = _affine_grads(ctx, weight, bias, 1)
            if lib is not None:
                ws, base, usable = _workspace(lib, patches.numel() // C, C, dev)
                L.check(lib.gdr_groupattn_norm_unpatchify_backward(M.ptr_or_none_if_empty(grad_rows), _DTYPES[grad_rows.dtype],
                                                                   M.ptr_or_none_if_empty(patches), _DTYPES[patches.dtype],
                                                                   M.ptr(weight), _dt(weight), _dt(bias), B, D, H, W, C, ctx.bs,
                                                                   ctx.eps, base, usable, M.ptr_or_none_if_empty(grad_patches),
                                                                   M.ptr(grad_w), M.ptr(grad_b), M.stream()),
                        "gdr_groupattn_norm_unpatchify_backward")
        return grad_patches, grad_w, grad_b, None, None, None, None


def layer_norm_unpatchify(patches, vol_shape, block_size, weight=None, bias=None, eps=1e-5, out_dtype=None):
    """patches (B G, bs^3, C) in patch order, vol_shape (B, C, D, H, W) -> F.layer_norm(patches) over C as a volume of that
    logical shape with channels_last_3d strides (out_dtype; by default float32 under autocast, else patches' dtype)."""
    M.check_float("patches", patches, 3)
    bs = int(block_size)
    shape = tuple(int(s) for s in vol_shape)
    rows = _check_volume(shape, bs)
    B, C, D, H, W = shape
    if patches.shape != (rows // bs ** 3, bs ** 3, C):
        raise ValueError(f"a volume {shape} in blocks of {bs} has patches ({rows // bs ** 3}, {bs ** 3}, {C}), got {tuple(patches.shape)}")
    _check_affine(weight, bias, C)
    out_dtype = _norm_out_dtype(patches, out_dtype)
    M.check_devices([("patches", patches)] + [(n, t) for n, t in (("weight", weight), ("bias", bias)) if t is not None], _NO_CPU)
    return _LayerNormUnpatchify.apply(patches, weight, bias, shape, bs, float(eps), out_dtype)


# ---- the attention of an nn.MultiheadAttention around the core --------------------------------------------------------------

def project_qkv(mha, x, cond):
    """(q (M, Lq, E), k, v (M, Lk, E), scale) of an nn.MultiheadAttention for queries x (M, Lq, E) and keys = values cond
    (M, Lk, kdim): two F.linear, k and v the halves of one product of cond with cat(Wk, Wv).  Pure torch (works on the CPU)."""
    if not isinstance(mha, torch.nn.MultiheadAttention):
        raise TypeError(f"mha must be an nn.MultiheadAttention, not {type(mha).__name__}")
    if not mha.batch_first:
        raise NotImplementedError("the group attention covers batch_first=True only")
    if mha.bias_k is not None or mha.bias_v is not None:
        raise NotImplementedError("add_bias_kv appends a learned key / value: the group attention does not cover it")
    if mha.add_zero_attn:
        raise NotImplementedError("add_zero_attn appends a zero key: the group attention does not cover it")
    if mha.dropout > 0 and mha.training:
        raise NotImplementedError("attention dropout in training mode: the group attention does not cover it")
    if mha.kdim != mha.vdim:
        raise NotImplementedError(f"kdim {mha.kdim} != vdim {mha.vdim}: keys and values must be the same tensor")
    E = mha.embed_dim
    if x.dim() != 3 or cond.dim() != 3 or cond.shape[0] != x.shape[0] or x.shape[2] != E or cond.shape[2] != mha.kdim:
        raise ValueError(f"the module takes x (M, Lq, {E}) and cond (M, Lk, {mha.kdim}), got {tuple(x.shape)} and {tuple(cond.shape)}")
    if mha._qkv_same_embed_dim:
        wq, wkv = mha.in_proj_weight[:E], mha.in_proj_weight[E:]
    else:
        wq, wkv = mha.q_proj_weight, torch.cat([mha.k_proj_weight, mha.v_proj_weight])
    bq = bkv = None
    if mha.in_proj_bias is not None:
        bq, bkv = mha.in_proj_bias[:E], mha.in_proj_bias[E:]
    kv = F.linear(cond, wkv, bkv)
    return F.linear(x, wq, bq), kv[..., :E], kv[..., E:], float(mha.head_dim) ** -0.5


_warned = False


def _warn_once(shape):
    global _warned
    if not _warned:
        _warned = True
        warnings.warn(f"group attention of shape (M, Lq, Lk, H, Dh) = {shape} is outside the HIP core's envelope: it runs through "
                      "F.scaled_dot_product_attention (said once)", RuntimeWarning, stacklevel=3)


def grouped_cross_attention(mha, x, cond):
    """x (M, Lq, E), cond (M, Lk, kdim) -> (M, Lq, E): `mha(x, cond, cond, need_weights=False)[0]` with the HIP core between
    the torch products; outside the core's envelope the core is F.scaled_dot_product_attention on the same tensors."""
    q, k, v, scale = project_qkv(mha, x, cond)
    m, lq, e = q.shape
    H, lk = mha.num_heads, k.shape[1]
    if in_envelope(m, lq, lk, H, e // H):
        o = group_cross_attention(q, k, v, scale, H)
    else:
        _warn_once((m, lq, lk, H, e // H))
        heads = [t.reshape(m, t.shape[1], H, e // H).transpose(1, 2) for t in (q, k, v)]
        o = F.scaled_dot_product_attention(*heads, scale=scale).transpose(1, 2).reshape(m, lq, e)
    return mha.out_proj(o)


def group_att_block_forward(self, x, cond, group_axis, block_size):
    """The forward of the reference's GroupAttBlock: x (B, C, D, H, W), cond (B G, Lk, cond width) -> (B, C, D, H, W) with
    channels_last_3d strides (the next block's patchify_layer_norm then reads it without a copy).  Reads only `self.norm1`, `self.cross_attn`, `self.norm2`, `self.mlp`, `self.norm3`, `self.cnn`.
    Bind it with `network.GroupAttBlock.forward = group_att_block_forward`."""
    # under autocast the reference's two permuting einsums run in the autocast dtype (einsum is on autocast's lower-precision
    # list): the patches, and with them the whole residual stream, and the volume handed to the convolution are rounded to it.
    # The first product would round norm1's float32 result as well: the kernels write all three in that dtype at once
    cast = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else None
    patches, normed = patchify_layer_norm(x, block_size, self.norm1.weight, self.norm1.bias, self.norm1.eps, out_dtype=cast,
                                          patches_dtype=cast)
    patches = patches + grouped_cross_attention(self.cross_attn, normed, cond)
    patches = patches + self.mlp(self.norm2(patches))
    vol = layer_norm_unpatchify(patches, x.shape, block_size, self.norm3.weight, self.norm3.bias, self.norm3.eps, out_dtype=cast)
    if CONV_BACKEND not in ("torch", "hip"):
        raise ValueError(f"groupattn.CONV_BACKEND must be 'torch' or 'hip', not {CONV_BACKEND!r}")
    if CONV_BACKEND == "hip" and C3.covers(self.cnn) and C3.in_envelope(vol.shape[0], self.cnn.in_channels, self.cnn.out_channels, *vol.shape[2:]):
        return C3.conv3d_of(self.cnn, vol, add_input=True)
    # torch's convolution gets an NCDHW copy: on channels-last input it measured 0.7 ms (fp32) to 6 ms (bf16) slower at the
    # reference shape, more than this forward saves (BASELINE §4-groupattn); the sum keeps vol's channels-last strides
    return vol + self.cnn(vol.contiguous())
