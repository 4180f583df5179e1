"""The residual junctions of the point decoder's Block on the MI355X (csrc/block.hip, include/gdr.h gdr_block_*; reference
lightning/point_decoder/autoencoder.py, Block.forward).  The submanifold conv (`spconv` drop-in), the patch attention
(`serattn`) and the `nn.Linear` products stay where they are; what is fused is the row-wise glue between them.

`junction(skip, branch, keep=None, pre=None, post=None, offset=None) -> (y, n or None)`, one launch, per row r of (N, C):

    b = pre(branch[r]);   y = rd(skip[r] + rd(keep[r] * b));   n = post(y)

A norm spec is None, `("ln", weight_or_None, bias_or_None, eps)` (F.layer_norm over the C channels) or `("ada", scale, eps)`
(`norm.ada_layer_norm`'s rules over `offset`, (B,) integer segment ends read on the device: rows at or behind offset[-1] are
zero through that norm, an empty segment is legal; y is defined for every row).  keep is (N,) / (N, 1) or None, the tensor
drop_path multiplies by.  `rd` rounds to the dtype the torch composition gives that intermediate, with autocast on and off
(`norm._result_dtype` for a norm's result, torch's promotion for the product and the sum).  n is None when post is None.
With an ada `post`, n is bit for bit `norm.ada_layer_norm(y, scale, offset)`; with a plain LN without affine it is
`norm.ada_layer_norm(y, ones, offset)`.

Arithmetic is fp32 from f32 / f16 / bf16 inputs (each input's dtype is independent).  The one-launch backward takes grad_y and
grad_n (either may be absent), recomputes b, y and both sets of statistics from skip, branch and keep, and writes grad_skip,
grad_branch and each norm's parameter gradient (ada: grad_scale by ada's fold; LN with affine: grad_weight / grad_bias from
per-workgroup partials folded in a fixed order).  No atomics (two calls are bitwise equal), a gradient nobody needs is not
stored, nothing synchronises with the host, autocast is switched off inside.  GPU tensors only.  Envelope: C a multiple of 8
in 8..1024, 1 <= B <= 1024, N below 2^31; N = 0 returns empty tensors without loading the library.

`block_forward` is a forward to bind onto the reference's class (`autoencoder.Block.forward = block.block_forward`): under
BLOCK_BACKEND = "hip", wherever `covers` and the shape hold, the conv and cpe[1], junction (pre = cpe[2], post = norm1),
self.attn, the drop-path draw (the reference's own, so a seeded run stays aligned), junction (post = norm2), the MLP, the second
draw, junction, replace_feature; anywhere else the reference's lines.
"""
from __future__ import annotations

import torch
from torch import nn

from . import _lib as L
from . import _marshal as M
from . import norm as _norm
from . import upscale as _upscale

__all__ = ["junction", "covers", "in_envelope", "block_forward", "BLOCK_BACKEND"]

# the path of the bound forward: "hip" (the junctions wherever they cover the module and the shape) or "torch" (the
# reference's lines over this repository's drop-ins).  "hip" is the default by the project's rule, on the plain LayerNorm that
# Network builds: under bf16 autocast forward + backward its median was lower and the ranges did not overlap at both base-config
# shapes (scripts/bench_block.py, BASELINE §4-block: 2014 us against 2147 us at 12 000 x 160, 3290 us against 3404 us at
# 19 200 x 256).  With AdaLayerNorm the medians were lower too (2147 against 2226, 3432 against 3443) but the ranges overlapped.
BLOCK_BACKEND = "hip"

MAX_CHANNELS, MAX_SEGMENTS, MAX_ROWS = _norm.MAX_CHANNELS, _norm.MAX_SEGMENTS, _norm.MAX_ROWS
_DTYPES = M.DTYPES
_NO_CPU = "the HIP Block junctions run on ROCm/HIP tensors only (no CPU fallback)"
_KINDS = {"ln": L.GDR_BLOCK_NORM_LN, "ada": L.GDR_BLOCK_NORM_ADA}


def in_envelope(N, C, B=1):
    """whether the kernels serve N rows of C channels in B segments"""
    return 0 <= N <= MAX_ROWS and 8 <= C <= MAX_CHANNELS and C % 8 == 0 and 1 <= B <= MAX_SEGMENTS


# ---- junction -------------------------------------------------------------------------------------------------------------

def _check_spec(name, spec, C):
    """-> (kind, w, b, eps): the spec checked; kind is a GDR_BLOCK_NORM_* code"""
    if spec is None:
        return L.GDR_BLOCK_NORM_NONE, None, None, 0.0
    if not isinstance(spec, (tuple, list)) or not spec or spec[0] not in _KINDS:
        raise TypeError(f"{name} must be None, ('ln', weight, bias, eps) or ('ada', scale, eps), not {spec!r}")
    if spec[0] == "ada":
        if len(spec) != 3:
            raise TypeError(f"{name} must be ('ada', scale, eps)")
        _, scale, eps = spec
        M.check_float(f"{name} scale", scale, 2)
        if scale.shape[1] != C:
            raise ValueError(f"{name} scale must be (B, {C}), got {tuple(scale.shape)}")
        return L.GDR_BLOCK_NORM_ADA, scale, None, float(eps)
    if len(spec) != 4:
        raise TypeError(f"{name} must be ('ln', weight, bias, eps)")
    _, w, b, eps = spec
    for what, t in (("weight", w), ("bias", b)):
        if t is not None:
            M.check_float(f"{name} {what}", t, 1)
            if t.shape[0] != C:
                raise ValueError(f"{name} {what} must be ({C},), got {tuple(t.shape)}")
    kind = L.GDR_BLOCK_NORM_LN if w is None and b is None else L.GDR_BLOCK_NORM_LN_AFFINE
    return kind, w, b, float(eps)


def _norm_dtype(kind, w, x_dtype):
    """the dtype of a norm's result on an input of x_dtype, as the torch composition gives it"""
    if kind == L.GDR_BLOCK_NORM_NONE:
        return x_dtype
    if kind == L.GDR_BLOCK_NORM_ADA:
        return _norm._result_dtype(x_dtype, w.dtype)
    return _norm._result_dtype(x_dtype)


def _desc(kind, w, b, eps, grad_w=None, grad_b=None):
    """the GdrBlockNorm of a norm (w, b as the kernels read them), or None"""
    if kind == L.GDR_BLOCK_NORM_NONE:
        return None
    d = L.GdrBlockNorm()
    d.kind, d.eps = kind, eps
    if w is not None:
        d.w, d.w_dtype = w.data_ptr(), _DTYPES[w.dtype]
        d.w_stride = M.stride0(w) if w.dim() == 2 else 0
        d.grad_w = None if grad_w is None else grad_w.data_ptr()
    if b is not None:
        d.b, d.b_dtype = b.data_ptr(), _DTYPES[b.dtype]
        d.grad_b = None if grad_b is None else grad_b.data_ptr()
    return d


def _param(kind, t):
    if t is None:
        return None
    return M.rows2d(t) if kind == L.GDR_BLOCK_NORM_ADA else M.dense_aligned(t)


class _Junction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, skip, branch, keep, pre_w, pre_b, post_w, post_b, offset, meta):
        pre_kind, pre_eps, post_kind, post_eps, b0_dtype, kb_dtype, y_dtype, n_dtype, B = meta
        N, Cc = skip.shape
        dev = skip.device
        skip, branch = M.rows2d(skip), M.rows2d(branch)
        pre_w, pre_b, post_w, post_b = _param(pre_kind, pre_w), _param(pre_kind, pre_b), _param(post_kind, post_w), _param(post_kind, post_b)
        if keep is not None:
            keep = keep.contiguous()
        with torch.cuda.device(dev):
            y = torch.empty(N, Cc, dtype=y_dtype, device=dev)
            n = torch.empty(N, Cc, dtype=n_dtype, device=dev) if post_kind != L.GDR_BLOCK_NORM_NONE else None
            pre, post = _desc(pre_kind, pre_w, pre_b, pre_eps), _desc(post_kind, post_w, post_b, post_eps)
            L.check(L.load().gdr_block_junction_forward(
                skip.data_ptr(), M.stride0(skip), _DTYPES[skip.dtype], branch.data_ptr(), M.stride0(branch), _DTYPES[branch.dtype],
                M.ptr(keep), _DTYPES[keep.dtype] if keep is not None else 0, pre, post, M.ptr(offset), N, B, Cc, _DTYPES[b0_dtype],
                _DTYPES[kb_dtype], y.data_ptr(), _DTYPES[y_dtype], M.ptr(n), _DTYPES[n_dtype], M.stream()), "gdr_block_junction_forward")
        ctx.save_for_backward(skip, branch, keep, pre_w, pre_b, post_w, post_b, offset)
        ctx.set_materialize_grads(False)      # a None upstream gradient stays None: the kernel reads it as zeros
        ctx.meta = meta
        if n is None:
            return y, None
        return y, n

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y, grad_n):
        skip, branch, keep, pre_w, pre_b, post_w, post_b, offset = ctx.saved_tensors
        pre_kind, pre_eps, post_kind, post_eps, b0_dtype, kb_dtype, y_dtype, n_dtype, B = ctx.meta
        N, Cc = skip.shape
        dev = skip.device
        need = ctx.needs_input_grad
        if grad_y is None and grad_n is None:
            return (None,) * 9
        grad_y = None if grad_y is None else M.rows2d(grad_y)
        grad_n = None if grad_n is None else M.rows2d(grad_n)
        with torch.cuda.device(dev):
            grad_skip = torch.empty_like(skip) if need[0] else None
            grad_branch = torch.empty_like(branch) if need[1] else None
            grads = [torch.empty_like(t) if t is not None and need[i] else None
                     for i, t in ((3, pre_w), (4, pre_b), (5, post_w), (6, post_b))]
            if need[0] or need[1] or any(g is not None for g in grads):
                lib = L.load()
                nbytes = lib.gdr_block_junction_backward_bytes(N, B, Cc)
                if nbytes == 0:
                    L.check(-1, "gdr_block_junction_backward_bytes")
                ws, base, usable = M.workspace(nbytes, dev)
                pre = _desc(pre_kind, pre_w, pre_b, pre_eps, grads[0], grads[1])
                post = _desc(post_kind, post_w, post_b, post_eps, grads[2], grads[3])
                L.check(lib.gdr_block_junction_backward(
                    M.ptr(grad_y), M.stride0(grad_y) if grad_y is not None else 0, _DTYPES[grad_y.dtype] if grad_y is not None else 0,
                    M.ptr(grad_n), M.stride0(grad_n) if grad_n is not None else 0, _DTYPES[grad_n.dtype] if grad_n is not None else 0,
                    skip.data_ptr(), M.stride0(skip), _DTYPES[skip.dtype], branch.data_ptr(), M.stride0(branch), _DTYPES[branch.dtype],
                    M.ptr(keep), _DTYPES[keep.dtype] if keep is not None else 0, pre, post, M.ptr(offset), N, B, Cc, _DTYPES[b0_dtype],
                    _DTYPES[kb_dtype], _DTYPES[y_dtype], base, usable, M.ptr(grad_skip), M.ptr(grad_branch), M.stream()),
                    "gdr_block_junction_backward")
        return (grad_skip, grad_branch, None, *grads, None, None)


def junction(skip, branch, keep=None, pre=None, post=None, offset=None):
    """skip, branch (N, C), keep (N,) / (N, 1) or None, pre / post norm specs, offset (B,) integer segment ends on the device
    (needed by an 'ada' norm) -> (y (N, C), n (N, C) or None): y = skip + keep * pre(branch), n = post(y)."""
    M.check_float("skip", skip, 2)
    M.check_float("branch", branch, 2)
    if keep is not None:
        if not isinstance(keep, torch.Tensor):
            raise TypeError(f"keep must be a tensor or None, not {type(keep).__name__}")
        if keep.dtype not in _DTYPES:
            raise TypeError(f"keep must be float32, float16 or bfloat16, not {keep.dtype}")
    N, Cc = skip.shape
    pre_kind, pre_w, pre_b, pre_eps = _check_spec("pre", pre, Cc)
    post_kind, post_w, post_b, post_eps = _check_spec("post", post, Cc)
    ada = [w for k, w in ((pre_kind, pre_w), (post_kind, post_w)) if k == L.GDR_BLOCK_NORM_ADA]
    B = 1
    if ada:
        if not isinstance(offset, torch.Tensor):
            raise TypeError(f"an 'ada' norm needs offset as a tensor, not {type(offset).__name__}")
        if offset.dtype.is_floating_point or offset.dtype.is_complex or offset.dtype == torch.bool:
            raise TypeError(f"offset must be an integer tensor, not {offset.dtype}")
        B = ada[0].shape[0]
        if offset.dim() != 1 or offset.shape[0] != B or any(w.shape[0] != B for w in ada):
            raise ValueError(f"offset must be (B,) for scale (B, {Cc}), got {tuple(offset.shape)} and {[tuple(w.shape) for w in ada]}")
        if not 1 <= B <= MAX_SEGMENTS:
            raise ValueError(f"{B} segments are outside the envelope 1..{MAX_SEGMENTS}")
    else:
        offset = None
    if branch.shape != (N, Cc):
        raise ValueError(f"skip {tuple(skip.shape)} needs branch ({N}, {Cc}), got {tuple(branch.shape)}")
    if keep is not None:
        if keep.shape not in ((N,), (N, 1)):
            raise ValueError(f"keep must be ({N},) or ({N}, 1), got {tuple(keep.shape)}")
        keep = keep.detach().reshape(N)
    _norm._check_channels(Cc)
    if N > MAX_ROWS:
        raise ValueError("more than 2^31 - 1 rows")
    named = [("skip", skip), ("branch", branch)] + [(n, t) for n, t in (("keep", keep), ("pre weight", pre_w), ("pre bias", pre_b),
                                                                       ("post weight", post_w), ("post bias", post_b),
                                                                       ("offset", offset)) if t is not None]
    M.check_devices(tuple(named), _NO_CPU)
    b0_dtype = _norm_dtype(pre_kind, pre_w, branch.dtype)
    kb_dtype = b0_dtype if keep is None else torch.promote_types(b0_dtype, keep.dtype)
    y_dtype = torch.promote_types(skip.dtype, kb_dtype)
    n_dtype = _norm_dtype(post_kind, post_w, y_dtype)
    if N == 0:
        return skip.new_empty((0, Cc), dtype=y_dtype), (skip.new_empty((0, Cc), dtype=n_dtype) if post_kind != L.GDR_BLOCK_NORM_NONE else None)
    meta = (pre_kind, pre_eps, post_kind, post_eps, b0_dtype, kb_dtype, y_dtype, n_dtype, B)
    with torch.autocast("cuda", enabled=False):
        return _Junction.apply(skip, branch, keep, pre_w, pre_b, post_w, post_b, None if offset is None else offset.long().contiguous(), meta)


# ---- the module forward ---------------------------------------------------------------------------------------------------

def _is_ada(m):
    return isinstance(m, nn.LayerNorm) and not m.elementwise_affine and isinstance(getattr(m, "affine", None), nn.Linear)


def _is_norm(m, C):
    return (type(m) is nn.LayerNorm or _is_ada(m)) and tuple(m.normalized_shape) == (C,)


def covers(module):
    """whether `module` is the layer list served: cpe = (SubMConv3d, nn.Linear, norm), norm1 and norm2 one norm each, a norm
    exactly nn.LayerNorm over (C,) or an nn.LayerNorm without affine that has an `affine` Linear child, mlp[0] = fc1, GELU,
    fc2, every nn.Dropout with p = 0, pre_norm true"""
    import spconv.pytorch as spconv

    if not getattr(module, "pre_norm", False) or not isinstance(getattr(module, "channels", None), int):
        return False
    Cc = module.channels
    try:
        cpe, norm1, norm2, mlp, drop_path = module.cpe, module.norm1, module.norm2, module.mlp, module.drop_path
        if (len(cpe), len(norm1), len(norm2), len(mlp), len(drop_path)) != (3, 1, 1, 1, 1):
            return False
        conv, lin, norms, ff = cpe[0], cpe[1], (cpe[2], norm1[0], norm2[0]), mlp[0]
        module.attn, drop_path[0]
    except (AttributeError, IndexError, KeyError, TypeError):
        return False
    if not isinstance(conv, spconv.SubMConv3d) or type(lin) is not nn.Linear or lin.out_features != Cc:
        return False
    if not all(_is_norm(m, Cc) for m in norms):
        return False
    if not (type(getattr(ff, "fc1", None)) is nn.Linear and type(getattr(ff, "act", None)) is nn.GELU
            and type(getattr(ff, "fc2", None)) is nn.Linear and ff.fc2.out_features == Cc):
        return False
    # every nn.Dropout below `module`.  The walk runs on every forward (a verdict kept per module would go stale when a child is
    # replaced), so it reads the child tables directly: module.modules() builds a dotted name per node and took 70 % of covers
    stack = [module]
    while stack:
        m = stack.pop()
        if m is None:
            continue
        if isinstance(m, nn.Dropout) and m.p != 0:
            return False
        stack.extend(m._modules.values())
    return True


def _spec(m, point):
    if _is_ada(m):
        return ("ada", m.affine(point.global_feat), m.eps)
    return ("ln", m.weight, m.bias, m.eps)


def _serves(self, point):
    feat, offset = point.feat, point.offset
    if not isinstance(feat, torch.Tensor) or not isinstance(offset, torch.Tensor) or feat.dim() != 2 or offset.dim() != 1:
        return False
    if not (feat.is_cuda and offset.is_cuda) or feat.dtype not in _DTYPES or feat.shape[1] != self.channels:
        return False
    B = 1
    if any(_is_ada(m) for m in (self.cpe[2], self.norm1[0], self.norm2[0])):
        g = point.get("global_feat") if hasattr(point, "get") else getattr(point, "global_feat", None)
        if not isinstance(g, torch.Tensor) or g.dim() != 2 or g.shape[0] != offset.shape[0] or g.device != feat.device:
            return False
        B = g.shape[0]
    return in_envelope(feat.shape[0], feat.shape[1], B)


def _reference_forward(self, point):
    """the reference's lines, over this repository's drop-ins"""
    if not self.cpe[0].training:
        self.cpe[0].train(True)
    shortcut = point.feat
    point = self.cpe(point)
    point.feat = shortcut + point.feat
    shortcut = point.feat
    if self.pre_norm:
        point = self.norm1(point)
    point = self.drop_path(self.attn(point))
    point.feat = shortcut + point.feat
    if not self.pre_norm:
        point = self.norm1(point)

    shortcut = point.feat
    if self.pre_norm:
        point = self.norm2(point)
    point = self.drop_path(self.mlp(point))
    point.feat = shortcut + point.feat
    if not self.pre_norm:
        point = self.norm2(point)
    point.sparse_conv_feat = point.sparse_conv_feat.replace_feature(point.feat)
    return point


def block_forward(self, point):
    """Block.forward of the reference.  Reads self.cpe, norm1, attn, norm2, mlp, drop_path, pre_norm, channels; reads
    point.feat, sparse_conv_feat, offset (global_feat with an AdaLayerNorm) and what self.attn reads; assigns point.feat and
    point.sparse_conv_feat."""
    if BLOCK_BACKEND not in ("torch", "hip"):
        raise ValueError(f"block.BLOCK_BACKEND must be 'torch' or 'hip', not {BLOCK_BACKEND!r}")
    if BLOCK_BACKEND != "hip" or not covers(self) or not _serves(self, point):
        return _reference_forward(self, point)
    if not self.cpe[0].training:
        self.cpe[0].train(True)
    offset, drop_path = point.offset, self.drop_path[0]
    sparse = self.cpe[0](point.sparse_conv_feat)
    y, n = junction(point.feat, self.cpe[1](sparse.features), None, _spec(self.cpe[2], point), _spec(self.norm1[0], point), offset)
    point.sparse_conv_feat = sparse
    point.feat = n
    branch = self.attn(point).feat
    y, n = junction(y, branch, _upscale._keep_tensor(drop_path, branch), None, _spec(self.norm2[0], point), offset)
    branch = self.mlp[0](n)
    y, _ = junction(y, branch, _upscale._keep_tensor(drop_path, branch), None, None, None)
    point.feat = y
    point.sparse_conv_feat = sparse.replace_feature(y)
    return point
