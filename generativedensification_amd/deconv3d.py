"""[LayerNorm +] 2x transposed convolution of channels-last volumes on the MI355X (csrc/deconv3d.hip, include/gdr.h
gdr_deconv3d_*): the `nn.LayerNorm(embed_dim, eps=1e-6)` and `nn.ConvTranspose3d(embed_dim, out_dim, kernel_size=2, stride=2)`
at the tail of the reference's `VolTransformer` (lightning/network.py), on volumes stored `channels_last_3d`, where a voxel is
one contiguous C-element row: what the bound blocks (groupattn.py, conv3d.py) hand on and what every later step reads.

    conv_transpose3d_2x(x, weight, bias=None, norm=None)       = F.conv_transpose3d(x, weight, bias, stride=2), with
                                                                 norm=(ln_weight, ln_bias, eps) of F.layer_norm over the channels
                                                                 of every voxel, in the same kernel
    conv_transpose3d_2x_of(deconv_module, x, norm_module=None) the same with the modules' parameters; refuses other settings
    covers(deconv_module, norm_module=None)                    whether the modules have the one set of settings served
    in_envelope(B, Cin, Cout, D, H, W)                         whether the kernels serve this shape
    vol_transformer_forward(self, image_feats)                 VolTransformer.forward with this tail; bound with one line,
                                                               network.VolTransformer.forward = deconv3d.vol_transformer_forward
    vol_transformer_forward_from_conds(self, conds, B)         the same behind its cond line, from the conds of volcond.volume_conds

x is (B, Cin, D, H, W), weight (Cin, Cout, 2, 2, 2) in nn.ConvTranspose3d's own layout, bias (Cout,) or None; the result is
(B, Cout, 2D, 2H, 2W) with dense channels_last_3d strides, so `out.permute(0, 2, 3, 4, 1)` is the reference's contiguous
`x_up` without a copy.  Kernel 2, stride 2, no padding: tap (i, j, k) of parent voxel (d, h, w) is child voxel
(2d + i, 2h + j, 2w + k) and nothing overlaps, so the layer is one GEMM.  Either affine tensor of `norm` may be None.

Layout: a dense channels_last_3d x with a 16-byte aligned base is read in place (a stride of a size-1 axis is never looked
at); anything else (NCDHW-contiguous, a channel slice, an unaligned base) is made so with one copy.
Dtypes: x is float32, float16 or bfloat16 and its dtype is the compute dtype; the parameters may each be any of the three.
weight and bias are rounded to the compute dtype by the pack kernel and in the epilogue (what autocast's cast does, without a
tensor of the rounded parameter); the LayerNorm's affine parameters are read as they are.  Sums are float32 (float64 for
float32 rows, whose normalised value is never rounded); the result and grad_x have x's dtype; parameter gradients come back in
the parameters' dtypes, rounded once.
Autocast: torch's rule for conv_transpose3d.  Under an enabled CUDA autocast a float32 x is first cast to the autocast dtype;
the Function itself runs with autocast disabled.  With `norm` the normalised row is computed in float32 from the row as
stored and rounded once to the compute dtype on its way into the MFMA operand: where the reference's composition rounds
under bf16 autocast (its LayerNorm returns float32 and the convolution's cast rounds it).
Autograd: once differentiable; x's rows, the weight, the affine parameters and two float64 per row of statistics are saved; a
gradient nobody needs is not launched (a frozen weight launches no weight gradient).  Works under no_grad and
torch.autograd.functional.vjp.
The kernels use no atomics (two calls are bitwise equal) and never synchronise with the host.  GPU tensors only (no CPU
fallback).  Wrong dtypes raise TypeError, shapes outside the envelope ValueError, all before any launch.  Envelope: Cin a
multiple of 8 in 8..MAX_CIN, Cout one in 8..MAX_COUT, D, H, W >= 1, B D H W <= MAX_ROWS (8 B D H W child rows below 2^31).
B = 0 or an empty axis returns an empty tensor without loading the library.  Non-finite inputs are memory-safe and otherwise
unspecified.
"""
from __future__ import annotations

import torch

from . import _lib as L
from . import _marshal as M

__all__ = ["conv_transpose3d_2x", "conv_transpose3d_2x_of", "covers", "in_envelope", "vol_transformer_forward",
           "vol_transformer_forward_from_conds", "TAIL_BACKEND", "MAX_CIN", "MAX_COUT", "MAX_ROWS", "TILE_ROWS", "GRAD_WEIGHT_SLAB_ROWS"]

MAX_CIN, MAX_COUT = L.GDR_DECONV3D_MAX_CIN, L.GDR_DECONV3D_MAX_COUT
MAX_ROWS = ((1 << 31) - 1) // 8     # parent voxels
TILE_ROWS = L.GDR_DECONV3D_TILE_ROWS                  # parent rows of one workgroup of the forward
GRAD_WEIGHT_SLAB_ROWS = L.GDR_DECONV3D_SLAB_MIN       # the weight gradient cuts one slab of parent rows per this many, 8 at most

# the tail of vol_transformer_forward: "hip" (this module wherever it covers the modules and the shape) or "torch" (the
# reference's four lines, on purpose: the A/B of scripts/bench_deconv3d.py)
TAIL_BACKEND = "hip"

_DTYPES = M.DTYPES
_dense = M.dense
_NO_CPU = "the HIP transposed convolution runs on ROCm/HIP tensors only (no CPU fallback)"


def in_envelope(B, Cin, Cout, D, H, W):
    """whether the kernels serve this shape"""
    return (8 <= Cin <= MAX_CIN and Cin % 8 == 0 and 8 <= Cout <= MAX_COUT and Cout % 8 == 0 and B >= 0 and min(D, H, W) >= 1
            and B * D * H * W <= MAX_ROWS)


def _rows(x):
    """x (B, C, D, H, W) as its (B, D, H, W, C) rows, dense from a 16-byte aligned base: a view of a channels_last_3d x (the
    strides of size-1 axes do not count), one copy of anything else"""
    return M.dense_aligned(x.permute(0, 2, 3, 4, 1))


def _workspace(lib, what, dt, rows, cin, cout, dev):
    return M.queried_workspace(lib.gdr_deconv3d_workspace_bytes, "gdr_deconv3d_workspace_bytes", dev, what, dt, rows, cin, cout)


def _dt(t, default):
    return default if t is None else _DTYPES[t.dtype]


def _packed(lib, w, transposed, dt, dev):
    cin, cout = w.shape[:2]
    ws, base, _ = _workspace(lib, L.GDR_DECONV3D_WS_PACKED, dt, 0, cin, cout, dev)
    L.check(lib.gdr_deconv3d_pack_weight(w.data_ptr(), _DTYPES[w.dtype], cin, cout, int(transposed), base, dt, M.stream()),
            "gdr_deconv3d_pack_weight")
    return ws, base


class _Deconv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, ln_w, ln_b, norm_eps):
        dev = x.device
        rows = _rows(x)
        B, D, H, W, cin = rows.shape
        cout = weight.shape[1]
        has_norm = norm_eps is not None
        w, b, lw, lb = _dense(weight), _dense(bias), _dense(ln_w), _dense(ln_b)
        n = B * D * H * W
        stats = None
        with torch.cuda.device(dev):
            out = torch.empty(B, 2 * D, 2 * H, 2 * W, cout, dtype=x.dtype, device=dev)
            if n:
                lib, dt = L.load(), _DTYPES[x.dtype]
                if has_norm and any(ctx.needs_input_grad):
                    stats = torch.empty(n, 2, dtype=torch.float64, device=dev)
                ws, base = _packed(lib, w, False, dt, dev)
                L.check(lib.gdr_deconv3d_forward(rows.data_ptr(), dt, base, M.ptr(b), _dt(b, dt), int(has_norm), M.ptr(lw), _dt(lw, dt),
                                                 M.ptr(lb), _dt(lb, dt), float(norm_eps or 0.0), B, D, H, W, cin, cout, M.ptr(stats),
                                                 out.data_ptr(), M.stream()), "gdr_deconv3d_forward")
        ctx.save_for_backward(rows, w, lw, lb, stats)
        ctx.has_norm = has_norm
        ctx.meta = [None if t is None else (t.dtype, t.shape) for t in (bias, ln_w, ln_b)]
        return out.permute(0, 4, 1, 2, 3)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        rows, w, lw, lb, stats = ctx.saved_tensors
        B, D, H, W, cin = rows.shape
        cout, dev, dt = w.shape[1], rows.device, _DTYPES[rows.dtype]
        need = ctx.needs_input_grad
        need_x, need_w = need[0], need[1]
        need_b, need_lw, need_lb = (ctx.meta[i] is not None and need[2 + i] for i in range(3))
        if grad_out.dtype != rows.dtype:
            grad_out = grad_out.to(rows.dtype)
        g = _rows(grad_out)
        n = B * D * H * W
        has_norm = ctx.has_norm

        def parameter_grad(meta):
            return (torch.zeros if not n else torch.empty)(meta[1], dtype=meta[0], device=dev)

        grad_x = grad_w = grad_b = grad_lw = grad_lb = None
        with torch.cuda.device(dev):
            lib = L.load() if n else None
            if need_x or need_lw or need_lb:
                grad_rows = torch.empty_like(rows) if need_x else None
                grad_lw = parameter_grad(ctx.meta[1]) if need_lw else None
                grad_lb = parameter_grad(ctx.meta[2]) if need_lb else None
                if n:
                    pws, pbase = _packed(lib, w, True, dt, dev)
                    ws, base, usable = (_workspace(lib, L.GDR_DECONV3D_WS_GRAD_INPUT, dt, n, cin, cout, dev) if need_lw or need_lb
                                        else (None, None, 0))
                    L.check(lib.gdr_deconv3d_grad_input(g.data_ptr(), dt, pbase, rows.data_ptr(), M.ptr(stats), int(has_norm), M.ptr(lw),
                                                        _dt(lw, dt), B, D, H, W, cin, cout, base, usable, M.ptr(grad_rows), M.ptr(grad_lw),
                                                        _dt(grad_lw, dt), M.ptr(grad_lb), _dt(grad_lb, dt), M.stream()),
                            "gdr_deconv3d_grad_input")
                if need_x:
                    grad_x = grad_rows.permute(0, 4, 1, 2, 3)
            if need_w:
                grad_w = torch.zeros_like(w) if not n else torch.empty_like(w)
                if n:
                    ws, base, usable = _workspace(lib, L.GDR_DECONV3D_WS_GRAD_WEIGHT, dt, n, cin, cout, dev)
                    L.check(lib.gdr_deconv3d_grad_weight(rows.data_ptr(), M.ptr(stats), int(has_norm), M.ptr(lw), _dt(lw, dt), M.ptr(lb),
                                                         _dt(lb, dt), g.data_ptr(), dt, B, D, H, W, cin, cout, base, usable,
                                                         grad_w.data_ptr(), _DTYPES[w.dtype], M.stream()), "gdr_deconv3d_grad_weight")
            if need_b:
                grad_b = parameter_grad(ctx.meta[0])
                if n:
                    ws, base, usable = _workspace(lib, L.GDR_DECONV3D_WS_GRAD_BIAS, dt, n, cin, cout, dev)
                    L.check(lib.gdr_deconv3d_grad_bias(g.data_ptr(), dt, 8 * n, cout, base, usable, grad_b.data_ptr(), _DTYPES[grad_b.dtype],
                                                       M.stream()), "gdr_deconv3d_grad_bias")
        return grad_x, grad_w, grad_b, grad_lw, grad_lb, None


def _check(x, weight, bias, norm):
    ln_w, ln_b, eps = norm if norm is not None else (None, None, None)
    named = [("x", x), ("weight", weight)] + [(name, t) for name, t in (("bias", bias), ("ln_weight", ln_w), ("ln_bias", ln_b)) if t is not None]
    for name, t in named:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, not {type(t).__name__}")
        if t.dtype not in _DTYPES:
            raise TypeError(f"{name} must be float32, float16 or bfloat16, not {t.dtype}")
    if norm is not None and (isinstance(eps, bool) or not isinstance(eps, (int, float))):
        raise TypeError(f"norm is (ln_weight, ln_bias, eps) with a number for eps, not {type(eps).__name__}")
    if x.dim() != 5:
        raise ValueError(f"x is (B, Cin, D, H, W), got {tuple(x.shape)}")
    B, cin, D, H, W = x.shape
    if weight.dim() != 5 or weight.shape[0] != cin or weight.shape[2:] != (2, 2, 2):
        raise ValueError(f"x {tuple(x.shape)} needs a weight ({cin}, Cout, 2, 2, 2), got {tuple(weight.shape)}")
    cout = weight.shape[1]
    for name, t, c in (("bias", bias, cout), ("ln_weight", ln_w, cin), ("ln_bias", ln_b, cin)):
        if t is not None and t.shape != (c,):
            raise ValueError(f"{name} must have {c} elements, got {tuple(t.shape)}")
    if norm is not None and not eps >= 0:
        raise ValueError(f"eps must be >= 0, got {eps}")
    for name, c, top in (("Cin", cin, MAX_CIN), ("Cout", cout, MAX_COUT)):
        if c < 8 or c > top or c % 8:
            raise ValueError(f"{name} = {c} is outside the envelope: a multiple of 8 in 8..{top}")
    if B * D * H * W > MAX_ROWS:
        raise ValueError("more than 2^31 - 1 child voxels")
    for name, t in named:
        if not t.is_cuda:
            raise RuntimeError(_NO_CPU)
    for name, t in named:
        if t.device != x.device:
            raise RuntimeError(f"{name} must live on x's device ({x.device}), not {t.device}")


def conv_transpose3d_2x(x, weight, bias=None, norm=None):
    """x (B, Cin, D, H, W), weight (Cin, Cout, 2, 2, 2), bias (Cout,) or None -> F.conv_transpose3d(x, weight, bias, stride=2) as a
    (B, Cout, 2D, 2H, 2W) tensor of x's dtype with channels_last_3d strides; norm = (ln_weight, ln_bias, eps): of
    F.layer_norm over the channels of every voxel of x first, in the same kernel (either affine tensor may be None)."""
    norm = tuple(norm) if norm is not None else None
    if norm is not None and len(norm) != 3:
        raise ValueError("norm is (ln_weight, ln_bias, eps)")
    _check(x, weight, bias, norm)
    ln_w, ln_b, eps = norm if norm is not None else (None, None, None)
    if x.dtype == torch.float32 and torch.is_autocast_enabled("cuda"):
        x = x.to(torch.get_autocast_dtype("cuda"))
    with torch.autocast("cuda", enabled=False):
        return _Deconv.apply(x, weight, bias, ln_w, ln_b, None if norm is None else float(eps))


def _triple(v):
    return (v,) * 3 if isinstance(v, int) else tuple(v)


def covers(deconv_module, norm_module=None):
    """whether `deconv_module` is an nn.ConvTranspose3d with the one set of settings the kernels implement and `norm_module`
    (if given) an nn.LayerNorm over exactly its input channels"""
    m = deconv_module
    ok = (isinstance(m, torch.nn.ConvTranspose3d) and _triple(m.kernel_size) == (2, 2, 2) and _triple(m.stride) == (2, 2, 2)
          and _triple(m.padding) == (0, 0, 0) and _triple(m.output_padding) == (0, 0, 0) and _triple(m.dilation) == (1, 1, 1)
          and m.groups == 1)
    if ok and norm_module is not None:
        ok = isinstance(norm_module, torch.nn.LayerNorm) and tuple(norm_module.normalized_shape) == (m.in_channels,)
    return ok


def conv_transpose3d_2x_of(deconv_module, x, norm_module=None):
    """`deconv_module(x)` for an nn.ConvTranspose3d(Cin, Cout, kernel_size=2, stride=2) through the HIP kernels, of
    `norm_module` (an nn.LayerNorm(Cin)) over the channels of every voxel first if given; any other kernel size, stride,
    padding, output padding, dilation or groups, or another normalized_shape, raises NotImplementedError."""
    if not covers(deconv_module, norm_module):
        raise NotImplementedError("the HIP transposed convolution covers nn.ConvTranspose3d with kernel_size 2, stride 2, padding 0, "
                                  "output_padding 0, dilation 1 and groups 1, and an nn.LayerNorm over its input channels only, got "
                                  f"{deconv_module!r} and {norm_module!r}")
    norm = None if norm_module is None else (norm_module.weight, norm_module.bias, norm_module.eps)
    return conv_transpose3d_2x(x, deconv_module.weight, deconv_module.bias, norm)


def _cond(image_feats, n_group, block_size):
    """the cond of the blocks of one group size, (B g^3, V bs^3, C), from image_feats (B, V, C, D, H, W): the reference's
    unfold / contiguous / einsum / reshape with ONE permuting copy; the same values bit for bit"""
    B, V, C = image_feats.shape[:3]
    blocks = image_feats.unfold(3, block_size, block_size).unfold(4, block_size, block_size).unfold(5, block_size, block_size)
    # (B, V, C, g, g, g, z, y, x) -> (B, g, g, g, V, z, y, x, C)
    return blocks.permute(0, 3, 4, 5, 1, 6, 7, 8, 2).reshape(B * n_group ** 3, block_size ** 3 * V, C)


def vol_transformer_forward(self, image_feats):
    """VolTransformer.forward of the reference (lightning/network.py): reads self.n_groups, block_size, pos_embed, layers, norm
    and deconv and returns the reference's contiguous (B, 2D, 2H, 2W, out_dim) tensor.  Each cond is built with one permuting
    copy, the initial volume is the broadcast pos_embed written once as channels_last_3d (so a bound block reads it in
    place), the layers are called as the reference calls them, and the LayerNorm + ConvTranspose3d tail is one launch of
    csrc/deconv3d.hip wherever `covers` and `in_envelope` hold and TAIL_BACKEND is "hip"; anywhere else it is the reference's
    four lines."""
    if TAIL_BACKEND not in ("torch", "hip"):
        raise ValueError(f"deconv3d.TAIL_BACKEND must be 'torch' or 'hip', not {TAIL_BACKEND!r}")
    B, V, C, D, H, W = image_feats.shape
    volume_feats = [_cond(image_feats, n_group, D // n_group) for n_group in self.n_groups]
    # the rows (B, d, h, w, E) of pos_embed repeated over the batch, one copy; seen as (B, E, d, h, w)
    x = self.pos_embed.expand(B, -1, -1, -1, -1).permute(0, 2, 3, 4, 1).clone(memory_format=torch.contiguous_format).permute(0, 4, 1, 2, 3)
    for i, layer in enumerate(self.layers):
        group_idx = i % len(self.block_size)
        x = layer(x, volume_feats[group_idx], self.n_groups[group_idx], self.block_size[group_idx])
    if (TAIL_BACKEND == "hip" and covers(self.deconv, self.norm)
            and in_envelope(x.shape[0], self.deconv.in_channels, self.deconv.out_channels, *x.shape[2:])):
        return conv_transpose3d_2x_of(self.deconv, x, self.norm).permute(0, 2, 3, 4, 1)
    x = self.norm(torch.einsum('bcdhw->bdhwc', x))
    x = torch.einsum('bdhwc->bcdhw', x)
    x_up = self.deconv(x)
    return torch.einsum('bcdhw->bdhwc', x_up).contiguous()


def vol_transformer_forward_from_conds(self, conds, B):
    """vol_transformer_forward behind its cond line (the same lines, restated: that function stays as it is): `conds` holds one
    (B g^3, V bs^3, C) cond per entry of self.n_groups (what volcond.volume_conds returns) and B is the batch size."""
    if TAIL_BACKEND not in ("torch", "hip"):
        raise ValueError(f"deconv3d.TAIL_BACKEND must be 'torch' or 'hip', not {TAIL_BACKEND!r}")
    volume_feats = list(conds)
    if len(volume_feats) != len(self.n_groups):
        raise ValueError(f"{len(self.n_groups)} group sizes need as many conds, got {len(volume_feats)}")
    # the rows (B, d, h, w, E) of pos_embed repeated over the batch, one copy; seen as (B, E, d, h, w)
    x = self.pos_embed.expand(B, -1, -1, -1, -1).permute(0, 2, 3, 4, 1).clone(memory_format=torch.contiguous_format).permute(0, 4, 1, 2, 3)
    for i, layer in enumerate(self.layers):
        group_idx = i % len(self.block_size)
        x = layer(x, volume_feats[group_idx], self.n_groups[group_idx], self.block_size[group_idx])
    if (TAIL_BACKEND == "hip" and covers(self.deconv, self.norm)
            and in_envelope(x.shape[0], self.deconv.in_channels, self.deconv.out_channels, *x.shape[2:])):
        return conv_transpose3d_2x_of(self.deconv, x, self.norm).permute(0, 2, 3, 4, 1)
    x = self.norm(torch.einsum('bcdhw->bdhwc', x))
    x = torch.einsum('bdhwc->bcdhw', x)
    x_up = self.deconv(x)
    return torch.einsum('bcdhw->bdhwc', x_up).contiguous()
