"""The torch glue of the point decoder's UpscaleModule / UpscaleResModule on either side of its Linears, on the MI355X
(csrc/upscale.hip, include/gdr.h gdr_upscale_*; reference lightning/point_decoder/autoencoder.py, UpscaleModule.forward).  The
five `nn.Linear` products stay torch's; what is fused is what lies between them.

`expand(t, coord, feat, frequencies, upscale_factor, grid_size, absolute_pe=False, eps=1e-5) -> (out_x, h)`: from
`t = delta_x(in_f)` (N, 3 S) to the child coordinates (N S, 3) and the input of `delta_f` (N S, 6 F + C), one launch.  For
parent p, child s, axis j, with rd the rounding to t's dtype:  u = rd(tanh(t[p, 3 s + j])), d = rd((0.5 * grid_size) * u),
out_x[p S + s, j] = coord[p, j] + d in the promotion of the two dtypes, and h[p S + s] is what `norm.pe_concat_layer_norm`
returns for x = d (x = out_x with `absolute_pe`) and feat: the same kernel source, the same column order, padded row stride and
result dtype.  No gather_csr, no temp_offset, no (rows, 3) or (rows, C) temporary.

`merge(skip, branch, keep, scale, offset, upscale_factor, eps=1e-5) -> out` (N S, Cout): the skip row, the drop-path branch and
`out_norm` in one launch.  skip (N, Cout) = self.skip(in_f) on the PARENTS, branch (N S, Cout) = delta_f, keep (N S,) / (N S, 1)
or None the tensor drop_path multiplies by, scale (B, Cout) = out_norm.affine(global_feat), offset (B,) the parents' segment ends
(read on the device).  y[r] = rd(skip[r // S] + rd(keep[r] * branch[r])), out[r] = scale[seg(r)] * layer_norm(y[r]) by
`norm.ada_layer_norm`'s rules (rows at or behind offset[-1] * S are zero, an empty segment is legal).

Both compute in fp32 from f32 / f16 / bf16 inputs (each input's dtype is independent), recompute their statistics in a
one-launch backward (merge: plus ada's fold for grad_scale), use no atomics (two calls are bitwise equal), store no gradient
nobody needs, never synchronise with the host and run with autocast switched off inside (result dtypes: `norm._result_dtype`).
GPU tensors only.  Envelope: norm's — C and Cout multiples of 8 in 8..1024, 1 <= F <= 16, 1 <= S <= 16, 1 <= B <= 1024, N and
N S below 2^31; N = 0 returns empty tensors without loading the library.

`upscale_module_forward` / `upscale_res_module_forward` are forwards to bind onto the reference's classes
(`autoencoder.UpscaleModule.forward = upscale_module_forward`): under UPSCALE_BACKEND = "hip", wherever `covers` and
`in_envelope` hold, the sequence in_norm, delta_x, expand, delta_f[1:], skip on the parents, the drop-path draw (the
reference's own, so a seeded run stays aligned), merge; anywhere else the reference's lines.
"""
from __future__ import annotations

import torch
from torch import nn

from . import _lib as L
from . import _marshal as M
from . import norm as _norm

__all__ = ["expand", "merge", "covers", "in_envelope", "upscale_module_forward", "upscale_res_module_forward", "UPSCALE_BACKEND"]

# the path of the two bound forwards: "hip" (this module wherever it covers the module and the shape) or "torch" (the
# reference's lines over this repository's drop-ins).  "hip" is the default by the project's rule: under bf16 autocast forward +
# backward its median was lower and the ranges did not overlap at both base-config shapes (scripts/bench_upscale.py,
# BASELINE §4-upscale: 1.43 ms against 1.82 ms at 12 000 x 2, 1.58 ms against 2.58 ms at 19 200 x 4).
UPSCALE_BACKEND = "hip"

MAX_CHANNELS, MAX_SEGMENTS, MAX_FREQS, MAX_UPSCALE, MAX_ROWS = (_norm.MAX_CHANNELS, _norm.MAX_SEGMENTS, _norm.MAX_FREQS,
                                                              _norm.MAX_UPSCALE, _norm.MAX_ROWS)
_DTYPES = M.DTYPES
_rows = M.dense_aligned


def in_envelope(N, S, C, Cout, F, B):
    """whether the kernels serve this shape"""
    return (0 <= N and 1 <= S <= MAX_UPSCALE and N * S <= MAX_ROWS and 1 <= F <= MAX_FREQS and 1 <= B <= MAX_SEGMENTS
            and all(8 <= c <= MAX_CHANNELS and c % 8 == 0 for c in (C, Cout)))


def _check_upscale(S):
    if not 1 <= S <= MAX_UPSCALE:
        raise ValueError(f"upscale_factor {S} is outside the envelope 1..{MAX_UPSCALE}")


# ---- expand ---------------------------------------------------------------------------------------------------------------

class _Expand(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, coord, feat, frequencies, S, half_grid, absolute, eps, x_dtype, h_dtype):
        N, C = feat.shape
        F, dev = frequencies.shape[0], feat.device
        W = 6 * F + C
        t, coord, feat, frequencies = t.contiguous(), coord.contiguous(), _rows(feat), frequencies.contiguous()
        with torch.cuda.device(dev):
            out_x = torch.empty(N * S, 3, dtype=x_dtype, device=dev)
            buf = torch.empty(N * S, (W + 7) // 8 * 8, dtype=h_dtype, device=dev)
            L.check(L.load().gdr_upscale_expand_forward(
                t.data_ptr(), _DTYPES[t.dtype], coord.data_ptr(), _DTYPES[coord.dtype], feat.data_ptr(), C, _DTYPES[feat.dtype],
                frequencies.data_ptr(), _DTYPES[frequencies.dtype], N, S, C, F, half_grid, int(absolute), eps, out_x.data_ptr(),
                _DTYPES[x_dtype], buf.data_ptr(), buf.shape[1], _DTYPES[h_dtype], M.stream()), "gdr_upscale_expand_forward")
        ctx.save_for_backward(t, coord, feat, frequencies)
        ctx.set_materialize_grads(False)      # a None upstream gradient stays None: the kernel reads it as zeros
        ctx.meta = (S, half_grid, absolute, eps, x_dtype, h_dtype)
        return out_x, buf[:, :W]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_x, grad_h):
        t, coord, feat, frequencies = ctx.saved_tensors
        S, half_grid, absolute, eps, x_dtype, h_dtype = ctx.meta
        N, C = feat.shape
        F, dev = frequencies.shape[0], feat.device
        need_t, need_coord, need_feat = ctx.needs_input_grad[:3]
        if grad_h is not None and (grad_h.stride(1) != 1 or grad_h.stride(0) % 2 or grad_h.stride(0) < grad_h.shape[1]
                                   or grad_h.data_ptr() % (2 * grad_h.element_size())):
            grad_h = grad_h.contiguous()       # (a dense row of 6F + C elements is even)
        if grad_x is not None:
            grad_x = grad_x.contiguous()
        with torch.cuda.device(dev):
            grad_t = torch.empty_like(t) if need_t else None
            grad_coord = torch.empty_like(coord) if need_coord else None
            grad_feat = torch.empty(N, C, dtype=feat.dtype, device=dev) if need_feat else None
            if need_t or need_coord or need_feat:
                L.check(L.load().gdr_upscale_expand_backward(
                    M.ptr(grad_h), grad_h.stride(0) if grad_h is not None else 0, _DTYPES[grad_h.dtype if grad_h is not None else h_dtype],
                    M.ptr(grad_x), _DTYPES[x_dtype], t.data_ptr(), _DTYPES[t.dtype], coord.data_ptr(), _DTYPES[coord.dtype],
                    feat.data_ptr(), C, _DTYPES[feat.dtype], frequencies.data_ptr(), _DTYPES[frequencies.dtype], N, S, C, F, half_grid,
                    int(absolute), eps, M.ptr(grad_t), M.ptr(grad_coord), M.ptr(grad_feat), M.stream()), "gdr_upscale_expand_backward")
        return (grad_t, grad_coord, grad_feat) + (None,) * 7


def expand(t, coord, feat, frequencies, upscale_factor, grid_size, absolute_pe=False, eps=1e-5):
    """t (N, 3 S) = delta_x(in_f), coord (N, 3), feat (N, C), frequencies (F,) on the device, grid_size a Python float ->
    (out_x (N S, 3), h (N S, 6 F + C)): the child coordinates and layer_norm([sin(f x), cos(f x), feat of the parent]) without
    affine, x the offset (the child coordinate with absolute_pe)."""
    M.check_float("t", t, 2)
    M.check_float("coord", coord, 2)
    M.check_float("feat", feat, 2)
    M.check_float("frequencies", frequencies, 1)
    if isinstance(grid_size, torch.Tensor):
        raise TypeError("grid_size must be a Python number (a tensor would have to be read back)")
    S = int(upscale_factor)
    F = frequencies.shape[0]
    if F == 0:
        raise NotImplementedError("frequencies is empty: the raw-coordinate variant (n_frequencies = 0) is not implemented")
    if not 1 <= F <= MAX_FREQS:
        raise ValueError(f"{F} frequencies are outside the envelope 1..{MAX_FREQS}")
    _check_upscale(S)
    N, C = feat.shape
    _norm._check_channels(C)
    if t.shape != (N, 3 * S) or coord.shape != (N, 3):
        raise ValueError(f"feat {tuple(feat.shape)} and upscale_factor {S} need t ({N}, {3 * S}) and coord ({N}, 3), got "
                         f"{tuple(t.shape)} and {tuple(coord.shape)}")
    if N * S > MAX_ROWS:
        raise ValueError("more than 2^31 - 1 rows")
    M.check_devices((("feat", feat), ("t", t), ("coord", coord), ("frequencies", frequencies)), _norm._NO_CPU)
    x_dtype = torch.promote_types(coord.dtype, t.dtype)
    h_dtype = _norm._result_dtype(frequencies.dtype, x_dtype if absolute_pe else t.dtype, feat.dtype)
    if N == 0:
        return t.new_empty((0, 3), dtype=x_dtype), feat.new_empty((0, 6 * F + C), dtype=h_dtype)
    with torch.autocast("cuda", enabled=False):
        return _Expand.apply(t, coord, feat, frequencies, S, float(0.5 * grid_size), bool(absolute_pe), float(eps), x_dtype, h_dtype)


# ---- merge ----------------------------------------------------------------------------------------------------------------

class _Merge(torch.autograd.Function):
    @staticmethod
    def forward(ctx, skip, branch, keep, scale, offset, S, eps, out_dtype):
        N, C = skip.shape
        B, dev = scale.shape[0], skip.device
        skip, branch, scale = _rows(skip), _rows(branch), _rows(scale)
        if keep is not None:
            keep = keep.contiguous()
        with torch.cuda.device(dev):
            out = torch.empty(N * S, C, dtype=out_dtype, device=dev)
            L.check(L.load().gdr_upscale_merge_forward(
                skip.data_ptr(), C, _DTYPES[skip.dtype], branch.data_ptr(), C, _DTYPES[branch.dtype], M.ptr(keep),
                _DTYPES[keep.dtype] if keep is not None else 0, scale.data_ptr(), C, _DTYPES[scale.dtype], offset.data_ptr(), N, S, B, C,
                eps, out.data_ptr(), _DTYPES[out_dtype], M.stream()), "gdr_upscale_merge_forward")
        ctx.save_for_backward(skip, branch, keep, scale, offset)
        ctx.meta = (S, eps)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        skip, branch, keep, scale, offset = ctx.saved_tensors
        S, eps = ctx.meta
        N, C = skip.shape
        B, dev = scale.shape[0], skip.device
        need_skip, need_branch, _, need_scale = ctx.needs_input_grad[:4]
        grad_out = _rows(grad_out)
        with torch.cuda.device(dev):
            grad_skip = torch.empty_like(skip) if need_skip else None
            grad_branch = torch.empty_like(branch) if need_branch else None
            grad_scale = torch.empty_like(scale) if need_scale else None
            if need_skip or need_branch or need_scale:
                lib = L.load()
                nbytes = lib.gdr_upscale_merge_backward_bytes(N, S, B, C)
                if nbytes == 0:
                    L.check(-1, "gdr_upscale_merge_backward_bytes")
                ws, base, usable = M.workspace(nbytes, dev)
                L.check(lib.gdr_upscale_merge_backward(
                    grad_out.data_ptr(), C, _DTYPES[grad_out.dtype], skip.data_ptr(), C, _DTYPES[skip.dtype], branch.data_ptr(), C,
                    _DTYPES[branch.dtype], M.ptr(keep), _DTYPES[keep.dtype] if keep is not None else 0, scale.data_ptr(), C,
                    _DTYPES[scale.dtype], offset.data_ptr(), N, S, B, C, eps, base, usable, M.ptr(grad_skip), M.ptr(grad_branch),
                    M.ptr(grad_scale), M.stream()), "gdr_upscale_merge_backward")
        return grad_skip, grad_branch, None, grad_scale, None, None, None, None


def merge(skip, branch, keep, scale, offset, upscale_factor, eps=1e-5):
    """skip (N, C) on the parents, branch (N S, C), keep (N S,) / (N S, 1) or None, scale (B, C), offset (B,) the parents'
    integer segment ends on the device -> (N S, C): scale[b] * layer_norm(skip[r // S] + keep[r] * branch[r]); rows at or behind
    offset[-1] * S are zero."""
    M.check_float("skip", skip, 2)
    M.check_float("branch", branch, 2)
    M.check_float("scale", scale, 2)
    if keep is not None:
        if not isinstance(keep, torch.Tensor):
            raise TypeError(f"keep must be a tensor or None, not {type(keep).__name__}")
        if keep.dtype not in _DTYPES:
            raise TypeError(f"keep must be float32, float16 or bfloat16, not {keep.dtype}")
    if not isinstance(offset, torch.Tensor):
        raise TypeError(f"offset must be a tensor, not {type(offset).__name__}")
    if offset.dtype.is_floating_point or offset.dtype.is_complex or offset.dtype == torch.bool:
        raise TypeError(f"offset must be an integer tensor, not {offset.dtype}")
    S = int(upscale_factor)
    _check_upscale(S)
    N, C = skip.shape
    B = scale.shape[0]
    if branch.shape != (N * S, C) or scale.shape[1] != C or offset.dim() != 1 or offset.shape[0] != B:
        raise ValueError(f"skip {tuple(skip.shape)} and upscale_factor {S} need branch ({N * S}, {C}), scale (B, {C}) and offset (B,), "
                         f"got {tuple(branch.shape)}, {tuple(scale.shape)} and {tuple(offset.shape)}")
    if keep is not None:
        if keep.shape not in ((N * S,), (N * S, 1)):
            raise ValueError(f"keep must be ({N * S},) or ({N * S}, 1), got {tuple(keep.shape)}")
        keep = keep.detach().reshape(N * S)
    if not 1 <= B <= MAX_SEGMENTS:
        raise ValueError(f"{B} segments are outside the envelope 1..{MAX_SEGMENTS}")
    _norm._check_channels(C)
    if N * S > MAX_ROWS:
        raise ValueError("more than 2^31 - 1 rows")
    named = [("skip", skip), ("branch", branch), ("scale", scale), ("offset", offset)] + ([("keep", keep)] if keep is not None else [])
    M.check_devices(tuple(named), _norm._NO_CPU)
    out_dtype = _norm._result_dtype(torch.promote_types(skip.dtype, branch.dtype), scale.dtype)
    if N == 0:
        return branch.new_empty((0, C), dtype=out_dtype)
    with torch.autocast("cuda", enabled=False):
        return _Merge.apply(skip, branch, keep, scale, offset.long().contiguous(), S, float(eps), out_dtype)


# ---- the module forwards --------------------------------------------------------------------------------------------------

def _is_mlp(seq, kinds):
    return isinstance(seq, nn.Sequential) and len(seq) == len(kinds) and all(type(m) is k for m, k in zip(seq, kinds))


def covers(module):
    """whether `module` is the layer list served: delta_x Linear-GELU-Linear, delta_f LayerNorm(elementwise_affine=False)-
    Linear-GELU-Linear, out_norm[0] a LayerNorm without affine that has an `affine` Linear child, n_frequencies > 0"""
    if not _is_mlp(getattr(module, "delta_x", None), (nn.Linear, nn.GELU, nn.Linear)):
        return False
    delta_f = getattr(module, "delta_f", None)
    if not _is_mlp(delta_f, (nn.LayerNorm, nn.Linear, nn.GELU, nn.Linear)) or delta_f[0].elementwise_affine:
        return False
    if not isinstance(getattr(module, "skip", None), nn.Linear) or getattr(module, "n_frequencies", 0) <= 0:
        return False
    try:
        an = module.out_norm[0]
        single = len(module.out_norm) == 1
    except (AttributeError, IndexError, KeyError, TypeError):
        return False
    if not single or not isinstance(an, nn.LayerNorm) or an.elementwise_affine or not isinstance(getattr(an, "affine", None), nn.Linear):
        return False
    return isinstance(getattr(module, "frequencies", None), torch.Tensor) and module.frequencies.dim() == 1


def _keep_tensor(drop_path, branch):
    """the tensor drop_path multiplies `branch` by, drawn exactly as the reference's DropPath draws it, or None where it is
    the identity"""
    prob = getattr(drop_path, "drop_prob", 0.0)
    if not prob or not drop_path.training:
        return None
    keep_prob = 1 - prob
    keep = branch.new_empty((branch.shape[0], 1)).bernoulli_(keep_prob)
    if keep_prob > 0.0 and getattr(drop_path, "scale_by_keep", True):
        keep.div_(keep_prob)
    return keep


def _reference_tail(self, point, res):
    """the reference's lines behind in_norm, over this repository's torch_scatter drop-in"""
    import torch_scatter

    in_x, in_f = point.coord, point.feat
    N = len(in_x)
    temp_offset = torch.arange(N + 1, dtype=torch.int64, device=in_x.device) * self.upscale_factor
    skip_x = torch_scatter.gather_csr(in_x, temp_offset)
    skip_f = torch_scatter.gather_csr(in_f, temp_offset)
    delta_x = self.delta_x(in_f).reshape(N * self.upscale_factor, 3)
    delta_x = 0.5 * point.grid_size * torch.tanh(delta_x)
    if self.n_frequencies > 0:
        x = skip_x + delta_x if self.enable_absolute_pe else delta_x
        fx = torch.flatten(self.frequencies[None, :, None] * x[:, None, :], -2, -1)
        _delta_x = torch.cat([torch.sin(fx), torch.cos(fx)], dim=-1)
    else:
        _delta_x = delta_x
    delta_f = self.delta_f(torch.cat([_delta_x, skip_f], dim=-1))
    out_x = skip_x + delta_x
    out_f = self.skip(skip_f) + self.drop_path(delta_f)
    point.coord = out_x
    point.feat = out_f
    point.offset = point.offset * self.upscale_factor
    if res and self.enable_residual_attribute and not self.is_first:
        point.attribute = torch_scatter.gather_csr(point.attribute, temp_offset)
    return self.out_norm(point)


def _serves(self, point):
    in_x, in_f, offset, g = point.coord, point.feat, point.offset, point.global_feat
    if isinstance(point.grid_size, torch.Tensor) or not all(isinstance(t, torch.Tensor) for t in (in_x, in_f, offset, g)):
        return False
    if in_f.dim() != 2 or in_x.dim() != 2 or in_x.shape[1] != 3 or g.dim() != 2 or offset.dim() != 1 or offset.shape[0] != g.shape[0]:
        return False
    if not (in_f.is_cuda and in_x.is_cuda and offset.is_cuda and g.is_cuda) or in_f.dtype not in _DTYPES or in_x.dtype not in _DTYPES:
        return False
    if self.frequencies.dtype not in _DTYPES or self.frequencies.device != in_f.device or in_f.shape[1] != self.skip.in_features:
        return False
    return in_envelope(in_f.shape[0], self.upscale_factor, in_f.shape[1], self.skip.out_features, self.frequencies.shape[0], g.shape[0])


def _forward(self, point, res):
    if UPSCALE_BACKEND not in ("torch", "hip"):
        raise ValueError(f"upscale.UPSCALE_BACKEND must be 'torch' or 'hip', not {UPSCALE_BACKEND!r}")
    point = self.in_norm(point)
    if UPSCALE_BACKEND != "hip" or not covers(self) or not _serves(self, point):
        return _reference_tail(self, point, res)
    S = self.upscale_factor
    in_f = point.feat
    out_x, h = expand(self.delta_x(in_f), point.coord, in_f, self.frequencies, S, point.grid_size, self.enable_absolute_pe,
                      self.delta_f[0].eps)
    branch = self.delta_f[1:](h)
    skip = self.skip(in_f)
    keep = _keep_tensor(self.drop_path, branch)
    an = self.out_norm[0]
    point.feat = merge(skip, branch, keep, an.affine(point.global_feat), point.offset, S, an.eps)
    point.coord = out_x
    point.offset = point.offset * S
    if res and self.enable_residual_attribute and not self.is_first:
        point.attribute = point.attribute.repeat_interleave(S, 0)
    return point


def upscale_module_forward(self, point):
    """UpscaleModule.forward of the reference.  Reads self.in_norm, delta_x, skip, delta_f, out_norm, drop_path, frequencies,
    upscale_factor, n_frequencies, enable_absolute_pe; updates point.coord, point.feat and point.offset."""
    return _forward(self, point, False)


def upscale_res_module_forward(self, point):
    """UpscaleResModule.forward of the reference: as upscale_module_forward, and with self.enable_residual_attribute and not
    self.is_first point.attribute is repeated S-fold (repeat_interleave: no read-back)."""
    return _forward(self, point, True)
