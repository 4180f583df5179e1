"""float64 numpy restatement of generativedensification_amd/upscale.py (csrc/upscale.hip): `expand`, `merge` and the
closed-form gradients the kernels implement, written from the arithmetic of the module's docstring.  Beside it the two torch
compositions the GPU tests compare with (the reference's lines without the read-back of gather_csr) and a small module with
UpscaleModule's attribute surface for the binding tests.  tests/test_upscale_cpu.py holds the gradients against central
differences; tests/test_gpu_upscale.py holds the kernels against all of it.

The truth has no intermediate rounding: the roundings `expand` and `merge` make where torch makes them are part of what the
accuracy bar measures, for both candidates alike."""
import math

import numpy as np

import norm_ref as NR

to_dtype, half_ulp = NR.to_dtype, NR.half_ulp


# ---- expand ---------------------------------------------------------------------------------------------------------------

def expand_offsets(t, grid_size):
    """(u, d) as (N S, 3): u = tanh(t), d = 0.5 * grid_size * u"""
    t = np.asarray(t, dtype=np.float64)
    u = np.tanh(t).reshape(-1, 3)
    return u, (0.5 * grid_size) * u


def expand(t, coord, feat, frequencies, upscale_factor, grid_size, absolute_pe=False, eps=1e-5):
    """(out_x, h)"""
    s = upscale_factor
    _, d = expand_offsets(t, grid_size)
    out_x = np.repeat(np.asarray(coord, dtype=np.float64), s, axis=0) + d
    return out_x, NR.pe_concat_layer_norm(out_x if absolute_pe else d, feat, frequencies, s, eps)


def expand_chain(t, grid_size, upscale_factor, grad_out_x, dx, absolute_pe):
    """(grad_t, grad_coord) from the gradient dx of h at the PE argument and grad_out_x: the chain rule behind the PE"""
    t = np.asarray(t, dtype=np.float64)
    u, _ = expand_offsets(t, grid_size)
    g, dx = np.asarray(grad_out_x, dtype=np.float64), np.asarray(dx, dtype=np.float64)
    gd = g + dx
    grad_t = (gd * (0.5 * grid_size) * (1.0 - u * u)).reshape(t.shape)
    grad_coord = (gd if absolute_pe else g).reshape(t.shape[0], upscale_factor, 3).sum(1)
    return grad_t, grad_coord


def expand_grad(t, coord, feat, frequencies, upscale_factor, grid_size, grad_out_x, grad_h, absolute_pe=False, eps=1e-5):
    """(grad_t, grad_coord, grad_feat); a None gradient is zeros"""
    s = upscale_factor
    out_x, _ = expand(t, coord, feat, frequencies, s, grid_size, absolute_pe, eps)
    _, d = expand_offsets(t, grid_size)
    n, c = np.asarray(feat).shape
    if grad_out_x is None:
        grad_out_x = np.zeros((n * s, 3))
    if grad_h is None:
        grad_h = np.zeros((n * s, 6 * len(frequencies) + c))
    dx, grad_feat = NR.pe_concat_layer_norm_grad(out_x if absolute_pe else d, feat, frequencies, s, grad_h, eps)
    grad_t, grad_coord = expand_chain(t, grid_size, s, grad_out_x, dx, absolute_pe)
    return grad_t, grad_coord, grad_feat


# ---- merge ----------------------------------------------------------------------------------------------------------------

def merge_rows(skip, branch, keep, upscale_factor):
    skip, branch = np.asarray(skip, dtype=np.float64), np.asarray(branch, dtype=np.float64)
    kb = branch if keep is None else np.asarray(keep, dtype=np.float64).reshape(-1, 1) * branch
    return np.repeat(skip, upscale_factor, axis=0) + kb


def merge(skip, branch, keep, scale, offset, upscale_factor, eps=1e-5):
    """offset: the parents' segment ends"""
    y = merge_rows(skip, branch, keep, upscale_factor)
    return NR.ada_layer_norm(y, scale, np.asarray(offset, dtype=np.int64) * upscale_factor, eps)


def merge_grad(skip, branch, keep, scale, offset, upscale_factor, grad_out, eps=1e-5):
    """(grad_skip, grad_branch, grad_scale)"""
    s = upscale_factor
    y = merge_rows(skip, branch, keep, s)
    dy, dscale = NR.ada_layer_norm_grad(y, scale, np.asarray(offset, dtype=np.int64) * s, grad_out, eps)
    n, c = np.asarray(skip).shape
    dbranch = dy if keep is None else np.asarray(keep, dtype=np.float64).reshape(-1, 1) * dy
    return dy.reshape(n, s, c).sum(1), dbranch, dscale


# ---- the torch compositions -----------------------------------------------------------------------------------------------

def torch_expand(t, coord, feat, frequencies, upscale_factor, grid_size, absolute_pe=False, eps=1e-5, keep=None):
    """the reference's lines with repeat_interleave for gather_csr -> (out_x, h); `keep`, a dict, receives the intermediate
    tensors delta_x and skip_x with retain_grad set"""
    import torch
    import torch.nn.functional as F

    s = upscale_factor
    skip_x = coord.repeat_interleave(s, 0)
    delta_x = 0.5 * grid_size * torch.tanh(t.reshape(-1, 3))
    if keep is not None:
        for name, v in (("delta_x", delta_x), ("skip_x", skip_x)):
            if v.requires_grad:
                v.retain_grad()
            keep[name] = v
    x = skip_x + delta_x if absolute_pe else delta_x
    fx = torch.flatten(frequencies[None, :, None] * x[:, None, :], -2, -1)
    z = torch.cat([torch.sin(fx), torch.cos(fx), feat.repeat_interleave(s, 0)], dim=-1)
    return skip_x + delta_x, F.layer_norm(z, z.shape[1:], eps=eps)


def torch_ada(feat, scale, offset, eps=1e-5):
    """gather(scale) * layer_norm(feat) without a read-back; rows at or behind offset[-1] are zero"""
    import torch
    import torch.nn.functional as F

    seg = torch.searchsorted(offset, torch.arange(feat.shape[0], device=feat.device), right=True)
    padded = torch.cat([scale, scale.new_zeros(1, scale.shape[1])])
    return padded.index_select(0, seg) * F.layer_norm(feat, feat.shape[1:], eps=eps)


def torch_merge(skip, branch, keep, scale, offset, upscale_factor, eps=1e-5):
    """the reference's `self.skip(skip_f) + self.drop_path(delta_f)` and out_norm, with the skip rows repeated"""
    s = upscale_factor
    kb = branch if keep is None else branch * keep.reshape(-1, 1)
    return torch_ada(skip.repeat_interleave(s, 0) + kb, scale, offset * s, eps)


# ---- a module with UpscaleModule's attribute surface ----------------------------------------------------------------------

class Point(dict):
    """attribute access onto a dict, as the reference's Point"""
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def make_module(in_channels, out_channels, upscale_factor, n_frequencies, global_channels=24, drop_path=0.0, absolute_pe=False,
                residual_attribute=False, is_first=True, seed=0, ada_forward=None, norm="ada"):
    """A module that has what upscale.upscale_module_forward reads and nothing else of the reference: in_norm / out_norm are
    one-element containers round a LayerNorm without affine that has an `affine` Linear child, called on the point; drop_path
    draws as timm's DropPath does.  `ada_forward(self, feat, global_feat, offset)` is bound onto the norm class (the fused
    AdaLayerNorm on the GPU); the default is the torch composition, which also runs in float64 on the CPU.  Parameters come
    from a seeded numpy draw.  norm: "ada", or "ln" for the nn.LayerNorm without affine and without a child that Network
    builds (the container hands it the features alone, as the reference's PointSequential does)."""
    import torch
    from torch import nn

    assert norm in ("ada", "ln")

    class AdaNorm(nn.LayerNorm):
        def __init__(self, channels):
            super().__init__(channels, elementwise_affine=False)
            self.affine = nn.Linear(global_channels, channels)

        forward = ada_forward or (lambda self, feat, global_feat, offset: torch_ada(feat, self.affine(global_feat), offset, self.eps))

    class PointSeq(nn.Module):
        def __init__(self, norm):
            super().__init__()
            self.add_module("0", norm)

        def __getitem__(self, i):
            return list(self._modules.values())[i]

        def __len__(self):
            return len(self._modules)

        def forward(self, point):
            for m in self._modules.values():
                point.feat = m(point.feat, point.global_feat, point.offset) if isinstance(m, AdaNorm) else m(point.feat)
            return point

    def norm_layer(channels):
        return AdaNorm(channels) if norm == "ada" else nn.LayerNorm(channels, elementwise_affine=False)

    class DropPath(nn.Module):
        def __init__(self, drop_prob, scale_by_keep=True):
            super().__init__()
            self.drop_prob, self.scale_by_keep = drop_prob, scale_by_keep

        def forward(self, x):
            if self.drop_prob == 0.0 or not self.training:
                return x
            keep_prob = 1 - self.drop_prob
            mask = x.new_empty((x.shape[0],) + (1,) * (x.ndim - 1)).bernoulli_(keep_prob)
            if keep_prob > 0.0 and self.scale_by_keep:
                mask.div_(keep_prob)
            return x * mask

    class UpscaleLike(nn.Module):
        def __init__(self):
            super().__init__()
            c, co, s, f = in_channels, out_channels, upscale_factor, n_frequencies
            self.is_first, self.in_channels, self.out_channels, self.upscale_factor, self.n_frequencies = is_first, c, co, s, f
            self.enable_absolute_pe, self.enable_residual_attribute = absolute_pe, residual_attribute
            self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
            self.in_norm = PointSeq(norm_layer(c))
            self.delta_x = nn.Sequential(nn.Linear(c, c), nn.GELU(), nn.Linear(c, 3 * s))
            self.skip = nn.Linear(c, co)
            self.delta_f = nn.Sequential(nn.LayerNorm(c + 6 * f, elementwise_affine=False), nn.Linear(c + 6 * f, c), nn.GELU(),
                                         nn.Linear(c, co))
            self.out_norm = PointSeq(norm_layer(co))
            self.register_buffer("frequencies", 2.0 ** torch.arange(f))

    m = UpscaleLike()
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        for p in m.parameters():
            fan = p.shape[-1] if p.dim() > 1 else 4
            p.copy_(torch.from_numpy(rng.standard_normal(tuple(p.shape)) / math.sqrt(fan)))
    return m


MUTANTS = ("cat_skip_then_pe", "cos_before_sin")


def reference_forward(self, point, res=False, gather=None, mut=None):
    """UpscaleModule.forward / UpscaleResModule.forward (res) of the reference restated; `gather(src, indptr)` is gather_csr
    (default: repeat_interleave, which also runs on the CPU).  `mut` switches one deliberate mistake on."""
    assert mut in (None,) + MUTANTS
    import torch

    s = self.upscale_factor
    point = self.in_norm(point)
    in_x, in_f = point.coord, point.feat
    n = len(in_x)
    if gather is None:
        def gather(src, indptr):
            return src.repeat_interleave(s, 0)
    temp_offset = torch.arange(n + 1, dtype=torch.int64, device=in_x.device) * s
    skip_x, skip_f = gather(in_x, temp_offset), gather(in_f, temp_offset)
    delta_x = self.delta_x(in_f).reshape(n * s, 3)
    delta_x = 0.5 * point.grid_size * torch.tanh(delta_x)
    x = skip_x + delta_x if self.enable_absolute_pe else delta_x
    fx = torch.flatten(self.frequencies[None, :, None] * x[:, None, :], -2, -1)
    pe = [torch.cos(fx), torch.sin(fx)] if mut == "cos_before_sin" else [torch.sin(fx), torch.cos(fx)]
    delta_f = self.delta_f(torch.cat([skip_f] + pe if mut == "cat_skip_then_pe" else pe + [skip_f], dim=-1))
    point.coord = skip_x + delta_x
    point.feat = self.skip(skip_f) + self.drop_path(delta_f)
    point.offset = point.offset * s
    if res and self.enable_residual_attribute and not self.is_first:
        point.attribute = gather(point.attribute, temp_offset)
    return self.out_norm(point)
