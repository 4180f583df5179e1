"""Fused volume conditioning of the volume transformer on the MI355X (csrc/volcond.hip, include/gdr.h gdr_volcond_*): the
stretch of the reference between its image encoder and the first GroupAttBlock, i.e. `Network.build_feat_vol`, the `view_embed`
concat of `Network.forward` and the cond regrouping at the head of `VolTransformer.forward` (lightning/network.py).

    ray_sh(rays, silu=False)                              (..., 6) rays (origin, direction) -> (..., 32) float32: [Y(d / max(|d|,
                                                          1e-12)), Y(o x that)], Y the 16 real spherical harmonics of degree <= 3
                                                          as polynomials (applied to the moment although it is no unit vector);
                                                          silu=True applies SiLU: what ModLN.mlp's Linear sees.  No gradient.
    mod_layer_norm(x, shift_scale, weight, bias, eps)     (layer_norm(x) * weight + bias) * (1 + scale) + shift over rows: x
                                                          (..., C), shift_scale (R, 2C) = [shift, scale], weight / bias (C,) or None
    sample_tokens(rows, points, w2cs, ixts, img_hw, n_group, view_embed=None, out_dtype=None, n_views=None)
                                                          rows (B V, h, w, C) channels-last token maps, points (r^3, 3) in (d, h, w)
                                                          grid order, cameras of an img_hw image -> the cond (B g^3, V bs^3, C + E)
                                                          of the blocks of group size g = n_group (bs = r / g), rows ordered
                                                          (B, g, g, g, V, z, y, x) like deconv3d._cond, view_embed[0, v, :, 0, 0, 0]
                                                          in the columns C..C+E
    build_feat_vol(self, src_inps, img_feats, n_views_sel, batch)   Network.build_feat_vol; bound with one line,
                                                          network.Network.build_feat_vol = volcond.build_feat_vol
    volume_conds(self, img_feats, n_views_sel, batch)     the conds of self.vol_decoder.n_groups, view embedding folded in; for
                                                          deconv3d.vol_transformer_forward_from_conds
    COND_BACKEND                                          "hip" or "torch" (the reference's composition restated here)

The sample position: the intrinsics refer to the full-resolution image (img_hw) while the token map is (h, w), so the map is
sampled at u = (x + 0.5) w / img_w - 0.5, v = (y + 0.5) h / img_h - 0.5, which is what the reference's
grid_sample(align_corners=False) of the normalised pixel does.  Neighbours, weights and their order are grid_sample's with zero
padding.  A (view, point) pair with a zero homogeneous depth or a non-finite / huge position samples zeros; a point behind the
camera projects mirrored (as pointfeat).

Dtypes: every input is float32, float16 or bfloat16 independently; arithmetic is float32.  mod_layer_norm returns what the torch
composition returns (float32 under autocast, the promotion of the input dtypes otherwise); sample_tokens returns the promotion of
rows and view_embed unless out_dtype says float16 / bfloat16.  Gradients come back in the inputs' dtypes: mod_layer_norm to x,
shift_scale, weight and bias (only those needed are computed), sample_tokens to rows and view_embed only (the grid and the
cameras are data).  x is read in place through up to two row strides (the (B V, L, C) token slice of an encoder output with a class
token is not copied); a copy is made only where the layout forces one.
The kernels use no atomics (two calls are bitwise equal, forward and backward) and never synchronise with the host: sample_tokens
saves a tap table (texel, weight per view, point and tap) and its backward groups it by texel with the library's stable radix
sort.  GPU tensors only (no CPU fallback).  Envelope: mod_layer_norm C a multiple of 8 in 8..1024, R < 2^31 (R = 0 returns empty
without a launch); sample_tokens C a multiple of 8 up to 4096, E a multiple of 8 or 0, h, w <= 1024, 4 B V r^3 <= 2^30 (the
sort's limit), n_group divides r.  Anything else raises before a launch.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn.functional as F

from . import _lib as L
from . import _marshal as M

__all__ = ["ray_sh", "mod_layer_norm", "sample_tokens", "build_feat_vol", "volume_conds", "COND_BACKEND", "SLAB_ROWS",
           "MAX_NORM_CHANNELS", "MAX_CHANNELS", "MAX_SIDE", "MAX_ENTRIES"]

SLAB_ROWS = L.GDR_VOLCOND_SLAB_ROWS          # rows per partial of mod_layer_norm's parameter gradients
MAX_NORM_CHANNELS = L.GDR_NORM_MAX_CHANNELS
MAX_CHANNELS, MAX_SIDE, MAX_ENTRIES = L.GDR_VOLCOND_MAX_CHANNELS, L.GDR_VOLCOND_MAX_SIDE, L.GDR_VOLCOND_MAX_ENTRIES
MAX_ROWS = (1 << 31) - 1

# build_feat_vol / volume_conds: "hip" (this module's kernels) or "torch" (the reference's composition restated below, on
# purpose: the A/B of scripts/bench_volcond.py)
COND_BACKEND = "hip"

_DTYPES = M.DTYPES
_NO_CPU = "the HIP volume conditioning runs on ROCm/HIP tensors only (no CPU fallback)"


# ---- argument checks ------------------------------------------------------------------------------------------------------

def _result_dtype(*dtypes):
    """What the torch composition returns: float32 under autocast (layer_norm runs in float32 there and the products with it
    promote), the promotion of the inputs otherwise."""
    if torch.is_autocast_enabled("cuda"):
        return torch.float32
    res = dtypes[0]
    for d in dtypes[1:]:
        res = torch.promote_types(res, d)
    return res


def _row_view(x):
    """x (..., C) as (tensor, row stride, inner rows, outer stride): its R rows through one stride, or through two where the
    leading axes merge to (outer, inner) only, e.g. the (B V, L, C) slice of a (B V, 1 + L, C) encoder output seen as
    (B V, h, w, C); otherwise, or where a stride or the base is not aligned, one contiguous copy."""
    Cn = x.shape[-1]
    R = x.numel() // Cn
    merged = []
    for n, st in zip(x.shape[:-1], x.stride()[:-1]):
        if n == 1:
            continue
        if merged and merged[-1][1] == st * n:
            merged[-1] = (merged[-1][0] * n, st)
        else:
            merged.append((n, st))
    if R and len(merged) <= 2 and x.stride(-1) == 1 and x.data_ptr() % 16 == 0 and all(st % 8 == 0 for _, st in merged):
        if len(merged) == 0:
            return x, Cn, 1, 0
        if merged[-1][1] >= Cn:
            if len(merged) == 1:
                return x, merged[0][1], R, 0
            if merged[0][1] >= 0:
                return x, merged[1][1], merged[1][0], merged[0][1]
    return x.contiguous(), Cn, max(R, 1), 0


# ---- 1: ray_sh --------------------------------------------------------------------------------------------------------------

def ray_sh(rays, silu=False):
    """rays (..., 6) = (origin, direction) -> (..., 32) float32: the degree <= 3 real spherical harmonics of the unit direction
    and of the moment origin x direction; SiLU of them with silu=True.  One launch, no gradient."""
    M.check_float("rays", rays)
    if rays.dim() < 1 or rays.shape[-1] != 6:
        raise ValueError(f"rays must be (..., 6), got {tuple(rays.shape)}")
    n = rays.numel() // 6
    if n * 32 > MAX_ROWS:
        raise ValueError("more than 2^31 - 1 output elements")
    M.check_devices((("rays", rays),), _NO_CPU)
    rays = M.dense(rays.detach())
    with torch.cuda.device(rays.device):
        out = torch.empty(*rays.shape[:-1], 32, dtype=torch.float32, device=rays.device)
        if n:
            L.check(L.load().gdr_volcond_ray_sh(rays.data_ptr(), _DTYPES[rays.dtype], n, int(bool(silu)), out.data_ptr(), M.stream()),
                    "gdr_volcond_ray_sh")
    return out


# ---- 2: mod_layer_norm ------------------------------------------------------------------------------------------------------

def _dt(t):
    return _DTYPES[torch.float32] if t is None else _DTYPES[t.dtype]


class _ModLayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ss, weight, bias, eps, out_dtype):
        dev, Cn = x.device, x.shape[-1]
        xv, xs, inner, outer = _row_view(x)
        R = x.numel() // Cn
        ss, w, b = M.rows2d(ss), M.dense_aligned(weight), M.dense_aligned(bias)
        with torch.cuda.device(dev):
            out = torch.empty(x.shape, dtype=out_dtype, device=dev)
            if R:
                L.check(L.load().gdr_volcond_modln_forward(xv.data_ptr(), xs, inner, outer, _DTYPES[x.dtype], ss.data_ptr(), M.stride0(ss),
                                                           _DTYPES[ss.dtype], M.ptr(w), _dt(w), M.ptr(b), _dt(b), R, Cn, eps,
                                                           out.data_ptr(), _DTYPES[out_dtype], M.stream()), "gdr_volcond_modln_forward")
        ctx.save_for_backward(xv, ss, w, b)
        ctx.geom = (xs, inner, outer, x.shape, R, Cn, eps)
        ctx.meta = [None if t is None else t.dtype for t in (weight, bias)]
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        xv, ss, w, b = ctx.saved_tensors
        xs, inner, outer, shape, R, Cn, eps = ctx.geom
        dev = xv.device
        need_x, need_ss = ctx.needs_input_grad[:2]
        need_w = ctx.meta[0] is not None and ctx.needs_input_grad[2]
        need_b = ctx.meta[1] is not None and ctx.needs_input_grad[3]
        g = M.rows2d(grad_out.reshape(R, Cn))
        lib = L.load()
        with torch.cuda.device(dev):
            grad_x = torch.empty(shape, dtype=xv.dtype, device=dev) if need_x else None
            grad_ss = torch.empty(R, 2 * Cn, dtype=ss.dtype, device=dev) if need_ss else None
            # (R = 0: the fold launch writes the zeros)
            grad_w = torch.empty(Cn, dtype=ctx.meta[0], device=dev) if need_w else None
            grad_b = torch.empty(Cn, dtype=ctx.meta[1], device=dev) if need_b else None
            ws, base, usable = None, None, 0
            if need_w or need_b:
                ws, base, usable = M.queried_workspace(lib.gdr_volcond_modln_backward_bytes, "gdr_volcond_modln_backward_bytes", dev, R, Cn)
            if need_x or need_ss or need_w or need_b:
                L.check(lib.gdr_volcond_modln_backward(M.ptr_or_none_if_empty(g), M.stride0(g), _DTYPES[g.dtype], M.ptr_or_none_if_empty(xv),
                                                       xs, inner, outer, _DTYPES[xv.dtype], M.ptr_or_none_if_empty(ss), M.stride0(ss),
                                                       _DTYPES[ss.dtype], M.ptr(w), _dt(w), M.ptr(b), _dt(b), R, Cn, eps, base, usable,
                                                       M.ptr_or_none_if_empty(grad_x), M.ptr_or_none_if_empty(grad_ss), M.ptr(grad_w),
                                                       M.ptr(grad_b), M.stream()), "gdr_volcond_modln_backward")
        return grad_x, grad_ss, grad_w, grad_b, None, None


def mod_layer_norm(x, shift_scale, weight=None, bias=None, eps=1e-5):
    """x (..., C) with R rows, shift_scale (R, 2C) with shift in [:, :C] and scale in [:, C:] (or (..., 2C) over the same leading
    axes), weight / bias (C,) or None -> (layer_norm(x) * weight + bias) * (1 + scale) + shift, shaped like x."""
    M.check_float("x", x)
    M.check_float("shift_scale", shift_scale)
    if x.dim() < 2:
        raise ValueError(f"x must be (..., C) rows with at least 2 dimensions, got {tuple(x.shape)}")
    Cn = x.shape[-1]
    R = x.numel() // Cn if Cn else 0
    named = [("x", x), ("shift_scale", shift_scale)]
    for name, t in (("weight", weight), ("bias", bias)):
        if t is not None:
            M.check_float(name, t, 1)
            if t.shape[0] != Cn:
                raise ValueError(f"{name} must have {Cn} elements, got {tuple(t.shape)}")
            named.append((name, t))
    if Cn < 8 or Cn > MAX_NORM_CHANNELS or Cn % 8:
        raise ValueError(f"{Cn} channels are outside the envelope: a multiple of 8 in 8..{MAX_NORM_CHANNELS}")
    if shift_scale.dim() < 2 or shift_scale.shape[-1] != 2 * Cn or shift_scale.numel() != R * 2 * Cn:
        raise ValueError(f"x {tuple(x.shape)} needs shift_scale ({R}, {2 * Cn}), got {tuple(shift_scale.shape)}")
    if isinstance(eps, bool) or not isinstance(eps, (int, float)):
        raise TypeError(f"eps must be a number, not {type(eps).__name__}")
    if not eps >= 0:
        raise ValueError(f"eps must be >= 0, got {eps}")
    if R > MAX_ROWS:
        raise ValueError("more than 2^31 - 1 rows")
    M.check_devices(named, _NO_CPU)
    out_dtype = _result_dtype(*(t.dtype for _, t in named))
    if shift_scale.dim() != 2:
        shift_scale = shift_scale.reshape(R, 2 * Cn)
    return _ModLayerNorm.apply(x, shift_scale, weight, bias, float(eps), out_dtype)


# ---- 3: sample_tokens -------------------------------------------------------------------------------------------------------

class _SampleTokens(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rows, ve, points, w2cs, ixts, args, out_dtype):
        dev = rows.device
        a = L.GdrVolcondSampleArgs(*args)
        rows = M.dense_aligned(rows)
        ve2 = None if ve is None else M.rows2d(ve[0, :a.V, :, 0, 0, 0])
        bs = a.r // a.n_group
        entries = 4 * a.B * a.V * a.r ** 3
        need = any(ctx.needs_input_grad[:1])
        with torch.cuda.device(dev):
            cond = torch.empty(a.B * a.n_group ** 3, a.V * bs ** 3, a.C + a.E, dtype=out_dtype, device=dev)
            keys = torch.empty(entries, dtype=torch.int64, device=dev) if need else None
            wts = torch.empty(entries, dtype=torch.float32, device=dev) if need else None
            L.check(L.load().gdr_volcond_sample_forward(C.byref(a), rows.data_ptr(), _DTYPES[rows.dtype], points.data_ptr(), w2cs.data_ptr(),
                                                        ixts.data_ptr(), M.ptr(ve2), 0 if ve2 is None else M.stride0(ve2), _dt(ve2),
                                                        cond.data_ptr(), _DTYPES[out_dtype], M.ptr(keys), M.ptr(wts), M.stream()),
                    "gdr_volcond_sample_forward")
        ctx.save_for_backward(keys, wts)
        ctx.args = args
        ctx.rows_meta = (rows.shape, rows.dtype)
        ctx.ve_meta = None if ve is None else (ve.shape, ve.dtype)
        return cond

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_cond):
        keys, wts = ctx.saved_tensors
        a = L.GdrVolcondSampleArgs(*ctx.args)
        dev = grad_cond.device
        need_rows = ctx.needs_input_grad[0]
        need_ve = ctx.ve_meta is not None and ctx.needs_input_grad[1]
        g = M.dense_aligned(grad_cond)
        lib = L.load()
        grad_rows = grad_ve = None
        with torch.cuda.device(dev):
            ws, base, usable = None, None, 0
            if need_rows:
                grad_rows = torch.empty(ctx.rows_meta[0], dtype=ctx.rows_meta[1], device=dev)
                ws, base, usable = M.queried_workspace(lib.gdr_volcond_sample_backward_bytes, "gdr_volcond_sample_backward_bytes", dev,
                                                       C.byref(a))
            gve = None
            if need_ve:
                shape, dtype = ctx.ve_meta
                grad_ve = (torch.zeros if shape[1] > a.V else torch.empty)(shape, dtype=dtype, device=dev)
                gve = torch.empty(a.V, a.E, dtype=dtype, device=dev)
            if need_rows or need_ve:
                L.check(lib.gdr_volcond_sample_backward(C.byref(a), g.data_ptr(), _DTYPES[g.dtype], M.ptr(keys), M.ptr(wts), base, usable,
                                                        M.ptr(grad_rows), _DTYPES[ctx.rows_meta[1]], M.ptr(gve), _dt(gve), M.stream()),
                        "gdr_volcond_sample_backward")
            if need_ve:
                grad_ve[0, :a.V, :, 0, 0, 0] = gve
        return grad_rows, grad_ve, None, None, None, None, None


def _check_camera(name, t, shape):
    if not isinstance(t, torch.Tensor) or t.dim() != len(shape) or tuple(t.shape) != shape:
        raise ValueError(f"{name} must be a {shape} tensor, got {tuple(getattr(t, 'shape', ()))}")
    if not t.dtype.is_floating_point:
        raise TypeError(f"{name} must be a floating-point tensor, not {t.dtype}")


def _camera(name, t, dev):
    """cameras and grid points keep any float type: converted, not refused"""
    if not t.is_cuda:
        raise RuntimeError(_NO_CPU)
    if t.device != dev:
        raise RuntimeError(f"{name} is on {t.device}, rows on {dev}")
    return t.detach().to(torch.float32).contiguous()


def sample_tokens(rows, points, w2cs, ixts, img_hw, n_group, view_embed=None, out_dtype=None, n_views=None):
    """rows (B V, h, w, C), points (r^3, 3) in (d, h, w) grid order, w2cs (B V, 4, 4), ixts (B V, 3, 3) of an img_hw = (H, W)
    image, view_embed (1, >= V, E, 1, 1, 1) or None -> cond (B g^3, V bs^3, C + E), g = n_group, bs = r / g.  n_views = V (default:
    every camera is a view of one batch element)."""
    M.check_float("rows", rows, 4)
    BV, h, w, Cn = rows.shape
    if isinstance(n_group, bool) or not isinstance(n_group, int) or n_group < 1:
        raise ValueError(f"n_group must be a positive integer, got {n_group!r}")
    V = BV if n_views is None else n_views
    if isinstance(V, bool) or not isinstance(V, int) or V < 1 or BV % V:
        raise ValueError(f"n_views must be a positive integer that divides the {BV} cameras, got {n_views!r}")
    B = BV // V
    try:
        img_h, img_w = (int(v) for v in img_hw)
    except (TypeError, ValueError):
        raise ValueError(f"img_hw must be (H, W), got {img_hw!r}") from None
    if img_h < 1 or img_w < 1:
        raise ValueError(f"img_hw must be positive, got {img_hw!r}")
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be (r^3, 3), got {tuple(getattr(points, 'shape', ()))}")
    N = points.shape[0]
    r = round(N ** (1.0 / 3.0))
    if r < 1 or r ** 3 != N:
        raise ValueError(f"points must hold r^3 grid points, got {N}")
    if r % n_group:
        raise ValueError(f"n_group {n_group} does not divide the grid resolution {r}")
    E = 0
    if view_embed is not None:
        M.check_float("view_embed", view_embed)
        if view_embed.dim() != 6 or view_embed.shape[0] != 1 or view_embed.shape[3:] != (1, 1, 1) or view_embed.shape[1] < V:
            raise ValueError(f"view_embed must be (1, >= {V}, E, 1, 1, 1), got {tuple(view_embed.shape)}")
        E = view_embed.shape[2]
    if Cn < 8 or Cn > MAX_CHANNELS or Cn % 8:
        raise ValueError(f"{Cn} channels are outside the envelope: a multiple of 8 in 8..{MAX_CHANNELS}")
    if E % 8 or E > MAX_CHANNELS or (view_embed is not None and E == 0):
        raise ValueError(f"view_embed's {E} channels are outside the envelope: a multiple of 8 up to {MAX_CHANNELS}")
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f"a {h} x {w} token map is outside the envelope: 1..{MAX_SIDE} a side")
    if BV < 1 or 4 * BV * N > MAX_ENTRIES:
        raise ValueError(f"4 B V r^3 = {4 * BV * N} is outside the envelope 1..{MAX_ENTRIES}")
    _check_camera("points", points, (N, 3))
    _check_camera("w2cs", w2cs, (BV, 4, 4))
    _check_camera("ixts", ixts, (BV, 3, 3))
    if out_dtype is not None and out_dtype not in _DTYPES:
        raise TypeError(f"out_dtype must be float32, float16 or bfloat16, not {out_dtype}")
    if not rows.is_cuda:
        raise RuntimeError(_NO_CPU)
    dev = rows.device
    if view_embed is not None and view_embed.device != dev:
        raise RuntimeError(f"view_embed must live on rows' device ({dev}), not {view_embed.device}")
    points, w2cs, ixts = _camera("points", points, dev), _camera("w2cs", w2cs, dev), _camera("ixts", ixts, dev)
    if out_dtype is None:
        out_dtype = rows.dtype if view_embed is None else torch.promote_types(rows.dtype, view_embed.dtype)
    args = (B, V, h, w, Cn, E, r, n_group, img_h, img_w)
    return _SampleTokens.apply(rows, view_embed, points, w2cs, ixts, args, out_dtype)


# ---- 4: bindings ------------------------------------------------------------------------------------------------------------

def _check_backend():
    if COND_BACKEND not in ("torch", "hip"):
        raise ValueError(f"volcond.COND_BACKEND must be 'torch' or 'hip', not {COND_BACKEND!r}")


def _rsh_cart_3(v):
    """the 16 real spherical harmonics of degree <= 3 as polynomials of v (..., 3), from the closed forms"""
    x, y, z = v.unbind(-1)
    pi = torch.pi
    c1, c2a, c2b, c2c = (3 / (4 * pi)) ** 0.5, (15 / (4 * pi)) ** 0.5, (5 / (16 * pi)) ** 0.5, (15 / (16 * pi)) ** 0.5
    c3a, c3b, c3c, c3d, c3e = ((35 / (32 * pi)) ** 0.5, (105 / (4 * pi)) ** 0.5, (21 / (32 * pi)) ** 0.5, (7 / (16 * pi)) ** 0.5,
                               (105 / (16 * pi)) ** 0.5)
    return torch.stack([torch.full_like(x, (1 / (4 * pi)) ** 0.5), -c1 * y, c1 * z, -c1 * x, c2a * x * y, -c2a * y * z,
                        c2b * (3 * z * z - 1), -c2a * x * z, c2c * (x * x - y * y), -c3a * y * (3 * x * x - y * y), c3b * x * y * z,
                        -c3c * y * (5 * z * z - 1), c3d * z * (5 * z * z - 3), -c3c * x * (5 * z * z - 1), c3e * z * (x * x - y * y),
                        -c3a * x * (x * x - 3 * y * y)], -1)


def _cameras(batch, n_views_sel):
    return batch['tar_w2c'][:, :n_views_sel].reshape(-1, 4, 4), batch['tar_ixt'][:, :n_views_sel].reshape(-1, 3, 3)


def _torch_feat_vol(self, src_inps, img_feats, n_views_sel, batch):
    """the reference's Network.build_feat_vol restated (COND_BACKEND = "torch")"""
    h, w = src_inps.shape[-2:]
    w2cs, ixts = _cameras(batch, n_views_sel)
    grid = self.volume_grid
    pts = grid.reshape(1, -1, 3) @ w2cs[:, :3, :3].permute(0, 2, 1) + w2cs[:, :3, 3][:, None]
    pts = pts @ ixts.permute(0, 2, 1)
    point_img = pts[..., :2] / pts[..., -1:]
    point_img = (point_img + 0.5) / torch.tensor([w, h], device=point_img.device) * 2 - 1.0
    rays = batch['tar_rays_down'][:, :n_views_sel]
    direction = F.normalize(rays[..., 3:6], p=2.0, dim=-1)
    plucker = torch.cat((direction, torch.cross(rays[..., :3], direction, dim=-1)), dim=-1).reshape(-1, *rays.shape[2:])
    feats_dir = torch.cat((_rsh_cart_3(plucker[..., :3]), _rsh_cart_3(plucker[..., 3:6])), dim=-1)
    x = torch.einsum('bchw->bhwc', img_feats)
    shift, scale = self.dir_norm.mlp(feats_dir).chunk(2, dim=-1)
    x = self.dir_norm.norm(x) * (1 + scale) + shift
    x = torch.einsum('bhwc->bchw', x)
    n_channel = x.shape[1]
    vol = F.grid_sample(x.float(), point_img.unsqueeze(1), align_corners=False).to(x)
    reso = self.feat_vol_reso
    return vol.view(-1, n_views_sel, n_channel, reso, reso, reso)


def _token_rows(self, img_feats, n_views_sel, batch):
    """the modulated, normalised token maps (B V, h, w, C) of build_feat_vol, channels-last, and the cameras"""
    w2cs, ixts = _cameras(batch, n_views_sel)
    rays = batch['tar_rays_down'][:, :n_views_sel]
    feats_dir = ray_sh(rays.reshape(-1, *rays.shape[2:]), silu=True)
    norm = self.dir_norm.norm
    x = img_feats.permute(0, 2, 3, 1)              # (B V, h, w, C): a view of the encoder's token-major output
    rows = mod_layer_norm(x, self.dir_norm.mlp[1](feats_dir), norm.weight, norm.bias, norm.eps)
    return rows, w2cs, ixts


def build_feat_vol(self, src_inps, img_feats, n_views_sel, batch):
    """Network.build_feat_vol of the reference (lightning/network.py): reads self.volume_grid, feat_vol_reso and dir_norm (its
    `mlp[1]` Linear and `norm` LayerNorm) and returns the (B, V, C, r, r, r) volume as a permuted view of the token-layout
    result.  Bind with `network.Network.build_feat_vol = volcond.build_feat_vol`."""
    _check_backend()
    if COND_BACKEND == "torch":
        return _torch_feat_vol(self, src_inps, img_feats, n_views_sel, batch)
    r = self.feat_vol_reso
    rows, w2cs, ixts = _token_rows(self, img_feats, n_views_sel, batch)
    # under autocast the reference's einsum copies leave its volume in the autocast dtype: the same dtype, rounded once
    out_dtype = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else None
    cond = sample_tokens(rows, self.volume_grid.reshape(-1, 3), w2cs, ixts, src_inps.shape[-2:], r, out_dtype=out_dtype,
                         n_views=n_views_sel)
    # (B r^3, V, C) -> (B, V, C, r, r, r)
    return cond.view(-1, r, r, r, n_views_sel, cond.shape[-1]).permute(0, 4, 5, 1, 2, 3)


def volume_conds(self, img_feats, n_views_sel, batch, img_hw=None):
    """The conds of the volume transformer's blocks, one (B g^3, V bs^3, C + E) tensor per entry of self.vol_decoder.n_groups,
    for deconv3d.vol_transformer_forward_from_conds: build_feat_vol, the view_embed concat (when cfg.model.view_embed_dim > 0)
    and the cond regrouping in one sampling launch per group size.  img_hw: the size the intrinsics refer to (default: that of
    batch['tar_rgb'], (B, N, H, W, 3))."""
    _check_backend()
    if img_hw is None:
        img_hw = batch['tar_rgb'].shape[2:4]
    n_groups = self.vol_decoder.n_groups
    ve = self.view_embed if self.cfg.model.view_embed_dim > 0 else None
    if COND_BACKEND == "torch":
        from .deconv3d import _cond
        r = self.feat_vol_reso
        vol = _torch_feat_vol(self, torch.empty(0, 0, *img_hw), img_feats, n_views_sel, batch)
        if ve is not None:
            vol = torch.cat((vol, ve[:, :n_views_sel].expand(vol.shape[0], -1, -1, r, r, r)), dim=2)
        return [_cond(vol, g, r // g) for g in n_groups]
    rows, w2cs, ixts = _token_rows(self, img_feats, n_views_sel, batch)
    points = self.volume_grid.reshape(-1, 3)
    return [sample_tokens(rows, points, w2cs, ixts, img_hw, g, view_embed=ve, n_views=n_views_sel) for g in n_groups]
