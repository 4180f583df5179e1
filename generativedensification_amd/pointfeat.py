"""Projected bilinear sampling of point and volume features on the MI355X (csrc/pointfeat.hip, include/gdr.h
gdr_point_feats_* / gdr_sample_views_*): the step between the reference's coarse and fine render calls.

`point_feats` is the fused form of `Network.get_point_feats` (lightning/network.py) after its `points[mask]`: it projects the
points into the V input views, samples the input image and the coarse `image`, `acc_map` and `depth` renders bilinearly with
zero padding where they already lie (no `cat`, no `einsum` copy), replaces the depth channel by |depth sample - point z| and
returns (N, V, 8) — upstream's `einsum('lcb->blc', point_feats)`.  `sample_views` is the generic form `build_feat_vol` needs:
(V, C, H, W) images sampled at the projections of N points -> (V, C, N) features and the (V, N) depths.

Both are differentiable towards the sampled images and the points (not towards the cameras), work under `no_grad`, under
`torch.autograd.functional.vjp` and under bf16 autocast (inputs are cast to fp32 inside, as the rasterizer's are).  Image
gradients are summed with float atomics; the forward and the point gradient are bitwise reproducible.  A gradient that is
not needed is not computed.  GPU tensors only (no CPU fallback); anything outside the envelope raises before a kernel is
launched: fp32, 1 <= V <= 16, 1 <= C <= 4096, H, W <= 16384, N < 2^31.  The arithmetic, and what happens to a point that
projects to nowhere (h2 == 0, a position that is not finite), is restated in the header of csrc/pointfeat.hip.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from . import _marshal as M

__all__ = ["point_feats", "sample_views", "MAX_VIEWS", "MAX_CHANNELS", "MAX_SIDE"]

MAX_VIEWS, MAX_CHANNELS, MAX_SIDE = L.GDR_PF_MAX_VIEWS, L.GDR_PF_MAX_CHANNELS, L.GDR_PF_MAX_SIDE


def _args(N, V, Cn, H, W):
    a = L.GdrPointfeatArgs()
    a.N, a.V, a.C, a.H, a.W = N, V, Cn, H, W
    return a


class _PointFeats(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, img_ref, image, acc_map, depth, points, w2cs, ixts):
        V, _, H, W = img_ref.shape
        N, dev = points.shape[0], points.device
        w2cs, ixts = w2cs.contiguous(), ixts.contiguous()
        ctx.set_materialize_grads(False)
        with torch.cuda.device(dev):
            out = torch.empty(N, V, 8, dtype=torch.float32, device=dev)
            L.check(L.load().gdr_point_feats_forward(
                C.byref(_args(N, V, 0, H, W)), img_ref.data_ptr(), M.strides(img_ref), image.data_ptr(), M.strides(image),
                acc_map.data_ptr(), M.strides(acc_map), depth.data_ptr(), M.strides(depth, 3), points.data_ptr(), M.strides(points),
                w2cs.data_ptr(), ixts.data_ptr(), out.data_ptr(), M.stream()), "gdr_point_feats_forward")
        ctx.save_for_backward(img_ref, image, acc_map, depth, points, w2cs, ixts)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, gout):
        img_ref, image, acc_map, depth, points, w2cs, ixts = ctx.saved_tensors
        need = ctx.needs_input_grad[:5]
        if gout is None or not any(need):
            return (None,) * 7
        V, _, H, W = img_ref.shape
        N, dev = points.shape[0], points.device
        gout = gout.float().contiguous()
        with torch.cuda.device(dev):
            # the image gradients are atomic sums: zero-filled; the point gradient is stored whole
            grads = [torch.zeros(s.shape, dtype=torch.float32, device=dev) if w else None
                     for s, w in zip((img_ref, image, acc_map, depth), need[:4])]
            grads.append(torch.empty(N, 3, dtype=torch.float32, device=dev) if need[4] else None)
            L.check(L.load().gdr_point_feats_backward(
                C.byref(_args(N, V, 0, H, W)), gout.data_ptr(), img_ref.data_ptr(), M.strides(img_ref), image.data_ptr(),
                M.strides(image), acc_map.data_ptr(), M.strides(acc_map), depth.data_ptr(), M.strides(depth, 3), points.data_ptr(),
                M.strides(points), w2cs.data_ptr(), ixts.data_ptr(), *(M.ptr(g) for g in grads), M.stream()),
                "gdr_point_feats_backward")
        return (*grads, None, None)


class _SampleViews(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, images, points, w2cs, ixts):
        V, Cn, H, W = images.shape
        N, dev = points.shape[0], points.device
        w2cs, ixts = w2cs.contiguous(), ixts.contiguous()
        ctx.set_materialize_grads(False)
        with torch.cuda.device(dev):
            out = torch.empty(V, Cn, N, dtype=torch.float32, device=dev)
            z = torch.empty(V, N, dtype=torch.float32, device=dev)
            L.check(L.load().gdr_sample_views_forward(
                C.byref(_args(N, V, Cn, H, W)), images.data_ptr(), M.strides(images), points.data_ptr(), M.strides(points),
                w2cs.data_ptr(), ixts.data_ptr(), out.data_ptr(), z.data_ptr(), M.stream()), "gdr_sample_views_forward")
        ctx.save_for_backward(images, points, w2cs, ixts)
        return out, z

    @staticmethod
    @torch.autograd.function.once_differentiable
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, gout, gz):
        images, points, w2cs, ixts = ctx.saved_tensors
        need_img, need_pts = ctx.needs_input_grad[:2]
        if (gout is None and gz is None) or not (need_img or need_pts):
            return (None,) * 4
        V, Cn, H, W = images.shape
        N, dev = points.shape[0], points.device
        with torch.cuda.device(dev):
            gout = torch.zeros(V, Cn, N, dtype=torch.float32, device=dev) if gout is None else gout.float().contiguous()
            gz = None if gz is None else gz.float().contiguous()
            g_img = torch.zeros(images.shape, dtype=torch.float32, device=dev) if need_img else None
            g_pts = torch.empty(N, 3, dtype=torch.float32, device=dev) if need_pts else None
            L.check(L.load().gdr_sample_views_backward(
                C.byref(_args(N, V, Cn, H, W)), gout.data_ptr(), M.ptr(gz), images.data_ptr(), M.strides(images), points.data_ptr(),
                M.strides(points), w2cs.data_ptr(), ixts.data_ptr(), M.ptr(g_img), M.ptr(g_pts), M.stream()),
                "gdr_sample_views_backward")
        return g_img, g_pts, None, None


def _check_shapes(named, shapes):
    """The (name, tensor) pairs against `shapes` (None = any extent)."""
    for (name, t), shape in zip(named, shapes):
        if not isinstance(t, torch.Tensor) or t.dim() != len(shape) or any(w is not None and s != w for s, w in zip(t.shape, shape)):
            want = "(" + ", ".join("*" if w is None else str(w) for w in shape) + ")"
            raise ValueError(f"{name} must be a {want} tensor, got {tuple(getattr(t, 'shape', ()))}")


def _check_tensors(named):
    """dtypes, then devices"""
    autocast = torch.is_autocast_enabled()
    for name, t in named:
        if t.dtype != torch.float32 and not (autocast and t.is_floating_point()):
            raise TypeError(f"{name} must be float32 (other floating types only under autocast), not {t.dtype}")
    for name, t in named:
        if not t.is_cuda:
            raise RuntimeError("the HIP feature sampling runs on ROCm/HIP tensors only (no CPU fallback)")
    dev = named[0][1].device
    for name, t in named:
        if t.device != dev:
            raise RuntimeError(f"{name} must live on {named[0][0]}'s device ({dev}), not {t.device}")


def _check_envelope(V, Cn, H, W, N):
    if not 1 <= V <= MAX_VIEWS:
        raise ValueError(f"{V} views are outside the envelope 1..{MAX_VIEWS}")
    if not 1 <= Cn <= MAX_CHANNELS:
        raise ValueError(f"{Cn} channels are outside the envelope 1..{MAX_CHANNELS}")
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"a {H}x{W} image is outside the envelope 1..{MAX_SIDE} per side")
    if N > L.GDR_PF_MAX_POINTS:
        raise ValueError("more than 2^31 - 1 points")


def point_feats(img_ref, image, acc_map, depth, points, w2cs, ixts):
    """img_ref (V, 3, H, W), image (V, H, W, 3), acc_map (V, H, W), depth (V, H, W, 1) or (V, H, W), points (N, 3), w2cs
    (V, 4, 4), ixts (V, 3, 3) -> (N, V, 8): ref rgb, render rgb, acc, |depth sample - z| of every point in every view."""
    if not isinstance(img_ref, torch.Tensor) or img_ref.dim() != 4:
        raise ValueError(f"img_ref must be a (V, 3, H, W) tensor, got {tuple(getattr(img_ref, 'shape', ()))}")
    V, _, H, W = img_ref.shape
    if isinstance(depth, torch.Tensor) and depth.dim() == 3:
        depth_shape = (V, H, W)
    else:
        depth_shape = (V, H, W, 1)
    named = (("img_ref", img_ref), ("image", image), ("acc_map", acc_map), ("depth", depth), ("points", points),
             ("w2cs", w2cs), ("ixts", ixts))
    _check_shapes(named, ((None, 3, None, None), (V, H, W, 3), (V, H, W), depth_shape, (None, 3), (V, 4, 4), (V, 3, 3)))
    _check_envelope(V, 1, H, W, points.shape[0])
    _check_tensors(named)
    return _PointFeats.apply(img_ref, image, acc_map, depth, points, w2cs, ixts)


def sample_views(images, points, w2cs, ixts):
    """images (V, C, H, W), points (N, 3), w2cs (V, 4, 4), ixts (V, 3, 3) -> (feats (V, C, N), z (V, N))."""
    if not isinstance(images, torch.Tensor) or images.dim() != 4:
        raise ValueError(f"images must be a (V, C, H, W) tensor, got {tuple(getattr(images, 'shape', ()))}")
    V, Cn, H, W = images.shape
    named = (("images", images), ("points", points), ("w2cs", w2cs), ("ixts", ixts))
    _check_shapes(named, ((None, None, None, None), (None, 3), (V, 4, 4), (V, 3, 3)))
    _check_envelope(V, Cn, H, W, points.shape[0])
    _check_tensors(named)
    return _SampleViews.apply(images, points, w2cs, ixts)
