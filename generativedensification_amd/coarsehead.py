"""The coarse Gaussian head on the MI355X (csrc/coarsehead.hip, include/gdr.h gdr_coarsehead_*): the reference's
`Decoder.forward_coarse` (lightning/network.py: `mlp_coarse` = Linear(C, C), ReLU, Linear(C, C), ReLU, Linear(C, K P), `.float()`,
the five-way split, the two shifts, `sigmoid * 2 - 1` on the offsets) and the three lines of `Network.forward` behind it
(`get_offseted_pt`, the opacity activation and `> 0.005`), in one launch from the dense (..., C) rows deconv3d.py hands on.

    coarse_head(x, w1, b1, w2, b2, w3, b3, K, sh_dim, opacity_shift, scaling_shift)  -> (offset, sh, scaling, rotation, opacity)
    coarse_gaussians(decoder, x, group_centers, half_cell, opacity_shift, scaling_shift, threshold=0.005)
                                                                   -> (centers, sh, scaling, rotation, opacity, mask)
    decoder_forward_coarse(self, feats, opacity_shift, scaling_shift)  Decoder.forward_coarse; bound with one line,
                                                                   network.Decoder.forward_coarse = coarsehead.decoder_forward_coarse
    covers(decoder)                                                whether the module has the one layer list served
    in_envelope(rows, C, K, sh_dim)                                whether the kernels serve this shape

x is (..., C) with any leading shape, B = x.shape[0] and N = rows / B; the parameters are in nn.Linear's layout, w1 and w2
(C, C), w3 (K P, C) with P = 3 + sh_dim + 1 + 3 + 4; the two shifts are Python floats.  The results are float32 whatever x's
dtype (the reference's `.float()`): offset (B, N K, 3), sh (B, N K, sh_dim / 3, 3), scaling (B, N K, 3), rotation (B, N K, 4),
opacity (B, N K, 1); centers (B, N K, 3) = group_centers[n] + offset half_cell with group_centers (N, 3) or (1, N, 3) float32;
mask (B, N K) bool = sigmoid(opacity) > threshold, without a gradient.
The outputs are DENSE tensors of their own.  The reference returns five strided views of one (..., K, P) tensor, which the
rasterizer boundary then copies dense; the values are the same, only `.stride()` differs.

Layout: x's rows are read in place when dense from a 16-byte aligned base; anything else is made so with one copy.
Dtypes: x is float32, float16 or bfloat16 and its dtype is the compute dtype; the parameters may each be any of the three and
are rounded to the compute dtype by the pack kernel and in the epilogues (what autocast's cast does, without a tensor of the
rounded parameter).  The hidden rows are rounded to the compute dtype where torch's Linear rounds them; the last layer's
float32 sum is NOT rounded to 16 bits.  Sums are float32 (float64 for float32 rows).  grad_x has x's dtype; parameter
gradients come back in the parameters' dtypes, rounded once.
Autocast: Linear's rule.  Under an enabled CUDA autocast a float32 x is first cast to the autocast dtype; the Function itself
runs with autocast disabled.
Autograd: once differentiable; x's rows, the parameters and the offset output are saved, the two hidden layers are recomputed
in the backward (a unit's gate is the sign of the rounded pre-activation the forward used).  A gradient nobody needs is not
launched: frozen parameters launch no fold and write no partial sums, an x without requires_grad gets no grad_x store.  A None
upstream gradient is zeros without a fill.  Works under no_grad and torch.autograd.functional.vjp.
The kernels use no atomics (two calls are bitwise equal) and never synchronise with the host.  GPU tensors only (no CPU
fallback).  Wrong dtypes raise TypeError, shapes outside the envelope ValueError, all before any launch.  Envelope: C a
multiple of 8 in 8..MAX_C, both hidden widths C, K in 1..4, sh_dim in (3, 12, 27, 48), K P <= MAX_OUT, rows K below 2^31.
Zero rows return empty tensors without loading the library.  Non-finite inputs are memory-safe and otherwise unspecified.
"""
from __future__ import annotations

import torch

from . import _lib as L
from . import _marshal as M

__all__ = ["coarse_head", "coarse_gaussians", "decoder_forward_coarse", "covers", "in_envelope", "HEAD_BACKEND", "MAX_C", "MAX_OUT",
           "TILE_ROWS", "SLAB_MIN", "SH_DIMS"]

MAX_C, MAX_OUT = L.GDR_COARSEHEAD_MAX_C, L.GDR_COARSEHEAD_MAX_OUT
TILE_ROWS = L.GDR_COARSEHEAD_TILE_ROWS        # rows of one workgroup of the forward
SLAB_MIN = L.GDR_COARSEHEAD_SLAB_MIN          # the parameter gradients cut one slab of rows per this many, 1024 at most
SH_DIMS = (3, 12, 27, 48)

# the path of decoder_forward_coarse and coarse_gaussians: "hip" (this module wherever it covers the module and the shape) or
# "torch" (the reference's lines, on purpose: the A/B of scripts/bench_coarsehead.py)
HEAD_BACKEND = "hip"

_DTYPES = M.DTYPES
_dense = M.dense
_NO_CPU = "the HIP coarse head runs on ROCm/HIP tensors only (no CPU fallback)"


def in_envelope(rows, C, K, sh_dim):
    """whether the kernels serve this shape"""
    return (8 <= C <= MAX_C and C % 8 == 0 and 1 <= K <= 4 and sh_dim in SH_DIMS and K * (sh_dim + 11) <= MAX_OUT
            and 0 <= rows and rows * K < 1 << 31)


def _rows(x):
    """x (..., C) as its (rows, C) matrix, dense from a 16-byte aligned base: a view where x is so already, one copy otherwise"""
    return M.dense_aligned(x.reshape(-1, x.shape[-1]))


def _workspace(lib, what, dt, rows, C, K, sh_dim, dev):
    return M.queried_workspace(lib.gdr_coarsehead_workspace_bytes, "gdr_coarsehead_workspace_bytes", dev, what, dt, rows, C, K, sh_dim)


def _packed(lib, ws3, backward, dt, C, K, sh_dim, dev):
    what = L.GDR_COARSEHEAD_WS_PACKED_BACKWARD if backward else L.GDR_COARSEHEAD_WS_PACKED_FORWARD
    ws, base, _ = _workspace(lib, what, dt, 0, C, K, sh_dim, dev)
    args = [a for w in ws3 for a in (w.data_ptr(), _DTYPES[w.dtype])]
    L.check(lib.gdr_coarsehead_pack(*args, C, K, sh_dim, int(backward), base, dt, M.stream()), "gdr_coarsehead_pack")
    return ws, base


def _grad(g, dev):
    """an upstream gradient as the kernel reads it: None, or dense float32"""
    if g is None:
        return None
    if g.dtype != torch.float32:
        g = g.float()
    return _dense(g)


class _Head(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, w3, b3, group_centers, K, sh_dim, opacity_shift, scaling_shift, half_cell, threshold):
        dev = x.device
        rows = _rows(x)
        n, C = rows.shape
        B = x.shape[0]
        E = n * K // B if B else 0
        params = [_dense(t) for t in (w1, b1, w2, b2, w3, b3)]
        with_centers = group_centers is not None
        gc = _dense(group_centers.reshape(-1, 3)) if with_centers else None
        f32 = dict(dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            offset, scaling = torch.empty(B, E, 3, **f32), torch.empty(B, E, 3, **f32)
            sh, rotation, opacity = torch.empty(B, E, sh_dim // 3, 3, **f32), torch.empty(B, E, 4, **f32), torch.empty(B, E, 1, **f32)
            centers = torch.empty(B, E, 3, **f32) if with_centers else None
            mask = torch.empty(B, E, dtype=torch.bool, device=dev) if with_centers else None
            if n:
                lib, dt = L.load(), _DTYPES[x.dtype]
                ws, base = _packed(lib, params[0::2], False, dt, C, K, sh_dim, dev)
                L.check(lib.gdr_coarsehead_forward(rows.data_ptr(), dt, base, params[1].data_ptr(), _DTYPES[params[1].dtype],
                                                   params[3].data_ptr(), _DTYPES[params[3].dtype], params[5].data_ptr(),
                                                   _DTYPES[params[5].dtype], n, gc.shape[0] if with_centers else 1, C, K, sh_dim,
                                                   opacity_shift, scaling_shift, M.ptr(gc), half_cell, threshold, offset.data_ptr(),
                                                   sh.data_ptr(), scaling.data_ptr(), rotation.data_ptr(), opacity.data_ptr(), M.ptr(centers),
                                                   M.ptr(mask), M.stream()), "gdr_coarsehead_forward")
        ctx.save_for_backward(rows, *params, offset)
        ctx.set_materialize_grads(False)      # a None upstream gradient stays None: the kernel reads it as zeros
        ctx.shape = (x.shape, K, sh_dim, half_cell)
        ctx.meta = [(t.dtype, t.shape) for t in (w1, b1, w2, b2, w3, b3)]
        if with_centers:
            ctx.mark_non_differentiable(mask)
            return offset, sh, scaling, rotation, opacity, centers, mask
        return offset, sh, scaling, rotation, opacity

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_offset, g_sh, g_scaling, g_rotation, g_opacity, g_centers=None, g_mask=None):
        rows, w1, b1, w2, b2, w3, b3, offset = ctx.saved_tensors
        x_shape, K, sh_dim, half_cell = ctx.shape
        n, C = rows.shape
        dev, dt = rows.device, _DTYPES[rows.dtype]
        need = ctx.needs_input_grad
        need_x, need_p = need[0], list(need[1:7])
        gs = [_grad(g, dev) for g in (g_offset, g_sh, g_scaling, g_rotation, g_opacity, g_centers)]
        grad_x = None
        grads = [None] * 6
        with torch.cuda.device(dev):
            if need_x:
                grad_x = torch.empty_like(rows)
            for i, (dtype, shape) in enumerate(ctx.meta):
                if need_p[i]:
                    grads[i] = (torch.empty if n else torch.zeros)(shape, dtype=dtype, device=dev)
            if n and (need_x or any(need_p)):
                lib = L.load()
                pws, pbase = _packed(lib, (w1, w2, w3), True, dt, C, K, sh_dim, dev)
                ws, base, usable = (_workspace(lib, L.GDR_COARSEHEAD_WS_PARTIALS, dt, n, C, K, sh_dim, dev) if any(need_p)
                                    else (None, None, 0))
                L.check(lib.gdr_coarsehead_backward(rows.data_ptr(), dt, pbase, b1.data_ptr(), _DTYPES[b1.dtype], b2.data_ptr(),
                                                    _DTYPES[b2.dtype], n, C, K, sh_dim, offset.data_ptr(), *[M.ptr(g) for g in gs],
                                                    half_cell, M.ptr(grad_x), base, usable, M.stream()), "gdr_coarsehead_backward")
                if any(need_p):
                    out = [a for g in grads for a in (M.ptr(g), _DTYPES[g.dtype] if g is not None else dt)]
                    L.check(lib.gdr_coarsehead_fold(base, usable, dt, n, C, K, sh_dim, *out, M.stream()), "gdr_coarsehead_fold")
        if need_x:
            grad_x = grad_x.view(x_shape)
        return (grad_x, *grads, None, None, None, None, None, None, None)


def _check(x, params, K, sh_dim, group_centers):
    named = [("x", x)] + list(zip(("w1", "b1", "w2", "b2", "w3", "b3"), params))
    for name, t in named:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, not {type(t).__name__}")
        if t.dtype not in _DTYPES:
            raise TypeError(f"{name} must be float32, float16 or bfloat16, not {t.dtype}")
    if group_centers is not None:
        if not isinstance(group_centers, torch.Tensor):
            raise TypeError(f"group_centers must be a tensor, not {type(group_centers).__name__}")
        if group_centers.dtype != torch.float32:
            raise TypeError(f"group_centers must be float32, not {group_centers.dtype}")
        named.append(("group_centers", group_centers))
    for name, v in (("K", K), ("sh_dim", sh_dim)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError(f"{name} must be an int, not {type(v).__name__}")
    if x.dim() < 2:
        raise ValueError(f"x is (B, ..., C), got {tuple(x.shape)}")
    C = x.shape[-1]
    rows = x.numel() // C if C else 0
    if not 1 <= K <= 4 or sh_dim not in SH_DIMS:
        raise ValueError(f"K = {K}, sh_dim = {sh_dim} are outside the envelope: K in 1..4, sh_dim one of {SH_DIMS}")
    KP = K * (sh_dim + 11)
    w1, b1, w2, b2, w3, b3 = params
    for name, t, shape in (("w1", w1, (C, C)), ("b1", b1, (C,)), ("w2", w2, (C, C)), ("b2", b2, (C,)), ("w3", w3, (KP, C)), ("b3", b3, (KP,))):
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {shape} (both hidden widths equal C = {C}, K P = {KP}), got {tuple(t.shape)}")
    if not in_envelope(rows, C, K, sh_dim):
        raise ValueError(f"rows = {rows}, C = {C}, K = {K}, sh_dim = {sh_dim} are outside the envelope: C a multiple of 8 in 8..{MAX_C}, "
                         f"K P <= {MAX_OUT}, rows K below 2^31")
    if group_centers is not None:
        B = x.shape[0]
        N = rows // B if B else 0
        if group_centers.numel() != 3 * N or group_centers.shape[-1] != 3:
            raise ValueError(f"group_centers must be (N, 3) or (1, N, 3) with N = {N}, got {tuple(group_centers.shape)}")
    for name, t in named:
        if not t.is_cuda:
            raise RuntimeError(_NO_CPU)
    for name, t in named:
        if t.device != x.device:
            raise RuntimeError(f"{name} must live on x's device ({x.device}), not {t.device}")


def _apply(x, params, group_centers, K, sh_dim, opacity_shift, scaling_shift, half_cell, threshold):
    _check(x, params, K, sh_dim, group_centers)
    if x.dtype == torch.float32 and torch.is_autocast_enabled("cuda"):
        x = x.to(torch.get_autocast_dtype("cuda"))
    with torch.autocast("cuda", enabled=False):
        return _Head.apply(x, *params, group_centers, K, sh_dim, float(opacity_shift), float(scaling_shift), float(half_cell), float(threshold))


def coarse_head(x, w1, b1, w2, b2, w3, b3, K, sh_dim, opacity_shift, scaling_shift):
    """x (B, ..., C) and mlp_coarse's parameters in nn.Linear's layout -> (offset, sh, scaling, rotation, opacity), dense float32
    tensors with the shapes and values of the reference's Decoder.forward_coarse."""
    return _apply(x, (w1, b1, w2, b2, w3, b3), None, K, sh_dim, opacity_shift, scaling_shift, 0.0, 0.0)


def covers(decoder):
    """whether `decoder.mlp_coarse` is exactly Sequential(Linear(C, C), ReLU, Linear(C, C), ReLU, Linear(C, P K)) with biases,
    and opacity_dim, scaling_dim, rotation_dim are 1, 3, 4"""
    mlp = getattr(decoder, "mlp_coarse", None)
    if not isinstance(mlp, torch.nn.Sequential) or len(mlp) != 5:
        return False
    kinds = (torch.nn.Linear, torch.nn.ReLU, torch.nn.Linear, torch.nn.ReLU, torch.nn.Linear)
    if any(type(m) is not k for m, k in zip(mlp, kinds)):
        return False
    l1, l2, l3 = mlp[0], mlp[2], mlp[4]
    if any(lin.bias is None for lin in (l1, l2, l3)):
        return False
    try:
        dims = (decoder.opacity_dim, decoder.scaling_dim, decoder.rotation_dim)
        K, sh_dim = decoder.K, decoder.sh_dim
    except AttributeError:
        return False
    C = l1.in_features
    return (dims == (1, 3, 4) and isinstance(K, int) and isinstance(sh_dim, int) and l1.out_features == C and l2.in_features == C
            and l2.out_features == C and l3.in_features == C and l3.out_features == K * (sh_dim + 11))


def _params(decoder):
    mlp = decoder.mlp_coarse
    return (mlp[0].weight, mlp[0].bias, mlp[2].weight, mlp[2].bias, mlp[4].weight, mlp[4].bias)


def _served(decoder, feats):
    if HEAD_BACKEND not in ("torch", "hip"):
        raise ValueError(f"coarsehead.HEAD_BACKEND must be 'torch' or 'hip', not {HEAD_BACKEND!r}")
    if HEAD_BACKEND != "hip" or not covers(decoder) or feats.dim() < 2:
        return False
    C = decoder.mlp_coarse[0].in_features
    return feats.shape[-1] == C and in_envelope(feats.numel() // C, C, decoder.K, decoder.sh_dim)


def _torch_forward_coarse(self, feats, opacity_shift, scaling_shift):
    """the reference's lines"""
    parameters = self.mlp_coarse(feats).float()
    parameters = parameters.view(*parameters.shape[:-1], self.K, -1)
    offset, sh, opacity, scaling, rotation = torch.split(
        parameters, [3, self.sh_dim, self.opacity_dim, self.scaling_dim, self.rotation_dim], dim=-1)
    opacity = opacity + opacity_shift
    scaling = scaling + scaling_shift
    offset = torch.sigmoid(offset) * 2 - 1.0
    B = opacity.shape[0]
    return (offset.view(B, -1, 3), sh.view(B, -1, self.sh_dim // 3, 3), scaling.view(B, -1, self.scaling_dim),
            rotation.view(B, -1, self.rotation_dim), opacity.view(B, -1, self.opacity_dim))


def decoder_forward_coarse(self, feats, opacity_shift, scaling_shift):
    """Decoder.forward_coarse of the reference (lightning/network.py): reads self.mlp_coarse, K, sh_dim, opacity_dim, scaling_dim and
    rotation_dim and returns the reference's order, offset, sh, scaling, rotation, opacity, as dense float32 tensors from one
    launch of csrc/coarsehead.hip wherever `covers` and `in_envelope` hold and HEAD_BACKEND is "hip"; anywhere else it is the
    reference's lines (strided views of one tensor)."""
    if _served(self, feats):
        return coarse_head(feats, *_params(self), self.K, self.sh_dim, opacity_shift, scaling_shift)
    return _torch_forward_coarse(self, feats, opacity_shift, scaling_shift)


def coarse_gaussians(decoder, x, group_centers, half_cell, opacity_shift, scaling_shift, threshold=0.005):
    """decoder.forward_coarse(x, ...), get_offseted_pt and the opacity mask of the reference's Network.forward in one launch:
    -> (centers, sh, scaling, rotation, opacity, mask) with centers = group_centers[n] + offset half_cell (B, N K, 3) and
    mask = sigmoid(opacity) > threshold (B, N K) bool, which carries no gradient.  group_centers is (N, 3) or (1, N, 3) float32."""
    if _served(decoder, x):
        res = _apply(x, _params(decoder), group_centers, decoder.K, decoder.sh_dim, opacity_shift, scaling_shift, half_cell, threshold)
        return res[5], res[1], res[2], res[3], res[4], res[6]
    offset, sh, scaling, rotation, opacity = _torch_forward_coarse(decoder, x, opacity_shift, scaling_shift)
    B = offset.shape[0]
    centers = group_centers.reshape(1, -1, 3).unsqueeze(-2).expand(B, -1, decoder.K, -1).reshape(offset.shape) + offset * half_cell
    mask = torch.sigmoid(opacity).squeeze(-1) > threshold
    return centers, sh, scaling, rotation, opacity, mask
