"""Densification masks of the point decoder on the MI355X (csrc/densify.hip, include/gdr.h gdr_densify_*): what the reference's
`MaskModule` / `MaskResModule` (lightning/point_decoder/autoencoder.py) do around their scores.

`segment_top_k(x, ratio, offset)` / `segment_top_p(x, ratio, offset)` -> `(mask, new_offset)`: per segment of `offset` the rows
are ranked by descending value (NaN above every number, -0 = +0, equal values by ascending row: the defined tie rule, one of the
outcomes of the reference's unstable sort).  top-k keeps the first `min(k_b, n_b)` ranks with `k_b` the reference's
`(float(ratio) * n_b.to(x.dtype)).ceil()`, rounding steps included; top-p keeps rank j iff the inclusive fp32 prefix sum of the
ranked values, rounded to x's dtype, is `<=` the ratio rounded to x's dtype.  Rows at or behind `offset[-1]` are never selected,
empty segments are legal, offsets are clamped to `[previous end, N]` on the device.  No gradient, no host synchronisation.
`top_k(x, ratio, batch)` / `top_p(x, ratio, offset)` carry the reference's signatures (`autoencoder.top_k = densify.top_k`);
`top_k` reads `batch[-1]` back once, as the reference's scatter with `dim_size=None` does, and needs an ascending `batch`.

`ste_gate(feat, prob, mask=None)` is the straight-through estimator of both modules: the value `feat` (or `feat * mask`),
exactly, with the gradients of `feat * prob`.  `split_rows(mask, coord, feat, prob=None, n_selected=None)` ->
`(coord_sel, feat_sel, coord_rest, feat_rest)` is `coord[mask], feat[mask], coord[~mask], feat[~mask]` in one launch behind a
scan of the mask, with the gate folded in when `prob` is given; it reads the selected count back once (8 bytes) unless
`n_selected` is given.  With a wrong `n_selected` the rows whose destination lies beyond it are dropped, rows of an output
that nothing maps to are unspecified, and nothing is written outside the outputs.

`mask_module_forward` / `mask_res_module_forward` bind onto the reference's classes
(`autoencoder.MaskModule.forward = densify.mask_module_forward`).

GPU tensors only (no CPU fallback).  No atomics: two calls are bitwise equal.  Envelope: N at most 2^30, 1 <= B <= 1024, C a
multiple of 8 in 8..1024; f32 / f16 / bf16, each input's dtype independent; N = 0 returns empty tensors without a launch.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn.functional as F

from . import _lib as L
from . import _marshal as M

__all__ = ["segment_top_k", "segment_top_p", "top_k", "top_p", "ste_gate", "split_rows", "mask_module_forward",
           "mask_res_module_forward", "MAX_CHANNELS", "MAX_SEGMENTS", "MAX_ROWS", "CHUNK", "POINT_KEYS", "LEAF_POINT_KEYS",
           "MASK_RES_KEYS"]

MAX_CHANNELS, MAX_SEGMENTS, CHUNK = L.GDR_DENSIFY_MAX_CHANNELS, L.GDR_DENSIFY_MAX_SEGMENTS, L.GDR_DENSIFY_CHUNK
MAX_ROWS = L.GDR_SERIAL_MAX_POINTS

# the keys of the Point objects MaskModule builds and of the update MaskResModule makes (tests/golden/densify_surface.json)
POINT_KEYS = ("coord", "feat", "global_feat", "offset", "grid_size", "leaf_point")
LEAF_POINT_KEYS = ("coord", "feat", "offset", "grid_size")
MASK_RES_KEYS = ("raw_prob", "prob", "non_leaf", "non_leaf_offset", "leaf", "leaf_offset")

_DTYPES = M.DTYPES
_NO_CPU = "the HIP densification masks run on ROCm/HIP tensors only (no CPU fallback)"


# ---- argument checks ------------------------------------------------------------------------------------------------------

def _check_vector(name, t):
    """t (N,) or (N, 1) of a floating dtype"""
    M.check_float(name, t)
    if t.dim() not in (1, 2) or (t.dim() == 2 and t.shape[1] != 1):
        raise ValueError(f"{name} must be (N,) or (N, 1), got {tuple(t.shape)}")


def _check_offset(offset):
    if not isinstance(offset, torch.Tensor):
        raise TypeError(f"offset must be a tensor, not {type(offset).__name__}")
    if offset.dtype.is_floating_point or offset.dtype.is_complex or offset.dtype == torch.bool:
        raise TypeError(f"offset must be an integer tensor, not {offset.dtype}")
    if offset.dim() != 1:
        raise ValueError(f"offset must be (B,), got {tuple(offset.shape)}")
    if not 1 <= offset.shape[0] <= MAX_SEGMENTS:
        raise ValueError(f"{offset.shape[0]} segments are outside the envelope 1..{MAX_SEGMENTS}")


def _check_ratio(ratio):
    ratio = float(ratio)
    if not (0.0 < ratio < 1.0 and 0.0 < C.c_float(ratio).value < 1.0):
        raise ValueError(f"ratio must lie in (0, 1), got {ratio}")
    return ratio


def _check_rows(name, t, N=None):
    M.check_float(name, t)
    if t.dim() != 2:
        raise ValueError(f"{name} must have 2 dimensions, got {tuple(t.shape)}")
    if N is not None and t.shape[0] != N:
        raise ValueError(f"{name} must have {N} rows, got {tuple(t.shape)}")
    c = t.shape[1]
    if c < 8 or c > MAX_CHANNELS or c % 8:
        raise ValueError(f"{c} channels are outside the envelope: a multiple of 8 in 8..{MAX_CHANNELS}")
    if t.shape[0] > MAX_ROWS:
        raise ValueError("more than 2^30 rows")


def _check_mask(mask, N):
    if not isinstance(mask, torch.Tensor):
        raise TypeError(f"mask must be a tensor, not {type(mask).__name__}")
    if mask.dtype != torch.bool:
        raise TypeError(f"mask must be a bool tensor, not {mask.dtype}")
    if mask.shape != (N,):
        raise ValueError(f"mask must be ({N},), got {tuple(mask.shape)}")


# ---- selection ------------------------------------------------------------------------------------------------------------

@torch.no_grad()
def _select(x, ratio, offset, mode):
    _check_vector("x", x)
    _check_offset(offset)
    ratio = _check_ratio(ratio)
    if x.shape[0] > MAX_ROWS:
        raise ValueError("more than 2^30 rows")
    M.check_devices((("x", x), ("offset", offset)), _NO_CPU)
    N, B, dev = x.shape[0], offset.shape[0], x.device
    x, offset = x.detach().reshape(-1).contiguous(), offset.long().contiguous()
    # top-p compares with the ratio as the reference's `x_cumsum <= ratio` sees it: cast to x's dtype (a host-side cast)
    threshold = float(torch.tensor(ratio, dtype=x.dtype).float())
    lib = L.load()
    with torch.cuda.device(dev):
        mask = torch.empty(N, dtype=torch.bool, device=dev)
        if N == 0:
            return mask, torch.zeros(B, dtype=torch.int64, device=dev)
        new_offset = torch.empty(B, dtype=torch.int64, device=dev)
        nbytes = lib.gdr_densify_select_bytes(N, B)
        if nbytes == 0:
            L.check(-1, "gdr_densify_select_bytes")
        ws, base, usable = M.workspace(nbytes, dev)
        L.check(lib.gdr_densify_select(x.data_ptr(), _DTYPES[x.dtype], offset.data_ptr(), N, B, L.GDR_DENSIFY_MODES[mode], ratio,
                                       threshold, base, usable, mask.data_ptr(), new_offset.data_ptr(), M.stream()),
                "gdr_densify_select")
    return mask, new_offset


def segment_top_k(x, ratio, offset):
    """x (N,) or (N, 1), 0 < ratio < 1, offset (B,) integer segment ends on the device -> mask (N,) bool, new_offset (B,) int64:
    the first min(k_b, n_b) rows of every segment's ranking, k_b = ceil(ratio * n_b) with the reference's rounding to x's dtype."""
    return _select(x, ratio, offset, "top_k")


def segment_top_p(x, ratio, offset):
    """As segment_top_k, selecting rank j iff the segment's inclusive fp32 prefix sum of the ranked values, rounded to x's
    dtype, is <= ratio rounded to x's dtype.  Negative or NaN values are outside the contract (memory-safe, unspecified)."""
    return _select(x, ratio, offset, "top_p")


@torch.no_grad()
def top_k(x, ratio, batch):
    """The reference's top_k(x, ratio, batch): `batch` (N,) ascending segment ids (offset2batch); one read of batch[-1]."""
    if not isinstance(batch, torch.Tensor):
        raise TypeError(f"batch must be a tensor, not {type(batch).__name__}")
    if batch.dtype.is_floating_point or batch.dtype.is_complex or batch.dtype == torch.bool:
        raise TypeError(f"batch must be an integer tensor, not {batch.dtype}")
    _check_vector("x", x)
    if batch.dim() != 1 or batch.shape[0] != x.shape[0]:
        raise ValueError(f"batch must be ({x.shape[0]},), got {tuple(batch.shape)}")
    ratio = _check_ratio(ratio)
    M.check_devices((("x", x), ("batch", batch)), _NO_CPU)
    N, dev = x.shape[0], x.device
    if N == 0:
        return torch.empty(0, dtype=torch.bool, device=dev), torch.zeros(0, dtype=torch.int64, device=dev)
    if N > MAX_ROWS:
        raise ValueError("more than 2^30 rows")
    batch = batch.long().contiguous()
    B = int(batch[-1]) + 1
    if not 1 <= B <= MAX_SEGMENTS:
        raise ValueError(f"{B} segments are outside the envelope 1..{MAX_SEGMENTS}")
    with torch.cuda.device(dev):
        indptr = torch.empty(B + 1, dtype=torch.int64, device=dev)
        L.check(L.load().gdr_seg_ptr_from_sorted(batch.data_ptr(), None, N, B, indptr.data_ptr(), M.stream()),
                "gdr_seg_ptr_from_sorted")
    return _select(x, ratio, indptr[1:], "top_k")


def top_p(x, ratio, offset):
    """The reference's top_p(x, ratio, offset)."""
    return _select(x, ratio, offset, "top_p")


# ---- gate and split -------------------------------------------------------------------------------------------------------

def _rows_backward(lib, mask, dest, N, Cn, g_sel, g_rest, n_sel, n_rest, feat, prob, gc_sel, gc_rest, coord_shape, coord_dtype,
                   need_feat, need_prob, need_coord, dev):
    """One launch of gdr_densify_rows_backward -> (grad_feat, grad_prob as (N,), grad_coord), None where not wanted."""
    g_sel = M.rows2d(g_sel)
    stride = M.stride0(g_sel)
    if g_rest is not None:                          # (the two sides share one row stride)
        g_sel, g_rest, stride = g_sel.contiguous(), g_rest.contiguous(), Cn
    grad_feat = torch.empty(N, Cn, dtype=feat.dtype, device=dev) if need_feat else None
    grad_prob = torch.empty(N, dtype=prob.dtype, device=dev) if need_prob else None
    grad_coord = torch.empty(coord_shape, dtype=coord_dtype, device=dev) if need_coord else None
    D = coord_shape[1] if need_coord else 0
    es = torch.empty(0, dtype=coord_dtype).element_size() if need_coord else 4
    if N:
        L.check(lib.gdr_densify_rows_backward(M.ptr(mask), M.ptr(dest), N, Cn, M.ptr_or_none_if_empty(g_sel),
                                              M.ptr_or_none_if_empty(g_rest), stride, _DTYPES[g_sel.dtype], n_sel, n_rest,
                                              feat.data_ptr(), M.stride0(feat), _DTYPES[feat.dtype], M.ptr(prob),
                                              _DTYPES[prob.dtype] if prob is not None else 0,
                                              M.ptr_or_none_if_empty(gc_sel) if need_coord else None,
                                              M.ptr_or_none_if_empty(gc_rest) if need_coord else None, D, es, M.ptr(grad_feat),
                                              M.ptr(grad_prob), M.ptr(grad_coord), M.stream()), "gdr_densify_rows_backward")
    return grad_feat, grad_prob, grad_coord


class _SteGate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, prob, mask, out_dtype):
        N, Cn = feat.shape
        dev = feat.device
        feat = M.rows2d(feat)
        with torch.cuda.device(dev):
            out = torch.empty(N, Cn, dtype=out_dtype, device=dev)
            if N:
                L.check(L.load().gdr_densify_gate_forward(feat.data_ptr(), M.stride0(feat), _DTYPES[feat.dtype], M.ptr(mask), N, Cn,
                                                          out.data_ptr(), _DTYPES[out_dtype], M.stream()), "gdr_densify_gate_forward")
        ctx.save_for_backward(feat, prob)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        feat, prob = ctx.saved_tensors
        N, Cn = feat.shape
        dev = feat.device
        with torch.cuda.device(dev):
            grad_feat, grad_prob, _ = _rows_backward(L.load(), None, None, N, Cn, grad_out, None, N, 0, feat,
                                                     prob.reshape(-1).contiguous(), None, None, None, None,
                                                     ctx.needs_input_grad[0], ctx.needs_input_grad[1], False, dev)
        return grad_feat, None if grad_prob is None else grad_prob.reshape(prob.shape), None, None


def ste_gate(feat, prob, mask=None):
    """feat (N, C), prob (N,) or (N, 1), mask None or (N,) bool -> (N, C) of promote_types(feat.dtype, prob.dtype): the value
    `feat` (MaskModule's `(feat - feat * prob).detach() + feat * prob`) or `feat * mask` (MaskResModule's), exactly; gradients
    grad_feat = prob * g and grad_prob[i] = sum_c feat[i, c] * g[i, c] (fp32 accumulation), in the dtypes of the inputs."""
    _check_rows("feat", feat)
    _check_vector("prob", prob)
    N = feat.shape[0]
    if prob.shape[0] != N:
        raise ValueError(f"prob must have {N} rows, got {tuple(prob.shape)}")
    named = [("feat", feat), ("prob", prob)]
    if mask is not None:
        _check_mask(mask, N)
        named.append(("mask", mask))
        mask = mask.contiguous()
    M.check_devices(named, _NO_CPU)
    return _SteGate.apply(feat, prob, mask, torch.promote_types(feat.dtype, prob.dtype))


class _SplitRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mask, coord, feat, prob, n_selected):
        N, Cn = feat.shape
        dev = feat.device
        feat, coord = M.rows2d(feat), coord.contiguous()
        out_dtype = feat.dtype if prob is None else torch.promote_types(feat.dtype, prob.dtype)
        lib = L.load()
        with torch.cuda.device(dev):
            dest = torch.empty(N, dtype=torch.int64, device=dev)
            count = torch.empty(1, dtype=torch.int64, device=dev)
            nbytes = lib.gdr_densify_split_bytes(N)
            if nbytes == 0:
                L.check(-1, "gdr_densify_split_bytes")
            ws, base, usable = M.workspace(nbytes, dev)
            L.check(lib.gdr_densify_split_scan(mask.data_ptr(), N, base, usable, dest.data_ptr(), count.data_ptr(), M.stream()),
                    "gdr_densify_split_scan")
            n_sel = int(count) if n_selected is None else n_selected      # (the one read-back: 8 bytes)
            n_rest = N - n_sel
            D = coord.shape[1]
            coord_sel, coord_rest = coord.new_empty(n_sel, D), coord.new_empty(n_rest, D)
            feat_sel = torch.empty(n_sel, Cn, dtype=out_dtype, device=dev)
            feat_rest = torch.empty(n_rest, Cn, dtype=out_dtype, device=dev)
            L.check(lib.gdr_densify_split_forward(mask.data_ptr(), dest.data_ptr(), N, Cn, feat.data_ptr(), M.stride0(feat),
                                                  _DTYPES[feat.dtype], M.ptr_or_none_if_empty(coord), D, coord.element_size(), n_sel,
                                                  n_rest, M.ptr_or_none_if_empty(feat_sel), M.ptr_or_none_if_empty(feat_rest),
                                                  _DTYPES[out_dtype], M.ptr_or_none_if_empty(coord_sel),
                                                  M.ptr_or_none_if_empty(coord_rest), M.stream()), "gdr_densify_split_forward")
        if not ctx.needs_input_grad[1]:
            ctx.mark_non_differentiable(coord_sel, coord_rest)
        ctx.save_for_backward(mask, dest, feat, prob)
        ctx.n_sel, ctx.n_rest, ctx.coord_shape, ctx.coord_dtype = n_sel, n_rest, coord.shape, coord.dtype
        return coord_sel, feat_sel, coord_rest, feat_rest

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_coord_sel, g_feat_sel, g_coord_rest, g_feat_rest):
        mask, dest, feat, prob = ctx.saved_tensors
        N, Cn = feat.shape
        dev = feat.device
        need_coord = ctx.needs_input_grad[1]
        with torch.cuda.device(dev):
            if need_coord:
                g_coord_sel, g_coord_rest = g_coord_sel.contiguous(), g_coord_rest.contiguous()
            grad_feat, grad_prob, grad_coord = _rows_backward(
                L.load(), mask, dest, N, Cn, g_feat_sel, g_feat_rest, ctx.n_sel, ctx.n_rest, feat,
                None if prob is None else prob.reshape(-1).contiguous(), g_coord_sel, g_coord_rest, ctx.coord_shape, ctx.coord_dtype,
                ctx.needs_input_grad[2], prob is not None and ctx.needs_input_grad[3], need_coord, dev)
        return None, grad_coord, grad_feat, None if grad_prob is None else grad_prob.reshape(prob.shape), None


def split_rows(mask, coord, feat, prob=None, n_selected=None):
    """mask (N,) bool, coord (N, D), feat (N, C), prob None or (N,) / (N, 1) -> (coord[mask], feat[mask], coord[~mask],
    feat[~mask]) with the row order kept.  With `prob` the gate ste_gate(feat, prob) is folded in: the values are feat's, in
    promote_types(feat.dtype, prob.dtype), and the backward gives grad_feat = prob * g and grad_prob = the row dot product from
    whichever side the row went to.  n_selected: the number of True rows if the caller knows it (no synchronisation then)."""
    _check_rows("feat", feat)
    N = feat.shape[0]
    _check_mask(mask, N)
    if not isinstance(coord, torch.Tensor):
        raise TypeError(f"coord must be a tensor, not {type(coord).__name__}")
    if coord.dim() != 2 or coord.shape[0] != N:
        raise ValueError(f"coord must be ({N}, D), got {tuple(coord.shape)}")
    if coord.element_size() not in (1, 2, 4, 8) or coord.dtype.is_complex:
        raise TypeError(f"coord must have elements of 1, 2, 4 or 8 bytes, not {coord.dtype}")
    named = [("feat", feat), ("mask", mask), ("coord", coord)]
    if prob is not None:
        _check_vector("prob", prob)
        if prob.shape[0] != N:
            raise ValueError(f"prob must have {N} rows, got {tuple(prob.shape)}")
        named.append(("prob", prob))
    if n_selected is not None:
        n_selected = int(n_selected)
        if not 0 <= n_selected <= N:
            raise ValueError(f"n_selected must lie in 0..{N}, got {n_selected}")
    M.check_devices(named, _NO_CPU)
    return _SplitRows.apply(mask.contiguous(), coord, feat, prob, n_selected)


# ---- the forwards of the reference's modules ------------------------------------------------------------------------------

def _non_leaf(self, prob, offset):
    if self.mask_sampling_type == "topk":
        return segment_top_k(prob, self.non_leaf_ratio, offset)
    return segment_top_p(prob, self.non_leaf_ratio, offset)


def mask_module_forward(self, point):
    """The forward of a MaskModule: reads `self.net`, `self.non_leaf_ratio` and `self.mask_sampling_type`.  Bind it with
    `autoencoder.MaskModule.forward = mask_module_forward`.  The reference's `assert torch.sum(non_leaf) == ...` holds by
    construction and is dropped; the one synchronisation is split_rows' read of the selected count."""
    Point = type(point)
    if self.non_leaf_ratio < 1.0:
        feat = point.feat
        prob = torch.sigmoid(self.net(feat))
        non_leaf, non_leaf_offset = _non_leaf(self, prob, point.offset)
        leaf_offset = point.offset - non_leaf_offset
        coord, feat, leaf_coord, leaf_feat = split_rows(non_leaf, point.coord, feat, prob)
        return Point(coord=coord, feat=feat, global_feat=point.global_feat, offset=non_leaf_offset, grid_size=point.grid_size,
                     leaf_point=Point(coord=leaf_coord, feat=leaf_feat, offset=leaf_offset, grid_size=point.grid_size))
    return Point(coord=point.coord, feat=point.feat, global_feat=point.global_feat, offset=point.offset, grid_size=point.grid_size,
                 leaf_point=Point(coord=point.coord, feat=point.feat, offset=point.offset, grid_size=point.grid_size))


def mask_res_module_forward(self, point):
    """The forward of a MaskResModule (`autoencoder.MaskResModule.forward = mask_res_module_forward`): reads `self.net`,
    `self.temperature`, `self.non_leaf_ratio` and `self.mask_sampling_type`; the segment softmax is the torch_geometric
    drop-in's.  No synchronisation."""
    from .segment import softmax as pyg_softmax

    update = dict.fromkeys(MASK_RES_KEYS)
    if self.non_leaf_ratio < 1.0:
        feat = point.feat
        raw_prob = self.net(feat)
        prob = pyg_softmax(src=raw_prob.to(torch.float32) / self.temperature, ptr=F.pad(point.offset, (1, 0), "constant", 0), dim=0)
        non_leaf, non_leaf_offset = _non_leaf(self, prob, point.offset)
        point.feat = ste_gate(feat, prob, non_leaf)
        update = {"raw_prob": raw_prob, "prob": prob, "non_leaf": non_leaf, "non_leaf_offset": non_leaf_offset,
                  "leaf": ~non_leaf, "leaf_offset": point.offset - non_leaf_offset}
    point.update(update)
    return point
