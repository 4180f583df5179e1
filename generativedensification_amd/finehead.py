"""The fine Gaussian head and the fine-set assembly on the MI355X (csrc/finehead.hip, include/gdr.h gdr_finehead_*): the stretch of
the reference's per-sample loop between the point decoder's last stage and the fine render.

    gaussian_head(feat, w1, b1, w2, b2, out_dtype=None)  -> attribute (N, P)
                                                   `feat2attr` of GaussianModule / GaussianResModule (lightning/point_decoder/
                                                   autoencoder.py): Linear(C, C), GELU, Linear(C, P), P = sh_dim + 1 + 3 + 4
    gaussian_module_forward(self, point)           GaussianModule.forward; bound with one line,
                                                   autoencoder.GaussianModule.forward = finehead.gaussian_module_forward
    gaussian_res_module_forward(self, point)       GaussianResModule.forward, bound the same way
    assemble_fine_gaussians(levels, centers_coarse, opacity_coarse, scaling_coarse, rotation_coarse, shs_fine, mask,
                            selected_pts_mask, sh_dim, opacity_shift, fine_scaling_shift, n_survivors=None)
                                                   -> (centers, shs, opacity, scaling, rotation): `_union_gaussians` and the five
                                                   concatenations behind it (lightning/network.py) for a single-sample union
    covers(module)                                 whether `module.feat2attr` is the one layer list served
    in_envelope(rows, C, sh_dim)                   whether the head's kernels serve this shape

The head.  feat is (N, C) float32, float16 or bfloat16 and its dtype is the compute dtype; the parameters are in nn.Linear's
layout, w1 (C, C), b1 (C,), w2 (P, C), b2 (P,), each of any of the three dtypes, rounded to the compute dtype by the pack kernel
and in the epilogues (what autocast's cast does, without a tensor of the rounded parameter).  GELU is torch's default, exact
form.  z1 and the hidden row are rounded to the compute dtype where torch rounds them, GELU and its derivative are evaluated in
float32 (float64 for float32 rows) from the rounded z1, sums are float32 (float64 for float32 rows).  out_dtype None returns the
compute dtype (the reference's `point.attribute`); torch.float32 stores the last layer's sum without a 16-bit rounding.  The hidden
row never leaves the workgroup: one launch plus the pack launch.  feat's rows are read in place when dense from a 16-byte aligned
base; anything else is made so with one copy.
Autocast: Linear's rule.  Under an enabled CUDA autocast a float32 feat is first cast to the autocast dtype; the Function itself
runs with autocast disabled.
Autograd: once differentiable; feat's rows and the parameters are saved, z1 and the hidden row are recomputed in the backward
(GELU' from the same rounded z1).  grad_x has feat's dtype; parameter gradients come back in the parameters' dtypes, summed in a
fixed order (slab partials plus a fold) and rounded once.  A gradient nobody needs is not launched: frozen parameters launch no
fold and write no partial sums, a feat without requires_grad gets no grad_x store.  A None upstream gradient is zeros without a
fill.  Works under no_grad and torch.autograd.functional.vjp.

The assembly.  levels is a list of (coord (n, 3) float32, attribute (n, P)) per decoder level, in order, optionally
(coord, attribute, offset); a multi-sample offset raises NotImplementedError.  The coarse tensors are (Nc, 3 | 1 | 3 | 4) float32,
shs_fine (n_masked, sh_dim / 3, 3) float32, mask (Nc,) bool, selected_pts_mask (n_masked,) bool.  The results are five dense
float32 tensors whose values are bitwise those of the reference's lines: the level rows (centers = coord, shs, opacity + shift,
scaling + shift, rotation, each converted to float32 before the add), then the survivors, the masked rows that were not selected,
copied from the coarse tensors and shs_fine.  One scan of the two masks (3 launches) and one launch that writes all five outputs.
n_survivors is the number of survivor rows, which the caller knows (n_masked - k_num, or 0 when everything is selected): given, the
call never synchronises; None reads the count back once (8 bytes).  A wrong n_survivors behaves as densify.split_rows with a
wrong n_selected: rows whose destination lies beyond it are dropped, rows nothing maps to are unspecified, nothing is written
outside the outputs.  The backward is one launch: level coords and attributes get their gradients (the attribute's in its dtype),
the coarse tensors and shs_fine dense gradients whose rows are their survivor's or zero.  The masks get no gradient.

The kernels use no atomics (two calls are bitwise equal).  GPU tensors only (no CPU fallback).  Wrong dtypes raise TypeError,
shapes outside the envelope ValueError, all before any launch.  Envelope: C a multiple of 8 in 8..MAX_C, the hidden width C,
sh_dim in (3, 12, 27, 48), every row count below 2^31, at most MAX_LEVELS levels.  Empty inputs return empty tensors without loading
the library.  Non-finite inputs are memory-safe and otherwise unspecified.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from . import _marshal as M

__all__ = ["gaussian_head", "gaussian_module_forward", "gaussian_res_module_forward", "assemble_fine_gaussians", "covers", "in_envelope",
           "backward_step", "HEAD_BACKEND", "MAX_C", "TILE_ROWS", "SLAB_MIN", "MAX_LEVELS", "SH_DIMS"]

MAX_C = L.GDR_FINEHEAD_MAX_C
TILE_ROWS = L.GDR_FINEHEAD_TILE_ROWS          # rows of one workgroup of the forward
SLAB_MIN = L.GDR_FINEHEAD_SLAB_MIN            # the parameter gradients cut one slab of rows per this many, 256 at most
MAX_LEVELS = L.GDR_FINEHEAD_MAX_LEVELS
SH_DIMS = (3, 12, 27, 48)

# the path of the two bound forwards: "hip" (this module wherever it covers the module and the shape) or "torch" (the
# reference's lines).  "torch" is the default: at the base config's C = 256 the fused head is slower than torch's two GEMMs in
# training (scripts/bench_finehead.py, BASELINE §4-finehead: bf16 forward + backward 1.9 ms against 0.6 ms at 76 800 rows), and
# the project's rule ships "hip" only where it measured faster.  gaussian_head itself always runs the kernels.
HEAD_BACKEND = "torch"

_DTYPES = M.DTYPES
_dense = M.dense
_NO_CPU = "the HIP fine head runs on ROCm/HIP tensors only (no CPU fallback)"


def in_envelope(rows, C, sh_dim):
    """whether the head's kernels serve this shape"""
    return 8 <= C <= MAX_C and C % 8 == 0 and sh_dim in SH_DIMS and 0 <= rows < 1 << 31


def backward_step(dtype, C, sh_dim):
    """the rows a workgroup of the head's backward takes per step (what fits LDS: 64, 32 or 16)"""
    step = L.load().gdr_finehead_backward_step(_DTYPES[dtype], C, sh_dim)
    if step == 0:
        L.check(-1, "gdr_finehead_backward_step")
    return step


def _rows(x):
    """x (N, C) dense from a 16-byte aligned base: x itself where it is so already, one copy otherwise"""
    return M.dense_aligned(x)


def _workspace(lib, what, dt, rows, C, sh_dim, dev):
    return M.queried_workspace(lib.gdr_finehead_workspace_bytes, "gdr_finehead_workspace_bytes", dev, what, dt, rows, C, sh_dim)


def _packed(lib, w1, w2, backward, dt, C, sh_dim, dev):
    what = L.GDR_FINEHEAD_WS_PACKED_BACKWARD if backward else L.GDR_FINEHEAD_WS_PACKED_FORWARD
    ws, base, _ = _workspace(lib, what, dt, 0, C, sh_dim, dev)
    L.check(lib.gdr_finehead_pack(w1.data_ptr(), _DTYPES[w1.dtype], w2.data_ptr(), _DTYPES[w2.dtype], C, sh_dim, int(backward), base, dt,
                                  M.stream()), "gdr_finehead_pack")
    return ws, base


class _Head(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, out_dtype):
        dev = x.device
        rows = _rows(x)
        n, Cc = rows.shape
        P = w2.shape[0]
        params = [_dense(t) for t in (w1, b1, w2, b2)]
        with torch.cuda.device(dev):
            out = torch.empty(n, P, dtype=out_dtype, device=dev)
            if n:
                lib, dt = L.load(), _DTYPES[x.dtype]
                ws, base = _packed(lib, params[0], params[2], False, dt, Cc, P - 8, dev)
                L.check(lib.gdr_finehead_forward(rows.data_ptr(), dt, base, params[1].data_ptr(), _DTYPES[params[1].dtype],
                                                 params[3].data_ptr(), _DTYPES[params[3].dtype], n, Cc, P - 8, out.data_ptr(),
                                                 _DTYPES[out_dtype], M.stream()), "gdr_finehead_forward")
        ctx.save_for_backward(rows, *params)
        ctx.set_materialize_grads(False)      # a None upstream gradient stays None: the kernel reads it as zeros
        ctx.meta = [(t.dtype, t.shape) for t in (w1, b1, w2, b2)]
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        rows, w1, b1, w2, b2 = ctx.saved_tensors
        n, Cc = rows.shape
        sh_dim = w2.shape[0] - 8
        dev, dt = rows.device, _DTYPES[rows.dtype]
        need = ctx.needs_input_grad
        need_x, need_p = need[0], list(need[1:5])
        if g is not None:
            g = _dense(g if g.dtype in _DTYPES else g.float())
        grad_x = None
        grads = [None] * 4
        with torch.cuda.device(dev):
            if need_x:
                grad_x = torch.empty_like(rows)
            for i, (dtype, shape) in enumerate(ctx.meta):
                if need_p[i]:
                    grads[i] = (torch.empty if n else torch.zeros)(shape, dtype=dtype, device=dev)
            if n and (need_x or any(need_p)):
                lib = L.load()
                pws, pbase = _packed(lib, w1, w2, True, dt, Cc, sh_dim, dev)
                ws, base, usable = (_workspace(lib, L.GDR_FINEHEAD_WS_PARTIALS, dt, n, Cc, sh_dim, dev) if any(need_p) else (None, None, 0))
                L.check(lib.gdr_finehead_backward(rows.data_ptr(), dt, pbase, b1.data_ptr(), _DTYPES[b1.dtype], n, Cc, sh_dim, M.ptr(g),
                                                  _DTYPES[g.dtype] if g is not None else dt, M.ptr(grad_x), base, usable, M.stream()),
                        "gdr_finehead_backward")
                if any(need_p):
                    out = [a for t in grads for a in (M.ptr(t), _DTYPES[t.dtype] if t is not None else dt)]
                    L.check(lib.gdr_finehead_fold(base, usable, dt, n, Cc, sh_dim, *out, M.stream()), "gdr_finehead_fold")
        return (grad_x, *grads, None)


def _check_head(feat, params, out_dtype):
    named = [("feat", feat)] + list(zip(("w1", "b1", "w2", "b2"), params))
    for name, t in named:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, not {type(t).__name__}")
        if t.dtype not in _DTYPES:
            raise TypeError(f"{name} must be float32, float16 or bfloat16, not {t.dtype}")
    if out_dtype is not None and out_dtype is not torch.float32:
        raise TypeError(f"out_dtype must be None (the compute dtype) or torch.float32, not {out_dtype}")
    if feat.dim() != 2:
        raise ValueError(f"feat is (N, C), got {tuple(feat.shape)}")
    n, Cc = feat.shape
    w1, b1, w2, b2 = params
    P = w2.shape[0] if w2.dim() == 2 else -1
    for name, t, shape in (("w1", w1, (Cc, Cc)), ("b1", b1, (Cc,)), ("w2", w2, (P, Cc)), ("b2", b2, (P,))):
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {shape} (the hidden width equals C = {Cc}), got {tuple(t.shape)}")
    if not in_envelope(n, Cc, P - 8):
        raise ValueError(f"rows = {n}, C = {Cc}, P = {P} are outside the envelope: C a multiple of 8 in 8..{MAX_C}, P - 8 one of {SH_DIMS}, "
                         "rows below 2^31")
    for name, t in named:
        if not t.is_cuda:
            raise RuntimeError(_NO_CPU)
    for name, t in named:
        if t.device != feat.device:
            raise RuntimeError(f"{name} must live on feat's device ({feat.device}), not {t.device}")


def gaussian_head(feat, w1, b1, w2, b2, out_dtype=None):
    """feat (N, C) and feat2attr's parameters in nn.Linear's layout -> attribute (N, P): Linear(C, C), GELU, Linear(C, P) in one
    launch; out_dtype None is feat's (compute) dtype, torch.float32 the unrounded sum of the last layer."""
    _check_head(feat, (w1, b1, w2, b2), out_dtype)
    if feat.dtype == torch.float32 and torch.is_autocast_enabled("cuda"):
        feat = feat.to(torch.get_autocast_dtype("cuda"))
    with torch.autocast("cuda", enabled=False):
        return _Head.apply(feat, w1, b1, w2, b2, feat.dtype if out_dtype is None else out_dtype)


def covers(module):
    """whether `module.feat2attr` is exactly Sequential(Linear(C, C), GELU(approximate='none'), Linear(C, P)) with biases"""
    mlp = getattr(module, "feat2attr", None)
    if not isinstance(mlp, torch.nn.Sequential) or len(mlp) != 3:
        return False
    if any(type(m) is not k for m, k in zip(mlp, (torch.nn.Linear, torch.nn.GELU, torch.nn.Linear))):
        return False
    l1, act, l2 = mlp
    if l1.bias is None or l2.bias is None or getattr(act, "approximate", "none") != "none":
        return False
    return l1.out_features == l1.in_features == l2.in_features and l2.out_features > 8


def _params(module):
    mlp = module.feat2attr
    return (mlp[0].weight, mlp[0].bias, mlp[2].weight, mlp[2].bias)


def _feat2attr(module, feat):
    if HEAD_BACKEND not in ("torch", "hip"):
        raise ValueError(f"finehead.HEAD_BACKEND must be 'torch' or 'hip', not {HEAD_BACKEND!r}")
    if HEAD_BACKEND == "hip" and covers(module) and feat.dim() == 2:
        l1, l2 = module.feat2attr[0], module.feat2attr[2]
        if feat.shape[1] == l1.in_features and feat.dtype in _DTYPES and in_envelope(feat.shape[0], l1.in_features, l2.out_features - 8):
            return gaussian_head(feat, *_params(module))
    return module.feat2attr(feat)


def gaussian_module_forward(self, point):
    """GaussianModule.forward of the reference: reads self.feat2attr and point.leaf_point.feat and updates point.leaf_point with
    `attribute`, from one launch of csrc/finehead.hip wherever `covers` and `in_envelope` hold and HEAD_BACKEND is "hip"; anywhere
    else it is the reference's lines."""
    attribute = _feat2attr(self, point.leaf_point.feat)
    point.leaf_point.update({"attribute": attribute})
    return point


def gaussian_res_module_forward(self, point):
    """GaussianResModule.forward of the reference: as gaussian_module_forward on point.feat and point itself; the residual
    `point.attribute + attribute` (self.enable_residual_attribute and not self.is_first) stays torch's."""
    attribute = _feat2attr(self, point.feat)
    if self.enable_residual_attribute and not self.is_first:
        attribute = point.attribute + attribute
    point.update({"attribute": attribute})
    return point


# ---- the assembly ---------------------------------------------------------------------------------------------------------------------

_WIDTHS = lambda sh_dim: (3, sh_dim, 1, 3, 4)      # noqa: E731  centers, shs, opacity, scaling, rotation


def _pointers(tensors):
    """a host array of device pointers (NULL for None and for empty tensors), or None for no tensors"""
    if not tensors:
        return None
    return (C.c_void_p * len(tensors))(*[None if t is None or t.numel() == 0 else t.data_ptr() for t in tensors])


def _scan(lib, mask, selected, dev):
    """the rank tables of the two masks -> (rank_masked, row_of_masked, rank_rest, masked_of_rest, count); 3 launches"""
    Nc, n_masked = mask.shape[0], selected.shape[0]
    i32 = dict(dtype=torch.int32, device=dev)
    tables = [torch.empty(Nc, **i32)] + [torch.empty(n_masked, **i32) for _ in range(3)]
    count = torch.empty(2, dtype=torch.int64, device=dev)
    nbytes = lib.gdr_finehead_scan_bytes(Nc, n_masked)
    if nbytes == 0:
        L.check(-1, "gdr_finehead_scan_bytes")
    ws, base, usable = M.workspace(nbytes, dev)
    L.check(lib.gdr_finehead_scan(M.ptr_or_none_if_empty(mask.view(torch.uint8)), Nc, M.ptr_or_none_if_empty(selected.view(torch.uint8)), n_masked,
                                  base, usable, *[M.ptr_or_none_if_empty(t) for t in tables], count.data_ptr(), M.stream()), "gdr_finehead_scan")
    return (*tables, count)


def _assemble_into(lib, coords, attrs, coarse, shs_fine, row_of_masked, masked_of_rest, n_rest, sh_dim, opacity_shift, scaling_shift, outs):
    """the one launch of the forward: writes sum(level rows) + n_rest rows of each of `outs` (dense float32, in the order centers,
    shs, opacity, scaling, rotation)"""
    level_rows = (C.c_int64 * max(len(coords), 1))(*[t.shape[0] for t in coords])
    attr_dt = _DTYPES[attrs[0].dtype] if attrs else _DTYPES[torch.float32]
    L.check(lib.gdr_finehead_assemble(len(coords), _pointers(coords), _pointers(attrs), level_rows, attr_dt, sh_dim,
                                      *[M.ptr_or_none_if_empty(t) for t in coarse], coarse[0].shape[0], M.ptr_or_none_if_empty(shs_fine),
                                      shs_fine.shape[0], M.ptr_or_none_if_empty(row_of_masked), M.ptr_or_none_if_empty(masked_of_rest), n_rest,
                                      opacity_shift, scaling_shift, *[t.data_ptr() for t in outs], M.stream()), "gdr_finehead_assemble")


class _Assemble(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sh_dim, opacity_shift, scaling_shift, n_survivors, mask, selected, shs_fine, centers_c, opacity_c, scaling_c, rotation_c,
                *levels):
        dev = centers_c.device
        coords, attrs = [_dense(t) for t in levels[0::2]], [_dense(t) for t in levels[1::2]]
        coarse = [_dense(t) for t in (centers_c, opacity_c, scaling_c, rotation_c)]
        fine = _dense(shs_fine).view(shs_fine.shape[0], sh_dim)
        mask, selected = _dense(mask), _dense(selected)
        Nc, n_masked, rows = mask.shape[0], selected.shape[0], sum(t.shape[0] for t in coords)
        tables = None
        with torch.cuda.device(dev):
            lib = L.load() if rows or n_masked else None
            n_rest = 0
            if n_masked:
                tables = _scan(lib, mask, selected, dev)
                n_rest = int(tables[4][1:2].item()) if n_survivors is None else n_survivors      # the one read-back, 8 bytes
            total = rows + n_rest
            outs = [torch.empty(total, w, dtype=torch.float32, device=dev) for w in _WIDTHS(sh_dim)]
            if total:
                _assemble_into(lib, coords, attrs, coarse, fine, tables[1] if tables else None, tables[3] if tables else None, n_rest, sh_dim,
                               opacity_shift, scaling_shift, outs)
        ctx.save_for_backward(*((tables[0], tables[2]) if tables else ()))
        ctx.set_materialize_grads(False)
        ctx.meta = (sh_dim, n_rest, Nc, n_masked, [t.shape[0] for t in coords], attrs[0].dtype if attrs else torch.float32, shs_fine.shape)
        outs[1] = outs[1].view(total, sh_dim // 3, 3)
        return tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *gs):
        sh_dim, n_rest, Nc, n_masked, level_rows, attr_dtype, fine_shape = ctx.meta
        ranks = ctx.saved_tensors
        need = ctx.needs_input_grad
        n_levels = len(level_rows)
        ref = next((g for g in gs if g is not None), None)
        if ref is None:
            return (None,) * (11 + 2 * n_levels)
        dev = ref.device
        gs = [None if g is None else _dense(g if g.dtype == torch.float32 else g.float()) for g in gs]
        f32 = dict(dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            g_fine = torch.empty(n_masked, sh_dim, **f32) if need[6] else None
            # (without masked rows there was no scan and no coarse row survives: zeros, and nothing for the kernel to write)
            g_coarse = [(torch.empty if ranks else torch.zeros)(Nc, w, **f32) if need[7 + i] else None for i, w in enumerate((3, 1, 3, 4))]
            g_coord = [torch.empty(n, 3, **f32) if need[11 + 2 * l] else None for l, n in enumerate(level_rows)]
            g_attr = [torch.empty(n, sh_dim + 8, dtype=attr_dtype, device=dev) if need[12 + 2 * l] else None for l, n in enumerate(level_rows)]
            coarse_out = g_coarse if ranks else [None] * 4
            if any(t is not None and t.numel() for t in [g_fine] + coarse_out + g_coord + g_attr):
                rows_arr = (C.c_int64 * max(n_levels, 1))(*level_rows)
                L.check(L.load().gdr_finehead_assemble_backward(
                    n_levels, rows_arr, _DTYPES[attr_dtype], sh_dim, *[M.ptr_or_none_if_empty(g) for g in gs],
                    M.ptr_or_none_if_empty(ranks[0]) if ranks else None, M.ptr_or_none_if_empty(ranks[1]) if ranks else None, Nc, n_masked, n_rest,
                    _pointers(g_coord), _pointers(g_attr), *[M.ptr_or_none_if_empty(t) for t in coarse_out], M.ptr_or_none_if_empty(g_fine),
                    M.stream()), "gdr_finehead_assemble_backward")
        if g_fine is not None:
            g_fine = g_fine.view(fine_shape)
        levels = [t for pair in zip(g_coord, g_attr) for t in pair]
        return (None, None, None, None, None, None, g_fine, *g_coarse, *levels)


def _check_assembly(levels, coarse, shs_fine, mask, selected, sh_dim, n_survivors):
    if isinstance(sh_dim, bool) or not isinstance(sh_dim, int):
        raise TypeError(f"sh_dim must be an int, not {type(sh_dim).__name__}")
    if n_survivors is not None and (isinstance(n_survivors, bool) or not isinstance(n_survivors, int)):
        raise TypeError(f"n_survivors must be an int or None, not {type(n_survivors).__name__}")
    levels = [tuple(level) for level in levels]
    if any(len(level) not in (2, 3) for level in levels):
        raise TypeError("a level is (coord, attribute) or (coord, attribute, offset)")
    named = ([(f"levels[{l}].coord", level[0], torch.float32) for l, level in enumerate(levels)] +
             [(f"levels[{l}].attribute", level[1], None) for l, level in enumerate(levels)] +
             list(zip(("centers_coarse", "opacity_coarse", "scaling_coarse", "rotation_coarse"), coarse, (torch.float32,) * 4)) +
             [("shs_fine", shs_fine, torch.float32), ("mask", mask, torch.bool), ("selected_pts_mask", selected, torch.bool)])
    for name, t, dtype in named:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, not {type(t).__name__}")
        if dtype is None and t.dtype not in _DTYPES:
            raise TypeError(f"{name} must be float32, float16 or bfloat16, not {t.dtype}")
        if dtype is not None and t.dtype != dtype:
            raise TypeError(f"{name} must be {dtype}, not {t.dtype}")
    if len({level[1].dtype for level in levels}) > 1:
        raise TypeError("the levels' attributes must share one dtype")
    if sh_dim not in SH_DIMS:
        raise ValueError(f"sh_dim = {sh_dim} is outside the envelope: one of {SH_DIMS}")
    if len(levels) > MAX_LEVELS:
        raise ValueError(f"{len(levels)} levels are outside the envelope: at most {MAX_LEVELS}")
    for l, level in enumerate(levels):
        if len(level) == 3 and level[2] is not None and level[2].numel() > 1:
            raise NotImplementedError("assemble_fine_gaussians serves the single-sample union of Network.forward; a multi-sample `offset` "
                                      "needs the sort of _union_gaussians' group_cat, which is not implemented")
        n = level[0].shape[0] if level[0].dim() else -1
        if tuple(level[0].shape) != (n, 3) or tuple(level[1].shape) != (n, sh_dim + 8):
            raise ValueError(f"level {l} must be coord (n, 3) and attribute (n, {sh_dim + 8}), got {tuple(level[0].shape)} and {tuple(level[1].shape)}")
    Nc = mask.shape[0] if mask.dim() == 1 else -1
    n_masked = selected.shape[0] if selected.dim() == 1 else -1
    if Nc < 0 or n_masked < 0:
        raise ValueError(f"mask is (Nc,) and selected_pts_mask (n_masked,), got {tuple(mask.shape)} and {tuple(selected.shape)}")
    for (name, t, _), w in zip(named[2 * len(levels):], (3, 1, 3, 4)):
        if tuple(t.shape) != (Nc, w):
            raise ValueError(f"{name} must be ({Nc}, {w}), got {tuple(t.shape)}")
    if tuple(shs_fine.shape) != (n_masked, sh_dim // 3, 3):
        raise ValueError(f"shs_fine must be ({n_masked}, {sh_dim // 3}, 3), got {tuple(shs_fine.shape)}")
    if n_masked > Nc:
        raise ValueError(f"n_masked = {n_masked} exceeds Nc = {Nc}")
    if n_survivors is not None and not 0 <= n_survivors <= n_masked:
        raise ValueError(f"n_survivors = {n_survivors} must lie in 0..n_masked = {n_masked}")
    rows = sum(level[0].shape[0] for level in levels) + n_masked
    if Nc >= 1 << 31 or rows >= 1 << 31:
        raise ValueError("Nc, n_masked and the output row count must be below 2^31")
    for name, t, _ in named:
        if not t.is_cuda:
            raise RuntimeError(_NO_CPU)
    for name, t, _ in named:
        if t.device != mask.device:
            raise RuntimeError(f"{name} must live on mask's device ({mask.device}), not {t.device}")
    return levels


def assemble_fine_gaussians(levels, centers_coarse, opacity_coarse, scaling_coarse, rotation_coarse, shs_fine, mask, selected_pts_mask, sh_dim,
                            opacity_shift, fine_scaling_shift, n_survivors=None):
    """-> (centers (T, 3), shs (T, sh_dim / 3, 3), opacity (T, 1), scaling (T, 3), rotation (T, 4)), dense float32: the rows of every
    level, then the masked coarse Gaussians that were not selected.  Bitwise the reference's `_union_gaussians` and its five
    concatenations for a single-sample union."""
    coarse = (centers_coarse, opacity_coarse, scaling_coarse, rotation_coarse)
    levels = _check_assembly(levels, coarse, shs_fine, mask, selected_pts_mask, sh_dim, n_survivors)
    flat = [t for level in levels for t in level[:2]]
    with torch.autocast("cuda", enabled=False):
        return _Assemble.apply(sh_dim, float(opacity_shift), float(fine_scaling_shift), n_survivors, mask, selected_pts_mask, shs_fine, *coarse, *flat)
