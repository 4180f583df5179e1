"""float64 restatement of generativedensification_amd/block.py (csrc/block.hip): the residual junction of the point decoder's
Block with the closed-form gradients the kernels implement (numpy), the torch composition the GPU tests compare with, and a
stand-in Block with the reference's child names (a recorded `state_dict` loads with strict=True) whose `restated_forward` is
Block.forward written from its arithmetic.  The attention comes from tests/serattn_ref.py / attn_ref.py, the submanifold conv
from tests/subm_ref.py's table model.  tests/test_block_cpu.py holds the closed forms against autograd of the torch
composition in float64; tests/test_gpu_block.py holds the kernels against all of it.

A norm spec is None, ("ln", weight_or_None, bias_or_None, eps) or ("ada", scale, eps).  The truth has no intermediate
rounding: the roundings the junction makes where torch makes them are part of what the accuracy bar measures, for both
candidates alike."""
import math

import numpy as np

import norm_ref as NR

to_dtype, half_ulp = NR.to_dtype, NR.half_ulp
MUTANTS = ("j1_branch_not_normed", "j2_norm_of_branch", "j3_skip_is_input")       # one per junction of the Block


# ---- the junction in numpy ------------------------------------------------------------------------------------------------

def _a(x):
    return None if x is None else np.asarray(x, dtype=np.float64)


def norm_forward(spec, x, offset):
    x = _a(x)
    if spec is None:
        return x
    if spec[0] == "ada":
        return NR.ada_layer_norm(x, spec[1], offset, spec[2])
    _, w, b, eps = spec
    xh, _ = NR._layer_norm(x, eps)
    return xh * (1.0 if w is None else _a(w)) + (0.0 if b is None else _a(b))


def norm_backward(spec, x, offset, g):
    """(dx, dw, db): the gradient at the norm's input, at its weight / scale and at its bias (None where there is none)"""
    x, g = _a(x), _a(g)
    if spec is None:
        return g, None, None
    if spec[0] == "ada":
        dx, dscale = NR.ada_layer_norm_grad(x, spec[1], offset, g, spec[2])
        return dx, dscale, None
    _, w, b, eps = spec
    xh, rstd = NR._layer_norm(x, eps)
    dx = NR._layer_norm_grad(g * (1.0 if w is None else _a(w)), xh, rstd)
    return dx, (None if w is None else (g * xh).sum(0)), (None if b is None else g.sum(0))


def junction(skip, branch, keep=None, pre=None, post=None, offset=None):
    """(y, n or None)"""
    b = norm_forward(pre, branch, offset)
    if keep is not None:
        b = _a(keep).reshape(-1, 1) * b
    y = _a(skip) + b
    return y, (None if post is None else norm_forward(post, y, offset))


def junction_grad(skip, branch, keep, pre, post, offset, grad_y, grad_n):
    """{"skip", "branch", "pre_w", "pre_b", "post_w", "post_b"}; a None upstream gradient is zeros"""
    y, _ = junction(skip, branch, keep, pre, post, offset)
    dy = np.zeros_like(y) if grad_y is None else _a(grad_y).copy()
    post_w = post_b = None
    if post is not None:
        d, post_w, post_b = norm_backward(post, y, offset, np.zeros_like(y) if grad_n is None else grad_n)
        dy = dy + d
    db = dy if keep is None else _a(keep).reshape(-1, 1) * dy
    dbranch, pre_w, pre_b = norm_backward(pre, branch, offset, db)
    return {"skip": dy, "branch": dbranch, "pre_w": pre_w, "pre_b": pre_b, "post_w": post_w, "post_b": post_b}


# ---- the torch composition ------------------------------------------------------------------------------------------------

def torch_ada(feat, scale, offset, eps=1e-5):
    """gather(scale) * layer_norm(feat) without a read-back; rows at or behind offset[-1] are zero"""
    import torch
    import torch.nn.functional as F

    seg = torch.searchsorted(offset, torch.arange(feat.shape[0], device=feat.device), right=True)
    padded = torch.cat([scale, scale.new_zeros(1, scale.shape[1])])
    return padded.index_select(0, seg) * F.layer_norm(feat, feat.shape[1:], eps=eps)


def torch_norm(spec, x, offset):
    import torch.nn.functional as F

    if spec is None:
        return x
    if spec[0] == "ada":
        return torch_ada(x, spec[1], offset, spec[2])
    return F.layer_norm(x, x.shape[1:], spec[1], spec[2], spec[3])


def torch_junction(skip, branch, keep=None, pre=None, post=None, offset=None):
    """the reference's lines: shortcut + drop_path(norm(branch)), then the next norm"""
    b = torch_norm(pre, branch, offset)
    if keep is not None:
        b = b * keep.reshape(-1, 1)
    y = skip + b
    return y, (None if post is None else torch_norm(post, y, offset))


# ---- a Block with the reference's child names -----------------------------------------------------------------------------

class Point(dict):
    """the attribute-and-key access of the reference's point"""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None

    __setattr__ = dict.__setitem__


def point_of(data, dtype=None, device="cpu", grad=False):
    """the point of block_cases.block_point's arrays, in `dtype` (default float64) on `device`"""
    import torch

    from generativedensification_amd.sparse_conv import SparseConvTensor

    dtype = dtype or torch.float64

    feat = to_dtype(data["feat"], dtype).to(device).requires_grad_(grad)
    sparse = SparseConvTensor(feat, torch.from_numpy(data["indices"]).to(device), data["spatial_shape"], data["batch_size"])
    return Point(feat=feat, sparse_conv_feat=sparse, offset=torch.from_numpy(data["offset"]).to(device),
                 global_feat=to_dtype(data["global_feat"], dtype).to(device),
                 serialized_order=torch.from_numpy(data["serialized_order"]).to(device),
                 serialized_inverse=torch.from_numpy(data["serialized_inverse"]).to(device))


def attention_forward(self, point):
    """SerializedAttention.forward restated over tests/serattn_ref.py (exact arithmetic in the module's dtype, CPU)"""
    import torch

    import attn_ref as AR
    import serattn_ref as SR

    pad, unpad, cu = AR.padded_patches(point.offset.tolist(), self.patch_size)
    order = point.serialized_order[self.order_index][pad]
    inverse = unpad[point.serialized_inverse[self.order_index]]
    feat = SR.forward(self.qkv(point.feat), order, inverse, [int(c) for c in cu], self.num_heads, self.scale)
    point.feat = self.proj_drop(self.proj(feat))
    return point


def make_block(channels, num_heads, patch_size, norm="ln", global_channels=24, drop_path=0.0, proj_drop=0.0, pre_norm=True,
               conv="table", seed=0, ada_forward=None, attn_forward=None, segment_norm=False):
    """A module that has what block.block_forward reads, under the reference's child names: cpe = (conv, Linear, norm), norm1,
    attn (qkv, proj), norm2, mlp = (MLP(fc1, act, fc2, drop)), drop_path, in containers that dispatch as the reference's
    PointSequential does.  norm: "ln" (nn.LayerNorm without affine, what Network builds), "affine" (nn.LayerNorm) or "ada" (a
    LayerNorm without affine with an `affine` Linear child, called with the point's global_feat and offset).  conv: "table"
    (tests/subm_ref.py's table model through autograd: any dtype, CPU) or "hip" (the product's spconv drop-in).
    `ada_forward(self, feat, global_feat, offset)` and `attn_forward(self, point)` are bound onto the norm and attention
    classes; the defaults are the torch composition and the restatement above.  Parameters come from a seeded numpy draw."""
    import torch
    from torch import nn

    import serattn_ref as SR
    import subm_ref as SM
    from generativedensification_amd import sparse_conv as SC

    class AdaNorm(nn.LayerNorm):
        def __init__(self, c):
            super().__init__(c, elementwise_affine=False)
            self.affine = nn.Linear(global_channels, c)

        forward = ada_forward or (lambda self, feat, global_feat, offset: torch_ada(feat, self.affine(global_feat), offset, self.eps))

    class SegmentNorm(nn.Module):
        """the surface of the reference's own segment-wise LayerNorm(input, offsets): not an nn.LayerNorm"""

        def __init__(self, c):
            super().__init__()
            self.eps, self.elementwise_affine, self.normalized_shape = 1e-5, False, (c,)

        def forward(self, feat, offsets):
            raise NotImplementedError

    class TableConv(SC.SparseModule):
        def __init__(self, cin, cout):
            super().__init__()
            self.weight = nn.Parameter(torch.empty(cout, 3, 3, 3, cin))
            self.bias = nn.Parameter(torch.empty(cout))

        def forward(self, sp):
            nbr, _ = SM.table_model(sp.indices.cpu().numpy(), sp.spatial_shape, sp.batch_size, (3, 3, 3))
            f, wk = sp.features, self.weight.reshape(self.weight.shape[0], -1, self.weight.shape[-1])
            out = self.bias.unsqueeze(0).expand(f.shape[0], -1)
            nb = torch.as_tensor(nbr).long()
            for k in range(nb.shape[0]):
                rows = torch.nonzero(nb[k] >= 0).squeeze(1)
                if rows.numel():
                    out = out.index_add(0, rows, f.index_select(0, nb[k, rows]) @ wk[:, k, :].t())
            return sp.replace_feature(out)

    class PointSeq(nn.Module):
        takes_point = True

        def __init__(self, *mods):
            super().__init__()
            for i, m in enumerate(mods):
                self.add_module(str(i), m)

        def __getitem__(self, i):
            return list(self._modules.values())[i]

        def __len__(self):
            return len(self._modules)

        def forward(self, point):
            for m in self._modules.values():
                if getattr(m, "takes_point", False):
                    point = m(point)
                elif SC.is_spconv_module(m):
                    point.sparse_conv_feat = m(point.sparse_conv_feat)
                    point.feat = point.sparse_conv_feat.features
                elif isinstance(m, SegmentNorm):
                    point.feat = m(point.feat, point.offset)
                elif isinstance(m, AdaNorm):
                    point.feat = m(point.feat, point.global_feat, point.offset)
                else:
                    point.feat = m(point.feat)
                    if "sparse_conv_feat" in point.keys():
                        point.sparse_conv_feat = point.sparse_conv_feat.replace_feature(point.feat)
            return point

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

    class MLP(nn.Module):
        def __init__(self, c, hidden):
            super().__init__()
            self.fc1, self.act, self.fc2, self.drop = nn.Linear(c, hidden), nn.GELU(), nn.Linear(hidden, c), nn.Dropout(proj_drop)

        def forward(self, x):
            return self.drop(self.fc2(self.drop(self.act(self.fc1(x)))))

    class Attention(SR.Module):
        takes_point = True
        forward = attn_forward or attention_forward

    def norm_layer(c):
        if segment_norm:
            return SegmentNorm(c)
        return AdaNorm(c) if norm == "ada" else nn.LayerNorm(c, elementwise_affine=norm == "affine")

    class BlockLike(nn.Module):
        takes_point = True

        def __init__(self):
            super().__init__()
            c = channels
            self.channels, self.pre_norm = c, pre_norm
            conv_layer = TableConv(c, c) if conv == "table" else SC.SubMConv3d(c, c, kernel_size=3, bias=True, indice_key="stem")
            self.cpe = PointSeq(conv_layer, nn.Linear(c, c), norm_layer(c))
            self.norm1 = PointSeq(norm_layer(c))
            self.attn = Attention(c, num_heads, patch_size)
            self.attn.proj_drop = nn.Dropout(proj_drop)
            self.norm2 = PointSeq(norm_layer(c))
            self.mlp = PointSeq(MLP(c, 4 * c))
            self.drop_path = PointSeq(DropPath(drop_path) if drop_path > 0.0 else nn.Identity())

    m = BlockLike()
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            fan = int(np.prod(p.shape[1:])) if p.dim() > 1 else 4
            draw = rng.standard_normal(tuple(p.shape)) / math.sqrt(fan)
            if norm == "affine" and name.endswith("weight") and p.dim() == 1:
                draw = 1.0 + 0.3 * draw                       # a LayerNorm weight
            p.copy_(torch.from_numpy(draw))
    return m


# ---- the recorded runs of the reference's own Block -----------------------------------------------------------------------

RECORDS = ("ln", "ada")


def load_record(kind):
    """tests/golden/block_<kind>.npz (tests/golden/make_block_record.py: the reference's Block.forward and its backward in float64)
    -> {"meta", "state" (name -> float64 tensor), "data" (what point_of takes), "up", "out", "gin" (name -> array), "gparam"}"""
    import json
    import os

    import torch

    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"block_{kind}.npz"))
    meta = json.loads(str(z["meta"]))
    assert meta["kind"] == kind and not meta["training"]
    part = lambda prefix: {k[len(prefix):]: z[k] for k in z.files if k.startswith(prefix)}      # noqa: E731
    data = {k: (v.astype(np.float64) if v.dtype.kind == "f" else v) for k, v in part("in/").items()}
    data.update(spatial_shape=tuple(meta["spatial_shape"]), batch_size=meta["batch_size"])
    return {"meta": meta, "state": {k: torch.from_numpy(v.astype(np.float64)) for k, v in part("state/").items()}, "data": data,
            "up": z["up/feat"].astype(np.float64), "out": z["out/feat"], "gin": part("gin/"), "gparam": part("gparam/")}


def block_of_record(rec, **kwargs):
    """the stand-in with the record's constructor arguments and, under strict=True, its state_dict; in float64"""
    ctor = rec["meta"]["ctor"]
    m = make_block(ctor["channels"], ctor["num_heads"], ctor["patch_size"], norm=rec["meta"]["kind"],
                   global_channels=rec["meta"]["global_channels"], **kwargs).double()
    m.load_state_dict(rec["state"], strict=True)
    return m.eval()


def _norm_t(m, x, point):
    import torch.nn.functional as F

    if hasattr(m, "affine"):
        return torch_ada(x, m.affine(point.global_feat), point.offset, m.eps)
    return F.layer_norm(x, x.shape[1:], m.weight, m.bias, m.eps)


def restated_forward(self, point, mut=None):
    """Block.forward written from its arithmetic (pre_norm, any dtype and device the parts run on): y1 = x + norm(linear(conv x)),
    y2 = y1 + drop_path(attn(norm1 y1)), y3 = y2 + drop_path(mlp(norm2 y2)); feat and sparse_conv_feat end as y3.  `mut` switches
    one deliberate mistake on, one per junction."""
    assert self.pre_norm and mut in (None,) + MUTANTS
    x = point.feat
    sparse = self.cpe[0](point.sparse_conv_feat)
    b = self.cpe[1](sparse.features)
    y1 = x + (b if mut == "j1_branch_not_normed" else _norm_t(self.cpe[2], b, point))
    point.sparse_conv_feat = sparse
    point.feat = _norm_t(self.norm1[0], y1, point)
    a = self.attn(point).feat
    y2 = y1 + self.drop_path[0](a)
    h = self.mlp[0](_norm_t(self.norm2[0], a if mut == "j2_norm_of_branch" else y2, point))
    y3 = (x if mut == "j3_skip_is_input" else y2) + self.drop_path[0](h)
    point.feat = y3
    point.sparse_conv_feat = sparse.replace_feature(y3)
    return point
