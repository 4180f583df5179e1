"""float64 restatement of generativedensification_amd/viewattn.py's core and of its gradients (numpy), the same core in torch
float64 for autograd, and the stand-in module the tests use for the reference's Decoder (built from
tests/golden/viewattn_surface.json).  The arithmetic is the definition in csrc/viewattn.hip's header."""
import json
import os

import numpy as np

SURFACE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "viewattn_surface.json")


def _softmax(s):
    e = np.exp(s - s.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def view_attention_pool(t, cond, scale):
    """t (N, H, Ck), cond (N, V, Ck) -> u (N, H, Ck)"""
    t, cond = np.asarray(t, dtype=np.float64), np.asarray(cond, dtype=np.float64)
    p = _softmax(scale * np.einsum("nhc,nvc->nhv", t, cond))
    return np.einsum("nhv,nvc->nhc", p, cond)


def view_attention_pool_grad(t, cond, scale, grad_out):
    """(dt, dcond)"""
    t, cond, g = (np.asarray(a, dtype=np.float64) for a in (t, cond, grad_out))
    p = _softmax(scale * np.einsum("nhc,nvc->nhv", t, cond))
    dp = np.einsum("nhc,nvc->nhv", g, cond)
    ds = p * (dp - (p * dp).sum(-1, keepdims=True))
    dt = scale * np.einsum("nhv,nvc->nhc", ds, cond)
    dcond = np.einsum("nhv,nhc->nvc", p, g) + scale * np.einsum("nhv,nhc->nvc", ds, t)
    return dt, dcond


def view_attention_pool_torch(t, cond, scale):
    """the core as a torch composition in the dtypes it is given (autograd supplies the gradients)"""
    import torch

    p = torch.softmax(scale * torch.einsum("nhc,nvc->nhv", t, cond), dim=-1)
    return torch.einsum("nhv,nvc->nhc", p, cond)


def folded_attention_torch(fold, x, cond, num_heads):
    """out (N, E) from the result of fold_attention_weights, in torch (any dtype, differentiable)"""
    import torch.nn.functional as F

    A, a_bias, Bm, b_bias, scale = fold
    t = F.linear(x, A, a_bias).view(x.shape[0], num_heads, -1)
    u = view_attention_pool_torch(t, cond, scale)
    return F.linear(u.reshape(x.shape[0], -1), Bm, b_bias)


def surface():
    with open(SURFACE) as f:
        return json.load(f)


def make_decoder(width, sh_width, seed=0, dtype=None):
    """A module with the four attributes the surface record lists as read by the fine forward, built from that record alone:
    a LayerNorm over `width` channels, an attention made by the recorded constructor with the recorded keywords, a Sequential
    of the recorded layer types (width -> width -> width + sh_width) and the split point of the result.  Weights are seeded,
    and the biases and the LayerNorm affine are moved off their initial values so that every parameter matters.  The module
    has no forward of its own: the tests call `torch_forward_fine(m, ...)` or bind `viewattn.decoder_forward_fine`."""
    import torch
    from torch import nn

    S = surface()
    given = {"in_dim": width, "cond_dim": S["cond_dim"]}
    keywords = {k: given[v] if isinstance(v, str) else v for k, v in S["cross_att"]["keywords"].items()}
    sizes = iter(zip((width, width), (width, width + sh_width)))
    layers = [nn.Linear(*next(sizes)) if kind == "Linear" else getattr(nn, kind)() for kind in S["mlp_fine"]["types"]]
    parts = {"norm": nn.LayerNorm(width), "cross_att": getattr(nn, S["cross_att"]["constructor"].split(".")[-1])(**keywords),
             "mlp_fine": nn.Sequential(*layers), "feature_dim": width}
    assert sorted(parts) == S["forward_fine"]["reads"]

    class Stand(nn.Module):
        pass

    m = Stand()
    for name in S["forward_fine"]["reads"]:
        setattr(m, name, parts[name])
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() == 1:
                p.copy_((1.0 if name == "norm.weight" else 0.0) + 0.2 * torch.randn(p.shape, generator=gen))
            else:
                p.copy_(torch.randn(p.shape, generator=gen) * (1.5 / p.shape[1] ** 0.5))
    return m.to(dtype) if dtype is not None else m


def torch_forward_fine(m, volume_feat, point_feats):
    """The unfolded torch path of such a module, the yardstick of the bound forward: every point is a sequence of one
    normalised query that attends to its views through the module's real nn.MultiheadAttention; the MLP follows, and the
    float32 result is cut at `feature_dim`.  Returns ((N, 1, feature_dim), (N, 1, rest))."""
    query = m.norm(volume_feat)[:, None]
    attended, _ = m.cross_att(query, point_feats, point_feats, need_weights=False)
    y = m.mlp_fine(attended).float()
    return y.split([m.feature_dim, y.shape[-1] - m.feature_dim], dim=-1)
