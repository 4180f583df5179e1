"""float64 restatement (numpy) of generativedensification_amd/deconv3d.py: the LayerNorm over the channels of every voxel, the
transposed convolution with kernel 2 and stride 2 as 8 strided products, and all gradients.  Independent of torch's
convolution; the arithmetic is the definition in csrc/deconv3d.hip's header.

x (B, Cin, D, H, W), weight (Cin, Cout, 2, 2, 2); tap (i, j, k) of parent voxel (d, h, w) is child voxel (2d + i, 2h + j, 2w + k):
    n = x, or with norm = (gamma, beta, eps): n[b, :, d, h, w] = (x - mean) / sqrt(var + eps) gamma + beta over the channel axis
    out[b, co, 2d + i, 2h + j, 2w + k] = bias[co] + sum over c of n[b, c, d, h, w] weight[c, co, i, j, k]
"""
import itertools

import numpy as np

TAPS = list(itertools.product(range(2), repeat=3))


def _bc(v):
    return np.asarray(v, dtype=np.float64)[None, :, None, None, None]


def normalised(x, norm):
    """(n, xhat, rstd); without a norm n = x and the others are None"""
    x = np.asarray(x, dtype=np.float64)
    if norm is None:
        return x, None, None
    gamma, beta, eps = norm
    mean = x.mean(1, keepdims=True)
    var = ((x - mean) ** 2).mean(1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    xhat = (x - mean) * rstd
    n = xhat
    if gamma is not None:
        n = n * _bc(gamma)
    if beta is not None:
        n = n + _bc(beta)
    return n, xhat, rstd


def children(a, tap):
    """the child voxels of tap (i, j, k): a view of a (B, C, 2D, 2H, 2W) array as (B, C, D, H, W)"""
    i, j, k = tap
    return a[:, :, i::2, j::2, k::2]


def deconv(x, weight, bias=None, norm=None):
    n, _, _ = normalised(x, norm)
    weight = np.asarray(weight, dtype=np.float64)
    B, _, D, H, W = n.shape
    out = np.zeros((B, weight.shape[1], 2 * D, 2 * H, 2 * W))
    for tap in TAPS:
        children(out, tap)[...] = np.einsum("bcdhw,co->bodhw", n, weight[(slice(None), slice(None)) + tap])
    if bias is not None:
        out += _bc(bias)
    return out


def deconv_grad(x, weight, grad_out, norm=None):
    """{"dx", "dw", "db", and with a norm "dgamma", "dbeta"}"""
    weight, g = np.asarray(weight, dtype=np.float64), np.asarray(grad_out, dtype=np.float64)
    n, xhat, rstd = normalised(x, norm)
    g_n, dw = np.zeros_like(n), np.zeros_like(weight)
    for tap in TAPS:
        w_t = weight[(slice(None), slice(None)) + tap]
        g_n += np.einsum("bodhw,co->bcdhw", children(g, tap), w_t)
        dw[(slice(None), slice(None)) + tap] = np.einsum("bcdhw,bodhw->co", n, children(g, tap))
    res = {"dw": dw, "db": g.sum((0, 2, 3, 4))}
    if norm is None:
        res["dx"] = g_n
        return res
    a = g_n if norm[0] is None else g_n * _bc(norm[0])
    res["dx"] = rstd * (a - a.mean(1, keepdims=True) - xhat * (a * xhat).mean(1, keepdims=True))
    res["dgamma"] = (g_n * xhat).sum((0, 2, 3, 4))
    res["dbeta"] = g_n.sum((0, 2, 3, 4))
    return res


# ---- the reference's VolTransformer: its recorded surface, a small mirror built from the record, its forward restated ------------

def surface():
    import json
    import os

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "voltransformer_surface.json")) as f:
        return json.load(f)


def make_mirror(layers, embed_dim=16, vol_low_res=4, n_groups=(2,), out_dim=8, seed=0):
    """a plain nn.Module with the attributes VolTransformer.forward reads; `norm` and `deconv` are constructed from the
    recorded constructor calls, `layers` are the caller's stand-ins taking (x, cond, n_group, block_size)"""
    import torch
    from torch import nn

    S = surface()
    given = {"embed_dim": embed_dim, "out_dim": out_dim, "eps": S["init"]["defaults"]["eps"]}

    def build(record):
        ctor = getattr(nn, record["constructor"].split(".")[-1])
        return ctor(*(given[a] if isinstance(a, str) else a for a in record["args"]),
                    **{k: given[v] if isinstance(v, str) else v for k, v in record["keywords"].items()})

    torch.manual_seed(seed)
    m = nn.Module()
    m.n_groups = list(n_groups)
    m.block_size = [vol_low_res // g for g in n_groups]
    m.pos_embed = nn.Parameter(torch.randn(1, embed_dim, vol_low_res, vol_low_res, vol_low_res) * (1.0 / embed_dim) ** 0.5)
    m.layers = nn.ModuleList(layers)
    m.norm = build(S["modules"]["norm"])
    m.deconv = build(S["modules"]["deconv"])
    with torch.no_grad():       # an affine that is not the identity
        m.norm.weight.add_(0.3 * torch.randn(embed_dim))
        m.norm.bias.add_(0.2 * torch.randn(embed_dim))
    assert set(S["forward"]["reads"]) <= set(dir(m))
    return m


def reference_forward(m, image_feats, conds=None):
    """VolTransformer.forward as the reference states it, line for line; `conds` (a list) receives every cond built"""
    import torch

    S = surface()["forward"]["einsum"]
    B, V, C, D, H, W = image_feats.shape
    volume_feats = []
    for n_group in m.n_groups:
        block_size = D // n_group
        blocks = image_feats.unfold(3, block_size, block_size).unfold(4, block_size, block_size).unfold(5, block_size, block_size)
        blocks = blocks.contiguous().view(B, V, C, n_group ** 3, block_size ** 3)
        blocks = torch.einsum(S[0], blocks).reshape(B * n_group ** 3, block_size ** 3 * V, C)
        volume_feats.append(blocks)
    if conds is not None:
        conds.extend(volume_feats)
    x = m.pos_embed.repeat(B, 1, 1, 1, 1)
    for i, layer in enumerate(m.layers):
        group_idx = i % len(m.block_size)
        x = layer(x, volume_feats[group_idx], m.n_groups[group_idx], m.block_size[group_idx])
    x = m.norm(torch.einsum(S[1], x))
    x = torch.einsum(S[2], x)
    x_up = m.deconv(x)
    return torch.einsum(S[3], x_up).contiguous()


def make_stub_layers(count, embed_dim=16, cond_dim=24, seed=1):
    """stand-ins for the blocks: plain nn.Modules taking (x, cond, n_group, block_size) that mix the channels of every voxel,
    let the cond in, and remember each cond they were handed.  They work on a contiguous copy of the voxel rows, so their
    arithmetic does not depend on the layout x arrives in."""
    import torch
    from torch import nn

    class StubLayer(nn.Module):
        def __init__(self):
            super().__init__()
            self.mix = nn.Linear(embed_dim, embed_dim)
            self.proj = nn.Linear(cond_dim, embed_dim)
            self.seen = []

        def forward(self, x, cond, n_group, block_size):
            self.seen.append((cond, n_group, block_size))
            rows = x.permute(0, 2, 3, 4, 1).contiguous()
            rows = rows + torch.tanh(self.mix(rows)) + 0.1 * self.proj(cond).mean((0, 1))
            return rows.permute(0, 4, 1, 2, 3)

    torch.manual_seed(seed)
    return [StubLayer() for _ in range(count)]
