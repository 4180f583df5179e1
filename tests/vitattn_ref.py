"""A mirror of timm's `timm.models.vision_transformer.Attention` for the tests of generativedensification_amd/vitattn.py: the
attribute surface that `vit_attention_forward` reads (num_heads, head_dim, scale, qkv, q_norm, k_norm, attn_drop, proj,
proj_drop) and, as `forward`, the lines of its fused branch.  timm is not installed where these tests run, so this is a
RESTATEMENT of its public forward in our own words, not a recording of it: the tests show that the bound function computes
what these lines compute, and that every fall-back returns their bits."""
import torch
import torch.nn.functional as F
from torch import nn


class Attention(nn.Module):
    def __init__(self, dim, num_heads, qkv_bias=True, qk_norm=False, attn_drop=0.0, proj_drop=0.0):
        super().__init__()
        assert dim % num_heads == 0
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.fused_attn = True
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.q_norm = nn.LayerNorm(self.head_dim) if qk_norm else nn.Identity()
        self.k_norm = nn.LayerNorm(self.head_dim) if qk_norm else nn.Identity()
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)

    def forward(self, x, attn_mask=None):
        B, N, C = x.shape
        qkv = self.qkv(x).reshape(B, N, 3, self.num_heads, self.head_dim).permute(2, 0, 3, 1, 4)
        q, k, v = qkv.unbind(0)
        q, k = self.q_norm(q), self.k_norm(k)
        x = F.scaled_dot_product_attention(q, k, v, attn_mask=attn_mask, scale=self.scale,
                                           dropout_p=self.attn_drop.p if self.training else 0.0)
        x = x.transpose(1, 2).reshape(B, N, C)
        x = self.proj(x)
        return self.proj_drop(x)


def make(dim, num_heads, seed, **kw):
    """a seeded module whose parameters break symmetries: a magnitude per output row of each Linear, biases that are not small"""
    g = torch.Generator().manual_seed(seed)
    m = Attention(dim, num_heads, **kw)
    with torch.no_grad():
        for lin, gain in ((m.qkv, 2.0), (m.proj, 1.0)):
            rows = 0.5 + torch.arange(lin.out_features, dtype=torch.float32) % 5 / 4
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) * gain / lin.in_features ** 0.5 * rows[:, None])
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=g) * 0.3)
    return m


def inputs(B, N, dim, seed):
    """x and the upstream gradient, each varying per token and channel"""
    g = torch.Generator().manual_seed(seed)
    tok = 0.5 + torch.arange(N, dtype=torch.float32).view(1, N, 1) % 5 / 3
    x = torch.randn(B, N, dim, generator=g) * tok
    dy = torch.randn(B, N, dim, generator=g) * (1.0 + 0.5 * torch.cos(torch.arange(dim, dtype=torch.float32) * 0.7))
    return x, dy
