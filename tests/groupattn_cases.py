"""Shapes and seeded inputs of the group-attention tests (tests/test_gpu_groupattn.py, tests/test_groupattn_cpu.py).

Core cases (M, Lq, Lk, H, Dh): the smallest at which the lane mapping of csrc/groupattn.hip can go wrong.  The forward is
flat, 256 lanes per workgroup over the M Lq H (group, query, head) lanes.  The backward gives a workgroup
upw = max(1, 512 // (Lq H)) whole groups and walks their Lq H query lanes, then their Lk H key lanes, in strides of 256.  So:
  ref        the reference's shape; upw = 4, the second workgroup holds one group
  lk2        two keys
  one        one key: out = v exactly, dq = 0 exactly; one lane in all
  m257       65 workgroups, the last with one group; more than one forward workgroup per row of heads
  g8         the n_groups 8 shape: 1024 query lanes of a group take four strides, its 512 key lanes two
  odd        nothing a power of two; 20 groups would fit a workgroup, 7 exist
  odd_tail   the same with 41 groups: workgroups of 20, 20 and 1 groups, 500 query lanes in 256-lane strides
  h20        540 query lanes per group (two strides and a tail), 240 key lanes (a partial stride)
  corner     the envelope's corner in Lq, Lk and Dh
  h64        64 heads
  lds_limit  64 queries x 64 heads: the 64 KiB of LDS records a backward workgroup can need at most
The first nine are the cases the feature was specified with; odd_tail and lds_limit were added for the backward's group
packing and its LDS bound.  STRIDED reuses the reference's shape with another layout; TWIN_KEYS has four keys, so that a row can still be near one-hot."""
import numpy as np

CASES = {
    "ref": (5, 8, 4, 16, 16),
    "lk2": (3, 8, 2, 16, 16),
    "one": (1, 1, 1, 1, 8),
    "m257": (257, 8, 4, 16, 16),
    "g8": (3, 64, 32, 16, 16),
    "odd": (7, 5, 7, 5, 8),
    "h20": (9, 27, 12, 20, 8),
    "corner": (2, 64, 64, 4, 32),
    "h64": (2, 8, 4, 64, 16),
    "odd_tail": (41, 5, 7, 5, 8),
    "lds_limit": (1, 64, 3, 64, 8),
    "strided": (5, 8, 4, 16, 16),       # k and v are the halves of one 2E-wide tensor, q sits behind a row stride > E
    "twin_keys": (6, 8, 4, 16, 16),     # keys 0 and 1 of every group are identical
}
STRIDED, TWIN_KEYS = "strided", "twin_keys"
SPAN = 12.0                             # s spans about +-SPAN
SEEDS = {"one": 37}                     # its single score is one draw of standard deviation 4: the seed that puts it at -9.6


def scale_of(name):
    return CASES[name][4] ** -0.5


def inputs(name, seed=None):
    """(q (M, Lq, E), k, v (M, Lk, E), grad_out (M, Lq, E)) float64.  k, v ~ N(0, 1).  The M Lq rows of q grow from 1 % to 100 %
    of the length at which s has a standard deviation of SPAN / 3, so the first rows are near uniform and the last near
    one-hot."""
    M, Lq, Lk, H, Dh = CASES[name]
    rng = np.random.default_rng([SEEDS.get(name, 0) if seed is None else seed, M, Lq, Lk, H, Dh])
    k, v = rng.standard_normal((M, Lk, H * Dh)), rng.standard_normal((M, Lk, H * Dh))
    if name == TWIN_KEYS:
        k[:, 1] = k[:, 0]
    sigma = SPAN / 3.0 / (scale_of(name) * np.sqrt(Dh))
    rows = np.linspace(0.01, 1.0, M * Lq) if M * Lq > 1 else np.ones(1)
    q = rng.standard_normal((M, Lq, H * Dh)) * sigma * rows.reshape(M, Lq, 1)
    g = rng.standard_normal((M, Lq, H * Dh))
    return q, k, v, g


# (B, C, D, H, W, bs) of the norm tests: the smallest width with three blocks per axis (432 rows: 32 to a forward workgroup,
# seven backward workgroups, the last with 48 rows); the reference's width (32 lanes per row, 8 rows per workgroup); bs = 1 (the
# identity map) at C = 40, where 5 of a row's 8 lanes hold channels; the widest row (two pieces per lane) with the largest
# block; a non-cubic volume with three different group counts
NORM_SHAPES = [(2, 8, 6, 6, 6, 2), (1, 256, 4, 4, 4, 2), (1, 40, 3, 3, 3, 1), (1, 1024, 8, 8, 8, 8), (2, 16, 4, 6, 2, 2)]


def norm_inputs(shape, seed=3):
    """(vol (B, C, D, H, W), weight (C,), bias (C,), grad_patches, grad_normed (B G, bs^3, C), grad_vol like vol) float64; the
    rows of vol have different means and spreads"""
    B, C, D, H, W, bs = shape
    rng = np.random.default_rng([seed, *shape])
    vol = rng.standard_normal((B, C, D, H, W)) * rng.uniform(0.2, 3.0, (B, 1, D, H, W)) + rng.standard_normal((B, 1, D, H, W))
    weight, bias = 1.0 + 0.3 * rng.standard_normal(C), 0.3 * rng.standard_normal(C)
    rows = (B * D * H * W // bs ** 3, bs ** 3, C)
    return vol, weight, bias, rng.standard_normal(rows), rng.standard_normal(rows), rng.standard_normal(vol.shape)


# (E, H, kdim, Lq, Lk) of the composition tests on the CPU: the reference's head width first
MHA_GRID = [(64, 4, 24, 8, 4), (40, 5, 16, 3, 5), (16, 1, 7, 1, 1)]


def mha_inputs(E, H, kdim, Lq, Lk, M=3, seed=1):
    """(x (M, Lq, E), cond (M, Lk, kdim)) float64"""
    rng = np.random.default_rng([seed, E, H, kdim, Lq, Lk])
    return rng.standard_normal((M, Lq, E)), rng.standard_normal((M, Lk, kdim))


def make_mha(E, H, kdim, bias, packed, seed=2):
    """a float64 nn.MultiheadAttention on the CPU with seeded weights (biases included, which torch initialises to zero);
    packed: kdim = vdim = E (one in_proj_weight), so kdim is ignored and cond is E wide"""
    import torch
    from torch import nn

    kw = {} if packed else {"kdim": kdim, "vdim": kdim}
    m = nn.MultiheadAttention(E, H, bias=bias, batch_first=True, dtype=torch.float64, **kw)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=gen, dtype=torch.float64) * (0.3 if p.dim() == 1 else p.shape[-1] ** -0.5))
    return m
