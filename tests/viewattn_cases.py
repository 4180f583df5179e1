"""Shapes and seeded inputs of the view-attention tests (tests/test_gpu_viewattn.py, tests/test_viewattn_cpu.py).

GPU cases (N, H, Ck, V): the smallest at which the lane mapping of csrc/viewattn.hip can go wrong.  A workgroup holds
256 / HP points (HP = H rounded up to a power of two), so N = 1, 3, 257 and 1000 are off every block size at H = 16; H = 20 and
5 leave idle lanes in a group; H = 1 puts 64 points into a wave; H = 64 makes a group a whole wave; V = 7, 9 and 16 take the
kernels that walk the views in rolled loops instead of holding cond in registers (V > 4); Ck = 4 and 16 take the narrow and
the two-piece row accesses, and (33, 5, 4, 7) has rows that are no multiple of 8 elements, which the host side pads.  The
first nine are the cases the feature was specified with; c8_v9 was added with the rolled kernels."""
import numpy as np

CASES = {
    "n1_v1": (1, 16, 8, 1),
    "n3_v2": (3, 16, 8, 2),
    "n257_v3": (257, 16, 8, 3),
    "n1000_v4": (1000, 16, 8, 4),
    "h20": (65, 20, 8, 4),
    "h1": (130, 1, 8, 4),
    "h5_c4_v7": (33, 5, 4, 7),
    "h32_c16_v16": (96, 32, 16, 16),
    "h64_c4": (70, 64, 4, 2),
    "c8_v9": (40, 16, 8, 9),    # (the many-view kernels at the decoder's H and Ck; 7 and 16 views are above at Ck = 4 and 16)
}
TWIN_VIEWS = "n257_v3"          # views 0 and 1 of every point are identical here
WIDE_ROWS = "n1000_v4"          # t is handed with a row stride larger than the row here
SPAN = 12.0                     # s spans about +-SPAN


def scale_of(name):
    """what the fold hands over for the reference's module (head_dim 5) at its shape, another value elsewhere"""
    N, H, Ck, V = CASES[name]
    return 5.0 ** -0.5 if (H, Ck) == (16, 8) else 0.3


def inputs(name, seed=0):
    """(t (N, H, Ck), cond (N, V, Ck), grad_out (N, H, Ck)) float64.  cond ~ N(0, 1), distinct per view and channel.  The rows
    of t grow from 1 % to 100 % of the length at which s has a standard deviation of SPAN / 3, so the first rows are near uniform
    and the last near one-hot."""
    N, H, Ck, V = CASES[name]
    rng = np.random.default_rng([seed, N, H, Ck, V])
    cond = rng.standard_normal((N, V, Ck))
    if name == TWIN_VIEWS:
        cond[:, 1] = cond[:, 0]
    sigma = SPAN / 3.0 / (scale_of(name) * np.sqrt(Ck))
    rows = np.linspace(0.01, 1.0, N) if N > 1 else np.ones(1)
    t = rng.standard_normal((N, H, Ck)) * sigma * rows[:, None, None]
    g = rng.standard_normal((N, H, Ck))
    return t, cond, g


# (E, H, Ck, V) of the fold tests: the reference's module first
FOLD_GRID = [(80, 16, 8, 3), (40, 20, 8, 4), (16, 1, 16, 1), (20, 5, 4, 7)]


def fold_inputs(E, H, Ck, V, N=6, seed=1):
    """(x (N, E), cond (N, V, Ck), grad (N, E)) float64"""
    rng = np.random.default_rng([seed, E, H, Ck, V])
    return rng.standard_normal((N, E)), rng.standard_normal((N, V, Ck)), rng.standard_normal((N, E))


def make_mha(E, H, Ck, bias, packed, seed=2):
    """a float64 nn.MultiheadAttention on the CPU with seeded weights (biases included, which torch initialises to zero);
    packed: kdim = vdim = E (one in_proj_weight), so Ck is ignored and the views are E wide"""
    import torch
    from torch import nn

    kw = {} if packed else {"kdim": Ck, "vdim": Ck}
    m = nn.MultiheadAttention(E, H, bias=bias, batch_first=True, dtype=torch.float64, **kw)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=gen, dtype=torch.float64) * (0.3 if p.dim() == 1 else p.shape[-1] ** -0.5))
    return m
