"""Inputs for the SSIM / MS-SSIM tests that break the symmetries of the kernels' index arithmetic (csrc/ssim.hip): shared by
tests/test_gpu_ssim.py (HIP against the f64 restatement) and tests/test_ssim_cpu.py (mutants of the restatement, which show
on the CPU that these inputs tell a wrong index from a right one and that the earlier inputs do not).

Everything is seeded and built on the CPU, then moved; layouts are applied after the move, because `.to(device)` and
`.clone()` do not keep a layout that is not dense."""
from __future__ import annotations

import torch

# the bars of test_gpu_ssim._assert_close
VALUE_ATOL = 5e-6        # |value - f64 value|
GRAD_RTOL = 2e-4         # max |g - g64| / max |g64|
COS_MIN = 1 - 1e-6       # cosine of g and g64


def images(shape, seed=0, scale=1.0, device="cpu", dtype=torch.float32):
    """Smooth-plus-noise X and a noisier Y in [0, scale] (the images test_gpu_ssim.py has used from the start)."""
    g = torch.Generator().manual_seed(seed)
    B, Ch, H, W = shape
    yy, xx = torch.meshgrid(torch.linspace(0, 3, H), torch.linspace(0, 5, W), indexing="ij")
    smooth = 0.5 + 0.3 * torch.sin(xx + yy)[None, None] * torch.linspace(0.5, 1.0, B * Ch).view(B, Ch, 1, 1)
    X = (smooth + 0.05 * torch.randn(shape, generator=g)).clamp(0, 1)
    Y = (X + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1)
    return (scale * X).to(device=device, dtype=dtype), (scale * Y).to(device=device, dtype=dtype)


def upstream(shape, seed, device="cpu", dtype=torch.float32):
    """A random upstream gradient of mixed sign and magnitude (three decades), different for every plane."""
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(shape, generator=g) * 10 ** (3 * torch.rand(shape, generator=g) - 2)
    return r.to(device=device, dtype=dtype)


def asym_window(k, channels=3):
    """Monotone taps arange(1, k + 1) / sum as the (C, 1, 1, k) tensor of identical rows that `win=` takes."""
    g = torch.arange(1, k + 1, dtype=torch.float32)
    return (g / g.sum()).reshape(1, 1, 1, k).repeat(channels, 1, 1, 1)


def pyramid(h, w, levels):
    """[(h_l, w_l)] of the 2x2 pool with padding size % 2."""
    out = []
    for _ in range(levels):
        out.append((h, w))
        h, w = (h + h % 2) // 2, (w + w % 2) // 2
    return out


# ---- A.3 every dispatched window size --------------------------------------------------------------------------------
WINDOW_SIZES = (1, 3, 5, 9, 13, 15)           # 7 and 11 are covered by the older tests
ONE_PIXEL_WEIGHTS = (0.3, 0.5, 0.4)           # three levels for the one-pixel case


def tile_crossing_shape(k):
    """ssim(): a valid region of 17 x 65, one pixel past a 16 x 64 tile on each axis."""
    return (2, 2, 16 + k, 64 + k)


def one_pixel_shape(k):
    """ms_ssim with three levels: (4k, 4k - 1) -> (2k, 2k) -> (k, k), a valid region of exactly one pixel at the coarsest."""
    return (2, 2, 4 * k, 4 * k - 1)


# ---- A.4 level counts and weights ------------------------------------------------------------------------------------
# id -> (weights, win_size, (H, W)); unequal and not normalised.  Eight levels with a 3-tap window need min(H, W) > 2 * 128:
# 300 x 270 -> 150 x 135 -> 75 x 68 -> 38 x 34 -> 19 x 17 -> 10 x 9 -> 5 x 5 -> 3 x 3
LEVEL_CASES = {
    "L1": ((1.7,), 11, (97, 130)),
    "L2": ((0.4, 1.9), 11, (97, 130)),
    "L3": ((1.2, 0.3, 0.8), 11, (97, 130)),
    "L8": ((0.5, 1.3, 0.2, 0.9, 0.4, 1.1, 0.7, 0.3), 3, (300, 270)),
}

# ---- A.5 axes that differ ----------------------------------------------------------------------------------------------
# five levels, 11 taps (min side > 160):
#   even_h_odd_w   192 x 161 -> 96 x 81 -> 48 x 41 -> 24 x 21 -> 12 x 11   (H even and W odd at every level)
#   odd_h_even_w   161 x 192 -> 81 x 96 -> 41 x 48 -> 21 x 24 -> 11 x 12   (the transpose)
#   wide           161 x 1500 -> 81 x 750 -> 41 x 375 -> 21 x 188 -> 11 x 94
#   tall           1500 x 161 -> 750 x 81 -> 375 x 41 -> 188 x 21 -> 94 x 11
AXIS_CASES = {"even_h_odd_w": (192, 161), "odd_h_even_w": (161, 192), "wide": (161, 1500), "tall": (1500, 161)}

# ---- A.6 layouts -------------------------------------------------------------------------------------------------------
LAYOUTS = ("x_nhwc", "y_nhwc", "x_slice", "y_expand")


def apply_layout(X, Y, kind):
    """(X, Y) with the same values in the layouts of A.6; `y_expand` replaces Y by its first sample over the batch."""
    def nhwc(t):
        return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)

    if kind == "same":
        return X.contiguous(), Y.contiguous()
    if kind == "x_nhwc":
        return nhwc(X), Y.contiguous()
    if kind == "y_nhwc":
        return X.contiguous(), nhwc(Y)
    if kind == "x_slice":
        B, C, H, W = X.shape
        big = torch.full((B, C + 1, H + 3, 2 * W + 5), 7.0, dtype=X.dtype, device=X.device)
        view = big[:, 1:, 2:2 + H, 3:3 + 2 * W:2]
        view.copy_(X)
        return view, Y.contiguous()
    if kind == "y_expand":
        return X.contiguous(), Y[:1].contiguous().expand(X.shape)
    raise ValueError(kind)


# ---- A.7 flat and degenerate content ---------------------------------------------------------------------------------
def flat_images(kind, shape, seed=0, device="cpu", dtype=torch.float32):
    """'white': X == Y == 1 (the renderer's background); 'half_white': the left half white in both, the right half textured
    and different; 'identical': X == Y textured."""
    X, Y = images(shape, seed, 1.0, "cpu", torch.float32)
    if kind == "white":
        X = torch.ones(shape)
        Y = X.clone()
    elif kind == "half_white":
        X[..., : shape[-1] // 2] = 1.0
        Y[..., : shape[-1] // 2] = 1.0
    elif kind == "identical":
        Y = X.clone()
    else:
        raise ValueError(kind)
    return X.to(device=device, dtype=dtype), Y.to(device=device, dtype=dtype)


def beyond_bar(v, grads, v_ref, grads_ref):
    """True when (v, grads) misses (v_ref, grads_ref) by more than the bars of test_gpu_ssim._assert_close."""
    if float((v.double() - v_ref.double()).abs().max()) >= VALUE_ATOL:
        return True
    for g, gr in zip(grads, grads_ref):
        g, gr = g.double(), gr.double()
        m = float(gr.abs().max())
        if float((g - gr).abs().max()) > GRAD_RTOL * m:
            return True
        if float((g * gr).sum() / (g.norm() * gr.norm())) < COS_MIN:
            return True
    return False
