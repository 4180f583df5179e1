"""Plain-torch restatement of SSIM / MS-SSIM (the specification in the header of
generativedensification_amd/csrc/ssim.hip, i.e. the published algorithm of pytorch_msssim 1.x), dtype-generic.

The blur is k shifted-slice multiply-adds and the 2x2 pool is pad + reshape-sum, so the f64 restatement runs on the GPU
without MIOpen and on the CPU; tests/test_ssim_cpu.py checks it against an F.conv2d / F.avg_pool2d composition."""
from __future__ import annotations

import torch
import torch.nn.functional as F

MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def gauss_window(size: int = 11, sigma: float = 1.5) -> torch.Tensor:
    """The normalised 1-D window, computed in fp32 as pytorch_msssim does (cast to the compute dtype by the caller)."""
    coords = torch.arange(size, dtype=torch.float32) - size // 2
    g = torch.exp(-(coords ** 2) / (2 * sigma ** 2))
    return g / g.sum()


def blur(x: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """Valid separable blur of (B, C, h, w): along H, then along W."""
    k = g.numel()
    h, w = x.shape[-2:]
    g = g.to(device=x.device, dtype=x.dtype)
    y = sum(g[t] * x[..., t:t + h - k + 1, :] for t in range(k))
    return sum(g[t] * y[..., :, t:t + w - k + 1] for t in range(k))


def pool2(x: torch.Tensor) -> torch.Tensor:
    """avg_pool2d(kernel 2, stride 2, padding (h % 2, w % 2), count_include_pad=True): output j averages inputs 2j - pad
    and 2j - pad + 1, input -1 read as 0, divisor 4."""
    h, w = x.shape[-2:]
    ph, pw = h % 2, w % 2
    x = F.pad(x, (pw, 0, ph, 0))
    B, C, H, W = x.shape
    return x.reshape(B, C, H // 2, 2, W // 2, 2).sum(dim=(3, 5)) / 4


def ssim_terms(X, Y, g, C1, C2):
    """Per-(batch, channel) means of ssim_map and cs_map, each (B, C)."""
    mu_x, mu_y = blur(X, g), blur(Y, g)
    s_xx = blur(X * X, g) - mu_x ** 2
    s_yy = blur(Y * Y, g) - mu_y ** 2
    s_xy = blur(X * Y, g) - mu_x * mu_y
    cs_map = (2 * s_xy + C2) / (s_xx + s_yy + C2)
    ssim_map = (2 * mu_x * mu_y + C1) / (mu_x ** 2 + mu_y ** 2 + C1) * cs_map
    return ssim_map.flatten(2).mean(-1), cs_map.flatten(2).mean(-1)


def _window(win_size, win_sigma, win):
    """The 1-D taps: the Gaussian, or a user `win` given as pytorch_msssim takes it, a (C, 1, 1, k) tensor of identical rows
    (or the 1-D taps themselves).  blur() applies taps g[t] to x[i + t], a correlation, along H and then along W: exactly
    what F.conv2d does with that tensor (conv2d does not flip its kernel), so an asymmetric window is not mirrored."""
    if win is None:
        return gauss_window(win_size, win_sigma)
    win = torch.as_tensor(win)
    rows = win.reshape(-1, win.shape[-1])
    assert bool((rows == rows[0]).all())
    return rows[0]


def ssim_planes(X, Y, data_range=255, win_size=11, win_sigma=1.5, win=None, K=(0.01, 0.03), nonnegative_ssim=False):
    """(B, C) per-plane SSIM: what the kernels return before the host-side mean."""
    K1, K2 = K
    s, _ = ssim_terms(X, Y, _window(win_size, win_sigma, win), (K1 * data_range) ** 2, (K2 * data_range) ** 2)
    return torch.relu(s) if nonnegative_ssim else s


def ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None, K=(0.01, 0.03),
         nonnegative_ssim=False):
    s = ssim_planes(X, Y, data_range, win_size, win_sigma, win, K, nonnegative_ssim)
    return s.mean() if size_average else s.mean(1)


def ms_ssim_planes(X, Y, data_range=255, win_size=11, win_sigma=1.5, win=None, weights=None, K=(0.01, 0.03), pool=None):
    """(B, C) per-plane MS-SSIM.  `pool` replaces pool2 (the CPU tests pass mutants of it)."""
    K1, K2 = K
    pool = pool2 if pool is None else pool
    g = _window(win_size, win_sigma, win)
    weights = MS_WEIGHTS if weights is None else weights
    w = (weights.to(dtype=X.dtype, device=X.device) if torch.is_tensor(weights)
         else torch.tensor(weights, dtype=X.dtype, device=X.device))
    assert min(X.shape[-2:]) > (g.numel() - 1) * 2 ** (w.numel() - 1)
    vals = []
    for lvl in range(w.numel()):
        s, cs = ssim_terms(X, Y, g, (K1 * data_range) ** 2, (K2 * data_range) ** 2)
        if lvl < w.numel() - 1:
            vals.append(torch.relu(cs))
            X, Y = pool(X), pool(Y)
    vals.append(torch.relu(s))
    return torch.prod(torch.stack(vals) ** w.view(-1, 1, 1), dim=0)


def ms_ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None, weights=None, K=(0.01, 0.03)):
    v = ms_ssim_planes(X, Y, data_range, win_size, win_sigma, win, weights, K)
    return v.mean() if size_average else v.mean(1)
