"""SSIM and MS-SSIM on the MI355X (csrc/ssim.hip, include/gdr.h gdr_ssim_*), with the signatures and defaults of
`pytorch_msssim` 1.x: the image-similarity half of the reference's training loss `MSE + 0.5 * (1 - MS_SSIM)`
(lightning/loss.py) and the `ssim(...)` of its evaluation.  The `pytorch_msssim` package of this repository re-exports
these names.  The semantics are restated in the header of csrc/ssim.hip.

Deviations from pytorch_msssim (each raises instead of warning or silently changing the computation):
  - 5-D (video) inputs and `spatial_dims != 2`;
  - a `win` whose rows differ per channel, and `win_size > 15` (the LDS tile of the kernels);
  - an `ssim()` input with an axis shorter than the window (pytorch_msssim warns and skips filtering on that axis);
  - CPU tensors (no CPU fallback anywhere in the product) and fp64 (fp32 native; fp16 / bf16 computed in fp32, their
    gradients returned in the input dtype).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from . import _marshal as M

__all__ = ["ssim", "ms_ssim", "SSIM", "MS_SSIM"]

_MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def _fspecial_gauss_1d(size: int, sigma: float) -> torch.Tensor:
    """The (1, 1, size) normalised 1-D Gaussian window."""
    coords = torch.arange(size, dtype=torch.float32) - size // 2
    g = torch.exp(-(coords ** 2) / (2 * sigma ** 2))
    return (g / g.sum()).reshape(1, 1, -1)


class _SSIMFunction(torch.autograd.Function):
    """(X, Y) fp32 (B, C, H, W) on the GPU -> (B, C) per-plane value (ssim, relu(ssim) or the MS-SSIM product)."""

    @staticmethod
    def forward(ctx, X, Y, args):
        lib = L.load()
        dev = X.device
        with torch.cuda.device(dev):
            ws = torch.empty(int(lib.gdr_ssim_workspace_bytes(C.byref(args))), dtype=torch.uint8, device=dev)
            out = torch.empty(args.B, args.C, dtype=torch.float32, device=dev)
            st = M.stream()
            L.check(lib.gdr_ssim_forward(C.byref(args), X.data_ptr(), M.strides(X), Y.data_ptr(), M.strides(Y), ws.data_ptr(),
                                         out.data_ptr(), st), "gdr_ssim_forward")
        ctx.save_for_backward(X, Y)
        ctx.ws, ctx.args = ws, args
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        lib = L.load()
        X, Y = ctx.saved_tensors
        args, dev = ctx.args, X.device
        want_dy = ctx.needs_input_grad[1]
        g = g.to(torch.float32).contiguous()
        dX = torch.empty_like(X)
        dY = torch.empty_like(Y) if want_dy else None
        with torch.cuda.device(dev):
            scratch = torch.empty(int(lib.gdr_ssim_scratch_bytes(C.byref(args), int(want_dy))), dtype=torch.uint8, device=dev)
            st = M.stream()
            L.check(lib.gdr_ssim_backward(C.byref(args), X.data_ptr(), M.strides(X), Y.data_ptr(), M.strides(Y), ctx.ws.data_ptr(),
                                          g.data_ptr(), dX.data_ptr(), M.strides(dX), dY.data_ptr() if want_dy else None,
                                          M.strides(dY) if want_dy else None, scratch.data_ptr(), st), "gdr_ssim_backward")
        return dX, dY, None


def _check_inputs(X: torch.Tensor, Y: torch.Tensor):
    if not X.shape == Y.shape:
        raise ValueError(f"Input images should have the same dimensions, but got {X.shape} and {Y.shape}.")
    if not X.type() == Y.type():
        raise ValueError(f"Input images should have the same dtype, but got {X.type()} and {Y.type()}.")
    for d in range(X.dim() - 1, 1, -1):   # as pytorch_msssim: drop trailing singleton axes
        X, Y = X.squeeze(dim=d), Y.squeeze(dim=d)
    if X.dim() == 5:
        raise ValueError("5-D (video) inputs are not supported by the HIP SSIM (spatial_dims = 2 only)")
    if X.dim() != 4:
        raise ValueError(f"Input images should be 4-d tensors, but got {tuple(X.shape)}")
    if X.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise ValueError(f"ssim / ms_ssim take float32, float16 or bfloat16 inputs, not {X.dtype}")
    return X, Y


def _window(win_size: int, win_sigma: float, win):
    """The 1-D window as host floats (one row for every channel)."""
    if win is not None:
        win_size = win.shape[-1]
    if not (win_size % 2 == 1):
        raise ValueError("Window size should be odd.")
    if win_size > L.GDR_SSIM_MAX_WIN:
        raise ValueError(f"win_size {win_size} > {L.GDR_SSIM_MAX_WIN} is not supported by the HIP SSIM")
    if win is None:
        return win_size, _fspecial_gauss_1d(win_size, win_sigma).reshape(-1).tolist()
    rows = win.detach().to("cpu", torch.float32).reshape(-1, win_size)
    if not bool((rows == rows[0]).all()):
        raise ValueError("a per-channel-different win is not supported by the HIP SSIM (its rows must be identical)")
    return win_size, rows[0].tolist()


def _run(X, Y, data_range, win_size, win_sigma, win, K, mode, weights):
    X, Y = _check_inputs(X, Y)
    k, g = _window(win_size, win_sigma, win)
    B, Ch, H, W = X.shape
    if mode != L.GDR_SSIM_MS and min(H, W) < k:
        raise ValueError(f"image {H}x{W} is smaller than the {k}-pixel window (pytorch_msssim would skip filtering on that "
                         "axis; the HIP SSIM does not)")
    if not X.is_cuda:
        raise RuntimeError("ssim / ms_ssim run on ROCm/HIP tensors only (no CPU fallback)")
    a = L.GdrSsimArgs()
    a.B, a.C, a.H, a.W = B, Ch, H, W
    a.win_size, a.levels, a.mode = k, len(weights), mode
    K1, K2 = K
    a.C1, a.C2 = float((K1 * data_range) ** 2), float((K2 * data_range) ** 2)
    for i, v in enumerate(g):
        a.win[i] = v
    for i, v in enumerate(weights):
        a.weights[i] = float(v)
    return _SSIMFunction.apply(X.to(torch.float32), Y.to(torch.float32), a)


def _reduce(v, size_average, dtype):
    # fp16 / bf16 inputs: reduced in fp32, returned (and through autograd their gradients) in the input dtype
    return (v.mean() if size_average else v.mean(1)).to(dtype)


def ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None, K=(0.01, 0.03),
         nonnegative_ssim=False):
    """SSIM of (N, C, H, W) images X and Y: a scalar if size_average, else (N,)."""
    mode = L.GDR_SSIM_NONNEG if nonnegative_ssim else L.GDR_SSIM_PLAIN
    v = _run(X, Y, data_range, win_size, win_sigma, win, K, mode, (1.0,))
    return _reduce(v, size_average, X.dtype)


def ms_ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None, weights=None, K=(0.01, 0.03)):
    """MS-SSIM of (N, C, H, W) images X and Y: a scalar if size_average, else (N,)."""
    if win is not None:
        win_size = win.shape[-1]
    if weights is None:
        weights = _MS_WEIGHTS
    weights = [float(w) for w in (weights.tolist() if torch.is_tensor(weights) else weights)]
    if not 1 <= len(weights) <= L.GDR_SSIM_MAX_LEVELS:
        raise ValueError(f"ms_ssim takes 1..{L.GDR_SSIM_MAX_LEVELS} level weights, got {len(weights)}")
    smaller_side = min(X.shape[-2:])
    assert smaller_side > (win_size - 1) * (2 ** (len(weights) - 1)), \
        "Image size should be larger than %d due to the %d downsamplings in ms-ssim" % (
            (win_size - 1) * (2 ** (len(weights) - 1)), len(weights) - 1)
    v = _run(X, Y, data_range, win_size, win_sigma, win, K, L.GDR_SSIM_MS, weights)
    return _reduce(v, size_average, X.dtype)


class SSIM(torch.nn.Module):
    def __init__(self, data_range=255, size_average=True, win_size=11, win_sigma=1.5, channel=3, spatial_dims=2,
                 K=(0.01, 0.03), nonnegative_ssim=False):
        super().__init__()
        if spatial_dims != 2:
            raise ValueError("the HIP SSIM supports spatial_dims = 2 only")
        self.win_size = win_size
        self.win = _fspecial_gauss_1d(win_size, win_sigma).repeat([channel, 1] + [1] * spatial_dims)
        self.size_average = size_average
        self.data_range = data_range
        self.K = K
        self.nonnegative_ssim = nonnegative_ssim

    def forward(self, X, Y):
        return ssim(X, Y, data_range=self.data_range, size_average=self.size_average, win=self.win, K=self.K,
                    nonnegative_ssim=self.nonnegative_ssim)


class MS_SSIM(torch.nn.Module):
    def __init__(self, data_range=255, size_average=True, win_size=11, win_sigma=1.5, channel=3, spatial_dims=2,
                 weights=None, K=(0.01, 0.03)):
        super().__init__()
        if spatial_dims != 2:
            raise ValueError("the HIP MS-SSIM supports spatial_dims = 2 only")
        self.win_size = win_size
        self.win = _fspecial_gauss_1d(win_size, win_sigma).repeat([channel, 1] + [1] * spatial_dims)
        self.size_average = size_average
        self.data_range = data_range
        self.weights = weights
        self.K = K

    def forward(self, X, Y):
        return ms_ssim(X, Y, data_range=self.data_range, size_average=self.size_average, win=self.win,
                       weights=self.weights, K=self.K)
