"""CPU: the plain-torch SSIM / MS-SSIM restatement (tests/ssim_ref.py) against closed forms, autograd and an F.conv2d /
F.avg_pool2d composition; the `pytorch_msssim` drop-in's names, signatures and argument errors; the gdr_ssim_* exports."""
import ctypes as C
import inspect

import pytest
import torch
import torch.nn.functional as F

import ssim_ref as R


def _images(shape, seed=0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    B, Ch, H, W = shape
    yy, xx = torch.meshgrid(torch.linspace(0, 3, H, dtype=torch.float64), torch.linspace(0, 5, W, dtype=torch.float64),
                            indexing="ij")
    smooth = 0.5 + 0.3 * torch.sin(xx + yy)[None, None] * torch.linspace(0.5, 1.0, B * Ch, dtype=torch.float64).view(B, Ch, 1, 1)
    X = (smooth + 0.05 * torch.randn(shape, generator=g, dtype=torch.float64)).clamp(0, 1)
    Y = (X + 0.1 * torch.randn(shape, generator=g, dtype=torch.float64)).clamp(0, 1)
    return X.to(dtype), Y.to(dtype)


def _conv_ms_ssim(X, Y, data_range=1.0, win_size=11, win_sigma=1.5, weights=R.MS_WEIGHTS, K=(0.01, 0.03)):
    """The same algorithm written with grouped separable F.conv2d and F.avg_pool2d (what pytorch_msssim runs)."""
    Ch = X.shape[1]
    g = R.gauss_window(win_size, win_sigma).to(X.dtype)
    wh = g.view(1, 1, -1, 1).repeat(Ch, 1, 1, 1)
    ww = g.view(1, 1, 1, -1).repeat(Ch, 1, 1, 1)

    def filt(t):
        return F.conv2d(F.conv2d(t, wh, groups=Ch), ww, groups=Ch)

    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    vals = []
    for lvl in range(len(weights)):
        mx, my = filt(X), filt(Y)
        sxx, syy, sxy = filt(X * X) - mx ** 2, filt(Y * Y) - my ** 2, filt(X * Y) - mx * my
        cs_map = (2 * sxy + C2) / (sxx + syy + C2)
        ssim_map = (2 * mx * my + C1) / (mx ** 2 + my ** 2 + C1) * cs_map
        if lvl < len(weights) - 1:
            vals.append(torch.relu(cs_map.flatten(2).mean(-1)))
            pad = [s % 2 for s in X.shape[2:]]
            X = F.avg_pool2d(X, kernel_size=2, padding=pad)
            Y = F.avg_pool2d(Y, kernel_size=2, padding=pad)
    vals.append(torch.relu(ssim_map.flatten(2).mean(-1)))
    w = torch.tensor(weights, dtype=X.dtype)
    return torch.prod(torch.stack(vals) ** w.view(-1, 1, 1), dim=0)


def test_identity_symmetry_and_constant_closed_form():
    X, Y = _images((2, 3, 181, 175))
    assert torch.allclose(R.ssim(X, X, data_range=1.0), torch.tensor(1.0, dtype=X.dtype), atol=1e-12)
    assert torch.allclose(R.ms_ssim(X, X, data_range=1.0), torch.tensor(1.0, dtype=X.dtype), atol=1e-12)
    assert torch.allclose(R.ssim(X, Y, data_range=1.0, size_average=False), R.ssim(Y, X, data_range=1.0, size_average=False),
                          atol=1e-14)
    assert torch.allclose(R.ms_ssim(X, Y, data_range=1.0), R.ms_ssim(Y, X, data_range=1.0), atol=1e-14)
    a, b, dr = 0.3, 0.7, 1.0
    C1 = (0.01 * dr) ** 2
    Xc, Yc = torch.full((1, 2, 40, 33), a, dtype=torch.float64), torch.full((1, 2, 40, 33), b, dtype=torch.float64)
    # (the fp32 window sums to 1 within ~1e-7, so mu = a to that accuracy)
    assert torch.allclose(R.ssim(Xc, Yc, data_range=dr), torch.tensor((2 * a * b + C1) / (a * a + b * b + C1), dtype=torch.float64),
                          atol=1e-6)


def test_restatement_matches_conv2d_avg_pool2d_composition_on_odd_sizes():
    for shape in ((2, 3, 333, 251), (1, 1, 199, 170)):
        X, Y = _images(shape, seed=3)
        ref = _conv_ms_ssim(X, Y)
        got = R.ms_ssim(X, Y, data_range=1.0, size_average=False)
        assert torch.allclose(got, ref.mean(1), atol=1e-13, rtol=0), (got, ref)
    for h, w in ((7, 9), (8, 9), (7, 8)):   # the pool alone, odd and even axes
        x = torch.randn(2, 3, h, w, dtype=torch.float64)
        assert torch.allclose(R.pool2(x), F.avg_pool2d(x, 2, padding=[h % 2, w % 2]), atol=1e-15)
    X, Y = _images((1, 3, 40, 37), seed=4)
    g = R.gauss_window(7, 1.0).to(X.dtype)
    ref = F.conv2d(F.conv2d(X, g.view(1, 1, -1, 1).repeat(3, 1, 1, 1), groups=3), g.view(1, 1, 1, -1).repeat(3, 1, 1, 1), groups=3)
    assert torch.allclose(R.blur(X, R.gauss_window(7, 1.0)), ref, atol=1e-14)


def test_restatement_gradcheck_f64():
    X, Y = _images((1, 2, 23, 21), seed=5)
    X.requires_grad_(True)
    Y.requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: R.ssim(a, b, data_range=1.0, win_size=5, size_average=False), (X, Y))
    assert torch.autograd.gradcheck(lambda a, b: R.ms_ssim(a, b, data_range=1.0, win_size=3, weights=(0.3, 0.3, 0.4)), (X, Y))


def test_dropin_package_names_signatures_and_defaults():
    import pytorch_msssim as P
    from generativedensification_amd import ssim as S

    assert P.ssim is S.ssim and P.ms_ssim is S.ms_ssim and P.SSIM is S.SSIM and P.MS_SSIM is S.MS_SSIM
    assert P.__file__.startswith(str(__import__("os").path.dirname(__import__("os").path.dirname(__file__))))

    def sig(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]

    E = inspect.Parameter.empty
    assert sig(P.ssim) == [("X", E), ("Y", E), ("data_range", 255), ("size_average", True), ("win_size", 11),
                           ("win_sigma", 1.5), ("win", None), ("K", (0.01, 0.03)), ("nonnegative_ssim", False)]
    assert sig(P.ms_ssim) == [("X", E), ("Y", E), ("data_range", 255), ("size_average", True), ("win_size", 11),
                              ("win_sigma", 1.5), ("win", None), ("weights", None), ("K", (0.01, 0.03))]
    assert sig(P.SSIM.__init__)[1:] == [("data_range", 255), ("size_average", True), ("win_size", 11), ("win_sigma", 1.5),
                                        ("channel", 3), ("spatial_dims", 2), ("K", (0.01, 0.03)), ("nonnegative_ssim", False)]
    assert sig(P.MS_SSIM.__init__)[1:] == [("data_range", 255), ("size_average", True), ("win_size", 11), ("win_sigma", 1.5),
                                           ("channel", 3), ("spatial_dims", 2), ("weights", None), ("K", (0.01, 0.03))]
    assert issubclass(P.MS_SSIM, torch.nn.Module) and P.MS_SSIM(data_range=1.0).win.shape == (3, 1, 1, 11)


def test_argument_errors():
    from pytorch_msssim import MS_SSIM, SSIM, ms_ssim, ssim

    X = torch.rand(1, 3, 200, 200)
    with pytest.raises(ValueError):
        ssim(X, torch.rand(1, 3, 200, 199))
    with pytest.raises(ValueError):
        ssim(X, X.double())
    with pytest.raises(ValueError):
        ssim(X, X, win_size=10)
    with pytest.raises(AssertionError):
        ms_ssim(torch.rand(1, 3, 160, 400), torch.rand(1, 3, 160, 400))
    with pytest.raises(RuntimeError):   # CPU tensors: no fallback
        ssim(X, X)
    with pytest.raises(RuntimeError):
        ms_ssim(X, X)
    with pytest.raises(ValueError):     # 5-D video
        ssim(torch.rand(1, 3, 4, 20, 20), torch.rand(1, 3, 4, 20, 20))
    with pytest.raises(ValueError):     # beyond the LDS bound
        ssim(X, X, win_size=17)
    with pytest.raises(ValueError):
        SSIM(spatial_dims=3)
    with pytest.raises(ValueError):
        MS_SSIM(spatial_dims=3)
    win = torch.rand(3, 1, 1, 11)
    with pytest.raises(ValueError):     # per-channel-different window
        ssim(X, X, win=win)


def test_library_exports_the_ssim_entry_points_and_refuses_bad_sizes():
    from generativedensification_amd import _lib as L

    lib = L.load()
    for n in ("gdr_ssim_workspace_bytes", "gdr_ssim_scratch_bytes", "gdr_ssim_forward", "gdr_ssim_backward"):
        assert hasattr(lib, n) and n in L.EXPORTED_SYMBOLS
    a = L.GdrSsimArgs()
    a.B, a.C, a.H, a.W, a.win_size, a.levels, a.mode = 3, 3, 512, 4096, 11, 5, L.GDR_SSIM_MS
    n = lib.gdr_ssim_workspace_bytes(C.byref(a))
    # pooled pyramid (levels 1..4 of X and Y) + partials + coefficients
    assert n >= 2 * 9 * 4 * sum((512 >> l) * (4096 >> l) for l in range(1, 5))
    assert lib.gdr_ssim_scratch_bytes(C.byref(a), 1) >= 9 * 502 * 4086 * 16
    assert lib.gdr_ssim_scratch_bytes(C.byref(a), 1) > lib.gdr_ssim_scratch_bytes(C.byref(a), 0)
    a.win_size = 10
    assert lib.gdr_ssim_workspace_bytes(C.byref(a)) == 0 and b"odd" in lib.gdr_last_error()
    a.win_size, a.H = 11, 100     # level 4 would be 7 rows < the window
    assert lib.gdr_ssim_workspace_bytes(C.byref(a)) == 0 and b"smaller" in lib.gdr_last_error()
    a.H, a.mode = 512, L.GDR_SSIM_PLAIN   # ssim() has exactly one level
    assert lib.gdr_ssim_workspace_bytes(C.byref(a)) == 0
    st = (C.c_int64 * 4)(0, 0, 0, 0)
    # refused before any launch: NULL buffers
    a.mode = L.GDR_SSIM_MS
    assert lib.gdr_ssim_forward(C.byref(a), None, st, None, st, None, None, None) == -1
    assert lib.gdr_ssim_backward(C.byref(a), None, st, None, st, None, None, None, st, None, None, None, None) == -1
