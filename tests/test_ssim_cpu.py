"""CPU: the plain-torch SSIM / MS-SSIM restatement (tests/ssim_ref.py) against closed forms, autograd and an F.conv2d /
F.avg_pool2d composition; the `pytorch_msssim` drop-in's names, signatures and argument errors; the gdr_ssim_* exports."""
import ctypes as C
import inspect

import pytest
import torch
import torch.nn.functional as F

import ssim_cases as SC
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
    # a 1-tap window and a single level are supported: the host checks pass them on (here to the refusal of CPU tensors)
    tiny = torch.rand(1, 1, 4, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ms_ssim(tiny, tiny, win_size=1, weights=(0.3, 0.5, 0.4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ms_ssim(torch.rand(1, 1, 11, 11), torch.rand(1, 1, 11, 11), weights=(1.7,))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ssim(tiny, tiny, win_size=1)
    for bad in ((), (0.1,) * 9):        # 1..GDR_SSIM_MAX_LEVELS weights
        with pytest.raises(ValueError):
            ms_ssim(X, X, weights=bad)


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


# ---- the inputs of ssim_cases.py discriminate: mutants of the restatement ---------------------------------------------
# Each mutant is the restatement with one index wrong, in the way a kernel could be wrong.  On its NEW input (the one
# test_gpu_ssim.py now runs) it must miss the true restatement by more than the bars the GPU test applies
# (ssim_cases.beyond_bar); on the OLD inputs (what test_gpu_ssim.py fed before: one layout for X and Y, a uniform upstream
# gradient, the Gaussian window, the five default weights) `old_sees` records whether it was visible at all.
def _planes_grads(X, Y, r, op="ms_ssim", fwd_win=None, pool=None, weights=None, **kw):
    """(per-sample value, [dX, dY]) of the restatement for the upstream gradient r over the (B, C) planes.  `fwd_win`
    replaces the window in the value only (the gradient keeps the true one): a forward-only tap flip."""
    X = X.detach().requires_grad_(True)
    Y = Y.detach().requires_grad_(True)

    def run(win):
        if op == "ssim":
            return R.ssim_planes(X, Y, data_range=1.0, win=win, **kw)
        return R.ms_ssim_planes(X, Y, data_range=1.0, win=win, weights=weights, pool=pool, **kw)

    true_win = kw.pop("win", None)
    v = run(true_win)
    grads = list(torch.autograd.grad(v, [X, Y], r))
    if fwd_win is not None:
        with torch.no_grad():
            v = run(fwd_win)
    return v.detach(), grads


def _swapped_pool(x):
    """pool2 with pady and padx exchanged (the output keeps its size): rows padded by w % 2, columns by h % 2."""
    h, w = x.shape[-2:]
    h2, w2 = (h + h % 2) // 2, (w + w % 2) // 2
    x = F.pad(x, (h % 2, 2, w % 2, 2))[..., :2 * h2, :2 * w2]
    B, Ch = x.shape[:2]
    return x.reshape(B, Ch, h2, 2, w2, 2).sum(dim=(3, 5)) / 4


def _through_x_layout(X, Y):
    """Y's memory read through X's strides."""
    flat = Y.contiguous().view(-1) if Y.is_contiguous() else Y.permute(0, 2, 3, 1).contiguous().view(-1)
    assert flat.numel() == Y.numel()
    return torch.as_strided(flat, X.shape, X.stride())


def _five(w):
    """Weights cut or padded to five levels (a level count or a coef stride written as the constant 5)."""
    return tuple((list(w) + list(R.MS_WEIGHTS[len(w):]))[:5])


def _mutant_pair(name, old):
    """((value, grads) of the true restatement, (value, grads) of the mutant) on the new or the old input."""
    B, Ch = 3, 2
    if name.startswith("upstream"):
        X, Y = SC.images((B, Ch, 60, 75), seed=11, dtype=torch.float64)
        r = torch.full((B, Ch), 1.0 / Ch, dtype=torch.float64) if old else SC.upstream((B, Ch), 12, dtype=torch.float64)
        rm = {"upstream_rolled_b": r.roll(1, 0), "upstream_rolled_c": r.roll(1, 1),
              "upstream_transposed": r.t().reshape(B, Ch)}[name]
        kw = dict(op="ms_ssim", win_size=3, weights=(0.3, 0.5, 0.4))
        return _planes_grads(X, Y, r, **kw), _planes_grads(X, Y, rm, **kw)
    r = torch.ones(B, Ch, dtype=torch.float64)
    if name == "window_reversed_forward":
        X, Y = SC.images((B, Ch, 60, 75), seed=20, dtype=torch.float64)
        win = R.gauss_window(7, 1.0).double() if old else SC.asym_window(7, Ch).double().reshape(Ch, 7)[0]
        return (_planes_grads(X, Y, r, op="ssim", win=win), _planes_grads(X, Y, r, op="ssim", win=win, fwd_win=win.flip(0)))
    if name == "y_through_x_layout":
        X, Y = SC.images((B, Ch, 60, 75), seed=80, dtype=torch.float64)
        X, Y = SC.apply_layout(X, Y, "same" if old else "x_nhwc")
        return _planes_grads(X, Y, r, op="ssim"), _planes_grads(X, _through_x_layout(X, Y), r, op="ssim")
    if name == "pool_padding_swapped":
        # old: (2, 3, 333, 251) of test_ms_ssim_odd_sizes..., whose level 1 is 167 x 126 (odd, even) -- cut to one plane here
        shape = (1, 1, 333, 251) if old else (1, 1) + SC.AXIS_CASES["even_h_odd_w"]
        X, Y = SC.images(shape, seed=2 if old else 70, dtype=torch.float64)
        r = torch.ones(1, 1, dtype=torch.float64)
        return _planes_grads(X, Y, r), _planes_grads(X, Y, r, pool=_swapped_pool)
    if name == "weights_forced_to_five":
        w, k, _ = SC.LEVEL_CASES["L3"]
        w = R.MS_WEIGHTS if old else w
        X, Y = SC.images((B, Ch, 60, 75), seed=63, dtype=torch.float64)
        return _planes_grads(X, Y, r, win_size=3, weights=w), _planes_grads(X, Y, r, win_size=3, weights=_five(w))
    raise ValueError(name)


# mutant -> (the test of test_gpu_ssim.py whose input exposes it, did the old inputs see it?)
SSIM_MUTANTS = {
    "upstream_rolled_b": ("test_upstream_gradient_differs_for_every_plane", False),
    "upstream_rolled_c": ("test_upstream_gradient_differs_for_every_plane", False),
    "upstream_transposed": ("test_upstream_gradient_differs_for_every_plane", False),
    "window_reversed_forward": ("test_asymmetric_window_is_a_correlation_forward_and_transposed_backward", False),
    "y_through_x_layout": ("test_layouts_that_differ_between_x_and_y", False),
    # the old odd sizes already had one level with an odd H beside an even W: the claim of the issue is dropped; the new
    # sizes differ in parity at every level and in both directions
    "pool_padding_swapped": ("test_axes_that_differ_at_every_level", True),
    "weights_forced_to_five": ("test_level_counts_and_unequal_weights", False),
}


@pytest.mark.parametrize("name", list(SSIM_MUTANTS))
def test_new_inputs_expose_the_mutant_and_the_old_ones_did_not(name):
    import test_gpu_ssim

    gpu_test, old_sees = SSIM_MUTANTS[name]
    assert hasattr(test_gpu_ssim, gpu_test)
    (v, g), (vm, gm) = _mutant_pair(name, old=False)
    assert SC.beyond_bar(vm, gm, v, g), name
    (v, g), (vm, gm) = _mutant_pair(name, old=True)
    if old_sees:
        assert SC.beyond_bar(vm, gm, v, g), name
    else:      # not merely within the bars: identical
        assert torch.equal(vm, v) and all(torch.equal(a, b) for a, b in zip(gm, g)), name


def test_restatement_window_argument_is_a_correlation():
    """`win=` in the restatement: the taps as given, along H then W, as F.conv2d applies a (C, 1, 1, k) tensor."""
    X, _ = SC.images((1, 3, 40, 37), seed=4, dtype=torch.float64)
    win = SC.asym_window(7, 3).double()
    ref = F.conv2d(F.conv2d(X, win.transpose(2, 3), groups=3), win, groups=3)
    assert torch.allclose(R.blur(X, R._window(11, 1.5, win)), ref, atol=1e-14)
    assert not torch.allclose(R.blur(X, R._window(11, 1.5, win).flip(0)), ref, atol=1e-6)
    Y = X.flip(-1).contiguous()
    assert torch.equal(R.ssim(X, Y, data_range=1.0, win=win), R.ssim(X, Y, data_range=1.0, win=win.reshape(3, 7)[0]))
    assert torch.equal(R.ssim(X, Y, data_range=1.0), R.ssim(X, Y, data_range=1.0, win=R.gauss_window(11, 1.5)))
