"""GPU: the HIP SSIM / MS-SSIM (csrc/ssim.hip through generativedensification_amd.ssim and the pytorch_msssim drop-in)
against the f64 plain-torch restatement (tests/ssim_ref.py), at the reference's training shape and on odd sizes, with
bitwise reproducibility, no host synchronisation, and end to end through the renderer with loss.py's formula; then on the
inputs of tests/ssim_cases.py, which break the symmetries of the kernels' index arithmetic (a per-plane upstream gradient,
an asymmetric window, every dispatched window size, level counts, axes and layouts that differ, flat content, graphs that
share nothing).  tests/test_ssim_cpu.py shows on mutants of the restatement that those inputs discriminate."""
import pytest
import torch

import ssim_cases as SC
import ssim_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _images(shape, seed=0, scale=1.0):
    """Smooth-plus-noise X and a noisier Y in [0, scale], fp32 on the GPU."""
    return SC.images(shape, seed, scale, DEV)


def _assert_close(v, v64, grads, grads64, value_atol=SC.VALUE_ATOL, grad_rtol=SC.GRAD_RTOL):
    """value 5e-6 absolute, gradient 2e-4 of the f64 maximum, cosine >= 1 - 1e-6 (ssim_cases holds the numbers); a case
    passes other bars only where it states the fp32-restatement error they come from."""
    assert v.shape == v64.shape
    err_v = float((v.double() - v64).abs().max())
    print(f"value err {err_v:.3e}")
    assert err_v < value_atol, (v, v64)
    for g, g64 in zip(grads, grads64):
        assert g.dtype == torch.float32 and bool(torch.isfinite(g).all())
        g, g64 = g.double(), g64.double()
        m = float(g64.abs().max())
        assert m > 0
        err = float((g - g64).abs().max())
        cos = float((g * g64).sum() / (g.norm() * g64.norm()))
        print(f"grad err {err:.3e} of max {m:.3e} ({err / m:.3e}), 1 - cos {1 - cos:.3e}")
        assert err <= grad_rtol * m, (err, m)
        assert cos >= SC.COS_MIN, cos


def _run(fn, X, Y, grad_y=True):
    X = X.detach().clone().requires_grad_(True)
    Y = Y.detach().clone().requires_grad_(grad_y)
    v = fn(X, Y)
    v.sum().backward()
    return v.detach(), [X.grad] + ([Y.grad] if grad_y else [])


def test_ms_ssim_at_the_reference_training_shape_from_a_permuted_nhwc_view():
    from pytorch_msssim import MS_SSIM

    B, H, W = 3, 512, 4096
    X, Y = _images((B, 3, H, W), seed=1)
    img = X.permute(0, 2, 3, 1).contiguous()     # (B, H, V*W, 3) as the renderer's output
    tar = Y.permute(0, 2, 3, 1).contiguous()
    crit = MS_SSIM(data_range=1.0, size_average=True, channel=3)
    img_h = img.clone().requires_grad_(True)
    v = crit(img_h.permute(0, 3, 1, 2), tar.permute(0, 3, 1, 2))
    v.backward()
    img64 = img.double().requires_grad_(True)
    v64 = R.ms_ssim(img64.permute(0, 3, 1, 2), tar.double().permute(0, 3, 1, 2), data_range=1.0)
    v64.backward()
    assert img_h.grad.stride() == img_h.stride()
    _assert_close(v.detach().reshape(1), v64.detach().reshape(1), [img_h.grad], [img64.grad])


@pytest.mark.parametrize("shape", [(2, 3, 333, 251), (1, 1, 201, 170), (2, 4, 177, 190)])
def test_ms_ssim_odd_sizes_and_channel_counts_grads_of_x_and_y(shape):
    from pytorch_msssim import ms_ssim

    X, Y = _images(shape, seed=2)
    v, gr = _run(lambda a, b: ms_ssim(a, b, data_range=1.0, size_average=False), X, Y)
    v64, gr64 = _run(lambda a, b: R.ms_ssim(a, b, data_range=1.0, size_average=False), X.double(), Y.double())
    _assert_close(v, v64, gr, gr64)


@pytest.mark.parametrize("nonneg", [False, True])
def test_ssim_per_sample_custom_window_constants_and_range(nonneg):
    from pytorch_msssim import ssim

    X, Y = _images((2, 3, 97, 130), seed=3, scale=255.0)
    kw = dict(data_range=255, size_average=False, win_size=7, win_sigma=1.0, K=(0.02, 0.04), nonnegative_ssim=nonneg)
    v, gr = _run(lambda a, b: ssim(a, b, **kw), X, Y)
    v64, gr64 = _run(lambda a, b: R.ssim(a, b, **kw), X.double(), Y.double())
    _assert_close(v, v64, gr, gr64)
    # defaults (11 / 1.5, size_average) and the module with its (C, 1, 1, k) window of identical rows
    from pytorch_msssim import SSIM
    X, Y = _images((1, 1, 64, 80), seed=4)
    v, gr = _run(lambda a, b: SSIM(data_range=1.0, channel=1, nonnegative_ssim=nonneg)(a, b).reshape(1), X, Y, grad_y=False)
    v64, gr64 = _run(lambda a, b: R.ssim(a, b, data_range=1.0, nonnegative_ssim=nonneg).reshape(1), X.double(), Y.double(),
                     grad_y=False)
    _assert_close(v, v64, gr, gr64)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_inputs_compute_in_fp32_and_return_grads_in_their_dtype(dtype):
    from pytorch_msssim import ms_ssim

    X, Y = _images((1, 3, 200, 230), seed=5)
    Xh, Yh = X.to(dtype), Y.to(dtype)
    v, gr = _run(lambda a, b: ms_ssim(a, b, data_range=1.0), Xh, Yh)
    v32, gr32 = _run(lambda a, b: ms_ssim(a, b, data_range=1.0), Xh.float(), Yh.float())
    assert all(g.dtype == dtype for g in gr)
    assert torch.equal(v.float(), v32.to(v.dtype).float())
    for g, g32 in zip(gr, gr32):
        assert torch.equal(g, g32.to(dtype))
    v64, gr64 = _run(lambda a, b: R.ms_ssim(a, b, data_range=1.0), Xh.double(), Yh.double())
    _assert_close(v32.reshape(1), v64.reshape(1), gr32, gr64)


def test_clamped_level_gives_an_exactly_zero_finite_gradient():
    from pytorch_msssim import ms_ssim

    X, Y = _images((2, 1, 180, 200), seed=6)
    g = torch.Generator().manual_seed(7)
    noise = torch.rand(180, 200, generator=g).to(DEV)
    X[0, 0], Y[0, 0] = noise, 1.0 - noise       # anti-correlated sample: cs < 0 at level 0, relu clamps it
    v, gr = _run(lambda a, b: ms_ssim(a, b, data_range=1.0, size_average=False), X, Y)
    v64, gr64 = _run(lambda a, b: R.ms_ssim(a, b, data_range=1.0, size_average=False), X.double(), Y.double())
    assert float(v64[0]) == 0.0 and float(v[0]) == 0.0 and float(v[1]) > 0.5
    for g in gr:
        assert bool(torch.isfinite(g).all())
        assert bool((g[0] == 0).all())
        assert float(g[1].abs().max()) > 0
    _assert_close(v, v64, gr, gr64)


def test_two_runs_are_bitwise_equal_and_no_host_synchronisation():
    from pytorch_msssim import MS_SSIM, ssim

    X, Y = _images((2, 3, 256, 512), seed=8)
    crit = MS_SSIM(data_range=1.0, channel=3)
    runs = []
    for _ in range(2):
        a, b = X.clone().requires_grad_(True), Y.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            v = crit(a, b)
            v.backward()
            s = ssim(a.detach(), b, data_range=1.0, size_average=False)
            s.sum().backward()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        runs.append((v.detach().clone(), s.detach().clone(), a.grad.clone(), b.grad.clone()))
    for t0, t1 in zip(*runs):
        assert torch.equal(t0, t1)


def test_end_to_end_rendered_views_with_the_reference_loss():
    from generativedensification_amd.camera import orbit_cameras
    from generativedensification_amd.renderer import Renderer
    from generativedensification_amd.synthetic import make_scene, make_targets
    from pytorch_msssim import MS_SSIM

    H, W, V = 192, 192, 4
    scene = make_scene(20000, seed=21, sh_degree=3, sigma0=(0.02, 0.005))
    cams = orbit_cameras(V, W, H, device="cpu")
    for cam in cams:
        for attr in ("world_view_transform", "full_proj_transform", "camera_center"):
            setattr(cam, attr, getattr(cam, attr).to(DEV))
    tar = make_targets(1, H, V * W, 22).to(DEV)            # (1, H, V*W, 3)
    crit = MS_SSIM(data_range=1.0, size_average=True, channel=3)

    def step(msssim):
        r = Renderer(sh_degree=3, white_background=True)
        g = {k: v.to(DEV).requires_grad_(True) for k, v in scene.items()}
        views = [r.render_img(c, None, g["centers"], g["shs"], g["opacity"], g["scales"], g["rotations"], DEV) for c in cams]
        image = torch.stack([torch.cat([o["image"] for o in views], dim=1)])   # network.py: views along the width
        loss = ((image - tar) ** 2).mean() + 0.5 * (1 - msssim(image.permute(0, 3, 1, 2), tar.permute(0, 3, 1, 2)))
        loss.backward()
        return float(loss.detach()), {k: v.grad for k, v in g.items()}

    loss, grads = step(crit)
    loss_ref, grads_ref = step(lambda a, b: R.ms_ssim(a, b, data_range=1.0))
    assert abs(loss - loss_ref) < 1e-5
    for k in grads:
        g, gr = grads[k], grads_ref[k]
        assert bool(torch.isfinite(g).all())
        m = float(gr.abs().max())
        assert float((g - gr).abs().max()) <= 2e-4 * m, k


# ---- inputs that break the kernels' symmetries (tests/ssim_cases.py) -------------------------------------------------
def _product(op, planes):
    """ssim / ms_ssim of the drop-in, or the raw (B, C) per-plane output of _SSIMFunction."""
    import pytorch_msssim as P
    from generativedensification_amd import _lib as L
    from generativedensification_amd import ssim as S

    if not planes:
        return getattr(P, op)

    def raw(X, Y, data_range=255, win_size=11, win_sigma=1.5, win=None, K=(0.01, 0.03), nonnegative_ssim=False,
            weights=None):
        if op == "ssim":
            return S._run(X, Y, data_range, win_size, win_sigma, win, K,
                          L.GDR_SSIM_NONNEG if nonnegative_ssim else L.GDR_SSIM_PLAIN, (1.0,))
        return S._run(X, Y, data_range, win_size, win_sigma, win, K, L.GDR_SSIM_MS,
                      list(R.MS_WEIGHTS if weights is None else weights))
    return raw


def _restated(op, planes):
    return getattr(R, op + "_planes") if planes else getattr(R, op)


def _grads(fn, X, Y, r, grad_y, kw):
    """(value, [dX, dY]) straight from the backward node (torch.autograd.grad: no accumulation into a leaf, so the strides
    are the ones the product chose).  X and Y keep their layouts: no clone."""
    X = X.detach().requires_grad_(True)
    Y = Y.detach().requires_grad_(grad_y)
    v = fn(X, Y, **kw)
    r = torch.ones_like(v) if r is None else r.to(v.dtype)
    return v.detach(), list(torch.autograd.grad(v, [X, Y] if grad_y else [X], r))


def _check(op, X, Y, kw, r=None, grad_y=True, planes=False, **bars):
    v, gr = _grads(_product(op, planes), X, Y, r, grad_y, kw)
    kw64 = {k: (t.double() if torch.is_tensor(t) and t.is_floating_point() else t) for k, t in kw.items()}
    v64, gr64 = _grads(_restated(op, planes), X.double(), Y.double(), None if r is None else r.double(), grad_y, kw64)
    if v.dim() == 0:
        v, v64 = v.reshape(1), v64.reshape(1)
    _assert_close(v, v64, gr, gr64, **bars)
    return v, gr


_UPSTREAM_OPS = {"ssim": ("ssim", {}), "ssim_nonneg": ("ssim", {"nonnegative_ssim": True}), "ms_ssim": ("ms_ssim", {})}


@pytest.mark.parametrize("planes", [False, True], ids=["per_sample", "per_plane"])
@pytest.mark.parametrize("name", list(_UPSTREAM_OPS))
def test_upstream_gradient_differs_for_every_plane(name, planes):
    """A.1: go[p] is read at p = b * C + c.  B = 3, C = 2 (so B != C and a transposed or rolled read lands elsewhere)."""
    op, extra = _UPSTREAM_OPS[name]
    B, C = 3, 2
    X, Y = SC.images((B, C, 177, 190), seed=11, device=DEV)
    r = SC.upstream((B, C) if planes else (B,), seed=12, device=DEV)
    kw = dict(data_range=1.0, **extra)
    if not planes:
        kw["size_average"] = False
    _check(op, X, Y, kw, r=r, planes=planes)


@pytest.mark.parametrize("k", [3, 7, 15])
@pytest.mark.parametrize("op", ["ssim", "ms_ssim"])
def test_asymmetric_window_is_a_correlation_forward_and_transposed_backward(op, k):
    """A.2: monotone taps through win=; a flipped tap order in either direction changes the value or the gradient."""
    win = SC.asym_window(k, 3).to(DEV)
    H, W = (97, 130) if op == "ssim" else ((k - 1) * 16 + 9, (k - 1) * 16 + 30)
    X, Y = SC.images((2, 3, H, W), seed=13 + k, device=DEV)
    _check(op, X, Y, dict(data_range=1.0, size_average=False, win=win))


@pytest.mark.parametrize("k", SC.WINDOW_SIZES)
@pytest.mark.parametrize("region", ["tile_plus_one", "one_pixel"])
def test_every_dispatched_window_size(region, k):
    """A.3: every K of GDR_SSIM_DISPATCH with a valid region one pixel past a 16 x 64 tile on each axis (ssim), and with
    a valid region of exactly one pixel on the coarsest of three levels (ms_ssim)."""
    sigma = max(k / 7.0, 0.5)
    if region == "tile_plus_one":
        shape = SC.tile_crossing_shape(k)
        assert (shape[2] - k + 1) % 16 == 1 and (shape[3] - k + 1) % 64 == 1
        X, Y = SC.images(shape, seed=20 + k, device=DEV)
        _check("ssim", X, Y, dict(data_range=1.0, size_average=False, win_size=k, win_sigma=sigma))
    else:
        shape = SC.one_pixel_shape(k)
        assert SC.pyramid(shape[2], shape[3], 3)[-1] == (k, k)
        X, Y = SC.images(shape, seed=40 + k, device=DEV)
        # K = 1: every variance is x*x - x*x, so cs == 1 and its gradient is pure cancellation, amplified by 1 / C2 = 1111.
        # The fp32 restatement on the CPU misses the f64 gradient of this input by 4.07e-4 of its maximum (dX; dY 2.90e-4),
        # above the common 2e-4: the bar of this one case is 4 x 4.07e-4 (another valid fp32 summation order).
        bars = dict(grad_rtol=4 * 4.07e-4) if k == 1 else {}
        _check("ms_ssim", X, Y, dict(data_range=1.0, size_average=False, win_size=k, win_sigma=sigma,
                                     weights=SC.ONE_PIXEL_WEIGHTS), **bars)


@pytest.mark.parametrize("name", list(SC.LEVEL_CASES) + ["L3_tensor"])
def test_level_counts_and_unequal_weights(name):
    """A.4: 1, 2, 3 and 8 (GDR_SSIM_MAX_LEVELS) levels with unequal weights that do not sum to 1; one tensor-valued."""
    weights, k, (H, W) = SC.LEVEL_CASES[name[:2]]
    if name.endswith("tensor"):
        weights = torch.tensor(weights, device=DEV)
    X, Y = SC.images((2, 2, H, W), seed=60 + len(weights), device=DEV)
    r = SC.upstream((2,), seed=61, device=DEV)
    _check("ms_ssim", X, Y, dict(data_range=1.0, size_average=False, win_size=k, weights=weights), r=r)


@pytest.mark.parametrize("name", list(SC.AXIS_CASES))
def test_axes_that_differ_at_every_level(name):
    """A.5 (per-level sizes in ssim_cases.AXIS_CASES): pady != padx at every pool, and extreme aspect ratios."""
    H, W = SC.AXIS_CASES[name]
    if name == "even_h_odd_w":
        assert all(h % 2 == 0 and w % 2 == 1 for h, w in SC.pyramid(H, W, 5))
    if name == "odd_h_even_w":
        assert all(h % 2 == 1 and w % 2 == 0 for h, w in SC.pyramid(H, W, 5))
    X, Y = SC.images((1, 2, H, W), seed=70, device=DEV)
    _check("ms_ssim", X, Y, dict(data_range=1.0, size_average=False))


@pytest.mark.parametrize("layout", SC.LAYOUTS)
@pytest.mark.parametrize("op", ["ssim", "ms_ssim"])
def test_layouts_that_differ_between_x_and_y(op, layout):
    """A.6: X, Y, dX and dY each go through their own strides."""
    X, Y = SC.images((3, 3, 177, 190), seed=80, device=DEV)
    X, Y = SC.apply_layout(X, Y, layout)
    grad_y = layout != "y_expand"
    assert X.stride() != Y.stride()
    r = SC.upstream((3,), seed=81, device=DEV)
    _, gr = _check(op, X, Y, dict(data_range=1.0, size_average=False), r=r, grad_y=grad_y)
    # the gradients come back dense, in the memory order of their input
    assert gr[0].stride() == torch.empty_like(X).stride()
    if layout == "x_nhwc":
        assert gr[0].stride() == X.stride() and gr[1].is_contiguous()
    elif layout == "y_nhwc":
        assert gr[0].is_contiguous() and gr[1].stride() == Y.stride()
    elif layout == "x_slice":
        assert gr[0].is_contiguous() and gr[1].is_contiguous()
    else:
        assert gr[0].is_contiguous() and len(gr) == 1


@pytest.mark.parametrize("op", ["ssim", "ms_ssim"])
def test_half_white_half_textured(op):
    """A.7: the renderer's white background beside content."""
    X, Y = SC.flat_images("half_white", (2, 3, 177, 190), seed=90, device=DEV)
    _check(op, X, Y, dict(data_range=1.0, size_average=False))


@pytest.mark.parametrize("kind", ["white", "identical"])
@pytest.mark.parametrize("op", ["ssim", "ms_ssim"])
def test_equal_images_give_one_and_a_vanishing_gradient(op, kind):
    """A.7: X == Y (constant white, or textured).  The value is 1 and the f64 gradient is zero (to f64 rounding), so
    _assert_close's relative bar has no scale.  The bar is absolute instead: 2e-4 (the relative bar) of the gradient
    maximum of a perturbed copy, the same X against the noisier Y of ssim_cases.images on the same seed."""
    shape = (2, 3, 177, 190)
    X, Y = SC.flat_images(kind, shape, seed=91, device=DEV)
    kw = dict(data_range=1.0, size_average=False)
    v, gr = _grads(_product(op, False), X, Y, None, True, kw)
    v64, gr64 = _grads(_restated(op, False), X.double(), Y.double(), None, True, kw)
    Xp, Yp = SC.images(shape, seed=91, device=DEV)
    _, grp = _grads(_restated(op, False), Xp.double(), Yp.double(), None, True, kw)
    assert float((v.double() - v64).abs().max()) < SC.VALUE_ATOL and float((v64 - 1).abs().max()) < 1e-12
    for g, g64, gp in zip(gr, gr64, grp):
        scale = float(gp.abs().max())
        assert float(g64.abs().max()) < 1e-9 * scale
        err = float((g.double() - g64).abs().max())
        print(f"{op} {kind}: |grad| {err:.3e} against a perturbed copy's {scale:.3e}")
        assert bool(torch.isfinite(g).all()) and err <= SC.GRAD_RTOL * scale, (err, scale)


def test_ms_ssim_data_range_255():
    """A.7: C1, C2 scale with data_range^2 and the images with data_range."""
    X, Y = SC.images((2, 3, 177, 190), seed=92, scale=255.0, device=DEV)
    _check("ms_ssim", X, Y, dict(data_range=255, size_average=False))


def test_backward_twice_and_two_graphs_alive_at_once():
    """A.8: the forward workspace is kept on ctx.  A second backward of the same graph and a backward of another graph
    (other images, other window size, other level count) that ran in between give bitwise the results of single runs."""
    from pytorch_msssim import ms_ssim

    XA, YA = SC.images((2, 3, 177, 190), seed=95, device=DEV)
    XB, YB = SC.images((2, 3, 120, 97), seed=96, device=DEV)
    kwA = dict(data_range=1.0, size_average=False)
    kwB = dict(data_range=1.0, size_average=False, win_size=5, weights=(0.4, 0.9, 0.6))
    rA, rB = SC.upstream((2,), 97, DEV), SC.upstream((2,), 98, DEV)
    vA1, gA1 = _grads(ms_ssim, XA, YA, rA, True, kwA)          # single runs
    vB1, gB1 = _grads(ms_ssim, XB, YB, rB, True, kwB)
    xa, ya = XA.clone().requires_grad_(True), YA.clone().requires_grad_(True)
    xb, yb = XB.clone().requires_grad_(True), YB.clone().requires_grad_(True)
    va = ms_ssim(xa, ya, **kwA)                                  # both graphs alive
    vb = ms_ssim(xb, yb, **kwB)
    ga1 = torch.autograd.grad(va, [xa, ya], rA, retain_graph=True)
    gb1 = torch.autograd.grad(vb, [xb, yb], rB, retain_graph=True)
    ga2 = torch.autograd.grad(va, [xa, ya], rA, retain_graph=True)
    gb2 = torch.autograd.grad(vb, [xb, yb], rB)
    assert torch.equal(va.detach(), vA1) and torch.equal(vb.detach(), vB1)
    for got, want in ((ga1, gA1), (ga2, gA1), (gb1, gB1), (gb2, gB1)):
        for g, w in zip(got, want):
            assert torch.equal(g, w)
    _check("ms_ssim", XB, YB, kwB, r=rB)
