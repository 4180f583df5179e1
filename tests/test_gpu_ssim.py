"""GPU: the HIP SSIM / MS-SSIM (csrc/ssim.hip through generativedensification_amd.ssim and the pytorch_msssim drop-in)
against the f64 plain-torch restatement (tests/ssim_ref.py), at the reference's training shape and on odd sizes, with
bitwise reproducibility, no host synchronisation, and end to end through the renderer with loss.py's formula."""
import pytest
import torch

import ssim_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _images(shape, seed=0, scale=1.0):
    """Smooth-plus-noise X and a noisier Y in [0, scale], fp32 on the GPU."""
    g = torch.Generator().manual_seed(seed)
    B, Ch, H, W = shape
    yy, xx = torch.meshgrid(torch.linspace(0, 3, H), torch.linspace(0, 5, W), indexing="ij")
    smooth = 0.5 + 0.3 * torch.sin(xx + yy)[None, None] * torch.linspace(0.5, 1.0, B * Ch).view(B, Ch, 1, 1)
    X = (smooth + 0.05 * torch.randn(shape, generator=g)).clamp(0, 1)
    Y = (X + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1)
    return (scale * X).to(DEV), (scale * Y).to(DEV)


def _assert_close(v, v64, grads, grads64):
    assert v.shape == v64.shape
    assert float((v.double() - v64).abs().max()) < 5e-6, (v, v64)
    for g, g64 in zip(grads, grads64):
        assert g.dtype == torch.float32 and bool(torch.isfinite(g).all())
        g, g64 = g.double(), g64.double()
        m = float(g64.abs().max())
        assert m > 0
        err = float((g - g64).abs().max())
        assert err <= 2e-4 * m, (err, m)
        cos = float((g * g64).sum() / (g.norm() * g64.norm()))
        assert cos >= 1 - 1e-6, cos


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
