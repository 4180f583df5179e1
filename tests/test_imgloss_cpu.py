"""CPU: the restatement of the image-space kernels (tests/imgloss_ref.py) against the adaptor's own torch sequence, autograd's
numerical check and hand-made planes; the inputs' conditioning (tests/imgloss_cases.py); the C ABI of csrc/loss.hip and
csrc/maps_surfel.hip as far as it goes without a device; and the refusals of the Python wrappers' argument check."""
import math

import pytest
import torch

import imgloss_cases as K
import imgloss_ref as R

GDR_ERR_INVALID_ARG = -1      # include/gdr.h
ALL_SHAPES = K.SMALL_SHAPES + (K.STRIDE_FWD, K.STRIDE_BWD)


def _adaptor_ops(a, rays, view, ratio):
    """renderer_2dgs.Renderer.render_img's torch branch, from allmap on"""
    from generativedensification_amd.renderer_2dgs import depth_to_normal

    alpha = a[1:2]
    normal_world = (a[2:5].permute(1, 2, 0) @ view[:3, :3].T).permute(2, 0, 1)
    depth_median = torch.nan_to_num(a[5:6], 0, 0)
    depth_expected = torch.nan_to_num(a[0:1] / alpha, 0, 0)
    surf_depth = depth_expected * (1 - ratio) + ratio * depth_median
    surf_normal, _ = depth_to_normal(rays, surf_depth)
    surf_normal = surf_normal.permute(2, 0, 1) * alpha.detach()
    return (surf_depth.permute(1, 2, 0), alpha.squeeze(0), normal_world.permute(1, 2, 0), surf_normal.permute(1, 2, 0),
            a[6:7].squeeze(0))


@pytest.mark.parametrize("ratio", K.RATIOS)
def test_maps_in_float32_are_the_adaptor_ops_bit_for_bit(ratio):
    for case in (K.smooth(57, 83), K.special()):
        want = _adaptor_ops(case["allmap"], case["rays"], case["view"], ratio)
        plain = R.maps(case["allmap"], case["rays"], case["view"], ratio)
        masked = R.maps(case["allmap"], case["rays"], case["view"], ratio, R.masks(case["allmap"]))
        for name, w, p, m in zip(R.MAP_NAMES, want, plain, masked):
            assert w.shape == p.shape == m.shape, name
            assert torch.equal(torch.isnan(w), torch.isnan(p)) and torch.equal(torch.nan_to_num(w, 7.0), torch.nan_to_num(p, 7.0)), name
            assert torch.equal(torch.nan_to_num(w, 7.0), torch.nan_to_num(m, 7.0)), name     # the mask changes no value
    # and no gradient where torch's is finite; where torch's is NaN (allmap[0:2] of empty pixels) the masked one is finite
    case = K.smooth(57, 83)
    ups = K.upstreams(57, 83)
    a1 = case["allmap"].clone().requires_grad_(True)
    torch.autograd.backward(_adaptor_ops(a1, case["rays"], case["view"], ratio), ups)
    g = R.run_maps(case, ratio, torch.float32, ups)["dL_dallmap"]
    nan = torch.isnan(a1.grad)
    assert torch.equal(nan[0], case["empty"]) and torch.equal(nan[1], case["empty"]) and not nan[2:].any()
    assert torch.isfinite(g).all() and torch.equal(g[~nan], a1.grad[~nan])
    assert torch.equal(g[0][case["empty"]], torch.zeros(int(case["empty"].sum())))
    assert torch.equal(g[1][case["empty"]], ups[1][case["empty"]])


def test_losses_equal_the_synthetic_losses_on_the_same_dict():
    from generativedensification_amd.synthetic import surfel_loss, view_loss

    H, W = 57, 83
    case = K.smooth(H, W)
    tg_hwc = case["target"].permute(1, 2, 0).contiguous()
    tg_chw = tg_hwc.permute(2, 0, 1)
    image = case["color"].clamp(0, 1).permute(1, 2, 0)
    for ratio in K.RATIOS:
        out = dict(zip(("depth", "acc_map", "rend_normal", "depth_normal", "rend_dist"),
                       _adaptor_ops(case["allmap"], case["rays"], case["view"], ratio)), image=image)
        got = R.surfel_loss(case["color"], case["allmap"], case["rays"], case["view"], tg_chw, ratio)
        assert torch.equal(got, surfel_loss(out, tg_hwc))
        terms = R.surfel_terms(*(case[k].double() for k in ("color", "allmap", "rays", "view", "target")), ratio)
        assert abs(float(terms.sum()) - float(got)) < 1e-5 * abs(float(got))
    out = {"image": image, "depth": case["depth"].permute(1, 2, 0), "acc_map": case["alpha"].squeeze(0)}
    got = R.view_loss(case["color"], case["depth"], case["alpha"], tg_chw)
    assert torch.equal(got, view_loss(out, tg_hwc))
    terms = R.view_terms(*(case[k].double() for k in ("color", "depth", "alpha", "target")))
    assert abs(float(terms.sum()) - float(got)) < 1e-5 * abs(float(got))


def test_gradcheck_of_the_f64_restatement():
    H, W = 5, 6
    case = {k: v.double() for k, v in K.smooth(H, W, holes=False).items() if k != "empty"}
    mask = R.masks(case["allmap"])
    color = case["color"].clone().requires_grad_(True)
    depth, alpha = case["depth"].clone().requires_grad_(True), case["alpha"].clone().requires_grad_(True)
    # alpha is detached inside depth_normal and inside the normal term, which a numerical derivative cannot know: the other
    # six channels are checked on everything with alpha held constant, alpha on what does not detach it
    rest = torch.cat((case["allmap"][0:1], case["allmap"][2:])).requires_grad_(True)
    const_a, args = case["allmap"][1:2], (case["rays"], case["view"])
    join = lambda x, a: torch.cat((x[0:1], a, x[1:]))
    for ratio in K.RATIOS:
        assert torch.autograd.gradcheck(lambda x: R.maps(join(x, const_a), *args, ratio, mask), (rest,))
        assert torch.autograd.gradcheck(lambda a: R.maps(join(rest.detach(), a), *args, ratio, mask)[:2], (alpha,))
        assert torch.autograd.gradcheck(lambda c, x: R.surfel_loss(c, join(x, const_a), *args, case["target"], ratio, mask=mask),
                                        (color, rest))
        assert torch.autograd.gradcheck(lambda a: R.surfel_loss(color.detach(), join(rest.detach(), a), *args, case["target"], ratio,
                                                                w_normal=0.0, mask=mask), (alpha,))
    assert torch.autograd.gradcheck(lambda c, d, a: R.view_loss(c, d, a, case["target"]), (color, depth, alpha))


def _plane(H, W, p, q):
    """parallel rays along +z from (x, y, 0); depth 1 + p x + q y: the surface z = 1 + p x + q y"""
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    rays = torch.stack((xx, yy, torch.zeros_like(xx), torch.zeros_like(xx), torch.zeros_like(xx), torch.ones_like(xx)), dim=-1)
    return rays, (1 + p * xx + q * yy)[None]


def test_pseudo_normal_of_a_plane_by_hand():
    H, W, p, q = 5, 7, 0.3, -0.7
    n = lambda a, b: torch.tensor([a, b, -1.0], dtype=torch.float64) / math.sqrt(a * a + b * b + 1)
    rays, depth = _plane(H, W, p, q)
    got = R.pseudo_normal(rays, depth)
    # row difference (0, 2, 2q) x column difference (2, 0, 2p) = (4p, 4q, -4)
    assert (got[1:-1, 1:-1] - n(p, q)).abs().max() < 1e-15
    assert torch.equal(got[0], torch.zeros(W, 3, dtype=torch.float64)) and torch.equal(got[:, -1], torch.zeros(H, 3, dtype=torch.float64))
    # the mirror image in x flips the x component only
    mirrored = R.pseudo_normal(rays, depth.flip(-1))
    assert (mirrored[1:-1, 1:-1] - n(-p, q)).abs().max() < 1e-15
    # rows and columns swapped: the plane z = 1 + q x + p y, another normal
    rays_t, _ = _plane(W, H, p, q)
    swapped = R.pseudo_normal(rays_t, depth.transpose(1, 2))
    assert (swapped[1:-1, 1:-1] - n(q, p)).abs().max() < 1e-15 and (n(q, p) - n(p, q)).abs().max() > 0.5
    # through the maps: alpha scales it, the ratio mixes the two depths, the view matrix turns only the rendered normal
    am = torch.zeros(7, H, W, dtype=torch.float64)
    am[1] = 0.5
    am[0], am[5] = 0.5 * depth[0], depth[0] + 1.0
    am[2] = 1.0
    view = torch.eye(4, dtype=torch.float64)
    view[:3, :3] = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    d, acc, rn, dn, dist = R.maps(am, rays, view, 0.25)
    assert (d[..., 0] - (depth[0] + 0.25)).abs().max() < 1e-15 and torch.equal(acc, am[1]) and torch.equal(dist, am[6])
    assert (dn[1:-1, 1:-1] - 0.5 * n(p, q)).abs().max() < 1e-15
    assert torch.equal(rn, torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64).expand(H, W, 3))


def test_chain_length_by_hand():
    assert R.chain_length(1, 2048) == 1 + 6 + 3 + 1
    assert R.chain_length(1000, 2) == 2 + 6 + 3 + 2
    assert R.chain_length(2048 * 256, 2048) == 1 + 6 + 3 + 2048
    assert R.chain_length(2048 * 256 + 4, 2048) == 2 + 6 + 3 + 2048
    assert K.STRIDE_FWD[0] * K.STRIDE_FWD[1] == 2048 * 256 + 4 and K.STRIDE_BWD[0] * K.STRIDE_BWD[1] == 4096 * 256 + 5


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cases_are_conditioned_and_clamped(shape):
    H, W = shape
    case = K.smooth(H, W)
    for ratio in K.RATIOS:
        ok, lo, zeros = R.conditioned(case["allmap"], case["rays"], ratio)
        print(f"{H}x{W} ratio {ratio}: smallest non-zero cond {lo:.3g}, exact zeros {zeros:.2%}")
        assert ok, (shape, ratio, lo)
    below, above = K.clamp_shares(case)
    assert below >= 0.2 and above >= 0.2, (below, above)
    rays, view = case["rays"].double(), case["view"].double()
    assert (view[:3, :3] @ view[:3, :3].T - torch.eye(3, dtype=torch.float64)).abs().max() < 1e-6
    assert (rays[..., :3] != 0).all() and view[:3, :3].abs().min() > 0.05          # origin and rotation off every axis
    if H * W >= 64:
        share = float(case["empty"].double().mean())
        assert 0.05 < share < 0.2 and bool((case["allmap"][:, case["empty"]] == 0).all())
    if H * W >= 1024:     # isolated empty pixels and blocks: some stencil has both neighbours of a pair empty
        assert R.conditioned(case["allmap"], case["rays"], 0.0)[2] > 0


def test_special_case_places_what_it_says():
    case = K.special()
    am = case["allmap"]
    m = R.masks(am)
    off = {p for p, what in K.SPECIAL.items() if not what.startswith("med")}
    assert {(int(y), int(x)) for y, x in (~m.exp_ok[0]).nonzero()} == off
    assert {(int(y), int(x)) for y, x in (~m.med_ok[0]).nonzero()} == set(K.SPECIAL) - off
    assert float(m.exp_fill[0, 2, 5]) == -R.FLT_MAX and float(m.exp_fill[0, 2, 2]) == 0.0 and float(m.exp_fill[0, 7, 4]) == 0.0
    assert float(am[1, 7, 4]) != 0.0 and float(am[0, 7, 4] / am[1, 7, 4]) == math.inf           # overflows with a != 0
    assert float(m.med_fill[0, 5, 8]) == -R.FLT_MAX and float(m.med_fill[0, 5, 2]) == 0.0 and float(m.med_fill[0, 5, 5]) == 0.0
    near = K.near_special()
    assert int(near.sum()) == 4 * len(K.SPECIAL) and not any(near[y, x] for y, x in K.SPECIAL)


def test_abi_symbols_and_refusals_without_a_gpu():
    from generativedensification_amd import _lib as L

    lib = L.load()
    names = ("gdr_view_loss_forward", "gdr_view_loss_backward", "gsr_maps_forward", "gsr_maps_backward", "gsr_view_loss_forward",
             "gsr_view_loss_backward")
    for name in names:
        assert hasattr(lib, name) and name in L.EXPORTED_SYMBOLS
    assert lib.gdr_abi_version() == 17
    f = 0x10000          # never dereferenced: every refusal comes before any device work
    w = (0.0, 1000.0, 0.2, 0.1, 0.1)
    calls = {        # name -> (arguments with H, W at `hw`, positions of the pointers that must not be null)
        "gdr_view_loss_forward": (lambda h, w_: [f, f, f, f, h, w_, 0.1, 0.1, f, None], (0, 1, 2, 3, 8)),
        "gdr_view_loss_backward": (lambda h, w_: [f, f, h, w_, 0.1, 0.1, f, f, f, f, None], (0, 1, 7, 8, 9)),
        "gsr_maps_forward": (lambda h, w_: [f, f, f, h, w_, 0.3, f, f, f, f, f, None], (0, 1, 2, 6, 7, 8, 9, 10)),
        "gsr_maps_backward": (lambda h, w_: [f, f, f, h, w_, 0.3, f, f, f, f, f, f, f, None], (0, 1, 2, 11, 12)),
        "gsr_view_loss_forward": (lambda h, w_: [f, f, f, f, f, h, w_, *w, f, None], (0, 1, 2, 3, 4, 12)),
        "gsr_view_loss_backward": (lambda h, w_: [f, f, f, f, f, h, w_, *w, f, f, f, f, None], (0, 1, 2, 3, 4, 13, 14, 15)),
    }
    for name in names:
        make, pointers = calls[name]
        fn = getattr(lib, name)
        for h, w_ in ((0, 4), (4, 0), (-1, 4), (4, -3)):
            assert fn(*make(h, w_)) == GDR_ERR_INVALID_ARG and b"bad argument" in lib.gdr_last_error(), (name, h, w_)
        for i in pointers:
            a = make(4, 4)
            a[i] = None
            assert fn(*a) == GDR_ERR_INVALID_ARG, (name, i)


def test_wrapper_argument_check_refuses_before_any_launch():
    from generativedensification_amd import _marshal as M
    from generativedensification_amd import losses

    ok = torch.zeros(3, 4, 5)
    assert M.f32_contiguous("target", ok.permute(0, 2, 1), (3, 5, 4)).is_contiguous()
    assert M.f32_contiguous("target", ok, (3, None, None)) is ok
    for bad in (ok.double(), ok.bfloat16(), ok.half(), ok.int()):
        with pytest.raises(TypeError, match="float32"):
            M.f32_contiguous("target", bad, (3, 4, 5))
    for bad in (torch.zeros(4, 5, 3), torch.zeros(1, 3, 4, 5), torch.zeros(3, 4, 6), None):
        with pytest.raises(ValueError, match="target"):
            M.f32_contiguous("target", bad, (3, 4, 5))
    with pytest.raises(ValueError, match="rays"):
        M.rays_and_view(torch.zeros(4, 5, 3), torch.eye(4), 4, 5, torch.device("cpu"))
    with pytest.raises(ValueError, match="viewmatrix"):
        M.rays_and_view(torch.zeros(4, 5, 6), torch.eye(3), 4, 5, torch.device("cpu"))
    rays, view = M.rays_and_view(torch.zeros(4, 6, 5, dtype=torch.float64).transpose(1, 2), torch.eye(4).T, 4, 5, torch.device("cpu"))
    assert rays.dtype == torch.float32 and rays.is_contiguous() and view.is_contiguous()
    with pytest.raises(RuntimeError, match="ROCm/HIP"):
        losses.view_loss_fused(ok, ok[:1], ok[:1], ok)
