"""GPU: the image-space kernels of csrc/loss.hip and csrc/maps_surfel.hip (through losses.view_loss_fused,
losses.surfel_view_loss_fused, renderer_2dgs._SurfelMaps, the C entry gsr_maps_backward and Renderer.render_views_loss) against
the f64 restatement (tests/imgloss_ref.py) on the inputs of tests/imgloss_cases.py.  Bars, max norm per tensor, with err_torch32
the error of the CPU f32 torch composition against the same truth and eps = 2^-23:
    elementwise outputs   err_hip <= 2 err_torch32 + 8 eps max|truth|                      (one different rounding order)
    scalar losses         err_hip <= 2 err_torch32 + chain_length(P, 2048) eps sum_p |term_p|   (a sum in any order)
dL_dallmap is judged per channel, and a second time on the pixels away from stencils whose cross product vanishes exactly:
such a stencil hands gradients of the order 1e12 to its neighbours, which would otherwise set max|truth| of channel 5.
Every case asserts the conditioning of its inputs: each interior pixel has |a x b| == 0 exactly or cond >= 1e-2."""
import numpy as np
import pytest
import torch

import imgloss_cases as K
import imgloss_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
GO = 1.75                      # the upstream scalar of the losses, handed over as a device tensor
MAPS_SHAPES = K.SMALL_SHAPES + (K.STRIDE_FWD,)
VIEW_SHAPES = K.SMALL_SHAPES + (K.STRIDE_FWD, K.STRIDE_BWD)
ids = lambda s: f"{s[0]}x{s[1]}"


def check(tag, got, truth, t32, k=8):
    assert got.shape == truth.shape and got.dtype == torch.float32, tag
    got = got.cpu()
    assert torch.isfinite(got).all(), tag
    err_hip, err_t32 = R.max_err(got, truth), R.max_err(t32, truth)
    b = R.bar(err_t32, truth, k) if truth.numel() else 0.0
    print(f"{tag}: err_hip {err_hip:.3e} err_torch32 {err_t32:.3e} bar {b:.3e}")
    assert err_hip <= b, (tag, err_hip, err_t32, b)


def check_allmap_grad(tag, got, truth, t32, case, ratio):
    got = got.cpu()
    away = R.away_from_clamped(case["allmap"], case["rays"], ratio)
    for c in range(7):
        check(f"{tag} dL_dallmap[{c}]", got[c], truth[c], t32[c])
        if not bool(away.all()):
            check(f"{tag} dL_dallmap[{c}] away from clamped stencils", got[c][away], truth[c][away], t32[c][away])


def check_scalar(tag, got, truth, t32, chain, terms):
    err_hip, err_t32 = abs(float(got) - float(truth)), abs(float(t32) - float(truth))
    b = R.scalar_bar(err_t32, chain, terms)
    print(f"{tag}: err_hip {err_hip:.3e} err_torch32 {err_t32:.3e} bar {b:.3e}")
    assert np.isfinite(float(got)) and err_hip <= b, (tag, err_hip, err_t32, b)


def assert_conditioned(case, ratio):
    ok, lo, zeros = R.conditioned(case["allmap"], case["rays"], ratio)
    assert ok, (lo, zeros)


def dev(case, *names):
    return [case[k].to(DEV) for k in names]


def hip_maps(case, ratio, ups=None, transform=None):
    """-> the five maps (detached, on the device) and dL_dallmap"""
    from generativedensification_amd.renderer_2dgs import _SurfelMaps

    am, rays, view = dev(case, "allmap", "rays", "view")
    if transform:
        am, rays, view = transform(am, rays, view)
    am = am.detach().requires_grad_(ups is not None)
    out = _SurfelMaps.apply(am, rays, view, ratio)
    if ups is not None:
        torch.autograd.backward(out, [u.to(DEV) for u in ups])
    return dict(zip(R.MAP_NAMES, (o.detach() for o in out)), dL_dallmap=am.grad)


def hip_surfel_loss(case, ratio, go=GO, transform=None, **w):
    from generativedensification_amd.losses import surfel_view_loss_fused

    t = dict(zip(("color", "allmap", "rays", "view", "target"), dev(case, "color", "allmap", "rays", "view", "target")))
    if transform:
        t = transform(t)
    color, am = t["color"].detach().requires_grad_(True), t["allmap"].detach().requires_grad_(True)
    loss = surfel_view_loss_fused(color, am, t["rays"], t["view"], t["target"], ratio, **w)
    (loss * torch.tensor(go, device=DEV)).backward()
    return dict(loss=loss.detach(), dL_dcolor=color.grad, dL_dallmap=am.grad)


def hip_view_loss(case, go=GO, transform=None):
    from generativedensification_amd.losses import view_loss_fused

    t = dict(zip(("color", "depth", "alpha", "target"), dev(case, "color", "depth", "alpha", "target")))
    if transform:
        t = transform(t)
    leaves = [t[k].detach().requires_grad_(True) for k in ("color", "depth", "alpha")]
    loss = view_loss_fused(*leaves, t["target"])
    (loss * torch.tensor(go, device=DEV)).backward()
    return dict(loss=loss.detach(), dL_dcolor=leaves[0].grad, dL_ddepth=leaves[1].grad, dL_dalpha=leaves[2].grad)


# ---- 1-3: the bars ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", K.RATIOS)
@pytest.mark.parametrize("shape", MAPS_SHAPES, ids=ids)
def test_surfel_maps_forward_and_backward(shape, ratio):
    H, W = shape
    case, ups, truth, t32 = R.maps_case(H, W, ratio)
    assert_conditioned(case, ratio)
    got = hip_maps(case, ratio, ups)
    tag = f"maps {H}x{W} r={ratio}"
    for name in R.MAP_NAMES:
        check(f"{tag} {name}", got[name], truth[name], t32[name])
    check_allmap_grad(tag, got["dL_dallmap"], truth["dL_dallmap"], t32["dL_dallmap"], case, ratio)


@pytest.mark.parametrize("w_dist", [1000.0, 0.0])
@pytest.mark.parametrize("ratio", K.RATIOS)
@pytest.mark.parametrize("shape", MAPS_SHAPES, ids=ids)
def test_surfel_view_loss_value_and_gradients(shape, ratio, w_dist):
    """dL_dallmap[2:5] is a rotation of depth_normal whose three terms can cancel: at 3x3, ratio 0.3, channel 2 has a single
    non-zero pixel, -4.22e-04 = 4.51e-03 - 5.80e-03 + 8.62e-04.  The bar measures against the cancelled sum, so it needs a
    depth_normal better than an ulp per component (surfel_loss_bwd_a forms it in double)."""
    H, W = shape
    case, truth, t32 = R.surfel_loss_case(H, W, ratio, w_dist, GO)
    assert_conditioned(case, ratio)
    got = hip_surfel_loss(case, ratio, w_dist=w_dist)
    tag = f"surfel_loss {H}x{W} r={ratio} w_dist={w_dist:g}"
    check_scalar(f"{tag} loss", got["loss"], truth["loss"], t32["loss"], R.chain_length(H * W, 2048), truth["terms"])
    check(f"{tag} dL_dcolor", got["dL_dcolor"], truth["dL_dcolor"], t32["dL_dcolor"])
    check_allmap_grad(tag, got["dL_dallmap"], truth["dL_dallmap"], t32["dL_dallmap"], case, ratio)


@pytest.mark.parametrize("shape", VIEW_SHAPES, ids=ids)
def test_view_loss_value_and_gradients(shape):
    H, W = shape
    case, truth, t32 = R.view_loss_case(H, W, GO)
    got = hip_view_loss(case)
    tag = f"view_loss {H}x{W}"
    check_scalar(f"{tag} loss", got["loss"], truth["loss"], t32["loss"], R.chain_length(H * W, 2048), truth["terms"])
    for name in ("dL_dcolor", "dL_ddepth", "dL_dalpha"):
        check(f"{tag} {name}", got[name], truth[name], t32[name])


# ---- 4: exact structure ----------------------------------------------------------------------------------------------------
def _f(x):
    return torch.tensor(x, dtype=torch.float32)


def _no_interior_neighbour(H, W):
    """(H, W) bool: pixels that are no interior pixel's neighbour: the four corners, or every pixel without an interior"""
    m = torch.ones(H, W, dtype=torch.bool)
    if H >= 3 and W >= 3:
        m[1:-1, :] = False
        m[:, 1:-1] = False
    return m


@pytest.mark.parametrize("shape", K.SMALL_SHAPES, ids=ids)
def test_exact_structure_of_the_maps_and_their_gradient(shape):
    H, W = shape
    free = _no_interior_neighbour(H, W)
    for ratio in K.RATIOS:
        case, ups = K.smooth(H, W), K.upstreams(H, W)
        got = {k: v.cpu() for k, v in hip_maps(case, ratio, ups).items()}
        dn, g, a = got["depth_normal"], got["dL_dallmap"], case["allmap"][1]
        border = torch.ones(H, W, dtype=torch.bool)
        border[1:-1, 1:-1] = False
        assert torch.equal(dn[border], torch.zeros(int(border.sum()), 3))
        if H < 3 or W < 3:
            assert torch.equal(dn, torch.zeros(H, W, 3))
        # where no stencil reaches, the gradient of the surface depth is the depth upstream alone, in the kernel's own f32 steps
        gsd = ups[0][..., 0]
        filled = free & ~case["empty"]
        assert torch.equal(g[5][free], (_f(ratio) * gsd)[free])
        assert torch.equal(g[0][filled], (((_f(1.0) - _f(ratio)) * gsd) / a)[filled])
        assert torch.equal(g[0][case["empty"]], torch.zeros(int(case["empty"].sum())))
        assert torch.equal(g[1][case["empty"]], ups[1][case["empty"]])           # the pure acc_map upstream
        if ratio == 0.0:
            assert torch.equal(g[5], torch.zeros(H, W))
        if ratio == 1.0:
            assert torch.equal(g[0], torch.zeros(H, W))
        assert torch.equal(g[6], ups[4])


@pytest.mark.parametrize("shape", K.SMALL_SHAPES, ids=ids)
def test_exact_structure_of_the_surfel_loss_gradient(shape):
    H, W = shape
    free = _no_interior_neighbour(H, W)
    case = K.smooth(H, W)
    a = case["allmap"][1]
    for ratio in K.RATIOS:
        g = hip_surfel_loss(case, ratio)["dL_dallmap"].cpu()
        # the depth-mean term in the kernel's own f32 steps: go / P, times w_depth, times r or (1 - r) / alpha
        gsd = _f(0.1) * (_f(GO) / _f(float(H * W)))
        filled = free & ~case["empty"]
        assert torch.equal(g[5][free], (_f(ratio) * gsd).expand(H, W)[free])
        assert torch.equal(g[0][filled], (((_f(1.0) - _f(ratio)) * gsd) / a)[filled])
        assert torch.equal(g[0][case["empty"]], torch.zeros(int(case["empty"].sum())))
        if ratio == 0.0:
            assert torch.equal(g[5], torch.zeros(H, W))
        if ratio == 1.0:
            assert torch.equal(g[0], torch.zeros(H, W))


@pytest.mark.parametrize("which", ["view", "surfel"])
def test_colour_gradient_is_zero_outside_the_clamp_and_alive_on_its_ends(which):
    H, W = 17, 31
    case = dict(K.smooth(H, W))
    color, target = case["color"].clone(), case["target"].clone()
    ends = ((0, 3, 4, 0.0), (1, 5, 6, 1.0), (2, 16, 30, 0.0), (0, 0, 0, 1.0))       # texels placed by hand
    for c, y, x, v in ends:
        color[c, y, x], target[c, y, x] = v, 0.25
    case.update(color=color, target=target)
    got = hip_view_loss(case) if which == "view" else hip_surfel_loss(case, 0.3)
    g = got["dL_dcolor"].cpu()
    outside = (color < 0) | (color > 1)
    assert 0.4 < float(outside.double().mean()) < 0.5
    assert torch.equal(g[outside], torch.zeros(int(outside.sum()))) and bool((g[~outside] != 0).all())
    for c, y, x, v in ends:
        want = GO * 2.0 * (v - 0.25) / (3 * H * W)
        assert abs(float(g[c, y, x]) - want) <= 4 * R.EPS * abs(want), (c, y, x)


# ---- 5: one-hot pixels -----------------------------------------------------------------------------------------------------
def _two_ulp(got, want):
    return abs(float(got) - want) <= 2 * float(np.spacing(np.float32(want)))


def test_one_hot_pixels_reach_the_forward_reductions_once():
    """adding zeros is exact in any order: the loss is the one non-zero term, wherever in the stride its pixel sits"""
    from generativedensification_amd.losses import surfel_view_loss_fused, view_loss_fused

    H, W = K.STRIDE_FWD
    P = H * W
    assert R.chain_length(P, 2048) == R.chain_length(P - 4, 2048) + 1          # the first striding size
    rays, view = dev(K.smooth(H, W), "rays", "view")
    z3, z1, am = torch.zeros(3, H, W, device=DEV), torch.zeros(1, H, W, device=DEV), torch.zeros(7, H, W, device=DEV)
    depth = torch.zeros(1, H, W, device=DEV)
    v = float(np.float32(0.37))
    for q in (0, 255, 256, 2 ** 19 - 1, 2 ** 19, P - 1):
        am.view(7, P)[6, q] = v
        depth.view(P)[q] = v
        ls = surfel_view_loss_fused(z3, am, rays, view, z3, 0.3)
        lv = view_loss_fused(z3, depth, z1, z3)
        am.view(7, P)[6, q] = 0.0
        depth.view(P)[q] = 0.0
        print(f"one-hot q={q}: surfel {float(ls):.9e} want {1000.0 * v / P:.9e}; view {float(lv):.9e} want {0.1 * v / P:.9e}")
        assert _two_ulp(ls, 1000.0 * v / P), q
        assert _two_ulp(lv, float(np.float32(0.1)) * v / P), q
    assert float(surfel_view_loss_fused(z3, am, rays, view, z3, 0.3)) == 0.0 and float(view_loss_fused(z3, depth, z1, z3)) == 0.0


# ---- 6: special values -----------------------------------------------------------------------------------------------------
def _special_sets():
    """-> case, exp_off, med_off, sp, near, near2: (H, W) bool masks of the pixels whose expected / median depth is masked, of
    the special pixels, of their four neighbours, and of everything a gradient can carry their values to"""
    H, W = K.SPECIAL_SHAPE
    case = K.special()
    mask = R.masks(case["allmap"])
    sp = torch.zeros(H, W, dtype=torch.bool)
    for y, x in K.SPECIAL:
        sp[y, x] = True
    # a gradient travels through two stencils: a pixel's own and, transposed, its neighbours'
    near2 = torch.zeros(H, W, dtype=torch.bool)
    for y, x in K.SPECIAL:
        for dy in range(-2, 3):
            for dx in range(-2 + abs(dy), 3 - abs(dy)):
                if 0 <= y + dy < H and 0 <= x + dx < W:
                    near2[y + dy, x + dx] = True
    assert int((~near2).sum()) > 0
    return case, ~mask.exp_ok[0], ~mask.med_ok[0], sp, K.near_special(), near2


def _same_finite_pattern(tag, g, plain_g, exp_off, med_off):
    """finite where torch's f32 gradient is finite, and non-finite nowhere but where torch's is; left aside: torch's 0/0 at the
    masked pixels of channels 0 and 1, which the kernels answer with their documented finite values, and 0 times a NaN
    upstream at a masked median depth, where the kernels write an exact 0 (both asserted by the caller)"""
    fin_t = torch.isfinite(plain_g)
    fin_t[0:2, exp_off] = True
    fin_t[5, med_off] = True
    differ = (torch.isfinite(g) != fin_t).nonzero().tolist()
    print(f"{tag}: non-finite gradient entries hip {int((~torch.isfinite(g)).sum())} torch32 {int((~fin_t).sum())}")
    assert not differ, (tag, differ)


def test_special_values():
    H, W = K.SPECIAL_SHAPE
    ups = K.upstreams(H, W)
    case, exp_off, med_off, sp, near, near2 = _special_sets()
    for ratio in K.RATIOS:
        got = {k: v.cpu() for k, v in hip_maps(case, ratio, ups).items()}
        plain = R.run_maps(case, ratio, torch.float32, ups, mask=False)          # torch's own composition, NaN gradients and all
        tag = f"special r={ratio}"
        assert torch.equal(got["depth"][sp], plain["depth"][sp]), tag
        if ratio == 0.0:
            assert float(got["depth"][2, 5]) == -R.FLT_MAX and float(got["depth"][7, 4]) == 0.0
            assert float(got["depth"][2, 2]) == 0.0 and float(got["depth"][2, 8]) == 0.0
        if ratio == 1.0:
            assert float(got["depth"][5, 8]) == -R.FLT_MAX and float(got["depth"][5, 2]) == 0.0 and float(got["depth"][5, 5]) == 0.0
        g = got["dL_dallmap"]
        assert torch.isnan(plain["dL_dallmap"][1, 7, 4])               # torch: 0 * (-D / a^2) = 0 * inf
        assert torch.equal(g[0][exp_off], torch.zeros(int(exp_off.sum()))), tag
        assert torch.equal(g[1][exp_off], ups[1][exp_off]), tag       # the depth part is 0: the pure acc_map upstream is left
        assert torch.equal(g[5][med_off], torch.zeros(int(med_off.sum()))), tag
        for name in R.MAP_NAMES:
            assert torch.isfinite(got[name][~near]).all(), (tag, name)
            assert torch.equal(torch.isfinite(got[name]), torch.isfinite(plain[name])), (tag, name)
        assert torch.isfinite(g[:, ~near2]).all(), tag
        _same_finite_pattern(tag, g, plain["dL_dallmap"], exp_off, med_off)
        # values away from everything special meet the elementwise bar against the masked truth
        truth, t32 = R.run_maps(case, ratio, torch.float64, ups), R.run_maps(case, ratio, torch.float32, ups)
        for name in R.MAP_NAMES:
            check(f"{tag} {name} away", got[name][~near & ~sp], truth[name][~near & ~sp], t32[name][~near & ~sp])
        for c in range(7):
            check(f"{tag} dL_dallmap[{c}] away", g[c][~near2], truth["dL_dallmap"][c][~near2], t32["dL_dallmap"][c][~near2])


def test_special_values_through_the_surfel_loss():
    """the loss kernels carry their own copy of the maps' arithmetic, and the backward forms depth_normal a second time in
    double where the f32 stencil is ordinary: the same special pixels, through losses.surfel_view_loss_fused"""
    H, W = K.SPECIAL_SHAPE
    case, exp_off, med_off, sp, near, near2 = _special_sets()
    for ratio in K.RATIOS:
        tag = f"special surfel_loss r={ratio}"
        got = {k: v.cpu() for k, v in hip_surfel_loss(case, ratio).items()}
        plain = R.run_surfel_loss(case, ratio, torch.float32, GO, mask=False)      # torch's own composition, NaN and all
        truth, t32 = R.run_surfel_loss(case, ratio, torch.float64, GO), R.run_surfel_loss(case, ratio, torch.float32, GO)
        # the value: what the f32 composition gives, a NaN included (a neighbour at -FLT_MAX overflows the f32 stencil)
        print(f"{tag}: loss hip {float(got['loss']):.9e} torch32 {float(plain['loss']):.9e}")
        if torch.isfinite(plain["loss"]):
            check_scalar(f"{tag} loss", got["loss"], truth["loss"], t32["loss"], R.chain_length(H * W, 2048), truth["terms"])
        else:
            assert torch.isnan(plain["loss"]) and torch.isnan(got["loss"]), tag
        check(f"{tag} dL_dcolor", got["dL_dcolor"], truth["dL_dcolor"], t32["dL_dcolor"])
        g = got["dL_dallmap"]
        # mask-off pixels: no gradient through the quotient or the median, in the kernel's own f32 steps
        invp = _f(GO) / _f(float(H * W))
        assert torch.equal(g[0][exp_off], torch.zeros(int(exp_off.sum()))), tag
        assert torch.equal(g[1][exp_off], (_f(0.1) * invp).expand(int(exp_off.sum()))), tag
        assert torch.equal(g[5][med_off], torch.zeros(int(med_off.sum()))), tag
        assert torch.isfinite(g[:, ~near2]).all(), tag
        _same_finite_pattern(tag, g, plain["dL_dallmap"], exp_off, med_off)
        # where both are finite next to a special pixel, the gradient of rend_normal follows the f32 stencil's normal (0
        # where |c| overflows), as the forward value does: the f32 composition is the reference there
        both = torch.isfinite(g[2:5]) & torch.isfinite(plain["dL_dallmap"][2:5]) & near2
        scale = float(truth["dL_dallmap"][2:5].abs().max())
        err = float((g[2:5] - plain["dL_dallmap"][2:5])[both].abs().max()) if bool(both.any()) else 0.0
        print(f"{tag}: dL_dallmap[2:5] near special pixels, against torch32: err {err:.3e}, 8 eps max|truth| {8 * R.EPS * scale:.3e}")
        assert err <= 8 * R.EPS * scale, tag
        # values away from everything special meet the elementwise bar against the masked truth
        for c in range(7):
            check(f"{tag} dL_dallmap[{c}] away", g[c][~near2], truth["dL_dallmap"][c][~near2], t32["dL_dallmap"][c][~near2])


# ---- 7: absent upstreams through the C entry ---------------------------------------------------------------------------------
@pytest.mark.parametrize("present", [(0, 1, 2, 4), (3,)], ids=["no_depth_normal_no_scratch", "only_depth_normal"])
def test_absent_upstreams_through_the_c_entry(present):
    from generativedensification_amd import _lib as L
    from generativedensification_amd import _marshal as M

    H, W, ratio = 17, 31, 0.3
    case = K.smooth(H, W)
    assert_conditioned(case, ratio)
    ups = [u if i in present else None for i, u in enumerate(K.upstreams(H, W))]
    truth, t32 = R.run_maps(case, ratio, torch.float64, ups), R.run_maps(case, ratio, torch.float32, ups)
    am, rays, view = dev(case, "allmap", "rays", "view")
    d = [None if u is None else u.to(DEV) for u in ups]
    scratch = torch.empty(6, H, W, device=DEV) if d[3] is not None else None
    out = torch.full((7, H, W), float("nan"), device=DEV)
    with torch.cuda.device(out.device):
        L.check(L.load().gsr_maps_backward(am.data_ptr(), rays.data_ptr(), view.data_ptr(), H, W, ratio, *(M.ptr(x) for x in d),
                                           M.ptr(scratch), out.data_ptr(), M.stream()), "gsr_maps_backward")
    check_allmap_grad(f"gsr_maps_backward upstreams {present}", out, truth["dL_dallmap"], t32["dL_dallmap"], case, ratio)


# ---- 8: determinism --------------------------------------------------------------------------------------------------------
def test_backwards_repeat_their_bits_and_forwards_stay_within_the_bar():
    H, W, ratio = 57, 83, 0.3
    case, ups = K.smooth(H, W), K.upstreams(H, W)
    a, b = hip_maps(case, ratio, ups), hip_maps(case, ratio, ups)
    assert all(torch.equal(a[k], b[k]) for k in a)
    a, b = hip_surfel_loss(case, ratio), hip_surfel_loss(case, ratio)
    assert torch.equal(a["dL_dcolor"], b["dL_dcolor"]) and torch.equal(a["dL_dallmap"], b["dL_dallmap"])
    terms = R.surfel_loss_case(H, W, ratio, 1000.0, GO)[1]["terms"]
    check_scalar("surfel_loss twice", a["loss"], b["loss"].double(), b["loss"].double(), R.chain_length(H * W, 2048), terms)
    a, b = hip_view_loss(case), hip_view_loss(case)
    assert all(torch.equal(a[k], b[k]) for k in a if k != "loss")
    terms = R.view_loss_case(H, W, GO)[1]["terms"]
    check_scalar("view_loss twice", a["loss"], b["loss"].double(), b["loss"].double(), R.chain_length(H * W, 2048), terms)


# ---- 9: the wrappers -------------------------------------------------------------------------------------------------------
def _wider(t, dim=-1):
    """the same values as a strided view of a wider buffer"""
    shape = list(t.shape)
    shape[dim] += 3
    buf = torch.full(shape, 7.0, device=t.device)
    view = buf.narrow(dim, 1, t.shape[dim])
    view.copy_(t)
    assert not view.is_contiguous() or t.numel() <= 1
    return view


def test_wrappers_bring_views_into_the_form_the_kernels_read():
    H, W, ratio = 16, 16, 0.3          # one workgroup: the forward sum has one order, so the losses repeat their bits too
    case = K.smooth(H, W)
    hwc = lambda t: t.permute(1, 2, 0).contiguous().permute(2, 0, 1)          # CHW values as a view of an HWC tensor
    base = hip_view_loss(case)
    for name, tr in (("target", lambda t: {**t, "target": hwc(t["target"])}),
                     ("depth alpha", lambda t: {**t, "depth": _wider(t["depth"]), "alpha": _wider(t["alpha"])}),
                     ("color", lambda t: {**t, "color": hwc(t["color"])})):
        got = hip_view_loss(case, transform=tr)
        assert all(torch.equal(got[k], base[k]) for k in base), name
    base = hip_surfel_loss(case, ratio)
    for name, tr in (("target", lambda t: {**t, "target": hwc(t["target"])}),
                     ("rays", lambda t: {**t, "rays": _wider(t["rays"]), "view": t["view"].T.contiguous().T}),
                     ("allmap color", lambda t: {**t, "allmap": _wider(t["allmap"]), "color": _wider(t["color"], 1)})):
        got = hip_surfel_loss(case, ratio, transform=tr)
        assert all(torch.equal(got[k], base[k]) for k in base), name
    ups = K.upstreams(H, W)
    base = hip_maps(case, ratio, ups)
    got = hip_maps(case, ratio, ups, transform=lambda am, rays, view: (_wider(am), _wider(rays, 1), view.double()))
    assert all(torch.equal(got[k], base[k]) for k in base)


def test_wrappers_refuse_other_dtypes_and_shapes_before_any_launch():
    from generativedensification_amd.losses import surfel_view_loss_fused, view_loss_fused
    from generativedensification_amd.renderer_2dgs import _SurfelMaps

    H, W = 5, 6
    case = K.smooth(H, W)
    v = dict(zip(("color", "depth", "alpha", "target"), dev(case, "color", "depth", "alpha", "target")))
    s = dict(zip(("color", "allmap", "rays", "view", "target"), dev(case, "color", "allmap", "rays", "view", "target")))
    call_v = lambda t: view_loss_fused(t["color"], t["depth"], t["alpha"], t["target"])
    call_s = lambda t: surfel_view_loss_fused(t["color"], t["allmap"], t["rays"], t["view"], t["target"], 0.3)
    for dtype in (torch.float64, torch.bfloat16):
        for k in ("color", "depth", "alpha", "target"):
            with pytest.raises(TypeError, match="float32"):
                call_v({**v, k: v[k].to(dtype)})
        for k in ("color", "allmap", "target"):
            with pytest.raises(TypeError, match="float32"):
                call_s({**s, k: s[k].to(dtype)})
        with pytest.raises(TypeError, match="float32"):
            _SurfelMaps.apply(s["allmap"].to(dtype), s["rays"], s["view"], 0.3)
    z = lambda *shape: torch.zeros(*shape, device=DEV)
    for k, bad in (("target", z(H, W, 3)), ("target", z(3, H, W + 1)), ("target", z(1, 3, H, W)), ("depth", z(H, W)),
                   ("alpha", z(1, H + 1, W)), ("color", z(4, H, W))):
        with pytest.raises(ValueError, match=k):
            call_v({**v, k: bad})
    for k, bad in (("target", z(H, W, 3)), ("allmap", z(6, H, W)), ("allmap", z(7, W, H)), ("allmap", z(H, W, 7)),
                   ("rays", z(H, W, 3)), ("view", z(3, 3))):
        with pytest.raises(ValueError, match=k):
            call_s({**s, k: bad})
    for bad in (z(6, H, W), z(7, H), z(H, W, 7)):
        with pytest.raises(ValueError, match="allmap|rays"):
            _SurfelMaps.apply(bad, s["rays"], s["view"], 0.3)
    with pytest.raises(RuntimeError, match="target"):
        call_v({**v, "target": case["target"]})                                  # left on the CPU


# ---- 10: the loss folded into K6 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (5, 37), (17, 300), (48, 48)], ids=ids)
def test_folded_loss_against_the_f64_loss_of_the_rendered_images(shape):
    from generativedensification_amd.camera import orbit_cameras
    from generativedensification_amd.renderer import Renderer
    from generativedensification_amd.synthetic import make_scene, make_targets

    H, W = shape
    V = 2
    sc = {k: v.to(DEV) for k, v in make_scene(300, 17, sh_degree=3, sigma0=(0.05,)).items()}
    sc["shs"][:, 0] *= 3.0          # a good share of pixels leaves [0, 1]
    cams = orbit_cameras(V, W, H, device=DEV)
    tg = make_targets(V, H, W, 17).permute(0, 3, 1, 2).contiguous()
    r = Renderer(sh_degree=3, fused=True)
    args = (sc["centers"], sc["shs"], sc["opacity"], sc["scales"], sc["rotations"], DEV)
    lv = r.render_views_loss(cams, None, tg.to(DEV), *args).detach().cpu()
    outs = r.render_views(cams, None, *args, raw=True)
    tiles = -(-H // 16) * -(-W // 16)
    for j, o in enumerate(outs):
        case = dict(color=o["color"].detach().cpu(), depth=o["depth"].detach().cpu(), alpha=o["alpha"].detach().cpu(), target=tg[j])
        assert case["color"].shape == (3, H, W) and (H * W < 100 or float(case["alpha"].max()) > 0.05)
        truth, t32 = R.run_view_loss(case, torch.float64), R.run_view_loss(case, torch.float32)
        check_scalar(f"folded loss {H}x{W} view {j}", lv[j], truth["loss"], t32["loss"], 8 + 3 + tiles, truth["terms"])
