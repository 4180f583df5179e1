"""GPU: the HIP projected bilinear sampling (csrc/pointfeat.hip through generativedensification_amd.pointfeat) against the f64
restatement (tests/pointfeat_ref.py).  Bars, max-norm per tensor, with err_torch32 the error of the CPU f32 torch
composition against the same truth and eps = 2^-23:
    forward and point gradient   err_hip <= 2 err_torch32 + 8 eps max|truth|     (one different rounding order)
    image gradients              err_hip <= 2 err_torch32 + k_max eps max|truth| (atomic sums of up to k_max terms per texel)
Points whose position in any view lies within 1e-3 px of an integer, where the point gradient jumps, leave the point-gradient
comparison only; every such test asserts that they are at most 3 %."""
import os

import pytest
import torch

import pointfeat_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
H, W = 45, 61
MAIN = (4096, 4, H, W)
BORDER_FOV = (30.0, 24.0)
IMAGE_GRADS = ("g_img_ref", "g_image", "g_acc_map", "g_depth")


def P():
    from generativedensification_amd import pointfeat
    return pointfeat


def hip_point_feats(inp, need=(True,) * 5, transform=None):
    """-> dict(out, g_*) on the CPU; need: which of img_ref, image, acc_map, depth, points require grad"""
    t = {k: inp[k].to(DEV) for k in R.FEAT_LEAVES + ("w2cs", "ixts")}
    if transform:
        t = transform(t)
    for k, n in zip(R.FEAT_LEAVES, need):
        t[k] = t[k].detach().requires_grad_(n)
    out = P().point_feats(*(t[k] for k in R.FEAT_LEAVES), t["w2cs"], t["ixts"])
    res = dict(out=out.detach().cpu())
    if any(need):
        out.backward(inp["gout"].to(DEV))
    for k in R.FEAT_LEAVES:
        res["g_" + k] = None if t[k].grad is None else t[k].grad.cpu()
    return res


def hip_sample_views(inp, need=(True, True), transform=None):
    t = {k: inp[k].to(DEV) for k in R.VIEWS_LEAVES + ("w2cs", "ixts")}
    if transform:
        t = transform(t)
    for k, n in zip(R.VIEWS_LEAVES, need):
        t[k] = t[k].detach().requires_grad_(n)
    out, z = P().sample_views(t["images"], t["points"], t["w2cs"], t["ixts"])
    res = dict(out=out.detach().cpu(), z=z.detach().cpu())
    if any(need):
        torch.autograd.backward((out, z), (inp["gfeat"].to(DEV), inp["gz"].to(DEV)))
    for k in R.VIEWS_LEAVES:
        res["g_" + k] = None if t[k].grad is None else t[k].grad.cpu()
    return res


def check(tag, got, truth, t32, inp, Hh, Ww, names=None, near_px=R.NEAR_INTEGER, pair_mask=None):
    """every tensor of `got` named in `names` (default: all that truth has) against the bars of the module docstring"""
    k_max = R.tap_stats(inp, Hh, Ww, pair_mask)[0]
    keep = R.keep_for_point_grad(inp, near_px, pair_mask)
    dropped = 1.0 - float(keep.double().mean()) if keep.numel() else 0.0
    print(f"{tag}: k_max {k_max}, {dropped:.2%} of the points leave the point-gradient comparison")
    assert dropped <= R.MAX_EXCLUDED
    for name in names or truth:
        a, T, S = got[name], truth[name], t32[name]
        assert a is not None and a.shape == T.shape and a.dtype == torch.float32, name
        assert torch.isfinite(a).all(), name
        if name == "g_points":
            a, T, S = a[keep], T[keep], S[keep]
        err_hip, err_t32 = R.max_err(a, T), R.max_err(S, T)
        b = R.bar(err_t32, T, k_max if name in IMAGE_GRADS + ("g_images",) else 8) if T.numel() else 0.0
        print(f"{tag} {name}: err_hip {err_hip:.3e} err_torch32 {err_t32:.3e} bar {b:.3e}")
        assert err_hip <= b, (tag, name, err_hip, err_t32, b)


# ---- main case -------------------------------------------------------------------------------------------------------------
def test_point_feats_main_case():
    inp, truth, t32 = R.feats_case(*MAIN)
    assert R.tap_stats(inp, H, W)[2] > 0.95          # nearly every pair lands inside
    check("point_feats main", hip_point_feats(inp), truth, t32, inp, H, W)


@pytest.mark.parametrize("C", [1, 3, 70])
def test_sample_views_main_case(C):
    inp, truth, t32 = R.views_case(*MAIN, C)
    check(f"sample_views C={C}", hip_sample_views(inp), truth, t32, inp, H, W)


# ---- exact case ------------------------------------------------------------------------------------------------------------
EXACT_H, EXACT_W = 5, 7


def _exact_inputs():
    xs = (-1.0, -0.5, 0.0, 0.25, EXACT_W - 1.0, EXACT_W - 0.5, float(EXACT_W))
    ys = (-1.0, -0.5, 0.0, 0.25, EXACT_H - 1.0, EXACT_H - 0.5, float(EXACT_H))
    pts = torch.tensor([[x, y, 1.0] for y in ys for x in xs])
    return pts, torch.eye(4)[None], torch.eye(3)[None]


def _exact_image_gradient(pts):
    """(EXACT_H, EXACT_W) f64: per texel the sum of the weights of the positions that touch it, which is the image gradient
    of a plain sum of the samples; exactly zero on every texel no position touches.  All weights are multiples of 1/16, so
    the sums are exact in f32 in any order."""
    touched = torch.zeros(EXACT_H + 4, EXACT_W + 4, dtype=torch.float64)        # a two-texel frame takes the outside taps
    for p in pts:
        x, y = float(p[0]), float(p[1])
        x0, y0 = int(x // 1), int(y // 1)
        for j, wy in ((y0, y0 + 1 - y), (y0 + 1, y - y0)):
            for i, wx in ((x0, x0 + 1 - x), (x0 + 1, x - x0)):
                touched[j + 2, i + 2] += wx * wy
    want_g = touched[2:-2, 2:-2]
    assert 0 < int((want_g != 0).sum()) < EXACT_H * EXACT_W        # some texels are touched by nobody
    return want_g


def test_exact_positions_sample_views():
    """w2c = I, K = I, points (x, y, 1): the position is (x, y) exactly; texels are distinct integers, so every weight
    product and sum is exact in f32"""
    pts, w2c, ixt = _exact_inputs()
    C = 3
    images = (torch.arange(C * EXACT_H * EXACT_W, dtype=torch.float32) + 1).view(1, C, EXACT_H, EXACT_W)
    dimg = images.to(DEV).requires_grad_(True)
    out, z = P().sample_views(dimg, pts.to(DEV), w2c.to(DEV), ixt.to(DEV))
    want = torch.stack([R.hand_bilinear(images[0], float(p[0]), float(p[1])) for p in pts], dim=1)
    assert torch.equal(out[0].cpu().double(), want) and torch.equal(z.cpu(), torch.ones(1, pts.shape[0]))
    # the image gradient of out.sum(): the same expected map in every channel
    out.sum().backward()
    want_g = _exact_image_gradient(pts)
    g = dimg.grad[0].cpu().double()
    for c in range(C):
        assert torch.equal(g[c], want_g), c


def test_exact_positions_point_feats():
    pts, w2c, ixt = _exact_inputs()
    base = (torch.arange(8 * EXACT_H * EXACT_W, dtype=torch.float32) + 1).view(1, 8, EXACT_H, EXACT_W)
    src = dict(img_ref=base[:, :3], image=base[:, 3:6].permute(0, 2, 3, 1), acc_map=base[:, 6], depth=base[:, 7:8].permute(0, 2, 3, 1))
    d = {k: v.to(DEV).requires_grad_(k != "img_ref") for k, v in src.items()}
    out = P().point_feats(d["img_ref"], d["image"], d["acc_map"], d["depth"], pts.to(DEV), w2c.to(DEV), ixt.to(DEV))
    want = torch.stack([R.hand_bilinear(base[0], float(p[0]), float(p[1])) for p in pts])        # (P, 8)
    want[:, 7] = (want[:, 7] - 1.0).abs()
    assert torch.equal(out[:, 0].cpu().double(), want)
    # the image gradients of out.sum(), scattered into (V, H, W, 3), (V, H, W) and (V, H, W, 1): the full expected map on
    # every render channel, exactly, zeros on the untouched texels included.  Every depth sample that reaches a texel with a
    # non-zero weight is above z = 1 (the depth texels start at 7 * 35 + 1 and the smallest weight is 1/4), so the |.|
    # channel passes the same map on with sign +1.  img_ref does not want a gradient and gets none.
    out.sum().backward()
    want_g = _exact_image_gradient(pts)
    assert float(want_g[0, 0]) == (0.5 + 1.0 + 0.75) ** 2 and float(want_g[2, 3]) == 0.0       # two texels by hand
    g_img, g_acc, g_depth = (d[k].grad.cpu().double() for k in ("image", "acc_map", "depth"))
    assert g_img.shape == (1, EXACT_H, EXACT_W, 3) and g_acc.shape == (1, EXACT_H, EXACT_W) and g_depth.shape == (1, EXACT_H, EXACT_W, 1)
    for c in range(3):
        assert torch.equal(g_img[0, ..., c], want_g), c
    assert torch.equal(g_acc[0], want_g) and torch.equal(g_depth[0, ..., 0], want_g)
    assert d["img_ref"].grad is None


# ---- border share ----------------------------------------------------------------------------------------------------------
def test_border_share_point_feats():
    inp, truth, t32 = R.feats_case(*MAIN, 1, BORDER_FOV)
    share = R.tap_stats(inp, H, W)[1]
    print(f"pairs with a neighbour outside the image: {share:.1%}")
    assert 0.15 <= share <= 0.40
    check("point_feats border", hip_point_feats(inp), truth, t32, inp, H, W)


def test_border_share_sample_views():
    inp, truth, t32 = R.views_case(*MAIN, 3, 1, BORDER_FOV)
    assert 0.15 <= R.tap_stats(inp, H, W)[1] <= 0.40
    check("sample_views border", hip_sample_views(inp), truth, t32, inp, H, W)


# ---- launch boundaries -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 257])
def test_launch_boundaries(N):
    inp, truth, t32 = R.feats_case(N, 3, 13, 17, 2)
    got = hip_point_feats(inp)
    assert got["out"].shape == (N, 3, 8) and got["g_points"].shape == (N, 3)
    check(f"point_feats N={N}", got, truth, t32, inp, 13, 17)
    inp, truth, t32 = R.views_case(N, 3, 13, 17, 5, 2)
    got = hip_sample_views(inp)
    assert got["out"].shape == (3, 5, N) and got["z"].shape == (3, N)
    check(f"sample_views N={N}", got, truth, t32, inp, 13, 17)


def test_one_texel_image_one_view():
    """positions spread about a texel around (0, 0): each of the four neighbours is the one texel for some points"""
    fov, principal = (28.0, 24.0), (-0.37, -0.61)
    inp, truth, t32 = R.feats_case(65, 1, 1, 1, 3, fov, principal)
    x, y = R.positions(inp)
    assert {(int(a), int(b)) for a, b in zip(torch.floor(x[0]).tolist(), torch.floor(y[0]).tolist())} >= {(-1, -1), (0, -1), (-1, 0), (0, 0)}
    check("point_feats 1x1", hip_point_feats(inp), truth, t32, inp, 1, 1)
    inp, truth, t32 = R.views_case(65, 1, 1, 1, 2, 3, fov, principal)
    check("sample_views 1x1", hip_sample_views(inp), truth, t32, inp, 1, 1)


def test_sixteen_views():
    """(a point has 16 chances to lie near an integer position: the excluded band is narrowed to 2e-4 px, still far above
    the f32 position error of ~1e-5 px, to keep the share under 3 %)"""
    inp, truth, t32 = R.feats_case(257, 16, 13, 17, 4)
    check("point_feats V=16", hip_point_feats(inp), truth, t32, inp, 13, 17, near_px=2e-4)
    inp, truth, t32 = R.views_case(257, 16, 13, 17, 2, 4)
    check("sample_views V=16", hip_sample_views(inp), truth, t32, inp, 13, 17, near_px=2e-4)


# ---- z cases ---------------------------------------------------------------------------------------------------------------
def test_point_behind_a_camera_equals_the_truth():
    """z < 0 is not degenerate: the point projects mirrored, as the arithmetic says"""
    inp = dict(R.make_inputs(257, 3, 13, 17, 2, seed=5))
    eye = -inp["w2cs"][1, :3, :3].T @ inp["w2cs"][1, :3, 3]
    inp["points"] = inp["points"].clone()
    inp["points"][7] = eye * 1.3 + torch.tensor([0.02, -0.03, 0.01])          # behind view 1, near its axis
    assert float(R.project(inp["points"].double(), inp["w2cs"].double(), inp["ixts"].double())[1][1, 7]) < 0
    check("point_feats behind", hip_point_feats(inp), R.run_point_feats(inp, torch.float64), R.run_point_feats(inp, torch.float32),
          inp, 13, 17)
    check("sample_views behind", hip_sample_views(inp), R.run_sample_views(inp, torch.float64),
          R.run_sample_views(inp, torch.float32), inp, 13, 17)


def test_h2_zero_in_one_view_only():
    """view 2 is an axis-aligned camera at z = -0.25 and point 5 lies in its plane z_cam = 0: h2 == 0 exactly, in f32 and
    f64.  That pair samples zeros and sends no gradient through x and y; the other views contribute as the truth says."""
    inp = dict(R.make_inputs(257, 3, 13, 17, 2, seed=6))
    inp["w2cs"] = inp["w2cs"].clone()
    inp["w2cs"][2] = torch.eye(4)
    inp["w2cs"][2, 2, 3] = 0.25
    inp["points"] = inp["points"].clone()
    inp["points"][5] = torch.tensor([0.125, 0.25, -0.25])
    z = R.project(inp["points"], inp["w2cs"], inp["ixts"])[1]
    assert float(z[2, 5]) == 0.0 and int((z == 0).sum()) == 1
    mask = z != 0
    with torch.autograd.set_detect_anomaly(True):
        feats, views = hip_point_feats(inp), hip_sample_views(inp)
    assert torch.equal(feats["out"][5, 2], torch.zeros(8)) and torch.equal(views["out"][2, :, 5], torch.zeros(2))
    assert float(views["z"][2, 5]) == 0.0
    # the restatement takes the degenerate pair out by a mask, and so do k_max and the exclusion list; the bars then hold
    # for every tensor, point 5 included
    assert bool(R.keep_for_point_grad(inp, pair_mask=mask)[5])        # point 5 stays in the point-gradient comparison
    for got in (feats, views):
        for name, a in got.items():
            assert torch.isfinite(a).all(), name
    check("point_feats h2=0", feats, R.run_point_feats(inp, torch.float64, mask), R.run_point_feats(inp, torch.float32, mask),
          inp, 13, 17, pair_mask=mask)
    check("sample_views h2=0", views, R.run_sample_views(inp, torch.float64, mask), R.run_sample_views(inp, torch.float32, mask),
          inp, 13, 17, pair_mask=mask)


# ---- layouts ---------------------------------------------------------------------------------------------------------------
def test_layouts_are_read_in_place_bit_for_bit():
    """sources as permuted views of CHW tensors (what the rasterizer returns), images channel-last behind a permute, points a
    strided slice of a wider buffer: same bits as from contiguous copies, forward and point gradient"""
    inp, _, _ = R.feats_case(257, 3, 13, 17, 2)

    def as_views(t):
        t = dict(t)
        t["image"] = t["image"].permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)          # (V, 3, H, W) storage
        t["depth"] = t["depth"].permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
        t["acc_map"] = torch.stack((t["acc_map"], t["acc_map"] + 1), dim=1)[:, 0]             # a (V, 1, H, W) slice, squeezed
        wide = torch.zeros(t["points"].shape[0], 2, 5, device=DEV)
        wide[:, 1, 1:4] = t["points"]
        t["points"] = wide[:, 1, 1:4]
        assert not any(t[k].is_contiguous() for k in ("image", "acc_map", "points"))
        return t

    a, b = hip_point_feats(inp), hip_point_feats(inp, transform=as_views)
    assert torch.equal(a["out"], b["out"]) and torch.equal(a["g_points"], b["g_points"])
    for k in IMAGE_GRADS:
        assert a[k].shape == b[k].shape and torch.allclose(a[k], b[k], rtol=1e-4, atol=1e-5), k

    inp, _, _ = R.views_case(257, 3, 13, 17, 5, 2)

    def channel_last(t):
        t = dict(t)
        t["images"] = t["images"].permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        t["points"] = t["points"].repeat(1, 2)[:, 1:4]             # columns y, z, x of a six-column buffer
        assert not t["images"].is_contiguous() and not t["points"].is_contiguous()
        return t

    def rolled(t):      # the contiguous copy of the same (rolled) points
        t = dict(t)
        t["points"] = t["points"].repeat(1, 2)[:, 1:4].contiguous()
        return t

    a, b = hip_sample_views(inp, transform=rolled), hip_sample_views(inp, transform=channel_last)
    assert torch.equal(a["out"], b["out"]) and torch.equal(a["z"], b["z"]) and torch.equal(a["g_points"], b["g_points"])
    assert torch.allclose(a["g_images"], b["g_images"], rtol=1e-4, atol=1e-5)


# ---- which gradients -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("need", [(True, True, True, True, False), (False, False, False, False, True), (False,) * 5,
                                  (False, True, True, True, True)], ids=["images", "points", "none", "no_img_ref"])
def test_which_gradients_point_feats(need):
    inp, truth, t32 = R.feats_case(257, 3, 13, 17, 2)
    got = hip_point_feats(inp, need)
    wanted = ["out"] + ["g_" + k for k, n in zip(R.FEAT_LEAVES, need) if n]
    for k, n in zip(R.FEAT_LEAVES, need):
        assert (got["g_" + k] is not None) == n, k
    check(f"point_feats need={need}", got, truth, t32, inp, 13, 17, wanted)


@pytest.mark.parametrize("need", [(True, False), (False, True), (False, False)], ids=["images", "points", "none"])
def test_which_gradients_sample_views(need):
    inp, truth, t32 = R.views_case(257, 3, 13, 17, 70, 2)
    got = hip_sample_views(inp, need)
    for k, n in zip(R.VIEWS_LEAVES, need):
        assert (got["g_" + k] is not None) == n, k
    check(f"sample_views need={need}", got, truth, t32, inp, 13, 17,
          ["out", "z"] + ["g_" + k for k, n in zip(R.VIEWS_LEAVES, need) if n])


# ---- reproducibility, no_grad, vjp, autocast ---------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits():
    inp, _, _ = R.feats_case(*MAIN)
    a, b = hip_point_feats(inp), hip_point_feats(inp)
    assert torch.equal(a["out"], b["out"]) and torch.equal(a["g_points"], b["g_points"])
    inp, _, _ = R.views_case(*MAIN, 3)
    a, b = hip_sample_views(inp), hip_sample_views(inp)
    assert torch.equal(a["out"], b["out"]) and torch.equal(a["z"], b["z"]) and torch.equal(a["g_points"], b["g_points"])


def test_no_grad_vjp_and_autocast():
    inp, truth, t32 = R.feats_case(257, 3, 13, 17, 2)
    t = {k: inp[k].to(DEV) for k in R.FEAT_LEAVES + ("w2cs", "ixts", "gout")}
    plain = hip_point_feats(inp)
    with torch.no_grad():
        out = P().point_feats(*(t[k].clone().requires_grad_(True) for k in R.FEAT_LEAVES), t["w2cs"], t["ixts"])
    assert not out.requires_grad and torch.equal(out.cpu(), plain["out"])
    out, (g_depth, g_points) = torch.autograd.functional.vjp(
        lambda d, p: P().point_feats(t["img_ref"], t["image"], t["acc_map"], d, p, t["w2cs"], t["ixts"]), (t["depth"], t["points"]),
        t["gout"])
    assert torch.equal(out.cpu(), plain["out"]) and torch.equal(g_points.cpu(), plain["g_points"])
    check("point_feats vjp", dict(g_depth=g_depth.cpu()), truth, t32, inp, 13, 17, ["g_depth"])
    # bf16 autocast: half inputs are cast to fp32 inside and the output is fp32; fp32 inputs give the fp32 result
    with torch.autocast("cuda", dtype=torch.bfloat16):
        same = P().point_feats(*(t[k] for k in R.FEAT_LEAVES), t["w2cs"], t["ixts"])
        image16 = t["image"].bfloat16().requires_grad_(True)
        half = P().point_feats(t["img_ref"], image16, t["acc_map"], t["depth"], t["points"], t["w2cs"], t["ixts"])
        feats, z = P().sample_views(t["img_ref"].bfloat16(), t["points"], t["w2cs"], t["ixts"])
    assert same.dtype == torch.float32 and torch.equal(same.cpu(), plain["out"])
    assert half.dtype == torch.float32 and feats.dtype == torch.float32 and z.dtype == torch.float32
    want = P().point_feats(t["img_ref"], image16.detach().float(), t["acc_map"], t["depth"], t["points"], t["w2cs"], t["ixts"])
    assert torch.equal(half, want)
    half.backward(t["gout"])
    assert image16.grad is not None and image16.grad.dtype == torch.bfloat16 and torch.isfinite(image16.grad).all()


# ---- with the rasterizer ---------------------------------------------------------------------------------------------------
def _raster_graph(mode):
    """2 views at 32x32 of a few hundred Gaussians through the product Renderer -> point_feats -> a random upstream
    gradient; -> the features and the gradients at the Gaussian parameters.  mode: "hip", "torch_gpu" (the torch composition
    on the GPU in the same graph) or "torch_cpu" (the CPU f32 torch composition on the renders copied out, its gradients
    handed back to the same rasterizer backward)"""
    import math

    from generativedensification_amd.camera import orbit_cameras
    from generativedensification_amd.renderer import Renderer
    from generativedensification_amd.synthetic import make_scene

    S, V, N = 32, 2, 300
    scene = make_scene(400, seed=3, sh_degree=1, sigma0=(0.05, 0.02))
    g = {k: v.to(DEV).requires_grad_(True) for k, v in scene.items()}
    cams = orbit_cameras(4, S, S, device=DEV)[:V]
    rend = Renderer(sh_degree=1, white_background=True).render_views(cams, None, g["centers"], g["shs"], g["opacity"], g["scales"],
                                                                   g["rotations"], DEV, stacked=True)
    gen = torch.Generator().manual_seed(9)
    w2cs = torch.stack([c.world_view_transform.T for c in cams]).float()
    f = 0.5 * S / math.tan(0.375)
    ixts = torch.tensor([[f, 0, S / 2], [0, f, S / 2], [0, 0, 1.0]]).repeat(V, 1, 1).to(DEV)
    img_ref = torch.rand(V, 3, S, S, generator=gen).to(DEV)
    points = g["centers"][:N] + 0.01
    gout = (torch.randn(N, V, 8, generator=gen) * (1 + torch.arange(8.0))).to(DEV)
    mid = (rend["image"], rend["acc_map"], rend["depth"], points)
    if mode == "torch_cpu":
        leaves = [t.detach().cpu().requires_grad_(True) for t in mid]
        out = R.point_feats(img_ref.cpu(), *leaves, w2cs.cpu(), ixts.cpu())
        out.backward(gout.cpu())
        torch.autograd.backward(mid, [t.grad.to(DEV) for t in leaves])
    else:
        out = (P().point_feats if mode == "hip" else R.point_feats)(img_ref, *mid, w2cs, ixts)
        out.backward(gout)
    torch.cuda.synchronize()
    where = dict(points=points.detach().cpu(), w2cs=w2cs.cpu(), ixts=ixts.cpu())
    return out.detach().cpu(), {k: v.grad.detach().cpu() for k, v in g.items()}, where


def test_with_the_rasterizer():
    """the gradients that reach the Gaussian parameters through the coarse renders and the centres, against the same graph
    with the torch composition in place of point_feats (same rasterizer, same K7: GDR_K7_PAIRS pinned).  Truth is the torch
    composition on the GPU; err_torch32 is the CPU f32 torch composition in the same graph against it.  The features take the
    forward bar.  The parameter gradients descend from point_feats' image gradients, so they take the image-gradient bar with
    k_max counted from this case's f64 positions; what the rasterizer's own atomic backward adds is the same in all three
    runs and is inside err_torch32."""
    from generativedensification_amd import _lib as L

    lib = L.load()
    lib.gdr_k7_tune_override(0)
    try:
        out_t, g_t, where = _raster_graph("torch_gpu")
        out_c, g_c, _ = _raster_graph("torch_cpu")
        out_h, g_h, _ = _raster_graph("hip")
    finally:
        lib.gdr_k7_tune_override(int(os.environ["GDR_K7_PAIRS"]) if os.environ.get("GDR_K7_PAIRS") is not None else -1)
    T = out_t.double()
    err, err_t32 = R.max_err(out_h, T), R.max_err(out_c, T)
    print(f"rasterizer out: err_hip {err:.3e} err_torch32 {err_t32:.3e} bar {R.bar(err_t32, T):.3e}")
    assert err <= R.bar(err_t32, T)
    k_max = R.tap_stats(where, 32, 32)[0]
    print(f"rasterizer: k_max {k_max}")
    for k in g_t:
        T = g_t[k].double()
        assert torch.isfinite(g_h[k]).all() and float(T.abs().max()) > 0, k
        err, err_t32 = R.max_err(g_h[k], T), R.max_err(g_c[k], T)
        b = R.bar(err_t32, T, k_max)
        print(f"rasterizer d{k}: err_hip {err:.3e} err_torch32 {err_t32:.3e} bar {b:.3e}")
        assert err <= b, k


# ---- envelope --------------------------------------------------------------------------------------------------------------
def test_envelope_raises_before_any_launch():
    p = P()
    pts = torch.zeros(4, 3, device=DEV)
    with pytest.raises(ValueError, match="views"):
        p.sample_views(torch.zeros(17, 1, 2, 2, device=DEV), pts, torch.eye(4, device=DEV).repeat(17, 1, 1),
                       torch.eye(3, device=DEV).repeat(17, 1, 1))
    with pytest.raises(ValueError, match="views"):
        p.point_feats(torch.zeros(17, 3, 2, 2, device=DEV), torch.zeros(17, 2, 2, 3, device=DEV), torch.zeros(17, 2, 2, device=DEV),
                      torch.zeros(17, 2, 2, 1, device=DEV), pts, torch.eye(4, device=DEV).repeat(17, 1, 1),
                      torch.eye(3, device=DEV).repeat(17, 1, 1))
    w2c, ixt = torch.eye(4, device=DEV)[None], torch.eye(3, device=DEV)[None]
    with pytest.raises(ValueError, match="channels"):
        p.sample_views(torch.zeros(1, 4097, 1, 1, device=DEV), pts, w2c, ixt)
    with pytest.raises(RuntimeError, match="no CPU fallback"):            # mismatched devices
        p.sample_views(torch.zeros(1, 2, 2, 2, device=DEV), pts.cpu(), w2c, ixt)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        p.sample_views(torch.zeros(1, 2, 2, 2), pts, w2c, ixt)
    with pytest.raises(TypeError, match="float32"):                       # fp16 outside autocast
        p.sample_views(torch.zeros(1, 2, 2, 2, device=DEV, dtype=torch.float16), pts, w2c, ixt)
    with pytest.raises(TypeError, match="float32"):
        p.point_feats(torch.zeros(1, 3, 2, 2, device=DEV), torch.zeros(1, 2, 2, 3, device=DEV, dtype=torch.float16),
                      torch.zeros(1, 2, 2, device=DEV), torch.zeros(1, 2, 2, 1, device=DEV), pts, w2c, ixt)
    out, z = p.sample_views(torch.zeros(1, 2, 2, 2, device=DEV), pts[:0], w2c, ixt)        # N = 0: empty, no launch
    assert out.shape == (1, 2, 0) and z.shape == (1, 0)
