"""-m gpu: HIP product path (through the C ABI) vs the CPU oracle on the same seeded
inputs.  Integer / index work must be BIT-EXACT; floats within 1e-4 relative
(BASELINE.json north_star), tolerance written at each assert."""
import numpy as np
import pytest
import torch

import util as U

pytestmark = pytest.mark.gpu

CASES = [
    # N, H, W, seed, deg, sigma0
    (10_000, 256, 256, 0, 3, (0.0052, 0.00065)),     # C1 of BASELINE.json
    (3_000, 250, 190, 3, 3, (0.03, 0.01)),           # non-multiple-of-16 image, long tile lists
    (20_000, 128, 128, 5, 1, (0.02,)),               # SH degree 1 (reference default, configs/base.yaml:14)
    (2_000, 64, 64, 7, 0, (0.05,)),                  # SH degree 0, heavy overlap (early termination)
    (5_000, 96, 160, 9, 2, (0.01, 0.002)),           # SH degree 2, M = 9 (unaligned SH rows)
]


def _check_forward(o, h):
    # ---- integers / indices: bit-exact --------------------------------------------
    assert h["num_rendered"] == o["num_rendered"]
    np.testing.assert_array_equal(h["radii"], o["radii"])
    np.testing.assert_array_equal(h["rect"], o["rect"])
    np.testing.assert_array_equal(h["tiles_touched"].astype(np.uint32), o["tiles_touched"])
    np.testing.assert_array_equal(h["keys_sorted"].view(np.uint64), o["keys_sorted"])
    np.testing.assert_array_equal(h["point_list"].view(np.uint32), o["point_list"])
    np.testing.assert_array_equal(h["ranges"].view(np.uint32), o["ranges"])
    cl = np.stack([(h["clamped"] >> k) & 1 for k in range(3)], 1)
    np.testing.assert_array_equal(cl, o["clamped"])
    # ---- per-Gaussian floats: same op order, no FMA contraction -> bit-exact ---------
    for k in ("depths", "xy", "conic_opacity", "cov3D"):
        np.testing.assert_array_equal(h[k], o[k], err_msg=k)
    np.testing.assert_array_equal(h["rgb"][:, :3], o["rgb"])
    # ---- rendered images: 1e-4 relative (exp ulp differences can flip a 1/255 or 1e-4
    #      threshold at isolated pixels; those are counted, not hidden) ------------------
    for k in ("color", "depth", "alpha"):
        assert U.rel_inf(h[k], o[k]) < 5e-3, k                      # worst single pixel (flip-sized)
        assert U.outlier_fraction(h[k], o[k], rtol=1e-4, atol=1e-5) < 1e-4, k  # 1e-4 relative bar
    assert U.psnr(np.clip(h["color"], 0, 1), np.clip(o["color"], 0, 1)) > 60.0
    assert (h["n_contrib"].view(np.uint32) != o["n_contrib"]).mean() < 1e-4
    assert U.outlier_fraction(h["final_T"], o["final_T"], rtol=1e-4, atol=1e-6) < 1e-4


@pytest.mark.parametrize("N,H,W,seed,deg,sigma0", CASES)
def test_forward_and_backward_vs_oracle(oracle_built, N, H, W, seed, deg, sigma0):
    case = U.make_case(N, H, W, seed, deg=deg, sigma0=sigma0)
    grads = U.rand_grads(case)
    o, og = U.run_oracle(case, "f32", grads)
    h, hg = U.run_hip(case, grads)
    _check_forward(o, h)
    _, og64 = U.run_oracle(case, "f64", grads)
    # per element against the f32 oracle (1e-4 |ref| + 1e-6 max|ref|), f64 oracle as arbiter: util.assert_grads
    U.assert_grads(hg, og64, og, ("means3D", "means2D", "shs", "opacities", "scales", "rotations"), f"N={N}")
    # culled Gaussians get exact zeros everywhere (set_detect_anomaly-safe, train_lightning.py:31)
    culled = o["radii"] == 0
    for k in ("means3D", "means2D", "shs", "opacities", "scales", "rotations"):
        assert np.isfinite(hg[k]).all(), k
        assert not hg[k][culled].any(), k


def test_colors_precomp_and_cov3d_precomp(oracle_built):
    case = U.make_case(4_000, 112, 144, 21, deg=0, sigma0=(0.02, 0.004), colors_precomp=True, cov_precomp=True)
    grads = U.rand_grads(case)
    o, og = U.run_oracle(case, "f32", grads)
    h, hg = U.run_hip(case, grads)
    assert h["num_rendered"] == o["num_rendered"]
    np.testing.assert_array_equal(h["point_list"].view(np.uint32), o["point_list"])
    assert U.outlier_fraction(h["color"], o["color"], 1e-4, 1e-5) < 1e-4
    _, og64 = U.run_oracle(case, "f64", grads)
    U.assert_grads(hg, og64, og, ("means3D", "means2D", "colors_precomp", "opacities", "cov3D_precomp"), "precomp")
    assert hg["shs"] is None and hg["scales"] is None and hg["rotations"] is None


def test_empty_and_all_culled(oracle_built):
    dev = torch.device("cuda:0")
    from generativedensification_amd.rasterizer import GaussianRasterizer

    case = U.make_case(100, 64, 64, 1, deg=1, sigma0=(0.02,))
    rs = U.settings_torch(case, dev)
    r = GaussianRasterizer(rs)
    # all behind the camera
    means = (case["means3D"] * 0 + case["campos"] * 0 - 100.0 * torch.tensor([0.0, 0.0, 0.0])).to(dev)
    means = (case["means3D"] + 50.0 * (case["view"][:3, 2])).to(dev) * -1.0
    means.requires_grad_(True)
    col, radii, dep, alp = r(means3D=means, means2D=torch.zeros(100, 4, device=dev, requires_grad=True),
                             shs=case["shs"].to(dev), opacities=case["opacities"].to(dev),
                             scales=case["scales"].to(dev), rotations=case["rotations"].to(dev))
    (col.sum() + dep.sum() + alp.sum()).backward()
    if int((radii > 0).sum()) == 0:
        assert torch.allclose(col, rs.bg[:, None, None].expand_as(col))
        assert float(alp.detach().abs().max()) == 0.0
        assert float(means.grad.abs().max()) == 0.0
    # N = 0
    z = torch.zeros(0, 3, device=dev)
    col, radii, dep, alp = r(means3D=z, means2D=torch.zeros(0, 4, device=dev), shs=torch.zeros(0, 4, 3, device=dev),
                             opacities=torch.zeros(0, 1, device=dev), scales=z, rotations=torch.zeros(0, 4, device=dev))
    assert radii.numel() == 0 and torch.allclose(col, rs.bg[:, None, None].expand_as(col))


# ---- golden fixtures (reference caller code + oracle, tests/golden/make_golden.py) ----------
import os

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _fovs(g):
    """(fovx, fovy) of a render_img fixture: `fov` where they are equal, `fovx`, `fovy` where they differ."""
    return (float(g["fovx"]), float(g["fovy"])) if "fovx" in g else (float(g["fov"]),) * 2


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name", ["render_img_deg3.npz", "render_img_deg1.npz", "render_img_fovxy.npz"])
def test_product_renderer_on_gpu_matches_golden_render_img(name, fused):
    """The repo's Renderer mirror + HIP rasterizer (the full product path, through the C ABI)
    against what the reference's own Renderer.render_img produced on the fixture."""
    from generativedensification_amd.camera import MiniCam
    from generativedensification_amd.renderer import Renderer
    from generativedensification_amd.synthetic import view_loss

    g = dict(np.load(os.path.join(GOLD, name)))
    dev = torch.device("cuda:0")
    cam = MiniCam(torch.from_numpy(g["c2w"]), int(g["w"]), int(g["h"]), torch.tensor(_fovs(g)[1]),
                  torch.tensor(_fovs(g)[0]), float(g["znear"]), float(g["zfar"]), dev)
    r = Renderer(sh_degree=int(g["sh_degree"]), white_background=True, fused=fused)
    r.set_bg_color(torch.from_numpy(g["bg"]))
    leaves = {k: torch.from_numpy(g[f"in_{k}"]).to(dev).requires_grad_(True)
              for k in ("centers", "shs", "opacity", "scales", "rotations")}
    ssp = torch.zeros(int(g["n"]), 4, device=dev, requires_grad=True)
    out = r.render_img(cam, None, leaves["centers"], leaves["shs"], leaves["opacity"], leaves["scales"],
                       leaves["rotations"], dev, screenspace_points=ssp)
    for k in ("image", "depth", "acc_map"):
        got = out[k].detach().cpu().numpy()
        assert got.shape == g[k].shape
        # 1e-4 relative; activations (sigmoid/exp/normalize) run in torch on the GPU here, so a
        # few-ulp input difference vs the CPU fixture is expected on top of kernel rounding
        assert U.outlier_fraction(got, g[k], rtol=1e-4, atol=2e-5) < 5e-4, k
    assert U.psnr(out["image"].detach().cpu().numpy(), g["image"]) > 60.0
    loss = view_loss(out, torch.from_numpy(g["target"]).to(dev))
    grads = torch.autograd.grad(loss, list(leaves.values()) + [ssp])
    for k, gr in zip(list(leaves) + ["screenspace_points"], grads):
        assert U.rel_inf(gr.cpu().numpy(), g[f"grad_{k}"]) < 2e-4, k
    assert grads[-1].shape == (int(g["n"]), 4) and float(grads[-1][:, 2:].min()) >= 0.0


def test_product_rasterizer_legacy_caller_on_gpu_matches_golden():
    """(N,3) means2D, colors_precomp, bg on device, visibility filter = radii > 0
    (lightning/point_decoder/layers/gaussian_renderer.py:88-114)."""
    import math

    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer

    g = dict(np.load(os.path.join(GOLD, "legacy_render_colors.npz")))
    dev = torch.device("cuda:0")
    n, h, w = int(g["n"]), int(g["h"]), int(g["w"])
    t = lambda k: torch.from_numpy(g[k]).to(dev).requires_grad_(True)
    pos, col, opa, sca, rot = t("position"), t("override_color"), t("opacity"), t("scaling"), t("rotation")
    ssp = torch.zeros(n, 3, device=dev, requires_grad=True)
    rs = GaussianRasterizationSettings(
        image_height=h, image_width=w, tanfovx=math.tan(0.375), tanfovy=math.tan(0.375),
        bg=torch.from_numpy(g["bg"]).to(dev), scale_modifier=1.0,
        viewmatrix=torch.from_numpy(g["world_view_transform"]).to(dev),
        projmatrix=torch.from_numpy(g["full_proj_transform"]).to(dev), sh_degree=0,
        campos=torch.from_numpy(g["camera_center"]).to(dev), prefiltered=False, debug=False)
    img, radii, depth, alpha = GaussianRasterizer(rs)(means3D=pos, means2D=ssp, shs=None, colors_precomp=col,
                                                      opacities=opa, scales=sca, rotations=rot, cov3D_precomp=None)
    np.testing.assert_array_equal(radii.cpu().numpy(), g["radii"])          # bit-exact ints (same inputs)
    np.testing.assert_array_equal((radii > 0).cpu().numpy(), g["visibility_filter"])
    assert U.outlier_fraction(img.detach().cpu().numpy(), g["render"], 1e-4, 1e-5) < 1e-4
    grads = torch.autograd.grad((img * torch.from_numpy(g["grad_image"]).to(dev)).sum(), [pos, col, opa, sca, rot, ssp])
    for k, gr in zip(["position", "override_color", "opacity", "scaling", "rotation", "screenspace_points"], grads):
        assert U.rel_inf(gr.cpu().numpy(), g[f"grad_{k}"]) < 1e-4, k
    assert grads[-1].shape == (n, 3) and not grads[-1][:, 2].any()
    vis = GaussianRasterizer(rs).markVisible(pos.detach())
    assert vis.dtype == torch.bool and vis.shape == (n,)


def test_vjp_and_no_grad_and_autocast_contracts():
    """torch.autograd.functional.vjp over 4 views w.r.t. the (N,4) carrier (network.py:865-878),
    torch.no_grad() eval (evaluation.py:45,77), bf16 autocast caller (train_lightning.py:79)."""
    from torch.autograd.functional import vjp

    from generativedensification_amd.camera import orbit_cameras
    from generativedensification_amd.renderer import Renderer
    from generativedensification_amd.synthetic import make_scene, make_targets

    dev = torch.device("cuda:0")
    n, h, w = 3000, 64, 64
    sc = {k: v.to(dev) for k, v in make_scene(n, 31, sh_degree=1, sigma0=(0.02,)).items()}
    cams = orbit_cameras(4, w, h, device=dev)
    tg = make_targets(4, h, w, 31).to(dev)
    r = Renderer(sh_degree=1)

    def fn(ssp):
        imgs = [r.render_img(c, None, sc["centers"], sc["shs"], sc["opacity"], sc["scales"], sc["rotations"], dev,
                             screenspace_points=ssp)["image"] for c in cams]
        return ((torch.stack(imgs) - tg) ** 2).mean()

    with torch.no_grad():  # evaluation.py wraps the whole net in no_grad; vjp re-enables grad inside
        loss, grad = vjp(fn, torch.zeros(n, 4, device=dev))
        out = r.render_img(cams[0], None, sc["centers"], sc["shs"], sc["opacity"], sc["scales"], sc["rotations"], dev)
    assert grad.shape == (n, 4) and torch.isfinite(grad).all() and float(grad[:, 2:].norm()) > 0
    assert (grad[:, 2:] >= grad[:, :2].abs() - 1e-6 * grad[:, 2:].abs().max()).all()  # sum|t| >= |sum t|
    assert not out["image"].requires_grad
    with torch.autocast("cuda", dtype=torch.bfloat16):
        o2 = r.render_img(cams[0], None, sc["centers"], sc["shs"], sc["opacity"], sc["scales"], sc["rotations"], dev)
    assert o2["image"].dtype == torch.float32
    assert torch.allclose(o2["image"], out["image"], atol=1e-6)
    with torch.autograd.set_detect_anomaly(True):  # train_lightning.py:31
        leaves = {k: v.clone().requires_grad_(True) for k, v in sc.items()}
        o3 = r.render_img(cams[1], None, leaves["centers"], leaves["shs"], leaves["opacity"], leaves["scales"],
                          leaves["rotations"], dev)
        (o3["image"].mean() + o3["depth"].mean() + o3["acc_map"].mean()).backward()
    assert all(torch.isfinite(v.grad).all() for v in leaves.values())


@pytest.mark.parametrize("V", [3, 10])   # 10 > GDR_MAX_VIEWS = 8: two kernel groups, the second accumulating
def test_fused_multiview_node_equals_per_view_sequence_on_identical_inputs(V):
    """The multi-view node (one K1 / K9 launch per <= 8 views, grads summed over the views inside K9, one D read-back,
    views on side streams) against the reference's sequence — one rasterizer call per view, autograd summing the
    gradients — on the SAME activated tensors (flags = 0: no in-kernel activations), so both run identical arithmetic
    per view: images, depth, alpha bit-equal; gradients differ by the order of fp32 sums only and meet the per-element
    bar with no allowance.  (The in-kernel activations of the RAW entry are compared with the ORACLE in
    test_gpu_oracle_fullsize.py::test_render_views_backward_vs_oracle — round 2's version of this test compared two HIP
    paths with different activations and loosened its bar when an alpha-threshold decision flipped.)"""
    import diff_gaussian_rasterization as D
    from generativedensification_amd import rasterizer as R
    from generativedensification_amd.camera import orbit_cameras
    from generativedensification_amd.renderer import Renderer
    from generativedensification_amd.synthetic import make_scene, make_targets

    dev = torch.device("cuda:0")
    n, h, w = 30_000, 160, 208
    sc = make_scene(n, 77, sh_degree=3, sigma0=(0.0052, 0.00065, 0.02))
    cams = orbit_cameras(V, w, h, device=dev)
    tg = make_targets(V, h, w, 77).to(dev).permute(0, 3, 1, 2)
    three = ([1.0, 1.0, 1.0], [0.5, 0.5, 0.5], [0.0, 0.0, 0.0])   # gobjverse.py:112-117
    r = Renderer(sh_degree=3)
    sets = []
    for j, c in enumerate(cams):
        r.set_bg_color(torch.tensor(three[j % 3], device=dev))
        sets.append(r.set_rasterizer(c, device=dev).raster_settings)
    act = dict(means3D=sc["centers"].to(dev), shs=sc["shs"].to(dev), opacities=torch.sigmoid(sc["opacity"]).to(dev),
               scales=torch.exp(sc["scales"]).to(dev), rotations=torch.nn.functional.normalize(sc["rotations"]).to(dev))

    def loss_of(colors, depths, alphas):
        return sum(((c.clamp(0, 1) - tg[j]) ** 2).mean() + 0.1 * d.mean() + 0.1 * a.mean()
                   for j, (c, d, a) in enumerate(zip(colors, depths, alphas)))

    def run(fused):
        leaves = {k: v.clone().requires_grad_(True) for k, v in act.items()}
        ssp = torch.zeros(n, 4, device=dev, requires_grad=True)
        if fused:
            colors, radii, depths, alphas = R.render_views_raw(leaves["means3D"], ssp, leaves["shs"], leaves["opacities"],
                                                               leaves["scales"], leaves["rotations"], sets, flags=0)
        else:
            outs = [D.GaussianRasterizer(rs)(means3D=leaves["means3D"], means2D=ssp, shs=leaves["shs"],
                                             opacities=leaves["opacities"], scales=leaves["scales"],
                                             rotations=leaves["rotations"]) for rs in sets]
            colors, depths, alphas = [o[0] for o in outs], [o[2] for o in outs], [o[3] for o in outs]
        grads = torch.autograd.grad(loss_of(colors, depths, alphas), list(leaves.values()) + [ssp])
        imgs = [torch.cat([c, d, a]).detach().cpu().numpy() for c, d, a in zip(colors, depths, alphas)]
        return imgs, {k: g_.cpu().numpy() for k, g_ in zip(list(leaves) + ["ssp"], grads)}

    o_ref, g_ref = run(False)
    o_fus, g_fus = run(True)
    for a, b in zip(o_fus, o_ref):
        np.testing.assert_array_equal(a, b)
    for k in g_ref:
        out, worst, maxn = U.elem_stats(g_fus[k], g_ref[k])
        assert out < U.MAX_OUTSIDE and maxn < 1e-4, (k, out, worst, maxn)
    assert g_fus["ssp"].shape == (n, 4) and (g_fus["ssp"][:, 2:] >= 0).all()


@pytest.mark.parametrize("V", [4, 9])
def test_k7_of_all_views_in_one_launch_equals_per_view_launches(V):
    """gdr_render_backward_views / _loss_views / _mean2d_views (round 4: K7 of the views of a node in ONE launch, the
    views interleaved — mode 1 — or one after the other — mode 2) against one K7 launch per view on side streams (mode 0):
    same kernel, same records, so the gradients differ by the order of the fp32 atomics only.  Lists long enough to be
    cut (sigma 0.02: several 256-entry segments per tile), per-view bg colours, V = 9 > GDR_MAX_VIEWS (two launches)."""
    from generativedensification_amd import rasterizer as R
    from generativedensification_amd.camera import orbit_cameras
    from generativedensification_amd.renderer import Renderer
    from generativedensification_amd.synthetic import make_scene, make_targets

    dev = torch.device("cuda:0")
    n, h, w = 30_000, 160, 208
    sc = make_scene(n, 78, sh_degree=3, sigma0=(0.0052, 0.00065, 0.02))
    cams = orbit_cameras(V, w, h, device=dev)
    tg = make_targets(V, h, w, 78).to(dev)
    tg_chw = tg.permute(0, 3, 1, 2).contiguous()
    three = ([1.0, 1.0, 1.0], [0.5, 0.5, 0.5], [0.0, 0.0, 0.0])
    bgs = [torch.tensor(three[j % 3], device=dev) for j in range(V)]
    wts = torch.linspace(0.5, 2.0, V, device=dev)
    r = Renderer(sh_degree=3, fused=True)

    def run(mode, entry):
        prev, R.K.K7_VIEWS = R.K.K7_VIEWS, mode
        try:
            leaves = {k: v.to(dev).clone().requires_grad_(True) for k, v in sc.items()}
            ssp = torch.zeros(n, 4, device=dev, requires_grad=True)
            args = (leaves["centers"], leaves["shs"], leaves["opacity"], leaves["scales"], leaves["rotations"], dev)
            if entry == "absgrad":
                loss, grad = r.screenspace_absgrad(cams, bgs, tg, *args)
                return {"loss": loss.detach().cpu().numpy(), "ssp": grad.cpu().numpy()}
            if entry == "loss":
                lv = r.render_views_loss(cams, bgs, tg_chw, *args, screenspace_points=ssp)
            else:
                outs = r.render_views(cams, bgs, *args, screenspace_points=ssp)
                lv = torch.stack([((o["image"] - tg[j]) ** 2).mean() + 0.1 * o["depth"].mean() + 0.1 * o["acc_map"].mean()
                                  for j, o in enumerate(outs)])
            grads = torch.autograd.grad((lv * wts).sum(), list(leaves.values()) + [ssp])
            return {k: g_.cpu().numpy() for k, g_ in zip(list(leaves) + ["ssp"], grads)}
        finally:
            R.K.K7_VIEWS = prev

    for entry in ("views", "loss", "absgrad"):
        ref = run(0, entry)
        for mode in (1, 2):
            got = run(mode, entry)
            for k in ref:
                out, worst, maxn = U.elem_stats(got[k], ref[k])
                assert out < U.MAX_OUTSIDE and maxn < 1e-4, (entry, mode, k, out, worst, maxn)


def test_k7_row_pair_kernel_equals_the_row_kernel_and_the_oracle(oracle_built):
    """render_bwd_pairs_kernel (round 4, include/gdr.h gdr_k7_tune_override): where the entries of a slice mostly cover both
    4x4 blocks of a row pair, the two rows walk the union of their lists and publish ONE record line — the same sums in
    another order.  Gaussians of 10-30 pixels (the regime it is for) mixed with sub-pixel ones (slices that stay in row
    mode), lists long enough to be cut; the three entries (full records, fused loss, mean2D only), one launch for the
    views; and the single-view path against the f32 / f64 oracles."""
    from generativedensification_amd import _lib as L
    from generativedensification_amd.camera import orbit_cameras
    from generativedensification_amd.renderer import Renderer
    from generativedensification_amd.synthetic import make_scene, make_targets

    lib = L.load()
    dev = torch.device("cuda:0")
    V, n, h, w = 4, 30_000, 160, 208
    sc = make_scene(n, 91, sh_degree=3, sigma0=(0.03, 0.0052, 0.06))
    cams = orbit_cameras(V, w, h, device=dev)
    tg = make_targets(V, h, w, 91).to(dev)
    tg_chw = tg.permute(0, 3, 1, 2).contiguous()
    wts = torch.linspace(0.5, 2.0, V, device=dev)
    r = Renderer(sh_degree=3, fused=True)

    def run(entry):
        leaves = {k: v.to(dev).clone().requires_grad_(True) for k, v in sc.items()}
        ssp = torch.zeros(n, 4, device=dev, requires_grad=True)
        args = (leaves["centers"], leaves["shs"], leaves["opacity"], leaves["scales"], leaves["rotations"], dev)
        if entry == "absgrad":
            loss, grad = r.screenspace_absgrad(cams, None, tg, *args)
            return {"loss": loss.detach().cpu().numpy(), "ssp": grad.cpu().numpy()}
        if entry == "loss":
            lv = r.render_views_loss(cams, None, tg_chw, *args, screenspace_points=ssp)
        else:
            outs = r.render_views(cams, None, *args, screenspace_points=ssp)
            lv = torch.stack([((o["image"] - tg[j]) ** 2).mean() + 0.1 * o["depth"].mean() + 0.1 * o["acc_map"].mean()
                              for j, o in enumerate(outs)])
        grads = torch.autograd.grad((lv * wts).sum(), list(leaves.values()) + [ssp])
        return {k: g_.cpu().numpy() for k, g_ in zip(list(leaves) + ["ssp"], grads)}

    try:
        for entry in ("views", "loss", "absgrad"):
            lib.gdr_k7_tune_override(0)
            ref = run(entry)
            lib.gdr_k7_tune_override(1)
            got = run(entry)
            for k in ref:
                out, worst, maxn = U.elem_stats(got[k], ref[k])
                assert out < U.MAX_OUTSIDE and maxn < 1e-4, (entry, k, out, worst, maxn)
        case = U.make_case(6000, 128, 144, 17, deg=3, sigma0=(0.05, 0.01))
        grads = U.rand_grads(case)
        _, g32 = U.run_oracle(case, "f32", grads)
        _, g64 = U.run_oracle(case, "f64", grads, nthreads=8)
        for mode in (0, 1):
            lib.gdr_k7_tune_override(mode)
            _, hg = U.run_hip(case, grads)
            U.assert_grads(hg, g64, g32, ("means3D", "means2D", "shs", "opacities", "scales", "rotations"), f"k7 variant {mode}")
    finally:
        lib.gdr_k7_tune_override(-1)


@pytest.mark.parametrize("interleave", [0, 1])
def test_k6_of_all_views_in_one_launch_reproduces_the_per_view_images(interleave):
    """gdr_composite_forward_views (include/gdr.h, v14; SURVEY section 7 step 5 "grid.z = view"): K6 of V views in ONE launch
    on the binning state a multi-view forward left behind — images, final T and contributor counts bit for bit those of the
    per-view launches (same kernel, same lists; measured on MI355X the one-launch form is not faster than per-view K6 behind
    each view's own binning chain — C4 +-0, C3 +1.3 %, C2 -1..-3 % — so the node keeps the chains)."""
    import ctypes as C
    from generativedensification_amd import _lib as L
    from generativedensification_amd import rasterizer as R
    from generativedensification_amd.camera import orbit_cameras
    from generativedensification_amd.renderer import Renderer
    from generativedensification_amd.synthetic import make_scene

    dev = torch.device("cuda:0")
    lib = L.load()
    V, n, h, w = 5, 30_000, 160, 208
    sc = make_scene(n, 79, sh_degree=2, sigma0=(0.0052, 0.00065, 0.02), device=dev)
    cams = orbit_cameras(V, w, h, device=dev)
    r = Renderer(sh_degree=2)
    sets = [r.set_rasterizer(c, device=dev).raster_settings for c in cams]
    with torch.no_grad():
        colors, radii, depths, alphas, states, keep, _ = R._forward_views_impl(
            sc["centers"], torch.empty(0, 4, device=dev), sc["shs"], sc["opacity"], sc["scales"], sc["rotations"], tuple(sets), R.RAW_ALL)
        torch.cuda.synchronize()
        ref = [(c.clone(), d.clone(), a.clone(), st.tensors()["n_contrib"].clone(), st.tensors()["final_T"].clone())
               for c, d, a, st in zip(colors, depths, alphas, states)]
        for st in states:     # wipe what K6 wrote
            st.tensors()["n_contrib"].zero_()
            st.tensors()["final_T"].zero_()
        out = [(torch.zeros_like(c), torch.zeros_like(d), torch.zeros_like(a)) for c, d, a in zip(colors, depths, alphas)]
        s_arr = keep[-1]
        g_arr, b_arr, i_arr = R._view_arrays(states, 0, V, 0)
        o_arr = (L.GdrOutputs * V)(*[L.GdrOutputs(c.data_ptr(), d.data_ptr(), a.data_ptr(), radii[v].data_ptr())
                                     for v, (c, d, a) in enumerate(out)])
        L.check(lib.gdr_composite_forward_views(V, s_arr, g_arr, b_arr, i_arr, o_arr, 0, None, 0.0, 0.0, 1.0, None, interleave,
                                                R._stream()), "gdr_composite_forward_views")
        torch.cuda.synchronize()
    for v in range(V):
        t = states[v].tensors()
        for got, want in zip(out[v] + (t["n_contrib"], t["final_T"]), ref[v]):
            assert torch.equal(got, want), v


def test_float64_noncontiguous_inputs_and_debug_mode():
    """The boundary accepts what a caller may hand it: float64 tensors, non-contiguous views (a transposed SH block, a
    strided slice of a bigger tensor) — same result as float32 contiguous inputs, gradients come back in the callers'
    dtypes — and `debug=True` (synchronise + check after every kernel) runs the same kernels."""
    import diff_gaussian_rasterization as D

    dev = torch.device("cuda:0")
    case = U.make_case(3000, 80, 96, 87, deg=1, sigma0=(0.02, 0.05))
    rs = U.settings_torch(case, dev)
    t = {k: case[k].to(dev) for k in ("means3D", "shs", "opacities", "scales", "rotations")}

    def run(inputs, settings):
        leaves = {k: v.clone().requires_grad_(True) for k, v in inputs.items()}
        m2 = torch.zeros(case["N"], 4, device=dev, dtype=leaves["opacities"].dtype, requires_grad=True)
        views = dict(leaves)
        if "shs_T" in leaves:      # (N,3,M) storage seen as (N,M,3): non-contiguous
            views["shs"] = leaves["shs_T"].transpose(1, 2)
        if "means_wide" in leaves:  # every second row of a (2N,3) tensor
            views["means3D"] = leaves["means_wide"][::2]
        img, radii, depth, alpha = D.GaussianRasterizer(settings)(
            means3D=views["means3D"], means2D=m2, shs=views["shs"], opacities=views["opacities"], scales=views["scales"],
            rotations=views["rotations"])
        loss = (img.float() ** 2).mean() + depth.float().mean() + alpha.float().mean()
        g = torch.autograd.grad(loss, list(leaves.values()))
        return img.detach().float().cpu().numpy(), dict(zip(leaves, g))

    img0, g0 = run(t, rs)
    # float64 everywhere
    img1, g1 = run({k: v.double() for k, v in t.items()}, rs)
    np.testing.assert_array_equal(img1, img0)
    for k in g0:
        assert g1[k].dtype == torch.float64
        assert U.rel_inf(g1[k].float().cpu().numpy(), g0[k].cpu().numpy()) < 1e-5, k
    # non-contiguous views
    wide = torch.zeros(2 * case["N"], 3, device=dev)
    wide[::2] = t["means3D"]
    nc = dict(t)
    nc.pop("shs"); nc.pop("means3D")
    nc["shs_T"] = t["shs"].transpose(1, 2).contiguous()
    nc["means_wide"] = wide
    img2, g2 = run(nc, rs)
    np.testing.assert_array_equal(img2, img0)
    assert U.rel_inf(g2["shs_T"].transpose(1, 2).cpu().numpy(), g0["shs"].cpu().numpy()) < 1e-5
    assert U.rel_inf(g2["means_wide"][::2].cpu().numpy(), g0["means3D"].cpu().numpy()) < 1e-5
    assert not g2["means_wide"][1::2].any()
    # debug mode
    img3, g3 = run(t, rs._replace(debug=True))
    np.testing.assert_array_equal(img3, img0)
    for k in g0:
        assert U.rel_inf(g3[k].cpu().numpy(), g0[k].cpu().numpy()) < 1e-5, k


@pytest.mark.parametrize("deg", [0, 1, 2])
def test_active_sh_degree_below_the_stored_coefficients(oracle_built, deg):
    """shs hold 16 coefficients (M = 16) but only (deg+1)^2 are active — the progressive-SH situation of 3DGS training
    (M > (sh_degree+1)^2: the un-staged K9 paths).  Single-view and multi-view kernels vs the oracle; the gradient of the
    inactive coefficients is exactly zero."""
    from generativedensification_amd import rasterizer as R

    case = U.make_case(5000, 96, 128, 83, deg=3, sigma0=(0.01, 0.04))
    case["deg"] = deg
    grads = U.rand_grads(case)
    hip, hg = U.run_hip(case, grads)
    ora, g32 = U.run_oracle(case, "f32", grads)
    _, g64 = U.run_oracle(case, "f64", grads, nthreads=8)
    np.testing.assert_array_equal(hip["point_list"], ora["point_list"])
    assert U.outlier_fraction(hip["color"], ora["color"], 1e-4, 1e-4) < 1e-4
    nb = (deg + 1) ** 2
    assert not hg["shs"].reshape(-1, 16, 3)[:, nb:].any()

    def close(x, k, scale=1.0):  # per element against the f32 oracle, f64 as arbiter (util.assert_grads)
        shape = g64[k].shape
        U.assert_grads({k: np.asarray(x).reshape(shape)}, {k: scale * g64[k]}, {k: scale * g32[k].reshape(shape)}, [k],
                       f"deg={deg} x{scale}")

    for k in ("means3D", "shs", "opacities", "scales", "rotations"):
        close(hg[k], k)
    # the multi-view node (V = 2: the same view twice) must give twice the single-view gradient
    dev = torch.device("cuda:0")
    rs = U.settings_torch(case, dev)
    leaves = {k: case[k].to(dev).clone().requires_grad_(True) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    m2 = torch.zeros(case["N"], 4, device=dev, requires_grad=True)
    colors, radii, depths, alphas = R.render_views_raw(leaves["means3D"], m2, leaves["shs"], leaves["opacities"],
                                                       leaves["scales"], leaves["rotations"], [rs, rs], flags=0)
    gc, gd, ga = (g.to(dev) for g in grads)
    loss = sum((c * gc).sum() + (d * gd).sum() + (a * ga).sum() for c, d, a in zip(colors, depths, alphas))
    gv = torch.autograd.grad(loss, list(leaves.values()))
    for k, x in zip(leaves, gv):
        close(x.cpu().numpy(), k, 2.0)
    assert not gv[1][:, nb:].any()


@pytest.mark.parametrize("surfel", [False, True])
def test_multiview_nodes_with_no_gaussians_at_all(surfel):
    """N = 0 through the multi-view nodes (forward, folded loss, backward): background images, zero-size gradients."""
    from generativedensification_amd.camera import build_rays, orbit_cameras

    dev = torch.device("cuda:0")
    h, w, V = 48, 64, 3
    cams = orbit_cameras(V, w, h, device=dev)
    bg = torch.tensor([0.3, 0.5, 0.7], device=dev)
    z = lambda *shape: torch.zeros(*shape, device=dev, requires_grad=True)
    tg = torch.rand(V, 3, h, w, device=dev)
    if surfel:
        from generativedensification_amd.renderer_2dgs import Renderer
        r = Renderer(sh_degree=1, white_background=False)
        rays = [build_rays(torch.inverse(c.world_view_transform.T.cpu()), 0.75, 0.75, h, w).to(dev) for c in cams]
        args = (z(0, 3), z(0, 4, 3), z(0, 1), z(0, 2), z(0, 4), dev)
        outs = r.render_views(cams, rays, bg, *args, raw=True)
        lv = r.render_views_loss(cams, rays, bg, tg, *args)
    else:
        from generativedensification_amd.renderer import Renderer
        r = Renderer(sh_degree=1, white_background=False)
        args = (z(0, 3), z(0, 4, 3), z(0, 1), z(0, 3), z(0, 4), dev)
        outs = r.render_views(cams, bg, *args, raw=True)
        lv = r.render_views_loss(cams, bg, tg, *args)
    for o in outs:
        torch.testing.assert_close(o["color"], bg.view(3, 1, 1).expand(3, h, w))
    assert lv.shape == (V,) and torch.isfinite(lv).all()
    g = torch.autograd.grad(lv.sum() + sum(o["color"].sum() for o in outs), list(args[:5]), allow_unused=True)
    for x, a in zip(g, args[:5]):
        assert x is None or x.shape == a.shape


@pytest.mark.parametrize("surfel", [False, True])
def test_multiview_node_with_a_view_that_sees_nothing(surfel):
    """One of three cameras looks away from the scene (num_rendered = 0 for that view: empty binning workspace, empty
    tile lists): its image is the background, and the node's gradients equal those of the two seeing views alone."""
    from generativedensification_amd.camera import MiniCam, look_at_c2w, orbit_cameras
    from generativedensification_amd.synthetic import make_scene

    dev = torch.device("cuda:0")
    n, h, w = 8000, 96, 112
    sc = make_scene(n, 5, sh_degree=1, sigma0=(0.01, 0.03))
    if surfel:
        from generativedensification_amd.renderer_2dgs import Renderer
        sc["scales"] = sc["scales"][:, :2].contiguous()
    else:
        from generativedensification_amd.renderer import Renderer
    cams = orbit_cameras(2, w, h, device=dev)
    eye = torch.tensor([0.0, 0.0, 1.9])
    away = MiniCam(look_at_c2w(eye, 2.0 * eye), w, h, 0.75, 0.75, 1.1, 2.7, dev)   # the scene is behind this camera
    bg = torch.tensor([0.2, 0.6, 1.0], device=dev)
    r = Renderer(sh_degree=1, white_background=False)

    def run(cs):
        leaves = {k: v.to(dev).clone().requires_grad_(True) for k, v in sc.items()}
        args = (leaves["centers"], leaves["shs"], leaves["opacity"], leaves["scales"], leaves["rotations"], dev)
        outs = r.render_views(cs, [None] * len(cs), bg, *args, raw=True) if surfel else r.render_views(cs, bg, *args, raw=True)
        loss = sum((o["color"] ** 2).mean() + (o["allmap"][:2] if surfel else o["depth"]).mean() for o in outs)
        g = torch.autograd.grad(loss, list(leaves.values()))
        return outs, {k: x.cpu().numpy() for k, x in zip(leaves, g)}

    o3, g3 = run([cams[0], away, cams[1]])
    o2, g2 = run(cams)
    blank = o3[1]["color"]
    torch.testing.assert_close(blank, bg.view(3, 1, 1).expand_as(blank))
    assert float((o3[1]["allmap"] if surfel else o3[1]["alpha"]).detach().abs().max()) == 0.0
    for a, b in ((o3[0], o2[0]), (o3[2], o2[1])):
        np.testing.assert_array_equal(a["color"].detach().cpu().numpy(), b["color"].detach().cpu().numpy())
    for k in g2:
        assert np.isfinite(g3[k]).all()
        assert U.rel_inf(g3[k], g2[k]) < 1e-5, k


def test_multiview_kernels_keep_integer_intermediates_bit_exact(oracle_built):
    """The multi-view K1 (inputs read once for V views) must give the oracle's radii / sorted list per view
    when fed the same ACTIVATED inputs (flags = 0)."""
    from generativedensification_amd import rasterizer as R
    from generativedensification_amd.camera import orbit_cameras

    dev = torch.device("cuda:0")
    case = U.make_case(20_000, 208, 176, 41, deg=3, sigma0=(0.0052, 0.00065))
    cams = orbit_cameras(3, 176, 208)
    sets = []
    for c in cams:
        cc = dict(case, view=c.world_view_transform.contiguous(), proj=c.full_proj_transform.contiguous(),
                  campos=c.camera_center.contiguous())
        sets.append(cc)
    t = lambda k: case[k].to(dev)
    colors, radii, depths, alphas = R.render_views_raw(t("means3D"), torch.zeros(case["N"], 4, device=dev), t("shs"),
                                                       t("opacities"), t("scales"), t("rotations"),
                                                       [U.settings_torch(cc, dev) for cc in sets], flags=0)
    for v, cc in enumerate(sets):
        o, _ = U.run_oracle(cc, "f32")
        np.testing.assert_array_equal(radii[v].cpu().numpy(), o["radii"])
        assert colors[v].shape == (3, 208, 176) and depths[v].shape == (1, 208, 176)
        assert U.outlier_fraction(colors[v].cpu().numpy(), o["color"], 1e-4, 1e-5) < 1e-4
        assert U.outlier_fraction(depths[v].cpu().numpy(), o["depth"], 1e-4, 1e-5) < 1e-4


def test_global_sort_fallback_paths(oracle_built):
    """(a) forced global LSD radix sort, (b) tile lists longer than one workgroup's LDS (automatic
    fallback): both must give the oracle's sorted list bit for bit."""
    from generativedensification_amd import rasterizer as R

    case = U.make_case(10_000, 256, 256, 0, deg=3)
    o, _ = U.run_oracle(case, "f32")
    R.K.FORCE_GLOBAL_SORT = True
    try:
        h, _ = U.run_hip(case)
    finally:
        R.K.FORCE_GLOBAL_SORT = False
    np.testing.assert_array_equal(h["point_list"].view(np.uint32), o["point_list"])
    np.testing.assert_array_equal(h["keys_sorted"].view(np.uint64), o["keys_sorted"])
    np.testing.assert_array_equal(h["ranges"].view(np.uint32), o["ranges"])
    # (a') the radix partition on the tile bits (the path of images with > 16384 tiles, where the LDS histogram of the
    # direct tile binning does not fit) instead of the direct tile binning: same lists
    for cc in (case, U.make_case(40_000, 250, 190, 5, deg=1, sigma0=(0.02, 0.003))):
        oo, _ = U.run_oracle(cc, "f32")
        R.K.FORCE_RADIX_PARTITION = True
        try:
            h, _ = U.run_hip(cc)
        finally:
            R.K.FORCE_RADIX_PARTITION = False
        np.testing.assert_array_equal(h["point_list"].view(np.uint32), oo["point_list"])
        np.testing.assert_array_equal(h["keys_sorted"].view(np.uint64), oo["keys_sorted"])
        np.testing.assert_array_equal(h["ranges"].view(np.uint32), oo["ranges"])
        assert U.outlier_fraction(h["color"], oo["color"], 1e-4, 1e-5) < 1e-4
    # (b) 16 tiles, ~15k entries per tile (> LDS capacity of ~9.7k)
    case = U.make_case(60_000, 64, 64, 23, deg=0, sigma0=(0.03,))
    o, _ = U.run_oracle(case, "f32")
    assert (o["ranges"][:, 1] - o["ranges"][:, 0]).max() > 10_000
    h, _ = U.run_hip(case)
    np.testing.assert_array_equal(h["point_list"].view(np.uint32), o["point_list"])
    np.testing.assert_array_equal(h["keys_sorted"].view(np.uint64), o["keys_sorted"])
    assert U.outlier_fraction(h["color"], o["color"], 1e-4, 1e-5) < 1e-4


def test_equal_depth_ties_keep_gaussian_index_order(oracle_built):
    """Many Gaussians with IDENTICAL depth bits in one tile: the sorted order must be ascending
    Gaussian index (what the reference's stable sort of emission order yields)."""
    case = U.make_case(3_000, 64, 64, 5, deg=0, sigma0=(0.02,))
    # put everything on a plane of constant view depth: project the centres onto the plane through the
    # origin orthogonal to the camera axis
    axis = case["view"][:3, 2].clone()
    axis = axis / axis.norm()
    m = case["means3D"]
    case["means3D"] = (m - (m @ axis)[:, None] * axis[None, :] * 1.0).contiguous()
    o, _ = U.run_oracle(case, "f32")
    keys = o["keys_sorted"]
    assert (keys[1:] == keys[:-1]).mean() > 0.01  # the case really has ties
    h, _ = U.run_hip(case)
    np.testing.assert_array_equal(h["point_list"].view(np.uint32), o["point_list"])
    np.testing.assert_array_equal(h["keys_sorted"].view(np.uint64), o["keys_sorted"])


def test_screenspace_absgrad_entry_matches_vjp_through_the_reference_sequence():
    """Renderer.screenspace_absgrad (mean2D-only K7, no K8/K9) == vjp of the MSE over 4 views w.r.t. the (N,4)
    carrier through render_img with torch activations — the computation of network.py:843-878."""
    from torch.autograd.functional import vjp

    from generativedensification_amd.camera import orbit_cameras
    from generativedensification_amd.renderer import Renderer
    from generativedensification_amd.synthetic import make_scene, make_targets

    dev = torch.device("cuda:0")
    n, h, w, V = 40_000, 224, 192, 4
    sc = {k: v.to(dev) for k, v in make_scene(n, 91, sh_degree=1, sigma0=(0.0052, 0.01)).items()}
    cams = orbit_cameras(V, w, h, device=dev)
    gt = make_targets(V, h, w, 91).to(dev)
    bgs = [torch.tensor([b, b, b], device=dev) for b in (1.0, 0.5, 0.0, 1.0)]
    r_ref = Renderer(sh_degree=1, fused=False)

    def fn(ssp):
        imgs = []
        for c, b in zip(cams, bgs):
            r_ref.set_bg_color(b)
            imgs.append(r_ref.render_img(c, None, sc["centers"], sc["shs"], sc["opacity"], sc["scales"],
                                         sc["rotations"], dev, screenspace_points=ssp)["image"])
        return ((torch.stack(imgs) - gt) ** 2).mean()

    loss_ref, grad_ref = vjp(fn, torch.zeros(n, 4, device=dev))
    loss, grad = Renderer(sh_degree=1).screenspace_absgrad(cams, bgs, gt, sc["centers"], sc["shs"], sc["opacity"],
                                                           sc["scales"], sc["rotations"], dev)
    assert abs(float(loss) - float(loss_ref)) <= 1e-5 * abs(float(loss_ref))
    assert grad.shape == (n, 4) and float(grad[:, 2:].min()) >= 0
    assert U.rel_inf(grad.cpu().numpy(), grad_ref.cpu().numpy()) < 1e-4
    # what the caller consumes: the norm of the abs channels, then top-k (network.py:876-893)
    k = 12_000
    sel = torch.topk(grad[:, 2:4].norm(dim=-1), k).indices
    sel_ref = torch.topk(grad_ref[:, 2:4].norm(dim=-1), k).indices
    assert len(set(sel.tolist()) & set(sel_ref.tolist())) >= k - 5
    # ... which the entry point also returns directly (topk=)
    loss2, grad2, idx = Renderer(sh_degree=1).screenspace_absgrad(cams, bgs, gt, sc["centers"], sc["shs"], sc["opacity"],
                                                                  sc["scales"], sc["rotations"], dev, topk=k)
    assert idx.shape == (k,) and len(set(idx.tolist()) & set(sel_ref.tolist())) >= k - 5
    assert U.rel_inf(grad2.cpu().numpy(), grad_ref.cpu().numpy()) < 1e-4


def test_fused_view_loss_matches_torch_loss_value_and_gradients():
    """losses.view_loss_fused (one HIP reduction forward, one elementwise kernel backward) == synthetic.view_loss on
    the clamped dict (renderer.py:261 clamp + loss.py:37-38 MSE + the §8d depth/alpha means): value to 1e-6
    relative (fp32 reduction order differs), image-space gradients elementwise to 1e-6, Gaussian gradients to 1e-4."""
    from generativedensification_amd.camera import orbit_cameras
    from generativedensification_amd.losses import view_loss_fused
    from generativedensification_amd.renderer import Renderer
    from generativedensification_amd.synthetic import make_scene, make_targets, view_loss

    dev = torch.device("cuda:0")
    n, h, w, V = 20_000, 144, 176, 2
    sc = make_scene(n, 91, sh_degree=3, sigma0=(0.0052, 0.02))
    sc["shs"][:, 0] *= 3.0   # push a good share of pixels outside [0,1] so the clamp mask matters
    cams = orbit_cameras(V, w, h, device=dev)
    tg = make_targets(V, h, w, 91).to(dev)
    tg_chw = tg.permute(0, 3, 1, 2).contiguous()
    r = Renderer(sh_degree=3, fused=True)

    def run(fused_loss):
        leaves = {k: v.to(dev).clone().requires_grad_(True) for k, v in sc.items()}
        args = (cams, None, leaves["centers"], leaves["shs"], leaves["opacity"], leaves["scales"], leaves["rotations"], dev)
        if fused_loss:
            outs = r.render_views(*args, raw=True)
            img = [o["color"] for o in outs]
            lv = torch.stack([view_loss_fused(o["color"], o["depth"], o["alpha"], tg_chw[j]) for j, o in enumerate(outs)])
        else:
            outs = r.render_views(*args)
            img = None
            lv = torch.stack([view_loss(o, tg[j]) for j, o in enumerate(outs)])
        # non-unit upstream gradients exercise the device-scalar g of the backward kernel
        wts = torch.tensor([0.7, 1.9], device=dev)
        grads = torch.autograd.grad((lv * wts).sum(), list(leaves.values()))
        return lv.detach().cpu().numpy(), {k: g_.cpu().numpy() for k, g_ in zip(leaves, grads)}, img

    l_ref, g_ref, _ = run(False)
    l_fus, g_fus, img = run(True)
    frac_out = float(((img[0] < 0) | (img[0] > 1)).float().mean())
    assert 0.02 < frac_out < 0.98, frac_out
    np.testing.assert_allclose(l_fus, l_ref, rtol=2e-6)
    for k in g_ref:
        assert U.rel_inf(g_fus[k], g_ref[k]) < 1e-4, k

    # image-space gradients of the loss kernel alone against torch autograd
    c = (torch.rand(3, h, w, device=dev) * 1.6 - 0.3).requires_grad_(True)
    d = torch.rand(1, h, w, device=dev).requires_grad_(True)
    a = torch.rand(1, h, w, device=dev).requires_grad_(True)
    lf = view_loss_fused(c, d, a, tg_chw[0])
    gf = torch.autograd.grad(lf * 3.0, [c, d, a])
    lt = view_loss({"image": c.clamp(0, 1).permute(1, 2, 0), "depth": d.permute(1, 2, 0), "acc_map": a.squeeze(0)}, tg[0])
    gt = torch.autograd.grad(lt * 3.0, [c, d, a])
    assert abs(lf.item() - lt.item()) <= 2e-6 * abs(lt.item())
    for x, y in zip(gf, gt):
        torch.testing.assert_close(x, y, rtol=1e-6, atol=1e-12)


@pytest.mark.parametrize("V", [3, 9])
def test_loss_folded_into_k6_k7_matches_the_torch_loss_on_render_views(V):
    """Renderer.render_views_loss (K6 epilogue accumulates the loss, K7 prologue forms dL/dpixel) == synthetic.view_loss
    on render_views' dicts + autograd: values to 2e-6, Gaussian gradients to 1e-4, per-view bg colours, non-unit
    upstream gradients, a good share of pixels outside [0,1] (clamp mask)."""
    from generativedensification_amd.camera import orbit_cameras
    from generativedensification_amd.renderer import Renderer
    from generativedensification_amd.synthetic import make_scene, make_targets, view_loss

    dev = torch.device("cuda:0")
    n, h, w = 25_000, 150, 200
    sc = make_scene(n, 93, sh_degree=3, sigma0=(0.0052, 0.02))
    sc["shs"][:, 0] *= 3.0
    cams = orbit_cameras(V, w, h, device=dev)
    tg = make_targets(V, h, w, 93).to(dev)
    tg_chw = tg.permute(0, 3, 1, 2).contiguous()
    three = ([1.0, 1.0, 1.0], [0.5, 0.5, 0.5], [0.0, 0.0, 0.0])
    bgs = [torch.tensor(three[j % 3], device=dev) for j in range(V)]
    wts = torch.tensor([0.7, 1.9, 1.0, 0.4, 1.3, 2.2, 0.9, 1.6, 0.5, 1.1][:V], device=dev)
    r = Renderer(sh_degree=3, fused=True)

    def run(folded):
        leaves = {k: v.to(dev).clone().requires_grad_(True) for k, v in sc.items()}
        ssp = torch.zeros(n, 4, device=dev, requires_grad=True)
        args = (leaves["centers"], leaves["shs"], leaves["opacity"], leaves["scales"], leaves["rotations"], dev)
        if folded:
            lv = r.render_views_loss(cams, bgs, tg_chw, *args, screenspace_points=ssp)
        else:
            outs = r.render_views(cams, bgs, *args, screenspace_points=ssp)
            lv = torch.stack([view_loss(o, tg[j]) for j, o in enumerate(outs)])
        grads = torch.autograd.grad((lv * wts).sum(), list(leaves.values()) + [ssp])
        return lv.detach().cpu().numpy(), {k: g_.cpu().numpy() for k, g_ in zip(list(leaves) + ["ssp"], grads)}

    l_ref, g_ref = run(False)
    l_fold, g_fold = run(True)
    np.testing.assert_allclose(l_fold, l_ref, rtol=2e-6)
    for k in g_ref:
        assert U.rel_inf(g_fold[k], g_ref[k]) < 1e-4, k
    assert g_fold["ssp"].shape == (n, 4) and (g_fold["ssp"][:, 2:] >= 0).all()


@pytest.mark.parametrize("H,W", [(1080, 1920), (4112, 4100)])
def test_large_images_tile_ids_beyond_12_bits(oracle_built, H, W):
    """8 160 tiles (13 tile bits) and 66 306 tiles (17 bits: a third partition pass, 260 chunks in the tile-order /
    cut-list scan): sorted list, ranges and image against the oracle."""
    case = U.make_case(1500, H, W, 61, deg=1, sigma0=(0.01, 0.08))
    hip, _ = U.run_hip(case, U.rand_grads(case))
    ora, _ = U.run_oracle(case, "f32", nthreads=8)
    for k in ("radii", "rect", "tiles_touched", "ranges", "point_list"):
        np.testing.assert_array_equal(np.asarray(hip[k]).astype(np.asarray(ora[k]).dtype).reshape(np.asarray(ora[k]).shape), ora[k], err_msg=k)
    assert hip["num_rendered"] == ora["num_rendered"] and hip["num_rendered"] > 50_000
    assert U.outlier_fraction(hip["color"], ora["color"], 1e-4, 1e-4) < 1e-4
    assert float((hip["n_contrib"].astype(np.int64) != ora["n_contrib"]).mean()) < 1e-4


@pytest.mark.parametrize("H,W", [(1, 1), (5, 37), (16, 16), (17, 300)])
def test_tiny_and_odd_image_sizes_both_paths(oracle_built, H, W):
    """Degenerate image shapes (single pixel, one partial tile, a 19-tile strip) through both rasterizers."""
    case = U.make_case(300, H, W, 31, deg=2, sigma0=(0.05, 0.3))
    grads = U.rand_grads(case)
    hip, hg = U.run_hip(case, grads)
    ora, _ = U.run_oracle(case, "f32")
    _, g64 = U.run_oracle(case, "f64", grads)
    for k in ("radii", "rect", "tiles_touched", "point_list", "ranges"):
        np.testing.assert_array_equal(np.asarray(hip[k]).astype(np.asarray(ora[k]).dtype).reshape(np.asarray(ora[k]).shape), ora[k], err_msg=k)
    assert U.outlier_fraction(hip["color"], ora["color"], 1e-4, 1e-4) < 2e-3
    for k in ("means3D", "shs", "opacities", "scales", "rotations"):
        assert U.rel_inf(hg[k].reshape(g64[k].shape), g64[k]) < 2e-4, k
    scase = U.make_surfel_case(300, H, W, 31, deg=2, sigma0=(0.05, 0.3))
    sg = U.rand_surfel_grads(scase)
    ship, shg = U.run_surfel_hip(scase, sg)
    sora, sg32 = U.run_surfel_oracle(scase, "f32", sg)
    _, sg64 = U.run_surfel_oracle(scase, "f64", sg)
    for k in ("radii", "rect", "tiles_touched", "point_list", "ranges"):
        np.testing.assert_array_equal(np.asarray(ship[k]).astype(np.asarray(sora[k]).dtype).reshape(np.asarray(sora[k]).shape), sora[k], err_msg=k)
    assert U.outlier_fraction(ship["color"], sora["color"], 1e-4, 1e-4) < 2e-3
    U.assert_grads_surfel(shg, sg64, sg32, ("means3D", "shs", "opacities", "scales", "rotations"), "surfel tiny")


@pytest.mark.parametrize("n,band", [(30_000, 0.7), (70_000, 0.0), (50_000, 1.0), (90_000, 1.0)])
def test_long_tile_lists_bucket_and_band_cases(oracle_built, n, band):
    """Tile lists of 30k-70k entries (far beyond the 16384-entry LDS capacity of the per-tile depth sort).  `band` = share
    of the Gaussians squeezed into a depth band ~1e-5 wide: 0.7 puts > 16384 entries into ONE of the 256 top-digit buckets
    (finished by the global LSD passes) next to ordinary buckets (sorted in LDS chunks); 1.0 is a list whose whole depth
    span is a few hundred float steps; 0.0 is the plain spread-out case.  Sorted list and ranges bit-exact."""
    case = U.make_case(n, 48, 48, 41, deg=0, sigma0=(0.01,))
    m = (case["means3D"] * 0.02).contiguous()
    nb = int(band * n)
    if nb:
        a = case["view"][:3, 2] / case["view"][:3, 2].norm()          # view axis (depth = [p,1] @ view[:,2])
        m[:nb] = m[:nb] - (1.0 - 1e-4) * (m[:nb] @ a)[:, None] * a    # squeeze the band along it
        m[5:nb:11] = m[5]                                             # exact ties inside the band
    case["means3D"] = m
    case["opacities"] = (case["opacities"] * 0.01).contiguous()
    hip, _ = U.run_hip(case, U.rand_grads(case))
    ora, _ = U.run_oracle(case, "f32")
    lens = ora["ranges"][:, 1].astype(np.int64) - ora["ranges"][:, 0].astype(np.int64)
    assert lens.max() > 3 * 8192
    np.testing.assert_array_equal(hip["ranges"], ora["ranges"])
    np.testing.assert_array_equal(hip["point_list"], ora["point_list"])
    assert U.outlier_fraction(hip["color"], ora["color"], 1e-3, 1e-4) < 1e-3


def test_parity_risk_switches_r1_and_r4(oracle_built):
    """the fork's source is unavailable, so two of its possible conventions are switchable.
    R1 (rasterizer.DEPTH_TO_MEAN / GDR_IN_NO_DEPTH_TO_MEAN): dL/d(depth image) does / does not move the centres —
    HIP == oracle in both settings, and the settings differ.  R4 (Renderer(depth_mode=...)): depth = sum w z (default)
    or sum w z / sum w."""
    from generativedensification_amd import rasterizer as R
    from generativedensification_amd.camera import orbit_cameras
    from generativedensification_amd.renderer import Renderer
    from generativedensification_amd.synthetic import make_scene

    case = U.make_case(4000, 96, 112, 51, deg=2, sigma0=(0.02, 0.05))
    grads = U.rand_grads(case)
    from oracle.gdr_oracle import Oracle
    o = Oracle("f64", nthreads=8)
    ctx = o.forward(U._np(case["means3D"]), U._np(case["opacities"]), U.settings_np(case), shs=U._np(case["shs"]),
                    scales=U._np(case["scales"]), rotations=U._np(case["rotations"]))
    res = {}
    try:
        for on in (True, False):
            R.DEPTH_TO_MEAN = on
            _, hg = U.run_hip(case, grads)
            g64 = o.backward(ctx, U._np(grads[0]), U._np(grads[1]), U._np(grads[2]), depth_to_mean=on)
            res[on] = hg["means3D"]
            assert U.rel_inf(hg["means3D"].reshape(g64["means3D"].shape), g64["means3D"]) < 1e-4, on
            for k in ("opacities", "scales", "rotations"):
                assert U.rel_inf(hg[k].reshape(g64[k].shape), g64[k]) < 1e-4, (on, k)
    finally:
        R.DEPTH_TO_MEAN = True
    assert U.rel_inf(res[False], res[True]) > 1e-2      # the depth path is a real part of the default gradient

    dev = torch.device("cuda:0")
    sc = {k: v.to(dev) for k, v in make_scene(5000, 9, sh_degree=1, sigma0=(0.02,)).items()}
    cam = orbit_cameras(1, 96, 80, device=dev)[0]
    args = (cam, None, sc["centers"], sc["shs"], sc["opacity"], sc["scales"], sc["rotations"], dev)
    a = Renderer(sh_degree=1).render_img(*args)
    leaf = sc["centers"].clone().requires_grad_(True)
    b = Renderer(sh_degree=1, depth_mode="normalized").render_img(cam, None, leaf, *args[3:])
    acc = a["acc_map"].unsqueeze(-1)
    torch.testing.assert_close(b["depth"], a["depth"] / acc.clamp_min(1e-10))
    hit = acc > 0.5
    dn = b["depth"].detach()[hit]
    assert float(dn.min()) > 0.5 and float(dn.max()) < 3.5   # metric z of the orbit cameras
    b["depth"].sum().backward()
    assert torch.isfinite(leaf.grad).all() and float(leaf.grad.abs().max()) > 0


def test_cut_tile_lists_give_the_gradients_of_the_uncut_walk(oracle_built):
    """Lists longer than seg_len are cut: K6 saves (T, prefix sums) per pixel at every cut, K7 walks the segments in
    parallel workgroups from those states.  Same case with seg_len = 2048 / 4096 / off: identical forward (bit for bit),
    gradients equal to the uncut walk's within float-summation noise and to the f64 oracle within tolerance; the
    tables K6 filled have the expected number of rows."""
    from generativedensification_amd import rasterizer as R

    case = U.make_case(40_000, 64, 48, 43, deg=1, sigma0=(0.003,))
    case["means3D"] = (case["means3D"] * 0.3).contiguous()             # two tiles with 25k / 31k entries
    case["opacities"] = (case["opacities"] * 0.05).contiguous()        # transmittance stays alive: 230 pixels whose
                                                                        # last contributor lies beyond position 8192
    grads = U.rand_grads(case)
    res = {}
    try:
        R.K.DEEP_MAX_BUSY = 0     # (the deep forward of cut tiles is compared with this one below)
        for sl in (0, 2048, 4096):
            R.K.SEG_LEN = sl
            res[sl] = U.run_hip(case, grads)
        R.K.DEEP_MAX_BUSY, R.K.SEG_LEN = None, 2048
        deep = U.run_hip(case, grads)
    finally:
        R.K.SEG_LEN, R.K.DEEP_MAX_BUSY = None, None
    (h0, g0) = res[0]
    if res[2048][0]["seg_len"] == 0:
        pytest.skip("cut lists disabled in this process (GDR_SEG_LEN=0)")
    lens = (h0["ranges"][:, 1].astype(np.int64) - h0["ranges"][:, 0]).clip(min=0)
    assert lens.max() > 3 * 2048
    for sl in (2048, 4096):
        h, g = res[sl]
        assert h["seg_len"] == sl
        nseg = np.where(lens > sl, -(-lens // sl), 0)
        assert int(h["seg_count"][0]) == int((nseg - (nseg > 0)).sum())   # rows: every segment but the last of its tile
        assert int(h["seg_count"][1]) == int(nseg.sum())                   # slots: cuts + end of list
        for k in ("color", "depth", "alpha", "n_contrib", "final_T"):   # the forward walk itself is unchanged by the cuts
            np.testing.assert_array_equal(h[k], h0[k])
        for k in ("means3D", "means2D", "shs", "opacities", "scales", "rotations"):
            assert U.rel_inf(g[k], g0[k]) < 2e-5, (sl, k, U.rel_inf(g[k], g0[k]))
    assert int(h0["seg_count"][0]) == 0 or h0["seg_len"] == 0
    # "deep" forward of the cut tiles (two busy tiles here: 16 pixels per wave, four list entries per pixel and iteration):
    # the transmittance chain is the standard kernel's operation for operation -> identical T, contributor counts and stop
    # decisions; the colour / depth / coverage sums are four partial sums per pixel -> equal up to summation order
    hd, gd = deep
    assert int(hd["seg_count"][2]) == 1 and int(res[2048][0]["seg_count"][2]) == 0
    for k in ("n_contrib", "final_T"):
        np.testing.assert_array_equal(hd[k], h0[k])
    for k in ("color", "depth", "alpha"):
        assert U.rel_inf(hd[k], h0[k]) < 2e-6, k
    for k in ("means3D", "means2D", "shs", "opacities", "scales", "rotations"):
        assert U.rel_inf(gd[k], g0[k]) < 2e-5, (k, U.rel_inf(gd[k], g0[k]))
    _, g64 = U.run_oracle(case, "f64", grads, nthreads=8)
    for sl in (0, 2048, 4096):
        for k in ("means3D", "opacities", "scales", "rotations", "shs"):
            assert U.rel_inf(res[sl][1][k].reshape(g64[k].shape), g64[k]) < 5e-4, (sl, k)


def test_one_tile_with_a_very_long_list_takes_the_global_sort_path(oracle_built):
    """40k Gaussians stacked on one spot: a single tile list beyond the 16384-entry LDS classes of the per-tile
    depth sort (tile_sort_long's global ping-pong), equal depths included; sorted list bit-exact, image within tolerance."""
    case = U.make_case(40_000, 48, 48, 37, deg=0, sigma0=(0.01,))
    case["means3D"] = (case["means3D"] * 0.02).contiguous()          # all inside one or two tiles at the image centre
    case["means3D"][::7] = case["means3D"][0]                         # exact depth ties
    case["opacities"] = (case["opacities"] * 0.02).contiguous()       # keep transmittance alive through the long list
    grads = U.rand_grads(case)
    hip, hg = U.run_hip(case, grads)
    ora, _ = U.run_oracle(case, "f32")
    lens = ora["ranges"][:, 1].astype(np.int64) - ora["ranges"][:, 0].astype(np.int64)
    assert lens.max() > 16384   # GDR_TSORT_LARGE (gdr_common.h): beyond the long class LDS capacity -> the TOP/global route
    np.testing.assert_array_equal(hip["point_list"], ora["point_list"])
    np.testing.assert_array_equal(hip["ranges"], ora["ranges"])
    assert U.outlier_fraction(hip["color"], ora["color"], 1e-3, 1e-4) < 1e-3
    assert float((hip["n_contrib"].astype(np.int64) != ora["n_contrib"]).mean()) < 1e-3
    _, g64 = U.run_oracle(case, "f64", grads, nthreads=8)
    for k in ("means3D", "opacities", "scales", "rotations"):
        assert U.rel_inf(hg[k].reshape(g64[k].shape), g64[k]) < 5e-4, k
