"""-m gpu: the HIP rasterizers against the oracle under the cameras of tests/camera_cases.py — fovx != fovy in both orders,
W != H in both orders, eyes inside / on the edge of / next to the scene cube looking past its centre, scale_modifier on both
sides of 1: Gaussians in the frustum clamp of the EWA Jacobian (xmul / ymul = 0 in the backward), just behind the near cull,
rects cut by all four image edges.  tests/test_camera_cases_cpu.py shows on the CPU that these cases reach those branches
and that an exchanged tanfovx / tanfovy, an ignored scale_modifier or a wrong xmul / ymul fails the bars used here; the bars
are the existing ones (test_gpu_parity._check_forward, util.assert_image_parity, util.assert_grads, util.assert_grads_surfel)."""
import numpy as np
import pytest
import torch

import camera_cases as CC
import util as U
from test_gpu_parity import _check_forward
from test_gpu_surfel import _check_forward as _check_surfel_forward

pytestmark = pytest.mark.gpu

GRAD_KEYS = ("means3D", "means2D", "shs", "opacities", "scales", "rotations")
PRECOMP_KEYS = ("means3D", "means2D", "colors_precomp", "opacities", "cov3D_precomp")
DEV = "cuda:0"


def _check_lists(o, h):
    assert h["num_rendered"] == o["num_rendered"]
    np.testing.assert_array_equal(h["radii"], o["radii"])
    np.testing.assert_array_equal(h["rect"], o["rect"])
    np.testing.assert_array_equal(h["tiles_touched"].astype(np.uint32), o["tiles_touched"])
    np.testing.assert_array_equal(h["keys_sorted"].view(np.uint64), o["keys_sorted"])
    np.testing.assert_array_equal(h["point_list"].view(np.uint32), o["point_list"])
    np.testing.assert_array_equal(h["ranges"].view(np.uint32), o["ranges"])
    for k in ("depths", "xy", "conic_opacity"):
        np.testing.assert_array_equal(h[k], o[k], err_msg=k)


# ---- (a) single view through the C ABI ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CC.NAMES)
def test_single_view_vs_oracle(oracle_built, name):
    case = CC.make_camera_case(name)
    keys = PRECOMP_KEYS if case["cov3D_precomp"] is not None else GRAD_KEYS
    grads = U.rand_grads(case)
    o, og = U.run_oracle(case, "f32", grads, nthreads=8)
    _, og64 = U.run_oracle(case, "f64", grads, nthreads=8)
    reach = CC.reach(case, o, og["means3D"])
    print(f"[{name}] reach {reach}")
    for b in case["branches"]:
        assert reach[b] >= CC.FLOOR, (name, b)
    h, hg = U.run_hip(case, grads)
    if case["cov3D_precomp"] is None:
        _check_forward(o, h)          # ints, lists, clamp bits and per-Gaussian floats bit-exact, images at 1e-4
    else:
        _check_lists(o, h)
    print(f"[{name}] image parity (n_contrib, final_T, image pixels, psnr) {U.image_parity_counts(h, o)}")
    U.assert_image_parity(h, o, name)
    U.assert_grads(hg, og64, og, keys, name)
    culled = o["radii"] == 0
    assert culled.sum() > 0
    if case["cov3D_precomp"] is None:      # cov3D is stored for culled Gaussians too: a render group's backward reads one
        assert np.abs(h["cov3D"][culled]).max(axis=1).min() > 0     # view's copy for all its views
    for k in keys:
        assert np.isfinite(hg[k]).all(), k
        assert not hg[k][culled].any(), k      # culled (behind the near plane, off screen): exact zeros
    if case["cov3D_precomp"] is not None:
        assert hg["shs"] is None and hg["scales"] is None and hg["rotations"] is None


@pytest.mark.parametrize("name", [n for n in CC.NAMES if n != "near_face"])     # the cases with radii above 100
def test_both_k7_variants_on_large_radii(oracle_built, name):
    from generativedensification_amd import _lib as L

    lib = L.load()
    case = CC.make_camera_case(name)
    keys = PRECOMP_KEYS if case["cov3D_precomp"] is not None else GRAD_KEYS
    grads = U.rand_grads(case)
    o, g32 = U.run_oracle(case, "f32", grads, nthreads=8)
    _, g64 = U.run_oracle(case, "f64", grads, nthreads=8)
    assert o["radii"].max() > 100
    try:
        for mode in (0, 1):
            lib.gdr_k7_tune_override(mode)
            _, hg = U.run_hip(case, grads)
            U.assert_grads(hg, g64, g32, keys, f"{name} k7 variant {mode}")
    finally:
        lib.gdr_k7_tune_override(-1)


def test_forced_sort_paths_on_the_longest_lists(oracle_built):
    """The forced global radix sort and the forced radix partition on the case whose few near Gaussians make the longest
    tile lists: the oracle's lists bit for bit, the images within the parity line."""
    from generativedensification_amd import rasterizer as R

    name = "outside_offaxis"
    case = CC.make_camera_case(name)
    o, _ = U.run_oracle(case, "f32", nthreads=8)
    assert (o["ranges"][:, 1].astype(np.int64) - o["ranges"][:, 0]).max() > 1000
    for flag in ("FORCE_GLOBAL_SORT", "FORCE_RADIX_PARTITION"):
        setattr(R.K, flag, True)
        try:
            h, _ = U.run_hip(case)
        finally:
            setattr(R.K, flag, False)
        _check_forward(o, h)
        U.assert_image_parity(h, o, f"{name} {flag}")


# ---- (e) markVisible ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CC.NAMES)
def test_mark_visible_is_the_near_plane_test(name):
    """K10 == (view-space depth > 0.2), the depth in float64 from the case; no case has a point within 1e-6 of the plane
    (asserted here and on the CPU), so the comparison is exact on every point."""
    from generativedensification_amd.rasterizer import GaussianRasterizer

    case = CC.make_camera_case(name)
    z, _, _ = CC.view_geometry(case)
    assert not (np.abs(z - CC.NEAR_CULL) < 1e-6).any()
    vis = GaussianRasterizer(U.settings_torch(case, torch.device(DEV))).markVisible(case["means3D"].to(DEV))
    assert vis.dtype == torch.bool and vis.shape == (case["N"],)
    want = z > CC.NEAR_CULL
    assert 0 < want.sum() < case["N"] or name == "outside_offaxis"
    np.testing.assert_array_equal(vis.cpu().numpy(), want)


# ---- (b) multi-view K1 / K9 with per-view FOVs ------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [3, 9])       # 9 > GDR_MAX_VIEWS: two launch groups, the second accumulating
def test_multiview_node_with_per_view_fovs_vs_oracle(oracle_built, V):
    """render_views_raw(flags=0) on views that all have their own (fovx, fovy) and bg: per view radii bit-exact and the
    images within the parity line of THAT view's oracle; gradients against the sum of the per-view oracle gradients."""
    from generativedensification_amd import rasterizer as R

    dev = torch.device(DEV)
    _, _, _, cases = CC.make_multiview_set(V)
    names = ("means3D", "shs", "opacities", "scales", "rotations")
    leaves = {k: cases[0][k].to(dev).clone().requires_grad_(True) for k in names}
    ssp = torch.zeros(CC.MV["N"], 4, device=dev, requires_grad=True)
    sets = [U.settings_torch(c, dev) for c in cases]
    colors, radii, depths, alphas = R.render_views_raw(leaves["means3D"], ssp, leaves["shs"], leaves["opacities"],
                                                       leaves["scales"], leaves["rotations"], sets, flags=0)
    loss, g32, g64 = 0.0, None, None
    for v, c in enumerate(cases):
        ups = U.rand_grads(c, seed=100 + v)
        o, a32 = U.run_oracle(c, "f32", ups, nthreads=8)
        _, a64 = U.run_oracle(c, "f64", ups, nthreads=8)
        m = CC.branch_masks(c, o)
        assert int(m["clamp_x"].sum()) >= CC.FLOOR and int(m["clamp_y"].sum()) >= CC.FLOOR
        np.testing.assert_array_equal(radii[v].cpu().numpy(), o["radii"])
        U.assert_rendered_parity(colors[v].detach().cpu().numpy(), depths[v].detach().cpu().numpy(),
                                 alphas[v].detach().cpu().numpy(), o, f"multi-view V={V} view {v}")
        loss = loss + (colors[v] * ups[0].to(dev)).sum() + (depths[v] * ups[1].to(dev)).sum() + (alphas[v] * ups[2].to(dev)).sum()
        if g32 is None:
            g32 = {k: np.array(a32[k], np.float64) for k in GRAD_KEYS}
            g64 = {k: np.array(a64[k], np.float64) for k in GRAD_KEYS}
        else:
            for k in GRAD_KEYS:
                g32[k] += a32[k]
                g64[k] += a64[k]
    got = torch.autograd.grad(loss, list(leaves.values()) + [ssp])
    hg = {k: g.cpu().numpy() for k, g in zip(names + ("means2D",), got)}
    U.assert_grads(hg, g64, g32, GRAD_KEYS, f"multi-view V={V}")


@pytest.mark.parametrize("V", [3, 9])
def test_raw_multiview_entries_equal_the_per_view_sequence_with_per_view_fovs(V):
    """Renderer.render_views / render_views_loss / screenspace_absgrad(topk=) (RAW tensors, activations inside K1) against one
    render_img per view on the same cameras, with the bars of the existing tests of those entries (elem_stats < MAX_OUTSIDE, max-norm < 1e-4)."""
    from generativedensification_amd.renderer import Renderer
    from generativedensification_amd.synthetic import make_targets, view_loss

    dev = torch.device(DEV)
    sc, cams, bgs, _ = CC.make_multiview_set(V, device=dev)
    tg = make_targets(V, CC.MV["H"], CC.MV["W"], 5).to(dev)
    wts = torch.linspace(0.5, 2.0, V, device=dev)
    r = Renderer(sh_degree=CC.MV["deg"])

    def run(entry):
        leaves = {k: v.to(dev).clone().requires_grad_(True) for k, v in sc.items()}
        ssp = torch.zeros(CC.MV["N"], 4, device=dev, requires_grad=True)
        args = (leaves["centers"], leaves["shs"], leaves["opacity"], leaves["scales"], leaves["rotations"], dev)
        if entry == "loss":
            lv = r.render_views_loss(cams, bgs, tg.permute(0, 3, 1, 2).contiguous(), *args, screenspace_points=ssp)
        else:
            if entry == "views":
                outs = r.render_views(cams, bgs, *args, screenspace_points=ssp)
            else:
                outs = []
                for cam, bg in zip(cams, bgs):
                    r.set_bg_color(bg)
                    outs.append(r.render_img(cam, None, *args, screenspace_points=ssp))
            lv = torch.stack([view_loss(o, tg[j]) for j, o in enumerate(outs)])
        grads = torch.autograd.grad((lv * wts).sum(), list(leaves.values()) + [ssp])
        return lv.detach().cpu().numpy(), {k: g.cpu().numpy() for k, g in zip(list(leaves) + ["ssp"], grads)}

    # screenspace_absgrad(topk=): MSE over the views differentiated w.r.t. the carrier only, then the top-k of the abs channels'
    # norm — the bars of test_gpu_parity.py::test_screenspace_absgrad_entry_matches_vjp_through_the_reference_sequence
    from torch.autograd.functional import vjp
    raw = {k: v.to(dev) for k, v in sc.items()}
    r_ref = Renderer(sh_degree=CC.MV["deg"], fused=False)

    def mse_of(ssp):
        imgs = []
        for cam, bg in zip(cams, bgs):
            r_ref.set_bg_color(bg)
            imgs.append(r_ref.render_img(cam, None, raw["centers"], raw["shs"], raw["opacity"], raw["scales"], raw["rotations"], dev,
                                         screenspace_points=ssp)["image"])
        return ((torch.stack(imgs) - tg) ** 2).mean()

    loss_ref, grad_ref = vjp(mse_of, torch.zeros(CC.MV["N"], 4, device=dev))
    n_top = 1500
    loss, grad, idx = r.screenspace_absgrad(cams, bgs, tg, raw["centers"], raw["shs"], raw["opacity"], raw["scales"],
                                            raw["rotations"], dev, topk=n_top)
    assert abs(float(loss) - float(loss_ref)) <= 1e-5 * abs(float(loss_ref))
    assert grad.shape == (CC.MV["N"], 4) and float(grad[:, 2:].min()) >= 0 and float(grad_ref[:, 2:].max()) > 0
    print(f"[raw absgrad V={V}] loss rel {abs(float(loss) - float(loss_ref)) / abs(float(loss_ref)):.2e} grad rel_inf "
          f"{U.rel_inf(grad.cpu().numpy(), grad_ref.cpu().numpy()):.2e}")
    assert U.rel_inf(grad.cpu().numpy(), grad_ref.cpu().numpy()) < 1e-4
    sel_ref = torch.topk(grad_ref[:, 2:4].norm(dim=-1), n_top).indices
    assert idx.shape == (n_top,) and len(set(idx.tolist()) & set(sel_ref.tolist())) >= n_top - 5

    l_ref, g_ref = run("sequence")
    for entry in ("views", "loss"):
        l_got, g_got = run(entry)
        np.testing.assert_allclose(l_got, l_ref, rtol=2e-5, err_msg=entry)
        for k in g_ref:
            out, worst, maxn = U.elem_stats(g_got[k], g_ref[k])
            print(f"[raw {entry} V={V}] {k:10s} outside {out:.2e} worst/tol {worst:.1f} max-norm rel {maxn:.2e}")
            assert out < U.MAX_OUTSIDE and maxn < 1e-4, (entry, k, out, worst, maxn)


# ---- (c) the reference's loop over cameras of differing FOV: the render-group path ----------------------------------------
def _loop(grouped, sc, sets, ups, dev):
    import diff_gaussian_rasterization as D
    from generativedensification_amd import viewgroup as G

    saved = G.GROUP_VIEWS
    G.GROUP_VIEWS = grouped
    try:
        leaves = {k: v.to(dev).clone().requires_grad_(True) for k, v in sc.items()}
        imgs, loss = [], 0.0
        for j, rs in enumerate(sets):
            ssp = torch.zeros(leaves["centers"].shape[0], 4, device=dev, requires_grad=True) + 0
            color, radii, depth, alpha = D.GaussianRasterizer(rs)(
                means3D=leaves["centers"], means2D=ssp, shs=leaves["shs"], opacities=torch.sigmoid(leaves["opacity"]),
                scales=torch.exp(leaves["scales"]), rotations=torch.nn.functional.normalize(leaves["rotations"]))
            imgs.append(torch.cat([color, depth, alpha]).detach().cpu().numpy())
            loss = loss + (color * ups[j][0]).sum() + (depth * ups[j][1]).sum() + (alpha * ups[j][2]).sum()
        loss.backward()
        torch.cuda.synchronize()
    finally:
        G.GROUP_VIEWS = saved
    return imgs, {k: v.grad.cpu().numpy() for k, v in leaves.items()}


@pytest.mark.parametrize("what", ["per_view_fov", "two_scale_modifiers"])
def test_render_groups_with_differing_fov_or_scale_modifier_equal_independent_calls(what):
    """One rasterizer call per view on one Gaussian set, one backward.  per_view_fov: every view its own (fovx, fovy).
    two_scale_modifiers: the same cameras rendered with scale_modifier 1 and 1.6 on the same tensors (two render groups:
    the key holds scale_modifier).  Images bit for bit and gradients within the bar of test_gpu_viewgroup.py of the run
    with grouping off."""
    dev = torch.device(DEV)
    sc, _, _, cases = CC.make_multiview_set(3)
    if what == "two_scale_modifiers":
        cases = [dict(c, scale_modifier=sm) for sm in (1.0, 1.6) for c in cases[:2]]
    sets = [U.settings_torch(c, dev) for c in cases]
    ups = [[g.to(dev) for g in U.rand_grads(c, seed=200 + j)] for j, c in enumerate(cases)]
    i0, g0 = _loop(False, sc, sets, ups, dev)
    i1, g1 = _loop(True, sc, sets, ups, dev)
    for a, b in zip(i1, i0):
        np.testing.assert_array_equal(a, b)
    if what == "two_scale_modifiers":
        assert not np.array_equal(i0[0], i0[2])
    for k in g0:
        out, worst, maxn = U.elem_stats(g1[k], g0[k])
        assert np.abs(g0[k]).max() > 0
        assert out < U.MAX_OUTSIDE and maxn < 1e-4, (what, k, out, worst, maxn)


# ---- (d) the view-reuse probe ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["tanfovy", "scale_modifier"])
def test_a_second_call_that_differs_in_one_camera_scalar_is_not_served_from_the_first(oracle_built, what):
    """The same Gaussians rendered twice in one graph with settings that differ ONLY in tanfovy (then only in scale_modifier):
    no reuse hit, and each image meets its own oracle."""
    import diff_gaussian_rasterization as D
    from generativedensification_amd import viewgroup as G

    dev = torch.device(DEV)
    sc, _, _, cases = CC.make_multiview_set(3)
    first = cases[1]
    second = dict(first, tanfovy=first["tanfovy"] * 1.25) if what == "tanfovy" else dict(first, scale_modifier=1.4)
    G._REUSE_HIST.clear()
    saved = G.REUSE_FORWARD
    G.REUSE_FORWARD = True
    G._REUSE_STATS.update(probes=0, hits=0)
    try:
        leaves = {k: v.to(dev).clone().requires_grad_(True) for k, v in sc.items()}
        outs, loss = [], 0.0
        for c in (first, second):
            act = dict(means3D=leaves["centers"], shs=leaves["shs"], opacities=torch.sigmoid(leaves["opacity"]),
                       scales=torch.exp(leaves["scales"]), rotations=torch.nn.functional.normalize(leaves["rotations"]))
            ssp = torch.zeros(CC.MV["N"], 4, device=dev, requires_grad=True) + 0
            color, radii, depth, alpha = D.GaussianRasterizer(U.settings_torch(c, dev))(means2D=ssp, **act)
            outs.append((c, {k: v.detach().cpu() for k, v in act.items()}, color, radii, depth, alpha))
            loss = loss + color.mean() + depth.mean() + alpha.mean()
        loss.backward()
        torch.cuda.synchronize()
        stats = dict(G._REUSE_STATS)
    finally:
        G.REUSE_FORWARD = saved
    print(f"[reuse {what}] {stats}")
    assert stats["hits"] == 0
    if what == "tanfovy":       # (another scale_modifier is another render group: its first call has nothing to probe)
        assert stats["probes"] >= 1
    assert not torch.equal(outs[0][2], outs[1][2])
    for c, act, color, radii, depth, alpha in outs:
        o, _ = U.run_oracle(dict(c, **act), "f32", nthreads=8)      # the oracle on the activations the GPU computed
        np.testing.assert_array_equal(radii.cpu().numpy(), o["radii"])
        U.assert_rendered_parity(color.detach().cpu().numpy(), depth.detach().cpu().numpy(), alpha.detach().cpu().numpy(), o,
                                 f"reuse {what}")
    assert all(torch.isfinite(v.grad).all() and float(v.grad.abs().max()) > 0 for v in leaves.values())


def test_reuse_probe_compares_every_camera_scalar():
    """gdr_view_reuse_probe called directly (a render group never holds two scale_modifiers, so the loop above cannot reach
    that comparison): candidates that differ from the probing settings in ONE of tanfovx, tanfovy, scale_modifier, with equal
    device tensors in other memory, are no match; the candidate that differs in nothing is, wherever it stands."""
    import ctypes as C
    from generativedensification_amd import _lib as L
    from generativedensification_amd import rasterizer as R

    dev = torch.device(DEV)
    lib = L.load()
    case = CC.make_multiview_set(3)[3][0]
    keep = []
    variants = [dict(case, tanfovx=case["tanfovy"], tanfovy=case["tanfovx"]), dict(case, tanfovx=case["tanfovx"] * 1.01),
                dict(case, tanfovy=case["tanfovy"] * 1.01), dict(case, scale_modifier=1.01), dict(case)]
    with torch.cuda.device(dev):
        now = R._settings_struct(U.settings_torch(case, dev), dev, keep)
        cands = [R._settings_struct(U.settings_torch(c, dev), dev, keep) for c in variants]     # (.to(dev): new memory each)
        scratch = torch.zeros(L.GDR_REUSE_MAX + 1, dtype=torch.int32, device=dev)
        for order, want in (([0, 1, 2, 3], -1), ([0, 1, 2, 3, 4], 4), ([4, 3], 0), ([3], -1), ([2], -1), ([1], -1), ([0], -1)):
            assert len(order) <= L.GDR_REUSE_MAX
            c_arr = (L.GdrSettings * len(order))(*[cands[i] for i in order])
            match, differ = C.c_int32(-2), C.c_uint32(0)
            L.check(lib.gdr_view_reuse_probe(C.byref(now), len(order), c_arr, None, scratch.data_ptr(), C.byref(match),
                                             C.byref(differ), R._stream()), "gdr_view_reuse_probe")
            torch.cuda.synchronize()
            assert match.value == want and differ.value == 0, (order, match.value, want)


# ---- (f) 2DGS -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CC.SURFEL_NAMES)
def test_surfel_single_view_vs_oracle(oracle_built, name):
    case = CC.as_surfel(CC.make_camera_case(name))
    grads = U.rand_surfel_grads(case)
    hip, hg = U.run_surfel_hip(case, grads)
    o32, g32 = U.run_surfel_oracle(case, "f32", grads, nthreads=8)
    _, g64 = U.run_surfel_oracle(case, "f64", grads, nthreads=8)
    assert int((o32["radii"] > 0).sum()) > 1000
    clamped, near = _surfel_reach(case, o32)
    print(f"[surfel {name}] visible {int((o32['radii'] > 0).sum())} clamped {clamped} near band {near}")
    if "clamp_x" in case["branches"] or "clamp_y" in case["branches"]:
        assert clamped >= CC.FLOOR
    if "near" in case["branches"]:
        assert near >= CC.FLOOR
    _check_surfel_forward(hip, o32)
    U.assert_grads_surfel(hg, g64, g32, GRAD_KEYS, f"surfel {name}")
    assert (hg["means2D"][:, 2:] >= 0).all()
    culled = o32["radii"] == 0
    for k in GRAD_KEYS:
        assert not hg[k][culled].any(), k


def _surfel_reach(case, o):
    """Visible surfels of the clamp branches and the near band (the surfel oracle's own radii)."""
    m = CC.branch_masks(case, dict(radii=o["radii"], xy=o["xy"]))
    return int((m["clamp_x"] | m["clamp_y"]).sum()), int(m["near"].sum())


@pytest.mark.parametrize("V", [3, 9])       # 9 > GDR_MAX_VIEWS
def test_surfel_multiview_node_and_render_group_with_per_view_fovs_vs_oracle(oracle_built, V):
    """The 2DGS multi-view node (render_surfel_views_raw, flags = 0) and the surfel render group (one
    diff_surfel_rasterization call per view, one backward) on views that all have their own (fovx, fovy) and bg, with surfels
    that the first view culls at its near plane and a later view sees: per view radii bit-exact and colour against that view's
    oracle, gradients against the SUM of the per-view f32 / f64 oracle gradients with util.assert_grads_surfel at the bar its
    existing multi-view users take (test_gpu_oracle_fullsize.py: sums over the views in another order than the oracle's)."""
    import diff_surfel_rasterization as DS
    from generativedensification_amd import surfel_rasterizer as S
    from generativedensification_amd import viewgroup as VG

    dev = torch.device(DEV)
    cases = [CC.as_surfel(c) for c in CC.make_multiview_set(V)[3]]
    names = ("means3D", "shs", "opacities", "scales", "rotations")
    sets = [U.settings_torch(c, dev) for c in cases]
    ups, outs, g32, g64 = [], [], None, None
    for v, c in enumerate(cases):
        up = U.rand_surfel_grads(c, seed=300 + v)
        o, a32 = U.run_surfel_oracle(c, "f32", up, nthreads=8)
        _, a64 = U.run_surfel_oracle(c, "f64", up, nthreads=8)
        clamped, near = _surfel_reach(c, o)
        assert clamped >= CC.FLOOR and near >= CC.FLOOR, (v, clamped, near)
        ups.append([u.to(dev) for u in up])
        outs.append(o)
        if g32 is None:
            g32 = {k: np.array(a32[k], np.float64) for k in GRAD_KEYS}
            g64 = {k: np.array(a64[k], np.float64) for k in GRAD_KEYS}
        else:
            for k in GRAD_KEYS:
                g32[k] += a32[k]
                g64[k] += a64[k]
    z0 = CC.view_geometry(cases[0])[0]
    assert int(((z0 <= CC.NEAR_CULL) & np.any([o["radii"] > 0 for o in outs[1:]], axis=0)).sum()) >= CC.FLOOR

    def check(colors, allmaps, radii, total, leaves, ssps, what):
        for v, o in enumerate(outs):
            np.testing.assert_array_equal(radii[v].cpu().numpy(), o["radii"])
            assert U.outlier_fraction(colors[v].detach().cpu().numpy(), o["color"], 1e-4, 1e-5) < 1e-4, (what, v)
            for ch in range(6):      # (the bars of test_gpu_oracle_fullsize.py::test_surfel_render_views_backward_vs_oracle)
                assert U.outlier_fraction(allmaps[v][ch].detach().cpu().numpy(), o["allmap"][ch], 1e-4, 1e-4) < 2e-4, (what, v, ch)
        got = torch.autograd.grad(total, list(leaves.values()) + ssps)
        hg = {k: g.cpu().numpy() for k, g in zip(names, got)}
        hg["means2D"] = sum(g.cpu().numpy() for g in got[len(names):])
        U.assert_grads_surfel(hg, g64, g32, GRAD_KEYS, f"surfel {what} V={V}", worst_factor=1.25,
                              max_outside=U.SURFEL_RAW_MAX_OUTSIDE, atol_rel=U.SURFEL_RAW_ATOL_REL)

    leaves = {k: cases[0][k].to(dev).clone().requires_grad_(True) for k in names}
    ssp = torch.zeros(CC.MV["N"], 4, device=dev, requires_grad=True)
    colors, radii, allmaps = S.render_surfel_views_raw(leaves["means3D"], ssp, leaves["shs"], leaves["opacities"], leaves["scales"],
                                                       leaves["rotations"], sets, flags=0)
    total = sum((colors[v] * ups[v][0]).sum() + (allmaps[v] * ups[v][1]).sum() for v in range(V))
    check(colors, allmaps, radii, total, leaves, [ssp], "multi-view node")

    VG.pace().solo_passes = 0
    leaves = {k: cases[0][k].to(dev).clone().requires_grad_(True) for k in names}
    ssps = [torch.zeros(CC.MV["N"], 4, device=dev, requires_grad=True) for _ in range(V)]
    res = [DS.GaussianRasterizer(rs)(means3D=leaves["means3D"], means2D=ssps[v], shs=leaves["shs"], opacities=leaves["opacities"],
                                     scales=leaves["scales"], rotations=leaves["rotations"]) for v, rs in enumerate(sets)]
    assert VG.GROUP_VIEWS and V in VG.live_group_views(), "the V calls did not form ONE surfel render group"   # (a group takes up to 64)
    total = sum((res[v][0] * ups[v][0]).sum() + (res[v][2] * ups[v][1]).sum() for v in range(V))
    check([x[0] for x in res], [x[2] for x in res], [x[1] for x in res], total, leaves, ssps, "render group")
