"""GPU: TSDF fusion and marching cubes (csrc/tsdf.hip through generativedensification_amd.mesh) against the numpy
restatement (tests/tsdf_ref.py) — same blocks and view masks, bit-equal voxels, identical triangles and vertices, same
cluster filter —, the analytic sphere at the reference's setting (48 views of 512^2, the AABB of configs/infer.yaml),
bitwise reproducibility, MeshExtractor end to end with the 3DGS and 2DGS renderers, and the errors; then the same
bit-for-bit comparison on the inputs of tests/tsdf_cases.py, which break the symmetries of the kernels' index arithmetic
(an asymmetric camera model, every sampling stride, 1 to 4 mask words, both colour dtypes and colours out of range, objects
far from the origin, clusters past 256 scan tiles, the other camera families and a non-square MeshExtractor run).
tests/test_tsdf_cpu.py shows on mutants of the restatement that those inputs discriminate."""
import glob
import math
import os

import numpy as np
import pytest
import torch

import tsdf_cases as TC
import tsdf_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
INFER_AABB = [-0.5, -0.5, -0.5, 0.5, 0.5, 0.5]
# median | |v| - 0.3 | of the Gaussian-shell meshes (MeshExtractor, 256^2 views).  The analytic sphere at the reference's
# setting gives 7.4e-4 (0.2 voxel); the opaque surface of a shell of sigma = s Gaussians lies ~0.9 s outside its centres
# (measured 1.07e-2 / 1.10e-2 for 2DGS / 3DGS at s = 0.012): the bar is 7.4e-4 + 0.9 s + 2 voxels of slack at s = 0.006
SHELL_SIGMA = 0.006
SHELL_MEDIAN_BAR = 0.0135


def _cameras(n_az, size, family="gobjeverse"):
    return TC.path_cameras(n_az, size, family)


def _to_gpu(views, layout="renderer"):
    """View tuples for TSDFVolume.integrate.  'renderer': depth (H, W, 1) and image (H, W, 3) as permuted views of
    (C, H, W) tensors, the renderer's layouts; 'transposed': depth as the transpose of a (W, H) tensor and colour as a
    permuted view of a (3, W, H) tensor, so that no stride is the dense one."""
    out = []
    for v in views:
        d, c = torch.from_numpy(v["depth"]), torch.from_numpy(v["rgb"])
        if layout == "renderer":
            dt = d[None].to(DEV).permute(1, 2, 0)
            ct = c.permute(2, 0, 1).contiguous().to(DEV).permute(1, 2, 0)
        else:
            dt = d.t().contiguous().to(DEV).t()
            ct = c.permute(2, 1, 0).contiguous().to(DEV).permute(2, 1, 0)
            assert not dt.is_contiguous() and not ct.is_contiguous()
        assert tuple(dt.shape[:2]) == v["depth"].shape and tuple(ct.shape) == v["rgb"].shape
        out.append((dt, ct, v["fx"], v["fy"], v["cx"], v["cy"], torch.from_numpy(np.asarray(v["E"])), v["depth_trunc"]))
    return out


def _views(n_az, size, radius=0.3, seed=0, noise=0.0, holes=False):
    """(GPU view tuples, restatement views) of an analytic sphere with a coloured, noisy depth."""
    views = TC.old_views(n_az, size, radius, seed, noise, holes)
    return _to_gpu(views), TC.ref_views(views)


def _volume(views, voxel, **kw):
    from generativedensification_amd.mesh import TSDFVolume

    vol = TSDFVolume(voxel, 2 * voxel, device=DEV, **kw)
    for v in views:
        vol.integrate(*v)
    return vol


def _assert_volume_equal(vol, ref, n_views):
    blocks, mask, T, Wt, C = ref
    np.testing.assert_array_equal(vol.blocks.cpu().numpy(), blocks)
    bits = vol.block_views.cpu().numpy().view(np.uint32)
    assert bits.shape[1] == (n_views + 31) // 32
    got_mask = np.stack([(bits[:, k // 32] >> (k % 32)) & 1 for k in range(n_views)], 1).astype(bool)
    np.testing.assert_array_equal(got_mask, mask)
    if n_views % 32:   # no bit beyond the last view
        assert not (bits[:, -1] >> (n_views % 32)).any()
    np.testing.assert_array_equal(vol.weight.cpu().numpy(), Wt)
    np.testing.assert_array_equal(vol.tsdf.cpu().numpy(), T)
    np.testing.assert_array_equal(vol.color.cpu().numpy(), C)


def _assert_matches_restatement(gpu, ref, voxel, stride=4, min_blocks=1, min_tris=1):
    """Blocks, view masks, tsdf, weight and colour bit-equal to tsdf_ref.fuse; identical triangles; vertices and colours
    to rtol = 1e-6.  Returns (volume, mesh, restated (vertices, triangles, colours))."""
    vol = _volume(gpu, voxel, depth_sampling_stride=stride)
    mesh = vol.extract_triangle_mesh()
    torch.cuda.synchronize()
    fused = R.fuse(ref, voxel, 2 * voxel, stride=stride)
    blocks, mask, T, Wt, C = fused
    assert len(blocks) >= min_blocks, len(blocks)
    _assert_volume_equal(vol, fused, len(ref))
    v, f, c = R.extract(blocks, T, Wt, C, voxel)
    assert len(f) >= min_tris, len(f)
    np.testing.assert_array_equal(mesh.triangles.cpu().numpy(), f)
    np.testing.assert_allclose(mesh.vertices.cpu().numpy(), v, rtol=1e-6, atol=0)
    np.testing.assert_allclose(mesh.vertex_colors.cpu().numpy(), c, rtol=1e-6, atol=0)
    return vol, mesh, (v, f, c)


def test_gpu_matches_restatement():
    from generativedensification_amd.mesh import crop_to_aabb, keep_largest_clusters, remove_unreferenced_vertices

    voxel = 0.006
    gpu, ref = _views(14, 96, noise=0.003, holes=True)     # 42 views: two mask words
    vol, mesh, (v, f, c) = _assert_matches_restatement(gpu, ref, voxel, min_blocks=100, min_tris=1001)
    assert 100 <= len(vol.blocks) <= 2000, len(vol.blocks)
    # post-processing: a crop that cuts the sphere into pieces, clusters, keep rule, unreferenced vertices
    aabb = [[-0.25, -0.4, -0.4], [0.4, 0.4, 0.22]]
    m = remove_unreferenced_vertices(keep_largest_clusters(crop_to_aabb(mesh, aabb), 10))
    rv, rc, rf = R.postprocess(v, f, c, aabb)
    np.testing.assert_array_equal(m.triangles.cpu().numpy(), rf)
    np.testing.assert_allclose(m.vertices.cpu().numpy(), rv, rtol=1e-6, atol=0)


def test_gpu_clusters_match_scipy():
    from generativedensification_amd.mesh import TriangleMesh, cluster_connected_triangles

    g = np.random.default_rng(5)
    for nv, nf in ((30, 12), (400, 300), (5000, 3000)):
        f = g.integers(0, nv, (nf, 3)).astype(np.int32)
        m = TriangleMesh(torch.zeros(nv, 3, device=DEV), torch.from_numpy(f).to(DEV), torch.zeros(nv, 3, device=DEV))
        label, counts = cluster_connected_triangles(m)
        rl, rc = R.clusters(f, nv)
        np.testing.assert_array_equal(label.cpu().numpy(), rl)
        np.testing.assert_array_equal(counts.cpu().numpy(), rc)


def _reference_setting(size=512):
    """48 views of an analytic sphere of radius 0.3 with the reference's AABB rule: (volume, voxel)."""
    aabb = np.array(INFER_AABB).reshape(2, 3) * 1.1
    centre, radius = aabb.mean(0), np.linalg.norm(aabb[1] - aabb[0]) * 0.5
    voxel = radius / 256
    views = []
    for cam in _cameras(16, size):
        f = size / (2 * math.tan(cam.FoVx / 2))
        d = R.sphere_depth(cam.view_world_transform.double().numpy(), f, f, size / 2, size / 2, size, size, 0.3)
        trunc = float(np.linalg.norm(cam.camera_center.numpy() - centre) + radius)
        views.append((torch.from_numpy(d).to(DEV), torch.full((size, size, 3), 0.5, device=DEV), f, f, size / 2, size / 2,
                      cam.world_view_transform.T, trunc))
    return _volume(views, voxel), voxel, aabb


def test_gpu_analytic_sphere_reference_setting():
    from generativedensification_amd.mesh import crop_to_aabb, keep_largest_clusters, remove_unreferenced_vertices

    vol, voxel, aabb = _reference_setting()
    mesh = remove_unreferenced_vertices(keep_largest_clusters(crop_to_aabb(vol.extract_triangle_mesh(), aabb), 10))
    v, f = mesh.vertices.cpu().numpy(), mesh.triangles.cpu().numpy()
    assert len(f) > 100_000
    r_err, per_edge, outward, n_clusters = R.mesh_checks(v, f, 0.3, voxel)
    lab, counts = R.clusters(f, len(v))
    main = counts.max() / len(f)
    rest = v[f[lab != counts.argmax()]].reshape(-1, 3)
    med = float(np.median(np.abs(np.linalg.norm(v, axis=1) - 0.3)))
    print(f"sphere 48x512^2: blocks={len(vol.blocks)} V={len(v)} F={len(f)} max|r-0.3|={r_err:.3f} voxel "
          f"median={med / voxel:.3f} voxel ({med:.2e}) clusters={n_clusters} main={main:.5f}")
    assert r_err < 1.0 and per_edge <= 2 and outward >= 0.99, (r_err, per_edge, outward)
    # the lowest camera ring of this path is 3.2 degrees below the equator: the bottom pole is seen only at grazing angles
    # and breaks into small fragments there (98.0 % of the triangles are in the main cluster at 512^2, 99.3 % at 256^2);
    # everything else is one cluster
    assert main >= 0.97 and (rest[:, 2] < -0.25).all(), (n_clusters, main, rest[:, 2].max(initial=-1))


def test_gpu_reproducible():
    gpu, _ = _views(16, 128, noise=0.002)
    a = _volume(gpu, 0.008).extract_triangle_mesh()
    b = _volume(gpu, 0.008).extract_triangle_mesh()
    for x, y in zip(a, b):
        assert x.shape == y.shape and torch.equal(x, y)


def _shell(n=60_000, seed=0, sh_degree=0):
    g = torch.Generator().manual_seed(seed)
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    centers = 0.3 * d
    shs = 0.3 * torch.randn(n, (sh_degree + 1) ** 2, 3, generator=g)
    opacity = torch.full((n, 1), 4.0)
    scales = torch.full((n, 3), math.log(SHELL_SIGMA))
    rotations = torch.nn.functional.normalize(torch.randn(n, 4, generator=g), dim=-1)
    mask = torch.rand(n, generator=g) < 0.95          # a partial mask, applied to all five inputs
    return [t.to(DEV) for t in (centers, shs, opacity, scales, rotations)] + [mask.to(DEV)]


@pytest.mark.parametrize("kind", ["3dgs", "2dgs"])
def test_gpu_mesh_extractor_end_to_end(tmp_path, kind):
    from generativedensification_amd.mesh import MeshExtractor, read_mesh

    params = _shell()
    if kind == "3dgs":
        from generativedensification_amd.renderer import Renderer
    else:
        from generativedensification_amd.renderer_2dgs import Renderer
        params[3] = params[3][:, :2].contiguous()
    ex = MeshExtractor(params, Renderer(sh_degree=0, white_background=True), aabb=INFER_AABB)
    path = str(tmp_path / "shell.obj")
    mesh = ex.extract(path, {"dataset_name": "gobjeverse", "img_size": (256, 256)}, device=DEV)
    v = mesh.vertices.cpu().numpy()
    assert len(mesh.triangles) > 10_000
    med = float(np.median(np.abs(np.linalg.norm(v, axis=1) - 0.3)))
    print(f"{kind}: V={len(v)} F={len(mesh.triangles)} median||v|-0.3|={med:.2e} phases={ex.phase_ms}")
    assert med < SHELL_MEDIAN_BAR, med
    rv, rf, _ = read_mesh(path)
    np.testing.assert_array_equal(rf, mesh.triangles.cpu().numpy())
    assert rv.shape == v.shape
    assert set(ex.phase_ms) == {"render", "integrate", "mc", "post"}


def test_gpu_errors():
    from generativedensification_amd.mesh import TSDFVolume

    vol = TSDFVolume(0.01, 0.02, device=DEV)
    E = torch.eye(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vol.integrate(torch.ones(8, 8), torch.zeros(8, 8, 3, device=DEV), 8, 8, 4, 4, E, 3.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vol.integrate(torch.ones(8, 8, device=DEV), torch.zeros(8, 8, 3), 8, 8, 4, 4, E, 3.0)
    with pytest.raises(RuntimeError, match="no view"):
        vol.extract_triangle_mesh()
    gpu, _ = _views(4, 64)
    with pytest.raises(RuntimeError, match="max_blocks"):
        _volume(gpu, 0.005, max_blocks=16).extract_triangle_mesh()
    with pytest.raises(RuntimeError, match="max_cells"):
        _volume(gpu, 0.005, max_cells=64).extract_triangle_mesh()
    # no depth at all: an empty mesh, not an error
    empty = TSDFVolume(0.01, 0.02, device=DEV)
    empty.integrate(torch.zeros(16, 16, device=DEV), torch.zeros(16, 16, 3, device=DEV), 16, 16, 8, 8, E, 3.0)
    m = empty.extract_triangle_mesh()
    assert all(len(t) == 0 for t in m)


# ---- inputs that break the kernels' symmetries (tests/tsdf_cases.py) -------------------------------------------------
def test_gpu_asymmetric_camera_model():
    """B.1: 90 x 131, fy 20 % above fx, the principal point off centre by different amounts on the two axes."""
    cam = TC.ASYM
    assert cam["H"] != cam["W"] and cam["H"] % 4 and cam["W"] % 4 and cam["fy"] >= 1.15 * cam["fx"]
    views = TC.sphere_views(6, seed=1)
    _assert_matches_restatement(_to_gpu(views), TC.ref_views(views), 0.008, min_blocks=100, min_tris=10_000)


@pytest.mark.parametrize("stride", TC.STRIDES)
def test_gpu_sampling_strides(stride):
    """B.2: the sampled grid ceil(H / S) x ceil(W / S) with and without a partial last row and column."""
    views = TC.sphere_views(6, seed=2)
    _assert_matches_restatement(_to_gpu(views), TC.ref_views(views), 0.012, stride=stride, min_blocks=40, min_tris=5000)


@pytest.mark.parametrize("n_views", TC.VIEW_COUNTS)
def test_gpu_view_mask_words(n_views):
    """B.3: 1 to 4 view-mask words, on both sides of every word boundary."""
    views = TC.sphere_views(n_views, cam=TC.SMALL, seed=n_views)
    vol, _, _ = _assert_matches_restatement(_to_gpu(views), TC.ref_views(views), 0.02, min_blocks=20, min_tris=5000)
    assert vol.block_views.shape[1] == (n_views + 31) // 32
    seen = vol.block_views.cpu().numpy().view(np.uint32)
    assert all(((seen[:, k // 32] >> (k % 32)) & 1).any() for k in range(n_views))     # every view touched a block


def test_gpu_colour_staging_float_and_uint8_agree():
    """B.4: float colours (exact 0.0, exact 1.0, all k / 255) and their host floor(rgb * 255) as uint8 give bit-equal
    volumes, both read through transposed, non-contiguous layouts."""
    views = TC.exact_colours(TC.sphere_views(5, seed=4))
    as_u8 = TC.as_uint8(views)
    assert as_u8[0]["rgb"].dtype == np.uint8 and as_u8[0]["rgb"].max() == 255 and as_u8[0]["rgb"].min() == 0
    vf, _, _ = _assert_matches_restatement(_to_gpu(views, "transposed"), TC.ref_views(views), 0.012, min_tris=5000)
    vu, _, _ = _assert_matches_restatement(_to_gpu(as_u8, "transposed"), TC.ref_views(as_u8), 0.012, min_tris=5000)
    for name in ("blocks", "block_views", "tsdf", "weight", "color"):
        assert torch.equal(getattr(vf, name), getattr(vu, name)), name
    assert float(vf.color.max()) == 255.0 and float(vf.color.min()) == 0.0


def test_gpu_colour_staging_out_of_range():
    """B.4: colours above 1, negative, NaN and infinite are truncated, then clipped to 0..255, NaN giving 0 (tsdf_ref.make_view
    states the rule); uint8 views of the same clipped values agree bit for bit."""
    views = TC.wild_colours(TC.sphere_views(5, seed=5), seed=6)
    rgb = np.stack([v["rgb"] for v in views])
    assert np.isnan(rgb).any() and (rgb > 1).any() and (rgb < 0).any() and np.isinf(rgb).any()
    ref = TC.ref_views(views)
    vf, _, _ = _assert_matches_restatement(_to_gpu(views, "transposed"), ref, 0.012, min_tris=5000)
    as_u8 = [dict(v, rgb=r["rgb"]) for v, r in zip(views, ref)]
    vu, _, _ = _assert_matches_restatement(_to_gpu(as_u8, "transposed"), ref, 0.012, min_tris=5000)
    assert torch.equal(vf.color, vu.color)
    assert 0.0 <= float(vf.color.min()) and float(vf.color.max()) <= 255.0 and bool(torch.isfinite(vf.color).all())


@pytest.mark.parametrize("name", list(TC.OFF_ORIGIN))
def test_gpu_off_origin_objects(name):
    """B.5: block coordinates far from 0, all negative, and a block grid with large empty stretches."""
    spheres = TC.OFF_ORIGIN[name]
    views = TC.sphere_views(6, spheres=spheres, seed=7, dists=(1.9, 1.2) if len(spheres) > 1 else (1.6, 0.7))
    vol, mesh, _ = _assert_matches_restatement(_to_gpu(views), TC.ref_views(views), 0.008, min_blocks=60, min_tris=10_000)
    b = vol.blocks.cpu().numpy()
    if name == "far_centre":
        assert b[:, 0].min() > 15 and b[:, 1].max() < -10 and b[:, 2].min() > 5
    elif name == "negative_octant":
        assert b.max() < 0
    else:
        cells = np.prod(b.max(0) - b.min(0) + 1)
        assert len(b) < 0.5 * cells     # the dense cell grid is mostly empty
        lab, counts = R.clusters(mesh.triangles.cpu().numpy(), len(mesh.vertices))
        assert (counts > 2000).sum() >= 2


@pytest.mark.parametrize("name", TC.CLUSTER_CASES)
def test_gpu_clusters_at_scale_and_in_adversarial_order(name):
    """B.6: more than 256 scan tiles, one long chain hooked in random order, many small components, F = 1 and F = 65."""
    from generativedensification_amd.mesh import TriangleMesh, cluster_connected_triangles

    f, nv = TC.cluster_case(name)
    m = TriangleMesh(torch.zeros(nv, 3, device=DEV), torch.from_numpy(f).to(DEV), torch.zeros(nv, 3, device=DEV))
    label, counts = cluster_connected_triangles(m)
    rl, rc = R.clusters(f, nv)
    if name == "strip_200k":
        assert len(rc) == 1
    if name == "pairs":
        assert len(rc) == len(f) // 2 and (rc == 2).all()
    if name == "random_2m":
        assert len(rc) > 1000 and rc.max() > len(f) // 2
    np.testing.assert_array_equal(label.cpu().numpy(), rl)
    np.testing.assert_array_equal(counts.cpu().numpy(), rc)


FIXTURES = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mesh_path_*.npz")))


def test_gpu_fixture_list():
    assert len(FIXTURES) == 5


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[10:-4] for p in FIXTURES])
def test_gpu_camera_families(path):
    """B.7: every recorded mesh-path family (its transform and FoV where the fixture carries them) on a non-square image,
    with the FoV-derived fx != fy of MeshExtractor."""
    views = TC.family_views(path)
    assert abs(views[0]["fx"] / views[0]["fy"] - 1) > 0.15
    _assert_matches_restatement(_to_gpu(views), TC.ref_views(views), 0.02, min_blocks=10, min_tris=5000)


def test_gpu_mesh_extractor_non_square_image(tmp_path):
    """B.7: img_size = (width, height) = (256, 192).  FoVx == FoVy = 0.75 on this family, so fx = 325 and fy = 244: a swap
    of fx / fy or of W / 2 and H / 2 in MeshExtractor.extract, or reading img_size as (height, width), stretches or shifts
    the shell by tens of per cent of its radius, far beyond the bar."""
    from generativedensification_amd.mesh import MeshExtractor
    from generativedensification_amd.renderer import Renderer

    ex = MeshExtractor(_shell(), Renderer(sh_degree=0, white_background=True), aabb=INFER_AABB)
    mesh = ex.extract(str(tmp_path / "shell.obj"), {"dataset_name": "gobjeverse", "img_size": (256, 192)}, device=DEV)
    assert tuple(ex.volume._depth[0].shape) == (192, 256)
    v = mesh.vertices.cpu().numpy()
    assert len(mesh.triangles) > 10_000
    r = np.linalg.norm(v, axis=1)
    med = float(np.median(np.abs(r - 0.3)))
    print(f"non-square: V={len(v)} F={len(mesh.triangles)} median||v|-0.3|={med:.2e}")
    assert med < SHELL_MEDIAN_BAR, med
