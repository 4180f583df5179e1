"""GPU: TSDF fusion and marching cubes (csrc/tsdf.hip through generativedensification_amd.mesh) against the numpy
restatement (tests/tsdf_ref.py) — same blocks and view masks, bit-equal voxels, identical triangles and vertices, same
cluster filter —, the analytic sphere at the reference's setting (48 views of 512^2, the AABB of configs/infer.yaml),
bitwise reproducibility, MeshExtractor end to end with the 3DGS and 2DGS renderers, and the errors."""
import math

import numpy as np
import pytest
import torch

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
    from generativedensification_amd.camera import mesh_path_cameras

    return mesh_path_cameras(n_az, {"dataset_name": family, "img_size": (size, size)})


def _views(n_az, size, radius=0.3, seed=0, noise=0.0, holes=False):
    """(GPU view tuples, restatement views) of an analytic sphere with a coloured, noisy depth."""
    g = np.random.default_rng(seed)
    gpu, ref = [], []
    for cam in _cameras(n_az, size):
        f = size / (2 * math.tan(cam.FoVx / 2))
        d = R.sphere_depth(cam.view_world_transform.double().numpy(), f, f, size / 2, size / 2, size, size, radius)
        d = (d * (1 + noise * g.standard_normal(d.shape))).astype(np.float32) * (d > 0)
        if holes:
            d[g.random(d.shape) < 0.01] = np.nan
            d[g.random(d.shape) < 0.01] = -1.0
            d[g.random(d.shape) < 0.01] = 50.0     # beyond depth_trunc
        rgb = g.random((size, size, 3)).astype(np.float32)
        E = cam.world_view_transform.T
        ref.append(R.make_view(d, rgb, f, f, size / 2, size / 2, E.numpy(), 4.0))
        # the renderer's layouts: depth (H, W, 1) and image (H, W, 3) as permuted views of (C, H, W) tensors
        dt = torch.from_numpy(d)[None].to(DEV).permute(1, 2, 0)
        ct = torch.from_numpy(rgb).permute(2, 0, 1).contiguous().to(DEV).permute(1, 2, 0)
        gpu.append((dt, ct, f, f, size / 2, size / 2, E, 4.0))
    return gpu, ref


def _volume(views, voxel, **kw):
    from generativedensification_amd.mesh import TSDFVolume

    vol = TSDFVolume(voxel, 2 * voxel, device=DEV, **kw)
    for v in views:
        vol.integrate(*v)
    return vol


def test_gpu_matches_restatement():
    from generativedensification_amd.mesh import crop_to_aabb, keep_largest_clusters, remove_unreferenced_vertices

    voxel = 0.006
    gpu, ref = _views(14, 96, noise=0.003, holes=True)     # 42 views: two mask words
    vol = _volume(gpu, voxel)
    mesh = vol.extract_triangle_mesh()
    torch.cuda.synchronize()
    blocks, mask, T, Wt, C = R.fuse(ref, voxel, 2 * voxel)
    assert 100 <= len(blocks) <= 2000, len(blocks)
    np.testing.assert_array_equal(vol.blocks.cpu().numpy(), blocks)
    bits = vol.block_views.cpu().numpy().view(np.uint32)
    got_mask = np.stack([(bits[:, k // 32] >> (k % 32)) & 1 for k in range(len(ref))], 1).astype(bool)
    np.testing.assert_array_equal(got_mask, mask)
    np.testing.assert_array_equal(vol.weight.cpu().numpy(), Wt)
    np.testing.assert_array_equal(vol.tsdf.cpu().numpy(), T)
    np.testing.assert_array_equal(vol.color.cpu().numpy(), C)
    v, f, c = R.extract(blocks, T, Wt, C, voxel)
    assert len(f) > 1000
    np.testing.assert_array_equal(mesh.triangles.cpu().numpy(), f)
    np.testing.assert_allclose(mesh.vertices.cpu().numpy(), v, rtol=1e-6, atol=0)
    np.testing.assert_allclose(mesh.vertex_colors.cpu().numpy(), c, rtol=1e-6, atol=0)
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
