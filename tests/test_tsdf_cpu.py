"""CPU: the numpy restatement of the TSDF fusion / marching cubes (tests/tsdf_ref.py) — its case table, and the restated
pipeline on an analytic sphere; the HIP file's table literal; the host-side parts of generativedensification_amd.mesh (keep
rule, AABB crop, unreferenced-vertex removal, .obj / .ply writers, refusal of CPU tensors) and the mesh-extraction camera
path against fixtures recorded from the reference (tests/golden/mesh_path_*.npz, make_golden_meshpath.py)."""
import glob
import math
import os
import re

import numpy as np
import pytest
import torch

import tsdf_cases as TC
import tsdf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_table_uses_exactly_the_sign_change_edges():
    assert len(R.TRI_TABLE) == 256 and R.MAX_TRIS == 5
    assert R.TRI_TABLE[0] == () and R.TRI_TABLE[255] == ()
    for case, tris in enumerate(R.TRI_TABLE):
        neg = [(case >> i) & 1 for i in range(8)]
        crossed = {e for e, (a, b) in enumerate(R.EDGES) if neg[a] != neg[b]}
        used = {e for t in tris for e in t}
        assert used == crossed, case
        # closed surface inside the cube: every interior triangle edge is shared by exactly two triangles
        pairs = {}
        for t in tris:
            for i in range(3):
                k = tuple(sorted((t[i], t[(i + 1) % 3])))
                pairs[k] = pairs.get(k, 0) + 1
        assert all(c <= 2 for c in pairs.values()), case
        # complementary cases give the same surface with the opposite winding
        flipped = {tuple(sorted(t)) for t in R.TRI_TABLE[255 - case]}
        assert {tuple(sorted(t)) for t in tris} == flipped or len(tris) != len(R.TRI_TABLE[255 - case]) or case in (0, 255) \
            or _same_edges(tris, R.TRI_TABLE[255 - case])


def _same_edges(a, b):
    return {e for t in a for e in t} == {e for t in b for e in t}


def test_case_one_points_away_from_the_negative_corner():
    mid = [(R.CORNERS[a] + R.CORNERS[b]) / 2 for a, b in R.EDGES]
    for i in range(8):
        (tri,) = R.TRI_TABLE[1 << i]
        v = [mid[e] for e in tri]
        n = np.cross(v[1] - v[0], v[2] - v[0])
        assert np.dot(n, np.mean(v, 0) - R.CORNERS[i]) > 0, i


def test_hip_table_literal_matches_the_restatement():
    src = open(os.path.join(ROOT, "generativedensification_amd", "csrc", "tsdf.hip")).read()
    body = src.split("c_tri_table[256][16] = {", 1)[1].split("};", 1)[0]
    rows = [[int(x) for x in r.split(",")] for r in re.findall(r"\{([-0-9,\s]+)\}", body)]
    assert len(rows) == 256
    for case, row in enumerate(rows):
        flat = [e for t in R.TRI_TABLE[case] for e in t]
        assert row[:len(flat)] == flat and all(x == -1 for x in row[len(flat):]), case
    offs = re.search(r"c_edge_off\[12\] = \{([^}]*)\}", src).group(1)
    axes = re.search(r"c_edge_axis\[12\] = \{([^}]*)\}", src).group(1)
    assert [int(x) for x in offs.split(",")] == [o[0] | (o[1] << 1) | (o[2] << 2) for o in R.EDGE_OFFSET]
    assert [int(x) for x in axes.split(",")] == list(R.EDGE_AXIS)


def _sphere_views(n_az, size, radius=0.3):
    from generativedensification_amd.mesh import mesh_path_cameras   # (camera.py, re-exported with the mesh path)

    views = []
    for cam in mesh_path_cameras(n_az, {"dataset_name": "gobjeverse", "img_size": (size, size)}):
        f = size / (2 * math.tan(cam.FoVx / 2))
        d = R.sphere_depth(cam.view_world_transform.double().numpy(), f, f, size / 2, size / 2, size, size, radius)
        rgb = np.broadcast_to(np.array([0.25, 0.5, 0.75], np.float32), (size, size, 3))
        views.append(R.make_view(d, rgb, f, f, size / 2, size / 2, cam.world_view_transform.T.numpy(), 10.0))
    return views


def test_restatement_on_an_analytic_sphere():
    voxel = 0.02
    views = _sphere_views(16, 96)
    blocks, mask, T, Wt, C = R.fuse(views, voxel, 2 * voxel)
    assert len(blocks) > 20 and mask.any(0).all()
    v, f, c = R.extract(blocks, T, Wt, C, voxel)
    assert len(f) > 1000
    r_err, per_edge, outward, n_clusters = R.mesh_checks(v, f, 0.3, voxel)
    assert r_err < 1.0 and per_edge <= 2 and outward >= 0.99 and n_clusters == 1, (r_err, per_edge, outward, n_clusters)
    np.testing.assert_array_equal(np.round(c * 255), np.broadcast_to([63, 127, 191], c.shape))   # floor(rgb * 255)
    v2, c2, f2 = R.postprocess(v, f, c, aabb=[[-0.55] * 3, [0.55] * 3])
    assert len(f2) == len(f) and len(v2) == len(v)


def test_keep_rule_with_ties():
    from generativedensification_amd.mesh import keep_cluster_mask

    for counts in ([5], [3, 9, 1], list(range(1, 13)), [7] * 12, [1, 2, 2, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 9],
                   [100] + [2] * 20, []):
        got = keep_cluster_mask(np.array(counts, np.int64))
        np.testing.assert_array_equal(got, R.keep_mask(np.array(counts, np.int64)))
    assert keep_cluster_mask(np.array([7] * 12)).sum() == 12                   # ties keep more than 10 clusters
    assert keep_cluster_mask(torch.tensor(list(range(1, 13)))).sum() == 10      # counts 3..12
    assert keep_cluster_mask(np.array([1, 2, 2, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 9])).sum() == 11


def _random_mesh(seed=0, nv=60, nf=90):
    g = np.random.default_rng(seed)
    v = g.uniform(-1, 1, (nv, 3)).astype(np.float32)
    f = g.integers(0, nv, (nf, 3)).astype(np.int32)
    c = g.uniform(0, 1, (nv, 3)).astype(np.float32)
    return v, f, c


def test_crop_and_unreferenced_vertices_on_cpu_tensors():
    from generativedensification_amd.mesh import TriangleMesh, crop_to_aabb, remove_unreferenced_vertices

    v, f, c = _random_mesh()
    aabb = np.array([[-0.625, -0.75, -0.5], [0.75, 0.625, 0.875]])   # exact in f32
    m = crop_to_aabb(TriangleMesh(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(c)), aabb)
    ref = R.crop(v, f, aabb)
    assert 0 < len(ref) < len(f)
    np.testing.assert_array_equal(m.triangles.numpy(), ref)
    assert m.vertices.data_ptr() == torch.from_numpy(v).data_ptr() or np.array_equal(m.vertices.numpy(), v)
    # a vertex exactly on the box is inside
    v_on = v.copy()
    v_on[f[0]] = aabb[1].astype(np.float32)
    m2 = crop_to_aabb(TriangleMesh(torch.from_numpy(v_on), torch.from_numpy(f[:1]), torch.from_numpy(c)), aabb)
    assert len(m2.triangles) == 1
    r = remove_unreferenced_vertices(m)
    rv, rc, rf = R.remove_unreferenced(v, c, ref)
    np.testing.assert_array_equal(r.vertices.numpy(), rv)
    np.testing.assert_array_equal(r.vertex_colors.numpy(), rc)
    np.testing.assert_array_equal(r.triangles.numpy(), rf)
    assert r.triangles.dtype == torch.int32


@pytest.mark.parametrize("ext", [".obj", ".ply"])
def test_writers_round_trip(tmp_path, ext):
    from generativedensification_amd.mesh import TriangleMesh, read_mesh, write_mesh

    v, f, c = _random_mesh(3)
    path = str(tmp_path / f"m{ext}")
    write_mesh(path, TriangleMesh(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(c)))
    rv, rf, rc = read_mesh(path)
    np.testing.assert_array_equal(rv, v)
    np.testing.assert_array_equal(rf, f)
    if ext == ".obj":
        np.testing.assert_array_equal(rc, c)
        lines = open(path).read().splitlines()
        assert lines[0].startswith("v ") and len(lines[0].split()) == 7 and lines[-1] == "f %d %d %d" % tuple(f[-1] + 1)
    else:
        np.testing.assert_array_equal(rc, np.round(c * 255) / 255)
        assert open(path, "rb").read(60).startswith(b"ply\nformat binary_little_endian 1.0\n")
    # an empty mesh is written, empty, without raising (the reference would fail in its cluster filter)
    e = str(tmp_path / f"e{ext}")
    write_mesh(e, TriangleMesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), torch.zeros(0, 3)))
    ev, ef, ec = read_mesh(e)
    assert ev.shape == (0, 3) and ef.shape == (0, 3) and ec.shape == (0, 3)
    with pytest.raises(ValueError):
        write_mesh(str(tmp_path / "m.stl"), TriangleMesh(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(c)))


def test_product_refuses_cpu_tensors():
    from generativedensification_amd.mesh import TSDFVolume, TriangleMesh, cluster_connected_triangles

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TSDFVolume(0.01, 0.02, device="cpu")
    with pytest.raises(ValueError, match="block_resolution"):
        TSDFVolume(0.01, 0.02, block_resolution=8)
    v, f, c = _random_mesh()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cluster_connected_triangles(TriangleMesh(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(c)))


FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "mesh_path_*.npz")))
# cameras only, fovx = 1.1 and fovy = 0.45 on a 22 x 14 image: PathCamera(c2w, w, h, fovy, fovx, ...) with the two far apart
PATHCAM_FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "pathcam_*.npz")))


def test_fixtures_present():
    assert len(FIXTURES) == 5 and len(PATHCAM_FIXTURES) == 1


@pytest.mark.parametrize("path", FIXTURES + PATHCAM_FIXTURES,
                         ids=[os.path.basename(p)[10:-4] for p in FIXTURES] + [os.path.basename(p)[:-4] for p in PATHCAM_FIXTURES])
def test_mesh_path_cameras_match_the_reference(path):
    from generativedensification_amd.mesh import mesh_path_cameras   # (camera.py, re-exported with the mesh path)

    z = np.load(path)
    data = {"dataset_name": str(z["dataset_name"]), "img_size": tuple(int(x) for x in z["img_size"])}
    sample = {"transform_mats": torch.from_numpy(z["transform_mats"])} if "transform_mats" in z else None
    fov = torch.from_numpy(z["fov"]) if "fov" in z else None
    cams = mesh_path_cameras(int(z["n"]), data, sample, fov)
    assert len(cams) == 48
    for key, fn in (("world_view_transform", lambda c: c.world_view_transform),
                    ("full_proj_transform", lambda c: c.full_proj_transform), ("camera_center", lambda c: c.camera_center),
                    ("fov_xy", lambda c: torch.tensor([float(c.FoVx), float(c.FoVy)])),
                    ("rays", lambda c: c.get_rays()[0])):
        got = np.stack([fn(c).numpy() for c in cams])
        np.testing.assert_allclose(got, z[key], rtol=1e-5, atol=2e-6, err_msg=key)
    assert cams[0].get_rays().shape == (1,) + tuple(z["rays"].shape[1:])


def test_mesh_path_unposed_and_unknown():
    from generativedensification_amd.mesh import mesh_path_cameras   # (camera.py, re-exported with the mesh path)

    with pytest.raises(NotImplementedError):
        mesh_path_cameras(16, {"dataset_name": "unposed", "img_size": (32, 32)})
    with pytest.raises(ValueError):
        mesh_path_cameras(16, {"dataset_name": "nerf", "img_size": (32, 32)})


def test_float_colour_staging_rule():
    """make_view: p = rgb * 255 in fp32, truncated, clipped to 0..255, NaN -> 0; floor(rgb * 255) on [0, 1]."""
    rgb = np.array([0.0, -0.0, 1.0, 254.9 / 255, 0.5, 256 / 255, 1.2, 1e30, np.inf, -0.3, -1e30, -np.inf, np.nan, 1 / 255],
                   np.float32)
    want = [0, 0, 255, 254, 127, 255, 255, 255, 255, 0, 0, 0, 0, int(np.float32(1 / 255) * np.float32(255))]
    v = R.make_view(np.ones((1, 14), np.float32), np.repeat(rgb[None, :, None], 3, 2), 1, 1, 0, 0, np.eye(4), 4.0)
    np.testing.assert_array_equal(v["rgb"][0, :, 0], want)
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    v = R.make_view(np.ones((1, 256), np.float32), np.repeat(k[None, :, None], 3, 2), 1, 1, 0, 0, np.eye(4), 4.0)
    np.testing.assert_array_equal(v["rgb"][0, :, 1], np.floor(k * np.float32(255)).astype(np.uint8))
    u8 = np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, 2)
    np.testing.assert_array_equal(R.make_view(np.ones((1, 256), np.float32), u8, 1, 1, 0, 0, np.eye(4), 4.0)["rgb"], u8)


def test_cluster_cases_have_the_structure_they_are_there_for():
    for name in ("strip_200k", "pairs", "one", "wave_plus_one"):
        f, nv = TC.cluster_case(name)
        assert f.dtype == np.int32 and f.max() < nv
        lab, counts = R.clusters(f, nv)
        assert len(lab) == len(f)
        if name == "strip_200k":
            assert len(counts) == 1 and len(f) == 200_000 and not (np.diff(f[:, 0]) == 1).all()
        if name == "pairs":
            assert len(counts) == 50_000 and (counts == 2).all()
        if name == "one":
            assert counts.tolist() == [1]
        if name == "wave_plus_one":
            assert len(f) == 65


# ---- the inputs of tsdf_cases.py discriminate: mutants of the restatement ---------------------------------------------
# Each mutant is tsdf_ref.fuse with one index wrong, in the way a kernel could be wrong.  On its NEW input (the one
# test_gpu_mesh.py now runs) its blocks, masks or voxels must differ from the true restatement's at all (the GPU test asks
# bit equality); on the OLD input (the builder test_gpu_mesh.py used before: square images, fx == fy, a centred principal
# point, H % 4 == 0) `old_sees` records whether the mutant was visible.
def _swap(views, a, b):
    return [dict(v, **{a: v[b], b: v[a]}) for v in views]


def _h_for_w(views):
    """depth and colour read at v * H + u instead of v * W + u."""
    out = []
    for v in views:
        H, W = v["depth"].shape
        idx = (np.arange(H)[:, None] * H + np.arange(W)[None]) % (H * W)
        out.append(dict(v, depth=v["depth"].reshape(-1)[idx], rgb=v["rgb"].reshape(-1, 3)[idx]))
    return out


def _fuse_mutant(name, views, voxel, stride):
    trunc = 2 * voxel
    if name == "fx_fy_swapped":
        return R.fuse(_swap(views, "fx", "fy"), voxel, trunc, stride=stride)
    if name == "cx_cy_swapped":
        return R.fuse(_swap(views, "cx", "cy"), voxel, trunc, stride=stride)
    if name == "h_for_w":
        return R.fuse(_h_for_w(views), voxel, trunc, stride=stride)
    if name == "partial_sample_dropped":     # sh = H / S, sw = W / S rounded down
        cut = []
        for v in views:
            H, W = v["depth"].shape
            d = v["depth"].copy()
            d[(H // stride) * stride:] = 0
            d[:, (W // stride) * stride:] = 0
            cut.append(dict(v, depth=d))
        blocks, mask = R.allocate(cut, voxel, trunc, stride=stride)
        return (blocks, mask) + R.integrate(views, blocks, mask, voxel, trunc)
    blocks, mask = R.allocate(views, voxel, trunc, stride=stride)
    if name == "mask_bit_in_word_0":         # view k recorded as bit k % 32 of word 0
        folded = np.zeros_like(mask)
        for k in range(mask.shape[1]):
            folded[:, k % 32] |= mask[:, k]
        return (blocks, folded) + R.integrate(views, blocks, folded, voxel, trunc)
    if name == "block_origin_off_by_one":    # the voxels of block b computed from b + (1, 0, 0)
        return (blocks, mask) + R.integrate(views, blocks + np.array([1, 0, 0]), mask, voxel, trunc)
    raise ValueError(name)


def _old_input(n_views=6):
    return TC.ref_views(TC.old_views(n_views // 3, 64, noise=0.003, holes=True)), 0.02, 4


def _new_input(kind):
    if kind == "asym":          # test_gpu_asymmetric_camera_model, test_gpu_sampling_strides[4]
        return TC.ref_views(TC.sphere_views(6, seed=1)), 0.012, 4
    if kind == "views_33":      # test_gpu_view_mask_words[33]
        return TC.ref_views(TC.sphere_views(33, cam=TC.SMALL, seed=33)), 0.02, 4
    if kind == "negative":      # test_gpu_off_origin_objects[negative_octant] (fewer views, coarser voxels)
        return TC.ref_views(TC.sphere_views(4, spheres=TC.OFF_ORIGIN["negative_octant"], seed=7)), 0.012, 4
    raise ValueError(kind)


# mutant -> (the new input that exposes it, the test of test_gpu_mesh.py that runs it, did the old inputs see it?)
TSDF_MUTANTS = {
    "fx_fy_swapped": ("asym", "test_gpu_asymmetric_camera_model", False),
    "cx_cy_swapped": ("asym", "test_gpu_asymmetric_camera_model", False),
    "h_for_w": ("asym", "test_gpu_asymmetric_camera_model", False),
    "partial_sample_dropped": ("asym", "test_gpu_sampling_strides", False),
    # test_gpu_matches_restatement already had 42 views, so a view >= 32 folded into word 0 was visible: the claim is
    # dropped; what is new is 3 and 4 words and V an exact multiple of 32
    "mask_bit_in_word_0": ("views_33", "test_gpu_view_mask_words", True),
    # an origin off by one block moves every voxel, wherever the object is: the old inputs saw it; the new ones add
    # coordinates that are all negative or far from 0
    "block_origin_off_by_one": ("negative", "test_gpu_off_origin_objects", True),
}


def _differs(a, b):
    return any(x.shape != y.shape or not np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", list(TSDF_MUTANTS))
def test_new_inputs_expose_the_mutant_and_the_old_ones_did_not(name):
    import test_gpu_mesh

    kind, gpu_test, old_sees = TSDF_MUTANTS[name]
    assert hasattr(test_gpu_mesh, gpu_test)
    views, voxel, stride = _new_input(kind)
    assert _differs(_fuse_mutant(name, views, voxel, stride), R.fuse(views, voxel, 2 * voxel, stride=stride)), name
    views, voxel, stride = _old_input(42 if name == "mask_bit_in_word_0" else 6)
    assert _differs(_fuse_mutant(name, views, voxel, stride), R.fuse(views, voxel, 2 * voxel, stride=stride)) == old_sees, name
