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


def test_fixtures_present():
    assert len(FIXTURES) == 5


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[10:-4] for p in FIXTURES])
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
