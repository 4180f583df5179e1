"""Inputs for the TSDF / marching-cubes / cluster tests that break the symmetries of the kernels' index arithmetic
(csrc/tsdf.hip): shared by tests/test_gpu_mesh.py (HIP against the numpy restatement, bit for bit) and
tests/test_tsdf_cpu.py (mutants of the restatement, which show on the CPU that these inputs tell a wrong index from a right
one and which of them the earlier inputs could not see).

A view is a dict of numpy values: depth (H, W) f32, rgb (H, W, 3) f32 or uint8, fx, fy, cx, cy, E (4x4 f64 world-to-camera,
x right, y down, z forward) and depth_trunc.  `ref_views` stages them for tsdf_ref; test_gpu_mesh.py moves them to the GPU."""
from __future__ import annotations

import math

import numpy as np

import tsdf_ref as R

# B.1: H != W, neither a multiple of the strides 4 or 5 (90 = 22 * 4 + 2, 131 = 32 * 4 + 3 = 26 * 5 + 1 = 43 * 3 + 2), fy 20 %
# above fx, the principal point 5.3 px right of and 3.7 px above the centre
ASYM = dict(H=90, W=131, fx=150.0, fy=180.0, cx=131 / 2 + 5.3, cy=90 / 2 - 3.7)
SMALL = dict(H=40, W=52, fx=60.0, fy=72.0, cx=52 / 2 + 2.3, cy=40 / 2 - 1.7)     # the many-view cases
STRIDES = (1, 3, 4, 5)
VIEW_COUNTS = (31, 32, 33, 64, 65, 100)       # 1 to 4 mask words and both sides of every word boundary
OFF_ORIGIN = {
    "far_centre": [((3.1, -2.3, 1.7), 0.3)],
    "negative_octant": [((-0.9, -0.8, -0.7), 0.3)],
    # two spheres 1.2 apart: blocks of 0.128 leave the volume between them empty, and every block has missing neighbours
    "two_spheres": [((-0.6, 0.1, 0.05), 0.22), ((0.6, -0.15, 0.1), 0.25)],
}


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """4x4 f64 camera-to-world, x right, y down, z forward."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = x, y, z, eye
    return c2w


def orbit(n, centre=(0.0, 0.0, 0.0), dists=(1.6, 0.7)):
    """n camera-to-world matrices around `centre`: a golden-angle spiral in azimuth, elevations in +-50 degrees, the
    distance cycling through `dists` (at 0.7 a sphere of radius 0.3 fills an ASYM image past all four borders, so the last
    partial sampled row and column carry depth; at 1.6 its silhouette is inside the image)."""
    out = []
    for i in range(n):
        az = i * 2.399963
        el = math.radians(50.0) * math.sin(1.7 * i + 0.3)
        d = dists[i % len(dists)]
        eye = np.asarray(centre) + d * np.array([math.cos(az) * math.cos(el), math.sin(az) * math.cos(el), math.sin(el)])
        out.append(look_at(eye, centre))
    return out


def scene_depth(c2w, cam, spheres):
    """Nearest hit of the pixel-centre rays with any of the spheres [(centre, radius)], 0 where all miss."""
    d = None
    for centre, radius in spheres:
        di = R.sphere_depth(c2w, cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["H"], cam["W"], radius, centre=centre)
        d = di if d is None else np.where((di > 0) & ((d == 0) | (di < d)), di, d)
    return d.astype(np.float32)


def sphere_views(n, cam=ASYM, spheres=(((0.0, 0.0, 0.0), 0.3),), seed=0, noise=0.002, dists=(1.6, 0.7), depth_trunc=6.0):
    """n views of the spheres with a noisy depth and a random float colour."""
    g = np.random.default_rng(seed)
    centre = np.mean([c for c, _ in spheres], 0)
    views = []
    for c2w in orbit(n, centre, dists):
        d = scene_depth(c2w, cam, spheres)
        d = (d * (1 + noise * g.standard_normal(d.shape))).astype(np.float32) * (d > 0)
        rgb = g.random((cam["H"], cam["W"], 3)).astype(np.float32)
        views.append(dict(depth=d, rgb=rgb, fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"], E=np.linalg.inv(c2w),
                          depth_trunc=depth_trunc))
    return views


def ref_views(views):
    return [R.make_view(v["depth"], v["rgb"], v["fx"], v["fy"], v["cx"], v["cy"], v["E"], v["depth_trunc"]) for v in views]


# ---- the inputs test_gpu_mesh.py has used from the start ---------------------------------------------------------------
def path_cameras(n_az, size, family="gobjeverse"):
    from generativedensification_amd.camera import mesh_path_cameras

    return mesh_path_cameras(n_az, {"dataset_name": family, "img_size": (size, size)})


def old_views(n_az, size, radius=0.3, seed=0, noise=0.0, holes=False):
    """Square images, fx == fy, the principal point at the centre, an object centred on the origin."""
    g = np.random.default_rng(seed)
    views = []
    for cam in path_cameras(n_az, size):
        f = size / (2 * math.tan(cam.FoVx / 2))
        d = R.sphere_depth(cam.view_world_transform.double().numpy(), f, f, size / 2, size / 2, size, size, radius)
        d = (d * (1 + noise * g.standard_normal(d.shape))).astype(np.float32) * (d > 0)
        if holes:
            d[g.random(d.shape) < 0.01] = np.nan
            d[g.random(d.shape) < 0.01] = -1.0
            d[g.random(d.shape) < 0.01] = 50.0     # beyond depth_trunc
        rgb = g.random((size, size, 3)).astype(np.float32)
        views.append(dict(depth=d, rgb=rgb, fx=f, fy=f, cx=size / 2, cy=size / 2, E=cam.world_view_transform.T.numpy(),
                          depth_trunc=4.0))
    return views


# ---- B.4 colour staging ------------------------------------------------------------------------------------------------
def exact_colours(views):
    """The same views with float colours that hit exact 0.0, exact 1.0 and all 256 values k / 255 (in fp32)."""
    out = []
    for i, v in enumerate(views):
        H, W = v["depth"].shape
        k = (np.arange(H * W * 3, dtype=np.int64) * 7 + 3 * i) % 256
        out.append(dict(v, rgb=(k.astype(np.float32) / np.float32(255)).reshape(H, W, 3)))
    assert out[0]["rgb"].min() == 0.0 and out[0]["rgb"].max() == 1.0 and len(np.unique(out[0]["rgb"])) == 256
    return out


def wild_colours(views, seed=0):
    """Float colours out of range: above 1 (up to 300 / 255 and far beyond), negative, NaN, +-inf, and exact edge values."""
    g = np.random.default_rng(seed)
    out = []
    for v in views:
        rgb = (g.random(v["rgb"].shape) * 1.6 - 0.3).astype(np.float32)
        sel = g.random(rgb.shape)
        rgb[sel < 0.02] = np.nan
        rgb[(sel >= 0.02) & (sel < 0.03)] = np.inf
        rgb[(sel >= 0.03) & (sel < 0.04)] = -np.inf
        rgb[(sel >= 0.04) & (sel < 0.05)] = 1e30
        rgb[(sel >= 0.05) & (sel < 0.06)] = -0.0
        rgb[(sel >= 0.06) & (sel < 0.07)] = 1.0
        rgb[(sel >= 0.07) & (sel < 0.08)] = np.float32(256) / np.float32(255)
        out.append(dict(v, rgb=rgb))
    return out


def as_uint8(views):
    """floor(rgb * 255) in fp32 on the host, for colours in [0, 1]."""
    return [dict(v, rgb=np.floor(v["rgb"] * np.float32(255)).astype(np.uint8)) for v in views]


# ---- B.6 clusters ------------------------------------------------------------------------------------------------------
SCAN_TILE = 4096          # csrc/tsdf.hip: the scan's carry loop runs past 256 tiles


def cluster_case(name, seed=0):
    """(triangles (F, 3) int32, number of vertices)."""
    g = np.random.default_rng(seed)
    if name == "random_2m":          # 513 scan tiles; edges are shared often enough for a giant cluster and many small ones
        nv, nf = 4000, 2_100_000
        assert nf > 256 * SCAN_TILE
        return g.integers(0, nv, (nf, 3)).astype(np.int32), nv
    if name == "strip_200k":         # one strip (i, i + 1, i + 2) in random order: one cluster, a long chain of hooks
        nf = 200_000
        i = np.arange(nf, dtype=np.int32)
        return np.stack([i, i + 1, i + 2], 1)[g.permutation(nf)], nf + 2
    if name == "pairs":              # 50 000 quads of two triangles each, shuffled
        n = 50_000
        q = 4 * np.arange(n, dtype=np.int32)
        f = np.concatenate([np.stack([q, q + 1, q + 2], 1), np.stack([q, q + 2, q + 3], 1)])
        return f[g.permutation(2 * n)], 4 * n
    if name == "one":
        return np.array([[0, 1, 2]], np.int32), 3
    if name == "wave_plus_one":      # 65 triangles: one lane past a wave
        return g.integers(0, 40, (65, 3)).astype(np.int32), 40
    raise ValueError(name)


CLUSTER_CASES = ("random_2m", "strip_200k", "pairs", "one", "wave_plus_one")


# ---- B.7 camera families -----------------------------------------------------------------------------------------------
def family_views(fixture, n_az=3, size=(44, 36), radius=0.3, seed=0):
    """Views of a sphere along the mesh path of one recorded family (tests/golden/mesh_path_*.npz gives the family's name,
    and its transform and FoV where it carries them), on a non-square image (width, height) with the intrinsics
    MeshExtractor derives: fx = W / (2 tan(FoVx / 2)), fy = H / (2 tan(FoVy / 2)).  The sphere sits where the optical axes meet."""
    import torch
    from generativedensification_amd.camera import mesh_path_cameras

    z = np.load(fixture)
    data = {"dataset_name": str(z["dataset_name"]), "img_size": size}
    sample = {"transform_mats": torch.from_numpy(z["transform_mats"])} if "transform_mats" in z else None
    fov = torch.from_numpy(z["fov"]) if "fov" in z else None
    cams = mesh_path_cameras(n_az, data, sample, fov)
    c2ws = [c.view_world_transform.double().numpy() for c in cams]
    A, b = np.zeros((3, 3)), np.zeros(3)
    for M in c2ws:                                    # least-squares meeting point of the optical axes
        P = np.eye(3) - np.outer(M[:3, 2], M[:3, 2])
        A += P
        b += P @ M[:3, 3]
    centre = np.linalg.solve(A, b)
    g = np.random.default_rng(seed)
    W, H = size
    views = []
    for cam, c2w in zip(cams, c2ws):
        assert (cam.image_width, cam.image_height) == (W, H)
        fx, fy = W / (2 * math.tan(cam.FoVx / 2)), H / (2 * math.tan(cam.FoVy / 2))
        d = R.sphere_depth(c2w, fx, fy, W / 2, H / 2, H, W, radius, centre=centre)
        rgb = g.random((H, W, 3)).astype(np.float32)
        views.append(dict(depth=d, rgb=rgb, fx=fx, fy=fy, cx=W / 2, cy=H / 2, E=cam.world_view_transform.T.numpy(),
                          depth_trunc=6.0))
    return views
