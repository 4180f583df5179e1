"""The cases of the volume conditioning tests (tests/test_volcond_cpu.py, tests/test_gpu_volcond.py) and their seeded float64
inputs.  The shapes are the smallest at which csrc/volcond.hip can still go wrong: one row and one lane group, rows that are no
multiple of the groups of a workgroup, both pieces-per-lane settings (C <= 512 and above), one row more than a slab of the
parameter gradients (include/gdr.h GDR_VOLCOND_SLAB_ROWS), non-square token maps under intrinsics of a 16 times larger image,
every block size of a 4^3 grid, and more than 16 views.  The module asserts the conditioning of every case on import."""
import numpy as np

import volcond_ref as R

SLAB_ROWS = 32     # include/gdr.h GDR_VOLCOND_SLAB_ROWS (checked against the package in the tests)
EPS = 1e-6


# ---- ray_sh -------------------------------------------------------------------------------------------------------------------

def ray_inputs():
    """37 rays: seeded, with one zero direction, one origin parallel to its direction (zero moment) and one |d| = 1e-20"""
    rng = np.random.default_rng(101)
    rays = np.concatenate([rng.standard_normal((37, 3)) * 1.2, rng.standard_normal((37, 3)) * rng.uniform(0.2, 3.0, (37, 1))], 1)
    rays[5, 3:] = 0.0
    rays[11, :3] = 0.7 * rays[11, 3:]
    rays[23, 3:] = np.array([0.6, 0.0, -0.8]) * 1e-20
    return rays


# ---- mod_layer_norm -----------------------------------------------------------------------------------------------------------

# name: (R, C, affine, layout)
MOD_CASES = {
    "r1_c8": (1, 8, True, "dense"),
    "r67_c24": (67, 24, True, "dense"),
    "r5_c768": (5, 768, True, "dense"),
    "r19_c1024": (19, 1024, True, "dense"),
    "slab_plus_1": (SLAB_ROWS + 1, 8, True, "dense"),
    "strided": (2 * 12, 16, True, "tokens"),      # the (2, 12, C) slice behind a class token, seen as (2, 3, 4, C)
    "no_affine": (9, 40, False, "dense"),
    "constant_row": (6, 24, True, "dense"),
}
CONSTANT_ROW = 2


def mod_inputs(name):
    """x (R, C), shift_scale (R, 2C), weight, bias (or None), grad_out (R, C)"""
    rows, c, affine, _ = MOD_CASES[name]
    rng = np.random.default_rng(sorted(MOD_CASES).index(name) + 7)
    x = rng.standard_normal((rows, c)) * rng.uniform(0.5, 2.0, (rows, 1)) + rng.uniform(-1.0, 1.0, (rows, 1))
    if name == "constant_row":
        x[CONSTANT_ROW] = 0.625
    ss = rng.standard_normal((rows, 2 * c)) * 0.5
    weight = 1.0 + 0.3 * rng.standard_normal(c) if affine else None
    bias = 0.2 * rng.standard_normal(c) if affine else None
    return x, ss, weight, bias, rng.standard_normal((rows, c))


for _name in MOD_CASES:
    _x = mod_inputs(_name)[0]
    _var = _x.var(-1)
    if _name == "constant_row":
        assert _var[CONSTANT_ROW] == 0.0
        _var = np.delete(_var, CONSTANT_ROW)
    assert _var.min() > 0.05, (_name, _var.min())     # no row whose statistics are ill-conditioned by accident


# ---- sample_tokens ------------------------------------------------------------------------------------------------------------

# name: (B, V, (h, w), (img_h, img_w), r, n_group, C, E, views of view_embed, geometry)
SAMPLE_CASES = {
    "b1v1_3x5_g4": (1, 1, (3, 5), (48, 80), 4, 4, 8, 0, 0, "orbit"),
    "b2v3_5x3_g2": (2, 3, (5, 3), (80, 48), 4, 2, 24, 8, 4, "orbit"),
    "b1v4_3x5_g1": (1, 4, (3, 5), (48, 80), 4, 1, 8, 8, 4, "orbit"),
    "b1v3_3x5_g4": (1, 3, (3, 5), (48, 80), 4, 4, 8, 0, 0, "orbit"),
    "b5v4_r2": (5, 4, (5, 3), (80, 48), 2, 2, 8, 0, 0, "orbit"),      # 20 views
    "degenerate": (1, 1, (3, 5), (48, 80), 4, 2, 8, 8, 1, "dyadic"),
}
FOV, RADIUS, ELEVATION, SCENE = 0.75, 1.2, 0.4, 0.5


def grid_points(r):
    """the reference's build_dense_grid: (r^3, 3) cell centres of the +-SCENE cube in (d, h, w) order"""
    a = (np.arange(r) + 0.5) / r * 2 - 1
    return np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3) * SCENE


def orbit_cameras(n, img_hw):
    """w2cs (n, 4, 4), ixts (n, 3, 3): cameras on a circle of RADIUS at ELEVATION looking at the origin (x right, y down, z
    forward), FOV over the longer image side"""
    H, W = img_hw
    w2cs, ixts = np.zeros((n, 4, 4)), np.zeros((n, 3, 3))
    f = 0.5 * max(H, W) / np.tan(0.5 * FOV)
    for i in range(n):
        az = 2 * np.pi * i / n + 0.3
        c = RADIUS * np.array([np.cos(ELEVATION) * np.cos(az), np.sin(ELEVATION), np.cos(ELEVATION) * np.sin(az)])
        fwd = -c / np.linalg.norm(c)
        right = np.cross(fwd, np.array([0.0, 1.0, 0.0]))
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        rot = np.stack([right, down, fwd])
        w2cs[i, :3, :3], w2cs[i, :3, 3], w2cs[i, 3, 3] = rot, -rot @ c, 1.0
        ixts[i] = [[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]]
    return w2cs, ixts


def dyadic_camera(img_hw):
    """one axis-aligned camera at z = 0.125: the grid points of a 4^3 grid with z = 0.125 have a homogeneous depth of exactly 0,
    those with z < 0.125 a negative one"""
    H, W = img_hw
    w2c = np.eye(4)[None].copy()
    w2c[0, 2, 3] = -0.125
    ixt = np.array([[[16.0, 0, W / 2], [0, 16.0, H / 2], [0, 0, 1]]])
    return w2c, ixt


def sample_inputs(name):
    """rows (BV, h, w, C), points, w2cs, ixts, view_embed (1, views, E, 1, 1, 1) or None, grad_cond"""
    B, V, (h, w), img_hw, r, g, C, E, views, geometry = SAMPLE_CASES[name]
    rng = np.random.default_rng(sorted(SAMPLE_CASES).index(name) + 31)
    rows = rng.standard_normal((B * V, h, w, C))
    w2cs, ixts = orbit_cameras(B * V, img_hw) if geometry == "orbit" else dyadic_camera(img_hw)
    ve = rng.standard_normal((1, views, E, 1, 1, 1)) if E else None
    bs = r // g
    grad = rng.standard_normal((B * g ** 3, V * bs ** 3, C + E))
    return rows, grid_points(r), w2cs, ixts, ve, grad


def tap_classes(name):
    """the fractions of (view, point) pairs with all four taps inside the map, some, none"""
    B, V, hw, img_hw = SAMPLE_CASES[name][:4]
    _, points, w2cs, ixts, _, _ = sample_inputs(name)
    inside = R.taps(points, w2cs, ixts, img_hw, hw)[2].sum(-1)
    return float((inside == 4).mean()), float(((inside > 0) & (inside < 4)).mean()), float((inside == 0).mean())


for _name, _case in SAMPLE_CASES.items():
    if _case[-1] == "orbit":
        assert min(tap_classes(_name)) >= 0.10, (_name, tap_classes(_name))
_pts, _w2c, _ixt = grid_points(4), *dyadic_camera((48, 80))
_h2 = (_pts @ _w2c[0, :3, :3].T + _w2c[0, :3, 3]) @ _ixt[0].T
assert (_h2[:, 2] == 0).sum() == 16 and (_h2[:, 2] < 0).sum() == 32 and (_h2[:, 2] > 0).sum() == 16
