"""Deterministic inputs of the image-space kernels' tests (tests/imgloss_ref.py is the arithmetic).  Everything is built in
f64 from a seed and rounded to f32 once; the truth upcasts those f32 numbers.

Smooth surface: a rotated pinhole (fx != fy, principal point off centre by a non-integer amount, origin off every axis) looks
at a tilted plane with low-frequency sines that differ along x and y.  The focal lengths follow the image size, so that two
rays one pixel apart in x and in y stay at an angle well above the conditioning floor (imgloss_ref.COND_FLOOR) at every shape:
where an empty pixel (depth 0, the point falls on the origin) makes both differences of a stencil run along the rays, the
cross product does not vanish by rounding.  About 10 % of the pixels are emptied (all seven channels 0), as isolated pixels
and, in images of 64 px and more, as a few 2x3 blocks, so some stencils have both neighbours of a pair empty
(|a x b| == 0 exactly).

Special values: the pixel with "an overflowing quotient although a != 0" has a = 1e-30 and D = OVERFLOW_D = 1e10; with D = 1
the quotient 1e30 would still be a finite f32.

Colours are a shuffled regular grid on [-0.4, 1.4]: 22 % of the values are clamped on each side at every size, 1x1 included
(a uniform draw on [-0.3, 1.3] would leave 18.75 % per side, below the 20 % the tests ask for)."""
import functools
import math

import torch

SMALL_SHAPES = ((1, 1), (1, 9), (9, 1), (2, 7), (7, 2), (3, 3), (3, 5), (5, 3), (4, 300), (57, 83), (16, 16), (17, 31))
STRIDE_FWD = (3, 174_764)          # 524 292 px: the first shape whose forward reductions (2048 workgroups) stride
STRIDE_BWD = (3, 349_527)          # 1 048 581 px: the first whose view_loss_bwd (4096 workgroups) strides
RATIOS = (0.0, 0.3, 1.0)
TAN_HALF = (0.9, 0.7)              # half field of view along x and y
PRINCIPAL = (0.37, -0.21)          # px off the image centre
ORIGIN = (0.7, -1.3, 0.45)
UP_SCALES = (1.0, 0.3, 2.0, 0.7, 5.0)          # upstream gradients of depth, acc_map, rend_normal, depth_normal, rend_dist

SPECIAL_SHAPE = (9, 11)
# isolated interior pixels (no two share a neighbour): what is placed there
SPECIAL = {(2, 2): "D=+1 a=0", (2, 5): "D=-1 a=0", (2, 8): "D=0 a=0", (5, 2): "med=nan", (5, 5): "med=+inf", (5, 8): "med=-inf",
           (7, 4): "a=1e-30"}
OVERFLOW_D = 1.0e10                # with a = 1e-30 the f32 quotient overflows to +inf although a != 0 (D = 1 would give a finite 1e30)


def rotation():
    """camera-to-world rotation: about an axis off every coordinate axis"""
    axis = torch.tensor([0.3, -0.5, 0.8], dtype=torch.float64)
    axis = axis / axis.norm()
    K = torch.tensor([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]], dtype=torch.float64)
    t = 0.6
    return torch.eye(3, dtype=torch.float64) + math.sin(t) * K + (1 - math.cos(t)) * (K @ K)


def make_rays(H, W):
    """-> rays (H, W, 6) f64 = origin | direction (z = 1 in the camera frame), view (4, 4) f64 with the rays' rotation in
    [:3, :3] and a translation row"""
    C = rotation()
    fx, fy = 0.5 * W / TAN_HALF[0], 0.5 * H / TAN_HALF[1]
    cx, cy = 0.5 * W + PRINCIPAL[0], 0.5 * H + PRINCIPAL[1]
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    d_cam = torch.stack(((xx - cx) / fx, (yy - cy) / fy, torch.ones_like(xx)), dim=-1)
    o = torch.tensor(ORIGIN, dtype=torch.float64)
    rays = torch.cat((o.expand(H, W, 3), d_cam @ C.T), dim=-1)
    view = torch.eye(4, dtype=torch.float64)
    view[:3, :3] = C
    view[3, :3] = -(o @ C)
    return rays, view


def surface(H, W):
    """-> z, median depth (H, W) f64"""
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    u, v = xx / W, yy / H
    z = 2.0 + 0.35 * u - 0.25 * v + 0.06 * torch.sin(2.3 * math.pi * u + 0.4) + 0.05 * torch.sin(1.7 * math.pi * v + 1.1)
    med = z + 0.01 * torch.sin(3.1 * math.pi * u + 5.3 * v + 0.7)
    return z, med


@functools.lru_cache(maxsize=None)
def smooth(H, W, seed=0, holes=True):
    """f32 CPU tensors: color, target (3, H, W); allmap (7, H, W); rays (H, W, 6); view (4, 4); depth, alpha (1, H, W) (the
    3DGS loss's inputs: the un-normalised depth sum and alpha); empty (H, W) bool.  Shared, never modified."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * H + W)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    rays, view = make_rays(H, W)
    z, med = surface(H, W)
    alpha = 0.35 + 0.6 * rnd(H, W)
    am = torch.empty(7, H, W, dtype=torch.float64)
    am[0], am[1], am[5] = alpha * z, alpha, med
    am[2:5] = rnd(3, H, W) - 0.5
    am[6] = 1e-3 * (0.5 + rnd(H, W))
    empty = torch.zeros(H, W, dtype=torch.bool)
    if holes:
        empty = rnd(H, W) < 0.07
        if H >= 2 and W >= 3 and H * W >= 64:
            for _ in range(max(1, (H * W) // 200)):
                y0 = int(torch.randint(0, H - 1, (1,), generator=g))
                x0 = int(torch.randint(0, W - 2, (1,), generator=g))
                empty[y0:y0 + 2, x0:x0 + 3] = True
        am[:, empty] = 0.0
    n = 3 * H * W
    color = ((torch.randperm(n, generator=g).double() + 0.5) / n * 1.8 - 0.4).view(3, H, W)
    out = dict(color=color, target=rnd(3, H, W), allmap=am, rays=rays, view=view, depth=am[0:1].clone(), alpha=am[1:2].clone())
    out = {k: t.float().contiguous() for k, t in out.items()}
    out["empty"] = empty
    return out


def clamp_shares(case):
    """share of the colour values below 0 and above 1"""
    c = case["color"]
    return float((c < 0).double().mean()), float((c > 1).double().mean())


@functools.lru_cache(maxsize=None)
def upstreams(H, W, seed=0):
    """upstream gradients of the five maps, f32, each with its own scale"""
    g = torch.Generator().manual_seed(1000 * seed + 13 * H + W + 5)
    shapes = ((H, W, 1), (H, W), (H, W, 3), (H, W, 3), (H, W))
    return tuple((s * torch.randn(*shape, generator=g, dtype=torch.float64)).float() for s, shape in zip(UP_SCALES, shapes))


@functools.lru_cache(maxsize=None)
def special():
    """the smooth case without holes on SPECIAL_SHAPE with the SPECIAL values placed"""
    H, W = SPECIAL_SHAPE
    case = {k: v.clone() for k, v in smooth(H, W, holes=False).items()}
    am = case["allmap"]
    for (y, x), what in SPECIAL.items():
        if what.startswith("D="):
            am[0, y, x], am[1, y, x] = float(what[2:4]), 0.0
        elif what.startswith("med="):
            am[5, y, x] = float(what[4:])
        else:
            am[0, y, x], am[1, y, x] = OVERFLOW_D, 1e-30
    return case


def near_special():
    """(H, W) bool: pixels with a special pixel among their four neighbours"""
    H, W = SPECIAL_SHAPE
    m = torch.zeros(H, W, dtype=torch.bool)
    for (y, x) in SPECIAL:
        for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            m[y + dy, x + dx] = True
    return m
