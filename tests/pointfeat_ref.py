"""Plain-torch restatement, dtype-generic, of the projected bilinear sampling of csrc/pointfeat.hip (include/gdr.h
gdr_point_feats_* / gdr_sample_views_*): projection, F.grid_sample with zero padding at the reference's normalised
coordinates, and the |depth sample - z| channel; gradients come from autograd.  In f64 it is the truth of
tests/test_gpu_pointfeat.py, in f32 (on the CPU) the yardstick of its bars.  Inputs are made in f32 and upcast, so both
precisions and the GPU see the same numbers.

Test cameras: eyes on a ring of radius 1.9 around the +-0.5 cube, looking at the origin from different heights, fovx != fovy,
a principal point off centre by a non-integer amount, non-square images.
"""
import functools
import math

import torch
import torch.nn.functional as F

EPS = 2.0 ** -23
NEAR_INTEGER = 1e-3        # px: points this close to an integer position may leave the point-gradient comparison
MAX_EXCLUDED = 0.03


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------
def project(points, w2cs, ixts, pair_mask=None):
    """points (N, 3), w2cs (V, 4, 4), ixts (V, 3, 3) -> xy (V, N, 2), z (V, N).  pair_mask (V, N) bool: False marks a
    degenerate pair, whose position is replaced by a constant far outside every image (zeros sampled, no gradient through
    x and y); z is left as it is."""
    q = torch.einsum("vij,nj->vni", w2cs[:, :3, :3], points) + w2cs[:, :3, 3][:, None]
    h = torch.einsum("vij,vnj->vni", ixts, q)
    z = h[..., 2]
    if pair_mask is None:
        return h[..., :2] / z[..., None], z
    safe = torch.where(pair_mask, z, torch.ones_like(z))
    xy = h[..., :2] / safe[..., None]
    return torch.where(pair_mask[..., None], xy, torch.full_like(xy, -1.0e4)), z


def sample(images, xy):
    """images (V, C, H, W), xy (V, N, 2) pixel positions -> (V, C, N), by the reference's route: normalise, grid_sample."""
    H, W = images.shape[-2:]
    grid = (xy + 0.5) / torch.tensor([W, H], dtype=xy.dtype, device=xy.device) * 2 - 1
    return F.grid_sample(images, grid[:, None], mode="bilinear", padding_mode="zeros", align_corners=False)[:, :, 0]


def sample_views(images, points, w2cs, ixts, pair_mask=None):
    xy, z = project(points, w2cs, ixts, pair_mask)
    return sample(images, xy), z


def point_feats(img_ref, image, acc_map, depth, points, w2cs, ixts, pair_mask=None):
    """-> (N, V, 8): ref rgb, render rgb, acc, |depth sample - z|"""
    coarse = torch.cat((image, acc_map[..., None], depth.reshape(*acc_map.shape, 1)), dim=-1).permute(0, 3, 1, 2)
    xy, z = project(points, w2cs, ixts, pair_mask)
    f = sample(torch.cat((img_ref, coarse), dim=1), xy)
    f = torch.cat((f[:, :7], (f[:, 7:] - z[:, None]).abs()), dim=1)
    return f.permute(2, 0, 1)


def hand_bilinear(image, x, y):
    """image (C, H, W), one position -> (C,): the four neighbours floor + {0, 1} weighted by the fractional parts, those
    outside the image left out.  Plain Python on f64."""
    C, H, W = image.shape
    x0, y0 = math.floor(x), math.floor(y)
    out = torch.zeros(C, dtype=torch.float64)
    for j, wy in ((y0, y0 + 1 - y), (y0 + 1, y - y0)):
        for i, wx in ((x0, x0 + 1 - x), (x0 + 1, x - x0)):
            if 0 <= i < W and 0 <= j < H:
                out += image[:, j, i].double() * (wx * wy)
    return out


# ---- cameras and inputs -----------------------------------------------------------------------------------------------------
def cameras(V, H, W, fov_deg=(60.0, 48.0), principal=(1.37, -0.83), radius=1.9):
    """-> w2cs (V, 4, 4), ixts (V, 3, 3) in f32 (x right, y down, z forward); principal: offset of the principal point from
    the image centre in px"""
    w2cs, ixts = [], []
    for i in range(V):
        a, e = 2 * math.pi * (i + 0.37) / V, 0.45 * math.sin(1.7 * i + 0.4)
        eye = radius * torch.tensor([math.cos(a) * math.cos(e), math.sin(a) * math.cos(e), math.sin(e)], dtype=torch.float64)
        fwd = -eye / eye.norm()
        right = torch.linalg.cross(fwd, torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64))
        right = right / right.norm()
        down = torch.linalg.cross(fwd, right)
        R = torch.stack((right, down, fwd))
        m = torch.eye(4, dtype=torch.float64)
        m[:3, :3], m[:3, 3] = R, -R @ eye
        k = torch.eye(3, dtype=torch.float64)
        k[0, 0] = 0.5 * W / math.tan(math.radians(fov_deg[0]) / 2)
        k[1, 1] = 0.5 * H / math.tan(math.radians(fov_deg[1]) / 2)
        k[0, 2], k[1, 2] = W / 2 + principal[0], H / 2 + principal[1]
        w2cs.append(m)
        ixts.append(k)
    return torch.stack(w2cs).float(), torch.stack(ixts).float()


def make_inputs(N, V, H, W, C=0, seed=0, fov_deg=(60.0, 48.0), principal=(1.37, -0.83)):
    """f32 CPU inputs of both ops and their upstream gradients; every channel and view has its own level and magnitude."""
    g = torch.Generator().manual_seed(seed)
    w2cs, ixts = cameras(V, H, W, fov_deg, principal)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")

    def planes(n, lo, hi):      # (V, n, H, W): a wave per plane plus noise, in [lo, hi]
        k = torch.arange(V * n, dtype=torch.float32).view(V, n, 1, 1)
        s = 0.5 + 0.3 * torch.sin(0.31 * (1 + k % 3) * xx + 0.23 * (1 + k % 5) * yy + k) + 0.2 * (torch.rand(V, n, H, W, generator=g) - 0.5)
        return lo + (hi - lo) * s

    inp = dict(w2cs=w2cs, ixts=ixts, points=torch.rand(N, 3, generator=g) - 0.5,
               img_ref=planes(3, 0.0, 1.0), image=planes(3, 0.0, 1.0).permute(0, 2, 3, 1).contiguous(),
               acc_map=planes(1, 0.0, 1.0)[:, 0].contiguous(),
               depth=planes(1, 1.2, 2.6).permute(0, 2, 3, 1).contiguous(),     # straddles the points' z: both signs of the z difference
               gout=torch.randn(N, V, 8, generator=g) * (1 + 0.5 * torch.arange(8, dtype=torch.float32)))
    if C:
        inp["images"] = torch.randn(V, C, H, W, generator=g) * (0.5 + torch.arange(C, dtype=torch.float32).view(1, C, 1, 1) % 4)
        inp["gfeat"] = torch.randn(V, C, N, generator=g) * (1 + torch.arange(V, dtype=torch.float32).view(V, 1, 1))
        inp["gz"] = torch.randn(V, N, generator=g)
    return inp


FEAT_LEAVES = ("img_ref", "image", "acc_map", "depth", "points")
VIEWS_LEAVES = ("images", "points")


def run_point_feats(inp, dtype, pair_mask=None):
    """-> dict(out, g_img_ref, g_image, g_acc_map, g_depth, g_points) in `dtype` on the CPU"""
    leaves = {k: inp[k].to(dtype).clone().requires_grad_(True) for k in FEAT_LEAVES}
    out = point_feats(**leaves, w2cs=inp["w2cs"].to(dtype), ixts=inp["ixts"].to(dtype), pair_mask=pair_mask)
    out.backward(inp["gout"].to(dtype))
    return dict(out=out.detach(), **{"g_" + k: v.grad for k, v in leaves.items()})


def run_sample_views(inp, dtype, pair_mask=None):
    """-> dict(out, z, g_images, g_points)"""
    leaves = {k: inp[k].to(dtype).clone().requires_grad_(True) for k in VIEWS_LEAVES}
    out, z = sample_views(**leaves, w2cs=inp["w2cs"].to(dtype), ixts=inp["ixts"].to(dtype), pair_mask=pair_mask)
    torch.autograd.backward((out, z), (inp["gfeat"].to(dtype), inp["gz"].to(dtype)))
    return dict(out=out.detach(), z=z.detach(), **{"g_" + k: v.grad for k, v in leaves.items()})


# ---- what the bars need from the f64 positions ------------------------------------------------------------------------------
def positions(inp, pair_mask=None):
    """f64 (x, y) of every pair: (V, N) each; a pair that pair_mask marks degenerate sits far outside every image"""
    xy, _ = project(inp["points"].double(), inp["w2cs"].double(), inp["ixts"].double(), pair_mask)
    return xy[..., 0], xy[..., 1]


def tap_stats(inp, H, W, pair_mask=None):
    """-> (k_max, border share, inside share): the largest number of (pair, neighbour) contributions one texel of one view
    receives; the share of pairs with at least one neighbour outside the image; the share of pairs whose four neighbours
    all lie inside.  A degenerate pair (pair_mask False) contributes to no texel."""
    x, y = positions(inp, pair_mask)
    V = x.shape[0]
    x0, y0 = torch.floor(x).long(), torch.floor(y).long()
    counts = torch.zeros(V * H * W, dtype=torch.long)
    n_in = torch.zeros_like(x0)
    for dy in (0, 1):
        for dx in (0, 1):
            xi, yi = x0 + dx, y0 + dy
            ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
            n_in += ok.long()
            flat = (torch.arange(V).view(V, 1) * H + yi) * W + xi
            counts += torch.bincount(flat[ok], minlength=V * H * W)
    return int(counts.max()), float((n_in < 4).double().mean()), float((n_in == 4).double().mean())


def keep_for_point_grad(inp, near_px=NEAR_INTEGER, pair_mask=None):
    """(N,) bool: points whose position in no view lies within near_px (<= NEAR_INTEGER) of an integer (there the point
    gradient jumps); the test asserts that at most MAX_EXCLUDED of the points are dropped.  A degenerate pair (pair_mask
    False) has no position and excludes nothing."""
    assert near_px <= NEAR_INTEGER
    x, y = positions(inp, pair_mask)
    near = ((x - torch.round(x)).abs() < near_px) | ((y - torch.round(y)).abs() < near_px)
    if pair_mask is not None:
        near &= pair_mask
    return ~near.any(dim=0)


def bar(err_t32, truth, k=8):
    return 2.0 * err_t32 + k * EPS * float(truth.abs().max())


def max_err(a, truth):
    return float((a.double() - truth).abs().max()) if truth.numel() else 0.0


@functools.lru_cache(maxsize=None)
def feats_case(N, V, H, W, seed=0, fov_deg=(60.0, 48.0), principal=(1.37, -0.83)):
    """inputs, f64 truth and f32 torch composition of point_feats, computed once per shape and shared (never modified)"""
    inp = make_inputs(N, V, H, W, 0, seed, fov_deg, principal)
    return inp, run_point_feats(inp, torch.float64), run_point_feats(inp, torch.float32)


@functools.lru_cache(maxsize=None)
def views_case(N, V, H, W, C, seed=0, fov_deg=(60.0, 48.0), principal=(1.37, -0.83)):
    inp = make_inputs(N, V, H, W, C, seed, fov_deg, principal)
    return inp, run_sample_views(inp, torch.float64), run_sample_views(inp, torch.float32)
