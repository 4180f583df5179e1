"""Plain-torch restatement, dtype-generic, of the image-space kernels of csrc/loss.hip and csrc/maps_surfel.hip: the five
maps the 2DGS adaptor derives from the rasterizer's allmap (renderer_2dgs.py's torch sequence), the clamp, and the terms of
synthetic.view_loss / synthetic.surfel_loss.  Gradients come from autograd.  In f64 it is the truth of
tests/test_gpu_imgloss.py, in f32 (on the CPU) the yardstick of its bars (err_torch32).  Inputs are rounded to f32 and
upcast, so both precisions and the GPU see the same numbers.

Degenerate pixels.  Torch returns NaN for the gradient of allmap[0:2] wherever the f32 quotient allmap[0] / alpha is not
finite (0 * inf behind nan_to_num), and nan_to_num's replacement of -inf depends on the dtype.  `masks()` finds those pixels
on the f32 inputs; with a mask the restatement replaces the quotient (and a non-finite median depth) there by the constant
the f32 nan_to_num gives, which passes no gradient.  Without a mask, `maps` is the adaptor's sequence verbatim."""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

EPS = 2.0 ** -23
FLT_MAX = 3.4028234663852886e38
COND_FLOOR = 1e-2

Masks = namedtuple("Masks", "exp_ok exp_fill med_ok med_fill")     # (1, H, W) each: bool, f32, bool, f32


def masks(allmap):
    """From the f32 allmap: where the expected-depth quotient and the median depth are finite in f32 (differentiable), and
    what torch.nan_to_num(x, 0, 0) puts in their place elsewhere (0, 0 or -FLT_MAX)."""
    am = allmap.float()
    e, med = am[0:1] / am[1:2], am[5:6]
    return Masks(torch.isfinite(e), torch.nan_to_num(e, 0, 0), torch.isfinite(med), torch.nan_to_num(med, 0, 0))


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------
def surf_depth(allmap, ratio, mask=None):
    """(1, H, W): (1 - r) nan0(allmap[0] / alpha) + r nan0(allmap[5])"""
    D, a, med = allmap[0:1], allmap[1:2], allmap[5:6]
    if mask is None:
        e, m = torch.nan_to_num(D / a, 0, 0), torch.nan_to_num(med, 0, 0)
    else:
        e = torch.where(mask.exp_ok, D / torch.where(mask.exp_ok, a, torch.ones_like(a)), mask.exp_fill.to(allmap.dtype))
        m = torch.where(mask.med_ok, med, mask.med_fill.to(allmap.dtype))
    return e * (1 - ratio) + ratio * m


def points(rays, depth):
    """rays (H, W, 6) = origin | direction, depth (1, H, W) -> (H, W, 3)"""
    p = rays[..., :3].reshape(-1, 3) + depth.reshape(-1, 1) * rays[..., 3:].reshape(-1, 3)
    return p.reshape(*depth.shape[1:], 3)


def differences(pts):
    """row and column central differences at the interior pixels: (H-2, W-2, 3) each"""
    return pts[2:, 1:-1] - pts[:-2, 1:-1], pts[1:-1, 2:] - pts[1:-1, :-2]


def pseudo_normal(rays, depth):
    """(H, W, 3): normalised cross product of the central differences, zero on the 1-px border"""
    pts = points(rays, depth)
    d_rows, d_cols = differences(pts)
    inner = F.normalize(torch.cross(d_rows, d_cols, dim=-1), dim=-1)          # eps = 1e-12
    normal = torch.zeros_like(pts)
    normal[1:-1, 1:-1, :] = inner
    return normal


def maps(allmap, rays, view, ratio, mask=None):
    """-> depth (H, W, 1), acc_map (H, W), rend_normal (H, W, 3), depth_normal (H, W, 3), rend_dist (H, W)"""
    alpha = allmap[1:2]
    normal_world = (allmap[2:5].permute(1, 2, 0) @ view[:3, :3].T).permute(2, 0, 1)
    sd = surf_depth(allmap, ratio, mask)
    sn = pseudo_normal(rays, sd).permute(2, 0, 1) * alpha.detach()
    return sd.permute(1, 2, 0), alpha.squeeze(0), normal_world.permute(1, 2, 0), sn.permute(1, 2, 0), allmap[6:7].squeeze(0)


def view_loss(color, depth, alpha, target, w_depth=0.1, w_alpha=0.1):
    """color, target (3, H, W), depth, alpha (1, H, W): synthetic.view_loss on the clamped dict"""
    image = color.clamp(0, 1).permute(1, 2, 0)
    return (((image - target.permute(1, 2, 0)) ** 2).mean() + w_depth * depth.permute(1, 2, 0).mean()
            + w_alpha * alpha.squeeze(0).mean())


def view_terms(color, depth, alpha, target, w_depth=0.1, w_alpha=0.1):
    """(H, W): what each pixel adds to view_loss"""
    P = depth.numel()
    se = ((color.clamp(0, 1) - target) ** 2).sum(0)
    return (se / 3 + w_depth * depth[0] + w_alpha * alpha[0]) / P


def surfel_loss(color, allmap, rays, view, target, ratio, w_dist=1000.0, w_normal=0.2, w_depth=0.1, w_alpha=0.1, mask=None):
    """synthetic.surfel_loss on the dict of the maps and the clamped colour"""
    depth, acc, rn, dn, dist = maps(allmap, rays, view, ratio, mask)
    image = color.clamp(0, 1).permute(1, 2, 0)
    loss = ((image - target.permute(1, 2, 0)) ** 2).mean()
    loss = loss + w_dist * dist.mean()
    normal_error = ((1 - (rn * dn).sum(dim=-1)) * acc.detach()).mean()
    return loss + w_normal * normal_error + w_depth * depth.mean() + w_alpha * acc.mean()


def surfel_terms(color, allmap, rays, view, target, ratio, w_dist=1000.0, w_normal=0.2, w_depth=0.1, w_alpha=0.1, mask=None):
    """(H, W): what each pixel adds to surfel_loss"""
    depth, acc, rn, dn, dist = maps(allmap, rays, view, ratio, mask)
    se = ((color.clamp(0, 1) - target) ** 2).sum(0)
    return (se / 3 + w_dist * dist + w_normal * (1 - (rn * dn).sum(-1)) * acc + w_depth * depth[..., 0] + w_alpha * acc) / acc.numel()


# ---- what the bars need -----------------------------------------------------------------------------------------------------
def cond(allmap, rays, ratio):
    """(H-2, W-2) f64: per interior pixel |a x b| / (|a| |b|) of the row difference a and the column difference b of the
    unprojected depth map; 0 where the cross product vanishes exactly (the clamped-denominator branch of the normalisation)"""
    am = allmap.double()
    a, b = differences(points(rays.double(), surf_depth(am, ratio, masks(allmap))))
    c = torch.cross(a, b, dim=-1).norm(dim=-1)
    return torch.where(c == 0, torch.zeros_like(c), c / (a.norm(dim=-1) * b.norm(dim=-1)).clamp_min(1e-300))


def conditioned(allmap, rays, ratio):
    """every interior pixel has |a x b| == 0 exactly or cond >= COND_FLOOR; -> (ok, smallest non-zero cond, share of zeros)"""
    c = cond(allmap, rays, ratio)
    nz = c[c != 0]
    lo = float(nz.min()) if nz.numel() else float("inf")
    return lo >= COND_FLOOR, lo, float((c == 0).double().mean()) if c.numel() else 0.0


def away_from_clamped(allmap, rays, ratio):
    """(H, W) bool: pixels that are no neighbour of an interior pixel whose cross product vanishes.  Such a stencil hands its
    neighbours gradients of the order 1e12 (the normalisation divides by its eps), which would set max|truth| of a whole
    channel; the tests judge the channels a second time on these pixels alone."""
    H, W = allmap.shape[1:]
    near = torch.zeros(H, W, dtype=torch.bool)
    if H >= 3 and W >= 3:
        zero = cond(allmap, rays, ratio) == 0
        near[:-2, 1:-1] |= zero
        near[2:, 1:-1] |= zero
        near[1:-1, :-2] |= zero
        near[1:-1, 2:] |= zero
    return ~near


def chain_length(P, cap):
    """the longest chain of additions of a grid-stride reduction over P pixels, 256 threads per workgroup, at most `cap`
    workgroups: the thread's own stride, 6 wave shuffles, 3 adds of the wave sums, one atomic add per workgroup"""
    groups = min(-(-P // 256), cap)
    return -(-P // (groups * 256)) + 6 + 3 + groups


def bar(err_t32, truth, k=8):
    return 2.0 * err_t32 + k * EPS * float(truth.abs().max())


def scalar_bar(err_t32, chain, terms):
    return 2.0 * err_t32 + chain * EPS * float(terms.double().abs().sum())


def max_err(a, truth):
    return float((a.double() - truth).abs().max()) if truth.numel() else 0.0


# ---- runs: truth in f64, yardstick in f32 -----------------------------------------------------------------------------------
MAP_NAMES = ("depth", "acc_map", "rend_normal", "depth_normal", "rend_dist")


def run_maps(case, ratio, dtype, ups=None, mask=True):
    """-> dict of the five maps and, with upstream gradients `ups` (five tensors or None for a zero one), dL_dallmap"""
    am = case["allmap"].to(dtype).clone().requires_grad_(ups is not None)
    out = maps(am, case["rays"].to(dtype), case["view"].to(dtype), ratio, masks(case["allmap"]) if mask else None)
    res = {k: v.detach() for k, v in zip(MAP_NAMES, out)}
    if ups is not None:
        torch.autograd.backward([o for o, u in zip(out, ups) if u is not None], [u.to(dtype) for u in ups if u is not None])
        res["dL_dallmap"] = am.grad
    return res


def run_surfel_loss(case, ratio, dtype, go=1.0, mask=True, **w):
    """-> dict(loss, terms, dL_dcolor, dL_dallmap); `go` scales the loss before the backward"""
    color = case["color"].to(dtype).clone().requires_grad_(True)
    am = case["allmap"].to(dtype).clone().requires_grad_(True)
    args = (case["rays"].to(dtype), case["view"].to(dtype), case["target"].to(dtype), ratio)
    mask = masks(case["allmap"]) if mask else None
    loss = surfel_loss(color, am, *args, mask=mask, **w)
    (loss * go).backward()
    with torch.no_grad():
        terms = surfel_terms(color, am, *args, mask=mask, **w)
    return dict(loss=loss.detach(), terms=terms, dL_dcolor=color.grad, dL_dallmap=am.grad)


def run_view_loss(case, dtype, go=1.0, **w):
    """-> dict(loss, terms, dL_dcolor, dL_ddepth, dL_dalpha)"""
    leaves = [case[k].to(dtype).clone().requires_grad_(True) for k in ("color", "depth", "alpha")]
    tg = case["target"].to(dtype)
    loss = view_loss(*leaves, tg, **w)
    (loss * go).backward()
    with torch.no_grad():
        terms = view_terms(*leaves, tg, **w)
    return dict(loss=loss.detach(), terms=terms, dL_dcolor=leaves[0].grad, dL_ddepth=leaves[1].grad, dL_dalpha=leaves[2].grad)


@functools.lru_cache(maxsize=None)
def maps_case(H, W, ratio):
    """inputs, upstream gradients, f64 truth and f32 torch composition of the maps, computed once per (shape, ratio) and
    shared (never modified)"""
    import imgloss_cases as K
    case = K.smooth(H, W)
    ups = K.upstreams(H, W)
    return case, ups, run_maps(case, ratio, torch.float64, ups), run_maps(case, ratio, torch.float32, ups)


@functools.lru_cache(maxsize=None)
def surfel_loss_case(H, W, ratio, w_dist, go):
    import imgloss_cases as K
    case = K.smooth(H, W)
    return case, run_surfel_loss(case, ratio, torch.float64, go, w_dist=w_dist), run_surfel_loss(case, ratio, torch.float32, go, w_dist=w_dist)


@functools.lru_cache(maxsize=None)
def view_loss_case(H, W, go):
    import imgloss_cases as K
    case = K.smooth(H, W)
    return case, run_view_loss(case, torch.float64, go), run_view_loss(case, torch.float32, go)
