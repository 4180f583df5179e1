"""The reference's torch composition of the volume conditioning, restated for the tests (dtype- and device-generic): what
Network.build_feat_vol, the view_embed concat of Network.forward and the cond lines of VolTransformer.forward compute
(lightning/network.py), including F.grid_sample."""
import torch
import torch.nn.functional as F


def rsh3(v):
    x, y, z = v.unbind(-1)
    pi = torch.pi
    k1, k2a, k2b, k2c = (3 / (4 * pi)) ** 0.5, (15 / (4 * pi)) ** 0.5, (5 / (16 * pi)) ** 0.5, (15 / (16 * pi)) ** 0.5
    k3a, k3b, k3c, k3d, k3e = ((35 / (32 * pi)) ** 0.5, (105 / (4 * pi)) ** 0.5, (21 / (32 * pi)) ** 0.5, (7 / (16 * pi)) ** 0.5,
                               (105 / (16 * pi)) ** 0.5)
    return torch.stack([torch.full_like(x, (1 / (4 * pi)) ** 0.5), -k1 * y, k1 * z, -k1 * x, k2a * x * y, -k2a * y * z,
                        k2b * (3 * z * z - 1), -k2a * x * z, k2c * (x * x - y * y), -k3a * y * (3 * x * x - y * y), k3b * x * y * z,
                        -k3c * y * (5 * z * z - 1), k3d * z * (5 * z * z - 3), -k3c * x * (5 * z * z - 1), k3e * z * (x * x - y * y),
                        -k3a * x * (x * x - 3 * y * y)], -1)


def ray_sh(rays, silu=False):
    origin, direction = rays[..., :3], rays[..., 3:6]
    direction = F.normalize(direction, p=2.0, dim=-1)
    plucker = torch.cat((direction, torch.cross(origin, direction, dim=-1)), dim=-1)
    out = torch.cat((rsh3(plucker[..., :3]), rsh3(plucker[..., 3:6])), dim=-1)
    return F.silu(out) if silu else out


def mod_layer_norm(x, shift_scale, weight, bias, eps):
    shift, scale = shift_scale.reshape(*x.shape[:-1], -1).chunk(2, dim=-1)
    return F.layer_norm(x, x.shape[-1:], weight, bias, eps) * (1 + scale) + shift


def feat_vol(maps, points, w2cs, ixts, img_hw, n_views):
    """maps (BV, C, h, w) -> (B, V, C, r, r, r): projection, normalisation by the image size, grid_sample"""
    h, w = img_hw
    pts = points.reshape(1, -1, 3) @ w2cs[:, :3, :3].permute(0, 2, 1) + w2cs[:, :3, 3][:, None]
    pts = pts @ ixts.permute(0, 2, 1)
    xy = pts[..., :2] / pts[..., -1:]
    xy = (xy + 0.5) / torch.tensor([w, h], device=xy.device) * 2 - 1.0
    work = maps if maps.dtype == torch.float64 else maps.float()
    vol = F.grid_sample(work, xy.unsqueeze(1).to(work.dtype), align_corners=False).to(maps)
    r = round(points.shape[0] ** (1 / 3))
    return vol.view(-1, n_views, maps.shape[1], r, r, r)


def cond_of(vol, n_group):
    """the cond lines of VolTransformer.forward"""
    B, V, C, D = vol.shape[:4]
    bs = D // n_group
    blocks = vol.unfold(3, bs, bs).unfold(4, bs, bs).unfold(5, bs, bs)
    blocks = blocks.contiguous().view(B, V, C, n_group ** 3, bs ** 3)
    return torch.einsum('bvcgl->bgvlc', blocks).reshape(B * n_group ** 3, bs ** 3 * V, C)


def sample_tokens(rows, points, w2cs, ixts, img_hw, n_group, n_views, view_embed=None):
    """rows (BV, h, w, C) channels-last -> cond (B g^3, V bs^3, C + E) by the reference's route"""
    vol = feat_vol(torch.einsum('bhwc->bchw', rows), points, w2cs, ixts, img_hw, n_views)
    if view_embed is not None:
        r = vol.shape[-1]
        vol = torch.cat((vol, view_embed[:, :n_views].expand(vol.shape[0], -1, -1, r, r, r)), dim=2)
    return cond_of(vol, n_group)
