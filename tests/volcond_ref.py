"""Float64 numpy restatement of the volume conditioning of csrc/volcond.hip (include/gdr.h gdr_volcond_*) and of its gradients:
ray_sh, mod_layer_norm and sample_tokens with the cond permutation, written from the definitions and independent of the
package (deconv3d._cond is not used)."""
import numpy as np

PI = np.pi
# the real spherical harmonics of degree <= 3, closed forms
K0 = np.sqrt(1 / (4 * PI))
K1 = np.sqrt(3 / (4 * PI))
K2A, K2B, K2C = np.sqrt(15 / (4 * PI)), np.sqrt(5 / (16 * PI)), np.sqrt(15 / (16 * PI))
K3A, K3B, K3C, K3D, K3E = (np.sqrt(35 / (32 * PI)), np.sqrt(105 / (4 * PI)), np.sqrt(21 / (32 * PI)), np.sqrt(7 / (16 * PI)),
                           np.sqrt(105 / (16 * PI)))


def rsh3(v):
    """v (..., 3) -> (..., 16): Y_l^m at l (l + 1) + m as polynomials of (x, y, z), Condon-Shortley phase"""
    v = np.asarray(v, dtype=np.float64)
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    return np.stack([np.full_like(x, K0), -K1 * y, K1 * z, -K1 * x, K2A * x * y, -K2A * y * z, K2B * (3 * z * z - 1), -K2A * x * z,
                     K2C * (x * x - y * y), -K3A * y * (3 * x * x - y * y), K3B * x * y * z, -K3C * y * (5 * z * z - 1),
                     K3D * z * (5 * z * z - 3), -K3C * x * (5 * z * z - 1), K3E * z * (x * x - y * y), -K3A * x * (x * x - 3 * y * y)], -1)


def ray_sh(rays, silu=False):
    rays = np.asarray(rays, dtype=np.float64)
    o, d = rays[..., :3], rays[..., 3:6]
    dh = d / np.maximum(np.sqrt((d * d).sum(-1, keepdims=True)), 1e-12)
    out = np.concatenate([rsh3(dh), rsh3(np.cross(o, dh))], -1)
    return out / (1 + np.exp(-out)) if silu else out


def _layer_norm(x, eps):
    mean = x.mean(-1, keepdims=True)
    var = ((x - mean) ** 2).mean(-1, keepdims=True)
    rstd = 1 / np.sqrt(var + eps)
    return (x - mean) * rstd, rstd


def mod_layer_norm(x, shift_scale, weight, bias, eps):
    x, ss = np.asarray(x, dtype=np.float64), np.asarray(shift_scale, dtype=np.float64)
    c = x.shape[-1]
    w = np.ones(c) if weight is None else np.asarray(weight, dtype=np.float64)
    b = np.zeros(c) if bias is None else np.asarray(bias, dtype=np.float64)
    xh, _ = _layer_norm(x, eps)
    return (xh * w + b) * (1 + ss[..., c:]) + ss[..., :c]


def mod_layer_norm_grad(x, shift_scale, weight, bias, eps, grad_out):
    """(dx, dshift_scale, dweight, dbias) for 2-D x"""
    x, ss, g = (np.asarray(t, dtype=np.float64) for t in (x, shift_scale, grad_out))
    c = x.shape[-1]
    w = np.ones(c) if weight is None else np.asarray(weight, dtype=np.float64)
    b = np.zeros(c) if bias is None else np.asarray(bias, dtype=np.float64)
    xh, rstd = _layer_norm(x, eps)
    y = xh * w + b
    dy = g * (1 + ss[:, c:])
    dss = np.concatenate([g, g * y], -1)
    dxh = dy * w
    dx = rstd * (dxh - dxh.mean(-1, keepdims=True) - xh * (dxh * xh).mean(-1, keepdims=True))
    return dx, dss, (dy * xh).sum(0), dy.sum(0)


def cond_rows(B, V, r, n_group):
    """row[b, v, n] of the (B g^3 * V bs^3) cond rows for grid point n = (z r + y) r + x: blocks (gz, gy, gx), then the view, then
    the voxel (iz, iy, ix) inside the block"""
    g, bs = n_group, r // n_group
    z, y, x = np.meshgrid(np.arange(r), np.arange(r), np.arange(r), indexing="ij")
    z, y, x = z.reshape(-1), y.reshape(-1), x.reshape(-1)
    block = ((z // bs) * g + y // bs) * g + x // bs
    inside = ((z % bs) * bs + y % bs) * bs + x % bs
    b = np.arange(B)[:, None, None]
    v = np.arange(V)[None, :, None]
    return ((b * g ** 3 + block[None, None]) * V + v) * bs ** 3 + inside[None, None]


def taps(points, w2cs, ixts, img_hw, hw):
    """texel (BV, N, 4) int (flat y w + x, clamped), weight (BV, N, 4), inside (BV, N, 4) bool; tap t = 2 (y neighbour) + x neighbour"""
    p, w2c, k = (np.asarray(t, dtype=np.float64) for t in (points, w2cs, ixts))
    h, w = hw
    q = np.einsum("vij,nj->vni", w2c[:, :3, :3], p) + w2c[:, None, :3, 3]
    hc = np.einsum("vij,vnj->vni", k, q)
    ok = hc[..., 2] != 0
    den = np.where(ok, hc[..., 2], 1.0)
    x, y = hc[..., 0] / den, hc[..., 1] / den
    u = (x + 0.5) * w / img_hw[1] - 0.5
    v = (y + 0.5) * h / img_hw[0] - 0.5
    ok &= np.isfinite(u) & np.isfinite(v) & (np.abs(x) <= 2.0 ** 30) & (np.abs(y) <= 2.0 ** 30) & (np.abs(u) <= 2.0 ** 30) & (np.abs(v) <= 2.0 ** 30)
    u, v = np.where(ok, u, 0.0), np.where(ok, v, 0.0)
    x0, y0 = np.floor(u), np.floor(v)
    tex, wt, inside = [], [], []
    for t in range(4):
        xi, yi = x0 + (t & 1), y0 + (t >> 1)
        wx = (u - x0) if t & 1 else (x0 + 1 - u)
        wy = (v - y0) if t >> 1 else (y0 + 1 - v)
        inside.append(ok & (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h))
        tex.append((np.clip(yi, 0, h - 1) * w + np.clip(xi, 0, w - 1)).astype(np.int64))
        wt.append(wx * wy)
    return np.stack(tex, -1), np.stack(wt, -1), np.stack(inside, -1)


def sample_tokens(rows, points, w2cs, ixts, img_hw, n_group, n_views, view_embed=None):
    """rows (BV, h, w, C) -> cond (B g^3, V bs^3, C + E)"""
    rows = np.asarray(rows, dtype=np.float64)
    BV, h, w, C = rows.shape
    V, B = n_views, BV // n_views
    N = np.asarray(points).shape[0]
    r = round(N ** (1 / 3))
    tex, wt, inside = taps(points, w2cs, ixts, img_hw, (h, w))
    flat = rows.reshape(BV, h * w, C)
    samp = np.zeros((BV, N, C))
    for t in range(4):
        samp += np.take_along_axis(flat, tex[..., t][..., None], 1) * (wt[..., t] * inside[..., t])[..., None]
    E = 0 if view_embed is None else np.asarray(view_embed).shape[2]
    ve = np.zeros((V, 0)) if view_embed is None else np.asarray(view_embed, dtype=np.float64)[0, :V, :, 0, 0, 0]
    full = np.concatenate([samp.reshape(B, V, N, C), np.broadcast_to(ve[None, :, None, :], (B, V, N, E))], -1)
    g, bs = n_group, r // n_group
    out = np.zeros((B * g ** 3 * V * bs ** 3, C + E))
    out[cond_rows(B, V, r, n_group).reshape(-1)] = full.reshape(-1, C + E)
    return out.reshape(B * g ** 3, V * bs ** 3, C + E)


def sample_tokens_grad(rows_shape, points, w2cs, ixts, img_hw, n_group, n_views, view_embed_shape, grad_cond):
    """(drows, dview_embed or None)"""
    BV, h, w, C = rows_shape
    V, B = n_views, BV // n_views
    N = np.asarray(points).shape[0]
    r = round(N ** (1 / 3))
    g = np.asarray(grad_cond, dtype=np.float64)
    W = g.shape[-1]
    per = g.reshape(-1, W)[cond_rows(B, V, r, n_group).reshape(-1)].reshape(B, V, N, W)
    tex, wt, inside = taps(points, w2cs, ixts, img_hw, (h, w))
    drows = np.zeros((BV, h * w, C))
    gs = per[..., :C].reshape(BV, N, C)
    for bv in range(BV):
        for t in range(4):
            np.add.at(drows[bv], tex[bv, :, t], gs[bv] * (wt[bv, :, t] * inside[bv, :, t])[:, None])
    dve = None
    if view_embed_shape is not None:
        dve = np.zeros(view_embed_shape)
        dve[0, :V, :, 0, 0, 0] = per[..., C:].sum((0, 2))
    return drows.reshape(BV, h, w, C), dve
