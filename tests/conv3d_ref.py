"""float64 restatement (numpy) of generativedensification_amd/conv3d.py: the forward and the three gradients of a 3x3x3
convolution with stride 1 and zero padding 1 as 27 shifted, zero-filled products.  Independent of torch's convolution; the
arithmetic is the definition in csrc/conv3d.hip's header.

x (B, Cin, D, H, W), weight (Cout, Cin, 3, 3, 3), tap (kd, kh, kw) has the offset (kd, kh, kw) - 1:
    out[b, co, z, y, x] = bias[co] + sum over taps and ci of weight[co, ci, kd, kh, kw] x[b, ci, z + kd - 1, y + kh - 1, x + kw - 1]
"""
import itertools

import numpy as np

TAPS = list(itertools.product(range(3), repeat=3))


def shifted(a, off):
    """s[..., z, y, x] = a[..., z + off[0], y + off[1], x + off[2]] where that voxel exists, zero elsewhere (the last three axes)"""
    a = np.asarray(a, dtype=np.float64)
    out = np.zeros_like(a)
    src, dst = [slice(None)] * (a.ndim - 3), [slice(None)] * (a.ndim - 3)
    for n, o in zip(a.shape[-3:], off):
        if abs(o) >= n:
            return out
        src.append(slice(max(o, 0), n + min(o, 0)))
        dst.append(slice(max(-o, 0), n + min(-o, 0)))
    out[tuple(dst)] = a[tuple(src)]
    return out


def conv3d(x, weight, bias=None, add_input=False):
    x, weight = np.asarray(x, dtype=np.float64), np.asarray(weight, dtype=np.float64)
    out = np.zeros((x.shape[0], weight.shape[0]) + x.shape[2:])
    for kd, kh, kw in TAPS:
        out += np.einsum("oc,bczyx->bozyx", weight[:, :, kd, kh, kw], shifted(x, (kd - 1, kh - 1, kw - 1)))
    if bias is not None:
        out += np.asarray(bias, dtype=np.float64)[None, :, None, None, None]
    return out + x if add_input else out


def conv3d_grad(x, weight, grad_out, add_input=False):
    """(grad_x, grad_weight, grad_bias)"""
    x, weight, g = (np.asarray(a, dtype=np.float64) for a in (x, weight, grad_out))
    grad_x, grad_w = np.zeros_like(x), np.zeros_like(weight)
    for kd, kh, kw in TAPS:
        off = (kd - 1, kh - 1, kw - 1)
        # out[v] reads x[v + off], so x[u] is read by out[u - off]
        grad_x += np.einsum("oc,bozyx->bczyx", weight[:, :, kd, kh, kw], shifted(g, tuple(-o for o in off)))
        grad_w[:, :, kd, kh, kw] = np.einsum("bozyx,bczyx->oc", g, shifted(x, off))
    if add_input:
        grad_x += g
    return grad_x, grad_w, g.sum((0, 2, 3, 4))
