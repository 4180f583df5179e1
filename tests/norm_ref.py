"""float64 numpy restatement of the fused row normalisations (generativedensification_amd/norm.py, csrc/norm.hip): both
forwards and the closed-form gradients the kernels implement.  tests/test_norm_cpu.py holds it against autograd of the torch
composition; tests/test_gpu_norm.py holds the kernels against it."""
import numpy as np


def _layer_norm(z, eps):
    """(xh, rstd): rows of z normalised over the last axis with the biased variance"""
    mean = z.mean(-1, keepdims=True)
    var = ((z - mean) ** 2).mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    return (z - mean) * rstd, rstd


def _layer_norm_grad(dxh, xh, rstd):
    return rstd * (dxh - dxh.mean(-1, keepdims=True) - xh * (dxh * xh).mean(-1, keepdims=True))


def segment_of_rows(offset, n):
    """For every row 0..n-1 the segment b with offset[b - 1] <= i < offset[b] (offset[-1] := 0); len(offset) behind the last."""
    return np.searchsorted(np.asarray(offset, dtype=np.int64), np.arange(n, dtype=np.int64), side="right")


def ada_layer_norm(feat, scale, offset, eps=1e-5):
    feat, scale = np.asarray(feat, dtype=np.float64), np.asarray(scale, dtype=np.float64)
    n = feat.shape[0]
    seg = segment_of_rows(offset, n)
    inside = seg < len(offset)
    xh, _ = _layer_norm(feat, eps)
    out = np.zeros_like(feat)
    out[inside] = scale[seg[inside]] * xh[inside]
    return out


def ada_layer_norm_grad(feat, scale, offset, grad_out, eps=1e-5):
    """(dfeat, dscale)"""
    feat, scale, g = (np.asarray(a, dtype=np.float64) for a in (feat, scale, grad_out))
    n = feat.shape[0]
    seg = segment_of_rows(offset, n)
    inside = seg < len(offset)
    xh, rstd = _layer_norm(feat, eps)
    dfeat = np.zeros_like(feat)
    dscale = np.zeros_like(scale)
    dxh = g[inside] * scale[seg[inside]]
    dfeat[inside] = _layer_norm_grad(dxh, xh[inside], rstd[inside])
    np.add.at(dscale, seg[inside], g[inside] * xh[inside])
    return dfeat, dscale


def pe_rows(x, feat, frequencies, upscale_factor):
    """z (P S, 6F + C): sin(f_k x[r, j]) at 3k + j, cos at 3F + 3k + j, then feat[r // S]"""
    x, feat, f = (np.asarray(a, dtype=np.float64) for a in (x, feat, frequencies))
    fx = (f[None, :, None] * x[:, None, :]).reshape(x.shape[0], -1)
    return np.concatenate([np.sin(fx), np.cos(fx), np.repeat(feat, upscale_factor, axis=0)], axis=-1), fx


def pe_concat_layer_norm(x, feat, frequencies, upscale_factor, eps=1e-5):
    z, _ = pe_rows(x, feat, frequencies, upscale_factor)
    return _layer_norm(z, eps)[0]


def pe_concat_layer_norm_grad(x, feat, frequencies, upscale_factor, grad_out, eps=1e-5):
    """(dx, dfeat)"""
    f = np.asarray(frequencies, dtype=np.float64)
    g = np.asarray(grad_out, dtype=np.float64)
    z, fx = pe_rows(x, feat, frequencies, upscale_factor)
    zh, rstd = _layer_norm(z, eps)
    dz = _layer_norm_grad(g, zh, rstd)
    t = fx.shape[1]
    dfx = np.cos(fx) * dz[:, :t] - np.sin(fx) * dz[:, t:2 * t]
    dx = (dfx.reshape(-1, len(f), 3) * f[None, :, None]).sum(1)
    p, c = np.asarray(feat).shape
    dfeat = dz[:, 2 * t:].reshape(p, upscale_factor, c).sum(1)
    return dx, dfeat


def to_dtype(a, dtype):
    """a float64 array rounded once to a torch dtype, as a torch tensor"""
    import torch

    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).to(dtype)


def half_ulp(dtype, magnitude):
    """half the spacing of `dtype` at |value| = magnitude"""
    import math

    import torch

    bits = {torch.float32: 23, torch.float16: 10, torch.bfloat16: 7}[dtype]
    tiny = {torch.float32: -126, torch.float16: -14, torch.bfloat16: -126}[dtype]
    e = max(math.floor(math.log2(magnitude)) if magnitude > 0 else tiny, tiny)
    return 0.5 * 2.0 ** (e - bits)
