"""CPU restatements of the submanifold sparse convolution (csrc/subm_conv.hip), independent of each other:

  dense truth   scatter the features into a dense (B, Cin, S0, S1, S2) grid, F.conv3d with padding k // 2 and the weight
                permuted to (Cout, Cin, k0, k1, k2), gather at the sites; gradients by autograd.  Valid when every site is
                inside the grid and no two share a voxel.  Shares nothing with the table method.
  table model   a dictionary from voxel to the LOWEST point index; nbr / rep from look-ups, out[i] = bias + sum_k
                feat[nbr[k, i]] @ W[k]; gradients by autograd through index_select.  It defines what happens to sites that
                share a voxel and to sites outside the grid.

Both take the dtype to compute in: float64 is the truth, float32 the yardstick whose own error sets the tests' bar.
"""
import numpy as np
import torch
import torch.nn.functional as F


def tap_offsets(ksize):
    k0, k1, k2 = ksize
    return [(t0 - k0 // 2, t1 - k1 // 2, t2 - k2 // 2) for t0 in range(k0) for t1 in range(k1) for t2 in range(k2)]


def table_model(indices, spatial_shape, batch_size, ksize):
    """indices (N, 4) ints -> nbr (K, N) int32, rep (N) int32."""
    idx = np.asarray(indices, dtype=np.int64)
    N = idx.shape[0]
    S = tuple(int(s) for s in spatial_shape)

    def inside(b, c):
        return 0 <= b < batch_size and all(0 <= c[d] < S[d] for d in range(3))

    first = {}
    for i in range(N):
        b, c = int(idx[i, 0]), tuple(int(v) for v in idx[i, 1:])
        if inside(b, c):
            first.setdefault((b,) + c, i)
    offs = tap_offsets(ksize)
    nbr = np.full((len(offs), N), -1, dtype=np.int32)
    rep = np.arange(N, dtype=np.int32)
    for i in range(N):
        b, c = int(idx[i, 0]), tuple(int(v) for v in idx[i, 1:])
        if not inside(b, c):
            continue
        rep[i] = first[(b,) + c]
        for k, o in enumerate(offs):
            q = (c[0] + o[0], c[1] + o[1], c[2] + o[2])
            if inside(b, q):
                nbr[k, i] = first.get((b,) + q, -1)
    return nbr, rep


def _leaves(feat, weight, bias, dtype):
    f = torch.as_tensor(feat).to(dtype).clone().requires_grad_(True)
    w = torch.as_tensor(weight).to(dtype).clone().requires_grad_(True)
    b = torch.as_tensor(bias).to(dtype).clone().requires_grad_(True)
    return f, w, b


def _finish(out, f, w, b, grad_out, dtype):
    res = {"out": out.detach()}
    if grad_out is not None:
        gs = torch.autograd.grad(out, (f, w, b), torch.as_tensor(grad_out).to(dtype), allow_unused=True)
        gf, gw, gb = (torch.zeros_like(t) if g is None else g for g, t in zip(gs, (f, w, b)))
        res.update(grad_feat=gf, grad_weight=gw, grad_bias=gb)
    return res


def table_all(nbr, feat, weight, bias, grad_out=None, dtype=torch.float64):
    """out and the three gradients of the table model's forward, computed in `dtype`."""
    f, w, b = _leaves(feat, weight, bias, dtype)
    Cout, Cin = w.shape[0], w.shape[-1]
    wk = w.reshape(Cout, -1, Cin)
    N = f.shape[0]
    out = b.unsqueeze(0).expand(N, Cout)
    nb = torch.as_tensor(nbr).long()
    for k in range(nb.shape[0]):
        rows = torch.nonzero(nb[k] >= 0).squeeze(1)
        if rows.numel():
            out = out.index_add(0, rows, f.index_select(0, nb[k, rows]) @ wk[:, k, :].t())
    return _finish(out, f, w, b, grad_out, dtype)


def dense_all(indices, spatial_shape, batch_size, ksize, feat, weight, bias, grad_out=None, dtype=torch.float64):
    """The same through F.conv3d on the densified grid (sites inside the grid, one per voxel)."""
    f, w, b = _leaves(feat, weight, bias, dtype)
    idx = torch.as_tensor(np.asarray(indices, dtype=np.int64))
    S = [int(s) for s in spatial_shape]
    N, Cin = f.shape
    if N == 0:
        out = b.unsqueeze(0).expand(0, w.shape[0])
        return _finish(out, f, w, b, grad_out, dtype)
    grid = torch.zeros(batch_size, S[0], S[1], S[2], Cin, dtype=dtype)
    grid = grid.index_put((idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]), f)
    dense = F.conv3d(grid.permute(0, 4, 1, 2, 3), w.permute(0, 4, 1, 2, 3), b, padding=tuple(k // 2 for k in ksize))
    out = dense.permute(0, 2, 3, 4, 1)[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]]
    return _finish(out, f, w, b, grad_out, dtype)


def round_to(x, dtype):
    """x (float64 array / tensor) rounded to `dtype` and back to float64."""
    return torch.as_tensor(x).to(dtype).to(torch.float64)
