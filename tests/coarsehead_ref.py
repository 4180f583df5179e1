"""The coarse Gaussian head restated in numpy float64 with a hand-written backward (what csrc/coarsehead.hip computes), the
reference's literal lines in torch, and a Decoder-shaped module built from tests/golden/coarsehead_surface.json.  Nothing here
reads the reference tree.

Shapes: x (B, N, C); w1, w2 (C, C), w3 (K P, C) in nn.Linear's layout, P = 3 + sh_dim + 1 + 3 + 4; with E = N K the results are
offset (B, E, 3), sh (B, E, sh_dim / 3, 3), scaling (B, E, 3), rotation (B, E, 4), opacity (B, E, 1), centers (B, E, 3),
mask (B, E)."""
import json
import os

import numpy as np

SURFACE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coarsehead_surface.json")
OUTPUTS = ("offset", "sh", "scaling", "rotation", "opacity")
PARAMS = ("w1", "b1", "w2", "b2", "w3", "b3")


def sigmoid(v):
    return np.where(v >= 0, 1.0 / (1.0 + np.exp(-np.abs(v))), np.exp(-np.abs(v)) / (1.0 + np.exp(-np.abs(v))))


def columns(K, sh_dim):
    """the columns of the (K, P) last layer behind each output: name -> (first column, width)"""
    return {"offset": (0, 3), "sh": (3, sh_dim), "opacity": (3 + sh_dim, 1), "scaling": (4 + sh_dim, 3), "rotation": (7 + sh_dim, 4)}


def hidden(x, w1, b1, w2, b2):
    z1 = x @ w1.T + b1
    h1 = np.maximum(z1, 0.0)
    z2 = h1 @ w2.T + b2
    return z1, h1, z2, np.maximum(z2, 0.0)


def head(x, w1, b1, w2, b2, w3, b3, K, sh_dim, opacity_shift, scaling_shift, group_centers=None, half_cell=0.0, threshold=0.005):
    """every output; with group_centers (N, 3) also centers and mask"""
    B, N, C = x.shape
    P = sh_dim + 11
    z1, h1, z2, h2 = hidden(x, w1, b1, w2, b2)
    v = (h2 @ w3.T + b3).reshape(B, N * K, P)
    cols = columns(K, sh_dim)
    res = {name: v[..., a:a + w].copy() for name, (a, w) in cols.items()}
    res["offset"] = 2.0 * sigmoid(res["offset"]) - 1.0
    res["opacity"] = res["opacity"] + opacity_shift
    res["scaling"] = res["scaling"] + scaling_shift
    res["sh"] = res["sh"].reshape(B, N * K, sh_dim // 3, 3)
    if group_centers is not None:
        res["centers"] = np.repeat(group_centers.reshape(N, 3), K, axis=0)[None] + res["offset"] * half_cell
        res["mask"] = sigmoid(res["opacity"][..., 0]) > threshold
    return res


def head_grad(x, w1, b1, w2, b2, w3, b3, K, sh_dim, grads, half_cell=0.0):
    """the gradients of sum over outputs of <grads[name], output> (grads: name -> array or None, names of OUTPUTS and
    "centers"), written out by hand: dx, dw1, db1, dw2, db2, dw3, db3"""
    B, N, C = x.shape
    P = sh_dim + 11
    z1, h1, z2, h2 = hidden(x, w1, b1, w2, b2)
    v = (h2 @ w3.T + b3).reshape(B, N * K, P)
    dv = np.zeros_like(v)
    for name, (a, w) in columns(K, sh_dim).items():
        g = grads.get(name)
        if g is not None:
            dv[..., a:a + w] += np.asarray(g, dtype=np.float64).reshape(B, N * K, w)
    if grads.get("centers") is not None:
        dv[..., 0:3] += np.asarray(grads["centers"], dtype=np.float64) * half_cell
    s = sigmoid(v[..., 0:3])
    dv[..., 0:3] *= 2.0 * s * (1.0 - s)
    dz3 = dv.reshape(B * N, K * P)
    xr, h1r, h2r = x.reshape(B * N, C), h1.reshape(B * N, C), h2.reshape(B * N, C)
    dz2 = (dz3 @ w3) * (z2.reshape(B * N, C) > 0)
    dz1 = (dz2 @ w2) * (z1.reshape(B * N, C) > 0)
    return {"dx": (dz1 @ w1).reshape(B, N, C), "dw1": dz1.T @ xr, "db1": dz1.sum(0), "dw2": dz2.T @ h1r, "db2": dz2.sum(0),
            "dw3": dz3.T @ h2r, "db3": dz3.sum(0)}


# ---- the reference's lines in torch, and a module with the Decoder's surface ---------------------------------------------------

def surface():
    with open(SURFACE) as f:
        return json.load(f)


def make_decoder(C, K, sh_dim, layers=None):
    """a module with the attributes the recorded Decoder.__init__ assigns and the recorded layer list of mlp_coarse (or
    `layers`, a list of nn.Modules, in its place)"""
    from torch import nn

    s = surface()
    values = {"in_dim": C, "sh_dim": sh_dim, "scaling_dim": 3, "rotation_dim": 4, "opacity_dim": 1, "K": K}
    values["out_dim"] = 3 + sh_dim + 1 + 3 + 4

    def size(names):
        n = 1
        for name in names:
            n *= values[name]
        return n

    class Decoder(nn.Module):
        pass

    m = Decoder()
    for attr, param in s["init"]["attributes"].items():
        setattr(m, attr, values[param])
    if layers is None:
        layers = [getattr(nn, layer["type"])(*[size(a) for a in layer["args"]]) for layer in s["mlp_coarse"]["layers"]]
    m.mlp_coarse = getattr(nn, s["mlp_coarse"]["constructor"])(*layers)
    return m


def reference_forward_coarse(self, feats, opacity_shift, scaling_shift, float64=False):
    """the composition Decoder.forward_coarse is: the lines the tests compare against, written from the recorded surface
    (float64: without the cast to float32, for the comparison with the float64 restatement)"""
    import torch

    parameters = self.mlp_coarse(feats)
    parameters = parameters if float64 else parameters.float()
    parameters = parameters.view(*parameters.shape[:-1], self.K, -1)
    offset, sh, opacity, scaling, rotation = torch.split(
        parameters, [3, self.sh_dim, self.opacity_dim, self.scaling_dim, self.rotation_dim], dim=-1)
    opacity = opacity + opacity_shift
    scaling = scaling + scaling_shift
    offset = torch.sigmoid(offset) * 2 - 1.0
    B = opacity.shape[0]
    sh = sh.view(B, -1, self.sh_dim // 3, 3)
    opacity = opacity.view(B, -1, self.opacity_dim)
    scaling = scaling.view(B, -1, self.scaling_dim)
    rotation = rotation.view(B, -1, self.rotation_dim)
    offset = offset.view(B, -1, 3)
    return offset, sh, scaling, rotation, opacity


def reference_tail(offset, opacity, group_centers, half_cell, K, threshold=0.005):
    """the three lines behind forward_coarse: the offset centres and the opacity mask; group_centers (1, N, 3)"""
    import torch

    B = offset.shape[0]
    centers = group_centers.unsqueeze(-2).expand(B, -1, K, -1).reshape(offset.shape) + offset * half_cell
    return centers, torch.sigmoid(opacity).squeeze(-1) > threshold
