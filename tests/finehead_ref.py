"""The fine Gaussian head and the fine-set assembly restated in numpy (what csrc/finehead.hip computes), the reference's lines in
torch, and modules / points built from tests/golden/finehead_surface.json.  Nothing here reads the reference tree.

The head in float64 with a hand-written backward: x (N, C); w1 (C, C), w2 (P, C) in nn.Linear's layout, P = sh_dim + 8.
The assembly copies and adds in float32, as the lines it restates do, so its results are exact."""
import json
import math
import os

import numpy as np

SURFACE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "finehead_surface.json")
PARAMS = ("w1", "b1", "w2", "b2")
OUTPUTS = ("centers", "shs", "opacity", "scaling", "rotation")


def _erf(a):
    """erf in float64 (torch's CPU erf on the array: numpy has none; tests/test_finehead_cpu.py holds it against math.erf)"""
    import torch

    return torch.erf(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))).numpy()


def gelu(z):
    return 0.5 * z * (1.0 + _erf(z / math.sqrt(2.0)))


def gelu_slope(z):
    return 0.5 * (1.0 + _erf(z / math.sqrt(2.0))) + z * np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def head(x, w1, b1, w2, b2):
    """attribute (N, P)"""
    return gelu(x @ w1.T + b1) @ w2.T + b2


def head_grad(x, w1, b1, w2, b2, g):
    """the gradients of <g, head(x, ...)>, written out by hand: dx, dw1, db1, dw2, db2"""
    z1 = x @ w1.T + b1
    h = gelu(z1)
    dz1 = (g @ w2) * gelu_slope(z1)
    return {"dx": dz1 @ w1, "dw1": dz1.T @ x, "db1": dz1.sum(0), "dw2": g.T @ h, "db2": g.sum(0)}


def columns(sh_dim):
    """the attribute's columns behind each output: name -> (first column, width)"""
    return {"shs": (0, sh_dim), "opacity": (sh_dim, 1), "scaling": (sh_dim + 1, 3), "rotation": (sh_dim + 4, 4)}


def survivors(mask, selected):
    """the coarse row and the masked row of every survivor, in order"""
    rows = np.flatnonzero(mask)
    keep = np.flatnonzero(~selected)
    return rows[keep], keep


def assemble(levels, coarse, shs_fine, mask, selected, sh_dim, opacity_shift, scaling_shift):
    """levels: [(coord (n, 3) float32, attribute (n, P) of values of its dtype held in float32)]; coarse: centers, opacity, scaling,
    rotation (Nc, w) float32; shs_fine (n_masked, sh_dim / 3, 3) float32 -> the five float32 outputs"""
    f32 = np.float32
    cols = columns(sh_dim)
    rows, keep = survivors(mask, selected)
    shift = {"shs": None, "opacity": f32(opacity_shift), "scaling": f32(scaling_shift), "rotation": None}
    out = {"centers": np.concatenate([c.astype(f32) for c, _ in levels] + [coarse[0][rows]])}
    for (name, (a, w)), tail in zip(cols.items(), (shs_fine.reshape(-1, sh_dim)[keep], coarse[1][rows], coarse[2][rows], coarse[3][rows])):
        parts = [attr[:, a:a + w].astype(f32) for _, attr in levels]
        if shift[name] is not None:
            parts = [p + shift[name] for p in parts]
        out[name] = np.concatenate(parts + [tail.astype(f32)])
    out["shs"] = out["shs"].reshape(-1, sh_dim // 3, 3)
    return out


def assemble_grad(level_rows, Nc, mask, selected, sh_dim, grads):
    """grads: name -> (T, ...) float32 or None -> per level (dcoord, dattr (float32, before the cast to the attribute's dtype)),
    the four dense coarse gradients and dshs_fine"""
    f32 = np.float32
    cols = columns(sh_dim)
    rows, keep = survivors(mask, selected)
    L, T = sum(level_rows), sum(level_rows) + len(rows)
    g = {k: (np.zeros((T, w), f32) if grads.get(k) is None else np.asarray(grads[k], f32).reshape(T, w))
         for k, w in (("centers", 3), ("shs", sh_dim), ("opacity", 1), ("scaling", 3), ("rotation", 4))}
    levels, at = [], 0
    for n in level_rows:
        dattr = np.concatenate([g[k][at:at + n] for k in cols], axis=1)
        levels.append((g["centers"][at:at + n].copy(), dattr))
        at += n
    dense = []
    for k, w in (("centers", 3), ("opacity", 1), ("scaling", 3), ("rotation", 4)):
        d = np.zeros((Nc, w), f32)
        d[rows] = g[k][L:]
        dense.append(d)
    dfine = np.zeros((len(selected), sh_dim), f32)
    dfine[keep] = g["shs"][L:]
    return levels, dense, dfine.reshape(-1, sh_dim // 3, 3)


# ---- the reference's lines in torch, and objects with the recorded surface -------------------------------------------------------

def surface():
    with open(SURFACE) as f:
        return json.load(f)


def make_module(kind, C, sh_degree, is_first=True, enable_residual_attribute=False, layers=None):
    """a module with the recorded attributes and `feat2attr` layer list of GaussianModule / GaussianResModule (or `layers`, a list
    of nn.Modules, in its place)"""
    from torch import nn

    s = surface()[kind]
    values = {"dim": C, "num_sh": 3 * (sh_degree + 1) ** 2}

    class Module(nn.Module):
        pass

    m = Module()
    m.dim, m.sh_degree, m.num_sh, m.is_first, m.enable_residual_attribute = C, sh_degree, values["num_sh"], is_first, enable_residual_attribute
    if layers is None:
        act = {"nn.GELU": nn.GELU}[s["init"]["defaults"]["act_layer"]]
        layers = []
        for layer in s["feat2attr"]["layers"]:
            args = [sum(values[n] for n in a["names"]) + a["plus"] for a in layer["args"]]
            layers.append(act() if layer["type"] == "act_layer" else getattr(nn, layer["type"])(*args))
    m.feat2attr = getattr(nn, s["feat2attr"]["constructor"])(*layers)
    return m


class Point(dict):
    """a dict with attribute access, as the reference's Point is"""
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def reference_module_forward(self, point):
    """GaussianModule.forward, written from the recorded surface"""
    point.leaf_point.update({"attribute": self.feat2attr(point.leaf_point.feat)})
    return point


def reference_res_module_forward(self, point):
    """GaussianResModule.forward, written from the recorded surface"""
    attribute = self.feat2attr(point.feat)
    if self.enable_residual_attribute and not self.is_first:
        attribute = point.attribute + attribute
    point.update({"attribute": attribute})
    return point


ASSEMBLE_MUTANTS = ("levels_not_sorted_by_batch", "shifts_swapped")


def reference_assemble(levels, coarse, shs_fine, mask, selected, sh_dim, opacity_shift, scaling_shift, offsets=None, mut=None):
    """`_union_gaussians` (the concatenation by group with its stable sort) and the five concatenations behind it, written from
    the recorded surface: the lines the GPU tests compare against, bit for bit.  offsets: per level the segment ends of its rows
    (None: one sample).  `mut` switches one deliberate mistake on."""
    import torch

    assert mut in (None,) + ASSEMBLE_MUTANTS
    if offsets is None:
        batches = [torch.zeros(c.shape[0], dtype=torch.long, device=c.device) for c, _ in levels]
    else:
        batches = [torch.searchsorted(o, torch.arange(c.shape[0], device=c.device), right=True) for (c, _), o in zip(levels, offsets)]
    index, perm = torch.cat(batches).sort(stable=True)
    if mut == "levels_not_sorted_by_batch":
        perm = torch.arange(perm.shape[0], device=perm.device)
    if mut == "shifts_swapped":
        opacity_shift, scaling_shift = scaling_shift, opacity_shift
    xyz = torch.cat([c for c, _ in levels], 0)[perm]
    attribute = torch.cat([a for _, a in levels], 0)[perm]
    sh, opacity, scaling, rotation = torch.split(attribute, [sh_dim, 1, 3, 4], dim=-1)
    centers_c, opacity_c, scaling_c, rotation_c = coarse
    return (torch.cat([xyz, centers_c[mask][~selected]], dim=0),
            torch.cat([sh.view(xyz.shape[0], sh_dim // 3, 3).float(), shs_fine[~selected]], dim=0),
            torch.cat([opacity.float() + opacity_shift, opacity_c[mask][~selected]], dim=0),
            torch.cat([scaling.float() + scaling_shift, scaling_c[mask][~selected]], dim=0),
            torch.cat([rotation.float(), rotation_c[mask][~selected]], dim=0))
