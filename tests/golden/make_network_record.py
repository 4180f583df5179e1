#!/usr/bin/env python
"""tests/golden/make_network_record.py — generates tests/golden/network_*.npz: forwards and backwards of the reference's own
decoder classes (lightning/network.py), run in float64 on the CPU.  Authoring only: it needs a checkout of the reference next
to this repository (or at $GD_REFERENCE_ROOT).  The tests read the files and never the reference (tests/network_record.py).

network.py is plain torch; it is loaded by path with a few lines of stand-ins for the packages its module body imports and
these classes never use (timm, pytorch_lightning with LightningModule = torch.nn.Module, torchvision, PIL, lightning.renderer,
lightning.utils, lightning.point_decoder.*).  tools/rsh.py is loaded for real.  Nothing of the reference is copied: a file holds
arrays, names, shapes and scalar settings.

Records (one file per case; `_pgrad*` files hold the parameter gradients of a case whose float64 arrays exceed the size cap):
    group_block_h4, group_block_h2   GroupAttBlock(32, 24, heads, eps=1e-6).forward: 4 heads of 8, 2 heads of 16 (the reference's)
    vol_transformer                  VolTransformer(16, 24, [2, 4], 4, 8, 8, 2, 2).forward, and the cond every layer was handed
    mod_ln                           ModLN(24, 32, eps=1e-6).forward
    feat_vol                         Network.build_feat_vol / ray_to_plucker / build_dense_grid, unbound on a SimpleNamespace
    coarse_k1, coarse_k2             Decoder(80, 12, 3, 4, 1, K).forward_coarse, then Network.get_offseted_pt
    fine_v2, fine_v4                 the K = 1 Decoder's forward_fine over 2 and 4 views
    point_feats                      Network.get_point_feats, unbound on a SimpleNamespace (no golden held a number it produced)

Every recorded input, upstream gradient and parameter is a bfloat16-representable value inside float16's normal range, so one
record is the float64 truth "on the inputs as rounded to their dtypes" for float32, bfloat16 and float16 runs alike.  Biases
and LayerNorm affines are moved off their initial values; a quarter of the rows a LayerNorm reads have a variance near 1e-3, where
an eps of 1e-6 in place of 1e-5 moves the result by about half a per cent.  The inputs keep clear of the kinks a 16-bit run would
cross (see low_variance_rows, clear_of_relu_kinks, point_feats): the Decoder's ReLU pre-activations stay 0.05 from zero, the points
of get_point_feats 0.02 px from an integer position and 0.02 from a zero depth difference.

The one liberty: inside build_feat_vol, `Tensor.float()` is the identity on float64 tensors while the record is taken
(F.grid_sample refuses a float32 map with a float64 grid).  forward_coarse and forward_fine keep their `.float()`: those
outputs are recorded as the float32 values the reference returns.

Widths: the Decoder has the reference's (80 wide, 16 heads of 5, sh_degree 1).  The block and the transformer cannot (at 256
channels the convolution alone has 1.8 M weights): the block is 32 wide, as in tests/test_gpu_conv3d.py, the transformer 16 wide
with 2 layers, all inside the envelopes of groupattn, conv3d and deconv3d.  Not narrower: the GPU tests judge max|error| against
twice torch's, and over an 8-element vector (a LayerNorm affine of an 8-wide transformer) that ratio of two maxima measured
above 2 in 1.4 % of the pairs over fresh upstream gradients, with a median of 0.9, and never over a longer tensor.

Usage: python tests/golden/make_network_record.py        (prints every file's size; running it twice gives the same arrays)
"""
import glob
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("GD_REFERENCE_ROOT",
                     os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(HERE))), "reference"))
CAP = 256 * 1024
sys.path.insert(0, os.path.dirname(HERE))

from network_record import (block_attrs, decoder_attrs, float_is_identity_on_float64, mod_ln_attrs,  # noqa: E402
                            transformer_attrs)


def load_network():
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        m.__path__ = []
        sys.modules[name] = m
        return m

    class _Any:
        def __init__(self, *a, **k):
            pass

    def by_path(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod

    stub("timm")
    stub("pytorch_lightning", LightningModule=torch.nn.Module)
    stub("torchvision", transforms=types.SimpleNamespace())
    try:
        import PIL.Image  # noqa: F401
    except ImportError:
        stub("PIL", Image=_Any)
    stub("lightning")
    stub("lightning.renderer", Renderer=_Any)
    stub("lightning.utils", MiniCam=_Any)
    stub("lightning.point_decoder")
    stub("lightning.point_decoder.utils")
    stub("lightning.point_decoder.utils.structure", Point=_Any)
    stub("lightning.point_decoder.utils.modules", PointModule=torch.nn.Module, PointSequential=torch.nn.Sequential)
    stub("lightning.point_decoder.autoencoder")
    stub("lightning.point_decoder.utils.misc", offset2batch=None, batch2offset=None)
    stub("tools")
    by_path("tools.rsh", os.path.join(REF, "tools", "rsh.py"))
    return by_path("lightning.network", os.path.join(REF, "lightning", "network.py"))


# ---- values -------------------------------------------------------------------------------------------------------------------

TINY = 2.0 ** -14          # float16's smallest normal


def q(t):
    """t rounded to bfloat16 and kept inside float16's normal range, as float64"""
    t = torch.as_tensor(t, dtype=torch.float64).detach().to(torch.bfloat16).to(torch.float64)
    small = t.abs() < TINY
    t = torch.where(small, torch.where(t < 0, -TINY, TINY).to(t), t)
    assert float(t.abs().max()) < 60000 and torch.equal(t, t.to(torch.float16).to(torch.float64))
    return t


def randn(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=torch.float64)


def low_variance_rows(gen, rows, positions=None):
    """rows (R, C) with every fourth row (by its position) replaced by 0.03 N(0, 1) around a level of the same size: a variance
    near 1e-3.  The level is not larger: with a level c >> 0.03, x - mean cancels log2(c / 0.03) bits in any float32 LayerNorm,
    those rows would carry all of a float32 run's error, and the comparison of two runs would measure which summation order was
    lucky on them."""
    rows = rows.clone()
    positions = torch.arange(rows.shape[0]) if positions is None else positions
    pick = positions % 4 == 1
    n = int(pick.sum())
    rows[pick] = 0.03 * randn(gen, n, 1) + 0.03 * randn(gen, n, rows.shape[1])
    return rows


RELU_MARGIN = 0.05


def clear_of_relu_kinks(gen, rows, redraw, preacts, margin=RELU_MARGIN):
    """rows: a tuple of (N, ...) tensors of rounded values; preacts(*rows) -> (N, units), what the ReLUs of the run see;
    redraw(gen, positions) -> fresh rows for those positions.  Redraws every row with a pre-activation within `margin` of zero.
    A 16-bit run carries an error of a few 1e-2 there (2^-9 of ~80 terms of size one): it would switch such a unit, and the
    largest error of a gradient would then be the size of the switched term in whichever run was unlucky, not its arithmetic."""
    rows = [r.clone() for r in rows]
    for _ in range(20000):
        with torch.no_grad():
            bad = ((preacts(*rows).abs() < margin).any(-1)).nonzero().reshape(-1)
        if not bad.numel():
            return rows
        for r, fresh in zip(rows, redraw(gen, bad)):
            r[bad] = fresh
    raise AssertionError("no draw clear of the ReLU kinks")


def set_parameters(module, gen):
    """seeded values for every parameter, rounded: LayerNorm weights around 1, every other vector (biases) around 0, matrices
    and kernels scaled by their fan-in"""
    with torch.no_grad():
        for name, p in module.named_parameters():
            leaf = name.split(".")[-1]
            owner = module.get_submodule(name.rsplit(".", 1)[0]) if "." in name else module
            if p.dim() == 1:
                centre = 1.0 if isinstance(owner, torch.nn.LayerNorm) and leaf == "weight" else 0.0
                p.copy_(q(centre + 0.2 * randn(gen, *p.shape)))
            elif name == "pos_embed":
                C = p.shape[1]
                rows = low_variance_rows(gen, randn(gen, p[0, 0].numel(), C) * (1.0 / C) ** 0.5 * 4)
                p.copy_(q(rows.T.reshape(p.shape)))
            else:
                p.copy_(q(randn(gen, *p.shape) * (1.2 / p[0].numel() ** 0.5)))


def volume(gen, B, C, D):
    """(B, C, D, D, D) with low-variance voxels"""
    rows = low_variance_rows(gen, randn(gen, B * D ** 3, C) * 1.5 + 0.2)
    return q(rows.reshape(B, D, D, D, C).permute(0, 4, 1, 2, 3).contiguous())


# ---- one record ---------------------------------------------------------------------------------------------------------------

def np64(t):
    return t.detach().to(torch.float64).numpy().copy()


def record(name, meta, module, inputs, outputs, ups, grad_inputs, extra_outputs=None, constants=()):
    """module: the live instance (state_dict and parameter gradients are taken from it); inputs: name -> tensor (rounded values);
    outputs: name -> tensor; ups: name -> upstream gradient of that output; grad_inputs: name -> leaf whose .grad is recorded;
    constants: the inputs the reference computed itself in float32 (a grid), kept as they are"""
    loss = sum((o.to(torch.float64) * ups[k]).sum() for k, o in outputs.items() if k in ups)
    loss.backward()
    main, pgrad = {"meta": np.array(json.dumps(meta, sort_keys=True))}, {}
    for k, v in module.state_dict().items():
        assert torch.equal(v.double(), q(v)), k
        main["state/" + k] = v.detach().to(torch.float32).numpy()
    for k, v in inputs.items():
        if v.dtype.is_floating_point:
            assert torch.equal(v.double(), v.float().double() if k in constants else q(v)), k
            main["in/" + k] = v.detach().to(torch.float32).numpy()
        else:
            main["in/" + k] = v.numpy()
    for k, v in ups.items():
        assert torch.equal(v, q(v)), k
        main["up/" + k] = v.to(torch.float32).numpy()
    for k, v in {**outputs, **(extra_outputs or {})}.items():
        main["out/" + k] = np64(v)
    for k, v in grad_inputs.items():
        main["gin/" + k] = np64(v.grad)
    for k, p in module.named_parameters():
        if p.grad is not None:
            pgrad["gparam/" + k] = np64(p.grad)
    for a in list(main.values()) + list(pgrad.values()):
        assert a.dtype.kind in "USi" or np.isfinite(a).all()
    path = os.path.join(HERE, f"network_{name}.npz")
    for old in glob.glob(os.path.join(HERE, f"network_{name}_pgrad*.npz")):
        os.remove(old)
    np.savez_compressed(path, **main, **pgrad)
    written = [path]
    if os.path.getsize(path) > CAP:     # float64 does not compress: the parameter gradients move out, largest first, file by file
        np.savez_compressed(path, **main)
        parts = []
        for k in sorted(pgrad, key=lambda k: -pgrad[k].nbytes):
            part = next((p for p in parts if sum(pgrad[j].nbytes for j in p) + pgrad[k].nbytes <= CAP - 8192), None)
            if part is None:
                parts.append([k])
            else:
                part.append(k)
        for i, part in enumerate(parts):
            side = os.path.join(HERE, f"network_{name}_pgrad{i if i else ''}.npz")
            np.savez_compressed(side, **{k: pgrad[k] for k in part})
            written.append(side)
    for p in written:
        size = os.path.getsize(p)
        print(f"{os.path.relpath(p, os.path.dirname(os.path.dirname(HERE)))}: {size} bytes")
        assert size <= CAP, (p, size)


def group_block(net, name, C, cond_dim, heads, D, bs, B, Lk, seed):
    gen = torch.Generator().manual_seed(seed)
    ctor = {"inner_dim": C, "cond_dim": cond_dim, "num_heads": heads, "eps": 1e-6}
    blk = net.GroupAttBlock(**ctor).double()
    set_parameters(blk, gen)
    G = (D // bs) ** 3
    x = volume(gen, B, C, D).requires_grad_(True)
    cond = q(randn(gen, B * G, Lk, cond_dim)).requires_grad_(True)
    out = blk(x, cond, D // bs, bs)
    meta = {"item": "group_block", "ctor": ctor, "attrs": block_attrs(blk), "call": {"group_axis": D // bs, "block_size": bs}}
    record(name, meta, blk, {"x": x, "cond": cond}, {"out": out}, {"out": q(randn(gen, *out.shape))}, {"x": x, "cond": cond})


def vol_transformer(net, seed):
    gen = torch.Generator().manual_seed(seed)
    ctor = {"embed_dim": 16, "image_feat_dim": 24, "n_groups": [2, 4], "vol_low_res": 4, "vol_high_res": 8, "out_dim": 8,
            "num_layers": 2, "num_heads": 2}
    vt = net.VolTransformer(**ctor).double()
    set_parameters(vt, gen)
    B, V = 2, 2
    feats = q(randn(gen, B, V, 24, 4, 4, 4)).requires_grad_(True)
    seen = []
    hooks = [layer.register_forward_pre_hook(lambda mod, args: seen.append(args)) for layer in vt.layers]
    out = vt(feats)
    for h in hooks:
        h.remove()
    conds = {f"cond_layer{i}": a[1] for i, a in enumerate(seen)}
    attrs = dict(transformer_attrs(vt), layer_calls=[{"group_axis": a[2], "block_size": a[3]} for a in seen])
    meta = {"item": "vol_transformer", "ctor": ctor, "attrs": attrs, "call": {}}
    record("vol_transformer", meta, vt, {"image_feats": feats}, {"out": out}, {"out": q(randn(gen, *out.shape))},
           {"image_feats": feats}, extra_outputs=conds)


def mod_ln(net, seed):
    gen = torch.Generator().manual_seed(seed)
    ctor = {"inner_dim": 24, "mod_dim": 32, "eps": 1e-6}
    m = net.ModLN(**ctor).double()
    set_parameters(m, gen)
    x = q(low_variance_rows(gen, randn(gen, 30, 24) * 1.3 - 0.1).reshape(2, 3, 5, 24)).requires_grad_(True)
    cond = q(randn(gen, 2, 3, 5, 32)).requires_grad_(True)
    out = m(x, cond)
    meta = {"item": "mod_ln", "ctor": ctor, "attrs": mod_ln_attrs(m), "call": {}}
    record("mod_ln", meta, m, {"x": x, "cond": cond}, {"out": out}, {"out": q(randn(gen, *out.shape))}, {"x": x, "cond": cond})


def feat_vol(net, seed):
    import volcond_cases as VC

    gen = torch.Generator().manual_seed(seed)
    Bn, Vn, views, (h, w), img_hw, Cn, r = 2, 2, 4, (3, 5), (48, 80), 24, 4
    ctor = {"inner_dim": Cn, "mod_dim": 32, "eps": 1e-6}
    dir_norm = net.ModLN(**ctor).double()
    set_parameters(dir_norm, gen)
    me = types.SimpleNamespace(dir_norm=dir_norm, feat_vol_reso=r, scene_size=0.5, device=torch.device("cpu"))
    me.ray_to_plucker = lambda rays: net.Network.ray_to_plucker(me, rays)
    grid = net.Network.build_dense_grid(me, r)
    me.volume_grid = grid.double()
    w2cs, ixts = VC.orbit_cameras(Bn * views, img_hw)
    batch = {"tar_w2c": q(w2cs).view(Bn, views, 4, 4), "tar_ixt": q(ixts).view(Bn, views, 3, 3),
             "tar_rays_down": q(torch.cat([randn(gen, Bn, views, h, w, 3) * 1.2, randn(gen, Bn, views, h, w, 3)], -1))}
    src_inps = torch.zeros(Bn * Vn, 3, *img_hw, dtype=torch.float64)
    img_feats = q(low_variance_rows(gen, randn(gen, Bn * Vn * h * w, Cn)).reshape(Bn * Vn, h, w, Cn).permute(0, 3, 1, 2).contiguous())
    img_feats.requires_grad_(True)
    with float_is_identity_on_float64():
        out = net.Network.build_feat_vol(me, src_inps, img_feats, Vn, batch)
    assert out.dtype == torch.float64 and out.shape == (Bn, Vn, Cn, r, r, r)
    rays = batch["tar_rays_down"][:, :Vn]
    plucker = net.Network.ray_to_plucker(me, rays)
    feats_dir = torch.cat((net.rsh_cart_3(plucker[..., :3]), net.rsh_cart_3(plucker[..., 3:6])), dim=-1)
    meta = {"item": "feat_vol", "ctor": ctor, "call": {"n_views_sel": Vn, "img_hw": list(img_hw)},
            "attrs": dict(mod_ln_attrs(dir_norm), feat_vol_reso=r, scene_size=0.5, volume_grid_dtype=str(grid.dtype))}
    record("feat_vol", meta, dir_norm, {"img_feats": img_feats, **batch}, {"out": out}, {"out": q(randn(gen, *out.shape))},
           {"img_feats": img_feats}, extra_outputs={"volume_grid": grid, "feats_dir": feats_dir})


DECODER = {"in_dim": 80, "sh_dim": 12, "scaling_dim": 3, "rotation_dim": 4, "opacity_dim": 1}


def make_decoder(net, K):
    """the same seed for every record of one K: coarse_k1, fine_v2 and fine_v4 hold one Decoder"""
    dec = net.Decoder(**DECODER, K=K).double()
    set_parameters(dec, torch.Generator().manual_seed(500 + K))
    return dec


def coarse(net, K, seed):
    gen = torch.Generator().manual_seed(seed)
    dec = make_decoder(net, K)
    B, reso, grid_reso, n_offset_groups = 2, 3, 32, 32
    voxel_size = 2.0 / (grid_reso * 2)
    opacity_shift, scaling_shift = -2.1792, float(np.log(0.5 * voxel_size / 3.0))
    me = types.SimpleNamespace(scene_size=0.5, n_offset_groups=n_offset_groups, device=torch.device("cpu"))
    centers = net.Network.build_dense_grid(me, reso).reshape(1, -1, 3)
    me.group_centers = centers.double()
    mlp = dec.mlp_coarse

    def preacts(f):
        z1 = mlp[0](f)
        return torch.cat((z1, mlp[2](mlp[1](z1))), dim=-1)

    feats, = clear_of_relu_kinks(gen, (q(randn(gen, B * reso ** 3, 80)),), lambda g, pos: (q(randn(g, len(pos), 80)),), preacts)
    feats = feats.reshape(B, reso, reso, reso, 80).requires_grad_(True)
    outs = dict(zip(("offset", "sh", "scaling", "rotation", "opacity"), dec.forward_coarse(feats, opacity_shift, scaling_shift)))
    outs["centers"] = net.Network.get_offseted_pt(me, outs["offset"], K)
    assert all(o.dtype == torch.float32 for k, o in outs.items() if k != "centers")
    meta = {"item": "coarse", "ctor": dict(DECODER, K=K), "attrs": decoder_attrs(dec),
            "call": {"opacity_shift": opacity_shift, "scaling_shift": scaling_shift, "half_cell": 0.5 * me.scene_size / n_offset_groups,
                     "out_dtypes": {k: str(o.dtype) for k, o in outs.items()}}}
    record(f"coarse_k{K}", meta, dec, {"feats": feats, "group_centers": me.group_centers}, outs,
           {k: q(randn(gen, *o.shape)) for k, o in outs.items()}, {"feats": feats}, constants=("group_centers",))


def fine(net, V, seed):
    gen = torch.Generator().manual_seed(seed)
    dec = make_decoder(net, 1)
    N = 37

    def draw(g, pos):
        return q(low_variance_rows(g, randn(g, len(pos), 80), pos)), q(randn(g, len(pos), V, 8))

    def preacts(vf, pf):
        return dec.mlp_fine[0](dec.cross_att(dec.norm(vf.unsqueeze(1)), pf, pf, need_weights=False)[0])[:, 0]

    volume_feat, point_feats = clear_of_relu_kinks(gen, draw(gen, torch.arange(N)), draw, preacts)
    volume_feat, point_feats = volume_feat.requires_grad_(True), point_feats.requires_grad_(True)
    outs = dict(zip(("features", "sh"), dec.forward_fine(volume_feat, point_feats)))
    assert all(o.dtype == torch.float32 for o in outs.values())
    meta = {"item": "fine", "ctor": dict(DECODER, K=1), "attrs": decoder_attrs(dec),
            "call": {"out_dtypes": {k: str(o.dtype) for k, o in outs.items()}}}
    record(f"fine_v{V}", meta, dec, {"volume_feat": volume_feat, "point_feats": point_feats}, outs,
           {k: q(randn(gen, *o.shape)) for k, o in outs.items()}, {"volume_feat": volume_feat, "point_feats": point_feats})


def point_feats(net, seed):
    import pointfeat_ref as PR

    gen = torch.Generator().manual_seed(seed)
    Bn, views, Vn, H, W, n_all, idx = 2, 4, 3, 12, 20, 48, 1
    w2cs, ixts = (q(a) for a in PR.cameras(Bn * views, H, W))
    batch = {"tar_w2c": w2cs.view(Bn, views, 4, 4), "tar_ixt": ixts.view(Bn, views, 3, 3)}
    inp = PR.make_inputs(n_all, Vn, H, W, seed=seed)
    leaves = {k: q(inp[k]).requires_grad_(True) for k in ("img_ref", "image", "acc_map", "depth")}
    mask = torch.rand(n_all, generator=gen) < 0.7
    points = q(torch.rand(n_all, 3, generator=gen, dtype=torch.float64) - 0.5)
    me = types.SimpleNamespace(device=torch.device("cpu"))
    renderings = {k: leaves[k] for k in ("image", "acc_map", "depth")}
    for _ in range(1000):     # redraw the points at a kink: near an integer position in a view, or |depth sample - z| near zero
        with torch.no_grad():
            xy, _z = net.projection(points, batch["tar_w2c"][idx, :Vn], batch["tar_ixt"][idx, :Vn])
            every, _ = net.Network.get_point_feats(me, idx, leaves["img_ref"], renderings, Vn, batch, points, torch.ones(n_all, dtype=torch.bool))
        near = ((xy - xy.round()).abs() < 0.02).any(-1).any(0) | (every[:, 7] < 0.02).any(0)
        if not near.any():
            break
        points[near] = q(torch.rand(int(near.sum()), 3, generator=gen, dtype=torch.float64) - 0.5)
    assert not near.any()
    points.requires_grad_(True)
    out, mask_out = net.Network.get_point_feats(me, idx, leaves["img_ref"], renderings, Vn, batch, points, mask)
    assert out.shape == (Vn, 8, int(mask.sum())) and mask_out is mask
    meta = {"item": "point_feats", "ctor": {}, "attrs": {}, "call": {"idx": idx, "n_views_sel": Vn}}
    record("point_feats", meta, torch.nn.Module(), {**leaves, "points": points, "mask": mask, **batch}, {"point_feats": out},
           {"point_feats": q(randn(gen, *out.shape))}, {**leaves, "points": points})


def main():
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    net = load_network()
    group_block(net, "group_block_h4", 32, 24, 4, 4, 2, 2, 5, seed=11)
    group_block(net, "group_block_h2", 32, 24, 2, 4, 2, 2, 3, seed=12)
    vol_transformer(net, seed=21)
    mod_ln(net, seed=31)
    feat_vol(net, seed=41)
    for K in (1, 2):
        coarse(net, K, seed=50 + K)
    for V in (2, 4):
        fine(net, V, seed=60 + V)
    point_feats(net, seed=71)


if __name__ == "__main__":
    main()
