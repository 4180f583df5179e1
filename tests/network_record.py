"""Reads tests/golden/network_*.npz (forwards and backwards of the reference's own decoder classes in float64, written by
tests/golden/make_network_record.py), builds the matching stand-in from the builders of tests/*_ref.py, loads the recorded
state_dict into it with strict=True, and runs a forward (the yardstick's or the product's) over the recorded inputs and upstream
gradients.  The strict load is itself a check: the names and shapes of a reference checkpoint fit what the bound forwards read.
Nothing here reads the reference tree.

A record: meta (item, ctor, attrs of the live instance, call), state (name -> float32 array, exact), inputs, ups (the upstream
gradient per output), outputs, gin (the gradient of every differentiated input) and gparam (of every parameter that got one),
the last three float64.  `run` returns {"out/<name>", "gin/<name>", "gparam/<name>"}: the keys of `expected`.
"""
import contextlib
import glob
import json
import os
import types

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RECORDS = ("group_block_h4", "group_block_h2", "vol_transformer", "mod_ln", "feat_vol", "coarse_k1", "coarse_k2", "fine_v2", "fine_v4",
           "point_feats")
COARSE_OUTPUTS = ("offset", "sh", "scaling", "rotation", "opacity")

_CACHE = {}


def load(name):
    """the record `name` (read once, shared and left unchanged): a SimpleNamespace of dicts of numpy arrays"""
    if name not in _CACHE:
        arrays = {}
        for path in [os.path.join(GOLDEN, f"network_{name}.npz")] + sorted(glob.glob(os.path.join(GOLDEN, f"network_{name}_pgrad*.npz"))):
            with np.load(path) as f:
                arrays.update({k: f[k] for k in f.files})
        rec = types.SimpleNamespace(name=name, meta=json.loads(str(arrays.pop("meta"))), state={}, inputs={}, ups={}, outputs={},
                                    gin={}, gparam={})
        kinds = {"state": rec.state, "in": rec.inputs, "up": rec.ups, "out": rec.outputs, "gin": rec.gin, "gparam": rec.gparam}
        for key, a in arrays.items():
            kind, rest = key.split("/", 1)
            a = a.astype(np.float64) if a.dtype.kind == "f" and kind != "state" else a
            a.setflags(write=False)
            kinds[kind][rest] = a
        rec.item = rec.meta["item"]
        _CACHE[name] = rec
    return _CACHE[name]


def expected(rec):
    """every recorded output and gradient: {"out/..", "gin/..", "gparam/.."} -> float64 array"""
    res = {"out/" + k: v for k, v in rec.outputs.items()}
    res.update({"gin/" + k: v for k, v in rec.gin.items()})
    res.update({"gparam/" + k: v for k, v in rec.gparam.items()})
    return res


# ---- the attributes the forwards read, taken from an instance (the recorder takes them from the reference's) ---------------------

def norm_eps(module):
    from torch import nn

    return {n: m.eps for n, m in module.named_modules() if isinstance(m, nn.LayerNorm)}


def mha_attrs(mha):
    return {"embed_dim": mha.embed_dim, "num_heads": mha.num_heads, "head_dim": mha.head_dim, "kdim": mha.kdim, "vdim": mha.vdim,
            "batch_first": mha.batch_first, "dropout": mha.dropout, "qkv_same_embed_dim": mha._qkv_same_embed_dim,
            "in_proj_bias": mha.in_proj_bias is not None, "out_proj_bias": mha.out_proj.bias is not None,
            "bias_k": mha.bias_k is not None, "add_zero_attn": mha.add_zero_attn}


def conv_attrs(conv):
    return {"kernel_size": list(conv.kernel_size), "padding": list(conv.padding), "stride": list(conv.stride), "bias": conv.bias is not None}


def block_attrs(blk):
    return {"eps": norm_eps(blk), "cross_attn": mha_attrs(blk.cross_attn), "mlp": [type(m).__name__ for m in blk.mlp],
            "cnn": conv_attrs(blk.cnn)}


def transformer_attrs(vt):
    res = {k: getattr(vt, k) for k in ("vol_low_res", "vol_high_res", "out_dim", "embed_dim") if hasattr(vt, k)}
    res.update({"n_groups": list(vt.n_groups), "block_size": list(vt.block_size), "eps": norm_eps(vt),
                "layers": [block_attrs(layer) for layer in vt.layers], "deconv": conv_attrs(vt.deconv)})
    return res


def mod_ln_attrs(m):
    return {"eps": norm_eps(m), "mlp": [type(a).__name__ for a in m.mlp]}


def decoder_attrs(dec):
    """of a Decoder, or of a stand-in that holds only what one of its forwards reads"""
    res = {k: getattr(dec, k) for k in ("K", "sh_dim", "opacity_dim", "scaling_dim", "rotation_dim", "out_dim", "feature_dim")
           if hasattr(dec, k)}
    res["eps"] = norm_eps(dec)
    for k in ("mlp_coarse", "mlp_fine"):
        if hasattr(dec, k):
            res[k] = [type(m).__name__ for m in getattr(dec, k)]
    if hasattr(dec, "mlp_coarse"):
        res["mlp_coarse_distinct"] = len({id(m) for m in dec.mlp_coarse})
    if hasattr(dec, "cross_att"):
        res["cross_att"] = mha_attrs(dec.cross_att)
    return res


ATTRS = {"group_block": block_attrs, "vol_transformer": transformer_attrs, "mod_ln": mod_ln_attrs, "feat_vol": mod_ln_attrs,
         "coarse": decoder_attrs, "fine": decoder_attrs, "point_feats": lambda m: {}}
# what a stand-in must hold of the recorded attributes: the ones its bound forward reads
READ = {"coarse": ("K", "sh_dim", "opacity_dim", "scaling_dim", "rotation_dim", "mlp_coarse"),
        "fine": ("feature_dim", "eps", "mlp_fine", "cross_att")}


# ---- stand-ins ------------------------------------------------------------------------------------------------------------------

def make_mod_ln(inner_dim, mod_dim):
    """a module with the two children ModLN's forward reads, as tests/test_gpu_volcond.py's `network` builds them"""
    from torch import nn

    class Stand(nn.Module):
        pass

    m = Stand()
    m.norm = nn.LayerNorm(inner_dim, eps=1e-6)
    m.mlp = nn.Sequential(nn.SiLU(), nn.Linear(mod_dim, 2 * inner_dim))
    return m


def state_for(rec):
    """the part of the recorded state_dict the stand-in of this item holds: all of it, but for the Decoder, whose two forwards
    have a stand-in each (mlp_coarse.* / everything else)"""
    coarse = {k: v for k, v in rec.state.items() if k.startswith("mlp_coarse.")}
    if rec.item == "coarse":
        return coarse
    if rec.item == "fine":
        return {k: v for k, v in rec.state.items() if k not in coarse}
    return rec.state


def stand_in(rec, dtype=None, device=None):
    """the stand-in of the record's item from the existing builders, the recorded state loaded with strict=True"""
    import torch
    from torch import nn

    import coarsehead_ref as CR
    import deconv3d_ref as DR
    import groupattn_ref as GR
    import viewattn_ref as VR

    c = rec.meta["ctor"]
    if rec.item == "group_block":
        m = GR.make_group_att_block(c["inner_dim"], c["cond_dim"], c["num_heads"])
    elif rec.item == "vol_transformer":
        layers = [GR.make_group_att_block(c["embed_dim"], c["image_feat_dim"], c["num_heads"]) for _ in range(c["num_layers"])]
        m = DR.make_mirror(layers, embed_dim=c["embed_dim"], vol_low_res=c["vol_low_res"], n_groups=tuple(c["n_groups"]),
                           out_dim=c["out_dim"])

        class Mirror(nn.Module):      # a class of its own, so that a forward can be bound on it
            pass

        m.__class__ = Mirror
    elif rec.item in ("mod_ln", "feat_vol"):
        m = make_mod_ln(c["inner_dim"], c["mod_dim"])
    elif rec.item == "coarse":
        m = CR.make_decoder(c["in_dim"], c["K"], c["sh_dim"])
    elif rec.item == "fine":
        m = VR.make_decoder(c["in_dim"], c["sh_dim"])
    elif rec.item == "point_feats":
        m = nn.Module()                                   # get_point_feats reads no module
    else:
        raise KeyError(rec.item)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state_for(rec).items()}, strict=True)
    m = m.to(dtype) if dtype is not None else m
    return m.to(device) if device is not None else m


@contextlib.contextmanager
def float_is_identity_on_float64():
    """the reference's build_feat_vol calls `.float()` on the map it samples; in a float64 run F.grid_sample would refuse the
    float32 map with the float64 grid.  The record was taken with `.float()` the identity on float64 tensors, and so are the
    float64 runs of the yardstick."""
    import torch

    real = torch.Tensor.float

    def keep(self, *a, **k):
        return self if self.dtype == torch.float64 else real(self, *a, **k)

    torch.Tensor.float = keep
    try:
        yield
    finally:
        torch.Tensor.float = real


# ---- running a forward over a record ------------------------------------------------------------------------------------------

def to_torch(a, dtype, device):
    import torch

    t = torch.from_numpy(np.array(a))
    return t.to(device=device, dtype=dtype if t.dtype.is_floating_point else None)


def run(rec, m, forward, dtype, device="cpu", autocast=None, differentiate=None):
    """forward(m, ins, call) -> {output name: tensor} over the record's inputs as `dtype` leaves on `device`, then one backward
    with the recorded upstream gradients (in each output's dtype).  Returns {"out/..", "gin/..", "gparam/.."} -> tensor.
    differentiate: the inputs that get a gradient (default: the recorded ones)."""
    import torch

    m.zero_grad()
    # (group_centers is a float32 buffer of the reference in every mode)
    ins = {k: to_torch(v, torch.float32 if k == "group_centers" and dtype != torch.float64 else dtype, device) for k, v in rec.inputs.items()}
    for k in (rec.gin if differentiate is None else differentiate):
        ins[k].requires_grad_(True)
    ctx = torch.autocast(torch.device(device).type, dtype=autocast) if autocast is not None else contextlib.nullcontext()
    with ctx:
        outs = forward(m, ins, rec.meta["call"])
    loss = None
    for k, o in outs.items():
        if k in rec.ups and o.requires_grad:
            up = to_torch(rec.ups[k], o.dtype, device)
            if up.shape != o.shape:         # (only a mutant that moves a cut gets here: the common corner, zeros elsewhere)
                common = tuple(slice(0, min(a, b)) for a, b in zip(up.shape, o.shape))
                fitted = torch.zeros_like(o)
                fitted[common] = up[common]
                up = fitted
            term = (o * up).sum(dtype=torch.float64 if o.dtype == torch.float64 else torch.float32)
            loss = term if loss is None else loss + term
    if loss is not None:
        loss.backward()
    res = {"out/" + k: o.detach() for k, o in outs.items()}
    res.update({"gin/" + k: ins[k].grad for k in ins if ins[k].requires_grad and ins[k].grad is not None})
    res.update({"gparam/" + k: p.grad for k, p in m.named_parameters() if p.grad is not None})
    return res


# ---- the yardsticks: the forwards the GPU tests use as `torch` ------------------------------------------------------------------

def yard_group_block(m, ins, call):
    import groupattn_ref as GR

    return {"out": GR.torch_forward(m, ins["x"], ins["cond"], call["group_axis"], call["block_size"])}


def yard_vol_transformer(m, ins, call):
    import deconv3d_ref as DR
    import groupattn_ref as GR

    for layer in m.layers:
        type(layer).forward = GR.torch_forward
    conds = []
    out = DR.reference_forward(m, ins["image_feats"], conds=conds)
    res = {"out": out}
    res.update({f"cond_layer{i}": conds[i % len(m.block_size)] for i in range(len(m.layers))})
    return res


def yard_mod_ln(m, ins, call):
    import volcond_torch as T

    return {"out": T.mod_layer_norm(ins["x"], m.mlp(ins["cond"]), m.norm.weight, m.norm.bias, m.norm.eps)}


def feat_vol_self(rec, m, dtype, device):
    """the stand-in for `self` of build_feat_vol: the grid of the project's own restatement, the resolution and the ModLN stand-in"""
    import volcond_cases as VC

    r = rec.meta["attrs"]["feat_vol_reso"]
    assert VC.SCENE == rec.meta["attrs"]["scene_size"]
    return types.SimpleNamespace(volume_grid=to_torch(VC.grid_points(r), dtype, device).view(r, r, r, 3), feat_vol_reso=r, dir_norm=m)


def feat_vol_args(rec, ins, device):
    import torch

    call = rec.meta["call"]
    batch = {k: ins[k] for k in ("tar_w2c", "tar_ixt", "tar_rays_down")}
    Bn, Vn = batch["tar_w2c"].shape[0], call["n_views_sel"]
    src_inps = torch.zeros(1, device=device).expand(Bn * Vn, 3, *call["img_hw"])
    return src_inps, ins["img_feats"], Vn, batch


def yard_feat_vol(rec):
    def forward(m, ins, call):
        import volcond_torch as T
        from generativedensification_amd import volcond as V

        x = ins["img_feats"]
        me = feat_vol_self(rec, m, x.dtype, x.device)
        with float_is_identity_on_float64():
            out = V._torch_feat_vol(me, *feat_vol_args(rec, ins, x.device))
        rays = ins["tar_rays_down"][:, :call["n_views_sel"]]
        return {"out": out, "volume_grid": me.volume_grid, "feats_dir": T.ray_sh(rays)}

    return forward


def yard_coarse(m, ins, call):
    import coarsehead_ref as CR
    from generativedensification_amd import coarsehead as CH

    outs = dict(zip(COARSE_OUTPUTS, CH._torch_forward_coarse(m, ins["feats"], call["opacity_shift"], call["scaling_shift"])))
    outs["centers"] = CR.reference_tail(outs["offset"], outs["opacity"], ins["group_centers"], call["half_cell"], m.K)[0]
    return outs


def yard_fine(m, ins, call):
    import viewattn_ref as VR

    return dict(zip(("features", "sh"), VR.torch_forward_fine(m, ins["volume_feat"], ins["point_feats"])))


def point_feats_args(ins, call):
    """the arguments of pointfeat.point_feats (and of its restatement) from those of Network.get_point_feats"""
    idx, V = call["idx"], call["n_views_sel"]
    return (ins["img_ref"], ins["image"], ins["acc_map"], ins["depth"], ins["points"][ins["mask"]], ins["tar_w2c"][idx, :V],
            ins["tar_ixt"][idx, :V])


def yard_point_feats(m, ins, call):
    """(N, V, 8) is the reference's result behind its caller's einsum('lcb->blc'): permuted back to (V, 8, N)"""
    import pointfeat_ref as PR

    return {"point_feats": PR.point_feats(*point_feats_args(ins, call)).permute(1, 2, 0)}


def yardstick(rec):
    return {"point_feats": yard_point_feats, "group_block": yard_group_block, "vol_transformer": yard_vol_transformer, "mod_ln": yard_mod_ln,
            "feat_vol": yard_feat_vol(rec), "coarse": yard_coarse, "fine": yard_fine}[rec.item]
