#!/usr/bin/env python
"""tests/golden/make_block_record.py — generates tests/golden/block_ln.npz and block_ada.npz: a forward and a backward of the
reference's own point-decoder Block (lightning/point_decoder/autoencoder.py), run in float64 on the CPU.  Authoring only: it needs
a checkout of the reference next to this repository (or at $GD_REFERENCE_ROOT).  The tests read the files and never the reference
(tests/block_ref.py: load_record).

autoencoder.py, utils/structure.py, utils/modules.py, utils/misc.py and layers/normalization.py are loaded by path, for real:
Block, SerializedAttention, MLP, Point, PointSequential and AdaLayerNorm are the reference's classes and Block.forward its lines.
The packages they import are stood in for as make_network_record.py does:
    spconv.pytorch     SubMConv3d is the table model of tests/subm_ref.py (table_all, output and gradients, in float64) behind a
                       torch.autograd.Function; SparseConvTensor holds features, indices, spatial_shape, batch_size
    torch_scatter      gather_csr is tests/scatter_ref.py's, with its closed-form gradient
    addict.Dict        a dict with attribute access
    pytorch_lightning  LightningModule = torch.nn.Module
    timm, torch_geometric, point_prompt_training, utils.serialization   names only: nothing a Block runs reaches them (drop_path
                       is 0.0, so the Block holds an nn.Identity and no DropPath is built)
`load_reference(stand_ins)` serves make_pointdec_record.py, which needs more of autoencoder.py; without the argument it is as above.
flash_attn is absent, and the Block is built with enable_flash=False, upcast_attention=False, upcast_softmax=False: the
reference's own torch attention over the same padded patches, which is the flash kernel's result in exact arithmetic (with the
upcasts on, `.float()` would take float64 down to float32).  Nothing of the reference is copied: a file holds arrays, names,
shapes and scalar settings.

Each record: C = 16, 2 heads of 8, patch 8, 48 points in two segments of 28 and 20 (neither a multiple of the patch, so both
are padded by the reference's get_padding_and_inverse), global_feat 24 wide, eval mode.
    block_ln    norm_layer = partial(nn.LayerNorm, elementwise_affine=False), what Network builds
    block_ada   norm_layer = partial(AdaLayerNorm, w_shape=24), what AutoEncoder builds

Every recorded input, upstream gradient and parameter is a bfloat16-representable value inside float16's normal range, so one
record is the float64 truth "on the inputs as rounded to their dtypes" for float32 and 16-bit runs alike.

Usage: python tests/golden/make_block_record.py        (prints every file's size; running it twice gives the same arrays)
"""
import importlib.util
import json
import os
import sys
import types
from functools import partial

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import block_cases as BC  # noqa: E402
import scatter_ref as SCR  # noqa: E402
import subm_ref as SM  # noqa: E402
from make_network_record import CAP, REF, np64, q, randn, set_parameters  # noqa: E402

COUNTS, CHANNELS, HEADS, PATCH, GLOBAL = (28, 20), 16, 2, 8, 24


# ---- the stand-ins for the packages -------------------------------------------------------------------------------------------

class Dict(dict):
    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None

    __setattr__ = dict.__setitem__


class SparseConvTensor:
    def __init__(self, features, indices, spatial_shape, batch_size):
        self.features, self.indices, self.spatial_shape, self.batch_size = features, indices, spatial_shape, batch_size

    def replace_feature(self, feature):
        return SparseConvTensor(feature, self.indices, self.spatial_shape, self.batch_size)


class _TableConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, weight, bias, nbr):
        ctx.save_for_backward(feat, weight, bias)
        ctx.nbr = nbr
        return SM.table_all(nbr, feat.detach(), weight.detach(), bias.detach())["out"]

    @staticmethod
    def backward(ctx, grad_out):
        feat, weight, bias = ctx.saved_tensors
        with torch.enable_grad():
            res = SM.table_all(ctx.nbr, feat.detach(), weight.detach(), bias.detach(), grad_out=grad_out)
        return res["grad_feat"], res["grad_weight"], res["grad_bias"], None


class SubMConv3d(torch.nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, bias=True, indice_key=None):
        super().__init__()
        assert bias
        self.kernel_size, self.indice_key = (kernel_size,) * 3, indice_key
        self.weight = torch.nn.Parameter(torch.empty(out_channels, *self.kernel_size, in_channels))
        self.bias = torch.nn.Parameter(torch.empty(out_channels))

    def forward(self, sp):
        assert sp.features.dtype == torch.float64
        nbr, _ = SM.table_model(sp.indices.numpy(), sp.spatial_shape, sp.batch_size, self.kernel_size)
        return sp.replace_feature(_TableConv.apply(sp.features, self.weight, self.bias, nbr))


class _GatherCsr(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, indptr):
        ctx.indptr = indptr.numpy()
        return torch.from_numpy(SCR.gather_csr(src.detach().numpy(), ctx.indptr))

    @staticmethod
    def backward(ctx, grad_out):
        return torch.from_numpy(SCR.gather_csr_grad(grad_out.numpy(), ctx.indptr)), None


def load_reference(stand_ins=None):
    """stand_ins: None for what a Block needs (above); make_pointdec_record.py passes {"Dict", "gather_csr", "segment_csr",
    "cumsum", "scatter", "softmax"} for the rest of autoencoder.py, and utils/serialization is then the reference's own package"""
    full = stand_ins is not None
    stand_ins = stand_ins or {}

    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        m.__path__ = []
        sys.modules[name] = m
        return m

    class _Any:
        def __init__(self, *a, **k):
            raise AssertionError("a stand-in for a class no Block uses was built")

    def by_path(name, *parts, package=False):
        path = os.path.join(REF, "lightning", "point_decoder", *parts)
        spec = importlib.util.spec_from_file_location(name, path, submodule_search_locations=[os.path.dirname(path)] if package else None)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod

    assert "flash_attn" not in sys.modules and importlib.util.find_spec("flash_attn") is None
    stub("addict", Dict=stand_ins.get("Dict", Dict))
    stub("pytorch_lightning", LightningModule=torch.nn.Module)
    sp = stub("spconv.pytorch", SubMConv3d=SubMConv3d, SparseConvTensor=SparseConvTensor,
              modules=types.SimpleNamespace(is_spconv_module=lambda m: isinstance(m, SubMConv3d)))
    stub("spconv", pytorch=sp)
    stub("torch_scatter", gather_csr=stand_ins.get("gather_csr", lambda src, indptr: _GatherCsr.apply(src, indptr)),
         segment_csr=stand_ins.get("segment_csr"))
    stub("timm")
    stub("timm.models")
    stub("timm.models.layers", DropPath=_Any)
    stub("torch_geometric")
    stub("torch_geometric.utils", cumsum=stand_ins.get("cumsum"), scatter=stand_ins.get("scatter"), softmax=stand_ins.get("softmax"))
    pd = "lightning.point_decoder"
    for pkg in ("lightning", pd, pd + ".utils", pd + ".layers"):
        stub(pkg)
    stub(pd + ".point_prompt_training", PDNorm=_Any)
    if full:
        by_path(pd + ".utils.serialization", "utils", "serialization", "__init__.py", package=True)
    else:
        stub(pd + ".utils.serialization", encode=None, decode=None)
    by_path(pd + ".utils.misc", "utils", "misc.py")
    by_path(pd + ".utils.structure", "utils", "structure.py")
    by_path(pd + ".layers.normalization", "layers", "normalization.py")
    by_path(pd + ".utils.modules", "utils", "modules.py")
    return by_path(pd + ".autoencoder", "autoencoder.py")


# ---- one record ---------------------------------------------------------------------------------------------------------------

def block_record(ae, kind, seed):
    gen = torch.Generator().manual_seed(seed)
    norm_layer = {"ln": partial(torch.nn.LayerNorm, elementwise_affine=False), "ada": partial(ae.AdaLayerNorm, w_shape=GLOBAL)}[kind]
    ctor = {"channels": CHANNELS, "num_heads": HEADS, "patch_size": PATCH, "cpe_indice_key": "stem", "enable_flash": False,
            "upcast_attention": False, "upcast_softmax": False}
    blk = ae.Block(norm_layer=norm_layer, **ctor).double()
    assert isinstance(blk.cpe, ae.PointSequential) and isinstance(blk.drop_path[0], torch.nn.Identity)
    set_parameters(blk, gen)
    blk.eval()
    data = BC.block_point(COUNTS, CHANNELS, GLOBAL, seed=seed)
    feat = q(randn(gen, sum(COUNTS), CHANNELS) * 1.2 + 0.2).requires_grad_(True)
    global_feat = q(randn(gen, len(COUNTS), GLOBAL)).requires_grad_(True)
    ints = {k: torch.from_numpy(data[k]) for k in ("offset", "indices", "serialized_order", "serialized_inverse")}
    point = ae.Point(feat=feat, global_feat=global_feat, offset=ints["offset"], serialized_order=ints["serialized_order"],
                     serialized_inverse=ints["serialized_inverse"],
                     sparse_conv_feat=SparseConvTensor(feat, ints["indices"], list(data["spatial_shape"]), data["batch_size"]))
    out = blk(point)
    assert blk.cpe[0].training and not blk.attn.training           # the reference's quirk
    assert out.feat is out.sparse_conv_feat.features and out.feat.dtype == torch.float64 and blk.attn.patch_size == PATCH
    up = q(randn(gen, *out.feat.shape))
    (out.feat * up).sum().backward()
    meta = {"item": "block", "kind": kind, "ctor": ctor, "global_channels": GLOBAL, "counts": list(COUNTS),
            "spatial_shape": list(data["spatial_shape"]), "batch_size": data["batch_size"], "training": False,
            "attn_patch_size": blk.attn.patch_size, "norm_eps": blk.norm1[0].eps}
    arrays = {"meta": np.array(json.dumps(meta, sort_keys=True))}
    for k, v in blk.state_dict().items():
        assert torch.equal(v, q(v)), k
        arrays["state/" + k] = v.to(torch.float32).numpy()
    arrays["in/feat"], arrays["in/global_feat"] = feat.detach().float().numpy(), global_feat.detach().float().numpy()
    arrays.update({"in/" + k: v.numpy() for k, v in ints.items()})
    arrays["up/feat"] = up.float().numpy()
    arrays["out/feat"] = np64(out.feat)
    arrays["gin/feat"] = np64(feat.grad)
    if kind == "ada":
        arrays["gin/global_feat"] = np64(global_feat.grad)
    else:
        assert global_feat.grad is None
    for k, p in blk.named_parameters():
        arrays["gparam/" + k] = np64(p.grad)
    assert all(a.dtype.kind in "USi" or np.isfinite(a).all() for a in arrays.values())
    path = os.path.join(HERE, f"block_{kind}.npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print(f"{os.path.relpath(path, os.path.dirname(os.path.dirname(HERE)))}: {size} bytes")
    assert size <= CAP, (path, size)


def main():
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    ae = load_reference()
    block_record(ae, "ln", seed=81)
    block_record(ae, "ada", seed=82)


if __name__ == "__main__":
    main()
