"""The recorded runs of what the reference's point decoder chains after its Blocks (tests/golden/pointdec_*.npz, made by
tests/golden/make_pointdec_record.py from the reference's own classes in float64), the stand-ins that take their state_dicts
under strict=True, and the restated forwards of the parts that had none: MaskModule, MaskResModule, SerializationModule with
Point.serialization / Point.sparsify, and the loop of Network.forward over the decoder stages.  Nothing here reads the reference.

The restatements are written over the project's own references: tests/densify_ref.py (selection, gate), scatter_ref.py
(segment softmax), serial_ref.py (codes, orders), upscale_ref.py, finehead_ref.py and block_ref.py.  Every forward takes
`mut`, one deliberate mistake of MUTANTS; tests/test_pointdec_record_cpu.py holds the unmutated ones to the records."""
import glob
import json
import os

import numpy as np

import block_ref as BR
import densify_ref as DR
import finehead_ref as FR
import scatter_ref as SCR
import serial_ref as SER
import upscale_ref as UR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CAP = 256 * 1024
UPSCALE = ("up_ln", "up_ada", "up_res")
MASK = ("mask_topk", "mask_topp")
MASK_RES = ("mask_res_topk", "mask_res_topp")
HEAD = ("head", "head_res")
CHAINS = ("chain_ln", "chain_ada")
NAMES = UPSCALE + MASK + MASK_RES + ("mask_full",) + HEAD + CHAINS
MASK_MUTANTS = ("gate_value_masked", "leaf_ungated", "floor_for_ceil")
CHAIN_MUTANTS = ("grid_size_not_divided", "per_segment_minimum") + FR.ASSEMBLE_MUTANTS
FINALS = ("centers", "shs", "opacity", "scaling", "rotation")


def files(name):
    return [os.path.join(GOLDEN, f"pointdec_{name}.npz")] + sorted(glob.glob(os.path.join(GOLDEN, f"pointdec_{name}_pgrad*.npz")))


def load(name):
    """-> {"meta", "arrays" (name -> array as stored), "state" (name -> float64 tensor)}"""
    import torch

    arrays = {}
    for path in files(name):
        z = np.load(path)
        arrays.update({k: z[k] for k in z.files})
    meta = json.loads(str(arrays.pop("meta")))
    state = {k[len("state/"):]: torch.from_numpy(v.astype(np.float64)) for k, v in arrays.items() if k.startswith("state/")}
    return {"name": name, "meta": meta, "arrays": arrays, "state": state}


def part(rec, prefix):
    return {k[len(prefix):]: v for k, v in rec["arrays"].items() if k.startswith(prefix)}


# ---- points and stand-ins -------------------------------------------------------------------------------------------------

class Point(dict):
    """the attribute-and-key access of the reference's point; a missing attribute reads as an empty Point, as addict's does"""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            if name.startswith("__"):
                raise AttributeError(name) from None
            return type(self)()

    __setattr__ = dict.__setitem__


def tensor(a, dtype=None, device="cpu", grad=False):
    """a stored array on `device`: floats in `dtype` (default float64), the rest as they are"""
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a))
    if t.dtype.is_floating_point:
        t = t.to(dtype or torch.float64)
    return t.to(device).requires_grad_(grad)


def input_point(rec, dtype=None, device="cpu", grad=(), keys=None):
    """the point of a per-module record's inputs; `grad`: the keys that are leaves"""
    vals = {k: tensor(v, dtype, device, k in grad) for k, v in part(rec, "in/").items() if keys is None or k in keys}
    return Point(grid_size=rec["meta"]["grid_size"], **vals)


def make_mask(dim, temperature, non_leaf_ratio, mask_sampling_type):
    """what densify.mask_module_forward / mask_res_module_forward read, under the reference's names"""
    from torch import nn

    class MaskLike(nn.Module):
        def __init__(self):
            super().__init__()
            self.dim, self.temperature, self.non_leaf_ratio, self.mask_sampling_type = dim, temperature, non_leaf_ratio, mask_sampling_type
            if non_leaf_ratio < 1.0:
                self.net = nn.Sequential(nn.Linear(dim, dim), nn.GELU(), nn.Linear(dim, 1))

    return MaskLike()


def make_serialization(stride, order):
    from torch import nn

    class SerializationLike(nn.Module):
        def __init__(self):
            super().__init__()
            self.stride, self.order, self.shuffle_orders, self.enable_residual_attribute = stride, tuple(order), False, False

    return SerializationLike()


def torch_module():
    """GlobalPooling: a module without parameters or attributes"""
    from torch import nn

    return nn.Module()


def _upscale(ctor, norm, global_channels, **kw):
    return UR.make_module(ctor["in_channels"], ctor["out_channels"], ctor["upscale_factor"], ctor["n_frequencies"],
                          global_channels=global_channels, drop_path=ctor["drop_path"], absolute_pe=ctor["enable_absolute_pe"],
                          residual_attribute=ctor["enable_residual_attribute"], is_first=ctor["is_first"], norm=norm, **kw)


def _head(cls, ctor):
    return FR.make_module(cls, ctor["dim"], ctor["sh_degree"], is_first=ctor["is_first"], enable_residual_attribute=ctor["enable_residual_attribute"])


def stand_in(rec, upscale_kw=None, block_kw=None):
    """the existing stand-in of the record's class with the record's state_dict under strict=True, in float64 and eval mode; for
    the chain a list of {name: module} per stage"""
    meta = rec["meta"]
    if meta["item"] == "chain":
        return chain_stand_in(rec, upscale_kw, block_kw)
    if meta["item"] == "upscale":
        m = _upscale(meta["ctor"], meta["norm"], meta["global_channels"], **(upscale_kw or {}))
    elif meta["item"] == "mask":
        m = make_mask(**meta["ctor"])
    else:
        m = _head(meta["class"], meta["ctor"])
    m = m.double()
    m.load_state_dict(rec["state"], strict=True)
    return m.eval()


def chain_stand_in(rec, upscale_kw=None, block_kw=None):
    cfg, stages, kind = rec["meta"]["chain"], [], rec["meta"]["norm"]
    ch = cfg["dec_channels"]
    for s, names in enumerate(rec["meta"]["stage_modules"]):
        cout = ch[s + 1] if s < len(ch) - 1 else ch[s]
        mods = {}
        for name in names:
            if name == "serialization":
                m = make_serialization(cfg["stride"], rec["meta"]["order"])
            elif name == "global":
                m = torch_module()
            elif name == "block0":
                m = BR.make_block(ch[s], cfg["dec_num_head"][s], cfg["patch_size"], norm=kind, global_channels=ch[0], **(block_kw or {}))
            elif name == "up":
                m = UR.make_module(ch[s], cout, cfg["upscale_factor"], cfg["n_frequencies"], global_channels=ch[0], is_first=s == 0, norm=kind,
                                   **(upscale_kw or {}))
            elif name == "mask":
                m = make_mask(cout, cfg["temperature"], cfg["non_leaf_ratio"] if s < len(ch) - 1 else 1.0, "topk")
            else:
                assert name == "head", name
                m = _head("GaussianModule", {"dim": cout, "sh_degree": cfg["sh_degree"], "is_first": s == 0, "enable_residual_attribute": False})
            m = m.double()
            prefix = f"s{s}.{name}."
            m.load_state_dict({k[len(prefix):]: v for k, v in rec["state"].items() if k.startswith(prefix)}, strict=True)
            mods[name] = m.eval()
        stages.append(mods)
    used = sum(len(m.state_dict()) for mods in stages for m in mods.values())
    assert used == len(rec["state"]), (used, len(rec["state"]))
    return stages


# ---- MaskModule and MaskResModule restated --------------------------------------------------------------------------------

def _functions():
    import torch

    class Gate(torch.autograd.Function):
        """densify_ref.ste_gate with densify_ref.ste_gate_grad behind it"""

        @staticmethod
        def forward(ctx, feat, prob, mask):
            ctx.save_for_backward(feat, prob)
            return torch.from_numpy(DR.ste_gate(feat.detach().numpy(), prob.detach().numpy(), None if mask is None else mask.numpy()))

        @staticmethod
        def backward(ctx, grad_out):
            feat, prob = ctx.saved_tensors
            dfeat, dprob = DR.ste_gate_grad(feat.detach().numpy(), prob.detach().numpy(), grad_out.numpy())
            return torch.from_numpy(dfeat), torch.from_numpy(dprob).reshape(prob.shape), None

    class SegmentSoftmax(torch.autograd.Function):
        """scatter_ref.softmax_ptr with scatter_ref.softmax_grad behind it"""

        @staticmethod
        def forward(ctx, src, ptr):
            y, ctx.index = SCR.softmax_ptr(src.detach().numpy(), ptr.numpy())
            ctx.segments = len(ptr) - 1
            y = torch.from_numpy(y)
            ctx.save_for_backward(y)
            return y

        @staticmethod
        def backward(ctx, grad_out):
            y, = ctx.saved_tensors
            return torch.from_numpy(SCR.softmax_grad(y.numpy(), grad_out.numpy(), ctx.index, ctx.segments)), None

    return Gate, SegmentSoftmax


def select(prob, ratio, sampling, offset, mut=None):
    """(mask, new_offset) as tensors, by densify_ref (the counts in float32, which at these sizes is every dtype's count)"""
    import torch

    x, off = prob.detach().numpy().reshape(-1), offset.numpy()
    if sampling == "topk" and mut == "floor_for_ceil":
        mask, counts = np.zeros(x.size, dtype=bool), []
        for a, e in DR.segments(off, x.size):
            k = int(np.floor(np.float32(ratio) * np.float32(e - a)))
            mask[a + DR.ranking(x[a:e])[:k]] = True
            counts.append(k)
        new = np.cumsum(np.asarray(counts, dtype=np.int64))
    else:
        mask, new = (DR.top_k if sampling == "topk" else DR.top_p)(x, ratio, off, "f32")
    return torch.from_numpy(mask), torch.from_numpy(new)


def restated_mask_forward(self, point, mut=None):
    """MaskModule.forward: sigmoid scores, the selection, the straight-through gate on EVERY row with the value `feat`, the
    selected rows and the leaf rows as two points -> (point, non_leaf or None at ratio 1.0)"""
    import torch

    assert mut in (None,) + MASK_MUTANTS
    P = type(point)
    if self.non_leaf_ratio >= 1.0:
        return P(coord=point.coord, feat=point.feat, global_feat=point.global_feat, offset=point.offset, grid_size=point.grid_size,
                 leaf_point=P(coord=point.coord, feat=point.feat, offset=point.offset, grid_size=point.grid_size)), None
    Gate, _ = _functions()
    feat = point.feat
    prob = torch.sigmoid(self.net(feat))
    non_leaf, non_leaf_offset = select(prob, self.non_leaf_ratio, self.mask_sampling_type, point.offset, mut)
    gated = Gate.apply(feat, prob, non_leaf if mut == "gate_value_masked" else None)
    leaf_feat = feat[~non_leaf] if mut == "leaf_ungated" else gated[~non_leaf]
    out = P(coord=point.coord[non_leaf], feat=gated[non_leaf], global_feat=point.global_feat, offset=non_leaf_offset, grid_size=point.grid_size,
            leaf_point=P(coord=point.coord[~non_leaf], feat=leaf_feat, offset=point.offset - non_leaf_offset, grid_size=point.grid_size))
    return out, non_leaf


def restated_mask_res_forward(self, point):
    """MaskResModule.forward: segment-softmax scores at the temperature, the selection, the gate with the value feat * non_leaf,
    six keys on the same point"""
    import torch
    import torch.nn.functional as F

    Gate, SegmentSoftmax = _functions()
    feat = point.feat
    raw_prob = self.net(feat)
    prob = SegmentSoftmax.apply(raw_prob / self.temperature, F.pad(point.offset, (1, 0)))
    non_leaf, non_leaf_offset = select(prob, self.non_leaf_ratio, self.mask_sampling_type, point.offset)
    point.feat = Gate.apply(feat, prob, non_leaf)
    point.update({"raw_prob": raw_prob, "prob": prob, "non_leaf": non_leaf, "non_leaf_offset": non_leaf_offset, "leaf": ~non_leaf,
                  "leaf_offset": point.offset - non_leaf_offset})
    return point


# ---- GlobalPooling restated ------------------------------------------------------------------------------------------------

def segment_mean(src, indptr, reduce="mean"):
    """scatter_ref.segment_csr with scatter_ref.segment_csr_grad behind it (CPU, float64)"""
    import torch

    class SegmentCsr(torch.autograd.Function):
        @staticmethod
        def forward(ctx, src):
            ctx.shape = tuple(src.shape)
            return torch.from_numpy(SCR.segment_csr(src.detach().numpy(), indptr.numpy(), reduce)[0])

        @staticmethod
        def backward(ctx, grad_out):
            return torch.from_numpy(SCR.segment_csr_grad(ctx.shape, indptr.numpy(), reduce, grad_out.numpy()))

    return SegmentCsr.apply(src)


def global_pooling_forward(self, point, segment_csr):
    """GlobalPooling.forward: global_feat is the mean of feat over each segment; `segment_csr(src, indptr, reduce=)` is
    torch_scatter's (the drop-in on the GPU, scatter_ref's on the CPU)"""
    import torch.nn.functional as F

    point.update({"global_feat": segment_csr(point.feat, F.pad(point.offset, (1, 0), "constant", 0), reduce="mean")})
    return point


# ---- SerializationModule restated -----------------------------------------------------------------------------------------

def offset2batch(offset):
    import torch

    return torch.searchsorted(offset, torch.arange(int(offset[-1]), device=offset.device), right=True)


def numpy_serialize(point, order, mut=None):
    """Point.serialization over serial_ref.serialize (CPU): the cells are trunc((coord - the minimum over the WHOLE batch) / grid_size)"""
    import torch

    coord, batch = point.coord.detach().numpy(), point.batch.numpy()
    low = coord.min(0)
    if mut == "per_segment_minimum":
        low = np.stack([coord[batch == b].min(0) for b in range(int(batch.max()) + 1)])[batch]
    grid = np.trunc((coord - low) / point.grid_size).astype(np.int32)
    depth = int(grid.max()).bit_length()
    code, order_, inverse = SER.serialize(grid, batch, depth, list(order))
    point["grid_coord"] = torch.from_numpy(grid)
    point["serialized_depth"] = depth
    point["serialized_code"], point["serialized_order"], point["serialized_inverse"] = (torch.from_numpy(a) for a in (code, order_, inverse))


def sparsify(point, pad=96):
    """Point.sparsify, over this project's SparseConvTensor"""
    import torch

    from generativedensification_amd.sparse_conv import SparseConvTensor

    sparse_shape = torch.add(torch.max(point.grid_coord, dim=0).values, pad).tolist()
    indices = torch.cat([point.batch.unsqueeze(-1).int(), point.grid_coord.int()], dim=1).contiguous()
    point["sparse_shape"] = sparse_shape
    point["sparse_conv_feat"] = SparseConvTensor(point.feat, indices, sparse_shape, int(point.batch[-1]) + 1)


def serialized(point, order, serialize=numpy_serialize, mut=None):
    point["batch"] = offset2batch(point.offset)
    serialize(point, order, mut) if serialize is numpy_serialize else serialize(point, order=order, shuffle_orders=False)
    sparsify(point)
    return point


def serialization_module_forward(self, point, serialize=numpy_serialize, mut=None):
    """SerializationModule.forward: a fresh point of five keys whose grid_size is the old one DIVIDED by the stride"""
    grid_size = point.grid_size if mut == "grid_size_not_divided" else point.grid_size / self.stride
    fresh = type(point)(coord=point.coord, feat=point.feat, global_feat=point.global_feat, offset=point.offset, grid_size=grid_size)
    return serialized(fresh, self.order, serialize, mut)


# ---- the loop of Network.forward over the stages --------------------------------------------------------------------------

def snapshot(point, prefix, into):
    import torch

    for k, v in point.items():
        if k == "leaf_point":
            snapshot(v, prefix + "leaf/", into)
        elif isinstance(v, torch.Tensor):
            into[prefix + k] = v
        elif k == "sparse_shape":
            into[prefix + k] = torch.tensor(v)


def assert_keys(rec, where, point):
    """the key set of a point of the chain (and of its leaf_point) is the recorded one; `batch`, which the reference's Point adds
    to itself wherever there is an offset, apart"""
    want = rec["meta"]["points"][where]
    assert sorted(k for k in point if k != "batch") == sorted(k for k in want["keys"] if k != "batch"), (where, list(point), want["keys"])
    if "leaf" in want:
        assert_keys({"meta": {"points": {where: want["leaf"]}}}, where, point.leaf_point)
    else:
        assert "leaf_point" not in point, where


def chain_input(rec, dtype=None, device="cpu", grad=False, serialize=numpy_serialize):
    a = rec["arrays"]
    point = Point(coord=tensor(a["in/coord"], dtype, device, grad), feat=tensor(a["in/feat"], dtype, device, grad),
                  offset=tensor(a["in/offset"], device=device), grid_size=rec["meta"]["grid_size"])
    return serialized(point, rec["meta"]["order"], serialize)


def stage_input(rec, s, dtype=None, device="cpu", serialize=numpy_serialize):
    """the recorded input point of stage s (what the stage before it returned), leaf_point and all"""
    if s == 0:
        return chain_input(rec, dtype, device, serialize=serialize)
    vals = part(rec, f"s{s}/in/")
    point = Point({k: tensor(v, dtype, device) for k, v in vals.items() if "/" not in k})
    point["grid_size"] = rec["meta"]["points"][f"s{s}/in"]["scalars"]["grid_size"]
    point["leaf_point"] = Point({k[len("leaf/"):]: tensor(v, dtype, device) for k, v in vals.items() if k.startswith("leaf/")})
    return point


def run_stage(rec, mods, point, forwards, arrays, s):
    """one `point = dec(point)`; forwards: name -> callable(module, point) (the restatements on the CPU, the bound forwards on
    the GPU)"""
    for name, m in mods.items():
        if name == "mask" and s == 0:
            arrays.update({f"s{s}/mask_in/{k}": point[k] for k in ("coord", "feat", "offset")})
        out = forwards[name](m, point)
        if name == "mask":
            if isinstance(out, tuple):          # (the restatement also hands the mask out; the bound forward cannot)
                out, non_leaf = out
                if non_leaf is not None:
                    arrays[f"s{s}/non_leaf"] = non_leaf
        if name == "serialization":
            snapshot(out, f"s{s}/serial/", arrays)
            assert_keys(rec, f"s{s}/serial", out)
        point = out
    return point


def cpu_forwards(mut=None):
    return {"serialization": lambda m, p: serialization_module_forward(m, p, mut=mut),
            "global": lambda m, p: global_pooling_forward(m, p, segment_mean),
            "block0": BR.restated_forward,
            "up": UR.reference_forward,
            "mask": lambda m, p: restated_mask_forward(m, p),
            "head": FR.reference_module_forward}


def run_chain(rec, stages, point, forwards):
    """-> (arrays under the record's names, the leaf points).  The key sets of every stage's input, output and serialized point
    are held to the recorded ones here."""
    arrays, leaf_points = {}, []
    for s, mods in enumerate(stages):
        snapshot(point, f"s{s}/in/", arrays)
        assert_keys(rec, f"s{s}/in", point)
        point = run_stage(rec, mods, point, forwards, arrays, s)
        snapshot(point, f"s{s}/out/", arrays)
        assert_keys(rec, f"s{s}/out", point)
        leaf_points.append(point.leaf_point)
    return arrays, leaf_points


def assemble(rec, leaf_points, dtype=None, device="cpu", mut=None):
    """`_union_gaussians` and the five concatenations over finehead_ref.reference_assemble -> name -> tensor, and the leaves"""
    a = rec["arrays"]
    coarse = {k: tensor(a["in/" + k], dtype, device) for k in ("centers_coarse", "opacity_coarse", "scaling_coarse", "rotation_coarse", "shs_fine")}
    out = FR.reference_assemble([(p.coord, p.attribute) for p in leaf_points],
                                [coarse[k] for k in ("centers_coarse", "opacity_coarse", "scaling_coarse", "rotation_coarse")], coarse["shs_fine"],
                                tensor(a["in/mask"], device=device), tensor(a["in/selected_pts_mask"], device=device), rec["meta"]["sh_dim"],
                                rec["meta"]["opacity_shift"], rec["meta"]["fine_scaling_shift"], offsets=[p.offset for p in leaf_points], mut=mut)
    return dict(zip(FINALS, out))
