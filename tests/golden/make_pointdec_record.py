#!/usr/bin/env python
"""tests/golden/make_pointdec_record.py — generates tests/golden/pointdec_*.npz: forwards and backwards of what the reference's
point decoder (lightning/point_decoder/autoencoder.py) chains after its Blocks in every decoder stage, run in float64 on the
CPU, in eval mode.  Authoring only: it needs a checkout of the reference next to this repository (or at $GD_REFERENCE_ROOT).
The tests read the files and never the reference (tests/pointdec_record.py).

autoencoder.py, utils/structure.py, utils/misc.py, utils/modules.py, layers/normalization.py and the utils/serialization
package are loaded by path, for real (make_block_record.load_reference with the stand-ins below); network.py is loaded as
make_network_record.py loads it, for `_union_gaussians`, `group_cat` and the five concatenations of the fine set, which are
read from its text at run time and executed as they stand.  The packages are stood in for as in make_block_record.py, and
    addict.Dict                     a dict with attribute access in which a missing attribute reads as an empty Dict
                                    (`point.global_feat` of a point without one, as addict gives it)
    torch_scatter.segment_csr       tests/scatter_ref.py's segment_csr / segment_csr_grad behind an autograd Function
    torch_geometric.utils           scatter, cumsum, softmax: scatter_ref.scatter, cumsum, softmax_ptr / softmax_grad
`top_p`'s sparse torch.mm and its autocast(enabled=False) run as they are.  Nothing of the reference is copied: a file holds
arrays, names, shapes and scalar settings.

The two liberties: while a MaskResModule record is taken, `Tensor.to(torch.float32)` is the identity on float64 tensors outside
no_grad (the reference casts the scores to float32 in front of the softmax; kept, the float64 truth would carry a float32
rounding of its own; inside top_k / top_p, which run under no_grad, the cast stays), and `.float()` is the identity on float64
tensors inside the five concatenations, as in make_network_record.py.

Per-module records: 48 points in two segments of 28 and 20, 16 channels, global_feat 24 wide, grid_size 0.25.
    up_ln        UpscaleModule 16 -> 16, S = 2, F = 10, LayerNorm without affine (what Network builds)
    up_ada       UpscaleModule 24 -> 16, S = 2, F = 10, AdaLayerNorm(w_shape=24), enable_absolute_pe
    up_res       UpscaleResModule 16 -> 16, S = 3, F = 10, AdaLayerNorm(w_shape=24), enable_residual_attribute, not first, an
                 attribute of 20 columns
    mask_topk, mask_topp            MaskModule(16, temperature 1.0, non_leaf_ratio 0.6)
    mask_res_topk, mask_res_topp    MaskResModule, the same, temperature 0.5
    mask_full    MaskModule(non_leaf_ratio 1.0): keys and identities
    head, head_res                  GaussianModule(16, sh_degree 1) on a leaf_point; GaussianResModule, residual, not first
chain_ln: 34 points in two segments of 20 and 14; the loop of Network.forward over two stages built as Network.__init__ builds them without residual attributes,
[Block, UpscaleModule, MaskModule(0.6, topk), GaussianModule] and [SerializationModule(2, four orders), Block, UpscaleModule,
MaskModule(1.0), GaussianModule], 16 and 8 wide, from a point serialized and sparsified as Network.forward does; then
`_union_gaussians` over the two leaf points and the five concatenations against a coarse set of 30 rows.  Stage 1 has ONE head
of 8, not two of 4: the HIP attention serves head dimensions 8, 16, 32 and 64, and the width that keeps 16 -> 8 was chosen here
instead of relaxing that envelope.
chain_ada: the same chain with a leading GlobalPooling and AdaLayerNorm(w_shape=16) norms, what AutoEncoder builds.

Every recorded float input, parameter and upstream gradient is a bfloat16-representable value inside float16's normal range.
Seeds are searched until the conditions of `mask_record` and `chain_record` hold: every selection's cut lies 8 times further
from its neighbours than the float32 and the bf16-autocast torch runs of the same reference module differ from the float64
run, no selection is empty or full, every coordinate that feeds a trunc lies 8 float32 errors from a cell border, no two points
of a segment share a cell, tanh stays out of saturation.  The seed and the margins are printed and kept in `meta`.

Usage: python tests/golden/make_pointdec_record.py        (prints every file's size; running it twice gives the same arrays)
"""
import contextlib
import copy
import glob
import json
import os
import sys
import textwrap
import types
from functools import partial

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import scatter_ref as SCR  # noqa: E402
import subm_ref as SM  # noqa: E402
import make_block_record as MB  # noqa: E402
from make_block_record import Dict, SubMConv3d, _GatherCsr, load_reference  # noqa: E402
from make_network_record import CAP, REF, load_network, np64, q, randn, set_parameters  # noqa: E402
from network_record import float_is_identity_on_float64  # noqa: E402

COUNTS, CHANNELS, GLOBAL, GRID, ATTR = (28, 20), 16, 24, 0.25, 20
ORDER = ("z", "z-trans", "hilbert", "hilbert-trans")
SAFETY = 8.0            # a cut or a cell border lies this many errors of the lower-precision torch runs away
F64 = torch.float64


# ---- the stand-ins for the packages -------------------------------------------------------------------------------------------

class PointDict(Dict):
    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            if name.startswith("__"):
                raise AttributeError(name) from None
            return type(self)()


def _in_float64(fn, src, *rest):
    """fn on float64; any other floating dtype goes through float64 and back (the float32 and autocast runs of the margins)"""
    if src.dtype.is_floating_point and src.dtype != F64:
        return fn(src.double(), *rest).to(src.dtype)
    return fn(src, *rest)


class _SegmentCsr(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, indptr, reduce):
        ctx.indptr, ctx.reduce, ctx.shape = indptr.numpy(), reduce, tuple(src.shape)
        return torch.from_numpy(SCR.segment_csr(src.detach().numpy(), ctx.indptr, reduce)[0])

    @staticmethod
    def backward(ctx, grad_out):
        return torch.from_numpy(SCR.segment_csr_grad(ctx.shape, ctx.indptr, ctx.reduce, grad_out.numpy())), None, None


class _Softmax(torch.autograd.Function):
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


def gather_csr(src, indptr):
    return _in_float64(_GatherCsr.apply, src, indptr)


def segment_csr(src, indptr, out=None, reduce="sum"):
    assert out is None
    return _in_float64(_SegmentCsr.apply, src, indptr, reduce)


def pyg_scatter(src, index, dim=0, dim_size=None, reduce="sum"):
    assert dim == 0
    size = int(index.max()) + 1 if dim_size is None else dim_size
    return torch.from_numpy(SCR.scatter(src.numpy(), index.numpy(), size, reduce)[0])


def pyg_cumsum(x, dim=0):
    assert dim == 0
    return torch.from_numpy(SCR.cumsum(x.numpy()))


def pyg_softmax(src, index=None, ptr=None, num_nodes=None, dim=0):
    assert index is None and ptr is not None and dim == 0
    return _in_float64(_Softmax.apply, src, ptr)


class AnyConv(SubMConv3d):
    """the table model, in float64 whatever dtype the features have"""

    def forward(self, sp):
        if sp.features.dtype == F64:
            return super().forward(sp)
        nbr, _ = SM.table_model(sp.indices.numpy(), sp.spatial_shape, sp.batch_size, self.kernel_size)
        out = MB._TableConv.apply(sp.features.double(), self.weight.double(), self.bias.double(), nbr)
        return sp.replace_feature(out.to(sp.features.dtype))


@contextlib.contextmanager
def to_float32_keeps_float64():
    real = torch.Tensor.to

    def keep(self, *a, **k):
        if self.dtype == F64 and a == (torch.float32,) and not k and torch.is_grad_enabled():
            return self
        return real(self, *a, **k)

    torch.Tensor.to = keep
    try:
        yield
    finally:
        torch.Tensor.to = real


@contextlib.contextmanager
def tapped(ae):
    """the calls of the reference's top_k / top_p: [{"x", "mask", "offset"}]"""
    calls, real = [], (ae.top_k, ae.top_p)

    def tap(fn):
        def run(**kw):
            mask, new_offset = fn(**kw)
            calls.append({"x": kw["x"].detach().reshape(-1).clone(), "mask": mask, "offset": new_offset})
            return mask, new_offset
        return run

    ae.top_k, ae.top_p = tap(real[0]), tap(real[1])
    try:
        yield calls
    finally:
        ae.top_k, ae.top_p = real


def load():
    net = load_network()
    ae = load_reference({"Dict": PointDict, "gather_csr": gather_csr, "segment_csr": segment_csr, "cumsum": pyg_cumsum,
                         "scatter": pyg_scatter, "softmax": pyg_softmax})
    ae.spconv.SubMConv3d = AnyConv
    net.offset2batch = sys.modules["lightning.point_decoder.utils.misc"].offset2batch
    return ae, net


# ---- writing ------------------------------------------------------------------------------------------------------------------

def write(name, meta, main, pgrad):
    """main, pgrad: name -> array.  The parameter gradients move into _pgrad files where the file would exceed the cap."""
    main = dict(main, meta=np.array(json.dumps(meta, sort_keys=True)))
    for a in list(main.values()) + list(pgrad.values()):
        assert a.dtype.kind in "USiub" or np.isfinite(a).all()
    path = os.path.join(HERE, f"pointdec_{name}.npz")
    for old in glob.glob(os.path.join(HERE, f"pointdec_{name}_pgrad*.npz")):
        os.remove(old)
    np.savez_compressed(path, **main, **pgrad)
    written = [path]
    if os.path.getsize(path) > CAP:
        np.savez_compressed(path, **main)
        parts = []
        for k in sorted(pgrad, key=lambda k: -pgrad[k].nbytes):
            part = next((p for p in parts if sum(pgrad[j].nbytes for j in p) + pgrad[k].nbytes <= CAP - 8192), None)
            if part is None:
                parts.append([k])
            else:
                part.append(k)
        for i, part in enumerate(parts):
            side = os.path.join(HERE, f"pointdec_{name}_pgrad{i if i else ''}.npz")
            np.savez_compressed(side, **{k: pgrad[k] for k in part})
            written.append(side)
    for p in written:
        size = os.path.getsize(p)
        print(f"{os.path.relpath(p, os.path.dirname(os.path.dirname(HERE)))}: {size} bytes")
        assert size <= CAP, (p, size)


def stored_in(t):
    """an input as it is stored: float32 of a rounded value, integers as they are"""
    if t.dtype.is_floating_point:
        assert torch.equal(t.detach().double(), q(t))
        return t.detach().to(torch.float32).numpy()
    return t.numpy()


def state_arrays(module, prefix="state/"):
    out = {}
    for k, v in module.state_dict().items():
        assert torch.equal(v.double(), q(v)) or k.endswith("frequencies"), k
        out[prefix + k] = v.detach().to(torch.float32).numpy()
    return out


def param_grads(module, prefix="gparam/"):
    return {prefix + k: np64(p.grad) for k, p in module.named_parameters() if p.grad is not None}


def common(gen, channels=CHANNELS):
    n = sum(COUNTS)
    coord = q(torch.rand(n, 3, generator=gen, dtype=F64) * 4.0 + torch.tensor([1.3, -2.1, 0.6], dtype=F64))
    feat = q(randn(gen, n, channels) * 1.2 + 0.2)
    return {"coord": coord, "feat": feat, "global_feat": q(randn(gen, len(COUNTS), GLOBAL)),
            "offset": torch.tensor(COUNTS).cumsum(0)}


def point_of(ae, inp, dtype=F64, grad=()):
    vals = {k: (v.to(dtype) if v.dtype.is_floating_point else v) for k, v in inp.items()}
    for k in grad:
        vals[k] = vals[k].clone().requires_grad_(True)
    return ae.Point(grid_size=GRID, **vals)


def lowered(module, run):
    """run(module', dtype) on a float32 copy of the module: once plainly, once under bfloat16 autocast"""
    m32 = copy.deepcopy(module).float()
    with torch.no_grad():
        a = run(m32, torch.float32)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            b = run(m32, torch.float32)
    return a, b


# ---- upscale ------------------------------------------------------------------------------------------------------------------

def upscale_record(ae, name, res, cin, cout, S, ada, absolute_pe, seed):
    for seed in range(seed, seed + 200):
        gen = torch.Generator().manual_seed(seed)
        norm_layer = partial(ae.AdaLayerNorm, w_shape=GLOBAL) if ada else partial(torch.nn.LayerNorm, elementwise_affine=False)
        ctor = {"is_first": not res, "in_channels": cin, "out_channels": cout, "upscale_factor": S, "n_frequencies": 10,
                "drop_path": 0.0, "enable_absolute_pe": absolute_pe, "enable_residual_attribute": res}
        m = (ae.UpscaleResModule if res else ae.UpscaleModule)(norm_layer=norm_layer, **ctor).double()
        set_parameters(m, gen)
        m.eval()
        inp = common(gen, cin)
        if res:
            inp["attribute"] = q(randn(gen, sum(COUNTS), ATTR))
        seen = {}
        hooks = [m.delta_x.register_forward_hook(lambda mod, a, out: seen.__setitem__("t", out)),
                 m.out_norm.register_forward_pre_hook(lambda mod, a: seen.__setitem__("y", a[0].feat))]
        leaves = ("coord", "feat") + (("global_feat",) if ada else ()) + (("attribute",) if res else ())
        p = point_of(ae, inp, grad=leaves)
        leaf = {k: p[k] for k in leaves}
        out = m(p)
        for h in hooks:
            h.remove()
        kinks = {"tanh_preact_max": float(seen["t"].abs().max()), "min_row_variance": float(min(inp["feat"].var(1, unbiased=False).min(),
                                                                                                   seen["y"].var(1, unbiased=False).min()))}
        if kinks["tanh_preact_max"] < 3.0 and kinks["min_row_variance"] > 1e-2:
            break
    else:
        raise AssertionError("no seed clear of the kinks")
    outs = {"coord": out.coord, "feat": out.feat}
    if res:
        outs["attribute"] = out.attribute
    ups = {k: q(randn(gen, *v.shape)) for k, v in outs.items()}
    sum((v * ups[k]).sum() for k, v in outs.items()).backward()
    meta = {"item": "upscale", "class": type(m).__name__, "ctor": ctor, "norm": "ada" if ada else "ln", "global_channels": GLOBAL,
            "grid_size": GRID, "counts": list(COUNTS), "seed": seed, "kinks": kinks, "keys": sorted(out.keys())}
    main = state_arrays(m)
    main.update({"in/" + k: stored_in(v) for k, v in inp.items()})
    main.update({"up/" + k: stored_in(v) for k, v in ups.items()})
    main.update({"out/" + k: np64(v) for k, v in outs.items()})
    main["out/offset"] = out.offset.numpy()
    main.update({"gin/" + k: np64(v.grad) for k, v in leaf.items()})
    print(f"pointdec_{name}: seed {seed}, {kinks}")
    write(name, meta, main, param_grads(m))


# ---- masks --------------------------------------------------------------------------------------------------------------------

def cut_margins(x, mask, offset, ratio, sampling):
    """per segment: how many rows are selected, the gap between the last selected and the first unselected score and, for
    top-p, the distance of the two prefix sums that straddle the ratio (as every dtype rounds it) from it"""
    x, mask = np.asarray(x, dtype=np.float64), np.asarray(mask, dtype=bool)
    ratio_lo, ratio_hi = min(ratio, float(torch.tensor(ratio).bfloat16())), max(ratio, float(torch.tensor(ratio).bfloat16()))
    ks, gaps, prefix_margin, a = [], [], [], 0
    for e in np.asarray(offset).tolist():
        s = np.sort(x[a:e])[::-1]
        k = int(mask[a:e].sum())
        ks.append(k)
        if not 0 < k < e - a or not np.array_equal(np.sort(x[a:e][mask[a:e]])[::-1], s[:k]):
            return None
        gaps.append(float(s[k - 1] - s[k]))
        if sampling == "topp":
            c = np.cumsum(s)
            prefix_margin.append(float(min(ratio_lo - c[k - 1], c[k] - ratio_hi)))
        a = e
    return {"k": ks, "gap": gaps, "prefix_margin": prefix_margin}


def sorted_scores(x, offset):
    x, a, srt, pre = np.asarray(x, dtype=np.float64), 0, [], []
    for e in np.asarray(offset).tolist():
        s = np.sort(x[a:e])[::-1]
        srt.append(s)
        pre.append(np.cumsum(s))
        a = e
    return np.concatenate(srt), np.concatenate(pre)


def selection_is_safe(m, calls64, lower_calls, ratio, sampling, offset):
    """-> the margins, or None where the seed does not hold the conditions"""
    c = calls64[0]
    marg = cut_margins(c["x"], c["mask"], offset, ratio, sampling)
    if marg is None or len(set(marg["k"])) == 1 or (sampling == "topp" and min(marg["k"]) < 3):
        return None
    diffs = {}
    for tag, low in lower_calls.items():
        if not torch.equal(low[0]["mask"], c["mask"]) or not torch.equal(low[0]["offset"], c["offset"]):
            return None
        diffs[tag] = float((low[0]["x"].double() - c["x"]).abs().max())
    worst = max(diffs.values())
    if min(marg["gap"]) < SAFETY * worst:
        return None
    extra = {}
    if sampling == "topp":
        # the prefix sums as each lower-precision run forms them (float32 sums of its own ranked scores, rounded to its dtype),
        # at the ranks up to the first unselected one, against the float64 run's
        extra["prefix_diff"] = {}
        for tag, low in lower_calls.items():
            worst_prefix, a = 0.0, 0
            for e, k in zip(np.asarray(offset).tolist(), marg["k"]):
                ranked = torch.sort(low[0]["x"][a:e], descending=True)[0]
                mine = torch.cumsum(ranked.float(), 0).to(ranked.dtype).double()[:k + 1]
                exact = torch.cumsum(torch.sort(c["x"][a:e], descending=True)[0], 0)[:k + 1]
                worst_prefix = max(worst_prefix, float((mine - exact).abs().max()))
                a = e
            extra["prefix_diff"][tag] = worst_prefix
        if min(marg["prefix_margin"]) < SAFETY * max(extra["prefix_diff"].values()):
            return None
    return dict(marg, score_diff=diffs, safety=SAFETY, **extra)


def mask_record(ae, name, res, sampling, ratio, temperature, seed):
    cls = ae.MaskResModule if res else ae.MaskModule
    ctor = {"dim": CHANNELS, "temperature": temperature, "non_leaf_ratio": ratio, "mask_sampling_type": sampling}
    lib = contextlib.nullcontext if not res else to_float32_keeps_float64
    for seed in range(seed, seed + 20000):
        gen = torch.Generator().manual_seed(seed)
        m = cls(**ctor).double()
        set_parameters(m, gen)
        m.eval()
        inp = common(gen)
        if ratio == 1.0:
            margins = {}
            with tapped(ae) as calls:
                p = point_of(ae, inp)
                out = m(p)
            assert not calls and not list(m.parameters())
            break
        with torch.no_grad():
            if not res and sampling == "topp":      # sigmoid scores near 0.09, so that several of them sum to the ratio
                m.net[2].weight.copy_(q(m.net[2].weight * 0.25))
                m.net[2].bias.copy_(q(torch.tensor([-2.3], dtype=F64)))
            elif sampling == "topp":                # a flat softmax, for the same reason
                m.net[2].weight.copy_(q(m.net[2].weight * 0.4))
            elif not res:                           # spread the sigmoids
                m.net[2].weight.copy_(q(m.net[2].weight * 3.0))
        with tapped(ae) as calls, lib():
            p = point_of(ae, inp, grad=("feat",))
            feat = p.feat
            out = m(p)
        lower_calls = {}
        with tapped(ae) as low:
            lowered(m, lambda mm, dt: mm(point_of(ae, inp, dt)))
        lower_calls["f32"], lower_calls["bf16_autocast"] = low[:1], low[1:]
        margins = selection_is_safe(m, calls, lower_calls, ratio, sampling, inp["offset"])
        if margins is not None:
            break
    else:
        raise AssertionError("no seed with a safe selection")
    print(f"pointdec_{name}: seed {seed}, margins {margins}")
    meta = {"item": "mask", "class": cls.__name__, "ctor": ctor, "grid_size": GRID, "counts": list(COUNTS), "seed": seed,
            "margins": margins, "keys": list(out.keys())}
    main = state_arrays(m)
    main.update({"in/" + k: stored_in(v) for k, v in inp.items()})
    pgrad = {}
    if ratio == 1.0:
        leaf = out.leaf_point
        meta["leaf_keys"] = list(leaf.keys())
        meta["identities"] = {f"{a}.{k}": bool(pt[k] is p[k]) for a, pt in (("point", out), ("leaf_point", leaf))
                              for k in ("coord", "feat", "offset")}
        meta["identities"]["point.global_feat"] = bool(out.global_feat is p.global_feat)
        assert all(meta["identities"].values()) and out.grid_size == leaf.grid_size == GRID
    elif not res:
        leaf = out.leaf_point
        meta["leaf_keys"] = list(leaf.keys())
        assert out.grid_size == leaf.grid_size == GRID and out.global_feat is p.global_feat
        c = calls[0]
        ups = {"feat": q(randn(gen, *out.feat.shape)), "leaf_feat": q(randn(gen, *leaf.feat.shape))}
        ((out.feat * ups["feat"]).sum() + (leaf.feat * ups["leaf_feat"]).sum()).backward()
        main.update({"up/" + k: stored_in(v) for k, v in ups.items()})
        main.update({"out/coord": np64(out.coord), "out/feat": np64(out.feat), "out/offset": out.offset.numpy(),
                     "out/leaf_coord": np64(leaf.coord), "out/leaf_feat": np64(leaf.feat), "out/leaf_offset": leaf.offset.numpy(),
                     "out/non_leaf": c["mask"].numpy(), "aux/prob": np64(c["x"])})
        main["aux/sorted"], main["aux/prefix"] = sorted_scores(c["x"], inp["offset"])
        main["gin/feat"] = np64(feat.grad)
        pgrad = param_grads(m)
    else:
        assert out is p
        c = calls[0]
        up = q(randn(gen, *out.feat.shape))
        (out.feat * up).sum().backward()
        main["up/feat"] = stored_in(up)
        main.update({"out/feat": np64(out.feat), "out/raw_prob": np64(out.raw_prob), "out/prob": np64(out.prob),
                     "out/non_leaf": out.non_leaf.numpy(), "out/non_leaf_offset": out.non_leaf_offset.numpy(),
                     "out/leaf": out.leaf.numpy(), "out/leaf_offset": out.leaf_offset.numpy(), "aux/prob": np64(c["x"])})
        main["aux/sorted"], main["aux/prefix"] = sorted_scores(c["x"], inp["offset"])
        main["gin/feat"] = np64(feat.grad)
        pgrad = param_grads(m)
    write(name, meta, main, pgrad)


# ---- heads --------------------------------------------------------------------------------------------------------------------

def head_record(ae, name, res, seed):
    gen = torch.Generator().manual_seed(seed)
    ctor = {"is_first": not res, "dim": CHANNELS, "sh_degree": 1, "enable_residual_attribute": res}
    m = (ae.GaussianResModule if res else ae.GaussianModule)(**ctor).double()
    set_parameters(m, gen)
    m.eval()
    inp = common(gen)
    leaves = ("feat",)
    if res:
        inp["attribute"] = q(randn(gen, sum(COUNTS), ATTR))
        leaves = ("feat", "attribute")
        p = point_of(ae, inp, grad=leaves)
        leaf = {k: p[k] for k in leaves}
        out = m(p)
        attribute = out.attribute
    else:
        inner = point_of(ae, {k: inp[k] for k in ("coord", "feat", "offset")}, grad=leaves)
        leaf = {"feat": inner.feat}
        out = m(ae.Point(leaf_point=inner))
        assert out.leaf_point is inner
        attribute = inner.attribute
    up = q(randn(gen, *attribute.shape))
    (attribute * up).sum().backward()
    meta = {"item": "head", "class": type(m).__name__, "ctor": ctor, "counts": list(COUNTS), "seed": seed, "grid_size": GRID}
    main = state_arrays(m)
    main.update({"in/" + k: stored_in(v) for k, v in inp.items()})
    main.update({"up/attribute": stored_in(up), "out/attribute": np64(attribute)})
    main.update({"gin/" + k: np64(v.grad) for k, v in leaf.items()})
    write(name, meta, main, param_grads(m))


# ---- the chain ----------------------------------------------------------------------------------------------------------------

CHAIN_COUNTS = (20, 14)     # fewer rows than the modules' records: the cut of 56 + 40 scores is rarely 8 bf16 errors wide
CHAIN = {"dec_channels": (16, 8), "dec_num_head": (2, 1), "patch_size": 8, "upscale_factor": 2, "n_frequencies": 10, "stride": 2,
         "non_leaf_ratio": 0.6, "temperature": 1.0, "sh_degree": 1, "n_coarse": 30}


def build_stages(ae, kind):
    ch, stages = CHAIN["dec_channels"], []
    ln = partial(ae.AdaLayerNorm, w_shape=ch[0]) if kind == "ada" else partial(torch.nn.LayerNorm, elementwise_affine=False)
    for s in range(len(ch)):
        dec = ae.PointSequential()
        if s == 0 and kind == "ada":
            dec.add(ae.GlobalPooling(), name="global")
        if s > 0:
            dec.add(ae.SerializationModule(stride=CHAIN["stride"], order=ORDER, shuffle_orders=False, enable_residual_attribute=False),
                    name="serialization")
        dec.add(ae.Block(channels=ch[s], num_heads=CHAIN["dec_num_head"][s], patch_size=CHAIN["patch_size"], drop_path=0.0,
                         norm_layer=ln, order_index=0, cpe_indice_key=f"stage{s}", enable_flash=False, upcast_attention=False,
                         upcast_softmax=False), name="block0")
        cout = ch[s + 1] if s < len(ch) - 1 else ch[s]
        dec.add(ae.UpscaleModule(is_first=s == 0, in_channels=ch[s], out_channels=cout, upscale_factor=CHAIN["upscale_factor"],
                                 n_frequencies=CHAIN["n_frequencies"], drop_path=0.0, enable_absolute_pe=False,
                                 enable_residual_attribute=False, norm_layer=ln), name="up")
        dec.add(ae.MaskModule(dim=cout, temperature=CHAIN["temperature"],
                              non_leaf_ratio=CHAIN["non_leaf_ratio"] if s < len(ch) - 1 else 1.0, mask_sampling_type="topk"), name="mask")
        dec.add(ae.GaussianModule(is_first=s == 0, dim=cout, sh_degree=CHAIN["sh_degree"], enable_residual_attribute=False), name="head")
        stages.append(dec)
    return torch.nn.ModuleList(stages)


def snapshot(point, prefix):
    """the tensors of a point under prefix + key (a leaf_point under prefix + "leaf/"), and its key lists and scalars"""
    arrays, info = {}, {"keys": list(point.keys()), "scalars": {}}
    for k, v in point.items():
        if k == "leaf_point":
            a, i = snapshot(v, prefix + "leaf/")
            arrays.update(a)
            info["leaf"] = i
        elif isinstance(v, torch.Tensor):
            arrays[prefix + k] = v
        elif k == "sparse_shape":
            arrays[prefix + k] = torch.tensor(v)
        elif isinstance(v, (int, float)):
            info["scalars"][k] = v
    return arrays, info


def cell_position(coord, grid_size):
    return (coord - coord.min(0)[0]) / grid_size


def run_chain(ae, stages, inp, dtype, only_stage=None):
    """the lines of Network.forward around `for dec in self.dec`; -> the snapshots, the leaf points and the taps"""
    point = ae.Point(coord=inp["coord"].to(dtype), feat=inp["feat"].to(dtype), offset=inp["offset"], grid_size=GRID)
    point.serialization(order=ORDER, shuffle_orders=False)
    point.sparsify()
    arrays, info, out_points, cells = {}, {}, [], [cell_position(point.coord, point.grid_size)]
    seen = {}
    hooks = [stages[1].serialization.register_forward_hook(lambda mod, a, out: seen.__setitem__("serial", snapshot(out, "s1/serial/")))]
    hooks += [stages[0].mask.register_forward_pre_hook(lambda mod, a: seen.__setitem__("mask_in", snapshot(a[0], "s0/mask_in/")))]
    hooks += [stages[s].up.delta_x.register_forward_hook(lambda mod, a, out, s=s: seen.__setitem__(f"t{s}", out)) for s in range(2)]
    variances = []
    hooks += [m.register_forward_pre_hook(lambda mod, a: variances.append(float(a[0].detach().double().var(1, unbiased=False).min())))
              for m in stages.modules() if isinstance(m, torch.nn.LayerNorm)]
    with tapped(ae) as calls:
        for s, dec in enumerate(stages):
            a, i = snapshot(point, f"s{s}/in/")
            arrays.update(a)
            info[f"s{s}/in"] = i
            if s > 0:
                cells.append(cell_position(point.coord, point.grid_size / CHAIN["stride"]))
            point = dec(point)
            a, i = snapshot(point, f"s{s}/out/")
            arrays.update(a)
            info[f"s{s}/out"] = i
            out_points.append(point.leaf_point)
            if only_stage == s:
                break
    for h in hooks:
        h.remove()
    if "mask_in" in seen:
        arrays.update({k: v for k, v in seen["mask_in"][0].items() if k.rsplit("/", 1)[1] in ("coord", "feat", "offset")})
    if "serial" in seen:
        arrays.update(seen["serial"][0])
        info["s1/serial"] = seen["serial"][1]
    if calls:
        arrays["s0/non_leaf"] = calls[0]["mask"]
    return {"arrays": arrays, "info": info, "leaf_points": out_points, "calls": calls, "cells": cells, "min_row_variance": min(variances),
            "tanh": max(float(seen[f"t{s}"].abs().max()) for s in range(2) if f"t{s}" in seen)}


def five_concatenations():
    """the five lines of Network.forward that build the fine set, as they stand in the reference's text"""
    with open(os.path.join(REF, "lightning", "network.py")) as f:
        lines = f.read().splitlines()
    first = next(i for i, l in enumerate(lines) if l.strip().startswith("_centers = torch.cat([xyz_pt"))
    block = lines[first:first + 5]
    assert [l.split("=")[0].strip() for l in block] == ["_centers", "_shs", "_opacity", "_scaling", "_rotation"]
    return compile(textwrap.dedent("\n".join(block)), "network.py:fine-set", "exec")


def no_shared_cell(arrays):
    for key in ("s0/in/", "s1/serial/"):
        cells = torch.cat([arrays[key + "batch"].reshape(-1, 1).long(), arrays[key + "grid_coord"].long()], 1)
        if len(torch.unique(cells, dim=0)) != len(cells):
            return False
    return True


def chain_record(ae, net, name, kind, seed):
    cats = five_concatenations()
    for seed in range(seed, seed + 20000):
        gen = torch.Generator().manual_seed(seed)
        stages = build_stages(ae, kind).double()
        set_parameters(stages, gen)
        with torch.no_grad():
            w = stages[0].mask.net[2].weight
            w.copy_(q(w * 3.0))
            for dec in stages:      # the two children of a parent leave it in opposite directions: siblings share no cell
                last = dec.up.delta_x[2]
                last.weight.copy_(q(last.weight * 0.5))
                last.bias.copy_(q(torch.tensor([1.2, -1.2], dtype=F64).repeat_interleave(3) + 0.2 * randn(gen, 6)))
        stages.eval()
        n = sum(CHAIN_COUNTS)
        inp = {"coord": q(torch.rand(n, 3, generator=gen, dtype=F64) * 4.0 + torch.tensor([1.3, -2.1, 0.6], dtype=F64)),
               "feat": q(randn(gen, n, CHAIN["dec_channels"][0]) * 1.2 + 0.2), "offset": torch.tensor(CHAIN_COUNTS).cumsum(0)}
        leaves = {k: inp[k].clone().requires_grad_(True) for k in ("coord", "feat")}
        run = run_chain(ae, stages, dict(inp, **leaves), F64)
        if run["tanh"] >= 3.0 or run["min_row_variance"] < 1e-2 or not no_shared_cell(run["arrays"]):
            continue
        marg = cut_margins(run["calls"][0]["x"], run["calls"][0]["mask"], run["arrays"]["s0/out/offset"] + run["arrays"]["s0/out/leaf/offset"],
                           CHAIN["non_leaf_ratio"], "topk")
        if marg is None or len(set(marg["k"])) == 1 or min(marg["gap"]) < 0.03:
            continue
        # the float32 run, free-running; under bf16 autocast the MaskModule alone, fed the float64 run's own input: behind a
        # Block and an UpscaleModule in bf16 the scores differ by 0.02 to 0.1, and no cut among 40 scores is 8 times that wide
        s32 = copy.deepcopy(stages).float()
        with torch.no_grad():
            low = run_chain(ae, s32, inp, torch.float32)
            fed = {k: run["arrays"]["s0/mask_in/" + k].detach() for k in ("coord", "feat", "offset")}
            with tapped(ae) as low16, torch.autocast("cpu", dtype=torch.bfloat16):
                s32[0].mask(ae.Point(coord=fed["coord"].float(), feat=fed["feat"].float(), offset=fed["offset"], grid_size=GRID))
        if not all(torch.equal(r[0]["mask"], run["calls"][0]["mask"]) for r in (low["calls"], low16)):
            continue
        diffs = {"f32": float((low["calls"][0]["x"].double() - run["calls"][0]["x"]).abs().max()),
                 "bf16_autocast_mask_alone": float((low16[0]["x"].double() - run["calls"][0]["x"]).abs().max())}
        if min(marg["gap"]) < SAFETY * max(diffs.values()):
            continue
        cell_err = max(float((a.double() - b).abs().max()) for a, b in zip(low["cells"], run["cells"]))
        border = []
        for u in run["cells"]:
            u = u.detach()
            d = torch.minimum(u - u.floor(), u.ceil() - u)
            border.append(float(d[u != 0].min()))           # (the point that attains the minimum sits at 0 exactly in every dtype)
        if min(border) < SAFETY * cell_err:
            continue
        break
    else:
        raise AssertionError("no seed holds the chain's conditions")
    # for the record: the scores of the reference's own bf16-autocast run of the WHOLE stage 0 against the float64 ones
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        free = run_chain(ae, s32, inp, torch.float32, only_stage=0)
    free_running = float((free["calls"][0]["x"].double() - run["calls"][0]["x"]).abs().max())
    margins = dict(bf16_autocast_stage0_free_running_score_diff=free_running, **dict(marg, score_diff=diffs, cell_error_f32=cell_err, cell_border=border, safety=SAFETY, tanh_preact_max=run["tanh"],
                   min_row_variance=run["min_row_variance"]))
    print(f"pointdec_{name}: seed {seed}, margins {margins}")
    for k in low["arrays"]:
        if not low["arrays"][k].dtype.is_floating_point:
            assert torch.equal(low["arrays"][k], run["arrays"][k]), k

    # the union and the five concatenations against a coarse set
    sh_dim = 3 * (CHAIN["sh_degree"] + 1) ** 2
    me = types.SimpleNamespace(cfg=types.SimpleNamespace(model=types.SimpleNamespace(use_mask=True)), sh_dim=sh_dim, opacity_dim=1,
                               scaling_dim=3, rotation_dim=4, sh_degree=CHAIN["sh_degree"], opacity_shift=-2.1792, fine_scaling_shift=-5.5)
    xyz_pt, shs_pt, opacity_pt, scaling_pt, rotation_pt = net.Network._union_gaussians(me, point_list=run["leaf_points"])
    nc = CHAIN["n_coarse"]
    mask = torch.rand(nc, generator=gen) < 0.7
    n_masked = int(mask.sum())
    selected = torch.rand(n_masked, generator=gen) < 0.5
    coarse = {"centers_coarse": q(randn(gen, nc, 3)), "opacity_coarse": q(randn(gen, nc, 1)), "scaling_coarse": q(randn(gen, nc, 3)),
              "rotation_coarse": q(randn(gen, nc, 4)), "shs_fine": q(randn(gen, n_masked, sh_dim // 3, 3))}
    assert 0 < int(selected.sum()) < n_masked < nc
    scope = {"torch": torch, "self": me, "i": 0, "xyz_pt": xyz_pt, "shs_pt": shs_pt, "opacity_pt": opacity_pt, "scaling_pt": scaling_pt,
             "rotation_pt": rotation_pt, "mask": mask, "selected_pts_mask": selected, "_centers_coarse": [coarse["centers_coarse"]],
             "_opacity_coarse": [coarse["opacity_coarse"]], "_scaling_coarse": [coarse["scaling_coarse"]],
             "_rotation_coarse": [coarse["rotation_coarse"]], "_shs_fine": coarse["shs_fine"]}
    with float_is_identity_on_float64():
        exec(cats, scope)
    finals = {k: scope["_" + k] for k in ("centers", "shs", "opacity", "scaling", "rotation")}
    assert all(v.dtype == F64 for v in finals.values())
    ups = {k: q(randn(gen, *v.shape)) for k, v in finals.items()}
    sum((v * ups[k]).sum() for k, v in finals.items()).backward()

    meta = {"item": "chain", "norm": kind, "chain": CHAIN, "order": list(ORDER), "grid_size": GRID, "counts": list(CHAIN_COUNTS), "seed": seed,
            "margins": margins, "points": run["info"], "opacity_shift": me.opacity_shift, "fine_scaling_shift": me.fine_scaling_shift,
            "sh_dim": sh_dim, "stage_modules": [list(dict(dec.named_children())) for dec in stages]}
    main = {}
    for s, dec in enumerate(stages):
        main.update(state_arrays(dec, f"state/s{s}."))
    main.update({"in/" + k: stored_in(v) for k, v in inp.items()})
    main.update({"in/" + k: stored_in(v) for k, v in coarse.items()})
    main.update({"in/mask": mask.numpy(), "in/selected_pts_mask": selected.numpy()})
    for k, v in run["arrays"].items():
        main[k] = np64(v) if v.dtype.is_floating_point else v.detach().numpy()
    main["aux/prob"] = np64(run["calls"][0]["x"])
    main.update({"up/" + k: stored_in(v) for k, v in ups.items()})
    main.update({"out/" + k: np64(v) for k, v in finals.items()})
    main.update({"gin/" + k: np64(v.grad) for k, v in leaves.items()})
    pgrad = {}
    for s, dec in enumerate(stages):
        pgrad.update(param_grads(dec, f"gparam/s{s}."))
    write(name, meta, main, pgrad)


def main():
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    ae, net = load()
    upscale_record(ae, "up_ln", False, 16, 16, 2, ada=False, absolute_pe=False, seed=100)
    upscale_record(ae, "up_ada", False, 24, 16, 2, ada=True, absolute_pe=True, seed=200)
    upscale_record(ae, "up_res", True, 16, 16, 3, ada=True, absolute_pe=False, seed=300)
    mask_record(ae, "mask_topk", False, "topk", 0.6, 1.0, seed=1000)
    mask_record(ae, "mask_topp", False, "topp", 0.6, 1.0, seed=2000)
    mask_record(ae, "mask_res_topk", True, "topk", 0.6, 0.5, seed=3000)
    mask_record(ae, "mask_res_topp", True, "topp", 0.6, 0.5, seed=4000)
    mask_record(ae, "mask_full", False, "topk", 1.0, 1.0, seed=5000)
    head_record(ae, "head", False, seed=600)
    head_record(ae, "head_res", True, seed=700)
    chain_record(ae, net, "chain_ln", "ln", seed=8000)
    chain_record(ae, net, "chain_ada", "ada", seed=9000)


if __name__ == "__main__":
    main()
