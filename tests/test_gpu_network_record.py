"""GPU: the product forwards, bound onto the stand-ins that hold a recorded state_dict of the reference's own decoder classes,
against the float64 runs of those classes (tests/golden/network_*.npz through tests/network_record.py).  Reads tests/golden only.

Accuracy bar (the project's, as tests/test_gpu_conv3d.py states it), for every recorded output and gradient: with
e_hip = max|hip - record| and e_torch = max|torch - record|, e_hip <= 2 e_torch + half an ulp of the result dtype at max|record|.
`torch` is the project's yardstick (tests/network_record.py `yardstick`) on the same GPU in the same precision; the recorded
values are exact in float32, bfloat16 and float16, so one record is the truth "on the inputs as rounded" of every mode.  For
the items with a convolution in float32, torch's error is the larger of its two layouts (torch picks its algorithm by layout).
Every pair is printed before it is asserted.  Every case counts the launches of its kernels and lets the torch fall-back raise:
a record that runs torch on both sides would prove nothing.  No synchronisation inside a checked region, no out-of-range input,
nothing that looks at kernel code."""
import contextlib
import types

import numpy as np
import pytest
import torch

import network_record as NR
from norm_ref import half_ulp

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
MODES = {"fp32": (F32, None), "bf16-autocast": (F32, BF16), "fp16": (F16, None)}       # (module and inputs, autocast)


def f64(t):
    return t.detach().double().cpu().numpy()


def bar(what, hip, tors, ref64):
    """prints the pair, then hands it to settle; tors: the yardstick's runs (e_torch is the largest of their errors)"""
    for tor in tors:
        assert hip.dtype == tor.dtype and hip.shape == tor.shape == ref64.shape, (what, hip.dtype, tor.dtype, hip.shape, tor.shape, ref64.shape)
    e_hip = float(np.abs(f64(hip) - ref64).max())
    e_torch = max(float(np.abs(f64(tor) - ref64).max()) for tor in tors)
    slack = half_ulp(hip.dtype, float(np.abs(ref64).max()))
    print(f"record-bar {what}: e_hip={e_hip:.3e} e_torch={e_torch:.3e} half_ulp={slack:.3e}")
    assert np.isfinite(f64(hip)).all(), what
    return what, e_hip, e_torch, slack


def settle(results):
    bad = [(w, eh, et, s) for w, eh, et, s in results if not eh <= 2 * et + s]
    assert not bad, bad


@contextlib.contextmanager
def counted(monkeypatch, names, raising=()):
    """counts the calls of the library's entry points `names` while the block runs (the way tests/test_gpu_conv3d.py replaces
    one) and lets every (object, attribute) of `raising`, the torch fall-backs, raise"""
    from generativedensification_amd import _lib as L

    lib, counts = L.load(), dict.fromkeys(names, 0)

    def counting(name, real):
        def call(*args):
            counts[name] += 1
            return real(*args)

        return call

    def boom(what):
        def call(*args, **kwargs):
            raise AssertionError(f"the torch fall-back {what} ran in the HIP path")

        return call

    with monkeypatch.context() as mp:
        for name in names:
            mp.setattr(lib, name, counting(name, getattr(lib, name)))
        for obj, attr in raising:
            mp.setattr(obj, attr, boom(attr))
        yield counts


def judge(rec, tag, hip, tors, skip=()):
    want = NR.expected(rec)
    assert set(want) - set(skip) <= set(hip), sorted(set(want) - set(hip))
    settle([bar(f"{tag}/{k}", hip[k], [t[k] for t in tors], want[k]) for k in want if k not in skip])


def stand_ins(rec, mode, n=2):
    dtype, autocast = MODES[mode]
    return dtype, autocast, [NR.stand_in(rec, dtype=dtype, device=DEV) for _ in range(n)]


# ---- GroupAttBlock ------------------------------------------------------------------------------------------------------------

BLOCK_KERNELS = ("gdr_groupattn_patchify_norm_forward", "gdr_groupattn_forward", "gdr_groupattn_norm_unpatchify_forward",
                 "gdr_groupattn_patchify_norm_backward", "gdr_groupattn_backward", "gdr_groupattn_norm_unpatchify_backward",
                 "gdr_conv3d_forward")


def yard_block(channels_last):
    import groupattn_ref as GR

    def forward(m, ins, call):
        return {"out": GR.torch_forward(m, ins["x"], ins["cond"], call["group_axis"], call["block_size"], conv_channels_last=channels_last)}

    return forward


@pytest.mark.parametrize("backend", ["torch", "hip"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["group_block_h4", "group_block_h2"])
def test_group_block(name, mode, backend, monkeypatch):
    from generativedensification_amd import groupattn as G

    rec = NR.load(name)
    dtype, autocast, (bound, m) = stand_ins(rec, mode)
    type(bound).forward = G.group_att_block_forward                  # the binding, on the stand-in's class
    monkeypatch.setattr(G, "CONV_BACKEND", backend)
    conv_calls = []
    bound.cnn.register_forward_hook(lambda *a: conv_calls.append(1))
    raising = [(G.F, "scaled_dot_product_attention")] + ([(bound.cnn, "forward")] if backend == "hip" else [])
    with counted(monkeypatch, BLOCK_KERNELS, raising) as counts:
        hip = NR.run(rec, bound, lambda mod, ins, call: {"out": mod(ins["x"], ins["cond"], call["group_axis"], call["block_size"])},
                     dtype, DEV, autocast)
    assert all(counts[k] == 1 for k in BLOCK_KERNELS[:6]), counts
    # (the kernel's forward entry point is also the product of its input gradient)
    assert (counts["gdr_conv3d_forward"], len(conv_calls)) == ((2, 0) if backend == "hip" else (0, 1)), (counts, conv_calls)
    tors = [NR.run(rec, m, yard_block(cl), dtype, DEV, autocast) for cl in ((False, True) if mode == "fp32" else (False,))]
    assert hip["out/out"].dtype == (BF16 if autocast else dtype)
    judge(rec, f"{name}/{mode}/conv-{backend}", hip, tors)


# ---- VolTransformer -------------------------------------------------------------------------------------------------------------

def yard_transformer(channels_last):
    import deconv3d_ref as DR
    import groupattn_ref as GR

    def layer_forward(self, x, cond, group_axis, block_size):
        return GR.torch_forward(self, x, cond, group_axis, block_size, conv_channels_last=channels_last)

    def forward(m, ins, call):
        for layer in m.layers:
            type(layer).forward = layer_forward
        return {"out": DR.reference_forward(m, ins["image_feats"])}

    return forward


@pytest.mark.parametrize("mode", list(MODES))
def test_vol_transformer(mode, monkeypatch):
    from generativedensification_amd import deconv3d as D
    from generativedensification_amd import groupattn as G

    rec = NR.load("vol_transformer")
    dtype, autocast, (bound, m) = stand_ins(rec, mode)
    assert D.TAIL_BACKEND == "hip"
    seen = []

    def layer_forward(self, x, cond, group_axis, block_size):
        seen.append((cond, group_axis, block_size))
        return G.group_att_block_forward(self, x, cond, group_axis, block_size)

    for layer in bound.layers:
        type(layer).forward = layer_forward
    type(bound).forward = D.vol_transformer_forward
    kernels = BLOCK_KERNELS[:6] + ("gdr_deconv3d_forward", "gdr_deconv3d_grad_input", "gdr_deconv3d_grad_weight")
    raising = [(G.F, "scaled_dot_product_attention"), (bound.deconv, "forward"), (bound.norm, "forward")]
    with counted(monkeypatch, kernels, raising) as counts:
        hip = NR.run(rec, bound, lambda mod, ins, call: {"out": mod(ins["image_feats"])}, dtype, DEV, autocast)
    assert all(counts[k] == 2 for k in BLOCK_KERNELS[:6]) and all(counts[k] == 1 for k in kernels[6:]), counts
    # every layer was handed the recorded cond (a permutation of the input: exact in every mode) with the recorded arguments
    calls = rec.meta["attrs"]["layer_calls"]
    assert [(g, b) for _, g, b in seen] == [(c["group_axis"], c["block_size"]) for c in calls]
    for i, (cond, _, _) in enumerate(seen):
        assert np.array_equal(f64(cond), rec.outputs[f"cond_layer{i}"]), i
    tors = [NR.run(rec, m, yard_transformer(cl), dtype, DEV, autocast) for cl in ((False, True) if mode == "fp32" else (False,))]
    assert hip["out/out"].dtype == (BF16 if autocast else dtype) and hip["out/out"].is_contiguous()
    judge(rec, f"vol_transformer/{mode}", hip, tors, skip=[k for k in NR.expected(rec) if k.startswith("out/cond_layer")])


# ---- ModLN and build_feat_vol ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", list(MODES))
def test_mod_ln(mode, monkeypatch):
    from generativedensification_amd import volcond as V

    rec = NR.load("mod_ln")
    dtype, autocast, (bound, m) = stand_ins(rec, mode)

    def product(mod, ins, call):
        return {"out": V.mod_layer_norm(ins["x"], mod.mlp(ins["cond"]), mod.norm.weight, mod.norm.bias, mod.norm.eps)}

    kernels = ("gdr_volcond_modln_forward", "gdr_volcond_modln_backward")
    with counted(monkeypatch, kernels, [(bound.norm, "forward")]) as counts:
        hip = NR.run(rec, bound, product, dtype, DEV, autocast)
    assert all(counts[k] == 1 for k in kernels), counts
    judge(rec, f"mod_ln/{mode}", hip, [NR.run(rec, m, NR.yardstick(rec), dtype, DEV, autocast)])


@pytest.mark.parametrize("mode", ["fp32", "bf16-autocast"])      # (without autocast the reference's lines refuse 16-bit inputs:
def test_feat_vol(mode, monkeypatch):                            # grid_sample gets a float32 map and a 16-bit grid)
    import groupattn_ref as GR
    from generativedensification_amd import volcond as V

    rec = NR.load("feat_vol")
    dtype, autocast, (bound, m) = stand_ins(rec, mode)
    assert V.COND_BACKEND == "hip"
    conds = []

    def product(mod, ins, call):
        me = NR.feat_vol_self(rec, mod, dtype, DEV)
        args = NR.feat_vol_args(rec, ins, DEV)
        out = V.build_feat_vol(me, *args)
        # the conds of the volume transformer from the same inputs, in the launch per group size the product makes
        me.vol_decoder = types.SimpleNamespace(n_groups=[2, 4])
        me.cfg = types.SimpleNamespace(model=types.SimpleNamespace(view_embed_dim=0))
        with torch.no_grad():
            conds.extend(V.volume_conds(me, args[1], args[2], args[3], img_hw=call["img_hw"]))
        return {"out": out, "feats_dir": V.ray_sh(ins["tar_rays_down"][:, :call["n_views_sel"]])}

    kernels = ("gdr_volcond_ray_sh", "gdr_volcond_modln_forward", "gdr_volcond_sample_forward", "gdr_volcond_modln_backward",
               "gdr_volcond_sample_backward")
    with counted(monkeypatch, kernels, [(V, "_torch_feat_vol"), (bound.norm, "forward")]) as counts:
        hip = NR.run(rec, bound, product, dtype, DEV, autocast)
    assert counts == {"gdr_volcond_ray_sh": 3, "gdr_volcond_modln_forward": 2, "gdr_volcond_sample_forward": 3,
                      "gdr_volcond_modln_backward": 1, "gdr_volcond_sample_backward": 1}, counts
    tor = NR.run(rec, m, NR.yardstick(rec), dtype, DEV, autocast)
    with torch.autocast("cuda", enabled=False):
        tor["out/feats_dir"] = tor["out/feats_dir"].float()
    assert hip["out/out"].dtype == (BF16 if autocast else F32)
    judge(rec, f"feat_vol/{mode}", hip, [tor], skip=["out/volume_grid"])
    # volume_conds: the recorded volume regrouped (a permutation of recorded numbers) is the truth of each cond
    vol = torch.from_numpy(np.array(rec.outputs["out"]))
    results = []
    for g, cond in zip((2, 4), conds):
        want = GR.cond_blocks(vol, g).numpy()
        results.append(bar(f"feat_vol/{mode}/volume_conds[{g}]", cond, [GR.cond_blocks(tor["out/out"].to(cond.dtype), g)], want))
    settle(results)


# ---- Decoder ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["coarse_k1", "coarse_k2"])
def test_forward_coarse(name, mode, monkeypatch):
    from generativedensification_amd import coarsehead as CH

    rec = NR.load(name)
    dtype, autocast, (bound, m) = stand_ins(rec, mode)
    type(bound).forward_coarse = CH.decoder_forward_coarse          # the binding, on the stand-in's class
    assert CH.HEAD_BACKEND == "hip" and CH.covers(bound)

    def product(mod, ins, call):
        """the bound forward for the reference's five outputs; the centres from the fused coarse_gaussians (another launch:
        the gradients of the two add up to the recorded ones, which are linear in the upstream gradients)"""
        shifts = (call["opacity_shift"], call["scaling_shift"])
        outs = dict(zip(NR.COARSE_OUTPUTS, mod.forward_coarse(ins["feats"], *shifts)))
        outs["centers"] = CH.coarse_gaussians(mod, ins["feats"], ins["group_centers"], call["half_cell"], *shifts)[0]
        return outs

    kernels = ("gdr_coarsehead_forward", "gdr_coarsehead_backward")
    with counted(monkeypatch, kernels, [(CH, "_torch_forward_coarse")]) as counts:
        hip = NR.run(rec, bound, product, dtype, DEV, autocast)
    assert counts["gdr_coarsehead_forward"] == 2 and counts["gdr_coarsehead_backward"] >= 1, counts
    assert all(hip["out/" + k].dtype == F32 for k in NR.COARSE_OUTPUTS + ("centers",))
    judge(rec, f"{name}/{mode}", hip, [NR.run(rec, m, NR.yardstick(rec), dtype, DEV, autocast)])


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["fine_v2", "fine_v4"])
def test_forward_fine(name, mode, monkeypatch):
    from generativedensification_amd import viewattn as VA

    rec = NR.load(name)
    dtype, autocast, (bound, m) = stand_ins(rec, mode)
    type(bound).forward_fine = VA.decoder_forward_fine              # the binding, on the stand-in's class

    def product(mod, ins, call):
        return dict(zip(("features", "sh"), mod.forward_fine(ins["volume_feat"], ins["point_feats"])))

    kernels = ("gdr_viewattn_forward", "gdr_viewattn_backward")
    with counted(monkeypatch, kernels, [(bound.cross_att, "forward")]) as counts:
        hip = NR.run(rec, bound, product, dtype, DEV, autocast)
    assert all(counts[k] == 1 for k in kernels), counts
    assert hip["out/features"].dtype == hip["out/sh"].dtype == F32
    judge(rec, f"{name}/{mode}", hip, [NR.run(rec, m, NR.yardstick(rec), dtype, DEV, autocast)])


# ---- get_point_feats ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["fp32", "bf16-autocast"])      # (the kernels take float32, other float types under autocast)
def test_point_feats(mode, monkeypatch):
    from generativedensification_amd import pointfeat as PF

    rec = NR.load("point_feats")
    dtype, autocast, (bound, m) = stand_ins(rec, mode)

    def product(mod, ins, call):
        return {"point_feats": PF.point_feats(*NR.point_feats_args(ins, call)).permute(1, 2, 0)}

    kernels = ("gdr_point_feats_forward", "gdr_point_feats_backward")
    with counted(monkeypatch, kernels, [(PF.torch.nn.functional, "grid_sample")]) as counts:
        hip = NR.run(rec, bound, product, dtype, DEV, autocast)
    assert all(counts[k] == 1 for k in kernels), counts
    judge(rec, f"point_feats/{mode}", hip, [NR.run(rec, m, NR.yardstick(rec), dtype, DEV, autocast)])
