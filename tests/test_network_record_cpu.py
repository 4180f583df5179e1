"""CPU: the project's yardsticks (the torch forwards the GPU tests judge the HIP kernels by) against runs of the reference's own
decoder classes recorded in float64 (tests/golden/network_*.npz, tests/network_record.py).  Reads tests/golden only.

Tolerance, for every recorded output and gradient b: max|a - b| <= 1e-9 max|b|.  Both sides are float64 torch on the same values
over sums of at most a few thousand terms, so their rounding is near 1e-12: 1e-9 leaves three decades and sits six below
bfloat16.  Where the reference returns float32 (forward_coarse, forward_fine) the outputs get half a float32 ulp at max|b| on top.
A mutant of a yardstick must land beyond 100 times that tolerance on at least one recorded tensor."""
import copy

import numpy as np
import pytest
import torch

import groupattn_ref as GR
import network_record as NR
from norm_ref import half_ulp

F64 = torch.float64


def tolerance(rec, key, b):
    top = float(np.abs(b).max()) if b.size else 0.0
    f32_out = key.startswith("out/") and rec.meta["call"].get("out_dtypes", {}).get(key[4:]) == "torch.float32"
    return 1e-9 * top + (half_ulp(torch.float32, top) if f32_out else 0.0)


def distances(rec, got):
    """{key: (max|a - b| over the common shape, tolerance)} for every recorded tensor"""
    res = {}
    want = NR.expected(rec)
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    for key, b in want.items():
        a = got[key].detach().double().numpy()
        if a.shape != b.shape:      # (a mutant that moves a cut: compared over the common corner)
            common = tuple(slice(0, min(m, n)) for m, n in zip(a.shape, b.shape))
            a, b = a[common], b[common]
        res[key] = (float(np.abs(a - b).max()) if b.size else 0.0, tolerance(rec, key, b))
    return res


def yard_run(rec, forward=None, prepare=None):
    m = NR.stand_in(rec, dtype=F64)
    if prepare is not None:
        prepare(m)
    return NR.run(rec, m, forward or NR.yardstick(rec), F64)


# ---- the records themselves ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NR.RECORDS)
def test_record_values_are_bfloat16_representable_inside_float16s_normal_range(name):
    rec = NR.load(name)
    values = {**{"state/" + k: v for k, v in rec.state.items()}, **{"in/" + k: v for k, v in rec.inputs.items() if k != "group_centers" and v.dtype.kind == "f"},
              **{"up/" + k: v for k, v in rec.ups.items()}}
    for key, a in values.items():
        t = torch.from_numpy(np.array(a, dtype=np.float64))
        assert torch.equal(t.to(torch.bfloat16).double(), t), key
        assert float(t.abs().min()) >= 2.0 ** -14 and float(t.abs().max()) <= 65504, key
    assert all(a.dtype == np.float32 for a in rec.state.values())
    assert set(rec.ups) <= set(rec.outputs) and rec.gin and (rec.gparam or rec.item == "point_feats")
    # moved off their initial values: no bias is zero, no LayerNorm weight is one
    for k, a in rec.state.items():
        if a.ndim == 1:
            assert np.abs(a).min() > 0 and not np.all(a == 1.0), k


def test_low_variance_rows_are_there():
    """the rows a LayerNorm reads directly include some with a variance near 1e-3"""
    for name, rows in (("group_block_h4", np.moveaxis(NR.load("group_block_h4").inputs["x"], 1, -1)),
                       ("mod_ln", NR.load("mod_ln").inputs["x"]), ("fine_v2", NR.load("fine_v2").inputs["volume_feat"])):
        var = rows.reshape(-1, rows.shape[-1]).var(-1)
        assert (var < 2e-3).mean() >= 0.2 and (var > 3e-4).all(), (name, var.min())


def test_decoder_inputs_keep_clear_of_the_relu_kinks():
    """what the ReLUs of the recorded runs see stays 0.05 from zero (a 16-bit run would otherwise switch units)"""
    for name in ("coarse_k1", "coarse_k2", "fine_v2", "fine_v4"):
        rec = NR.load(name)
        m = NR.stand_in(rec, dtype=F64)
        ins = {k: torch.from_numpy(np.array(v)) for k, v in rec.inputs.items()}
        with torch.no_grad():
            if rec.item == "coarse":
                z1 = m.mlp_coarse[0](ins["feats"])
                z = torch.cat((z1, m.mlp_coarse[2](torch.relu(z1))), dim=-1)
            else:
                z = m.mlp_fine[0](m.cross_att(m.norm(ins["volume_feat"])[:, None], ins["point_feats"], ins["point_feats"], need_weights=False)[0])
        assert float(z.abs().min()) >= 0.05 and (z > 0).any() and (z < 0).any(), (name, float(z.abs().min()))


@pytest.mark.parametrize("name", NR.RECORDS)
def test_stand_in_takes_the_recorded_state_strictly_and_has_the_recorded_attributes(name):
    rec = NR.load(name)
    m = NR.stand_in(rec)                                           # load_state_dict(strict=True) inside
    for k, p in m.state_dict().items():
        assert p.dtype == torch.float32 and np.array_equal(p.numpy(), rec.state[k]), k
    live, mine = rec.meta["attrs"], NR.ATTRS[rec.item](m)
    assert set(NR.READ.get(rec.item, ())) <= set(mine)
    for k, v in mine.items():
        if k == "eps" and rec.item == "coarse":
            assert v == {}                                           # forward_coarse reads no norm
        else:
            assert v == live[k], (k, v, live[k])                     # every norm's eps, name by name, among them


def test_recorded_eps_and_attention_are_what_the_reference_builds():
    """what a restatement gets wrong quietly, read off the live instances"""
    blk = NR.load("group_block_h2").meta
    assert blk["ctor"]["eps"] == 1e-6 and blk["attrs"]["eps"] == {"norm1": 1e-5, "norm2": 1e-5, "norm3": 1e-5}
    vt = NR.load("vol_transformer").meta["attrs"]
    assert vt["eps"] == {"norm": 1e-6, **{f"layers.{i}.norm{j}": 1e-5 for i in (0, 1) for j in (1, 2, 3)}}
    assert vt["layer_calls"] == [{"group_axis": 2, "block_size": 2}, {"group_axis": 4, "block_size": 1}]
    assert NR.load("mod_ln").meta["attrs"]["eps"] == {"norm": 1e-6}
    dec = NR.load("fine_v2").meta["attrs"]
    assert dec["eps"] == {"norm": 1e-5} and dec["mlp_coarse_distinct"] == 5
    att = dec["cross_att"]
    assert (att["num_heads"], att["head_dim"], att["kdim"], att["qkv_same_embed_dim"], att["in_proj_bias"], att["out_proj_bias"]) == (
        16, 5, 8, False, False, False)
    assert {"cross_att.q_proj_weight", "cross_att.k_proj_weight", "cross_att.v_proj_weight", "cross_att.out_proj.weight"} <= set(
        NR.load("fine_v2").state) and not any("in_proj" in k for k in NR.load("fine_v2").state)


def test_the_two_decoder_stand_ins_share_out_the_decoders_state():
    coarse, fine = NR.load("coarse_k1"), NR.load("fine_v2")
    assert set(coarse.state) == set(fine.state)
    assert all(np.array_equal(coarse.state[k], fine.state[k]) for k in coarse.state)      # one Decoder(K = 1)
    a, b = set(NR.state_for(coarse)), set(NR.state_for(fine))
    assert a and b and not a & b and a | b == set(coarse.state)
    assert set(coarse.gparam) == a and set(fine.gparam) == b


# ---- the yardsticks reproduce the records -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NR.RECORDS)
def test_yardstick_reproduces_the_record(name):
    rec = NR.load(name)
    d = distances(rec, yard_run(rec))
    for key, (err, tol) in d.items():
        print(f"record-cpu {name}/{key}: err={err:.3e} tol={tol:.3e}")
    bad = {k: v for k, v in d.items() if not v[0] <= v[1]}
    assert not bad, bad


def test_cond_blocks_and_the_products_cond_equal_the_recorded_conds_exactly():
    """a pure permutation of the inputs: exact"""
    from generativedensification_amd import deconv3d as D

    rec = NR.load("vol_transformer")
    feats = torch.from_numpy(np.array(rec.inputs["image_feats"]))
    for i, call in enumerate(rec.meta["attrs"]["layer_calls"]):
        want = rec.outputs[f"cond_layer{i}"]
        assert np.array_equal(GR.cond_blocks(feats, call["group_axis"]).numpy(), want)
        assert np.array_equal(D._cond(feats, call["group_axis"], call["block_size"]).numpy(), want)


# ---- mutants ------------------------------------------------------------------------------------------------------------------

def _eps_1e6(m):
    for norm in (m.norm1, m.norm2, m.norm3):
        norm.eps = 1e-6


def _modulate_without_one(m, ins, call):
    import volcond_torch as T

    ss = m.mlp(ins["cond"])
    shift, scale = ss.chunk(2, dim=-1)
    return {"out": T.mod_layer_norm(ins["x"], torch.cat((shift, scale - 1), dim=-1), m.norm.weight, m.norm.bias, m.norm.eps)}


def _chunks_swapped(m, ins, call):
    import volcond_torch as T

    shift, scale = m.mlp(ins["cond"]).chunk(2, dim=-1)
    return {"out": T.mod_layer_norm(ins["x"], torch.cat((scale, shift), dim=-1), m.norm.weight, m.norm.bias, m.norm.eps)}


def _cut_one_column_off(m):
    m.feature_dim += 1


def _opacity_shift_on_scaling(m, ins, call):
    return NR.yard_coarse(m, ins, dict(call, scaling_shift=call["opacity_shift"]))


def _group_idx_zero(m):
    m.n_groups, m.block_size = m.n_groups[:1], m.block_size[:1]


def _unfold_axes_swapped(monkeypatch):
    """the cond lines with their first two unfold axes swapped, through the surface record GR.cond_blocks reads"""
    surface = copy.deepcopy(GR.surface())
    axes = surface["cond"]["unfold_axes"]
    axes[0], axes[1] = axes[1], axes[0]
    monkeypatch.setattr(GR, "surface", lambda: surface)

    def forward(m, ins, call):
        res = NR.yard_vol_transformer(m, ins, call)
        res.update({f"cond_layer{i}": GR.cond_blocks(ins["image_feats"], m.n_groups[i % len(m.n_groups)]) for i in range(len(m.layers))})
        return res

    return forward


MUTANTS = {
    "eps 1e-6 in the block's norms": ("group_block_h4", None, _eps_1e6),
    "x * scale + shift in modulate": ("mod_ln", _modulate_without_one, None),
    "shift and scale chunks swapped": ("mod_ln", _chunks_swapped, None),
    "the cut of forward_fine one column off": ("fine_v2", None, _cut_one_column_off),
    "opacity_shift added to scaling": ("coarse_k2", _opacity_shift_on_scaling, None),
    "the first two unfold axes of the cond swapped": ("vol_transformer", _unfold_axes_swapped, None),
    "group_idx fixed at 0": ("vol_transformer", None, _group_idx_zero),
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_a_mutant_of_the_yardstick_lands_beyond_100_tolerances(mutant, monkeypatch):
    name, forward, prepare = MUTANTS[mutant]
    rec = NR.load(name)
    if forward is _unfold_axes_swapped:
        forward = forward(monkeypatch)
    d = distances(rec, yard_run(rec, forward, prepare))
    key, (err, tol) = max(d.items(), key=lambda kv: kv[1][0] / kv[1][1] if kv[1][1] else 0.0)
    print(f"record-mutant '{mutant}' on {name}: furthest at {key}: distance={err:.3e} = {err / tol:.3e} x tolerance {tol:.3e}")
    assert err > 100 * tol, (mutant, key, err, tol)
    if mutant.startswith("eps"):
        top = float(np.abs(rec.outputs["out"]).max())
        assert d["out/out"][0] > 1e-3 * top            # a low-variance row moves by a fraction of a per cent, not by rounding


def test_the_reference_was_not_loaded():
    import sys

    assert "lightning.network" not in sys.modules and "tools.rsh" not in sys.modules
