"""CPU: the stand-ins and restated forwards of the point decoder's densification stages against the recorded runs of the
reference's own classes (tests/golden/pointdec_*.npz, made by tests/golden/make_pointdec_record.py in float64).

Every record's state_dict loads into the existing stand-in of its class with strict=True.  Then the restated forwards —
upscale_ref.reference_forward and upscale._reference_tail, the finehead_ref forwards, pointdec_record's MaskModule /
MaskResModule / SerializationModule over densify_ref, scatter_ref and serial_ref, block_ref.restated_forward inside the chain,
finehead_ref.reference_assemble behind it — must give every recorded float output and gradient to 1e-12 of its largest entry
and every recorded integer and bool array exactly.  Measured: 0.0 on every per-module record (the same torch
operations in the same order) and 3.9e-14 on the chain (BASELINE §4-record-pointdec).

One deliberate mistake per line that can be misread lands at least 1e6 tolerances away (or on another integer array):
`cat([skip_f, pe])`, cos before sin, the gate value feat * non_leaf in MaskModule, leaf rows without the gate, floor for ceil,
grid_size not divided by the stride, a per-segment minimum, levels concatenated without the stable sort by batch, the two
shifts swapped.  Two conceivable mistakes have no mutant.  An order of shift and scale: the reference's AdaLayerNorm has a scale
and no shift, so there is nothing to swap.  `<` for `<=` in top_p: the two differ only where a prefix sum EQUALS the ratio, which
the recorder's margins (a cut 8 errors of the lower-precision runs wide) exclude by construction."""
import sys
import types

import numpy as np
import pytest
import torch

import finehead_ref as FR
import network_record as NR
import pointdec_record as P
import upscale_ref as UR

TOL = 1e-12
FAR = 1e6 * TOL


def compare(got, rec, prefixes, skip=()):
    """-> (worst relative error over the float arrays, the integer / bool arrays that differ)"""
    want = {k: v for k, v in rec["arrays"].items() if k.startswith(prefixes) and not k.endswith("/batch") and k not in skip}
    assert want and set(want) <= set(got), sorted(set(want) - set(got))
    errs, unequal = {}, []
    largest = max((float(np.abs(w).max()) for k, w in want.items() if k.startswith("gparam/")), default=0.0)
    for k, w in want.items():
        g = got[k]
        g = g.detach().numpy() if isinstance(g, torch.Tensor) else np.asarray(g)
        if w.dtype.kind == "f":
            assert w.dtype == np.float64, k
            # a parameter gradient that vanishes in exact arithmetic (the last bias in front of a softmax: the record holds 0 or the
            # round-off of one BLAS, 1e-17) has no largest entry of its own: it is held to the record's largest parameter gradient
            scale = float(np.abs(w).max())
            if k.startswith("gparam/") and scale < 1e-9 * largest:
                scale = largest
            errs[k] = float(np.abs(g - w).max() / scale) if g.shape == w.shape else float("inf")
        elif g.shape != w.shape or not np.array_equal(g, w):
            unequal.append(k)
    return errs, unequal


def grads(leaves, modules):
    got = {"gin/" + k: (torch.zeros_like(v) if v.grad is None else v.grad) for k, v in leaves.items()}
    for prefix, m in modules.items():
        got.update({f"gparam/{prefix}{k}": (torch.zeros_like(v) if v.grad is None else v.grad) for k, v in m.named_parameters()})
    return got


def settle(tag, errs, unequal):
    worst = max(errs, key=errs.get)
    print(f"pointdec-record {tag}: worst {errs[worst]:.2e} at {worst}, {len(errs)} float arrays, unequal integers {unequal}")
    assert not unequal and errs[worst] <= TOL, (tag, unequal, {k: v for k, v in errs.items() if v > TOL})


def far(tag, errs, unequal, on=None):
    worst = max(errs.values()) if errs else 0.0
    print(f"pointdec-record {tag}: worst {worst:.2e}, unequal integers {unequal}")
    assert unequal or worst >= FAR, tag
    if on is not None:
        assert any(k in unequal or errs.get(k, 0.0) >= FAR for k in on), (tag, on)


# ---- the records themselves -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", P.NAMES)
def test_record_is_small_finite_and_representable(name):
    import os

    rec = P.load(name)
    for path in P.files(name):
        assert os.path.getsize(path) <= P.CAP, path
    for k, a in rec["arrays"].items():
        assert a.dtype.kind in "iub" or np.isfinite(a).all(), k
        if k.startswith(("in/", "up/", "state/")) and a.dtype.kind == "f" and not k.endswith("frequencies"):
            t = torch.from_numpy(np.ascontiguousarray(a)).double()
            assert a.dtype == np.float32 and torch.equal(t, t.to(torch.bfloat16).double()) and torch.equal(t, t.to(torch.float16).double()), k


def cut(prob, mask, offset):
    out, a = [], 0
    for e in offset.tolist():
        s = np.sort(prob[a:e])[::-1]
        k = int(mask[a:e].sum())
        assert 0 < k < e - a and np.array_equal(np.sort(prob[a:e][mask[a:e]])[::-1], s[:k])
        out.append((k, float(s[k - 1] - s[k]), np.cumsum(s)))
        a = e
    return out


@pytest.mark.parametrize("name", P.MASK + P.MASK_RES + P.CHAINS)
def test_recorded_margins_follow_from_the_recorded_scores(name):
    rec = P.load(name)
    a, marg = rec["arrays"], rec["meta"]["margins"]
    chain = name in P.CHAINS
    mask = a["s0/non_leaf"] if chain else a["out/non_leaf"]
    offset = a["s0/mask_in/offset"] if chain else a["in/offset"]
    cuts = cut(a["aux/prob"], mask, offset)
    assert [c[0] for c in cuts] == marg["k"] and np.allclose([c[1] for c in cuts], marg["gap"], rtol=0, atol=1e-15)
    worst = max(marg["score_diff"].values())
    assert min(c[1] for c in cuts) >= marg["safety"] * worst > 0
    assert len(set(marg["k"])) > 1                                # the two segments keep different numbers of rows
    if name.endswith("topp"):
        assert min(marg["k"]) >= 3                                # several ranks go into every prefix sum that decides
        ratio = rec["meta"]["ctor"]["non_leaf_ratio"]
        hi = float(torch.tensor(ratio).bfloat16())
        prefix = [min(ratio - c[2][c[0] - 1], c[2][c[0]] - hi) for c in cuts]
        assert np.allclose(prefix, marg["prefix_margin"], rtol=0, atol=1e-15) and min(prefix) >= marg["safety"] * max(marg["prefix_diff"].values()) > 0
        srt = np.concatenate([np.sort(s)[::-1] for s in np.split(a["aux/prob"], offset[:-1])])
        assert np.array_equal(srt, a["aux/sorted"])
        assert np.array_equal(np.concatenate([c[2] for c in cuts]), a["aux/prefix"])
    if chain:
        grid = rec["meta"]["grid_size"]
        for coord, g, border in zip((a["s0/in/coord"], a["s1/in/coord"]), (grid, grid / rec["meta"]["chain"]["stride"]), marg["cell_border"]):
            u = (coord - coord.min(0)) / g
            d = np.minimum(u - np.floor(u), np.ceil(u) - u)[u != 0].min()
            assert np.isclose(d, border, rtol=0, atol=1e-12) and d >= marg["safety"] * marg["cell_error_f32"] > 0
        for key in ("s0/in/", "s1/serial/"):
            cells = np.concatenate([a[key + "batch"][:, None], a[key + "grid_coord"]], 1)
            assert len(np.unique(cells, axis=0)) == len(cells)
        assert marg["tanh_preact_max"] < 3.0 and marg["min_row_variance"] > 1e-2


# ---- UpscaleModule, UpscaleResModule --------------------------------------------------------------------------------------

def cpu_gather(src, indptr):
    counts = (indptr[1:] - indptr[:-1])
    return src.repeat_interleave(counts, 0)


def run_upscale(rec, forward):
    m = P.stand_in(rec)
    leaves = tuple(P.part(rec, "gin/"))
    p = P.input_point(rec, grad=leaves)
    leaf = {k: p[k] for k in leaves}
    out = forward(m, p)
    outs = {k: out[k] for k in P.part(rec, "up/")}
    sum((v * P.tensor(rec["arrays"]["up/" + k])).sum() for k, v in outs.items()).backward()
    got = {"out/" + k: v for k, v in outs.items()}
    got["out/offset"] = out.offset
    got.update(grads(leaf, {"": m}))
    return got, out


@pytest.mark.parametrize("name", P.UPSCALE)
def test_upscale_stand_in_reproduces_the_reference(name, monkeypatch):
    from generativedensification_amd import upscale as U

    rec = P.load(name)
    res = rec["meta"]["class"] == "UpscaleResModule"
    assert set(P.part(rec, "gin/")) == {"coord", "feat"} | ({"global_feat"} if rec["meta"]["norm"] == "ada" else set()) | ({"attribute"} if res else set())
    monkeypatch.setitem(sys.modules, "torch_scatter", types.SimpleNamespace(gather_csr=cpu_gather))
    forwards = {"reference_forward": lambda m, p: UR.reference_forward(m, p, res=res),
                "_reference_tail": lambda m, p: U._reference_tail(m, m.in_norm(p), res)}
    for tag, forward in forwards.items():
        got, out = run_upscale(rec, forward)
        assert sorted(k for k in out.keys()) == sorted(k for k in rec["meta"]["keys"] if k != "batch")
        settle(f"{name}/{tag}", *compare(got, rec, ("out/", "gin/", "gparam/")))


@pytest.mark.parametrize("mut", UR.MUTANTS)
@pytest.mark.parametrize("name", P.UPSCALE)
def test_a_misread_upscale_line_lands_far_from_the_record(name, mut):
    rec = P.load(name)
    res = rec["meta"]["class"] == "UpscaleResModule"
    got, _ = run_upscale(rec, lambda m, p: UR.reference_forward(m, p, res=res, mut=mut))
    far(f"{name}/{mut}", *compare(got, rec, ("out/", "gin/", "gparam/")), on=("out/feat",))


# ---- MaskModule, MaskResModule --------------------------------------------------------------------------------------------

def run_mask(rec, mut=None):
    m = P.stand_in(rec)
    p = P.input_point(rec, grad=("feat",))
    feat = p.feat
    out, non_leaf = P.restated_mask_forward(m, p, mut)
    leaf = out.leaf_point
    got = {"out/coord": out.coord, "out/feat": out.feat, "out/offset": out.offset, "out/leaf_coord": leaf.coord, "out/leaf_feat": leaf.feat,
           "out/leaf_offset": leaf.offset, "out/non_leaf": non_leaf}
    a = rec["arrays"]
    if out.feat.shape == a["up/feat"].shape:
        ((out.feat * P.tensor(a["up/feat"])).sum() + (leaf.feat * P.tensor(a["up/leaf_feat"])).sum()).backward()
    got.update(grads({"feat": feat}, {"": m}))
    return got, out, p


@pytest.mark.parametrize("name", P.MASK)
def test_mask_module_restated_reproduces_the_reference(name):
    from generativedensification_amd import densify as D

    rec = P.load(name)
    got, out, p = run_mask(rec)
    assert [k for k in rec["meta"]["keys"] if k != "batch"] == list(out) == list(D.POINT_KEYS)
    assert [k for k in rec["meta"]["leaf_keys"] if k != "batch"] == list(out.leaf_point) == list(D.LEAF_POINT_KEYS)
    assert out.global_feat is p.global_feat and out.grid_size == out.leaf_point.grid_size == rec["meta"]["grid_size"]
    settle(name, *compare(got, rec, ("out/", "gin/", "gparam/")))


@pytest.mark.parametrize("name,mut", [(n, m) for n in P.MASK for m in P.MASK_MUTANTS if not (m == "floor_for_ceil" and n.endswith("topp"))])
def test_a_misread_mask_line_lands_far_from_the_record(name, mut):
    rec = P.load(name)
    got, _, _ = run_mask(rec, mut)
    on = {"gate_value_masked": ("out/leaf_feat",), "leaf_ungated": ("gin/feat", "gparam/net.0.weight"), "floor_for_ceil": ("out/non_leaf", "out/offset")}[mut]
    far(f"{name}/{mut}", *compare(got, rec, ("out/", "gin/", "gparam/")), on=on)


@pytest.mark.parametrize("name", P.MASK_RES)
def test_mask_res_module_restated_reproduces_the_reference(name):
    from generativedensification_amd import densify as D

    rec = P.load(name)
    m = P.stand_in(rec)
    p = P.input_point(rec, grad=("feat",))
    feat = p.feat
    out = P.restated_mask_res_forward(m, p)
    assert out is p and [k for k in rec["meta"]["keys"] if k != "batch"][-6:] == list(D.MASK_RES_KEYS)
    (out.feat * P.tensor(rec["arrays"]["up/feat"])).sum().backward()
    got = {"out/" + k: out[k] for k in D.MASK_RES_KEYS + ("feat",)}
    got.update(grads({"feat": feat}, {"": m}))
    settle(name, *compare(got, rec, ("out/", "gin/", "gparam/")))
    # the gate's value is feat * non_leaf here, and plain feat in MaskModule: the two classes differ in exactly this
    assert torch.equal(out.feat.detach(), feat.detach() * out.non_leaf[:, None])


def test_mask_module_at_ratio_one_passes_the_point_through():
    from generativedensification_amd import densify as D

    rec = P.load("mask_full")
    m = P.stand_in(rec)
    assert not list(m.parameters()) and not rec["state"]
    p = P.input_point(rec)
    out, non_leaf = P.restated_mask_forward(m, p)
    assert non_leaf is None
    assert [k for k in rec["meta"]["keys"] if k != "batch"] == list(out) == list(D.POINT_KEYS)
    assert [k for k in rec["meta"]["leaf_keys"] if k != "batch"] == list(out.leaf_point) == list(D.LEAF_POINT_KEYS)
    for who, pt in (("point", out), ("leaf_point", out.leaf_point)):
        for k in ("coord", "feat", "offset"):
            assert rec["meta"]["identities"][f"{who}.{k}"] and pt[k] is p[k]
    assert rec["meta"]["identities"]["point.global_feat"] and out.global_feat is p.global_feat


# ---- GaussianModule, GaussianResModule ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", P.HEAD)
def test_head_stand_in_reproduces_the_reference(name):
    rec = P.load(name)
    m = P.stand_in(rec)
    leaves = tuple(P.part(rec, "gin/"))
    if name == "head_res":
        p = P.input_point(rec, grad=leaves)
        leaf = {k: p[k] for k in leaves}
        attribute = FR.reference_res_module_forward(m, p).attribute
    else:
        inner = P.input_point(rec, grad=leaves, keys=("coord", "feat", "offset"))
        leaf = {"feat": inner.feat}
        out = FR.reference_module_forward(m, P.Point(leaf_point=inner))
        assert out.leaf_point is inner
        attribute = inner.attribute
    (attribute * P.tensor(rec["arrays"]["up/attribute"])).sum().backward()
    got = {"out/attribute": attribute, **grads(leaf, {"": m})}
    settle(name, *compare(got, rec, ("out/", "gin/", "gparam/")))


# ---- the chain ------------------------------------------------------------------------------------------------------------

def run_chain(rec, mut=None):
    stages = P.stand_in(rec)
    point = P.chain_input(rec, grad=True)
    leaves = {"coord": point.coord, "feat": point.feat}
    arrays, leaf_points = P.run_chain(rec, stages, point, P.cpu_forwards(mut if mut in P.CHAIN_MUTANTS[:2] else None))
    with NR.float_is_identity_on_float64():
        finals = P.assemble(rec, leaf_points, mut=mut if mut in FR.ASSEMBLE_MUTANTS else None)
    if all(finals[k].shape == rec["arrays"]["up/" + k].shape for k in finals):
        sum((v * P.tensor(rec["arrays"]["up/" + k])).sum() for k, v in finals.items()).backward()
    got = dict(arrays)
    got.update({"out/" + k: v for k, v in finals.items()})
    got.update(grads(leaves, {f"s{s}.{name}.": m for s, mods in enumerate(stages) for name, m in mods.items()}))
    return got


@pytest.mark.parametrize("name", P.CHAINS)
def test_chain_restated_reproduces_the_reference(name):
    rec = P.load(name)
    assert ("global" in rec["meta"]["stage_modules"][0]) == (name == "chain_ada") and rec["meta"]["norm"] == name[len("chain_"):]
    got = run_chain(rec)
    errs, unequal = compare(got, rec, ("s0/", "s1/", "out/", "gin/", "gparam/"))
    integers = [k for k, v in rec["arrays"].items() if k.startswith(("s0/", "s1/")) and v.dtype.kind in "iub" and not k.endswith("/batch")]
    assert {"s0/in/grid_coord", "s0/in/serialized_code", "s0/in/serialized_order", "s0/in/serialized_inverse", "s0/in/sparse_shape",
            "s0/non_leaf", "s0/out/offset", "s0/out/leaf/offset", "s1/serial/grid_coord", "s1/serial/serialized_code",
            "s1/serial/serialized_order", "s1/serial/serialized_inverse", "s1/serial/sparse_shape", "s1/out/offset"} <= set(integers)
    assert len([k for k in rec["arrays"] if k.startswith("gparam/")]) == len(rec["state"]) - 2          # (the two `frequencies` buffers)
    settle(name, errs, unequal)


@pytest.mark.parametrize("mut", P.CHAIN_MUTANTS)
@pytest.mark.parametrize("name", P.CHAINS)
def test_a_misread_chain_line_lands_far_from_the_record(name, mut):
    rec = P.load(name)
    got = run_chain(rec, mut)
    on = {"grid_size_not_divided": ("s1/serial/grid_coord",), "per_segment_minimum": ("s0/in/grid_coord", "s1/serial/grid_coord"),
          "levels_not_sorted_by_batch": ("out/centers", "out/shs"), "shifts_swapped": ("out/opacity", "out/scaling")}[mut]
    far(f"{name}/{mut}", *compare(got, rec, ("s0/", "s1/", "out/", "gin/", "gparam/")), on=on)
