"""CPU: the float64 restatement of the Block junction (tests/block_ref.py) against autograd of the torch composition in
float64; the restated Block.forward against the reference's lines as block.py states them, on the stand-in; the argument
checks of `junction` that raise before the library loads; `covers` on stand-ins of both norm kinds and on each way to fall
outside; the surface generativedensification_amd/block.py reads against what the reference's Block declares
(tests/golden/block_surface.json); the entry points in _lib.py and include/gdr.h."""
import ast
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import block_cases as BC
import block_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ENTRY_POINTS = ("gdr_block_junction_forward", "gdr_block_junction_backward_bytes", "gdr_block_junction_backward")


def block():
    from generativedensification_amd import block as B

    return B


def t64(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))


def spec64(spec, leaves):
    """the numpy spec as float64 torch leaves (appended to `leaves` as (name, tensor))"""
    if spec is None:
        return None
    parts = []
    for i, p in enumerate(spec[1:-1]):
        p = None if p is None else t64(p).requires_grad_(True)
        parts.append(p)
        leaves.append(p)
    return (spec[0], *parts, spec[-1])


@pytest.mark.parametrize("name", list(BC.CASES))
def test_restatement_matches_autograd_of_the_torch_composition(name):
    skip, branch, keep, pre, post, offset, gy, gn = BC.inputs(name)
    y, n = R.junction(skip, branch, keep, pre, post, offset)
    want = R.junction_grad(skip, branch, keep, pre, post, offset, gy, gn)
    a, b = t64(skip).requires_grad_(True), t64(branch).requires_grad_(True)
    pre_leaves, post_leaves = [], []
    t_pre, t_post = spec64(pre, pre_leaves), spec64(post, post_leaves)
    ty, tn = R.torch_junction(a, b, t64(keep), t_pre, t_post, torch.from_numpy(offset))
    assert np.abs(ty.detach().numpy() - y).max() < 1e-12 and (n is None) == (tn is None)
    outs, gs = [ty], [t64(gy)]
    if n is not None:
        assert np.abs(tn.detach().numpy() - n).max() < 1e-12
        outs.append(tn)
        gs.append(t64(gn))
    torch.autograd.backward(outs, gs)
    pre_leaves += [None] * (2 - len(pre_leaves))
    post_leaves += [None] * (2 - len(post_leaves))
    pairs = [(a, want["skip"]), (b, want["branch"]), (pre_leaves[0], want["pre_w"]), (pre_leaves[1], want["pre_b"]),
             (post_leaves[0], want["post_w"]), (post_leaves[1], want["post_b"])]
    for leaf, w in pairs:
        assert (leaf is None) == (w is None)
        if leaf is not None:
            assert np.abs(leaf.grad.numpy() - w).max() <= 1e-11 * max(1.0, np.abs(w).max())
    # rows behind the last end: zero through an ada norm, and y defined everywhere
    seg = np.searchsorted(offset, np.arange(skip.shape[0]), side="right")
    behind = seg >= len(offset)
    if post is not None and post[0] == "ada" and behind.any():
        assert not n[behind].any()
    if pre is not None and pre[0] == "ada" and behind.any():
        assert np.array_equal(y[behind], np.asarray(skip)[behind]) and not want["branch"][behind].any()


point_of = R.point_of


@pytest.mark.parametrize("norm", ["ln", "affine", "ada"])
def test_restated_forward_is_the_reference_lines_on_the_stand_in(norm):
    """the torch path of the bound forward (the reference's lines through the containers' dispatch) and the restatement from the
    arithmetic agree in float64, output and input gradient, at the third norm kind too (LN with affine, which no record holds).
    What the reference's own Block computes, and the mutants, are judged in tests/test_block_record_cpu.py."""
    B = block()
    m = R.make_block(16, 2, 8, norm=norm).double()
    data = BC.block_point((20, 13), 16)
    assert B.BLOCK_BACKEND in ("torch", "hip")
    p1 = point_of(data, grad=True)
    leaf1 = p1.feat
    got = B._reference_forward(m, p1)            # (CPU tensors: the hip path does not serve them either way)
    p2 = point_of(data, grad=True)
    leaf2 = p2.feat
    want = R.restated_forward(m, p2)
    assert got.feat is got.sparse_conv_feat.features and want.feat is want.sparse_conv_feat.features
    assert np.abs((got.feat - want.feat).detach().numpy()).max() < 1e-12
    g = torch.from_numpy(np.random.default_rng(0).standard_normal(tuple(want.feat.shape)))
    got.feat.backward(g)
    want.feat.backward(g)
    assert np.abs((leaf1.grad - leaf2.grad).numpy()).max() < 1e-11
    # the bound forward runs the same lines for CPU tensors under either backend
    again = B.block_forward(m, point_of(data))
    assert torch.equal(again.feat, got.feat)


def test_covers_holds_for_both_norm_kinds_and_fails_on_each_way_out():
    B = block()
    for norm in ("ln", "affine", "ada"):
        assert B.covers(R.make_block(16, 2, 8, norm=norm, conv="hip")), norm
    assert B.covers(R.make_block(16, 2, 8, conv="hip", drop_path=0.3))
    assert not B.covers(R.make_block(16, 2, 8, conv="hip", pre_norm=False))
    assert not B.covers(R.make_block(16, 2, 8, conv="hip", proj_drop=0.1))
    assert not B.covers(R.make_block(16, 2, 8, conv="hip", segment_norm=True))
    assert not B.covers(R.make_block(16, 2, 8, conv="table"))            # cpe[0] is not the SubMConv3d
    for child in ("norm1", "mlp", "attn", "drop_path", "cpe"):
        m = R.make_block(16, 2, 8, conv="hip")
        delattr(m, child)
        assert not B.covers(m), child
    m = R.make_block(16, 2, 8, conv="hip")
    del m.mlp[0].fc2
    assert not B.covers(m)
    m = R.make_block(16, 2, 8, conv="hip")
    m.mlp[0].act = torch.nn.ReLU()
    assert not B.covers(m)
    m = R.make_block(16, 2, 8, norm="ada", conv="hip")
    del m.norm2[0].affine                                                  # an nn.LayerNorm subclass that is neither kind
    assert not B.covers(m)
    assert B.in_envelope(19200, 256, 1) and B.in_envelope(0, 8, 1024) and B.in_envelope(12000, 160)
    for bad in ((10, 12, 1), (10, 1032, 1), (10, 0, 1), (10, 8, 0), (10, 8, 1025), (1 << 31, 8, 1), (-1, 8, 1)):
        assert not B.in_envelope(*bad), bad


def test_argument_checks_raise_before_the_library_loads(monkeypatch):
    B = block()
    from generativedensification_amd import _lib as L

    def no_load():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(L, "load", no_load)
    skip, branch = torch.zeros(4, 16), torch.zeros(4, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        B.junction(skip, branch)
    with pytest.raises(TypeError):
        B.junction(skip.double(), branch)
    with pytest.raises(TypeError):
        B.junction(skip, branch, keep=[1.0] * 4)
    with pytest.raises(TypeError):
        B.junction(skip, branch, keep=torch.zeros(4, dtype=torch.float64))
    with pytest.raises(TypeError):
        B.junction(skip, branch, pre=("rms", None, 1e-5))
    with pytest.raises(TypeError):
        B.junction(skip, branch, post=("ln", None, 1e-5))                  # ('ln', weight, bias, eps)
    with pytest.raises(TypeError):
        B.junction(skip, branch, post=("ada", torch.zeros(1, 16), 1e-5))   # no offset
    with pytest.raises(TypeError):
        B.junction(skip, branch, post=("ada", torch.zeros(1, 16), 1e-5), offset=torch.tensor([4.0]))
    for bad in (dict(branch=torch.zeros(5, 16)), dict(keep=torch.zeros(5)), dict(post=("ln", torch.zeros(8), None, 1e-5)),
                dict(pre=("ada", torch.zeros(2, 16), 1e-5), offset=torch.tensor([4])), dict(post=("ada", torch.zeros(1, 8), 1e-5),
                                                                                            offset=torch.tensor([4]))):
        args = dict(skip=skip, branch=branch)
        args.update(bad)
        with pytest.raises(ValueError):
            B.junction(**args)
    with pytest.raises(ValueError):
        B.junction(torch.zeros(4, 12), torch.zeros(4, 12))
    with pytest.raises(ValueError):
        B.junction(torch.zeros(4, 1032), torch.zeros(4, 1032))
    with pytest.raises(ValueError):
        B.junction(torch.zeros(4, 16, 1), branch)
    m = R.make_block(16, 2, 8)
    B_old = B.BLOCK_BACKEND
    try:
        B.BLOCK_BACKEND = "cuda"
        with pytest.raises(ValueError):
            B.block_forward(m, point_of(BC.block_point((9,), 16)))
    finally:
        B.BLOCK_BACKEND = B_old


def self_and_point_accesses():
    """the attributes of `self` / `module` and of `point` that block.py reads or assigns"""
    tree = ast.parse(open(os.path.join(ROOT, "generativedensification_amd", "block.py")).read())
    reads, writes = {"self": set(), "point": set()}, {"self": set(), "point": set()}
    for n in ast.walk(tree):
        if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name):
            owner = {"self": "self", "module": "self", "point": "point"}.get(n.value.id)
            if owner:
                (reads if isinstance(n.ctx, ast.Load) else writes)[owner].add(n.attr)
        if (isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id == "getattr" and isinstance(n.args[0], ast.Name)
                and n.args[0].id in ("self", "module", "point") and isinstance(n.args[1], ast.Constant)):
            reads["self" if n.args[0].id != "point" else "point"].add(n.args[1].value)
    return reads, writes


def test_surface_matches_the_reference():
    surface = json.load(open(os.path.join(HERE, "golden", "block_surface.json")))
    blk, mlp, dp = surface["Block"], surface["MLP"], surface["DropPath"]
    B = block()
    assert list(inspect.signature(B.block_forward).parameters) == blk["forward"] == ["self", "point"]
    reads, writes = self_and_point_accesses()
    # from the module: what the reference's forward reads, and `channels` (the width, assigned by its __init__)
    assert reads["self"] == set(blk["reads"]) | {"channels"} and not writes["self"]
    assert set(blk["reads"]) | {"channels"} <= set(blk["assigned"])
    # from the point: the reference's, and offset / global_feat, which the reference reads inside its norms
    assert reads["point"] - {"get"} == set(blk["point_reads"]) | {"offset", "global_feat"} and writes["point"] == set(blk["point_writes"])
    assert blk["defaults"]["pre_norm"] == "True" and blk["defaults"]["drop_path"] == "0.0" and blk["defaults"]["mlp_ratio"] == "4.0"
    assert blk["defaults"]["norm_layer"] == "nn.LayerNorm" and blk["defaults"]["act_layer"] == "nn.GELU"
    assert mlp["assigned"] == ["fc1", "act", "fc2", "drop"] and mlp["defaults"]["act_layer"] == "nn.GELU" and mlp["defaults"]["drop"] == "0.0"
    assert dp["init"][1:] == ["drop_prob", "scale_by_keep"] and set(dp["reads"]) == {"drop_prob", "scale_by_keep", "training"}
    # the stand-in of the tests has every attribute the reference assigns, under the reference's child names
    m = R.make_block(16, 2, 8, norm="ada", drop_path=0.2)
    assert all(hasattr(m, name) for name in blk["assigned"]) and all(hasattr(m.mlp[0], name) for name in mlp["assigned"])
    assert all(hasattr(m.drop_path[0], name) for name in dp["reads"])
    keys = set(m.state_dict())
    assert {"cpe.0.weight", "cpe.0.bias", "cpe.1.weight", "cpe.2.affine.weight", "norm1.0.affine.bias", "attn.qkv.weight",
            "attn.proj.bias", "norm2.0.affine.weight", "mlp.0.fc1.weight", "mlp.0.fc2.bias"} <= keys and len(keys) == 18


def test_entry_points_are_declared():
    from generativedensification_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "gdr.h")).read()
    for name in ENTRY_POINTS:
        assert name in L.EXPORTED_SYMBOLS, name
        m = re.search(r"^(?:int|size_t) " + name + r"\(([^;]*)\);", header, re.M)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(L._PROTOS[name][1]), name
    assert re.search(r"#define GDR_ABI_VERSION\s+17\b", header)
    # the struct of a norm: the same fields in the same order on both sides
    body = re.search(r"typedef struct GdrBlockNorm \{(.*?)\} GdrBlockNorm;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip().lstrip("*") for decl in body.split(";") if decl.strip() for f in decl.strip().split(" ", 1 + decl.strip().startswith("const"))[-1].split(",")]
    assert fields == [f[0] for f in L.GdrBlockNorm._fields_], fields
    codes = dict(re.findall(r"#define (GDR_BLOCK_NORM_\w+) (\d+)", header))
    assert {k: int(v) for k, v in codes.items()} == {k: getattr(L, k) for k in ("GDR_BLOCK_NORM_NONE", "GDR_BLOCK_NORM_LN",
                                                                                 "GDR_BLOCK_NORM_LN_AFFINE", "GDR_BLOCK_NORM_ADA")}
