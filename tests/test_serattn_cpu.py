"""CPU: the float64 restatement of the gather form of the attention (tests/serattn_ref.py) against central differences and
against autograd of the same composition, on a case whose padding holds points twice; the surface
generativedensification_amd/serattn.py reads against what the reference's SerializedAttention declares
(tests/golden/serattn_surface.json); the entry points in _lib.py and include/gdr.h; `covers`, `in_envelope` and the refusals
that need no GPU."""
import ast
import ctypes
import inspect
import itertools
import json
import os
import re

import pytest
import torch

import attn_cases as AC
import attn_ref as R
import serattn_cases as SC
import serattn_ref as SR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ENTRY_POINTS = ("gdr_attn_gather_forward", "gdr_attn_gather_backward")


def serattn():
    from generativedensification_amd import serattn as S

    return S


def tiny():
    """patch 4, segments of 5 (3 copies) and 3 (one short sequence); H = 2, D = 3"""
    patch, offsets, H, D = 4, (5, 8), 2, 3
    order, inverse, cu, _ = SC.tables(offsets, patch, 7)
    assert order.numel() == 11 and cu.tolist() == [0, 4, 8, 11] and sorted(torch.bincount(order).tolist()) == [1] * 5 + [2] * 3
    g = torch.Generator().manual_seed(8)
    qkv = torch.randn(8, 3 * H * D, generator=g, dtype=torch.float64)
    dout = torch.randn(8, H * D, generator=g, dtype=torch.float64)
    return qkv, dout, order, inverse, cu.tolist(), H


def test_restatement_against_central_differences():
    qkv, dout, order, inverse, cu, H = tiny()
    got = SR.backward(qkv, order, inverse, cu, H, dout, 0.7)
    want = torch.zeros_like(qkv)
    flat, h = qkv.reshape(-1), 1e-6
    for i in range(flat.numel()):
        keep = float(flat[i])
        flat[i] = keep + h
        hi = float((SR.forward(qkv, order, inverse, cu, H, 0.7) * dout).sum())
        flat[i] = keep - h
        lo = float((SR.forward(qkv, order, inverse, cu, H, 0.7) * dout).sum())
        flat[i] = keep
        want.reshape(-1)[i] = (hi - lo) / (2 * h)
    assert float((got - want).abs().max()) < 1e-7 and float(want.abs().max()) > 0.1


def test_restatement_equals_autograd_of_the_same_composition():
    qkv, dout, order, inverse, cu, H = tiny()
    leaf = qkv.clone().requires_grad_(True)
    out = SR.forward(leaf, order, inverse, cu, H)
    out.backward(dout)
    assert float((out.detach() - SR.forward(qkv, order, inverse, cu, H)).abs().max()) == 0
    assert float((leaf.grad - SR.backward(qkv, order, inverse, cu, H, dout)).abs().max()) < 1e-13
    # a point the padding holds twice receives more than its own slot's gradient
    Tp, C = order.numel(), qkv.shape[1] // 3
    dslots = torch.zeros(Tp, C, dtype=qkv.dtype)
    dslots[inverse] = dout
    import attn_ref as R

    own_only = R.attention_backward(qkv[order].reshape(Tp, 3, H, C // H), cu, dslots.reshape(Tp, H, C // H)).reshape(Tp, 3 * C)[inverse]
    twice = torch.bincount(order, minlength=qkv.shape[0]) > 1
    diff = (leaf.grad - own_only).abs().amax(dim=1)
    assert bool((diff[twice] > 1e-4).all()) and float(diff[~twice].max()) < 1e-13
    assert float((leaf.grad - own_only)[:, :C].abs().max()) < 1e-13          # dQ of a copy is zero


def test_the_cases_are_what_their_names_say():
    for name, (patch, offsets, H, D, _) in SC.SHAPES.items():
        case = SC.make(name, "f16")
        assert case["N"] <= 1500 and case["order"].numel() - case["N"] == SC.COPIES[name] == int(case["has_copy"].sum())
        assert case["cu"][-1] == case["order"].numel() and max(b - a for a, b in zip(case["cu"][:-1], case["cu"][1:])) <= patch
        # every copy sits one sequence behind its point's own slot, at the same position
        slots = torch.arange(case["order"].numel())
        copy = case["inverse"][case["order"]] != slots
        assert bool((case["order"][slots[copy] - patch] == case["order"][copy]).all())
        assert bool((case["inverse"][case["order"]][copy] == slots[copy] - patch).all())
    assert len(SC.CASES) == 39
    # the tile cases, segment by segment: patch + 1 points, two patches, a short one, an empty one, two patches and a point
    for name in SC.TILES:
        patch, offsets, H, *_ = SC.SHAPES[name]
        assert [b - a for a, b in zip((0,) + offsets, offsets)] == [patch + 1, 2 * patch, 30, 0, 2 * patch + 1]
        assert SC.COPIES[name] == 2 * (patch - 1) and H % 2 and offsets[-1] <= 1312
        cu = SC.make(name, "f16")["cu"]
        assert [b - a for a, b in zip(cu[:-1], cu[1:])] == [patch] * 4 + [30] + [patch] * 3


def test_the_case_table_reaches_every_head_dim_and_row_tile():
    """a (D, RP) is a kernel of its own in the gather form, forward and backward: the cases select all twelve"""
    reached = {(D, AC.row_tile(patch)) for patch, _, _, D, _ in SC.SHAPES.values()}
    assert reached == set(itertools.product((8, 16, 32, 64), (64, 128, 256)))
    # a patch that fills the tile under every tile, and the smallest patch of the two upper tiles
    assert {64, 128, 256, 65, 129} <= {SC.SHAPES[name][0] for name in SC.TILES}


def _kernel_model(case, dt):
    """what a correct kernel of the gather form gives (attn_ref.kernel_model over the gathered rows): every element rounded to
    fp16, f32 arithmetic, the result rounded to fp16 and then to qkv's dtype; delta from the fp16 result for f16 qkv and from
    the f32 one for f32 and bf16 qkv; the two contributions of a point held twice summed in f32, then rounded to fp16 and to
    qkv's dtype.  -> out (N, C), dqkv (N, 3 C) in qkv's dtype"""
    dtype, H, C, Tp = SC.DTYPES[dt], case["H"], case["C"], case["order"].numel()
    packed = case["qkv"][case["order"]].half().reshape(Tp, 3, H, C // H)
    dslots = torch.zeros(Tp, C, dtype=torch.float16)
    dslots[case["inverse"]] = case["dout"].half()
    out, dpacked = R.kernel_model(packed, case["cu"], dslots.reshape(Tp, H, C // H), case["scale"],
                                  delta_from_rounded=dtype == torch.float16)
    dqkv = torch.zeros(case["N"], 3 * C).index_add_(0, case["order"], dpacked.reshape(Tp, 3 * C))
    return out.reshape(Tp, C).to(dtype)[case["inverse"]], dqkv.half().to(dtype)


@pytest.mark.parametrize("name", SC.TILES)
def test_a_correct_kernel_leaves_room_under_the_bar_on_every_tile_case(name):
    """A condition on the INPUTS, not a tolerance on the kernel (tests/test_attn_cpu.py has the packed form's): the model must
    stay within 0.8 of the bar of test_gpu_serattn.py, built here from the all-torch composition run on the CPU, in out, dQ, dK
    and dV and in all three dtypes."""
    worst = 0.0
    for dt, dtype in SC.DTYPES.items():
        c = SC.make(name, dt)
        q64, d64, C = c["qkv"].half().double(), c["dout"].half().double(), c["C"]
        t_out = SR.forward(q64, c["order"], c["inverse"], c["cu"], c["H"], c["scale"])
        t_dqkv = SR.backward(q64, c["order"], c["inverse"], c["cu"], c["H"], d64, c["scale"])
        pt_out, pt_dqkv = SR.torch_composition(c["qkv"], c["order"], c["inverse"], c["cu"], c["H"], c["scale"], c["dout"])
        out, dqkv = _kernel_model(c, dt)
        assert out.dtype == dtype and dqkv.dtype == dtype
        triples = [("out", out, t_out, pt_out)]
        triples += [(w, dqkv[:, i * C:(i + 1) * C], t_dqkv[:, i * C:(i + 1) * C], pt_dqkv[:, i * C:(i + 1) * C])
                    for i, w in enumerate(("dq", "dk", "dv"))]
        shares = {w: float((got.double() - t).abs().max()) / AC.bar(float((pt.double() - t).abs().max()), dtype, t)
                  for w, got, t, pt in triples}
        print(f"{name} {dt}: share of the bar " + " ".join(f"{w} {s:.2f}" for w, s in shares.items()))
        worst = max(worst, *shares.values())
    assert worst <= 0.8, (name, worst)


def self_and_point_reads():
    """the attributes of `self` / `module` and of `point` that serattn.py reads or assigns, and the string keys it uses"""
    tree = ast.parse(open(os.path.join(ROOT, "generativedensification_amd", "serattn.py")).read())
    reads = {"self": set(), "point": set()}
    writes = {"self": set(), "point": set()}
    for n in ast.walk(tree):
        if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name):
            owner = {"self": "self", "module": "self", "point": "point"}.get(n.value.id)
            if owner and isinstance(n.ctx, ast.Load):
                reads[owner].add(n.attr)
            if owner and isinstance(n.ctx, ast.Store):
                writes[owner].add(n.attr)
        if (isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id == "getattr" and isinstance(n.args[0], ast.Name)
                and n.args[0].id in ("self", "module") and isinstance(n.args[1], ast.Constant)):
            reads["self"].add(n.args[1].value)
    strings = {n.value for n in ast.walk(tree) if isinstance(n, ast.Constant) and isinstance(n.value, str)}
    return reads, writes, strings


def test_surface_matches_the_reference():
    surface = json.load(open(os.path.join(HERE, "golden", "serattn_surface.json")))["SerializedAttention"]
    S = serattn()
    assert list(inspect.signature(S.serialized_attention_forward).parameters) == surface["forward"]
    reads, writes, strings = self_and_point_reads()
    # the bound forward stands for forward and the two methods it calls: it reads what they read, and calls neither
    assert surface["methods"] == ["get_padding_and_inverse", "get_rel_pos"]
    assert reads["self"] == set(surface["reads"]) and writes["self"] == set(surface["writes"])
    assert set(surface["reads"]) - {"training"} <= set(surface["assigned"])
    assert reads["point"] == set(surface["point_reads"]) and writes["point"] == set(surface["point_writes"])
    assert all(k in strings for k in surface["point_keys"])
    # the stand-in module of the tests has every attribute the reference assigns
    m = SR.Module(16, 2, 4)
    assert all(hasattr(m, name) for name in surface["assigned"])
    assert list(inspect.signature(S.serialized_attention).parameters) == ["qkv", "order", "inverse", "cu_seqlens", "num_heads",
                                                                         "patch_size", "softmax_scale"]


def test_entry_points_are_declared():
    from generativedensification_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "gdr.h")).read()
    for name in ENTRY_POINTS:
        assert name in L.EXPORTED_SYMBOLS, name
        m = re.search(r"^int " + name + r"\(([^;]*)\);", header, re.M)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(L._PROTOS[name][1]), name
    assert re.search(r"#define GDR_ABI_VERSION\s+17\b", header)
    # the args struct: ten 4-byte fields, as the header declares them
    body = re.search(r"typedef struct gdr_attn_gather_args \{(.*?)\} gdr_attn_gather_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.strip().split(" ", 1)[1].split(",")]
    assert names == [f[0] for f in L.GdrAttnGatherArgs._fields_] and ctypes.sizeof(L.GdrAttnGatherArgs) == 40
    # GDR_ATTN_F32 is the header's GDR_F32, and that is 2
    assert (L.GDR_ATTN_F16, L.GDR_ATTN_BF16, L.GDR_ATTN_F32) == (0, 1, 2)
    assert re.search(r"#define GDR_ATTN_F32\s+GDR_F32\b", header) and re.search(r"#define GDR_F32\s+2\b", header)


def test_covers_and_in_envelope():
    S = serattn()
    assert S.covers(SR.Module(160, 20, 48))
    assert not S.covers(SR.Module(160, 20, 48, enable_flash=False))
    assert not S.covers(SR.Module(160, 20, 48, enable_rpe=True))
    m = SR.Module(160, 20, 48, attn_drop=0.1)
    assert m.training and not S.covers(m)
    m.eval()
    assert S.covers(m)
    assert not S.covers(object())
    assert S.in_envelope(12000, 160, 20, 48) and S.in_envelope(19200, 256, 32, 48, 19248) and S.in_envelope(0, 8, 1, 256)
    assert S.in_envelope(5, 128, 2, 1) and S.in_envelope((1 << 31) - 1, 8, 1, 48)
    for bad in ((10, 160, 20, 257), (10, 160, 20, 0), (10, 160, 16, 48), (10, 24, 2, 48), (10, 256, 2, 48), (10, 160, 0, 48),
                (1 << 31, 8, 1, 48), (10, 8, 1, 48, 1 << 31), (10, 8, 1, 48, 9), (-1, 8, 1, 48)):
        assert not S.in_envelope(*bad), bad


def test_refusals_that_need_no_gpu():
    S = serattn()
    qkv, order, inverse, cu = torch.zeros(6, 48), torch.arange(6), torch.arange(6), torch.tensor([0, 6], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.serialized_attention(qkv, order, inverse, cu, 2, 48)
    with pytest.raises(TypeError):
        S.serialized_attention(qkv.double(), order, inverse, cu, 2, 48)
    with pytest.raises(TypeError):
        S.serialized_attention(qkv, order.int(), inverse, cu, 2, 48)
    with pytest.raises(TypeError):
        S.serialized_attention(qkv, order, inverse.int(), cu, 2, 48)
    with pytest.raises(TypeError):
        S.serialized_attention(qkv, order, inverse, cu.long(), 2, 48)
    with pytest.raises(TypeError):
        S.serialized_attention(qkv, order, inverse, cu, 2, 48, softmax_scale=torch.tensor(0.3))
    with pytest.raises(ValueError):
        S.serialized_attention(torch.zeros(6, 47), order, inverse, cu, 2, 48)        # not (N, 3 C)
    with pytest.raises(ValueError):
        S.serialized_attention(qkv, order, inverse, cu, 4, 48)                       # D = 4
    with pytest.raises(ValueError):
        S.serialized_attention(qkv, order, inverse, cu, 2, 300)                      # patch > 256
    with pytest.raises(ValueError):
        S.serialized_attention(qkv, order, inverse[:5], cu, 2, 48)                   # inverse is (N,)
    with pytest.raises(ValueError):
        S.serialized_attention(qkv, order[:5], inverse, cu, 2, 48)                   # fewer slots than points
    with pytest.raises(ValueError):
        S.serialized_attention(qkv, order, inverse, cu[:0], 2, 48)
    old = S.SERATTN_BACKEND
    try:
        S.SERATTN_BACKEND = "triton"
        with pytest.raises(ValueError, match="SERATTN_BACKEND"):
            S.serialized_attention_forward(SR.Module(16, 2, 4), SR.Point())
    finally:
        S.SERATTN_BACKEND = old
