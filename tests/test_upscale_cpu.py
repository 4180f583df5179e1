"""CPU: the float64 restatement of expand / merge (tests/upscale_ref.py) against central differences and against autograd of
the torch compositions; the surface generativedensification_amd/upscale.py reads against what the reference's two Upscale
classes declare (tests/golden/upscale_surface.json); the entry points in _lib.py and include/gdr.h; `covers`, `in_envelope`
and the refusals that need no GPU."""
import ast
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import upscale_cases as UC
import upscale_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ENTRY_POINTS = ("gdr_upscale_expand_forward", "gdr_upscale_expand_backward", "gdr_upscale_merge_forward",
                "gdr_upscale_merge_backward_bytes", "gdr_upscale_merge_backward")


def upscale():
    from generativedensification_amd import upscale as U

    return U


def central(fn, x, g, h=1e-6):
    """d <fn(x), g> / dx by central differences"""
    out = np.zeros_like(x)
    flat, oflat = x.reshape(-1), out.reshape(-1)
    for i in range(flat.size):
        keep = flat[i]
        flat[i] = keep + h
        hi = (fn(x) * g).sum()
        flat[i] = keep - h
        lo = (fn(x) * g).sum()
        flat[i] = keep
        oflat[i] = (hi - lo) / (2 * h)
    return out


@pytest.mark.parametrize("absolute", [False, True])
def test_expand_gradients_against_central_differences(absolute):
    rng = np.random.default_rng(3)
    n, s, c, f, grid = 3, 2, 8, 2, 0.5
    t, coord, feat = rng.standard_normal((n, 3 * s)), rng.uniform(-1, 1, (n, 3)), rng.standard_normal((n, c))
    freq = 2.0 ** np.arange(f)
    gx, gh = rng.standard_normal((n * s, 3)), rng.standard_normal((n * s, 6 * f + c))

    def loss_parts(t_, coord_, feat_):
        out_x, h = R.expand(t_, coord_, feat_, freq, s, grid, absolute)
        return np.concatenate([out_x.reshape(-1), h.reshape(-1)])

    g = np.concatenate([gx.reshape(-1), gh.reshape(-1)])
    dt, dcoord, dfeat = R.expand_grad(t, coord, feat, freq, s, grid, gx, gh, absolute)
    assert np.abs(central(lambda v: loss_parts(v, coord, feat), t.copy(), g) - dt).max() < 1e-7
    assert np.abs(central(lambda v: loss_parts(t, v, feat), coord.copy(), g) - dcoord).max() < 1e-7
    assert np.abs(central(lambda v: loss_parts(t, coord, v), feat.copy(), g) - dfeat).max() < 1e-7
    # a None gradient is zeros
    only_x = R.expand_grad(t, coord, feat, freq, s, grid, gx, None, absolute)
    assert not only_x[2].any() and np.allclose(only_x[1], gx.reshape(n, s, 3).sum(1))


def test_merge_gradients_against_central_differences():
    rng = np.random.default_rng(4)
    n, s, c = 5, 3, 8
    offset = np.array([2, 2, 4])
    skip, branch, scale = rng.standard_normal((n, c)), rng.standard_normal((n * s, c)), rng.standard_normal((3, c))
    keep = (rng.uniform(size=n * s) < 0.7) / 0.7
    g = rng.standard_normal((n * s, c))
    for k in (keep, None):
        dskip, dbranch, dscale = R.merge_grad(skip, branch, k, scale, offset, s, g)
        assert np.abs(central(lambda v: R.merge(v, branch, k, scale, offset, s), skip.copy(), g) - dskip).max() < 1e-7
        assert np.abs(central(lambda v: R.merge(skip, v, k, scale, offset, s), branch.copy(), g) - dbranch).max() < 1e-7
        assert np.abs(central(lambda v: R.merge(skip, branch, k, v, offset, s), scale.copy(), g) - dscale).max() < 1e-7
        out = R.merge(skip, branch, k, scale, offset, s)
        assert not out[4 * s:].any() and not dskip[4:].any() and not dbranch[4 * s:].any() and not dscale[1].any()


def test_restatement_equals_autograd_of_the_torch_compositions():
    t64 = lambda a, grad=True: torch.from_numpy(np.ascontiguousarray(a)).double().requires_grad_(grad)   # noqa: E731
    for name in ("c40_s3_abs", "c160_s2"):
        t, coord, feat, freq, s, absolute, gx, gh = UC.expand_inputs(name)
        leaves = [t64(a) for a in (t, coord, feat)]
        out_x, h = R.torch_expand(*leaves, t64(freq, False), s, UC.GRID_SIZE, absolute)
        torch.autograd.backward([out_x, h], [t64(gx, False), t64(gh, False)])
        want = R.expand_grad(t, coord, feat, freq, s, UC.GRID_SIZE, gx, gh, absolute)
        ref = R.expand(t, coord, feat, freq, s, UC.GRID_SIZE, absolute)
        assert np.abs(out_x.detach().numpy() - ref[0]).max() < 1e-13 and np.abs(h.detach().numpy() - ref[1]).max() < 1e-10
        for leaf, w in zip(leaves, want):
            assert np.abs(leaf.grad.numpy() - w).max() <= 1e-9 * max(1.0, np.abs(w).max())
    for name in ("c8_s3_b3", "c256_s16"):
        skip, branch, keep, scale, offset, s, g = UC.merge_inputs(name)
        leaves = [t64(a) for a in (skip, branch, scale)]
        out = R.torch_merge(leaves[0], leaves[1], None if keep is None else t64(keep, False), leaves[2], torch.from_numpy(offset), s)
        out.backward(t64(g, False))
        assert np.abs(out.detach().numpy() - R.merge(skip, branch, keep, scale, offset, s)).max() < 1e-12
        for leaf, w in zip(leaves, R.merge_grad(skip, branch, keep, scale, offset, s, g)):
            assert np.abs(leaf.grad.numpy() - w).max() <= 1e-11 * max(1.0, np.abs(w).max())


def self_and_point_reads():
    """the attributes of `self` / `module` and of `point` that upscale.py reads or assigns"""
    tree = ast.parse(open(os.path.join(ROOT, "generativedensification_amd", "upscale.py")).read())
    reads = {"self": set(), "point": set()}
    writes = set()
    for n in ast.walk(tree):
        if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name):
            owner = {"self": "self", "module": "self", "point": "point"}.get(n.value.id)
            if owner and isinstance(n.ctx, ast.Load):
                reads[owner].add(n.attr)
            if owner == "point" and isinstance(n.ctx, ast.Store):
                writes.add(n.attr)
        if (isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id == "getattr" and isinstance(n.args[0], ast.Name)
                and n.args[0].id in ("self", "module") and isinstance(n.args[1], ast.Constant)):
            reads["self"].add(n.args[1].value)
    return reads, writes


def test_surface_matches_the_reference():
    surface = json.load(open(os.path.join(HERE, "golden", "upscale_surface.json")))
    plain, res = surface["UpscaleModule"], surface["UpscaleResModule"]
    U = upscale()
    assert plain["forward"] == res["forward"] == list(inspect.signature(U.upscale_module_forward).parameters)
    assert list(inspect.signature(U.upscale_res_module_forward).parameters) == res["forward"]
    reads, writes = self_and_point_reads()
    # what the bound forwards read from the module is what the reference's forwards read (the Res twin's two flags included)
    assert reads["self"] == set(res["reads"]) and set(plain["reads"]) | {"enable_residual_attribute", "is_first"} == set(res["reads"])
    assert set(res["reads"]) <= set(res["assigned"])
    # from the point: the reference's, and global_feat, which the reference reads inside out_norm
    assert reads["point"] == set(res["point_reads"]) | {"global_feat"} and writes == set(res["point_writes"])
    # the stand-in module of the tests has every attribute the reference assigns
    m = R.make_module(8, 16, 2, 3)
    assert all(hasattr(m, name) for name in plain["assigned"])
    assert U.covers(m) and [type(x).__name__ for x in m.delta_f] == ["LayerNorm", "Linear", "GELU", "Linear"]


def test_entry_points_are_declared():
    from generativedensification_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "gdr.h")).read()
    for name in ENTRY_POINTS:
        assert name in L.EXPORTED_SYMBOLS, name
        m = re.search(r"^(?:int|size_t) " + name + r"\(([^;]*)\);", header, re.M)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(L._PROTOS[name][1]), name
    assert re.search(r"#define GDR_ABI_VERSION\s+17\b", header)


def test_covers_and_in_envelope():
    U = upscale()
    m = R.make_module(16, 24, 2, 3)
    assert U.covers(m)
    m.delta_x = torch.nn.Sequential(torch.nn.Linear(16, 6))
    assert not U.covers(m)
    m = R.make_module(16, 24, 2, 3)
    m.delta_f[0] = torch.nn.LayerNorm(16 + 18)                     # with affine
    assert not U.covers(m)
    m = R.make_module(16, 24, 2, 3)
    m.n_frequencies = 0
    assert not U.covers(m)
    m = R.make_module(16, 24, 2, 3)
    del m.out_norm[0].affine
    assert not U.covers(m)
    assert U.in_envelope(19200, 4, 256, 256, 15, 1) and U.in_envelope(0, 2, 8, 1024, 1, 1024)
    for bad in ((10, 17, 8, 8, 1, 1), (10, 2, 12, 8, 1, 1), (10, 2, 8, 1032, 1, 1), (10, 2, 8, 8, 17, 1), (10, 2, 8, 8, 0, 1),
                (10, 2, 8, 8, 1, 1025), (1 << 30, 2, 8, 8, 1, 1)):
        assert not U.in_envelope(*bad), bad


def test_refusals_that_need_no_gpu():
    U = upscale()
    t, coord, feat, freq = torch.zeros(4, 6), torch.zeros(4, 3), torch.zeros(4, 16), torch.ones(3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        U.expand(t, coord, feat, freq, 2, 0.01)
    with pytest.raises(ValueError):
        U.expand(t, coord, feat, freq, 3, 0.01)                   # t is (N, 3 S)
    with pytest.raises(ValueError):
        U.expand(torch.zeros(4, 51), coord, feat, freq, 17, 0.01)
    with pytest.raises(ValueError):
        U.expand(t, coord, torch.zeros(4, 12), freq, 2, 0.01)
    with pytest.raises(NotImplementedError):
        U.expand(t, coord, feat, torch.ones(0), 2, 0.01)
    with pytest.raises(TypeError):
        U.expand(t.double(), coord, feat, freq, 2, 0.01)
    with pytest.raises(TypeError):
        U.expand(t, coord, feat, freq, 2, torch.tensor(0.01))
    skip, branch, scale, offset = torch.zeros(4, 16), torch.zeros(8, 16), torch.zeros(1, 16), torch.tensor([4])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        U.merge(skip, branch, None, scale, offset, 2)
    with pytest.raises(ValueError):
        U.merge(skip, branch, None, scale, offset, 3)
    with pytest.raises(ValueError):
        U.merge(skip, branch, torch.zeros(7), scale, offset, 2)
    with pytest.raises(TypeError):
        U.merge(skip, branch, None, scale, offset.float(), 2)
    with pytest.raises(TypeError):
        U.merge(skip, branch, torch.zeros(8, dtype=torch.bool), scale, offset, 2)
    old = U.UPSCALE_BACKEND
    try:
        U.UPSCALE_BACKEND = "triton"
        with pytest.raises(ValueError, match="UPSCALE_BACKEND"):
            U.upscale_module_forward(R.make_module(8, 8, 2, 1), R.Point())
    finally:
        U.UPSCALE_BACKEND = old
