"""CPU: the numpy restatement of the fine Gaussian head and the fine-set assembly (tests/finehead_ref.py) against torch autograd of
the literal composition in float64, the recorded surface of the reference (tests/golden/finehead_surface.json), the case tables
(tests/finehead_cases.py), and everything generativedensification_amd.finehead decides before it touches a GPU."""
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

import finehead_cases as FC
import finehead_ref as R

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "gdr.h")
REFERENCE = os.environ.get("GDR_REFERENCE_TREE", "/root/reference")


def fh():
    from generativedensification_amd import finehead as H

    return H


def test_surface_record_equals_the_reference():
    if not os.path.exists(os.path.join(REFERENCE, "lightning", "network.py")):
        pytest.skip("the reference tree is not on this machine")
    spec = importlib.util.spec_from_file_location("make_finehead_surface", os.path.join(HERE, "golden", "make_finehead_surface.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.record(REFERENCE) == R.surface()


def test_surface_is_what_the_module_serves():
    s = R.surface()
    for kind in ("GaussianModule", "GaussianResModule"):
        assert [layer["type"] for layer in s[kind]["feat2attr"]["layers"]] == ["Linear", "act_layer", "Linear"]
        assert s[kind]["init"]["defaults"]["act_layer"] == "nn.GELU" and s[kind]["feat2attr"]["constructor"] == "Sequential"
        assert s[kind]["feat2attr"]["layers"][2]["args"][1] == {"names": ["num_sh"], "plus": 8}
        assert s[kind]["slices"] == ["slice_sh", "slice_opacity", "slice_scale", "slice_rotation"]      # the attribute's column order
        assert s[kind]["forward"]["update_keys"] == ["attribute"]
    assert s["GaussianModule"]["forward"]["reads"] == ["point.leaf_point.feat", "self.feat2attr"] and s["GaussianModule"]["forward"]["updates"] == ["point.leaf_point"]
    assert set(s["GaussianResModule"]["forward"]["reads"]) == {"point.attribute", "point.feat", "self.enable_residual_attribute", "self.feat2attr", "self.is_first"}
    assert s["GaussianResModule"]["forward"]["updates"] == ["point"]
    assert s["group_cat"]["params"] == ["tensors", "index", "dim", "return_index"] and s["_union_gaussians"]["params"] == ["self", "point_list"]
    assert s["_union_gaussians"]["split"] == ["sh", "opacity", "scaling", "rotation"] == s["_union_gaussians"]["returns"][1:]
    assert s["_union_gaussians"]["split_sizes"] == ["sh_dim", "opacity_dim", "scaling_dim", "rotation_dim"]
    assert [c["name"] for c in s["concatenations"]] == ["_" + k for k in R.OUTPUTS]
    shifted = {c["name"]: [m for m in c["fine"] if m.endswith("_shift")] for c in s["concatenations"]}
    assert shifted == {"_centers": [], "_shs": [], "_opacity": ["self.opacity_shift"], "_scaling": ["self.fine_scaling_shift"], "_rotation": []}
    for c in s["concatenations"]:
        assert "selected_pts_mask" in c["survivors"] and (("mask" in c["survivors"]) == (c["name"] != "_shs"))


def test_erf_and_gelu_of_the_restatement():
    z = np.linspace(-6.0, 6.0, 241)
    want = np.array([math.erf(v) for v in z])
    assert np.abs(R._erf(z) - want).max() <= 4e-16
    assert np.abs(R.gelu(z) - torch.nn.functional.gelu(torch.from_numpy(z)).numpy()).max() <= 1e-15
    eps = 1e-6
    assert np.abs(R.gelu_slope(z) - (R.gelu(z + eps) - R.gelu(z - eps)) / (2 * eps)).max() <= 1e-9


@pytest.mark.parametrize("shape", [(17, 8, 3), (65, 40, 12), (33, 160, 48)], ids=lambda s: "rows%d-C%d-sh%d" % s)
def test_head_restatement_equals_torch_float64_and_autograd(shape):
    rows, C, sh_dim = shape
    p = FC.head_params(C, sh_dim, F32)
    xa, ga = FC.head_draw(rows, C, sh_dim, F32, 0)
    m = R.make_module("GaussianModule", C, {3: 0, 12: 1, 48: 3}[sh_dim]).double()
    params = fh()._params(m)
    with torch.no_grad():
        for t, k in zip(params, R.PARAMS):
            t.copy_(torch.from_numpy(np.array(p[k])))
    x = torch.from_numpy(np.array(xa)).requires_grad_(True)
    point = R.reference_module_forward(m, R.Point(leaf_point=R.Point(feat=x)))
    out = point.leaf_point.attribute
    out.backward(torch.from_numpy(np.array(ga)))
    args = [xa] + [p[k] for k in R.PARAMS]
    ref = {"out": R.head(*args), **R.head_grad(*args, ga)}
    got = {"out": out, "dx": x.grad, **{"d" + k: t.grad for k, t in zip(R.PARAMS, params)}}
    for k, v in got.items():
        a = v.detach().numpy()
        assert a.shape == ref[k].shape, k
        assert np.abs(a - ref[k]).max() <= 1e-12 * max(1.0, np.abs(ref[k]).max()), k


@pytest.mark.parametrize("attr_dt", [F32, BF16], ids=["float32", "bfloat16"])
@pytest.mark.parametrize("name", [n for n in FC.ASSEMBLY if FC.ASSEMBLY[n][0]])
def test_assembly_restatement_equals_the_torch_lines_on_the_cpu(name, attr_dt):
    d = FC.assembly_inputs(name, attr_dt)
    level_rows, Nc, _, _, sh_dim = FC.ASSEMBLY[name]
    t = lambda a, dt=F32: torch.from_numpy(np.array(a)).to(dt)      # noqa: E731
    levels = [(t(c).requires_grad_(True), t(a, attr_dt).requires_grad_(True)) for c, a in d["levels"]]
    coarse = [t(a).requires_grad_(True) for a in d["coarse"]]
    fine = t(d["shs_fine"]).requires_grad_(True)
    res = R.reference_assemble(levels, coarse, fine, t(d["mask"], torch.bool), t(d["selected"], torch.bool), sh_dim, FC.OPACITY_SHIFT, FC.SCALING_SHIFT)
    ref = R.assemble(d["levels"], d["coarse"], d["shs_fine"], d["mask"], d["selected"], sh_dim, FC.OPACITY_SHIFT, FC.SCALING_SHIFT)
    for a, k in zip(res, R.OUTPUTS):
        assert a.dtype == F32 and np.array_equal(a.detach().numpy().view(np.uint32), ref[k].view(np.uint32)), (name, k)
    torch.autograd.backward(list(res), [t(d["grads"][k]) for k in R.OUTPUTS])
    glevels, dense, dfine = R.assemble_grad(list(level_rows), Nc, d["mask"], d["selected"], sh_dim, d["grads"])
    for (c, a), (dc, da) in zip(levels, glevels):
        assert torch.equal(c.grad, t(dc)) and a.grad.dtype == attr_dt and torch.equal(a.grad, t(da).to(attr_dt))
    assert all(torch.equal(c.grad, t(g)) for c, g in zip(coarse, dense)) and torch.equal(fine.grad, t(dfine))


def test_cases_are_what_they_are_for():
    H = fh()
    assert FC.TILE_ROWS == H.TILE_ROWS and FC.SLAB_MIN == H.SLAB_MIN
    from generativedensification_amd import _lib as L

    assert FC.SCAN_CHUNK == L.GDR_FINEHEAD_SCAN_CHUNK
    shapes = FC.head_shapes(H.backward_step)
    assert {s[1] for s in shapes} == {8, 40, 160, 256} and {s[2] for s in shapes} == {3, 12, 48}
    for C in FC.HEAD_C:
        for sh in FC.HEAD_SH:
            rows = {s[0] for s in shapes if s[1:] == (C, sh)}
            assert {17, H.TILE_ROWS + 1, H.SLAB_MIN + 1} <= rows
            for dt in (F32, BF16, F16):
                step = H.backward_step(dt, C, sh)
                assert step in (16, 32, 64) and step + 1 in rows
            assert FC.repeats(C, sh) * min(C, sh + 8) >= FC.MIN_ELEMENTS
    assert H.backward_step(BF16, 256, 12) < H.backward_step(BF16, 8, 12)      # both ends of the LDS rule are among the cases
    lv, Nc, _, _, _ = FC.ASSEMBLY["chunks"]
    d = FC.assembly_inputs("chunks", F32)
    assert Nc > 2 * FC.SCAN_CHUNK and d["mask"].sum() > FC.SCAN_CHUNK and sum(lv) % 4
    assert any(0 in FC.ASSEMBLY[n][0] for n in FC.ASSEMBLY) and {len(FC.ASSEMBLY[n][0]) for n in FC.ASSEMBLY} >= {0, 1, 2, 3}
    assert FC.assembly_inputs("no_survivors", F32)["selected"].all() and not FC.assembly_inputs("all_survive", F32)["selected"].any()
    assert FC.assembly_inputs("mask_all", F32)["mask"].all()


def test_constants_equal_the_header():
    H = fh()
    text = open(HEADER).read()
    defines = dict(re.findall(r"#define (GDR_FINEHEAD_\w+) (\d+)", text))
    assert int(defines["GDR_FINEHEAD_MAX_C"]) == H.MAX_C and int(defines["GDR_FINEHEAD_TILE_ROWS"]) == H.TILE_ROWS
    assert int(defines["GDR_FINEHEAD_SLAB_MIN"]) == H.SLAB_MIN and int(defines["GDR_FINEHEAD_MAX_LEVELS"]) == H.MAX_LEVELS
    from generativedensification_amd import _lib as L

    for name, value in defines.items():
        assert getattr(L, name) == int(value), name
    declared = set(re.findall(r"\b(gdr_finehead_\w+)\(", text))
    assert declared and declared <= set(L.EXPORTED_SYMBOLS)


def test_envelope_edges():
    H = fh()
    assert H.in_envelope(76800, 256, 12) and H.in_envelope(4800, 256, 12)            # the base config's two levels
    assert H.in_envelope(0, 8, 3) and H.in_envelope(1, 256, 48) and H.in_envelope((1 << 31) - 1, 8, 27)
    assert not any(H.in_envelope(*s) for s in ((1, 4, 3), (1, 12, 3), (1, 264, 3), (1, 8, 4), (1, 8, 75), (1, 8, 0), (1 << 31, 8, 3), (-1, 8, 3)))


def test_covers_is_true_exactly_for_the_recorded_layer_list():
    H = fh()
    C, P = 16, 20
    lin = lambda i, o, **kw: nn.Linear(i, o, **kw)      # noqa: E731
    for kind in ("GaussianModule", "GaussianResModule"):
        m = R.make_module(kind, 256, 1)
        assert H.covers(m) and m.feat2attr[2].out_features == 20 and isinstance(m.feat2attr[1], nn.GELU)
        assert H.covers(R.make_module(kind, C, 1, layers=[lin(C, C), nn.GELU(approximate="none"), lin(C, P)]))
        for layers in ([lin(C, C), nn.GELU(approximate="tanh"), lin(C, P)], [lin(C, C, bias=False), nn.GELU(), lin(C, P)],
                       [lin(C, C), nn.GELU(), lin(C, P, bias=False)], [lin(C, 32), nn.GELU(), lin(32, P)], [lin(C, C), nn.ReLU(), lin(C, P)],
                       [lin(C, C), nn.GELU(), lin(C, P), nn.Identity()], [lin(C, P)], [lin(C, C), nn.GELU(), lin(C, 8)]):
            assert not H.covers(R.make_module(kind, C, 1, layers=layers))
    assert not H.covers(nn.Linear(4, 4))


def test_torch_backend_and_uncovered_modules_run_the_reference_lines_on_the_cpu():
    H = fh()
    feat = torch.randn(5, 16)
    saved = H.HEAD_BACKEND
    try:
        for kind, forward, reference in (("GaussianModule", H.gaussian_module_forward, R.reference_module_forward),
                                         ("GaussianResModule", H.gaussian_res_module_forward, R.reference_res_module_forward)):
            m = R.make_module(kind, 16, 1, is_first=False, enable_residual_attribute=True)
            prior = torch.randn(5, 20)
            point = lambda: (lambda p: R.Point(leaf_point=p) if kind == "GaussianModule" else p)(R.Point(feat=feat, attribute=prior))      # noqa: E731
            attr = lambda p: (p.leaf_point if kind == "GaussianModule" else p).attribute      # noqa: E731
            H.HEAD_BACKEND = "torch"
            assert torch.equal(attr(forward(m, point())), attr(reference(m, point())))
            H.HEAD_BACKEND = "cuda"
            with pytest.raises(ValueError):
                forward(m, point())
            H.HEAD_BACKEND = "hip"
            with pytest.raises(RuntimeError, match="no CPU fallback"):      # covered and in the envelope: the kernels, which need the GPU
                forward(m, point())
            other = R.make_module(kind, 16, 1, layers=[nn.Linear(16, 16), nn.GELU(approximate="tanh"), nn.Linear(16, 20)])
            assert torch.equal(attr(forward(other, point())), attr(reference(other, point())))      # not covered: the torch lines
            odd = R.make_module(kind, 12, 1)                                                            # C = 12 is outside the envelope
            p12 = R.Point(feat=torch.randn(5, 12), attribute=prior)
            p12 = R.Point(leaf_point=p12) if kind == "GaussianModule" else p12
            assert attr(forward(odd, p12)).shape == (5, 20)
    finally:
        H.HEAD_BACKEND = saved


def test_cpu_tensors_raise_runtime_error_and_checks_come_before_the_library(monkeypatch):
    H = fh()
    from generativedensification_amd import _lib as L

    def no_load():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(L, "load", no_load)
    z = torch.zeros
    good = [z(5, 8), z(8, 8), z(8), z(11, 8), z(11)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.gaussian_head(*good)
    for bad in (good[:1] + [z(8, 8).double()] + good[2:], [good[0].long()] + good[1:], [None] + good[1:]):
        with pytest.raises(TypeError):
            H.gaussian_head(*bad)
    with pytest.raises(TypeError):
        H.gaussian_head(*good, out_dtype=torch.float16)
    for bad in ([z(5, 12), z(12, 12), z(12), z(11, 12), z(11)], good[:3] + [z(12, 8), z(12)], [z(5)] + good[1:], good[:1] + [z(8, 16)] + good[2:]):
        with pytest.raises(ValueError):
            H.gaussian_head(*bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # a CPU tensor is refused whatever its size
        H.gaussian_head(z(0, 8), *good[1:])

    b = lambda n: z(n, dtype=torch.bool)      # noqa: E731
    lv = [(z(2, 3), z(2, 20))]
    ok = dict(levels=lv, centers_coarse=z(3, 3), opacity_coarse=z(3, 1), scaling_coarse=z(3, 3), rotation_coarse=z(3, 4), shs_fine=z(2, 4, 3), mask=b(3),
              selected_pts_mask=b(2), sh_dim=12, opacity_shift=0.0, fine_scaling_shift=0.0)
    call = lambda **kw: H.assemble_fine_gaussians(**{**ok, **kw})      # noqa: E731
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call()
    for kw in (dict(mask=z(3)), dict(selected_pts_mask=z(2)), dict(centers_coarse=z(3, 3).double()), dict(levels=[(z(2, 3), z(2, 20).double())]),
               dict(levels=[(z(2, 3).half(), z(2, 20))]), dict(levels=[(z(2, 3), z(2, 20)), (z(1, 3), z(1, 20).half())]), dict(sh_dim=12.0),
               dict(n_survivors=1.5), dict(levels=[(z(2, 3),)]), dict(shs_fine=z(2, 4, 3).half())):
        with pytest.raises(TypeError):
            call(**kw)
    for kw in (dict(sh_dim=4), dict(levels=lv * 9), dict(levels=[(z(2, 3), z(2, 21))]), dict(levels=[(z(2, 4), z(2, 20))]), dict(opacity_coarse=z(3, 2)),
               dict(shs_fine=z(2, 12)), dict(shs_fine=z(3, 4, 3)), dict(n_survivors=3), dict(n_survivors=-1), dict(mask=b(1)), dict(mask=z(3, 1, dtype=torch.bool))):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(NotImplementedError, match="_union_gaussians"):
        call(levels=[(z(2, 3), z(2, 20), torch.tensor([1, 2]))])
    # (a single-sample offset passes that check and reaches the device test)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(levels=[(z(2, 3), z(2, 20), torch.tensor([2]))])


def test_library_refuses_before_any_launch_without_a_gpu():
    from generativedensification_amd import _lib as L

    lib = L.load()
    f32, bf16 = L.GDR_NORM_DTYPES["f32"], L.GDR_NORM_DTYPES["bf16"]
    fake, ws = 0x1000, 0x10000              # aligned, never dereferenced
    q = lib.gdr_finehead_workspace_bytes
    assert q(L.GDR_FINEHEAD_WS_PACKED_FORWARD, bf16, 0, 256, 12) >= (256 * 256 + 20 * 256) * 2
    assert q(L.GDR_FINEHEAD_WS_PACKED_BACKWARD, f32, 0, 256, 12) >= (2 * 256 * 256 + 20 * 256) * 4
    one = q(L.GDR_FINEHEAD_WS_PARTIALS, f32, L.GDR_FINEHEAD_SLAB_MIN, 8, 3)
    raw = (8 * 8 + 11 * 8 + 8 + 11) * 8          # one partial set of f64
    two = q(L.GDR_FINEHEAD_WS_PARTIALS, f32, L.GDR_FINEHEAD_SLAB_MIN + 1, 8, 3)
    assert raw <= one < 2 * raw <= two and one % 256 == two % 256 == 0      # a second slab
    for bad in ((7, f32, 1, 8, 3), (0, 5, 1, 8, 3), (2, f32, -1, 8, 3), (2, f32, 1, 12, 3), (2, f32, 1, 8, 4), (2, f32, 1 << 31, 8, 3)):
        assert q(*bad) == 0 and b"finehead" in lib.gdr_last_error(), bad
    assert lib.gdr_finehead_backward_step(bf16, 12, 3) == 0 and lib.gdr_finehead_backward_step(7, 8, 3) == 0

    def fwd(x=fake, dt=f32, rows=4, C=8, sh=3, out=fake, odt=f32):
        return lib.gdr_finehead_forward(x, dt, fake, fake, f32, fake, f32, rows, C, sh, out, odt, None)

    def bwd(x=fake, dt=f32, rows=4, C=8, sh=3, gx=fake, w=None, nbytes=0):
        return lib.gdr_finehead_backward(x, dt, fake, fake, f32, rows, C, sh, fake, f32, gx, w, nbytes, None)

    assert fwd(rows=0) == 0
    for kw in ({"C": 12}, {"C": 264}, {"sh": 4}, {"rows": 1 << 31}, {"x": fake + 8}, {"out": fake + 2}):
        assert fwd(**kw) == -3 and b"finehead" in lib.gdr_last_error(), kw
    for kw in ({"rows": -1}, {"dt": 3}, {"x": None}, {"out": None}, {"odt": bf16}):
        assert fwd(**kw) == -1 and b"finehead" in lib.gdr_last_error(), kw
    for kw in ({"C": 12}, {"sh": 5}, {"x": fake + 4}, {"gx": fake + 8}, {"w": ws + 16, "nbytes": 1 << 20}):
        assert bwd(**kw) == -3 and b"finehead" in lib.gdr_last_error(), kw
    assert bwd(gx=None) == -1 and bwd(x=None) == -1 and bwd(dt=9) == -1 and bwd(w=ws, nbytes=64) == L.GDR_ERR_WORKSPACE
    fold = lambda w=ws, nbytes=1 << 20, C=8, out=fake, odt=f32: lib.gdr_finehead_fold(      # noqa: E731
        w, nbytes, f32, 4, C, 3, out, odt, None, f32, None, f32, None, f32, None)
    assert fold(w=None) == -1 and fold(odt=7) == -1 and fold(C=12) == -3 and fold(w=ws + 16) == -3 and fold(nbytes=64) == L.GDR_ERR_WORKSPACE
    pack = lambda w=fake, wdt=f32, C=8, packed=fake, dt=f32: lib.gdr_finehead_pack(w, wdt, fake, f32, C, 3, 0, packed, dt, None)      # noqa: E731
    assert pack(C=12) == -3 and pack(packed=fake + 8) == -3 and pack(w=None) == -1 and pack(wdt=4) == -1 and pack(dt=-1) == -1
    assert lib.gdr_finehead_scan_bytes(-1, 0) == 0 and lib.gdr_finehead_scan_bytes(1 << 31, 0) == 0 and lib.gdr_finehead_scan_bytes(2049, 1) >= 16
    scan = lambda mask=fake, Nc=4, count=fake, w=ws, nbytes=1 << 20: lib.gdr_finehead_scan(mask, Nc, fake, 2, w, nbytes, fake, fake, fake, fake, count, None)      # noqa: E731
    assert scan(mask=None) == -1 and scan(count=None) == -1 and scan(Nc=-1) == -1 and scan(Nc=1 << 31) == -3 and scan(w=ws + 8) == -1
    assert scan(nbytes=0) == L.GDR_ERR_WORKSPACE
    import ctypes as C

    one_ptr, rows1 = (C.c_void_p * 1)(fake), (C.c_int64 * 1)(2)
    asm = lambda n_levels=1, rows=rows1, adt=f32, sh=12, Nc=3, n_masked=2, n_rest=1, out=fake, maps=fake: lib.gdr_finehead_assemble(      # noqa: E731
        n_levels, one_ptr, one_ptr, rows, adt, sh, fake, fake, fake, fake, Nc, fake, n_masked, maps, maps, n_rest, 0.0, 0.0, out, fake, fake, fake, fake, None)
    assert asm(n_levels=9) == -3 and asm(sh=5) == -3 and asm(n_rest=3) == -3 and asm(Nc=1 << 31) == -3 and asm(rows=(C.c_int64 * 1)(1 << 31)) == -3
    assert asm(adt=5) == -1 and asm(Nc=-1) == -1 and asm(out=None) == -1 and asm(out=fake + 2) == -1 and asm(maps=None) == -1
    assert asm(rows=(C.c_int64 * 1)(-1)) == -3 and b"finehead" in lib.gdr_last_error()
    asm_bwd = lambda n_levels=1, adt=f32, sh=12, n_rest=1, ranks=fake, gc=fake: lib.gdr_finehead_assemble_backward(      # noqa: E731
        n_levels, rows1, adt, sh, fake, None, None, None, None, ranks, ranks, 3, 2, n_rest, one_ptr, one_ptr, gc, None, None, None, None, None)
    assert asm_bwd(n_levels=9) == -3 and asm_bwd(sh=5) == -3 and asm_bwd(n_rest=3) == -3 and asm_bwd(adt=5) == -1 and asm_bwd(ranks=None) == -1
    assert asm_bwd(gc=fake + 2) == -1
