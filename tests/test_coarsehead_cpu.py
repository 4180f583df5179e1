"""CPU: the float64 restatement of the coarse Gaussian head (tests/coarsehead_ref.py) against torch autograd of the literal
composition, what the case builder (tests/coarsehead_cases.py) asserts about gates and mask, the recorded surface of the
reference's Decoder, and everything generativedensification_amd.coarsehead decides before it touches a GPU."""
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

import coarsehead_cases as CC
import coarsehead_ref as R

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
GRADS = ("g_offset", "g_sh", "g_scaling", "g_rotation", "g_opacity", "g_centers")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gdr.h")


def ch():
    from generativedensification_amd import coarsehead as H

    return H


@pytest.mark.parametrize("name", list(CC.CASES))
def test_restatement_equals_torch_float64_and_autograd(name):
    B, N, C, K, sh_dim = CC.shape_of(name)
    d = CC.inputs(name, F32)
    t = {k: torch.from_numpy(np.array(v)) for k, v in d.items()}
    x = t["x"].clone().requires_grad_(True)
    dec = R.make_decoder(C, K, sh_dim).double()
    params = ch()._params(dec)
    with torch.no_grad():
        for p, k in zip(params, R.PARAMS):
            p.copy_(t[k])
    out = R.reference_forward_coarse(dec, x, CC.OPACITY_SHIFT, CC.SCALING_SHIFT, float64=True)
    centers, mask = R.reference_tail(out[0], out[4], t["group_centers"].view(1, N, 3), CC.HALF_CELL, K, CC.THRESHOLD)
    torch.autograd.backward(list(out) + [centers], [t[k] for k in GRADS])
    p = [d[k] for k in R.PARAMS]
    ref = R.head(d["x"], *p, K, sh_dim, CC.OPACITY_SHIFT, CC.SCALING_SHIFT, d["group_centers"], CC.HALF_CELL, CC.THRESHOLD)
    ref.update(R.head_grad(d["x"], *p, K, sh_dim, {k[2:]: d[k] for k in GRADS}, CC.HALF_CELL))
    got = dict(zip(R.OUTPUTS + ("centers",), list(out) + [centers]))
    got["dx"] = x.grad
    got.update({"d" + k: q.grad for k, q in zip(R.PARAMS, params)})
    for k, v in got.items():
        a = v.detach().numpy()
        assert a.shape == ref[k].shape, k
        assert np.abs(a - ref[k]).max() <= 1e-12 * max(1.0, np.abs(ref[k]).max()), k
    assert np.array_equal(mask.numpy(), ref["mask"])


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("name", list(CC.CASES))
def test_builder_settles_gates_and_mask(name, dtype):
    H = ch()
    B, N, C, K, sh_dim = CC.shape_of(name)
    d = CC.inputs(name, dtype)               # its own assertions: gates, switching units, both sides of the threshold, the mask
    P = sh_dim + 11
    assert d["x"].shape == (B, N, C) and d["w3"].shape == (K * P, C) and d["group_centers"].shape == (N, 3) and H.in_envelope(B * N, C, K, sh_dim)
    for k in ("x",) + R.PARAMS:
        assert np.array_equal(CC.rounded(d[k], dtype), d[k]), k
    z1, z2, e1, e2 = CC._bounds(d["x"].reshape(B * N, C), d["w1"], d["b1"], d["w2"], d["b2"])
    assert (np.abs(z1) >= 8 * e1).all() and (np.abs(z2) >= 8 * e2).all()
    ref = R.head(d["x"], *(d[k] for k in R.PARAMS), K, sh_dim, CC.OPACITY_SHIFT, CC.SCALING_SHIFT, d["group_centers"], CC.HALF_CELL, CC.THRESHOLD)
    assert (np.abs(ref["opacity"] - CC.LOGIT_THRESHOLD) > CC.MASK_MARGIN[dtype]).all()
    if name == "sat":
        assert (np.abs(ref["offset"]) == 1.0).all()


def test_cases_are_what_they_are_for():
    H = ch()
    assert CC.TILE_ROWS == H.TILE_ROWS and CC.SLAB_MIN == H.SLAB_MIN
    rows = {n: s[0][0] * s[0][1] for n, s in CC.CASES.items()}
    assert rows["one"] == 1 and rows["run"] == H.TILE_ROWS + 3 and rows["slabs"] == H.SLAB_MIN + 1
    assert CC.CASES["ref_slim"][1:] == (80, 1, 12) and CC.CASES["k2"][2] == 2 and CC.CASES["k2"][0][0] == 2
    assert CC.CASES["wide"][1] > 128 and CC.CASES["wide"][1] % 32 and (CC.CASES["wide"][3] + 11) % 16


def test_constants_equal_the_header():
    H = ch()
    text = open(HEADER).read()
    defines = dict(re.findall(r"#define (GDR_COARSEHEAD_\w+) (\d+)", text))
    assert int(defines["GDR_COARSEHEAD_MAX_C"]) == H.MAX_C and int(defines["GDR_COARSEHEAD_MAX_OUT"]) == H.MAX_OUT
    assert int(defines["GDR_COARSEHEAD_TILE_ROWS"]) == H.TILE_ROWS and int(defines["GDR_COARSEHEAD_SLAB_MIN"]) == H.SLAB_MIN
    from generativedensification_amd import _lib as L

    for name, value in defines.items():
        assert getattr(L, name) == int(value), name


def test_envelope_edges():
    H = ch()
    assert H.in_envelope(3 * 64 ** 3, 80, 1, 12)            # the reference shape
    assert H.in_envelope(0, 8, 1, 3) and H.in_envelope(1, 256, 4, 12) and H.in_envelope(1, 8, 2, 48) and H.in_envelope((1 << 31) - 1, 8, 1, 3)
    assert H.in_envelope(((1 << 31) - 1) // 4, 8, 4, 12)
    assert not any(H.in_envelope(*s) for s in ((1, 4, 1, 3), (1, 12, 1, 3), (1, 264, 1, 3), (1, 8, 0, 3), (1, 8, 5, 3), (1, 8, 1, 4), (1, 8, 1, 75),
                                               (1, 8, 3, 48), (1, 8, 4, 27), (1 << 31, 8, 1, 3), (1 << 29, 8, 4, 3), (-1, 8, 1, 3)))


def test_covers_is_true_exactly_for_the_recorded_layer_list():
    H = ch()
    s = R.surface()
    assert [layer["type"] for layer in s["mlp_coarse"]["layers"]] == ["Linear", "ReLU", "Linear", "ReLU", "Linear"]
    assert s["forward_coarse"]["returns"] == list(R.OUTPUTS) and s["forward_coarse"]["split"] == ["offset", "sh", "opacity", "scaling", "rotation"]
    assert s["forward_coarse"]["split_sizes"] == [3, "sh_dim", "opacity_dim", "scaling_dim", "rotation_dim"]
    assert s["forward_coarse"]["params"] == ["self", "feats", "opacity_shift", "scaling_shift"]
    # what decoder_forward_coarse and covers read is what the reference's method reads and its __init__ assigns
    assert set(s["forward_coarse"]["reads"]) == {"mlp_coarse", "K", "sh_dim", "opacity_dim", "scaling_dim", "rotation_dim"}
    assert set(s["forward_coarse"]["reads"]) - {"mlp_coarse"} <= set(s["init"]["attributes"])
    dec = R.make_decoder(80, 1, 12)
    assert H.covers(dec) and H.covers(R.make_decoder(24, 2, 12)) and dec.mlp_coarse[4].out_features == 23
    C = 16
    lin = lambda i, o, **kw: nn.Linear(i, o, **kw)      # noqa: E731
    for layers in ([lin(C, C), nn.ReLU(), lin(C, 14)], [lin(C, C), nn.GELU(), lin(C, C), nn.ReLU(), lin(C, 14)],
                   [lin(C, 32), nn.ReLU(), lin(32, C), nn.ReLU(), lin(C, 14)], [lin(C, C), nn.ReLU(), lin(C, C), nn.ReLU(), lin(C, 15)],
                   [lin(C, C), nn.ReLU(), lin(C, C, bias=False), nn.ReLU(), lin(C, 14)],
                   [lin(C, C), nn.ReLU(), lin(C, C), nn.ReLU(), lin(C, 14), nn.Identity()]):
        assert not H.covers(R.make_decoder(C, 1, 3, layers))
    other = R.make_decoder(C, 1, 3)
    assert H.covers(other)
    other.opacity_dim = 2
    assert not H.covers(other) and not H.covers(nn.Linear(4, 4))


def test_torch_backend_and_uncovered_modules_run_the_reference_lines_on_the_cpu():
    H = ch()
    dec = R.make_decoder(16, 2, 3)
    x = torch.randn(2, 5, 16)
    saved = H.HEAD_BACKEND
    try:
        H.HEAD_BACKEND = "torch"
        got = H.decoder_forward_coarse(dec, x, -2.0, 0.5)
        gc = torch.randn(1, 5, 3)
        full = H.coarse_gaussians(dec, x, gc, 0.25, -2.0, 0.5)
        H.HEAD_BACKEND = "cuda"
        with pytest.raises(ValueError):
            H.decoder_forward_coarse(dec, x, -2.0, 0.5)
    finally:
        H.HEAD_BACKEND = saved
    want = R.reference_forward_coarse(dec, x, -2.0, 0.5)
    assert all(torch.equal(a, b) and a.stride() == b.stride() for a, b in zip(got, want))
    centers, mask = R.reference_tail(want[0], want[4], gc, 0.25, 2)
    assert torch.equal(full[0], centers) and torch.equal(full[5], mask) and all(torch.equal(a, b) for a, b in zip(full[1:5], want[1:]))
    other = R.make_decoder(16, 2, 3, [nn.Linear(16, 28)])          # not covered: the torch lines, even with HEAD_BACKEND "hip"
    assert all(torch.equal(a, b) for a, b in zip(H.decoder_forward_coarse(other, x, -2.0, 0.5), R.reference_forward_coarse(other, x, -2.0, 0.5)))


def test_cpu_tensors_raise_runtime_error_and_checks_come_before_the_library(monkeypatch):
    H = ch()
    from generativedensification_amd import _lib as L

    def no_load():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(L, "load", no_load)
    z = torch.zeros
    good = [z(2, 3, 8), z(8, 8), z(8), z(8, 8), z(8), z(14, 8), z(14)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.coarse_head(*good, 1, 3, 0.0, 0.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.decoder_forward_coarse(R.make_decoder(8, 1, 3), good[0], 0.0, 0.0)
    for bad in (good[:1] + [z(8, 8).double()] + good[2:], [good[0].long()] + good[1:], [None] + good[1:]):
        with pytest.raises(TypeError):
            H.coarse_head(*bad, 1, 3, 0.0, 0.0)
    for k, s in ((0, 3), (1, 5), (2, 3)):
        with pytest.raises(ValueError):
            H.coarse_head(*good, k, s, 0.0, 0.0)


def test_library_refuses_before_any_launch_without_a_gpu():
    from generativedensification_amd import _lib as L

    lib = L.load()
    f32, bf16 = L.GDR_NORM_DTYPES["f32"], L.GDR_NORM_DTYPES["bf16"]
    fake, ws = 0x1000, 0x10000              # aligned, never dereferenced
    q = lib.gdr_coarsehead_workspace_bytes
    assert q(L.GDR_COARSEHEAD_WS_PACKED_FORWARD, bf16, 0, 80, 1, 12) >= (2 * 80 * 80 + 23 * 80) * 2
    assert q(L.GDR_COARSEHEAD_WS_PACKED_BACKWARD, f32, 0, 80, 1, 12) >= (4 * 80 * 80 + 23 * 80) * 4
    one = q(L.GDR_COARSEHEAD_WS_PARTIALS, f32, L.GDR_COARSEHEAD_SLAB_MIN, 8, 1, 3)
    raw = (2 * 8 * 8 + 14 * 8 + 2 * 8 + 14) * 8          # one partial set of f64
    two = q(L.GDR_COARSEHEAD_WS_PARTIALS, f32, L.GDR_COARSEHEAD_SLAB_MIN + 1, 8, 1, 3)
    assert raw <= one < 2 * raw <= two and one % 256 == two % 256 == 0      # a second slab
    for bad in ((7, f32, 1, 8, 1, 3), (0, 5, 1, 8, 1, 3), (2, f32, -1, 8, 1, 3), (2, f32, 1, 12, 1, 3), (2, f32, 1, 8, 1, 4), (2, f32, 1 << 31, 8, 1, 3)):
        assert q(*bad) == 0 and b"coarsehead" in lib.gdr_last_error(), bad

    def fwd(x=fake, dt=f32, rows=4, C=8, K=1, sh=3, out=fake, centers=None, gc=None, N=1):
        return lib.gdr_coarsehead_forward(x, dt, fake, fake, f32, fake, f32, fake, f32, rows, N, C, K, sh, 0.0, 0.0, gc, 0.0, 0.0, out, fake, fake, fake,
                                          fake, centers, None, None)

    def bwd(x=fake, dt=f32, rows=4, C=8, K=1, sh=3, gx=fake, w=None, nbytes=0):
        return lib.gdr_coarsehead_backward(x, dt, fake, fake, f32, fake, f32, rows, C, K, sh, fake, fake, None, None, None, None, None, 0.0, gx, w,
                                           nbytes, None)

    assert fwd(rows=0) == 0
    for kw in ({"C": 12}, {"C": 264}, {"K": 5}, {"sh": 4}, {"K": 3, "sh": 48}, {"rows": 1 << 31}, {"x": fake + 8}, {"out": fake + 2}):
        assert fwd(**kw) == -3 and b"coarsehead" in lib.gdr_last_error(), kw
    for kw in ({"rows": -1}, {"dt": 3}, {"x": None}, {"out": None}, {"centers": fake}, {"centers": fake, "gc": fake, "N": 3}):
        assert fwd(**kw) == -1 and b"coarsehead" in lib.gdr_last_error(), kw
    for kw in ({"C": 12}, {"sh": 5}, {"x": fake + 4}, {"gx": fake + 8}, {"w": ws + 16, "nbytes": 1 << 20}):
        assert bwd(**kw) == -3 and b"coarsehead" in lib.gdr_last_error(), kw
    assert bwd(gx=None) == -1 and bwd(x=None) == -1 and bwd(dt=9) == -1 and bwd(w=ws, nbytes=64) == L.GDR_ERR_WORKSPACE
    fold = lambda w=ws, nbytes=1 << 20, C=8, out=fake, odt=f32: lib.gdr_coarsehead_fold(      # noqa: E731
        w, nbytes, f32, 4, C, 1, 3, out, odt, None, f32, None, f32, None, f32, None, f32, None, f32, None)
    assert fold(w=None) == -1 and fold(odt=7) == -1 and fold(C=12) == -3 and fold(w=ws + 16) == -3 and fold(nbytes=64) == L.GDR_ERR_WORKSPACE
    pack = lambda w=fake, wdt=f32, C=8, packed=fake, dt=f32: lib.gdr_coarsehead_pack(w, wdt, fake, f32, fake, f32, C, 1, 3, 0, packed, dt, None)      # noqa: E731
    assert pack(C=12) == -3 and pack(packed=fake + 8) == -3 and pack(w=None) == -1 and pack(wdt=4) == -1 and pack(dt=-1) == -1
