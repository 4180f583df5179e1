"""CPU: the numpy restatement of the LayerNorm + 2x transposed convolution (tests/deconv3d_ref.py) against torch's float64
F.layer_norm / F.conv_transpose3d and their autograd on every case, the envelope and `covers` truth tables, the size query
and the refusals of the C ABI (which need no GPU), the argument checks of generativedensification_amd/deconv3d.py (which
raise before the library loads), vol_transformer_forward with the torch tail against the reference's lines, and the
recorded surface of the reference's tail."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import deconv3d_cases as DC
import deconv3d_ref as R


def d3():
    from generativedensification_amd import deconv3d as D3

    return D3


NORMS = ("none", "plain", "affine")


def norm_of(kind, ln_w, ln_b):
    return {"none": None, "plain": (None, None, DC.EPS), "affine": (ln_w, ln_b, DC.EPS)}[kind]


@pytest.mark.parametrize("kind", NORMS)
@pytest.mark.parametrize("name", list(DC.CASES))
def test_restatement_equals_torch_float64_and_autograd(name, kind):
    x64, w64, b64, lw64, lb64, g64 = DC.inputs(name)
    x, w, b, lw, lb = (torch.from_numpy(a).requires_grad_(True) for a in (x64, w64, b64, lw64, lb64))
    n = x
    if kind != "none":
        affine = (lw, lb) if kind == "affine" else (None, None)
        n = F.layer_norm(x.permute(0, 2, 3, 4, 1), (x.shape[1],), *affine, eps=DC.EPS).permute(0, 4, 1, 2, 3)
    out = F.conv_transpose3d(n, w, b, stride=2)
    out.backward(torch.from_numpy(g64))
    norm = norm_of(kind, lw64, lb64)
    ref, grads = R.deconv(x64, w64, b64, norm), R.deconv_grad(x64, w64, g64, norm)
    pairs = [("out", out.detach(), ref), ("dx", x.grad, grads["dx"]), ("dw", w.grad, grads["dw"]), ("db", b.grad, grads["db"])]
    if kind == "affine":
        pairs += [("dgamma", lw.grad, grads["dgamma"]), ("dbeta", lb.grad, grads["dbeta"])]
    else:
        assert lw.grad is None and lb.grad is None
    # float64 sums in two orders.  A few eps of the sum of magnitudes; a row that is BIG times the others or constant passes
    # through rstd up to 1 / sqrt(eps) = 1e3, which scales the absolute rounding of the mean accordingly
    for what, got, want in pairs:
        err, top = np.abs(got.numpy() - want).max(), np.abs(want).max()
        print(f"deconv3d-restatement {name}/{kind}/{what}: max|d|={err:.3e} max|ref|={top:.3e}")
        assert got.shape == want.shape and err <= 1e-9 * max(top, 1.0), what


def test_inputs_are_what_the_cases_are_for():
    D3 = d3()
    assert DC.TILE_ROWS == D3.TILE_ROWS and DC.SLAB_ROWS == D3.GRAD_WEIGHT_SLAB_ROWS
    rows = {n: s[0] * s[3] * s[4] * s[5] for n, s in DC.CASES.items()}
    assert rows["run"] == DC.TILE_ROWS + 3 and rows["slabs"] == DC.SLAB_ROWS + 1 and rows["one"] == 1
    assert DC.CASES["ref_slim"][1:3] == (256, 80) and 256 < DC.CASES["mid"][1] <= 512 < DC.CASES["wide"][1] and DC.CASES["wide"][2] > 128
    for name, (B, cin, cout, D, H, W) in DC.CASES.items():
        x, w, b, lw, lb, g = DC.inputs(name)
        assert x.shape == (B, cin, D, H, W) and w.shape == (cin, cout, 2, 2, 2) and b.shape == (cout,) and lw.shape == lb.shape == (cin,)
        assert g.shape == (B, cout, 2 * D, 2 * H, 2 * W) and D3.in_envelope(B, cin, cout, D, H, W)
        assert not np.array_equal(w, w[:, :, ::-1, ::-1, ::-1])
    x = DC.inputs("flat")[0]
    assert np.ptp(x[(0, slice(None)) + DC.FLAT_ROW]) == 0 and np.abs(x[(0, slice(None)) + DC.BIG_ROW]).mean() > 300 * np.abs(x[0, :, 0, 1, 0]).mean()


def test_envelope_and_covers_truth_tables():
    D3 = d3()
    assert D3.in_envelope(3, 256, 80, 32, 32, 32)           # the reference shape
    assert D3.in_envelope(0, 8, 8, 1, 1, 1) and D3.in_envelope(1, 1024, 256, 1, 1, 1) and D3.in_envelope(1 << 8, 8, 8, 1 << 7, 1 << 7, (1 << 6) - 1)
    assert not any(D3.in_envelope(*s) for s in ((1, 4, 8, 2, 2, 2), (1, 12, 8, 2, 2, 2), (1, 8, 12, 2, 2, 2), (1, 1032, 8, 2, 2, 2),
                                                (1, 8, 264, 2, 2, 2), (1, 8, 8, 0, 2, 2), (-1, 8, 8, 2, 2, 2),
                                                (1 << 8, 8, 8, 1 << 7, 1 << 7, 1 << 6)))      # 2^31 child voxels
    good = nn.ConvTranspose3d(8, 16, kernel_size=2, stride=2)
    assert D3.covers(good) and D3.covers(nn.ConvTranspose3d(8, 16, (2, 2, 2), stride=(2, 2, 2), padding=0, bias=False))
    assert D3.covers(good, nn.LayerNorm(8, eps=1e-6)) and D3.covers(good, nn.LayerNorm(8, elementwise_affine=False))
    x = torch.zeros(1, 8, 2, 2, 2)
    for m in (nn.ConvTranspose3d(8, 16, 3, stride=2), nn.ConvTranspose3d(8, 16, 2, stride=1), nn.ConvTranspose3d(8, 16, 2, stride=2, padding=1),
              nn.ConvTranspose3d(8, 16, 2, stride=2, output_padding=1), nn.ConvTranspose3d(8, 16, 2, stride=2, dilation=2),
              nn.ConvTranspose3d(8, 16, 2, stride=2, groups=2), nn.ConvTranspose3d(8, 16, (2, 2, 1), stride=2),
              nn.ConvTranspose3d(8, 16, 2, stride=(2, 2, 1)), nn.ConvTranspose2d(8, 16, 2, stride=2), nn.Conv3d(8, 16, 2, stride=2), nn.Linear(8, 8)):
        assert not D3.covers(m)
        with pytest.raises(NotImplementedError):
            D3.conv_transpose3d_2x_of(m, x)
    for norm in (nn.LayerNorm(16), nn.LayerNorm((2, 8)), nn.LayerNorm((8, 2, 2, 2)), nn.GroupNorm(2, 8), nn.Identity()):
        assert not D3.covers(good, norm)
        with pytest.raises(NotImplementedError):
            D3.conv_transpose3d_2x_of(good, x, norm)


def test_cpu_tensors_raise_runtime_error():
    D3 = d3()
    x, w = torch.zeros(1, 8, 2, 2, 2), torch.zeros(8, 8, 2, 2, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D3.conv_transpose3d_2x(x, w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D3.conv_transpose3d_2x(x, w, torch.zeros(8), norm=(torch.ones(8), None, 1e-6))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D3.conv_transpose3d_2x_of(nn.ConvTranspose3d(8, 8, 2, stride=2), x, nn.LayerNorm(8))


def test_argument_checks_raise_their_documented_types_before_the_library_is_loaded(monkeypatch):
    D3 = d3()
    from generativedensification_amd import _lib as L

    def no_load():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(L, "load", no_load)
    x, w, b = torch.zeros(2, 8, 2, 3, 4), torch.zeros(8, 16, 2, 2, 2), torch.zeros(16)
    ok_norm = (torch.ones(8), torch.zeros(8), 1e-6)
    for bad in ((x.double(), w, b), (x, w.double(), b), (x, w, b.long()), (x.numpy(), w, b), (x, None, b), (x.to(torch.int32), w, None),
                (x, w, b, (torch.ones(8).double(), None, 1e-6)), (x, w, b, (None, torch.ones(8).long(), 1e-6)), (x, w, b, (None, None, "1e-6"))):
        with pytest.raises(TypeError):
            D3.conv_transpose3d_2x(*bad)
    for bad in ((x[0], w, b), (x, w[:, :, 0], b), (x, torch.zeros(8, 16, 2, 2, 1), b), (x, torch.zeros(16, 16, 2, 2, 2), b),
                (x, torch.zeros(8, 16, 3, 3, 3), b), (x, w, torch.zeros(8)), (x, w, torch.zeros(16, 1)),
                (torch.zeros(2, 12, 2, 2, 2), torch.zeros(12, 8, 2, 2, 2), None), (torch.zeros(1, 4, 2, 2, 2), torch.zeros(4, 8, 2, 2, 2), None),
                (x, torch.zeros(8, 12, 2, 2, 2), None), (x, torch.zeros(8, 264, 2, 2, 2), None),
                (torch.zeros(1, 1032, 1, 1, 1), torch.zeros(1032, 8, 2, 2, 2), None),
                (x, w, b, (torch.ones(16), None, 1e-6)), (x, w, b, (None, torch.ones(4), 1e-6)), (x, w, b, (None, None, -1.0)), (x, w, b, (None, None))):
        with pytest.raises(ValueError):
            D3.conv_transpose3d_2x(*bad)
    huge = torch.zeros(1, dtype=torch.bfloat16).expand(1 << 8, 8, 1 << 7, 1 << 7, 1 << 6)      # 2^31 child voxels, no memory
    with pytest.raises(ValueError, match="voxels"):
        D3.conv_transpose3d_2x(huge, torch.zeros(8, 8, 2, 2, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # everything else in order: only the device is wrong
        D3.conv_transpose3d_2x(x, w, b, ok_norm)


def test_workspace_query_answers_without_a_gpu_and_grows_monotonically():
    from generativedensification_amd import _lib as L

    lib = L.load()
    f32, bf16 = L.GDR_NORM_DTYPES["f32"], L.GDR_NORM_DTYPES["bf16"]
    q = lib.gdr_deconv3d_workspace_bytes
    kinds = (L.GDR_DECONV3D_WS_PACKED, L.GDR_DECONV3D_WS_GRAD_WEIGHT, L.GDR_DECONV3D_WS_GRAD_BIAS, L.GDR_DECONV3D_WS_GRAD_INPUT,
             L.GDR_DECONV3D_WS_STATS)
    assert q(L.GDR_DECONV3D_WS_PACKED, bf16, 0, 256, 80) >= 8 * 256 * 80 * 2 and q(L.GDR_DECONV3D_WS_PACKED, f32, 0, 256, 80) >= 8 * 256 * 80 * 4
    for what in kinds:
        prev = 0
        for rows, c in ((0, 8), (1, 8), (64, 8), (4096, 16), (4097, 16), (98304, 256), (1 << 24, 256), (((1 << 31) - 1) // 8, 256)):
            n = q(what, f32, rows, c, c)
            assert n >= prev and n % 256 == 0 and n > 0, (what, rows, c)
            prev = n
    assert q(L.GDR_DECONV3D_WS_GRAD_WEIGHT, f32, 4097, 16, 16) == 2 * q(L.GDR_DECONV3D_WS_GRAD_WEIGHT, f32, 4096, 16, 16)      # a second slab
    assert q(L.GDR_DECONV3D_WS_GRAD_BIAS, f32, 98304, 256, 80) >= 80 * 8 and q(L.GDR_DECONV3D_WS_STATS, f32, 98304, 256, 80) >= 98304 * 16
    for bad in ((7, f32, 64, 8, 8), (0, 5, 64, 8, 8), (1, f32, -1, 8, 8)):
        assert q(*bad) == 0 and b"deconv3d" in lib.gdr_last_error(), bad
    for bad in ((1, f32, 64, 12, 8), (1, f32, 64, 8, 264), (1, f32, 64, 1032, 8), (1, f32, 1 << 28, 8, 8)):
        assert q(*bad) == 0 and b"deconv3d" in lib.gdr_last_error(), bad


def test_library_refuses_before_any_launch_without_a_gpu():
    """-1 for invalid arguments, GDR_ERR_UNSUPPORTED (-3) beyond the envelope or for a misaligned buffer, GDR_ERR_WORKSPACE for a
    short workspace; B = 0 is GDR_OK without a launch"""
    from generativedensification_amd import _lib as L

    lib = L.load()
    fake, ws = 0x1000, 0x10000              # aligned, never dereferenced
    f32 = L.GDR_NORM_DTYPES["f32"]

    def fwd(x=fake, dt=f32, packed=fake, bias=None, has_norm=0, lw=None, lb=None, eps=1e-6, B=1, D=2, H=2, W=2, cin=8, cout=8, stats=None,
            out=fake):
        return lib.gdr_deconv3d_forward(x, dt, packed, bias, f32, has_norm, lw, f32, lb, f32, eps, B, D, H, W, cin, cout, stats, out, None)

    def gin(g=fake, packed=fake, x=fake, stats=fake, has_norm=1, lw=None, B=1, D=2, H=2, W=2, cin=8, cout=8, w=ws, nbytes=1 << 20, gx=fake,
            glw=None, glb=None, dt=f32):
        return lib.gdr_deconv3d_grad_input(g, dt, packed, x, stats, has_norm, lw, f32, B, D, H, W, cin, cout, w, nbytes, gx, glw, f32, glb, f32,
                                           None)

    def gw(x=fake, stats=None, has_norm=0, g=fake, B=1, D=2, H=2, W=2, cin=8, cout=8, w=ws, nbytes=1 << 20, out=fake, odt=f32):
        return lib.gdr_deconv3d_grad_weight(x, stats, has_norm, None, f32, None, f32, g, f32, B, D, H, W, cin, cout, w, nbytes, out, odt, None)

    def gb(g=fake, n=64, cout=8, w=ws, nbytes=1 << 20, out=fake):
        return lib.gdr_deconv3d_grad_bias(g, f32, n, cout, w, nbytes, out, f32, None)

    def pack(w=fake, wdt=f32, cin=8, cout=8, packed=fake, dt=f32):
        return lib.gdr_deconv3d_pack_weight(w, wdt, cin, cout, 0, packed, dt, None)

    assert fwd(B=0) == 0
    for kw in ({"cin": 4}, {"cout": 12}, {"cin": 1032}, {"cout": 264}, {"B": 1 << 10, "D": 64, "H": 64, "W": 64}, {"x": fake + 8}, {"out": fake + 4},
               {"packed": fake + 8}, {"has_norm": 1, "stats": fake + 8}, {"bias": fake + 2}, {"has_norm": 1, "lw": fake + 1}):
        assert fwd(**kw) == -3 and b"deconv3d" in lib.gdr_last_error(), kw
    for kw in ({"B": -1}, {"D": 0}, {"W": 0}, {"dt": 3}, {"x": None}, {"packed": None}, {"out": None}, {"lw": fake}, {"has_norm": 1, "eps": -1.0},
               {"has_norm": 1, "eps": float("nan")}):
        assert fwd(**kw) == -1 and b"deconv3d" in lib.gdr_last_error(), kw
    for kw in ({"cin": 20}, {"cout": 2048}, {"g": fake + 4}, {"gx": fake + 8}, {"glw": fake, "w": ws + 16}, {"D": 1 << 16, "H": 1 << 16, "W": 1 << 16}):
        assert gin(**kw) == -3 and b"deconv3d" in lib.gdr_last_error(), kw
    assert gin(gx=None) == -1 and gin(stats=None) == -1 and gin(g=None) == -1 and gin(dt=9) == -1 and gin(has_norm=0, glw=fake) == -1
    assert gin(glw=fake, w=None) == -1 and gin(glb=fake, nbytes=64) == L.GDR_ERR_WORKSPACE
    for kw in ({"cin": 20}, {"cout": 2048}, {"x": fake + 4}, {"w": ws + 16}, {"D": 1 << 16, "H": 1 << 16, "W": 1 << 16}):
        assert gw(**kw) == -3 and b"deconv3d" in lib.gdr_last_error(), kw
    assert gw(w=None) == -1 and gw(out=None) == -1 and gw(H=0) == -1 and gw(odt=9) == -1 and gw(g=None) == -1 and gw(has_norm=1) == -1
    assert gw(nbytes=64) == L.GDR_ERR_WORKSPACE and gb(nbytes=16) == L.GDR_ERR_WORKSPACE
    assert gb(cout=12) == -3 and gb(g=fake + 8) == -3 and gb(n=-8) == -1 and gb(n=12) == -1 and gb(out=None) == -1
    assert pack(cin=12) == -3 and pack(cout=264) == -3 and pack(packed=fake + 8) == -3 and pack(w=None) == -1 and pack(wdt=4) == -1 and pack(dt=-1) == -1


# ---- vol_transformer_forward ------------------------------------------------------------------------------------------------------

def mirror_inputs(B=2, V=2, cond_dim=24, res=4):
    rng = np.random.default_rng([29, B, V, cond_dim, res])
    return torch.from_numpy(rng.standard_normal((B, V, cond_dim, res, res, res))).float()


def test_torch_tail_equals_the_reference_lines_bit_for_bit_on_the_cpu():
    D3 = d3()
    m = R.make_mirror(R.make_stub_layers(2))
    bound = copy.deepcopy(m)
    feats = mirror_inputs()
    saved = D3.TAIL_BACKEND
    try:
        D3.TAIL_BACKEND = "torch"
        out = D3.vol_transformer_forward(bound, feats)
        D3.TAIL_BACKEND = "nothing"
        with pytest.raises(ValueError, match="TAIL_BACKEND"):
            D3.vol_transformer_forward(bound, feats)
        D3.TAIL_BACKEND = "hip"                    # no CPU fallback: the switch does not change what a CPU tensor gets
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            D3.vol_transformer_forward(bound, feats)
    finally:
        D3.TAIL_BACKEND = saved
    conds = []
    want = R.reference_forward(m, feats, conds)
    assert out.shape == want.shape == (2, 8, 8, 8, 8) and out.dtype == want.dtype and out.is_contiguous() and torch.equal(out, want)
    # each layer was handed the reference's cond (one permuting copy, the same values) and a channels-last volume
    assert len(conds) == 1 and conds[0].shape == (2 * 8, 8 * 2, 24)
    for layer in bound.layers:
        cond, n_group, block_size = layer.seen[0]
        assert (n_group, block_size) == (2, 2) and cond.is_contiguous() and torch.equal(cond, conds[0])
    out.sum().backward()
    want.sum().backward()
    for (name, p), (_, q) in zip(bound.named_parameters(), m.named_parameters()):
        assert torch.equal(p.grad, q.grad), name


def test_initial_volume_is_the_broadcast_pos_embed_in_channels_last():
    D3 = d3()
    seen = []

    class Probe(nn.Module):
        def forward(self, x, cond, n_group, block_size):
            seen.append(x)
            return x

    m = R.make_mirror([Probe()])
    saved = D3.TAIL_BACKEND
    try:
        D3.TAIL_BACKEND = "torch"
        D3.vol_transformer_forward(m, mirror_inputs(B=3))
    finally:
        D3.TAIL_BACKEND = saved
    x = seen[0]
    assert x.shape == (3, 16, 4, 4, 4) and x.permute(0, 2, 3, 4, 1).is_contiguous() and torch.equal(x, m.pos_embed.repeat(3, 1, 1, 1, 1))
    assert x.data_ptr() != m.pos_embed.data_ptr()


def test_recorded_surface_of_the_reference_tail_is_served():
    S = R.surface()
    assert S["modules"]["norm"] == {"constructor": "nn.LayerNorm", "args": ["embed_dim"], "keywords": {"eps": "eps"}}
    assert S["modules"]["deconv"] == {"constructor": "nn.ConvTranspose3d", "args": ["embed_dim", "out_dim"],
                                      "keywords": {"kernel_size": 2, "stride": 2, "padding": 0}}
    assert S["init"]["defaults"] == {"eps": 1e-6} == {"eps": DC.EPS}
    assert S["forward"]["params"] == ["self", "image_feats"]
    assert S["forward"]["reads"] == ["block_size", "deconv", "layers", "n_groups", "norm", "pos_embed"]
    assert S["forward"]["einsum"] == ["bvcgl->bgvlc", "bcdhw->bdhwc", "bdhwc->bcdhw", "bcdhw->bdhwc"]
    D3 = d3()
    m = R.make_mirror([])
    assert D3.covers(m.deconv, m.norm) and m.norm.eps == 1e-6 and m.deconv.weight.shape == (16, 8, 2, 2, 2) and m.deconv.bias is not None
    # vol_transformer_forward reads exactly the recorded attributes
    import ast
    import inspect

    fn = ast.parse(inspect.getsource(D3.vol_transformer_forward))
    reads = sorted({n.attr for n in ast.walk(fn) if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name) and n.value.id == "self"})
    assert reads == S["forward"]["reads"]
