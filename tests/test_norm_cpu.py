"""CPU: the float64 restatement of the fused row normalisations (tests/norm_ref.py) against autograd of the torch composition
written here from torch operators; the surface of the mirror class and functions against what the reference declares
(tests/golden/norm_surface.json); the refusals that need no GPU; the workspace query."""
import inspect
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_cases as NC
import norm_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-13


def norm():
    from generativedensification_amd import norm as N

    return N


def t64(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).double().requires_grad_(grad)


def torch_ada(feat, scale, offset):
    """gather(scale) * layer_norm(feat), rows behind the last end zero: index_select on a zero-padded scale"""
    n = feat.shape[0]
    seg = torch.searchsorted(offset, torch.arange(n), right=True)
    padded = torch.cat([scale, scale.new_zeros(1, scale.shape[1])])
    return padded.index_select(0, seg) * F.layer_norm(feat, feat.shape[1:])


def torch_pe(x, feat, freq, s):
    fx = torch.flatten(freq[None, :, None] * x[:, None, :], -2, -1)
    z = torch.cat([torch.sin(fx), torch.cos(fx), feat.repeat_interleave(s, 0)], dim=-1)
    return F.layer_norm(z, z.shape[1:])


def close(got, want, what):
    err = float(np.abs(np.asarray(got) - want.detach().numpy()).max()) if want.numel() else 0.0
    assert err <= TOL, (what, err)


ADA_LAYOUTS = {          # an empty segment, a one-row segment and tail rows behind offset[-1]
    "plain": (9, 8, [9]),
    "empty_one_row_tail": (23, 16, [4, 4, 5, 17]),
    "first_empty": (12, 24, [0, 7, 12]),
    "all_tail": (5, 8, [0]),
}


@pytest.mark.parametrize("layout", list(ADA_LAYOUTS))
def test_ada_restatement_agrees_with_autograd_of_the_composition(layout):
    n, c, offset = ADA_LAYOUTS[layout]
    rng = np.random.default_rng(n)
    feat, scale, g = rng.standard_normal((n, c)) * 2 + 0.5, rng.standard_normal((len(offset), c)), rng.standard_normal((n, c))
    f_t, s_t = t64(feat, True), t64(scale, True)
    out = torch_ada(f_t, s_t, torch.tensor(offset))
    out.backward(t64(g))
    close(R.ada_layer_norm(feat, scale, offset), out, "out")
    dfeat, dscale = R.ada_layer_norm_grad(feat, scale, offset, g)
    close(dfeat, f_t.grad, "dfeat")
    close(dscale, s_t.grad, "dscale")
    seg = R.segment_of_rows(offset, n)
    assert not np.any(R.ada_layer_norm(feat, scale, offset)[seg >= len(offset)]) and not np.any(dfeat[seg >= len(offset)])
    for b in range(len(offset)):
        if not np.any(seg == b):
            assert not np.any(dscale[b])


@pytest.mark.parametrize("case", ["one_parent", "c160", "f16_base1.5"])
def test_pe_restatement_agrees_with_autograd_of_the_composition(case):
    x, feat, freq, s, g = NC.pe_inputs(case)
    x = x * 1000.0                                   # arguments up to the tens: every quadrant of sin / cos
    x_t, f_t = t64(x, True), t64(feat, True)
    out = torch_pe(x_t, f_t, t64(freq), s)
    out.backward(t64(g))
    close(R.pe_concat_layer_norm(x, feat, freq, s), out, "out")
    dx, dfeat = R.pe_concat_layer_norm_grad(x, feat, freq, s, g)
    scale = max(1.0, float(freq.max()))              # dx carries a factor f_k: the bound is relative to it
    assert float(np.abs(dx - x_t.grad.numpy()).max()) <= TOL * scale
    close(dfeat, f_t.grad, "dfeat")


def test_a_constant_row_gives_zeros_and_finite_gradients():
    feat, scale, offset, g = NC.ada_inputs("c160", constant_row=7)
    out = R.ada_layer_norm(feat, scale, offset)
    dfeat, dscale = R.ada_layer_norm_grad(feat, scale, offset, g)
    assert not np.any(out[7]) and np.isfinite(dfeat).all() and np.isfinite(dscale).all()


def test_surface_matches_the_reference():
    surface = json.load(open(os.path.join(HERE, "golden", "norm_surface.json")))
    ada, pe = surface["AdaLayerNorm"], surface["positional_encoding"]
    N = norm()
    assert list(inspect.signature(N.AdaLayerNorm.__init__).parameters) == ada["init"]
    assert list(inspect.signature(N.AdaLayerNorm.forward).parameters) == ada["forward"]
    assert list(inspect.signature(N.ada_layer_norm_forward).parameters) == ada["forward"]
    assert inspect.signature(N.AdaLayerNorm.__init__).parameters["eps"].default == ada["init_defaults"]["eps"] == 1e-5
    assert inspect.signature(N.ada_layer_norm).parameters["eps"].default == ada["init_defaults"]["eps"]
    assert inspect.signature(N.pe_concat_layer_norm).parameters["eps"].default == torch.nn.LayerNorm(8).eps
    m = N.AdaLayerNorm(16, 24)
    assert ada["children"] == [{"name": "affine", "module": "Linear"}]
    assert [n for n, _ in m.named_children()] == [c["name"] for c in ada["children"]] and isinstance(m.affine, torch.nn.Linear)
    assert sorted(m.state_dict()) == ["affine.bias", "affine.weight"] and m.eps == 1e-5
    assert (m.affine.in_features, m.affine.out_features) == (24, 16)
    # the column order of the restatement is positional_encoding's: frequencies first, [sin, cos], then the features
    assert pe["params"] == ["f", "x"] and pe["concatenates"] == ["sin", "cos"]
    assert list(inspect.signature(N.pe_concat_layer_norm).parameters) == ["x", "feat", "frequencies", "upscale_factor", "eps"]
    z, _ = R.pe_rows(np.array([[0.1, 0.2, 0.3]]), np.zeros((1, 8)), np.array([1.0, 2.0]), 1)
    assert np.allclose(z[0, :12], np.concatenate([np.sin([0.1, 0.2, 0.3, 0.2, 0.4, 0.6]), np.cos([0.1, 0.2, 0.3, 0.2, 0.4, 0.6])]))


def test_refusals_that_need_no_gpu():
    N = norm()
    feat, scale, offset = torch.zeros(4, 16), torch.zeros(1, 16), torch.tensor([4])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        N.ada_layer_norm(feat, scale, offset)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        N.AdaLayerNorm(16, 8)(feat, torch.zeros(1, 8), offset)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        N.pe_concat_layer_norm(torch.zeros(8, 3), feat, torch.ones(2), 2)
    with pytest.raises(NotImplementedError, match="raw-coordinate"):
        N.pe_concat_layer_norm(torch.zeros(8, 3), feat, torch.ones(0), 2)
    with pytest.raises(TypeError, match="float32, float16 or bfloat16"):
        N.ada_layer_norm(feat.double(), scale, offset)
    with pytest.raises(TypeError, match="float32, float16 or bfloat16"):
        N.pe_concat_layer_norm(torch.zeros(8, 3), feat, torch.arange(2), 2)
    with pytest.raises(TypeError, match="integer tensor"):
        N.ada_layer_norm(feat, scale, offset.float())
    with pytest.raises(TypeError, match="must be a tensor"):
        N.ada_layer_norm(feat, scale, [4])
    # the C entry points refuse the same before any launch
    lib = __import__("generativedensification_amd._lib", fromlist=["load"]).load()
    fake = 0x1000                                    # never dereferenced: every refusal happens before a launch
    f32 = 2
    assert lib.gdr_norm_ada_forward(fake, 12, f32, fake, 12, f32, fake, 4, 1, 12, 1e-5, fake, f32, None) == -3       # C % 8
    assert b"multiple of 8" in lib.gdr_last_error()
    assert lib.gdr_norm_ada_forward(fake, 2048, f32, fake, 2048, f32, fake, 4, 1, 2048, 1e-5, fake, f32, None) == -3  # C > 1024
    assert lib.gdr_norm_ada_forward(fake, 16, f32, fake, 16, f32, fake, 4, 0, 16, 1e-5, fake, f32, None) == -1       # B = 0
    assert lib.gdr_norm_ada_forward(fake, 16, f32, fake, 16, f32, fake, 4, 1025, 16, 1e-5, fake, f32, None) == -3    # B > 1024
    assert lib.gdr_norm_ada_forward(fake, 16, 7, fake, 16, f32, fake, 4, 1, 16, 1e-5, fake, f32, None) == -1         # dtype
    assert lib.gdr_norm_ada_forward(fake, 16, f32, fake, 16, f32, fake, 1 << 31, 1, 16, 1e-5, fake, f32, None) == -3  # N >= 2^31
    assert lib.gdr_norm_ada_forward(fake + 4, 16, f32, fake, 16, f32, fake, 4, 1, 16, 1e-5, fake, f32, None) == -1   # unaligned
    assert lib.gdr_norm_ada_forward(None, 16, f32, None, 16, f32, None, 0, 1, 16, 1e-5, None, f32, None) == 0        # N = 0
    assert lib.gdr_norm_pe_forward(fake, f32, fake, 16, f32, fake, f32, 4, 2, 16, 0, 1e-5, fake, 16, f32, None) == -3    # F = 0
    assert lib.gdr_norm_pe_forward(fake, f32, fake, 16, f32, fake, f32, 4, 2, 16, 17, 1e-5, fake, 120, f32, None) == -3  # F > 16
    assert lib.gdr_norm_pe_forward(fake, f32, fake, 16, f32, fake, f32, 4, 17, 16, 2, 1e-5, fake, 32, f32, None) == -3   # S > 16
    assert lib.gdr_norm_pe_forward(fake, f32, fake, 16, f32, fake, f32, 1 << 30, 2, 16, 2, 1e-5, fake, 32, f32, None) == -3
    assert lib.gdr_norm_pe_forward(fake, f32, fake, 16, f32, fake, f32, 4, 2, 16, 2, 1e-5, fake, 28, f32, None) == -1    # out stride
    assert lib.gdr_norm_pe_forward(None, f32, None, 16, f32, None, f32, 0, 2, 16, 2, 1e-5, None, 32, f32, None) == 0     # P = 0
    assert lib.gdr_norm_pe_backward(fake, 29, f32, fake, f32, fake, 16, f32, fake, f32, 4, 2, 16, 2, 1e-5, fake, fake, None) == -1
    assert b"even stride" in lib.gdr_last_error()
    assert lib.gdr_norm_ada_backward(fake, 16, f32, fake, 16, f32, fake, 16, f32, fake, 64, 1, 16, 1e-5, 0x1000, 16, fake, fake,
                                     None) == -4     # workspace too small
    for bad in ((4, 0, 16), (4, 1, 12), (-1, 1, 16), (4, 1025, 16)):
        assert lib.gdr_norm_ada_backward_bytes(*bad) == 0


def test_python_refuses_the_envelope_without_a_gpu():
    """Types, shapes and the envelope are checked before the device, with the exception types segment.py uses."""
    N = norm()
    offset = torch.tensor([4])
    for c in (12, 1032):
        with pytest.raises(ValueError, match="multiple of 8"):
            N.ada_layer_norm(torch.zeros(4, c), torch.zeros(1, c), offset)
        with pytest.raises(ValueError, match="multiple of 8"):
            N.pe_concat_layer_norm(torch.zeros(8, 3), torch.zeros(4, c), torch.ones(2), 2)
    with pytest.raises(ValueError, match="segments are outside"):
        N.ada_layer_norm(torch.zeros(4, 16), torch.zeros(0, 16), torch.zeros(0, dtype=torch.int64))
    with pytest.raises(ValueError, match="needs scale"):
        N.ada_layer_norm(torch.zeros(4, 16), torch.zeros(2, 16), offset)
    with pytest.raises(ValueError, match="frequencies are outside"):
        N.pe_concat_layer_norm(torch.zeros(8, 3), torch.zeros(4, 16), torch.ones(17), 2)
    with pytest.raises(ValueError, match="upscale_factor"):
        N.pe_concat_layer_norm(torch.zeros(68, 3), torch.zeros(4, 16), torch.ones(2), 17)
    with pytest.raises(ValueError, match="x must be"):
        N.pe_concat_layer_norm(torch.zeros(9, 3), torch.zeros(4, 16), torch.ones(2), 2)


def test_workspace_query_is_monotone_in_n():
    lib = __import__("generativedensification_amd._lib", fromlist=["load"]).load()
    for b, c in ((1, 8), (4, 160), (1024, 1024)):
        prev = 0
        for n in (0, 1, 31, 32, 33, 4999, 76_800, 1 << 20, (1 << 31) - 1):
            nbytes = lib.gdr_norm_ada_backward_bytes(n, b, c)
            assert nbytes >= prev and nbytes > 0 and nbytes % 256 == 0, (n, b, c)
            prev = nbytes
        assert lib.gdr_norm_ada_backward_bytes(76_800, b, c) >= (76_800 // 32) * 2 * c * 4 + b * c * 4
