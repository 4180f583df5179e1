"""CPU: the fold of generativedensification_amd/viewattn.py against nn.MultiheadAttention itself in float64, the gradients of
the fold, the numpy gradient restatement against central differences, the recorded surface of the reference's
Decoder.forward_fine against what decoder_forward_fine reads, and the argument checks (which raise before the library loads)."""
import ast
import inspect
import itertools

import numpy as np
import pytest
import torch
from torch import nn

import viewattn_cases as VC
import viewattn_ref as R

F64 = torch.float64
GRID = list(itertools.product(VC.FOLD_GRID, (False, True), (False, True)))


def va():
    from generativedensification_amd import viewattn as V

    return V


def _case(shape, bias, packed):
    E, H, Ck, V = shape
    mha = VC.make_mha(E, H, Ck, bias, packed)
    x, cond, g = VC.fold_inputs(E, H, E if packed else Ck, V)
    return mha, x, cond, g


@pytest.mark.parametrize("shape,bias,packed", GRID, ids=str)
def test_fold_and_numpy_core_equal_multihead_attention_in_float64(shape, bias, packed):
    mha, x, cond, _ = _case(shape, bias, packed)
    # (kdim = vdim = embed_dim is the packed layout whether it is asked for or not)
    assert (mha.in_proj_weight is not None) == (packed or shape[2] == shape[0]) and (mha.in_proj_bias is not None) == bias
    with torch.no_grad():
        ref = mha(torch.from_numpy(x)[:, None], torch.from_numpy(cond), torch.from_numpy(cond), need_weights=False)[0][:, 0].numpy()
        A, a_bias, Bm, b_bias, scale = va().fold_attention_weights(mha)
    H = shape[1]
    assert A.dtype == F64 and A.shape == (H * cond.shape[2], shape[0]) and Bm.shape == (shape[0], H * cond.shape[2])
    assert (a_bias is None) == (b_bias is None) == (not bias) and scale == (shape[0] // H) ** -0.5
    t = x @ A.numpy().T + (a_bias.numpy() if bias else 0.0)
    u = R.view_attention_pool(t.reshape(len(x), H, -1), cond, scale)
    out = u.reshape(len(x), -1) @ Bm.numpy().T + (b_bias.numpy() if bias else 0.0)
    err, top = np.abs(out - ref).max(), np.abs(ref).max()
    print(f"fold {shape} bias={bias} packed={packed}: max|d|={err:.3e} max|ref|={top:.3e}")
    assert err <= 1e-12 * top


@pytest.mark.parametrize("shape,bias,packed", GRID, ids=str)
def test_gradients_through_the_fold_equal_autograd_through_multihead_attention(shape, bias, packed):
    mha, x, cond, g = _case(shape, bias, packed)
    g = torch.from_numpy(g)
    grads = []
    for folded in (False, True):
        mha.zero_grad()
        xs, cs = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(cond).requires_grad_(True)
        if folded:
            out = R.folded_attention_torch(va().fold_attention_weights(mha), xs, cs, shape[1])
        else:
            out = mha(xs[:, None], cs, cs, need_weights=False)[0][:, 0]
        out.backward(g)
        grads.append({"x": xs.grad, "cond": cs.grad, **{n: p.grad.clone() for n, p in mha.named_parameters()}})
    assert set(grads[0]) == set(grads[1]) and len(grads[0]) == 2 + len(list(mha.parameters()))
    for name, want in grads[0].items():
        if name == "in_proj_bias":       # the k third has no gradient either way: the k bias drops out of the softmax
            E = shape[0]
            assert float(want[E:2 * E].abs().max()) <= 1e-12 and float(grads[1][name][E:2 * E].abs().max()) == 0.0
        err, top = float((grads[1][name] - want).abs().max()), float(want.abs().max())
        if shape[3] == 1 and name in ("x", "q_proj_weight", "k_proj_weight", "in_proj_weight", "in_proj_bias"):
            # one view: p = 1 whatever s is, so nothing flows through s and the exact gradient of x, q and k is zero.  What
            # both sides hold there is the rounding of terms that cancel, and those are of the size of the gradient that
            # does flow, cond's; that is the scale (in_proj_* also hold the v third, which is of that size itself)
            top = max(top, float(grads[0]["cond"].abs().max()))
        print(f"fold-grad {shape} bias={bias} packed={packed} {name}: max|d|={err:.3e} max|ref|={top:.3e}")
        assert err <= 1e-10 * top, name


def test_numpy_gradients_equal_central_differences():
    rng = np.random.default_rng(5)
    N, H, Ck, V, scale = 3, 2, 4, 3, 0.7
    t, cond, g = rng.standard_normal((N, H, Ck)), rng.standard_normal((N, V, Ck)), rng.standard_normal((N, H, Ck))
    dt, dcond = R.view_attention_pool_grad(t, cond, scale, g)

    def loss(t_, cond_):
        return float((R.view_attention_pool(t_, cond_, scale) * g).sum())

    h = 1e-6
    for arr, grad, which in ((t, dt, 0), (cond, dcond, 1)):
        num = np.zeros_like(arr)
        for idx in np.ndindex(arr.shape):
            hi, lo = arr.copy(), arr.copy()
            hi[idx] += h
            lo[idx] -= h
            num[idx] = (loss(hi, cond) - loss(lo, cond) if which == 0 else loss(t, hi) - loss(t, lo)) / (2 * h)
        # central differences in float64: truncation h^2 |f'''| ~ 1e-12, rounding eps |f| / h ~ 1e-9
        assert np.abs(num - grad).max() <= 1e-7 * max(1.0, np.abs(grad).max()), which
    # the torch restatement states the same function
    tt, cc = torch.from_numpy(t).requires_grad_(True), torch.from_numpy(cond).requires_grad_(True)
    out = R.view_attention_pool_torch(tt, cc, scale)
    out.backward(torch.from_numpy(g))
    assert np.abs(out.detach().numpy() - R.view_attention_pool(t, cond, scale)).max() <= 1e-14
    assert np.abs(tt.grad.numpy() - dt).max() <= 1e-13 and np.abs(cc.grad.numpy() - dcond).max() <= 1e-13


def test_surface_of_the_reference_is_what_decoder_forward_fine_reads():
    S = R.surface()
    fn = va().decoder_forward_fine
    assert list(inspect.signature(fn).parameters) == S["forward_fine"]["params"]
    tree = ast.parse(inspect.getsource(fn))
    reads = sorted({n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name)
                    and n.value.id == "self"})
    assert reads == S["forward_fine"]["reads"] == ["cross_att", "feature_dim", "mlp_fine", "norm"]
    # the indices it takes from mlp_fine are the recorded Linear, ReLU, Linear
    taken = sorted({n.slice.value for n in ast.walk(tree) if isinstance(n, ast.Subscript) and isinstance(n.value, ast.Attribute)
                    and n.value.attr == "mlp_fine"})
    assert taken == [0, 1, 2] and S["mlp_fine"]["types"] == ["Linear", "ReLU", "Linear"]
    assert S["mlp_fine"]["indices"] == {"Linear": [0, 2], "ReLU": [1]}
    assert S["cross_att"]["constructor"] == "nn.MultiheadAttention"
    assert S["cross_att"]["keywords"] == {"embed_dim": "in_dim", "num_heads": 16, "kdim": "cond_dim", "vdim": "cond_dim",
                                          "dropout": 0.0, "bias": False, "batch_first": True} and S["cond_dim"] == 8
    # the stand-in built from the record has the parameter names the fold reads, and the fold covers it
    m = R.make_decoder(80, 12)
    names = {n for n, _ in m.cross_att.named_parameters()}
    assert names == {"q_proj_weight", "k_proj_weight", "v_proj_weight", "out_proj.weight"}
    assert m.cross_att.in_proj_bias is None and m.cross_att.out_proj.bias is None
    A, a_bias, Bm, b_bias, scale = va().fold_attention_weights(m.cross_att)
    assert A.shape == (128, 80) and Bm.shape == (80, 128) and a_bias is None and b_bias is None and scale == 5 ** -0.5
    assert A.dtype == torch.float32 and A.requires_grad and Bm.requires_grad
    assert [type(layer).__name__ for layer in m.mlp_fine] == S["mlp_fine"]["types"] and m.mlp_fine[2].out_features == 92


def test_fold_runs_in_float32_whatever_the_autocast_state_and_the_module_dtype():
    m = VC.make_mha(80, 16, 8, True, False).to(torch.bfloat16)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        A, a_bias, Bm, b_bias, _ = va().fold_attention_weights(m)
    assert {x.dtype for x in (A, a_bias, Bm, b_bias)} == {torch.float32}


def test_fold_refuses_what_it_does_not_cover():
    V = va()
    refused = [nn.MultiheadAttention(16, 2, batch_first=False), nn.MultiheadAttention(16, 2, batch_first=True, add_bias_kv=True),
               nn.MultiheadAttention(16, 2, batch_first=True, add_zero_attn=True),
               nn.MultiheadAttention(16, 2, batch_first=True, dropout=0.1), nn.MultiheadAttention(16, 2, batch_first=True, kdim=8, vdim=4)]
    for m in refused:
        with pytest.raises(NotImplementedError):
            V.fold_attention_weights(m)
    V.fold_attention_weights(nn.MultiheadAttention(16, 2, batch_first=True, dropout=0.1).eval())     # (no dropout in eval mode)
    with pytest.raises(TypeError):
        V.fold_attention_weights(nn.Linear(4, 4))


def test_argument_checks_raise_their_documented_types_before_the_library_is_loaded(monkeypatch):
    V = va()
    from generativedensification_amd import _lib as L

    def no_load():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(L, "load", no_load)
    t, cond = torch.zeros(5, 16, 8), torch.zeros(5, 3, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.view_attention_pool(t, cond, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.view_attention_pool(t.view(5, 128), cond, 0.5, num_heads=16)
    for bad_t, bad_cond in ((t.double(), cond), (t, cond.double()), (t.long(), cond), (t.numpy(), cond), (t, None)):
        with pytest.raises(TypeError):
            V.view_attention_pool(bad_t, bad_cond, 0.5)
    for bad_t, bad_cond, kw in ((t, cond[0], {}), (t.view(5, 128), cond, {}), (t, cond, {"num_heads": 16}), (t[:4], cond, {}),
                                (torch.zeros(5, 16, 4), cond, {}), (torch.zeros(5, 16, 5), torch.zeros(5, 3, 5), {}),
                                (torch.zeros(5, 65, 8), cond, {}), (torch.zeros(5, 0, 8), cond, {}),
                                (t, torch.zeros(5, 17, 8), {}), (t, torch.zeros(5, 0, 8), {}),
                                (t.view(5, 128), cond, {"num_heads": 8})):
        with pytest.raises(ValueError):
            V.view_attention_pool(bad_t, bad_cond, 0.5, **kw)
    with pytest.raises(ValueError):
        V.view_attention_pool(t, cond, float("nan"))
    m = R.make_decoder(80, 12)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.decoder_forward_fine(m, torch.zeros(5, 80), cond)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.single_query_cross_attention(m.cross_att, torch.zeros(5, 80), cond)
    with pytest.raises(ValueError):
        V.single_query_cross_attention(m.cross_att, torch.zeros(5, 40), cond)
    with pytest.raises(ValueError):
        V.single_query_cross_attention(m.cross_att, torch.zeros(5, 80), torch.zeros(5, 3, 4))


def test_library_refuses_what_lies_beyond_the_envelope_without_a_gpu():
    """the entry points check their arguments before any device work: GDR_ERR_UNSUPPORTED (-3) beyond the envelope"""
    from generativedensification_amd import _lib as L

    lib = L.load()
    fake = 0x1000                  # 16-byte aligned, never dereferenced
    f32 = L.GDR_NORM_DTYPES["f32"]

    def fwd(N=4, H=16, Ck=8, V=3, t=fake, ts=128, cs=24, os_=128, dt=f32):
        return lib.gdr_viewattn_forward(t, ts, dt, fake, cs, f32, N, H, Ck, V, 0.5, fake, os_, f32, None)

    def bwd(N=4, H=16, Ck=8, V=3, gt=fake, gs=128):
        return lib.gdr_viewattn_backward(fake, gs, f32, fake, 128, f32, fake, 24, f32, N, H, Ck, V, 0.5, gt, fake, None)

    assert lib.gdr_abi_version() == 17
    assert fwd(N=0) == 0 and bwd(N=0) == 0
    for kw in ({"Ck": 5}, {"Ck": 32}, {"H": 65}, {"V": 17}, {"N": (1 << 27) + 1}, {"t": fake + 8}, {"ts": 132}, {"ts": 120}, {"cs": 16},
               {"os_": 100}):
        assert fwd(**kw) == -3 and b"viewattn" in lib.gdr_last_error(), kw
    for kw in ({"Ck": 2}, {"H": 128}, {"V": 32}, {"gt": fake + 4}, {"gs": 12}):
        assert bwd(**kw) == -3 and b"viewattn" in lib.gdr_last_error(), kw
    for kw in ({"N": -1}, {"H": 0}, {"V": 0}, {"dt": 7}, {"t": None}):
        assert fwd(**kw) == -1, kw
