"""GPU: the fused row normalisations (csrc/norm.hip through generativedensification_amd.norm) against the float64 restatement
(tests/norm_ref.py) and against the torch composition on the same GPU in the same dtypes.

Accuracy bar, for every output and gradient: with e_hip = max|hip - ref64| and e_torch = max|torch - ref64| (ref64 on the inputs as
rounded to their dtypes), e_hip <= 2 e_torch + half an ulp of the result dtype at max|ref64|.  The factor 2 is for another
summation order and one differently rounded rsqrt; nothing else may differ.  Every pair is printed before it is asserted."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_cases as NC
import norm_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16


def norm():
    from generativedensification_amd import norm as N

    return N


def dev(a, dtype=None):
    return R.to_dtype(a, dtype).to(DEV) if dtype is not None else torch.as_tensor(np.asarray(a)).to(DEV)


def f64(t):
    return t.detach().double().cpu().numpy()


def torch_ada(feat, scale, offset):
    """the reference's composition without the read-back: gather(scale) * layer_norm(feat), rows behind the last end zero"""
    seg = torch.searchsorted(offset, torch.arange(feat.shape[0], device=feat.device), right=True)
    padded = torch.cat([scale, scale.new_zeros(1, scale.shape[1])])
    return padded.index_select(0, seg) * F.layer_norm(feat, feat.shape[1:])


def torch_pe(x, feat, freq, s):
    fx = torch.flatten(freq[None, :, None] * x[:, None, :], -2, -1)
    z = torch.cat([torch.sin(fx), torch.cos(fx), feat.repeat_interleave(s, 0)], dim=-1)
    return F.layer_norm(z, z.shape[1:])


def bar(what, hip, tor, ref64):
    """prints the pair, then asserts the bar"""
    assert hip.dtype == tor.dtype and hip.shape == tor.shape == ref64.shape, (what, hip.dtype, tor.dtype, hip.shape, tor.shape)
    e_hip = float(np.abs(f64(hip) - ref64).max()) if ref64.size else 0.0
    e_torch = float(np.abs(f64(tor) - ref64).max()) if ref64.size else 0.0
    slack = R.half_ulp(hip.dtype, float(np.abs(ref64).max()) if ref64.size else 0.0)
    print(f"norm-bar {what}: e_hip={e_hip:.3e} e_torch={e_torch:.3e} half_ulp={slack:.3e}")
    assert np.isfinite(f64(hip)).all(), what
    return what, e_hip, e_torch, slack


def settle(results):
    bad = [(w, eh, et, s) for w, eh, et, s in results if not eh <= 2 * et + s]
    assert not bad, bad


def run_ada(name, feat_dt, scale_dt, constant_row=None):
    N = norm()
    feat64, scale64, offset, g64 = NC.ada_inputs(name, constant_row)
    feat, scale = dev(feat64, feat_dt), dev(scale64, scale_dt)
    off = dev(offset)
    ins64 = (f64(feat), f64(scale))
    leaves = [t.clone().requires_grad_(True) for t in (feat, scale)]
    out = N.ada_layer_norm(*leaves, off)
    g = dev(g64, out.dtype)
    out.backward(g)
    t_leaves = [t.clone().requires_grad_(True) for t in (feat, scale)]
    t_out = torch_ada(*t_leaves, off)
    t_out.backward(g)
    ref_out = R.ada_layer_norm(*ins64, offset)
    ref_dfeat, ref_dscale = R.ada_layer_norm_grad(*ins64, offset, f64(g))
    tag = f"A/{name}/{feat_dt}/{scale_dt}".replace("torch.", "")
    res = [bar(tag + "/out", out, t_out, ref_out), bar(tag + "/dfeat", leaves[0].grad, t_leaves[0].grad, ref_dfeat),
           bar(tag + "/dscale", leaves[1].grad, t_leaves[1].grad, ref_dscale)]
    seg = R.segment_of_rows(offset, feat.shape[0])
    tail = torch.as_tensor(seg >= len(offset)).to(DEV)
    assert not out[tail].any() and not leaves[0].grad[tail].any(), "rows behind the last end"
    empty = torch.as_tensor(np.bincount(seg, minlength=len(offset) + 1)[:len(offset)] == 0).to(DEV)
    assert not leaves[1].grad[empty].any(), "empty segments"
    return res, out, leaves


@pytest.mark.parametrize("name", list(NC.ADA))
def test_ada_f32_at_every_shape(name):
    res, _, _ = run_ada(name, F32, F32)
    settle(res)


@pytest.mark.parametrize("dtypes", [(BF16, BF16), (F16, F16), (BF16, F32), (F16, F32)], ids=str)
@pytest.mark.parametrize("name", NC.ADA_DTYPE_CASES)
def test_ada_16_bit(name, dtypes):
    res, out, leaves = run_ada(name, *dtypes)
    assert out.dtype == torch.promote_types(*dtypes) and leaves[0].grad.dtype == dtypes[0] and leaves[1].grad.dtype == dtypes[1]
    settle(res)


def test_ada_constant_row_gives_zeros_and_finite_gradients():
    for feat_dt in (F32, BF16):
        res, out, leaves = run_ada("c160", feat_dt, F32, constant_row=7)
        assert not out[7].any() and torch.isfinite(leaves[0].grad).all() and torch.isfinite(leaves[1].grad).all()
        settle(res)


def run_pe(name, x_dt, feat_dt, freq_dt):
    N = norm()
    x64, feat64, freq64, s, g64 = NC.pe_inputs(name)
    x, feat, freq = dev(x64, x_dt), dev(feat64, feat_dt), dev(freq64, freq_dt)
    ins64 = (f64(x), f64(feat), f64(freq), s)
    leaves = [t.clone().requires_grad_(True) for t in (x, feat)]
    out = N.pe_concat_layer_norm(*leaves, freq, s)
    assert out.stride(1) == 1 and out.stride(0) % 8 == 0
    g = dev(g64, out.dtype)
    out.backward(g)
    t_leaves = [t.clone().requires_grad_(True) for t in (x, feat)]
    t_out = torch_pe(*t_leaves, freq, s)
    t_out.backward(g)
    ref_out = R.pe_concat_layer_norm(*ins64)
    ref_dx, ref_dfeat = R.pe_concat_layer_norm_grad(*ins64, f64(g))
    tag = f"B/{name}/{x_dt}/{feat_dt}/{freq_dt}".replace("torch.", "")
    res = [bar(tag + "/out", out, t_out, ref_out), bar(tag + "/dx", leaves[0].grad, t_leaves[0].grad, ref_dx),
           bar(tag + "/dfeat", leaves[1].grad, t_leaves[1].grad, ref_dfeat)]
    return res, out, leaves, (x, feat, freq, s, g)


@pytest.mark.parametrize("name", list(NC.PE))
def test_pe_f32_at_every_shape(name):
    res, out, leaves, (x, feat, freq, s, g) = run_pe(name, F32, F32, F32)
    settle(res)
    # a dense gradient (rows that start on 8 bytes only) takes the narrow load path: the same bits as the padded one
    N = norm()
    again = [t.clone().requires_grad_(True) for t in (x, feat)]
    out2 = N.pe_concat_layer_norm(*again, freq, s)
    padded = torch.zeros(out2.shape[0], out2.stride(0), dtype=g.dtype, device=DEV)
    padded[:, :g.shape[1]] = g
    out2.backward(padded[:, :g.shape[1]])
    assert torch.equal(out, out2) and torch.equal(again[0].grad, leaves[0].grad) and torch.equal(again[1].grad, leaves[1].grad)


@pytest.mark.parametrize("dtypes", [(BF16, BF16, BF16), (F16, F16, F16), (BF16, BF16, F32)], ids=str)
@pytest.mark.parametrize("name", NC.PE_DTYPE_CASES)
def test_pe_16_bit(name, dtypes):
    res, out, leaves, _ = run_pe(name, *dtypes)
    assert leaves[0].grad.dtype == dtypes[0] and leaves[1].grad.dtype == dtypes[1]
    settle(res)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=str)
@pytest.mark.parametrize("name", ["c160", "f16_base1.5"])
def test_pe_16_bit_gradient_as_padded_view_equals_the_dense_one(name, dtype):
    """Outside autocast an all-16-bit call returns 16 bits and its gradient may come back as the padded view (16-byte rows, 8
    elements per lane, the last piece of a 250-element row element-wise) or dense (two elements per lane): the same bits."""
    N = norm()
    x64, feat64, freq64, s, g64 = NC.pe_inputs(name)
    x, feat, freq = dev(x64, dtype), dev(feat64, dtype), dev(freq64, dtype)
    grads = []
    for padded in (False, True):
        leaves = [t.clone().requires_grad_(True) for t in (x, feat)]
        out = N.pe_concat_layer_norm(*leaves, freq, s)
        assert out.dtype == dtype
        g = dev(g64, dtype)
        if padded:
            buf = torch.full((out.shape[0], out.stride(0)), float("nan"), dtype=dtype, device=DEV)   # the padding is never read
            buf[:, :g.shape[1]] = g
            g = buf[:, :g.shape[1]]
            assert g.stride(0) % 8 == 0 and g.data_ptr() % 16 == 0
        out.backward(g)
        grads.append((leaves[0].grad, leaves[1].grad))
    assert torch.isfinite(grads[1][0]).all() and torch.isfinite(grads[1][1]).all()
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])


def test_two_calls_are_bitwise_equal():
    N = norm()
    feat64, scale64, offset, g64 = NC.ada_inputs("long_segment")
    x64, pf64, freq64, s, pg64 = NC.pe_inputs("many_groups")
    runs = []
    for _ in range(2):
        feat, scale = dev(feat64, BF16).requires_grad_(True), dev(scale64, F32).requires_grad_(True)
        out = N.ada_layer_norm(feat, scale, dev(offset))
        out.backward(dev(g64, out.dtype))
        x, pf = dev(x64, F32).requires_grad_(True), dev(pf64, F32).requires_grad_(True)
        pout = N.pe_concat_layer_norm(x, pf, dev(freq64, F32), s)
        pout.backward(dev(pg64, pout.dtype))
        runs.append((out.detach(), feat.grad, scale.grad, pout.detach(), x.grad, pf.grad))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_result_dtype_is_the_compositions_with_and_without_autocast():
    N = norm()
    feat64, scale64, offset, _ = NC.ada_inputs("c160")
    x64, pf64, freq64, s, _ = NC.pe_inputs("c160")
    off = dev(offset)
    for autocast in (False, True):
        for feat_dt, scale_dt in ((F32, F32), (BF16, BF16), (BF16, F32), (F32, BF16), (F16, BF16)):
            feat, scale = dev(feat64, feat_dt), dev(scale64, scale_dt)
            with torch.autocast("cuda", dtype=BF16, enabled=autocast):
                got, want = N.ada_layer_norm(feat, scale, off), torch_ada(feat, scale, off)
            assert got.dtype == want.dtype, (autocast, feat_dt, scale_dt, got.dtype, want.dtype)
            if autocast:
                assert got.dtype == F32
        for x_dt, feat_dt, freq_dt in ((F32, F32, F32), (BF16, BF16, F32), (BF16, BF16, BF16), (F16, F32, F16)):
            x, pf, freq = dev(x64, x_dt), dev(pf64, feat_dt), dev(freq64, freq_dt)
            with torch.autocast("cuda", dtype=BF16, enabled=autocast):
                got, want = N.pe_concat_layer_norm(x, pf, freq, s), torch_pe(x, pf, freq, s)
            assert got.dtype == want.dtype and got.shape == want.shape, (autocast, x_dt, feat_dt, freq_dt, got.dtype, want.dtype)
    # under the trainer's autocast the module takes a bf16 scale from its Linear and returns float32, as the composition does
    m = N.AdaLayerNorm(160, 24).to(DEV)
    glob = torch.randn(1, 24, device=DEV)
    with torch.autocast("cuda", dtype=BF16):
        got = m(dev(feat64, BF16), glob, off)
        want = torch_ada(dev(feat64, BF16), m.affine(glob), off)
    assert got.dtype == want.dtype == F32
    assert float((got - want).detach().abs().max()) <= 2 ** -7 * float(want.detach().abs().max())


def test_module_mirror_and_rebinding_function_equal_the_functional_form():
    N = norm()
    feat64, _, offset, g64 = NC.ada_inputs("empty_segment")
    feat, off = dev(feat64, F32), dev(offset)
    gen = torch.Generator().manual_seed(3)
    state = {"affine.weight": torch.randn(256, 24, generator=gen), "affine.bias": torch.randn(256, generator=gen)}
    m = N.AdaLayerNorm(256, 24).to(DEV)
    m.load_state_dict(state)
    glob = torch.randn(3, 24, generator=gen).to(DEV)
    want = N.ada_layer_norm(feat, F.linear(glob, state["affine.weight"].to(DEV), state["affine.bias"].to(DEV)), off, 1e-5)
    assert torch.equal(m(feat, glob, off), want)
    stand_in = types.SimpleNamespace(affine=m.affine, eps=1e-5)
    assert torch.equal(N.ada_layer_norm_forward(stand_in, feat, glob, off), want)
    # a class of another family takes the forward as the reference's class does
    other = type("Other", (torch.nn.LayerNorm,), {"forward": N.ada_layer_norm_forward})(256, 1e-5, elementwise_affine=False)
    other.affine = m.affine
    assert torch.equal(other(feat, glob, off), want)
    # gradients reach the Linear
    m.zero_grad()
    m(feat, glob, off).backward(dev(g64, F32))
    assert m.affine.weight.grad is not None and torch.isfinite(m.affine.weight.grad).all() and m.affine.weight.grad.abs().max() > 0


def test_runs_under_vjp_and_under_no_grad():
    N = norm()
    feat64, scale64, offset, g64 = NC.ada_inputs("tail")
    feat, scale, off, g = dev(feat64, F32), dev(scale64, F32), dev(offset), dev(g64, F32)
    out, (dfeat, dscale) = torch.autograd.functional.vjp(lambda a, b: N.ada_layer_norm(a, b, off), (feat, scale), g)
    a, b = feat.clone().requires_grad_(True), scale.clone().requires_grad_(True)
    o = N.ada_layer_norm(a, b, off)
    o.backward(g)
    assert torch.equal(out, o) and torch.equal(dfeat, a.grad) and torch.equal(dscale, b.grad)
    with torch.no_grad():
        assert torch.equal(N.ada_layer_norm(a, b, off), o) and not N.ada_layer_norm(a, b, off).requires_grad
    x64, pf64, freq64, s, pg64 = NC.pe_inputs("c160")
    x, pf, freq, pg = dev(x64, F32), dev(pf64, F32), dev(freq64, F32), dev(pg64, F32)
    pout, (dx, dpf) = torch.autograd.functional.vjp(lambda a, b: N.pe_concat_layer_norm(a, b, freq, s), (x, pf), pg)
    a, b = x.clone().requires_grad_(True), pf.clone().requires_grad_(True)
    o = N.pe_concat_layer_norm(a, b, freq, s)
    o.backward(pg)
    assert torch.equal(pout, o) and torch.equal(dx, a.grad) and torch.equal(dpf, b.grad)
    with torch.no_grad():
        assert torch.equal(N.pe_concat_layer_norm(a, b, freq, s), o)
    # only one input wants a gradient
    a = x.clone().requires_grad_(True)
    N.pe_concat_layer_norm(a, pf, freq, s).backward(pg)
    assert torch.equal(a.grad, dx)


def test_empty_inputs_return_empty_tensors():
    N = norm()
    out = N.ada_layer_norm(torch.zeros(0, 16, device=DEV, requires_grad=True), torch.zeros(2, 16, device=DEV), dev(np.array([0, 0])))
    assert out.shape == (0, 16)
    out.sum().backward()
    pout = N.pe_concat_layer_norm(torch.zeros(0, 3, device=DEV), torch.zeros(0, 16, device=DEV), torch.ones(3, device=DEV), 4)
    assert pout.shape == (0, 34)


def test_no_host_synchronisation():
    N = norm()
    feat64, scale64, offset, g64 = NC.ada_inputs("empty_segment")
    x64, pf64, freq64, s, pg64 = NC.pe_inputs("c160")
    off, g, pg, freq = dev(offset), dev(g64, F32), dev(pg64, F32), dev(freq64, F32)
    m = N.AdaLayerNorm(256, 24).to(DEV)
    glob = torch.randn(3, 24, device=DEV)

    def work():
        feat, scale = dev(feat64, F32).requires_grad_(True), dev(scale64, F32).requires_grad_(True)
        x, pf = dev(x64, F32).requires_grad_(True), dev(pf64, F32).requires_grad_(True)
        torch.cuda.synchronize()
        return feat, scale, x, pf

    def calls(feat, scale, x, pf):
        N.ada_layer_norm(feat, scale, off).backward(g)
        m(feat, glob, off).backward(g)
        N.pe_concat_layer_norm(x, pf, freq, s).backward(pg)

    calls(*work())                                   # warm-up: library load, kernel images, the GEMM of the Linear
    args = work()
    torch.cuda.synchronize()
    previous = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        raised = False
        try:
            off[-1].item()                           # the canary: what gather_csr's read-back does
        except RuntimeError:
            raised = True
        if raised:
            calls(*args)
    finally:
        torch.cuda.set_sync_debug_mode(previous)
    if not raised:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not raise on .item() in this torch build")
    torch.cuda.synchronize()
    assert torch.isfinite(args[0].grad).all() and torch.isfinite(args[2].grad).all()
