"""GPU: the folded view cross attention (csrc/viewattn.hip through generativedensification_amd.viewattn) against the float64
restatement (tests/viewattn_ref.py) and against the torch composition on the same GPU in the same dtypes.

Accuracy bar (the one of tests/test_gpu_norm.py), for the output and both gradients: with e_hip = max|hip - ref64| and
e_torch = max|torch - ref64| (ref64 on the inputs as rounded to their dtypes), e_hip <= 2 e_torch + half an ulp of the result
dtype at max|ref64|.  The factor 2 is for another summation order over Ck and V and one differently rounded exponential;
nothing else may differ.  Every pair is printed before it is asserted.  The torch composition of a mixed pair runs in the
promotion of the two dtypes and its result is rounded to t's dtype, which is what the HIP path returns."""
import copy

import numpy as np
import pytest
import torch

import viewattn_cases as VC
import viewattn_ref as R
from norm_ref import half_ulp, to_dtype

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
PAIRS = [(F32, F32), (BF16, F32), (F16, F16), (F32, BF16)]


def va():
    from generativedensification_amd import viewattn as V

    return V


def dev(a, dtype):
    return to_dtype(a, dtype).to(DEV)


def f64(t):
    return t.detach().double().cpu().numpy()


def bar(what, hip, tor, ref64):
    """prints the pair, then hands it to settle"""
    assert hip.dtype == tor.dtype and hip.shape == tor.shape == ref64.shape, (what, hip.dtype, tor.dtype, hip.shape, tor.shape)
    e_hip = float(np.abs(f64(hip) - ref64).max()) if ref64.size else 0.0
    e_torch = float(np.abs(f64(tor) - ref64).max()) if ref64.size else 0.0
    slack = half_ulp(hip.dtype, float(np.abs(ref64).max()) if ref64.size else 0.0)
    print(f"viewattn-bar {what}: e_hip={e_hip:.3e} e_torch={e_torch:.3e} half_ulp={slack:.3e}")
    assert np.isfinite(f64(hip)).all(), what
    return what, e_hip, e_torch, slack


def settle(results):
    bad = [(w, eh, et, s) for w, eh, et, s in results if not eh <= 2 * et + s]
    assert not bad, bad


def torch_pool(t, cond, scale):
    wide = torch.promote_types(t.dtype, cond.dtype)
    return R.view_attention_pool_torch(t.to(wide), cond.to(wide), scale).to(t.dtype)


def wide_rows(t):
    """the same values behind a row stride larger than the row (N, H Ck): what a slice of a wider activation looks like"""
    N, H, Ck = t.shape
    buf = torch.full((N, H * Ck + 24), float("nan"), dtype=t.dtype, device=t.device)      # (the padding is never read)
    buf[:, :H * Ck] = t.reshape(N, H * Ck)
    return buf[:, :H * Ck]


def run(name, t_dt, cond_dt):
    V = va()
    N, H, Ck, nv = VC.CASES[name]
    scale = VC.scale_of(name)
    t64, cond64, g64 = VC.inputs(name)
    t, cond, g = dev(t64, t_dt), dev(cond64, cond_dt), dev(g64, t_dt)
    a, b = t.clone().requires_grad_(True), cond.clone().requires_grad_(True)
    if name == VC.WIDE_ROWS:
        rows = wide_rows(a)
        assert rows.stride(0) > H * Ck
        out = V.view_attention_pool(rows, b, scale, num_heads=H)
    else:
        out = V.view_attention_pool(a, b, scale)
    assert out.shape == (N, H, Ck) and out.dtype == t_dt
    out.backward(g)
    ta, tb = t.clone().requires_grad_(True), cond.clone().requires_grad_(True)
    t_out = torch_pool(ta, tb, scale)
    t_out.backward(g)
    ins = (f64(t), f64(cond), scale)
    ref_dt, ref_dcond = R.view_attention_pool_grad(*ins, f64(g))
    tag = f"{name}/{t_dt}/{cond_dt}".replace("torch.", "")
    assert a.grad.dtype == t_dt and b.grad.dtype == cond_dt
    res = [bar(tag + "/out", out, t_out, R.view_attention_pool(*ins)), bar(tag + "/dt", a.grad, ta.grad, ref_dt),
           bar(tag + "/dcond", b.grad, tb.grad, ref_dcond)]
    return res, out, a.grad, b.grad


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}".replace("torch.", ""))
@pytest.mark.parametrize("name", list(VC.CASES))
def test_output_and_gradients_meet_the_bar(name, pair):
    res, _, _, _ = run(name, *pair)
    settle(res)


def test_inputs_reach_near_one_hot_and_near_uniform_rows():
    """what the cases are for: s spans about +-12, the first rows near uniform and the last near one-hot (checked on the host)"""
    t, cond, _ = VC.inputs("n1000_v4")
    s = VC.scale_of("n1000_v4") * np.einsum("nhc,nvc->nhv", t, cond)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    assert 10 <= np.abs(s).max() <= 25 and p[-50:].max(-1).max() > 0.999 and p[0].max() < 0.27
    t, cond, _ = VC.inputs(VC.TWIN_VIEWS)
    assert np.array_equal(cond[:, 0], cond[:, 1]) and not np.array_equal(cond[:, 0], cond[:, 2])


def test_one_view_returns_the_view_itself_and_no_gradient_for_t():
    V = va()
    name = "n1_v1"
    for N in (1, 37):
        rng = np.random.default_rng(N)
        t = dev(rng.standard_normal((N, 16, 8)) * 9, F32).requires_grad_(True)
        cond = dev(rng.standard_normal((N, 1, 8)), F32).requires_grad_(True)
        g = dev(rng.standard_normal((N, 16, 8)), F32)
        out = V.view_attention_pool(t, cond, VC.scale_of(name))
        out.backward(g)
        assert torch.equal(out, cond.detach().expand(N, 16, 8))
        assert torch.equal(t.grad, torch.zeros_like(t))
        settle([bar(f"one-view/{N}/dcond", cond.grad, g.sum(1, keepdim=True), f64(g).sum(1, keepdims=True))])


def _forward_backward(name, t_dt, cond_dt, cond_view=None):
    V = va()
    t64, cond64, g64 = VC.inputs(name)
    t = dev(t64, t_dt).requires_grad_(True)
    cond = (cond_view if cond_view is not None else dev(cond64, cond_dt)).detach().requires_grad_(True)
    out = V.view_attention_pool(t, cond, VC.scale_of(name))
    out.backward(dev(g64, t_dt))
    return out.detach(), t.grad, cond.grad


def test_two_calls_are_bitwise_equal():
    for name, pair in (("n1000_v4", (F32, F32)), ("h20", (BF16, F32)), ("h32_c16_v16", (F32, F32)), ("h5_c4_v7", (F16, F16))):
        first, second = _forward_backward(name, *pair), _forward_backward(name, *pair)
        for a, b in zip(first, second):
            assert torch.equal(a, b), name


def test_strided_view_of_cond_gives_the_bits_of_its_contiguous_copy():
    name = "n257_v3"
    N, H, Ck, nv = VC.CASES[name]
    _, cond64, _ = VC.inputs(name)
    stacked = dev(cond64, F32).permute(1, 2, 0).contiguous()               # (V, Ck, N), as the sampler stacks the views
    view = torch.einsum("lcb->blc", stacked)
    assert view.stride() == (1, Ck * N, N) and not view.is_contiguous()
    got, want = _forward_backward(name, F32, F32, view), _forward_backward(name, F32, F32, view.contiguous())
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert got[2].shape == (N, nv, Ck)


def test_runs_under_vjp_and_under_no_grad():
    V = va()
    name = "h20"
    scale = VC.scale_of(name)
    t64, cond64, g64 = VC.inputs(name)
    t, cond, g = dev(t64, F32), dev(cond64, F32), dev(g64, F32)
    out, (dt, dcond) = torch.autograd.functional.vjp(lambda a, b: V.view_attention_pool(a, b, scale), (t, cond), g)
    a, b = t.clone().requires_grad_(True), cond.clone().requires_grad_(True)
    o = V.view_attention_pool(a, b, scale)
    o.backward(g)
    assert torch.equal(out, o) and torch.equal(dt, a.grad) and torch.equal(dcond, b.grad)
    with torch.no_grad():
        again = V.view_attention_pool(a, b, scale)
    assert torch.equal(again, o) and not again.requires_grad
    # only one input wants a gradient
    a = t.clone().requires_grad_(True)
    V.view_attention_pool(a, cond, scale).backward(g)
    assert torch.equal(a.grad, dt)


def test_empty_input_returns_an_empty_tensor():
    V = va()
    t = torch.zeros(0, 16, 8, device=DEV, requires_grad=True)
    out = V.view_attention_pool(t, torch.zeros(0, 3, 8, device=DEV), 0.5)
    assert out.shape == (0, 16, 8) and out.dtype == F32
    out.sum().backward()
    assert t.grad.shape == (0, 16, 8)
    assert V.view_attention_pool(torch.zeros(0, 20, device=DEV, dtype=BF16), torch.zeros(0, 7, 4, device=DEV), 0.5, num_heads=5).shape == (0, 5, 4)


def test_no_host_synchronisation():
    V = va()
    name = "n1000_v4"
    t64, cond64, g64 = VC.inputs(name)
    g = dev(g64, F32)
    m = R.make_decoder(80, 12).to(DEV)
    vol, pts = torch.randn(64, 80, device=DEV), torch.randn(64, 3, 8, device=DEV)

    def work():
        t, cond = dev(t64, F32).requires_grad_(True), dev(cond64, F32).requires_grad_(True)
        torch.cuda.synchronize()
        return t, cond

    def calls(t, cond):
        V.view_attention_pool(t, cond, VC.scale_of(name)).backward(g)
        feats, shs = V.decoder_forward_fine(m, vol, pts)
        (feats.sum() + shs.sum()).backward()

    calls(*work())                                   # warm-up: library load, kernel images, the GEMMs
    args = work()
    torch.cuda.synchronize()
    previous = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        raised = False
        try:
            g[0, 0, 0].item()                        # the canary
        except RuntimeError:
            raised = True
        if raised:
            calls(*args)
    finally:
        torch.cuda.set_sync_debug_mode(previous)
    assert raised, "torch.cuda.set_sync_debug_mode('error') did not raise on .item(): the calls above were not checked"
    torch.cuda.synchronize()
    assert torch.isfinite(args[0].grad).all() and torch.isfinite(args[1].grad).all()


# ---- the bound forward ----------------------------------------------------------------------------------------------------

_F64_RUNS = {}


def _bound_inputs(N, nv):
    rng = np.random.default_rng([7, N, nv])
    vol = rng.standard_normal((N, 80)) * 2.0 + 0.3
    pts = rng.standard_normal((N, nv, 8))
    pts[..., 7] *= 3.0                               # (the depth-difference channel is not bounded like the image features)
    return vol, pts, rng.standard_normal((N, 1, 80)), rng.standard_normal((N, 1, 12))


def _run_module(m, fn, vol, pts, g_feat, g_sh, autocast):
    m.zero_grad()
    vol, pts = vol.clone().requires_grad_(True), pts.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=BF16, enabled=autocast):
        feats, shs = fn(vol, pts)
    torch.autograd.backward([feats, shs], [g_feat, g_sh])
    res = {"feats": feats.detach(), "shs": shs.detach(), "d volume_feat": vol.grad, "d point_feats": pts.grad}
    res.update({"d " + n: p.grad.clone() for n, p in m.named_parameters()})
    return res


def _f64_run(N, nv):
    """the torch path of the stand-in in float64 on the CPU, once per shape, on the float32-rounded inputs"""
    if (N, nv) not in _F64_RUNS:
        m = R.make_decoder(80, 12).double()
        ins = [torch.from_numpy(a).float().double() for a in _bound_inputs(N, nv)]
        m.zero_grad()
        vol, pts = ins[0].requires_grad_(True), ins[1].requires_grad_(True)
        feats, shs = R.torch_forward_fine(m, vol, pts)
        torch.autograd.backward([feats, shs], [ins[2], ins[3]])
        res = {"feats": feats.detach(), "shs": shs.detach(), "d volume_feat": vol.grad, "d point_feats": pts.grad}
        res.update({"d " + n: p.grad.clone() for n, p in m.named_parameters()})
        _F64_RUNS[(N, nv)] = {k: v.numpy() for k, v in res.items()}
    return _F64_RUNS[(N, nv)]


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "bf16-autocast"])
@pytest.mark.parametrize("N,nv", [(257, 3), (257, 4), (1000, 3), (1000, 4)])
def test_bound_forward_equals_the_torch_path_of_the_module(N, nv, autocast):
    V = va()
    m = R.make_decoder(80, 12).to(DEV)
    bound = copy.deepcopy(m)
    type(bound).forward_fine = V.decoder_forward_fine            # the binding, on the stand-in's class
    ins = [torch.from_numpy(a).float().to(DEV) for a in _bound_inputs(N, nv)]
    hip = _run_module(bound, bound.forward_fine, *ins, autocast)
    tor = _run_module(m, lambda a, b: R.torch_forward_fine(m, a, b), *ins, autocast)
    ref = _f64_run(N, nv)
    assert hip["feats"].shape == (N, 1, 80) and hip["shs"].shape == (N, 1, 12)
    assert hip["feats"].dtype == hip["shs"].dtype == F32 == tor["feats"].dtype
    assert set(hip) == set(tor) == set(ref) and len(hip) == 4 + len(list(m.parameters()))
    tag = f"bound/{N}/{nv}/{'bf16-autocast' if autocast else 'fp32'}/"
    settle([bar(tag + k, hip[k], tor[k], ref[k]) for k in hip])


def test_single_query_cross_attention_equals_the_module():
    V = va()
    m = R.make_decoder(80, 12).to(DEV)
    vol, pts, _, _ = (torch.from_numpy(a).float().to(DEV) for a in _bound_inputs(257, 3))
    with torch.no_grad():
        got = V.single_query_cross_attention(m.cross_att, vol, pts)
        want = m.cross_att(vol[:, None], pts, pts, need_weights=False)[0][:, 0]
        ref = m.double().cpu().cross_att(vol.double().cpu()[:, None], pts.double().cpu(), pts.double().cpu(), need_weights=False)[0][:, 0]
    settle([bar("single-query/out", got, want, ref.numpy())])


def test_bound_forward_of_a_decoder_held_in_bfloat16_without_autocast():
    """the module's parameters are bf16 and nothing casts for it: the fold and the core still run in fp32, the rest in bf16"""
    V = va()
    m = R.make_decoder(80, 12).to(BF16)
    ref_m = copy.deepcopy(m).double()
    vol64, pts64, _, _ = _bound_inputs(257, 3)
    vol, pts = dev(vol64, BF16), dev(pts64, BF16)
    m = m.to(DEV)
    with torch.no_grad():
        hip = V.decoder_forward_fine(m, vol, pts)
        tor = R.torch_forward_fine(m, vol, pts)
        ref = R.torch_forward_fine(ref_m, vol.double().cpu(), pts.double().cpu())
    assert hip[0].shape == (257, 1, 80) and hip[1].shape == (257, 1, 12) and hip[0].dtype == hip[1].dtype == F32
    settle([bar("bound/bf16-module/feats", hip[0], tor[0], ref[0].numpy()), bar("bound/bf16-module/shs", hip[1], tor[1], ref[1].numpy())])
