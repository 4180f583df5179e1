"""GPU: the group cross attention and the two permuting LayerNorms (csrc/groupattn.hip through
generativedensification_amd.groupattn) against the float64 restatements (tests/groupattn_ref.py, tests/norm_ref.py) and
against the torch compositions on the same GPU in the same dtypes.

Accuracy bar (the one of tests/test_gpu_norm.py and tests/test_gpu_viewattn.py), for every output and gradient: with
e_hip = max|hip - ref64| and e_torch = max|torch - ref64| (ref64 on the inputs as rounded to their dtypes),
e_hip <= 2 e_torch + half an ulp of the result dtype at max|ref64|.  The factor 2 is for another summation order and one
differently rounded exponential or reciprocal square root; nothing else may differ.  Every pair is printed before it is
asserted.  The torch composition of a mixed pair runs in the promotion of the dtypes and its result is rounded to q's dtype,
which is what the HIP path returns."""
import copy
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import groupattn_cases as GC
import groupattn_ref as R
from norm_ref import _layer_norm, _layer_norm_grad, half_ulp, to_dtype

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
PAIRS = [(F32, F32), (BF16, BF16), (F16, F16), (BF16, F32)]       # (q and grad_out, k and v)
CL = torch.channels_last_3d


def ga():
    from generativedensification_amd import groupattn as G

    return G


def dev(a, dtype):
    return to_dtype(a, dtype).to(DEV)


def f64(t):
    return t.detach().double().cpu().numpy()


def bar(what, hip, tor, ref64, e_torch_floor=0.0):
    """prints the pair, then hands it to settle; e_torch_floor: the error of another torch run of the same composition"""
    assert hip.dtype == tor.dtype and hip.shape == tor.shape == ref64.shape, (what, hip.dtype, tor.dtype, hip.shape, tor.shape, ref64.shape)
    e_hip = float(np.abs(f64(hip) - ref64).max()) if ref64.size else 0.0
    e_torch = max(float(np.abs(f64(tor) - ref64).max()) if ref64.size else 0.0, e_torch_floor)
    slack = half_ulp(hip.dtype, float(np.abs(ref64).max()) if ref64.size else 0.0)
    print(f"groupattn-bar {what}: e_hip={e_hip:.3e} e_torch={e_torch:.3e} half_ulp={slack:.3e}")
    assert np.isfinite(f64(hip)).all(), what
    return what, e_hip, e_torch, slack


def settle(results):
    bad = [(w, eh, et, s) for w, eh, et, s in results if not eh <= 2 * et + s]
    assert not bad, bad


# ---- the core -------------------------------------------------------------------------------------------------------------

def torch_core(q, k, v, scale, H):
    wide = torch.promote_types(q.dtype, k.dtype)
    return R.group_cross_attention_torch(q.to(wide), k.to(wide), v.to(wide), scale, H).to(q.dtype)


def run_core(name, q_dt, kv_dt):
    G = ga()
    M, Lq, Lk, H, Dh = GC.CASES[name]
    E, scale = H * Dh, GC.scale_of(name)
    q64, k64, v64, g64 = GC.inputs(name)
    q, k, v, g = dev(q64, q_dt), dev(k64, kv_dt), dev(v64, kv_dt), dev(g64, q_dt)
    a = q.clone().requires_grad_(True)
    if name == GC.STRIDED:
        kv = torch.cat([k, v], dim=-1).requires_grad_(True)            # (M, Lk, 2E): what one product with cat(Wk, Wv) returns
        kk, vv = kv[..., :E], kv[..., E:]
        buf = torch.full((M, Lq, E + 24), float("nan"), dtype=q_dt, device=DEV)   # (the padding is never read)
        buf[..., :E] = a
        rows = buf[..., :E]
        for t in (kk, vv, rows):                                       # read through their strides: no copy is made
            assert G._rows(t)[0] is t and G._rows(t)[1] == t.stride(1) > E
        out = G.group_cross_attention(rows, kk, vv, scale, H)
    else:
        b, c = k.clone().requires_grad_(True), v.clone().requires_grad_(True)
        out = G.group_cross_attention(a, b, c, scale, H)
    assert out.shape == (M, Lq, E) and out.dtype == q_dt and out.is_contiguous()
    out.backward(g)
    if name == GC.STRIDED:
        dk, dv = kv.grad[..., :E], kv.grad[..., E:]
    else:
        dk, dv = b.grad, c.grad
    ta, tb, tc = (t.clone().requires_grad_(True) for t in (q, k, v))
    t_out = torch_core(ta, tb, tc, scale, H)
    t_out.backward(g)
    ins = (f64(q), f64(k), f64(v), scale, H)
    ref_dq, ref_dk, ref_dv = R.group_cross_attention_grad(*ins, f64(g))
    tag = f"{name}/{q_dt}/{kv_dt}".replace("torch.", "")
    assert a.grad.dtype == q_dt and dk.dtype == dv.dtype == kv_dt
    res = [bar(tag + "/out", out, t_out, R.group_cross_attention(*ins)), bar(tag + "/dq", a.grad, ta.grad, ref_dq),
           bar(tag + "/dk", dk, tb.grad, ref_dk), bar(tag + "/dv", dv, tc.grad, ref_dv)]
    return res, (out.detach(), a.grad, dk.clone(), dv.clone())


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}".replace("torch.", ""))
@pytest.mark.parametrize("name", list(GC.CASES))
def test_core_output_and_gradients_meet_the_bar(name, pair):
    res, _ = run_core(name, *pair)
    settle(res)


def test_one_key_returns_the_value_itself_and_no_gradient_for_q():
    G = ga()
    for M, Lq, H, Dh in ((1, 1, 1, 8), (37, 5, 16, 8)):
        rng = np.random.default_rng(M)
        q = dev(rng.standard_normal((M, Lq, H * Dh)) * 9, F32).requires_grad_(True)
        k = dev(rng.standard_normal((M, 1, H * Dh)), F32).requires_grad_(True)
        v = dev(rng.standard_normal((M, 1, H * Dh)), F32).requires_grad_(True)
        g = dev(rng.standard_normal((M, Lq, H * Dh)), F32)
        out = G.group_cross_attention(q, k, v, Dh ** -0.5, H)
        out.backward(g)
        assert torch.equal(out, v.detach().expand(M, Lq, H * Dh))
        assert torch.equal(q.grad, torch.zeros_like(q)) and torch.equal(k.grad, torch.zeros_like(k))
        settle([bar(f"one-key/{M}/dv", v.grad, g.sum(1, keepdim=True), f64(g).sum(1, keepdims=True))])


def test_core_runs_under_vjp_and_under_no_grad():
    G = ga()
    name = "odd"
    M, Lq, Lk, H, Dh = GC.CASES[name]
    scale = GC.scale_of(name)
    q, k, v, g = (dev(a, F32) for a in GC.inputs(name))
    out, grads = torch.autograd.functional.vjp(lambda a, b, c: G.group_cross_attention(a, b, c, scale, H), (q, k, v), g)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    o = G.group_cross_attention(*leaves, scale, H)
    o.backward(g)
    assert torch.equal(out, o) and all(torch.equal(a, b.grad) for a, b in zip(grads, leaves))
    with torch.no_grad():
        again = G.group_cross_attention(*leaves, scale, H)
    assert torch.equal(again, o) and not again.requires_grad
    a = q.clone().requires_grad_(True)                               # only one input wants a gradient
    G.group_cross_attention(a, k, v, scale, H).backward(g)
    assert torch.equal(a.grad, grads[0])


def test_empty_inputs_return_empty_tensors():
    G = ga()
    q = torch.zeros(0, 8, 64, device=DEV, requires_grad=True)
    out = G.group_cross_attention(q, torch.zeros(0, 4, 64, device=DEV), torch.zeros(0, 4, 64, device=DEV, dtype=BF16), 0.25, 4)
    assert out.shape == (0, 8, 64) and out.dtype == F32
    out.sum().backward()
    assert q.grad.shape == (0, 8, 64)
    w = torch.ones(8, device=DEV, requires_grad=True)
    vol = torch.zeros(0, 8, 4, 4, 4, device=DEV, requires_grad=True)
    patches, normed = G.patchify_layer_norm(vol, 2, w, None)
    assert patches.shape == normed.shape == (0, 8, 8)
    back = G.layer_norm_unpatchify(normed, vol.shape, 2, w, None)
    assert back.shape == (0, 8, 4, 4, 4)
    (back.sum() + patches.sum()).backward()
    assert vol.grad.shape == vol.shape and torch.equal(w.grad, torch.zeros_like(w))


# ---- the two norms ----------------------------------------------------------------------------------------------------------

def run_norms(shape, dtype, affine, channels_last=False):
    """both norms forward and backward; (results for the bar, every HIP tensor for bitwise comparisons)"""
    G = ga()
    B, C, D, H, W, bs = shape
    vol64, w64, b64, gp64, gn64, gv64 = GC.norm_inputs(shape)
    eps = 1e-5
    vol, gp, gn, gv = dev(vol64, dtype), dev(gp64, dtype), dev(gn64, dtype), dev(gv64, dtype)
    if channels_last:
        vol = vol.contiguous(memory_format=CL)
    params = [dev(w64, dtype), dev(b64, dtype)] if affine else [None, None]
    tag = f"norm/{shape}/{dtype}/{'affine' if affine else 'plain'}".replace("torch.", "")

    def leaves():
        return vol.clone(memory_format=torch.preserve_format).requires_grad_(True), [p.clone().requires_grad_(True) if affine else None for p in params]

    # patchify + norm
    a, (w, b) = leaves()
    patches, normed = G.patchify_layer_norm(a, bs, w, b, eps)
    torch.autograd.backward([patches, normed], [gp, gn])
    ta, (tw, tb) = leaves()
    t_patches = R.patchify_torch(ta, bs)
    t_normed = F.layer_norm(t_patches, (C,), tw, tb, eps)
    torch.autograd.backward([t_patches, t_normed], [gp, gn])
    assert patches.dtype == dtype and torch.equal(patches, t_patches)          # the same bits as the torch permutation
    wr, br = (f64(params[0]), f64(params[1])) if affine else (1.0, 0.0)
    p64 = R.patchify(f64(vol), bs)
    xh, rstd = _layer_norm(p64, eps)
    dp64 = f64(gp) + _layer_norm_grad(f64(gn) * wr, xh, rstd)
    res = [bar(tag + "/patchify/normed", normed, t_normed, xh * wr + br),
           bar(tag + "/patchify/dvol", a.grad, ta.grad, R.unpatchify(dp64, vol.shape, bs))]
    hip = [patches.detach(), normed.detach(), a.grad]
    if affine:
        res += [bar(tag + "/patchify/dweight", w.grad, tw.grad, (f64(gn) * xh).sum((0, 1))),
                bar(tag + "/patchify/dbias", b.grad, tb.grad, f64(gn).sum((0, 1)))]
        hip += [w.grad, b.grad]

    # norm + unpatchify, on the patches as input
    src = patches.detach()
    a2, (w, b) = src.clone().requires_grad_(True), leaves()[1]
    out = G.layer_norm_unpatchify(a2, vol.shape, bs, w, b, eps)
    assert out.shape == vol.shape and out.dtype == dtype and out.permute(0, 2, 3, 4, 1).is_contiguous()
    out.backward(gv)
    ta2, (tw, tb) = src.clone().requires_grad_(True), leaves()[1]
    t_out = R.unpatchify_torch(F.layer_norm(ta2, (C,), tw, tb, eps), vol.shape, bs)
    t_out.backward(gv)
    gv_p = R.patchify(f64(gv), bs)
    res += [bar(tag + "/unpatchify/vol", out, t_out, R.unpatchify(xh * wr + br, vol.shape, bs)),
            bar(tag + "/unpatchify/dpatches", a2.grad, ta2.grad, _layer_norm_grad(gv_p * wr, xh, rstd))]
    hip += [out.detach(), a2.grad]
    if affine:
        res += [bar(tag + "/unpatchify/dweight", w.grad, tw.grad, (gv_p * xh).sum((0, 1))),
                bar(tag + "/unpatchify/dbias", b.grad, tb.grad, gv_p.sum((0, 1)))]
        hip += [w.grad, b.grad]
    return res, hip


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["float32", "bfloat16"])
@pytest.mark.parametrize("shape", GC.NORM_SHAPES, ids=str)
def test_norms_meet_the_bar_and_patches_are_the_bits_of_the_torch_permutation(shape, dtype, affine):
    res, _ = run_norms(shape, dtype, affine)
    settle(res)


def test_a_volume_that_is_not_channels_last_gives_the_bits_of_its_channels_last_copy():
    shape = GC.NORM_SHAPES[4]
    _, plain = run_norms(shape, F32, True)
    _, cl = run_norms(shape, F32, True, channels_last=True)
    for a, b in zip(plain, cl):
        assert torch.equal(a, b)


def test_norm_result_dtype_follows_out_dtype_and_autocast():
    G = ga()
    vol = torch.randn(1, 16, 2, 2, 2, device=DEV)
    w = torch.ones(16, device=DEV)
    _, normed = G.patchify_layer_norm(vol.to(BF16), 2, w, None)
    assert normed.dtype == BF16
    patches, normed = G.patchify_layer_norm(vol, 2, w, None, out_dtype=BF16)
    assert patches.dtype == F32 and normed.dtype == BF16
    assert torch.equal(normed, G.patchify_layer_norm(vol, 2, w, None)[1].to(BF16))       # float32 arithmetic, one rounding
    rounded, of_rounded = G.patchify_layer_norm(vol, 2, w, None, patches_dtype=BF16)
    assert rounded.dtype == BF16 and of_rounded.dtype == F32 and torch.equal(rounded, patches.to(BF16))
    assert torch.equal(of_rounded, G.patchify_layer_norm(vol.to(BF16).float(), 2, w, None)[1])          # the norm of the patches as stored
    with torch.autocast("cuda", dtype=BF16):
        assert G.patchify_layer_norm(vol.to(BF16), 2, w, None)[1].dtype == F32
        assert G.layer_norm_unpatchify(patches.to(BF16), vol.shape, 2, w, None).dtype == F32


def test_two_calls_are_bitwise_equal():
    for name, pair in (("m257", (F32, F32)), ("h20", (BF16, F32)), ("g8", (F32, F32)), ("odd_tail", (F16, F16)), ("strided", (BF16, BF16))):
        first, second = run_core(name, *pair)[1], run_core(name, *pair)[1]
        for a, b in zip(first, second):
            assert torch.equal(a, b), name
    for shape, dtype in ((GC.NORM_SHAPES[0], F32), (GC.NORM_SHAPES[1], BF16), (GC.NORM_SHAPES[3], F32)):
        first, second = run_norms(shape, dtype, True)[1], run_norms(shape, dtype, True)[1]
        assert len(first) == 9
        for a, b in zip(first, second):
            assert torch.equal(a, b), shape


def test_no_host_synchronisation():
    G = ga()
    name = "ref"
    M, Lq, Lk, H, Dh = GC.CASES[name]
    q64, k64, v64, g64 = GC.inputs(name)
    g = dev(g64, F32)
    m = R.make_group_att_block(32, 24, 4).to(DEV)
    gv = torch.randn(2, 32, 4, 4, 4, device=DEV)

    def work():
        leaves = [dev(a, F32).requires_grad_(True) for a in (q64, k64, v64)]
        vol, cond = torch.randn(2, 32, 4, 4, 4, device=DEV, requires_grad=True), torch.randn(16, 3, 24, device=DEV, requires_grad=True)
        torch.cuda.synchronize()
        return leaves, vol, cond

    def calls(leaves, vol, cond):
        G.group_cross_attention(*leaves, GC.scale_of(name), H).backward(g)
        patches, normed = G.patchify_layer_norm(vol, 2, m.norm1.weight, m.norm1.bias, m.norm1.eps)
        patches = patches + G.grouped_cross_attention(m.cross_attn, normed, cond)
        G.layer_norm_unpatchify(patches, vol.shape, 2, m.norm3.weight, m.norm3.bias, m.norm3.eps).backward(gv)

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
    assert all(torch.isfinite(t.grad).all() for t in (*args[0], args[1], args[2], m.norm1.weight, m.norm3.bias, m.cross_attn.q_proj_weight))


# ---- the bound forward ----------------------------------------------------------------------------------------------------

# (C, heads, cond width, D, bs, cond tokens, B): eight queries of head width 8 over three keys; one query of head width 16
BOUND = {"c32_bs2": (32, 4, 24, 4, 2, 3, 2), "c64_bs1": (64, 4, 24, 3, 1, 3, 2)}
DETOUR = (32, 4, 24, 5, 5, 3, 1)                     # Lq = 125: outside the core's envelope
_F64_RUNS = {}


def _bound_inputs(cfg):
    C, heads, cw, D, bs, Lk, B = cfg
    rng = np.random.default_rng([11, *cfg])
    G = (D // bs) ** 3
    return rng.standard_normal((B, C, D, D, D)) * 1.5 + 0.2, rng.standard_normal((B * G, Lk, cw)), rng.standard_normal((B, C, D, D, D))


def _run_block(m, fn, x, cond, g, autocast):
    m.zero_grad()
    x, cond = x.clone(memory_format=torch.preserve_format).requires_grad_(True), cond.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=BF16, enabled=autocast):
        out = fn(x, cond)
    out.backward(g)
    res = {"out": out.detach(), "d x": x.grad, "d cond": cond.grad}
    res.update({"d " + n: p.grad.clone() for n, p in m.named_parameters()})
    return res


def _f64_run(cfg):
    """the torch path of the stand-in in float64 on the CPU, once per configuration, on the float32-rounded inputs"""
    if cfg not in _F64_RUNS:
        C, heads, cw, D, bs, Lk, B = cfg
        m = R.make_group_att_block(C, cw, heads).double()
        x, cond, g = (torch.from_numpy(a).float().double() for a in _bound_inputs(cfg))
        x, cond = x.requires_grad_(True), cond.requires_grad_(True)
        out = R.torch_forward(m, x, cond, D // bs, bs)
        out.backward(g)
        res = {"out": out.detach(), "d x": x.grad, "d cond": cond.grad}
        res.update({"d " + n: p.grad.clone() for n, p in m.named_parameters()})
        _F64_RUNS[cfg] = {k: v.numpy() for k, v in res.items()}
    return _F64_RUNS[cfg]


def _bound_against_torch(cfg, autocast, tag):
    G = ga()
    C, heads, cw, D, bs, Lk, B = cfg
    m = R.make_group_att_block(C, cw, heads).to(DEV)
    bound = copy.deepcopy(m)
    type(bound).forward = G.group_att_block_forward                  # the binding, on the stand-in's class
    x, cond, g = (torch.from_numpy(a).float().to(DEV) for a in _bound_inputs(cfg))
    hip = _run_block(bound, lambda a, b: bound(a, b, D // bs, bs), x, cond, g, autocast)
    tor = _run_block(m, lambda a, b: R.torch_forward(m, a, b, D // bs, bs), x, cond, g, autocast)
    ref = _f64_run(cfg)
    # under autocast the reference's einsums round the patches and the volume to the autocast dtype: the result has it
    assert hip["out"].shape == tor["out"].shape == x.shape and hip["out"].dtype == tor["out"].dtype == (BF16 if autocast else F32)
    assert hip["out"].permute(0, 2, 3, 4, 1).is_contiguous()         # channels-last: the next block takes the fast path
    assert set(hip) == set(tor) == set(ref) and len(hip) == 3 + len(list(m.parameters()))
    floors = dict.fromkeys(hip, 0.0)
    if not autocast:
        # the HIP path hands the convolution channels-last tensors, and the convolution's algorithm choice is not ours: the
        # torch path's error is the larger of its errors with NCDHW and with channels-last input
        cl = _run_block(m, lambda a, b: R.torch_forward(m, a, b, D // bs, bs, conv_channels_last=True), x.contiguous(memory_format=CL), cond,
                        g.contiguous(memory_format=CL), False)
        floors = {k: float(np.abs(f64(cl[k]) - ref[k]).max()) for k in hip}
    settle([bar(tag + k, hip[k], tor[k], ref[k], floors[k]) for k in hip])


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "bf16-autocast"])
@pytest.mark.parametrize("name", list(BOUND))
def test_bound_forward_equals_the_torch_path_of_the_module(name, autocast):
    _bound_against_torch(BOUND[name], autocast, f"bound/{name}/{'bf16-autocast' if autocast else 'fp32'}/")


def test_outside_the_envelope_the_core_detours_through_sdpa_and_warns_once(monkeypatch):
    G = ga()
    monkeypatch.setattr(G, "_warned", False)
    assert not G.in_envelope(1, 125, 3, 4, 8)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        _bound_against_torch(DETOUR, False, "detour/fp32/")
        _bound_against_torch(DETOUR, True, "detour/bf16-autocast/")
    said = [w for w in caught if issubclass(w.category, RuntimeWarning) and "envelope" in str(w.message)]
    assert len(said) == 1 and "scaled_dot_product_attention" in str(said[0].message)


def test_grouped_cross_attention_equals_the_module():
    G = ga()
    for bias in (False, True):
        m = GC.make_mha(64, 4, 24, bias, False).float().to(DEV)
        x64, cond64 = GC.mha_inputs(64, 4, 24, 8, 4, M=19)
        x, cond = dev(x64, F32), dev(cond64, F32)
        with torch.no_grad():
            got = G.grouped_cross_attention(m, x, cond)
            want = m(x, cond, cond, need_weights=False)[0]
            md = copy.deepcopy(m).double().cpu()
            ref = md(x.double().cpu(), cond.double().cpu(), cond.double().cpu(), need_weights=False)[0]
        settle([bar(f"grouped/bias={bias}/out", got, want, ref.numpy())])
