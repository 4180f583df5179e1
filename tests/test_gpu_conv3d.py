"""GPU: the channels-last 3x3x3 convolution (csrc/conv3d.hip through generativedensification_amd.conv3d) against the float64
restatement (tests/conv3d_ref.py) and against F.conv3d on the same GPU in the same compute dtype, and the bound
GroupAttBlock forward with groupattn.CONV_BACKEND = "hip".

Accuracy bar (the one of tests/test_gpu_norm.py, tests/test_gpu_viewattn.py and tests/test_gpu_groupattn.py), for the output and
for every gradient: with e_hip = max|hip - ref64| and e_torch = max|torch - ref64| (ref64 on the inputs as rounded to their
dtypes), e_hip <= 2 e_torch + half an ulp of the result dtype at max|ref64|.  `torch` casts the parameters to the compute
dtype as autocast would.  Every pair is printed before it is asserted.  The tests never synchronise inside a checked region,
provoke no out-of-range access and look at no kernel's code."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv3d_cases as CC
import conv3d_ref as R
import groupattn_ref as GR
from norm_ref import half_ulp, to_dtype

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
PAIRS = [(F32, F32), (BF16, BF16), (F16, F16), (BF16, F32)]       # (x and grad_out, weight and bias); the last is autocast's
CL = torch.channels_last_3d


def c3():
    from generativedensification_amd import conv3d as C3

    return C3


def dev(a, dtype):
    return to_dtype(a, dtype).to(DEV)


def cl(t):
    """t with the strides of a dense (B, D, H, W, C) tensor (`.contiguous(memory_format=...)` may leave a size-1 axis as it is)"""
    return t.permute(0, 2, 3, 4, 1).clone(memory_format=torch.contiguous_format).permute(0, 4, 1, 2, 3)


def f64(t):
    return t.detach().double().cpu().numpy()


def bar(what, hip, tor, ref64, e_torch_floor=0.0):
    """prints the pair, then hands it to settle; e_torch_floor: the error of another torch run of the same composition"""
    assert hip.dtype == tor.dtype and hip.shape == tor.shape == ref64.shape, (what, hip.dtype, tor.dtype, hip.shape, tor.shape, ref64.shape)
    e_hip = float(np.abs(f64(hip) - ref64).max()) if ref64.size else 0.0
    e_torch = max(float(np.abs(f64(tor) - ref64).max()) if ref64.size else 0.0, e_torch_floor)
    slack = half_ulp(hip.dtype, float(np.abs(ref64).max()) if ref64.size else 0.0)
    print(f"conv3d-bar {what}: e_hip={e_hip:.3e} e_torch={e_torch:.3e} half_ulp={slack:.3e}")
    assert np.isfinite(f64(hip)).all(), what
    return what, e_hip, e_torch, slack


def settle(results):
    bad = [(w, eh, et, s) for w, eh, et, s in results if not eh <= 2 * et + s]
    assert not bad, bad


def is_dense_channels_last(t):
    return t.permute(0, 2, 3, 4, 1).is_contiguous() and (t.numel() == 0 or t.permute(0, 2, 3, 4, 1).stride() == torch.empty(
        t.permute(0, 2, 3, 4, 1).shape).stride())


# ---- accuracy -----------------------------------------------------------------------------------------------------------------

_REFS = {}


def ref64(name, x, w, b, g, with_bias, add_input):
    """the float64 restatement on the inputs as rounded, once per (case, dtypes, variant)"""
    key = (name, x.dtype, w.dtype, with_bias, add_input)
    if key not in _REFS:
        ins = f64(x), f64(w)
        _REFS[key] = (R.conv3d(*ins, f64(b) if with_bias else None, add_input), *R.conv3d_grad(*ins, f64(g), add_input))
    return _REFS[key]


def run_case(name, x_dt, p_dt, with_bias, add_input, layout="cl"):
    """one forward and backward of the HIP path and of torch's; (results for the bar, the HIP tensors)"""
    C3 = c3()
    B, cin, cout, D, H, W = CC.CASES[name]
    x64, w64, b64, g64 = CC.inputs(name)
    x, w, b, g = dev(x64, x_dt), dev(w64, p_dt), dev(b64, p_dt), dev(g64, x_dt)
    x, g = cl(x), cl(g)

    def leaves():
        return (x.clone(memory_format=torch.preserve_format).requires_grad_(True), w.clone().requires_grad_(True),
                b.clone().requires_grad_(True) if with_bias else None)

    a, hw, hb = leaves()
    src = a
    if layout == "ncdhw":
        src = a.contiguous()
    elif layout == "slice":
        wide = torch.full((B, cin + 16, D, H, W), float("nan"), dtype=x_dt, device=DEV).contiguous(memory_format=CL)
        wide[:, 8:8 + cin] = a
        src = wide[:, 8:8 + cin]
    out = C3.conv3d(src, hw, hb, add_input=add_input)
    assert out.shape == (B, cout, D, H, W) and out.dtype == x_dt and is_dense_channels_last(out)
    out.backward(g)
    ta, tw, tb = leaves()
    t_out = F.conv3d(ta, tw.to(x_dt), tb.to(x_dt) if with_bias else None, padding=1)
    if add_input:
        t_out = t_out + ta
    t_out.backward(g)
    r_out, r_dx, r_dw, r_db = ref64(name, x, w, b, g, with_bias, add_input)
    tag = f"{name}/{x_dt}/{p_dt}/{'bias' if with_bias else 'nobias'}/{'add' if add_input else 'plain'}".replace("torch.", "")
    assert a.grad.dtype == x_dt and hw.grad.dtype == p_dt and hw.grad.shape == w.shape
    res = [bar(tag + "/out", out, t_out, r_out), bar(tag + "/dx", a.grad, ta.grad, r_dx), bar(tag + "/dw", hw.grad, tw.grad, r_dw)]
    hip = [out.detach(), a.grad, hw.grad]
    if with_bias:
        assert hb.grad.dtype == p_dt
        res.append(bar(tag + "/db", hb.grad, tb.grad, r_db))
        hip.append(hb.grad)
    return res, hip


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}".replace("torch.", ""))
@pytest.mark.parametrize("name", list(CC.CASES))
def test_output_and_gradients_meet_the_bar(name, pair):
    B, cin, cout = CC.CASES[name][:3]
    res = []
    for with_bias in (False, True):
        for add_input in (False, True) if cin == cout else (False,):
            res += run_case(name, *pair, with_bias, add_input)[0]
    settle(res)


# ---- exact checks ---------------------------------------------------------------------------------------------------------------

TAP = (0, 1, 2)                                 # an asymmetric tap: offset (-1, 0, +1)


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["float32", "bfloat16", "float16"])
def test_identity_at_one_tap_shifts_with_zero_fill_and_its_gradient_shifts_back(dtype):
    C3 = c3()
    B, C, D, H, W = 2, 16, 3, 5, 9                  # two bricks along D... W, none of them full
    rng = np.random.default_rng(3)
    x = cl(dev(rng.standard_normal((B, C, D, H, W)) + 0.5, dtype)).requires_grad_(True)
    g = cl(dev(rng.standard_normal((B, C, D, H, W)) - 0.5, dtype))
    w = torch.zeros(C, C, 3, 3, 3, dtype=dtype, device=DEV)
    w[torch.arange(C), torch.arange(C), TAP[0], TAP[1], TAP[2]] = 1
    off = tuple(t - 1 for t in TAP)
    out = C3.conv3d(x, w)
    out.backward(g)
    want = torch.from_numpy(R.shifted(f64(x), off)).to(dtype).to(DEV)
    want_dx = torch.from_numpy(R.shifted(f64(g), tuple(-o for o in off))).to(dtype).to(DEV)
    assert want.abs().sum() > 0 and not torch.equal(want, x.detach())
    assert torch.equal(out, want)
    assert torch.equal(x.grad, want_dx)


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["float32", "bfloat16", "float16"])
def test_zero_weight_with_add_input_returns_x(dtype):
    C3 = c3()
    x = cl(dev(np.random.default_rng(4).standard_normal((2, 24, 5, 4, 9)) * 3, dtype))
    out = C3.conv3d(x, torch.zeros(24, 24, 3, 3, 3, dtype=dtype, device=DEV), add_input=True)
    assert torch.equal(out, x) and out.data_ptr() != x.data_ptr()


# ---- layouts, determinism, autograd, synchronisation ------------------------------------------------------------------------------

def test_layouts_give_the_bits_of_the_dense_channels_last_input_and_that_one_is_not_copied():
    C3 = c3()
    for name, pair in (("odd", (F32, F32)), ("seam", (BF16, F32))):
        dense = run_case(name, *pair, True, False)[1]
        for layout in ("ncdhw", "slice"):
            for a, b in zip(dense, run_case(name, *pair, True, False, layout=layout)[1]):
                assert torch.equal(a, b), (name, layout)
    x = cl(torch.randn(2, 8, 3, 4, 5, device=DEV))
    assert C3._rows(x).data_ptr() == x.data_ptr() and C3._rows(x.contiguous()).data_ptr() != x.data_ptr()
    # a size-1 axis leaves the strides ambiguous: whichever way torch wrote them, a dense volume is read in place
    for shape in ((1, 8, 1, 1, 1), (1, 8, 1, 1, 5), (1, 8, 4, 4, 4)):
        v = cl(torch.randn(shape, device=DEV))
        for t in (v, v.contiguous(memory_format=CL)) + ((v.contiguous(),) if shape[2:] == (1, 1, 1) else ()):
            assert C3._rows(t).data_ptr() == t.data_ptr(), (shape, t.stride())
    odd_base = torch.randn(8 * 27 + 1, device=DEV)[1:].view(1, 27, 8).permute(0, 2, 1).view(1, 8, 3, 3, 3)      # 4 bytes off alignment
    assert odd_base.data_ptr() % 16 and C3._rows(odd_base).data_ptr() % 16 == 0


def test_two_calls_are_bitwise_equal():
    for name, pair, add in (("odd", (F32, F32), False), ("ref_width", (BF16, F32), True), ("brick_plus", (F16, F16), True), ("c40", (F32, F32), True)):
        first, second = run_case(name, *pair, True, add)[1], run_case(name, *pair, True, add)[1]
        assert len(first) == 4
        for a, b in zip(first, second):
            assert torch.equal(a, b), name


def test_runs_under_no_grad_and_vjp_and_a_frozen_weight_launches_no_weight_gradient(monkeypatch):
    C3 = c3()
    from generativedensification_amd import _lib as L

    x64, w64, b64, g64 = CC.inputs("odd")
    x, w, b, g = cl(dev(x64, F32)), dev(w64, F32), dev(b64, F32), cl(dev(g64, F32))
    leaves = [t.clone(memory_format=torch.preserve_format).requires_grad_(True) for t in (x, w, b)]
    out = C3.conv3d(*leaves)
    out.backward(g)
    got, grads = torch.autograd.functional.vjp(lambda a, ww, bb: C3.conv3d(a, ww, bb), (x, w, b), g)
    assert torch.equal(got, out) and all(torch.equal(a, t.grad) for a, t in zip(grads, leaves))
    with torch.no_grad():
        again = C3.conv3d(*leaves)
    assert torch.equal(again, out) and not again.requires_grad

    def boom(*args):
        raise AssertionError("a weight gradient was launched for a frozen weight")

    monkeypatch.setattr(L.load(), "gdr_conv3d_grad_weight", boom)
    a = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
    frozen, bias = w.clone(), b.clone().requires_grad_(True)
    C3.conv3d(a, frozen, bias).backward(g)
    assert frozen.grad is None and torch.equal(a.grad, leaves[0].grad) and torch.equal(bias.grad, leaves[2].grad)
    module = torch.nn.Conv3d(16, 24, 3, padding=1).to(DEV).requires_grad_(False)
    a2 = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
    C3.conv3d_of(module, a2).sum().backward()
    assert module.weight.grad is None and module.bias.grad is None and a2.grad is not None


def test_no_host_synchronisation():
    C3 = c3()
    x64, w64, b64, g64 = CC.inputs("c40")

    def work():
        args = [cl(dev(x64, BF16)).requires_grad_(True), dev(w64, F32).requires_grad_(True), dev(b64, F32).requires_grad_(True), cl(dev(g64, BF16))]
        torch.cuda.synchronize()
        return args

    def calls(x, w, b, g):
        C3.conv3d(x, w, b, add_input=True).backward(g)
        C3.conv3d(x.detach().float().contiguous(), w, None).sum().backward()        # a copied layout, fp32, no bias

    calls(*work())                                   # warm-up: library load, kernel images
    args = work()
    previous = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        raised = False
        try:
            args[3][0, 0, 0, 0, 0].item()            # the canary
        except RuntimeError:
            raised = True
        if raised:
            calls(*args)
    finally:
        torch.cuda.set_sync_debug_mode(previous)
    assert raised, "torch.cuda.set_sync_debug_mode('error') did not raise on .item(): the calls above were not checked"
    torch.cuda.synchronize()
    assert all(torch.isfinite(t.grad).all() for t in args[:3])


def test_autocast_casts_a_float32_input_and_keeps_float32_parameter_gradients():
    C3 = c3()
    x64, w64, b64, g64 = CC.inputs("c40")
    x, w, b = (t.requires_grad_(True) for t in (cl(dev(x64, F32)), dev(w64, F32), dev(b64, F32)))
    with torch.autocast("cuda", dtype=BF16):
        out = C3.conv3d(x, w, b, add_input=True)
        t_out = F.conv3d(x, w, b, padding=1)
    assert out.dtype == t_out.dtype == BF16 and is_dense_channels_last(out)
    out.backward(cl(dev(g64, BF16)))
    assert x.grad.dtype == w.grad.dtype == b.grad.dtype == F32
    # the same bits as the call on the input cast by hand: the parameters were rounded by the pack kernel, not by torch
    a = x.detach().to(BF16).requires_grad_(True)
    assert torch.equal(C3.conv3d(a, w.detach(), b.detach(), add_input=True), out)


def test_empty_inputs_return_empty_tensors(monkeypatch):
    C3 = c3()
    from generativedensification_amd import _lib as L

    def no_load():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(L, "load", no_load)
    w = torch.ones(16, 8, 3, 3, 3, device=DEV, requires_grad=True)
    b = torch.ones(16, device=DEV, requires_grad=True)
    for shape in ((0, 8, 2, 2, 2), (2, 8, 0, 3, 3), (1, 8, 2, 2, 0)):
        x = torch.zeros(shape, device=DEV, dtype=BF16, requires_grad=True)
        out = C3.conv3d(x, w, b)
        assert out.shape == (shape[0], 16) + shape[2:] and out.dtype == BF16
        out.sum().backward()
        assert x.grad.shape == x.shape and torch.equal(w.grad, torch.zeros_like(w)) and torch.equal(b.grad, torch.zeros_like(b))


# ---- the bound block ------------------------------------------------------------------------------------------------------------

CFG = (32, 4, 24, 4, 2, 3, 2)                   # (C, heads, cond width, D, bs, cond tokens, B): C = 32, D = 4, bs = 2
_F64_RUN = {}


def _bound_inputs():
    C, heads, cw, D, bs, Lk, B = CFG
    rng = np.random.default_rng([17, *CFG])
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


def _f64_run():
    """the torch path of the stand-in in float64 on the CPU, once, on the float32-rounded inputs"""
    if not _F64_RUN:
        C, heads, cw, D, bs, Lk, B = CFG
        m = GR.make_group_att_block(C, cw, heads).double()
        x, cond, g = (torch.from_numpy(a).float().double() for a in _bound_inputs())
        x, cond = x.requires_grad_(True), cond.requires_grad_(True)
        out = GR.torch_forward(m, x, cond, D // bs, bs)
        out.backward(g)
        res = {"out": out.detach(), "d x": x.grad, "d cond": cond.grad}
        res.update({"d " + n: p.grad.clone() for n, p in m.named_parameters()})
        _F64_RUN.update({k: v.numpy() for k, v in res.items()})
    return _F64_RUN


def _stand_ins():
    from generativedensification_amd import groupattn as G

    C, heads, cw, D, bs, Lk, B = CFG
    m = GR.make_group_att_block(C, cw, heads).to(DEV)
    bound = copy.deepcopy(m)
    type(bound).forward = G.group_att_block_forward                  # the binding, on the stand-in's class
    x, cond, g = (torch.from_numpy(a).float().to(DEV) for a in _bound_inputs())
    return G, m, bound, x, cond, g


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "bf16-autocast"])
def test_bound_block_with_the_hip_backend_meets_the_bar(autocast):
    G, m, bound, x, cond, g = _stand_ins()
    C, heads, cw, D, bs, Lk, B = CFG
    saved = G.CONV_BACKEND
    try:
        G.CONV_BACKEND = "hip"
        hip = _run_block(bound, lambda a, b: bound(a, b, D // bs, bs), x, cond, g, autocast)
    finally:
        G.CONV_BACKEND = saved
    tor = _run_block(m, lambda a, b: GR.torch_forward(m, a, b, D // bs, bs), x, cond, g, autocast)
    ref = _f64_run()
    assert hip["out"].shape == x.shape and hip["out"].dtype == tor["out"].dtype == (BF16 if autocast else F32)
    assert is_dense_channels_last(hip["out"])
    assert set(hip) == set(tor) == set(ref) and len(hip) == 3 + 15 == 3 + len(list(m.parameters()))
    floors = dict.fromkeys(hip, 0.0)
    if not autocast:
        # torch's convolution picks its algorithm by layout: its error is the larger of those with NCDHW and channels-last input
        other = _run_block(m, lambda a, b: GR.torch_forward(m, a, b, D // bs, bs, conv_channels_last=True), cl(x), cond, cl(g), False)
        floors = {k: float(np.abs(f64(other[k]) - ref[k]).max()) for k in hip}
    tag = f"bound-hip/{'bf16-autocast' if autocast else 'fp32'}/"
    settle([bar(tag + k, hip[k], tor[k], ref[k], floors[k]) for k in hip])


def _parent_forward(self, x, cond, group_axis, block_size):
    """group_att_block_forward as it stood before the switch: the same calls, the module's own convolution on an NCDHW copy"""
    from generativedensification_amd import groupattn as G

    cast = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else None
    patches, normed = G.patchify_layer_norm(x, block_size, self.norm1.weight, self.norm1.bias, self.norm1.eps, out_dtype=cast,
                                            patches_dtype=cast)
    patches = patches + G.grouped_cross_attention(self.cross_attn, normed, cond)
    patches = patches + self.mlp(self.norm2(patches))
    vol = G.layer_norm_unpatchify(patches, x.shape, block_size, self.norm3.weight, self.norm3.bias, self.norm3.eps, out_dtype=cast)
    return vol + self.cnn(vol.contiguous())


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "bf16-autocast"])
def test_bound_block_with_the_torch_backend_equals_the_parents_path_bit_for_bit(autocast):
    G, m, bound, x, cond, g = _stand_ins()
    C, heads, cw, D, bs, Lk, B = CFG
    assert G.CONV_BACKEND == "torch"
    now = _run_block(bound, lambda a, b: bound(a, b, D // bs, bs), x, cond, g, autocast)
    parent = _run_block(m, lambda a, b: _parent_forward(m, a, b, D // bs, bs), x, cond, g, autocast)
    assert set(now) == set(parent) and len(now) == 18
    for k in now:
        assert now[k].dtype == parent[k].dtype and now[k].stride() == parent[k].stride() and torch.equal(now[k], parent[k]), k
