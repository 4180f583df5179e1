"""GPU: the fused coarse Gaussian head (csrc/coarsehead.hip through generativedensification_amd.coarsehead) against the float64
restatement (tests/coarsehead_ref.py) and against the reference's lines on the same GPU in the same compute dtype.

Accuracy bar (the one of tests/test_gpu_conv3d.py), for every output and every gradient: with e_hip = max|hip - ref64| and
e_torch = max|torch - ref64| (ref64 on the inputs as rounded to their dtypes), e_hip <= 2 e_torch + half an ulp of the result
dtype at max|ref64|.  `torch` casts the parameters to the compute dtype as autocast would.  Every pair is printed before it is
asserted.  The ReLU gates of every case are settled by tests/coarsehead_cases.py, so the three computations gate alike.  The
tests never synchronise inside a checked region, provoke no out-of-range access and look at no kernel's code."""
import numpy as np
import pytest
import torch

import coarsehead_cases as CC
import coarsehead_ref as R
from norm_ref import half_ulp, to_dtype

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
PAIRS = [(F32, F32), (BF16, BF16), (F16, F16), (BF16, F32)]       # (x, parameters); the last is autocast's
PAIR_IDS = lambda p: f"{p[0]}-{p[1]}".replace("torch.", "")      # noqa: E731
GRADS = ("g_offset", "g_sh", "g_scaling", "g_rotation", "g_opacity", "g_centers")
OS, SS, HC, THR = CC.OPACITY_SHIFT, CC.SCALING_SHIFT, CC.HALF_CELL, CC.THRESHOLD


def ch():
    from generativedensification_amd import coarsehead as H

    return H


def dev(a, dtype):
    return to_dtype(a, dtype).to(DEV)


def f64(t):
    return t.detach().double().cpu().numpy()


def bar(what, hip, tor, ref64):
    """prints the pair, then hands it to settle"""
    assert hip.dtype == tor.dtype and hip.shape == tor.shape == ref64.shape, (what, hip.dtype, tor.dtype, hip.shape, tor.shape, ref64.shape)
    e_hip = float(np.abs(f64(hip) - ref64).max())
    e_torch = float(np.abs(f64(tor) - ref64).max())
    slack = half_ulp(hip.dtype, float(np.abs(ref64).max()))
    print(f"coarsehead-bar {what}: e_hip={e_hip:.3e} e_torch={e_torch:.3e} half_ulp={slack:.3e}")
    assert np.isfinite(f64(hip)).all(), what
    return what, e_hip, e_torch, slack


def settle(results):
    bad = [(w, eh, et, s) for w, eh, et, s in results if not eh <= 2 * et + s]
    assert not bad, bad


def tensors(name, x_dt, p_dt):
    d = CC.inputs(name, x_dt)
    x = dev(d["x"], x_dt)
    params = [dev(d[k], p_dt) for k in R.PARAMS]
    grads = [dev(d[k], F32) for k in GRADS]
    return d, x, params, grads, dev(d["group_centers"], F32)


def torch_lines(x, params, gc, K, sh_dim):
    """the reference's lines on parameters already cast to x's dtype -> offset, sh, scaling, rotation, opacity, centers, mask"""
    w1, b1, w2, b2, w3, b3 = params
    m = torch.nn.Module()
    m.K, m.sh_dim, m.opacity_dim, m.scaling_dim, m.rotation_dim = K, sh_dim, 1, 3, 4
    F = torch.nn.functional
    m.mlp_coarse = lambda t: F.linear(F.relu(F.linear(F.relu(F.linear(t, w1, b1)), w2, b2)), w3, b3)      # noqa: E731
    out = R.reference_forward_coarse(m, x, OS, SS)
    centers, mask = R.reference_tail(out[0], out[4], gc.view(1, -1, 3), HC, K, THR)
    return (*out, centers, mask)


_REFS = {}


def ref64(name, x_dt):
    if (name, x_dt) not in _REFS:
        d = CC.inputs(name, x_dt)
        _, _, _, K, sh_dim = CC.shape_of(name)
        p = [d[k] for k in R.PARAMS]
        res = R.head(d["x"], *p, K, sh_dim, OS, SS, d["group_centers"], HC, THR)
        res.update(R.head_grad(d["x"], *p, K, sh_dim, {k[2:]: d[k] for k in GRADS}, HC))
        _REFS[(name, x_dt)] = res
    return _REFS[(name, x_dt)]


def run_hip(name, x_dt, p_dt):
    """one forward (with centers and mask) and backward through the Function -> dict of tensors"""
    H = ch()
    _, _, _, K, sh_dim = CC.shape_of(name)
    d, x, params, grads, gc = tensors(name, x_dt, p_dt)
    x = x.clone().requires_grad_(True)
    params = [t.clone().requires_grad_(True) for t in params]
    res = H._apply(x, params, gc, K, sh_dim, OS, SS, HC, THR)
    torch.autograd.backward(list(res[:6]), grads)
    out = dict(zip(R.OUTPUTS + ("centers", "mask"), (t.detach() for t in res)))
    out["dx"] = x.grad
    out.update({"d" + k: t.grad for k, t in zip(R.PARAMS, params)})
    assert all(out[k].dtype == F32 and out[k].is_contiguous() for k in R.OUTPUTS + ("centers",)) and out["mask"].dtype == torch.bool
    assert out["dx"].dtype == x_dt and all(out["d" + k].dtype == p_dt for k in R.PARAMS)
    return out


def run_torch(name, x_dt, p_dt):
    _, _, _, K, sh_dim = CC.shape_of(name)
    d, x, params, grads, gc = tensors(name, x_dt, p_dt)
    x = x.clone().requires_grad_(True)
    params = [t.clone().requires_grad_(True) for t in params]
    res = torch_lines(x, [t.to(x_dt) for t in params], gc, K, sh_dim)
    torch.autograd.backward(list(res[:6]), grads)
    out = dict(zip(R.OUTPUTS + ("centers", "mask"), (t.detach() for t in res)))
    out["dx"] = x.grad
    out.update({"d" + k: t.grad for k, t in zip(R.PARAMS, params)})
    return out


CHECKED = R.OUTPUTS + ("centers", "dx") + tuple("d" + k for k in R.PARAMS)


# ---- 1, 2: the accuracy bar and the mask ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("name", list(CC.CASES))
def test_outputs_gradients_and_mask_meet_the_bar(name, pair):
    hip, tor, ref = run_hip(name, *pair), run_torch(name, *pair), ref64(name, pair[0])
    tag = f"{name}/{pair[0]}/{pair[1]}/".replace("torch.", "")
    results = [bar(tag + k, hip[k], tor[k].contiguous(), ref[k]) for k in CHECKED]
    # the mask, wherever the float64 opacity is further from the threshold than the bar lets an opacity be wrong (plus the
    # float32 rounding of the sigmoid and of the threshold, 1e-5 in opacity)
    _, e_hip, e_torch, slack = next(r for r in results if r[0] == tag + "opacity")
    allowance = 2 * e_torch + slack + 1e-5
    compared = np.abs(ref["opacity"][..., 0] - CC.LOGIT_THRESHOLD) > allowance
    print(f"coarsehead-mask {tag}: allowance={allowance:.3e} left out {int((~compared).sum())} of {compared.size}")
    settle(results)
    assert (~compared).sum() <= 0.01 * compared.size
    assert (hip["mask"].cpu().numpy() == ref["mask"])[compared].all()
    if name == "sat":
        assert float(hip["offset"].abs().min()) == 1.0 and np.isfinite(f64(hip["dx"])).all()


# ---- 3: column routing ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F32, BF16], ids=["float32", "bfloat16"])
def test_a_value_on_one_last_layer_column_lands_in_exactly_its_element(dtype):
    H = ch()
    C, K, sh_dim, rows = 8, 2, 3, 5
    P = sh_dim + 11
    x = torch.ones(1, rows, C, dtype=dtype, device=DEV)
    z = lambda *s: torch.zeros(*s, dtype=dtype, device=DEV)      # noqa: E731
    w1 = w2 = torch.eye(C, dtype=dtype, device=DEV)
    cols = R.columns(K, sh_dim)
    base = {"offset": 0.0, "sh": 0.0, "scaling": 0.75, "rotation": 0.0, "opacity": -0.5}      # the shifts and 2 sigmoid(0) - 1
    for via_bias in (True, False):
        for j in range(K * P):
            w3, b3 = z(K * P, C), z(K * P)
            if via_bias:
                b3[j] = 2.0
            else:
                w3[j, 3] = 2.0                # h2 = 1 everywhere: the same 2 on column j
            out = dict(zip(R.OUTPUTS, H.coarse_head(x, w1, z(C), w2, z(C), w3, b3, K, sh_dim, -0.5, 0.75)))
            k, c = divmod(j, P)
            hit = next(n for n, (a, w) in cols.items() if a <= c < a + w)
            for n, (a, w) in cols.items():
                want = torch.full((1, rows * K, w), base[n], dtype=F32, device=DEV)
                if n == hit:
                    want[0, k::K, c - a] = base[n] + 2.0 if n != "offset" else float(np.tanh(1.0))
                got = out[n].reshape(1, rows * K, w)
                if n == "offset" and n == hit:
                    assert torch.equal(got == 0, want == 0) and torch.allclose(got, want, rtol=0, atol=1e-6), (j, n)
                else:
                    assert torch.equal(got, want), (j, n, via_bias)


# ---- 4: tile isolation --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F32, BF16], ids=["float32", "bfloat16"])
def test_a_large_second_tile_does_not_reach_the_first(dtype):
    H = ch()
    _, _, _, K, sh_dim = CC.shape_of("run")
    d, x, params, grads, gc = tensors("run", dtype, dtype)
    T = H.TILE_ROWS
    assert x.shape[1] > T
    big = x.clone()
    big[:, T:] *= 1000.0
    runs = []
    for inp in (x, big):
        a = inp.clone().requires_grad_(True)
        res = H._apply(a, params, gc, K, sh_dim, OS, SS, HC, THR)
        torch.autograd.backward(list(res[:6]), grads)
        runs.append([t.detach() for t in res] + [a.grad])
    for one, two in zip(*runs):
        assert torch.equal(one[:, :T * K], two[:, :T * K])
    assert not torch.equal(runs[0][1][:, T * K:], runs[1][1][:, T * K:])


# ---- 5: launch discipline -----------------------------------------------------------------------------------------------------------

def test_two_calls_are_bitwise_equal():
    for name, pair in (("slabs", (F32, F32)), ("ref_slim", (BF16, F32)), ("k2", (F16, F16)), ("wide", (BF16, BF16))):
        first, second = run_hip(name, *pair), run_hip(name, *pair)
        for k in first:
            assert torch.equal(first[k], second[k]), (name, k)


def test_no_host_synchronisation():
    H = ch()
    _, _, _, K, sh_dim = CC.shape_of("ref_slim")

    def work():
        d, x, params, grads, gc = tensors("ref_slim", BF16, F32)
        args = (x.requires_grad_(True), [t.requires_grad_(True) for t in params], grads, gc)
        torch.cuda.synchronize()
        return args

    def calls(x, params, grads, gc):
        res = H._apply(x, params, gc, K, sh_dim, OS, SS, HC, THR)
        torch.autograd.backward(list(res[:6]), grads)
        sum(t.sum() for t in H.coarse_head(x.detach().float(), *params, K, sh_dim, OS, SS)).backward()

    calls(*work())                                   # warm-up: library load, kernel images
    args = work()
    previous = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        raised = False
        try:
            args[3][0, 0].item()                     # the canary
        except RuntimeError:
            raised = True
        if raised:
            calls(*args)
    finally:
        torch.cuda.set_sync_debug_mode(previous)
    assert raised, "torch.cuda.set_sync_debug_mode('error') did not raise on .item(): the calls above were not checked"
    torch.cuda.synchronize()
    assert all(torch.isfinite(t.grad).all() for t in [args[0]] + args[1])


def test_runs_under_no_grad_and_vjp_and_unneeded_gradients_are_not_launched(monkeypatch):
    H = ch()
    from generativedensification_amd import _lib as L

    _, _, _, K, sh_dim = CC.shape_of("k2")
    d, x, params, grads, gc = tensors("k2", F32, F32)
    fn = lambda a, *p: H.coarse_head(a, *p, K, sh_dim, OS, SS)      # noqa: E731
    leaves = [t.clone().requires_grad_(True) for t in [x] + params]
    out = fn(*leaves)
    torch.autograd.backward(list(out), grads[:5])
    got, vjps = torch.autograd.functional.vjp(fn, tuple([x] + params), tuple(grads[:5]))
    assert all(torch.equal(a, b) for a, b in zip(got, out)) and all(torch.equal(a, t.grad) for a, t in zip(vjps, leaves))
    with torch.no_grad():
        again = fn(*leaves)
    assert all(torch.equal(a, b) and not a.requires_grad for a, b in zip(again, out))

    # a None upstream gradient for some outputs: only sh and opacity are used
    a = x.clone().requires_grad_(True)
    part = fn(a, *params)
    (part[1] * grads[1]).sum().add((part[4] * grads[4]).sum()).backward()
    want = R.head_grad(d["x"], *(d[k] for k in R.PARAMS), K, sh_dim, {"sh": d["g_sh"], "opacity": d["g_opacity"]})["dx"]
    assert np.abs(f64(a.grad) - want).max() <= 1e-5 * np.abs(want).max()

    lib = L.load()
    real = lib.gdr_coarsehead_backward
    seen = []

    def boom(*args):
        raise AssertionError("a gradient nobody needs was launched")

    def spy(*args):
        seen.append(args)
        return real(*args)

    monkeypatch.setattr(lib, "gdr_coarsehead_fold", boom)            # frozen parameters: no fold, no partial sums
    monkeypatch.setattr(lib, "gdr_coarsehead_backward", spy)
    a = x.clone().requires_grad_(True)
    torch.autograd.backward(list(fn(a, *params)), grads[:5])
    assert torch.equal(a.grad, leaves[0].grad)
    grad_x_arg, workspace_arg = seen[-1][-4], seen[-1][-3]
    assert grad_x_arg is not None and workspace_arg is None
    monkeypatch.undo()
    monkeypatch.setattr(lib, "gdr_coarsehead_backward", spy)          # a non-differentiable x: no grad_x store
    only = [t.clone().requires_grad_(True) for t in params]
    torch.autograd.backward(list(fn(x, *only)), grads[:5])
    assert seen[-1][-4] is None and seen[-1][-3] is not None
    assert all(torch.equal(t.grad, leaf.grad) for t, leaf in zip(only, leaves[1:]))


# ---- 6: autocast ----------------------------------------------------------------------------------------------------------------------

def test_autocast_casts_a_float32_input_and_keeps_float32_parameter_gradients():
    H = ch()
    _, _, _, K, sh_dim = CC.shape_of("ref_slim")
    d, x16, params, grads, gc = tensors("ref_slim", BF16, F32)
    x = x16.float().requires_grad_(True)
    leaves = [t.clone().requires_grad_(True) for t in params]
    with torch.autocast("cuda", dtype=BF16):
        out = H.coarse_head(x, *leaves, K, sh_dim, OS, SS)
    assert all(t.dtype == F32 for t in out)
    torch.autograd.backward(list(out), grads[:5])
    assert x.grad.dtype == F32 and all(t.grad.dtype == F32 for t in leaves)
    a = x16.clone().requires_grad_(True)
    again_leaves = [t.clone().requires_grad_(True) for t in params]
    again = H.coarse_head(a, *again_leaves, K, sh_dim, OS, SS)
    torch.autograd.backward(list(again), grads[:5])
    assert all(torch.equal(s, t) for s, t in zip(out, again)) and torch.equal(a.grad.float(), x.grad)
    assert all(torch.equal(s.grad, t.grad) for s, t in zip(leaves, again_leaves))


# ---- 7: the binding -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "bf16-autocast"])
def test_bound_forward_coarse_meets_the_bar_against_the_torch_backend(autocast):
    H = ch()
    name = "ref_slim"
    B, N, C, K, sh_dim = CC.shape_of(name)
    x_dt = BF16 if autocast else F32
    d, x, params, grads, gc = tensors(name, x_dt, F32)
    dec = R.make_decoder(C, K, sh_dim).to(DEV)
    with torch.no_grad():
        for t, s in zip(H._params(dec), params):
            t.copy_(s)
    type(dec).forward_coarse = H.decoder_forward_coarse
    assert H.covers(dec)
    runs = {}
    saved = H.HEAD_BACKEND
    try:
        for backend in ("hip", "torch"):
            H.HEAD_BACKEND = backend
            dec.zero_grad()
            a = x.float().requires_grad_(True)
            with torch.autocast("cuda", dtype=BF16, enabled=autocast):
                out = dec.forward_coarse(a, OS, SS)
                full = H.coarse_gaussians(dec, a, gc.view(1, N, 3), HC, OS, SS, THR)
            assert all(t.dtype == F32 for t in out) and full[5].dtype == torch.bool and not full[5].requires_grad
            assert all(t.is_contiguous() for t in out) == (backend == "hip")
            torch.autograd.backward(list(out) + [full[0]], grads)
            runs[backend] = dict(zip(R.OUTPUTS + ("centers",), [t.detach().contiguous() for t in out] + [full[0].detach()]))
            runs[backend]["dx"] = a.grad
            runs[backend].update({"d" + k: t.grad.clone() for k, t in zip(R.PARAMS, H._params(dec))})
    finally:
        H.HEAD_BACKEND = saved
    ref = ref64(name, x_dt)
    tag = f"bound/{'bf16-autocast' if autocast else 'fp32'}/"
    settle([bar(tag + k, runs["hip"][k], runs["torch"][k], ref[k]) for k in CHECKED])
    # another layer list is not covered, and then the torch lines run: strided views of one tensor
    other = R.make_decoder(C, K, sh_dim, [torch.nn.Linear(C, C), torch.nn.ReLU(), torch.nn.Linear(C, K * (sh_dim + 11))]).to(DEV)
    assert not H.covers(other)
    out = H.decoder_forward_coarse(other, x.float(), OS, SS)
    assert not out[1].is_contiguous() and out[0].shape == (B, N * K, 3)


# ---- 8: refusals and empties ------------------------------------------------------------------------------------------------------------

def test_refusals_come_before_a_launch_and_empty_inputs_return_empty_tensors(monkeypatch):
    H = ch()
    from generativedensification_amd import _lib as L

    def no_load():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(L, "load", no_load)
    z = lambda *s, dtype=F32: torch.zeros(*s, dtype=dtype, device=DEV)      # noqa: E731
    C, K, sh = 8, 1, 3
    good = [z(2, 3, C), z(C, C), z(C), z(C, C), z(C), z(14, C), z(14)]
    for i in (0, 1, 6):
        bad = list(good)
        bad[i] = bad[i].double()
        with pytest.raises(TypeError):
            H.coarse_head(*bad, K, sh, 0.0, 0.0)
    with pytest.raises(TypeError):
        H.coarse_head(*good, 1.0, sh, 0.0, 0.0)
    for bad, k, s in ((good, 1, 4), (good, 5, 3), (good, 2, 3), ([z(2, 3, 12), z(12, 12), z(12), z(12, 12), z(12), z(14, 12), z(14)], 1, 3),
                      (good[:3] + [z(16, C)] + good[4:], 1, 3), ([z(C)] + good[1:], 1, 3),
                      ([z(1, 264), z(264, 264), z(264), z(264, 264), z(264), z(14, 264), z(14)], 1, 3)):
        with pytest.raises(ValueError):
            H.coarse_head(*bad, k, s, 0.0, 0.0)
    huge = z(1, dtype=BF16).expand(1 << 31, C)          # 2^31 rows, no memory
    with pytest.raises(ValueError, match="envelope"):
        H.coarse_head(huge, *good[1:], K, sh, 0.0, 0.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.coarse_head(good[0], good[1].cpu(), *good[2:], K, sh, 0.0, 0.0)
    params = [t.clone().requires_grad_(True) for t in good[1:]]
    for shape in ((0, C), (2, 0, C), (0, 4, 4, C)):
        x = torch.zeros(shape, device=DEV, dtype=BF16, requires_grad=True)
        out = H.coarse_head(x, *params, K, sh, 0.0, 0.0)
        assert [tuple(t.shape) for t in out] == [(shape[0], 0, 3), (shape[0], 0, 1, 3), (shape[0], 0, 3), (shape[0], 0, 4), (shape[0], 0, 1)]
        sum(t.sum() for t in out).backward()
        assert x.grad.shape == x.shape and all(torch.equal(t.grad, torch.zeros_like(t)) for t in params)
