"""GPU: the fused fine Gaussian head and the fine-set assembly (csrc/finehead.hip through generativedensification_amd.finehead)
against the numpy restatement (tests/finehead_ref.py) and against the reference's lines on the same GPU.

The head's accuracy bar (the one of tests/test_gpu_coarsehead.py), for the output and every gradient: with e_hip = max|hip - ref64|
and e_torch = max|torch - ref64| (ref64 on the inputs as rounded to their dtypes), e_hip <= 2 e_torch + half an ulp of the result
dtype at max|ref64|.  `torch` casts the parameters to the compute dtype as autocast would.  Every pair is printed before it is
asserted.  The maxima are taken over all draws of a case together (tests/finehead_cases.py: every tensor under the bar then has at
least 256 elements).  The assembly is compared bit for bit.  The tests never synchronise inside a checked region, provoke no
out-of-range access and look at no kernel's code."""
import warnings

import numpy as np
import pytest
import torch

import finehead_cases as FC
import finehead_ref as R
from norm_ref import half_ulp, to_dtype

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
PAIRS = [(F32, F32), (BF16, BF16), (F16, F16), (BF16, F32)]       # (feat, parameters); the last is autocast's
PAIR_IDS = lambda p: f"{p[0]}-{p[1]}".replace("torch.", "")      # noqa: E731
OS, SS = FC.OPACITY_SHIFT, FC.SCALING_SHIFT
CHECKED = ("out", "dx") + tuple("d" + k for k in R.PARAMS)


def fh():
    from generativedensification_amd import finehead as H

    return H


def dev(a, dtype):
    return to_dtype(a, dtype).to(DEV)


def f64(t):
    return t.detach().double().cpu().numpy()


def bar(what, hip, tor, ref64, dtype):
    """prints the pair, then hands it to settle; hip, tor, ref64: float64 arrays of values of `dtype`, all draws together"""
    assert hip.shape == tor.shape == ref64.shape and hip.size >= FC.MIN_ELEMENTS, (what, hip.shape, tor.shape, ref64.shape)
    e_hip = float(np.abs(hip - ref64).max())
    e_torch = float(np.abs(tor - ref64).max())
    slack = half_ulp(dtype, float(np.abs(ref64).max()))
    print(f"finehead-bar {what}: e_hip={e_hip:.3e} e_torch={e_torch:.3e} half_ulp={slack:.3e} ratio={e_hip / (2 * e_torch + slack):.3f}")
    assert np.isfinite(hip).all(), what
    return what, e_hip, e_torch, slack


def settle(results):
    bad = [(w, eh, et, s) for w, eh, et, s in results if not eh <= 2 * et + s]
    assert not bad, bad


def head_shapes():
    return FC.head_shapes(fh().backward_step)


def leaves(C, sh_dim, x_dt, p_dt):
    p = FC.head_params(C, sh_dim, x_dt)
    return [dev(p[k], p_dt) for k in R.PARAMS]


def run_hip(x, g, params, out_dtype):
    """one forward and backward through the Function -> dict of tensors"""
    H = fh()
    x = x.clone().requires_grad_(True)
    params = [t.clone().requires_grad_(True) for t in params]
    out = H.gaussian_head(x, *params, out_dtype=out_dtype)
    assert out.dtype == (x.dtype if out_dtype is None else out_dtype) and out.is_contiguous()
    out.backward(g.to(out.dtype))
    res = {"out": out.detach(), "dx": x.grad}
    res.update({"d" + k: t.grad for k, t in zip(R.PARAMS, params)})
    assert res["dx"].dtype == x.dtype and all(res["d" + k].dtype == t.dtype for k, t in zip(R.PARAMS, params))
    return res


def run_torch(x, g, params, out_dtype):
    """the reference's lines on parameters cast to x's dtype"""
    F = torch.nn.functional
    x = x.clone().requires_grad_(True)
    params = [t.clone().requires_grad_(True) for t in params]
    w1, b1, w2, b2 = [t.to(x.dtype) for t in params]
    out = F.linear(F.gelu(F.linear(x, w1, b1)), w2, b2)
    if out_dtype is not None:
        out = out.to(out_dtype)
    out.backward(g.to(out.dtype))
    res = {"out": out.detach(), "dx": x.grad}
    res.update({"d" + k: t.grad for k, t in zip(R.PARAMS, params)})
    return res


_REFS = {}


def ref64(rows, C, sh_dim, x_dt, out_dt, rep):
    """the float64 results of one draw; the upstream gradient is the draw's g as rounded to the output's dtype"""
    key = (rows, C, sh_dim, x_dt, out_dt, rep)
    if key not in _REFS:
        p = FC.head_params(C, sh_dim, x_dt)
        x, g = FC.head_draw(rows, C, sh_dim, x_dt, rep)
        args = [x] + [p[k] for k in R.PARAMS]
        res = {"out": R.head(*args)}
        res.update(R.head_grad(*args, FC.rounded(g, out_dt)))
        _REFS[key] = res
    return _REFS[key]


# ---- 1: the accuracy bar ------------------------------------------------------------------------------------------------------------

WORST = {"ratio": 0.0}


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("shape", head_shapes(), ids=lambda s: "rows%d-C%d-sh%d" % s)
def test_output_and_gradients_meet_the_bar(shape, pair):
    rows, C, sh_dim = shape
    x_dt, p_dt = pair
    params = leaves(C, sh_dim, x_dt, p_dt)
    results = []
    for out_dtype in ((None,) if x_dt == F32 else (None, F32)):
        out_dt = x_dt if out_dtype is None else out_dtype
        pooled = {k: ([], [], []) for k in CHECKED}
        for rep in range(FC.repeats(C, sh_dim)):
            xa, ga = FC.head_draw(rows, C, sh_dim, x_dt, rep)
            x, g = dev(xa, x_dt), dev(ga, F32)
            hip, tor, ref = run_hip(x, g, params, out_dtype), run_torch(x, g, params, out_dtype), ref64(rows, C, sh_dim, x_dt, out_dt, rep)
            for k in CHECKED:
                assert hip[k].dtype == tor[k].dtype and hip[k].shape == tor[k].shape == ref[k].shape, (k, hip[k].dtype, tor[k].dtype)
                for acc, a in zip(pooled[k], (f64(hip[k]), f64(tor[k]), ref[k])):
                    acc.append(a.reshape(-1))
        tag = f"rows{rows}/C{C}/sh{sh_dim}/{x_dt}/{p_dt}/out-{out_dt}/".replace("torch.", "")
        dtype_of = {"out": out_dt, "dx": x_dt, "dw1": p_dt, "db1": p_dt, "dw2": p_dt, "db2": p_dt}
        results += [bar(tag + k, *(np.concatenate(a) for a in pooled[k]), dtype_of[k]) for k in CHECKED]
    worst = max(eh / (2 * et + s) for _, eh, et, s in results)
    WORST["ratio"] = max(WORST["ratio"], worst)
    print(f"finehead-bar worst ratio of this case {worst:.3f}, so far {WORST['ratio']:.3f}")
    settle(results)


# ---- 2: the one-row call ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_one_row_equals_row_zero_of_the_17_row_call(pair):
    x_dt, p_dt = pair
    for C, sh_dim in ((8, 3), (256, 12), (40, 48)):
        params = leaves(C, sh_dim, x_dt, p_dt)
        xa, ga = FC.head_draw(17, C, sh_dim, x_dt, 0)
        x, g = dev(xa, x_dt), dev(ga, F32)
        for out_dtype in (None, F32):
            full, one = run_hip(x, g, params, out_dtype), run_hip(x[:1], g[:1], params, out_dtype)
            assert torch.equal(one["out"], full["out"][:1]) and torch.equal(one["dx"], full["dx"][:1]), (C, sh_dim, out_dtype)
            # the column sum of one row is the row: the upstream gradient as the kernel reads it (rounded to the compute dtype), rounded
            # once more to the parameter's dtype
            want = g[:1].to(one["out"].dtype).to(x_dt).to(p_dt).reshape(-1)
            assert torch.equal(one["db2"], want), (C, sh_dim, out_dtype)


# ---- 3: launch discipline -----------------------------------------------------------------------------------------------------------

def test_two_calls_are_bitwise_equal():
    for (rows, C, sh_dim), pair in (((FC.SLAB_MIN + 1, 256, 12), (BF16, F32)), ((FC.SLAB_MIN + 1, 40, 48), (F32, F32)), ((65, 160, 3), (F16, F16))):
        params = leaves(C, sh_dim, *pair)
        xa, ga = FC.head_draw(rows, C, sh_dim, pair[0], 0)
        x, g = dev(xa, pair[0]), dev(ga, F32)
        first, second = run_hip(x, g, params, None), run_hip(x, g, params, None)
        for k in first:
            assert torch.equal(first[k], second[k]), (rows, C, sh_dim, k)


def test_strided_or_misaligned_feat_costs_one_copy_and_gives_the_same_bits():
    H = fh()
    rows, C, sh_dim = 65, 40, 12
    params = leaves(C, sh_dim, BF16, BF16)
    xa, ga = FC.head_draw(rows, C, sh_dim, BF16, 0)
    x, g = dev(xa, BF16), dev(ga, F32)
    want = run_hip(x, g, params, None)
    wide = torch.zeros(rows, 2 * C, dtype=BF16, device=DEV)
    wide[:, :C] = x
    shifted = torch.zeros(rows * C + 1, dtype=BF16, device=DEV)
    shifted[1:] = x.reshape(-1)
    for other in (wide[:, :C], shifted[1:].view(rows, C)):
        assert not other.is_contiguous() or other.data_ptr() % 16
        assert H._rows(other).data_ptr() % 16 == 0 and H._rows(other).is_contiguous() and H._rows(x) is x
        got = run_hip(other, g, params, None)
        assert all(torch.equal(got[k], want[k]) for k in want)


def test_no_host_synchronisation():
    H = fh()
    rows, C, sh_dim = 65, 40, 12

    def work():
        params = [t.requires_grad_(True) for t in leaves(C, sh_dim, BF16, F32)]
        xa, ga = FC.head_draw(rows, C, sh_dim, BF16, 0)
        d, levels, coarse, fine, mask, selected = assembly_tensors("two_levels", BF16)
        levels = [(c.requires_grad_(True), a.requires_grad_(True)) for c, a in levels]
        args = (dev(xa, BF16).requires_grad_(True), params, dev(ga, F32),
                (levels, *[c.requires_grad_(True) for c in coarse], fine.requires_grad_(True), mask, selected), int((~d["selected"]).sum()))
        torch.cuda.synchronize()
        return args

    def calls(x, params, g, assembly, n_survivors):
        out = H.gaussian_head(x, *params)
        out.backward(g.to(out.dtype))
        H.gaussian_head(x.detach().float(), *params, out_dtype=F32).sum().backward()
        res = H.assemble_fine_gaussians(*assembly, 3, OS, SS, n_survivors=n_survivors)
        torch.autograd.backward(list(res), [torch.ones_like(t) for t in res])

    calls(*work())                                   # warm-up: library load, kernel images
    args = work()
    previous = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        raised = False
        try:
            args[2][0, 0].item()                     # the canary
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
    H = fh()
    from generativedensification_amd import _lib as L

    rows, C, sh_dim = 33, 40, 12
    params = leaves(C, sh_dim, F32, F32)
    xa, ga = FC.head_draw(rows, C, sh_dim, F32, 0)
    x, g = dev(xa, F32), dev(ga, F32)
    fn = lambda a, *p: H.gaussian_head(a, *p)      # noqa: E731
    lv = [t.clone().requires_grad_(True) for t in [x] + params]
    out = fn(*lv)
    out.backward(g)
    got, vjps = torch.autograd.functional.vjp(fn, tuple([x] + params), g)
    assert torch.equal(got, out) and all(torch.equal(a, t.grad) for a, t in zip(vjps, lv))
    with torch.no_grad():
        again = fn(*lv)
    assert torch.equal(again, out) and not again.requires_grad

    lib = L.load()
    real = lib.gdr_finehead_backward
    seen = []

    def boom(*args):
        raise AssertionError("a gradient nobody needs was launched")

    def spy(*args):
        seen.append(args)
        return real(*args)

    monkeypatch.setattr(lib, "gdr_finehead_fold", boom)            # frozen parameters: no fold, no partial sums
    monkeypatch.setattr(lib, "gdr_finehead_backward", spy)
    a = x.clone().requires_grad_(True)
    fn(a, *params).backward(g)
    assert torch.equal(a.grad, lv[0].grad)
    grad_x_arg, workspace_arg = seen[-1][-4], seen[-1][-3]
    assert grad_x_arg is not None and workspace_arg is None
    monkeypatch.undo()
    monkeypatch.setattr(lib, "gdr_finehead_backward", spy)          # a non-differentiable feat: no grad_x store
    only = [t.clone().requires_grad_(True) for t in params]
    fn(x, *only).backward(g)
    assert seen[-1][-4] is None and seen[-1][-3] is not None
    assert all(torch.equal(t.grad, leaf.grad) for t, leaf in zip(only, lv[1:]))
    # a None upstream gradient reaches the kernel as NULL and reads as zeros without a fill: grad_b2, the column sums of g, is
    # exactly zero.  (autograd never calls the node of a single output without a gradient, so this goes through the C entry)
    zero = torch.zeros(sh_dim + 8, device=DEV)
    gb2 = torch.full_like(zero, 7.0)
    dt = L.GDR_NORM_DTYPES["f32"]
    ws, base, usable = H._workspace(lib, L.GDR_FINEHEAD_WS_PARTIALS, dt, rows, C, sh_dim, DEV)
    pws, pbase = H._packed(lib, params[0], params[2], True, dt, C, sh_dim, DEV)
    from generativedensification_amd import _marshal as M

    L.check(real(x.data_ptr(), dt, pbase, params[1].data_ptr(), dt, rows, C, sh_dim, None, dt, None, base, usable, M.stream()), "backward")
    L.check(lib.gdr_finehead_fold(base, usable, dt, rows, C, sh_dim, None, dt, None, dt, None, dt, gb2.data_ptr(), dt, M.stream()), "fold")
    assert torch.equal(gb2, zero)


def test_autocast_casts_a_float32_feat_and_keeps_float32_parameter_gradients():
    H = fh()
    rows, C, sh_dim = 65, 40, 12
    params = leaves(C, sh_dim, BF16, F32)
    xa, ga = FC.head_draw(rows, C, sh_dim, BF16, 0)
    x16, g = dev(xa, BF16), dev(ga, F32)
    x = x16.float().requires_grad_(True)
    lv = [t.clone().requires_grad_(True) for t in params]
    with torch.autocast("cuda", dtype=BF16):
        out = H.gaussian_head(x, *lv)
    assert out.dtype == BF16
    out.backward(g.to(BF16))
    assert x.grad.dtype == F32 and all(t.grad.dtype == F32 for t in lv)
    want = run_hip(x16, g, params, None)
    assert torch.equal(out, want["out"]) and torch.equal(x.grad, want["dx"].float())
    assert all(torch.equal(t.grad, want["d" + k]) for t, k in zip(lv, R.PARAMS))


# ---- 4: the bindings ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "bf16-autocast"])
def test_bound_forwards_equal_gaussian_head(autocast):
    H = fh()
    rows, C, sh_degree = 65, 40, 1
    sh_dim = 12
    xa, _ = FC.head_draw(rows, C, sh_dim, BF16, 0)
    feat = dev(xa, F32)
    saved = H.HEAD_BACKEND
    try:
        for kind, forward, reference in (("GaussianModule", H.gaussian_module_forward, R.reference_module_forward),
                                         ("GaussianResModule", H.gaussian_res_module_forward, R.reference_res_module_forward)):
            m = R.make_module(kind, C, sh_degree, is_first=False, enable_residual_attribute=True).to(DEV)
            assert H.covers(m)
            type(m).forward = forward
            prior = torch.randn(rows, sh_dim + 8, device=DEV)

            def point():
                inner = R.Point(feat=feat, attribute=prior)
                return R.Point(leaf_point=inner) if kind == "GaussianModule" else inner

            with torch.autocast("cuda", dtype=BF16, enabled=autocast):
                H.HEAD_BACKEND = "hip"
                got = m(point())
                head = H.gaussian_head(feat, *H._params(m))
                H.HEAD_BACKEND = "torch"
                tor = m(point())
                want = reference(m, point())
            if kind == "GaussianModule":
                got, tor, want = got.leaf_point, tor.leaf_point, want.leaf_point
                assert torch.equal(got.attribute, head)
            else:
                assert torch.equal(got.attribute, prior + head)
            assert torch.equal(tor.attribute, want.attribute) and got.attribute.dtype == want.attribute.dtype
            assert (got.attribute.float() - want.attribute.float()).abs().max() <= (0.1 if autocast else 1e-4)
    finally:
        H.HEAD_BACKEND = saved
    other = R.make_module("GaussianModule", C, sh_degree, layers=[torch.nn.Linear(C, C), torch.nn.GELU(approximate="tanh"), torch.nn.Linear(C, sh_dim + 8)]).to(DEV)
    assert not H.covers(other)
    p = H.gaussian_module_forward(other, R.Point(leaf_point=R.Point(feat=feat)))
    assert torch.equal(p.leaf_point.attribute, other.feat2attr(feat))


# ---- 5: refusals and empties ------------------------------------------------------------------------------------------------------------

def test_refusals_come_before_a_launch_and_empty_inputs_return_empty_tensors(monkeypatch):
    H = fh()
    from generativedensification_amd import _lib as L

    def no_load():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(L, "load", no_load)
    z = lambda *s, dtype=F32: torch.zeros(*s, dtype=dtype, device=DEV)      # noqa: E731
    C, P = 8, 11
    good = [z(5, C), z(C, C), z(C), z(P, C), z(P)]
    for i in (0, 1, 4):
        bad = list(good)
        bad[i] = bad[i].double()
        with pytest.raises(TypeError):
            H.gaussian_head(*bad)
    with pytest.raises(TypeError):
        H.gaussian_head(*good, out_dtype=BF16)
    for bad in ([z(5, 12), z(12, 12), z(12), z(P, 12), z(P)], good[:1] + [z(16, C)] + good[2:], [z(2, 5, C)] + good[1:], good[:3] + [z(12, C), z(12)],
                [z(5, 264), z(264, 264), z(264), z(P, 264), z(P)], good[:2] + [z(C + 1)] + good[3:]):
        with pytest.raises(ValueError):
            H.gaussian_head(*bad)
    huge = z(1, dtype=BF16).expand(1 << 31, C)          # 2^31 rows, no memory
    with pytest.raises(ValueError, match="envelope"):
        H.gaussian_head(huge, *good[1:])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.gaussian_head(good[0], good[1].cpu(), *good[2:])
    params = [t.clone().requires_grad_(True) for t in good[1:]]
    x = torch.zeros(0, C, device=DEV, dtype=BF16, requires_grad=True)
    out = H.gaussian_head(x, *params)
    assert out.shape == (0, P) and out.dtype == BF16
    out.sum().backward()
    assert x.grad.shape == x.shape and all(torch.equal(t.grad, torch.zeros_like(t)) for t in params)
    # the assembly: an all-empty result
    res = H.assemble_fine_gaussians([(z(0, 3), z(0, 20))], z(0, 3), z(0, 1), z(0, 3), z(0, 4), z(0, 4, 3), z(0, dtype=torch.bool), z(0, dtype=torch.bool),
                                    12, OS, SS)
    assert [tuple(t.shape) for t in res] == [(0, 3), (0, 4, 3), (0, 1), (0, 3), (0, 4)]
    with pytest.raises(NotImplementedError, match="_union_gaussians"):
        H.assemble_fine_gaussians([(z(2, 3), z(2, 20), torch.tensor([1, 2], device=DEV))], z(3, 3), z(3, 1), z(3, 3), z(3, 4), z(0, 4, 3),
                                  z(3, dtype=torch.bool), z(0, dtype=torch.bool), 12, OS, SS)
    with pytest.raises(TypeError):
        H.assemble_fine_gaussians([(z(2, 3), z(2, 20))], z(3, 3), z(3, 1), z(3, 3), z(3, 4), z(0, 4, 3), z(3), z(0, dtype=torch.bool), 12, OS, SS)
    with pytest.raises(ValueError):
        H.assemble_fine_gaussians([(z(2, 3), z(2, 21))], z(3, 3), z(3, 1), z(3, 3), z(3, 4), z(0, 4, 3), z(3, dtype=torch.bool), z(0, dtype=torch.bool), 12, OS, SS)


# ---- 6: the assembly --------------------------------------------------------------------------------------------------------------------

def assembly_tensors(name, attr_dt):
    d = FC.assembly_inputs(name, attr_dt)
    t = lambda a, dt=F32: torch.from_numpy(np.array(a)).to(dt).to(DEV)      # noqa: E731
    levels = [(t(c), t(a, attr_dt)) for c, a in d["levels"]]
    return d, levels, [t(a) for a in d["coarse"]], t(d["shs_fine"]), t(d["mask"], torch.bool), t(d["selected"], torch.bool)


def run_assembly(name, attr_dt, n_survivors=None, reference=False):
    """-> the five outputs and the leaves (levels flattened, the coarse tensors, shs_fine), all requiring grad"""
    H = fh()
    d, levels, coarse, fine, mask, selected = assembly_tensors(name, attr_dt)
    sh_dim = FC.ASSEMBLY[name][4]
    levels = [(c.requires_grad_(True), a.requires_grad_(True)) for c, a in levels]
    coarse = [c.requires_grad_(True) for c in coarse]
    fine.requires_grad_(True)
    if n_survivors == "known":
        n_survivors = int((~d["selected"]).sum())
    if reference:
        res = R.reference_assemble(levels, coarse, fine, mask, selected, sh_dim, OS, SS) if levels else None
    else:
        res = H.assemble_fine_gaussians(levels, coarse[0], coarse[1], coarse[2], coarse[3], fine, mask, selected, sh_dim, OS, SS, n_survivors=n_survivors)
    return res, [t for level in levels for t in level] + coarse + [fine]


ASSEMBLY_WITH_LEVELS = [n for n in FC.ASSEMBLY if FC.ASSEMBLY[n][0]]


@pytest.mark.parametrize("attr_dt", [F32, BF16, F16], ids=["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("name", ASSEMBLY_WITH_LEVELS)
def test_assembly_and_its_gradients_equal_the_torch_lines_bitwise(name, attr_dt):
    d = FC.assembly_inputs(name, attr_dt)
    sh_dim = FC.ASSEMBLY[name][4]
    T = sum(FC.ASSEMBLY[name][0]) + int((~d["selected"]).sum())
    one_hot = {k: np.zeros_like(v) for k, v in d["grads"].items()}
    for k, v in one_hot.items():
        v.reshape(-1)[(v.size * 2) // 3 if v.size else slice(0, 0)] = 1.0      # an element of the survivor rows where there are some
    for upstream in (d["grads"], one_hot):
        gs = [torch.from_numpy(upstream[k]).to(DEV) for k in R.OUTPUTS]
        runs = []
        for reference, n_surv in ((False, None), (False, "known"), (True, None)):
            res, leaves_ = run_assembly(name, attr_dt, n_survivors=n_surv, reference=reference)
            assert [tuple(t.shape) for t in res] == [(T, 3), (T, sh_dim // 3, 3), (T, 1), (T, 3), (T, 4)]
            assert all(t.dtype == F32 for t in res) and (reference or all(t.is_contiguous() for t in res))
            torch.autograd.backward(list(res), gs)
            runs.append(([t.detach() for t in res], [t.grad for t in leaves_]))
        want = runs[2]
        ref = R.assemble([(c, a) for c, a in d["levels"]], d["coarse"], d["shs_fine"], d["mask"], d["selected"], sh_dim, OS, SS)
        for got in runs[:2]:
            for a, b, k in zip(got[0], want[0], R.OUTPUTS):
                assert torch.equal(a, b) and np.array_equal(a.cpu().numpy().view(np.uint32), ref[k].view(np.uint32)), (name, k)
            for i, (a, b) in enumerate(zip(got[1], want[1])):
                if b is None:          # torch hands no gradient to a tensor that reaches no output: ours is exactly zero
                    assert a is None or not a.any(), (name, i)
                else:
                    assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (name, i)
        # the dense coarse gradients are exactly zero off the survivor rows
        rows, keep = R.survivors(d["mask"], d["selected"])
        off = np.ones(len(d["mask"]), bool)
        off[rows] = False
        n_levels = len(FC.ASSEMBLY[name][0])
        for gc in runs[0][1][2 * n_levels:2 * n_levels + 4]:
            assert not gc[torch.from_numpy(off).to(DEV)].any()
        off_fine = torch.from_numpy(d["selected"]).to(DEV)
        assert not runs[0][1][-1][off_fine].any()


def test_assembly_without_levels_and_none_upstream_gradients():
    d = FC.assembly_inputs("no_levels", F32)
    res, leaves_ = run_assembly("no_levels", F32)
    ref = R.assemble([], d["coarse"], d["shs_fine"], d["mask"], d["selected"], 3, OS, SS)
    assert all(np.array_equal(a.detach().cpu().numpy(), ref[k]) for a, k in zip(res, R.OUTPUTS))
    # only opacity is used downstream: every other upstream gradient is None and reads as zeros
    res, leaves_ = run_assembly("two_levels", BF16, n_survivors="known")
    d = FC.assembly_inputs("two_levels", BF16)
    g = torch.from_numpy(d["grads"]["opacity"]).to(DEV)
    res[2].backward(g)
    levels, dense, dfine = R.assemble_grad(list(FC.ASSEMBLY["two_levels"][0]), len(d["mask"]), d["mask"], d["selected"], 3, {"opacity": d["grads"]["opacity"]})
    want = [a for c, attr in levels for a in (c, FC.rounded(attr, BF16))] + dense + [dfine]
    for got, w in zip(leaves_, want):
        assert got.grad is not None and np.array_equal(got.grad.double().cpu().numpy(), np.asarray(w, dtype=np.float64))


def test_a_given_survivor_count_never_synchronises_and_none_reads_back_once():
    run_assembly("chunks", BF16)                       # warm-up
    torch.cuda.synchronize()
    previous = torch.cuda.get_sync_debug_mode()
    try:
        d, levels, coarse, fine, mask, selected = assembly_tensors("chunks", BF16)      # (the uploads are not what is counted)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("warn")
        H = fh()
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            fine.requires_grad_(True)
            res = H.assemble_fine_gaussians(levels, *coarse, fine, mask, selected, 12, OS, SS, n_survivors=int((~d["selected"]).sum()))
            torch.autograd.backward(list(res), [torch.ones_like(t) for t in res])
        assert not [w for w in seen if "synchroniz" in str(w.message)], [str(w.message) for w in seen]
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            again = H.assemble_fine_gaussians(levels, *coarse, fine, mask, selected, 12, OS, SS)
        assert len([w for w in seen if "synchroniz" in str(w.message)]) == 1, [str(w.message) for w in seen]
    finally:
        torch.cuda.set_sync_debug_mode(previous)
    assert all(torch.equal(a, b) for a, b in zip(res, again))


def test_a_too_small_survivor_count_leaves_the_guard_rows_untouched():
    H = fh()
    from generativedensification_amd import _lib as L

    name, sh_dim, guard = "chunks", 12, 7
    d, levels, coarse, fine, mask, selected = assembly_tensors(name, F16)
    full = H.assemble_fine_gaussians(levels, *coarse, fine, mask, selected, sh_dim, OS, SS)
    rows = sum(FC.ASSEMBLY[name][0])
    true = int((~d["selected"]).sum())
    short = true - 5
    lib = L.load()
    tables = H._scan(lib, mask, selected, DEV)
    assert tables[4].tolist() == [int(d["mask"].sum()), true]
    for offset in (0, 1):                              # outputs on 16 bytes, and one float off them: the scalar stores
        bufs = [torch.full(((rows + short + guard) * w + offset,), -7.0, device=DEV) for w in (3, sh_dim, 1, 3, 4)]
        outs = [b[offset:offset + (rows + short) * w].view(rows + short, w) for b, w in zip(bufs, (3, sh_dim, 1, 3, 4))]
        H._assemble_into(lib, [c for c, _ in levels], [a for _, a in levels], coarse, fine.view(-1, sh_dim), tables[1], tables[3], short, sh_dim, OS, SS, outs)
        for b, o, f, w in zip(bufs, outs, full, (3, sh_dim, 1, 3, 4)):
            assert torch.equal(o, f.reshape(-1, w)[:rows + short])
            assert (b[:offset] == -7.0).all() and (b[offset + (rows + short) * w:] == -7.0).all()
    # through the public call: the result is the first rows of the full one
    got = H.assemble_fine_gaussians(levels, *coarse, fine, mask, selected, sh_dim, OS, SS, n_survivors=short)
    assert all(torch.equal(a, b[:rows + short]) for a, b in zip(got, full))
