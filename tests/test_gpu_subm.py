"""GPU: the HIP submanifold convolution (csrc/subm_conv.hip through generativedensification_amd.sparse_conv and the `spconv`
drop-in) against the CPU restatements of tests/subm_ref.py on the cases of tests/subm_cases.py.

Bar per tensor: |result - truth| <= 2 * err_yardstick + 8 * eps32 * max|truth| (+ one ulp of the half type times |truth| per
element for a 16-bit result), err_yardstick = the f32 restatement's own largest error against the f64 truth on that case.
Truth: the dense composition where it applies, the table model for shared voxels and sites outside the grid.  For the half
types truth and yardstick are computed on operands first rounded to that type."""
import functools

import numpy as np
import pytest
import torch

import subm_ref as R
from subm_cases import by_name, cases

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
ULP = {torch.float32: 0.0, torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
NAMES = ("out", "grad_feat", "grad_weight", "grad_bias")


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def model(case):
    return R.table_model(case.indices, case.shape, case.batch, case.ksize)


@functools.lru_cache(maxsize=None)
def reference(case, dtype):
    """(operands rounded to dtype as f64, truth f64, err_yardstick per tensor): computed once per (case, dtype)"""
    ops = [R.round_to(x, dtype) for x in (case.feat, case.weight, case.bias, case.grad_out)]
    nbr, _ = model(case)
    if case.dense_ok:
        truth = R.dense_all(case.indices, case.shape, case.batch, case.ksize, *ops, dtype=torch.float64)
        yard = R.dense_all(case.indices, case.shape, case.batch, case.ksize, *ops, dtype=torch.float32)
    else:
        truth = R.table_all(nbr, *ops, dtype=torch.float64)
        yard = R.table_all(nbr, *ops, dtype=torch.float32)
    err = {k: float((yard[k].double() - truth[k]).abs().max()) if truth[k].numel() else 0.0 for k in NAMES}
    return ops, truth, err


def gpu_inputs(case, dtype, ops):
    feat, weight, bias, go = (t.to(dtype).to(dev()) for t in ops)
    if case.slice_of:
        wide = torch.randn(case.N, case.slice_of, device=dev()).to(dtype)
        wide[:, case.slice_off:case.slice_off + case.cin] = feat
        wide.requires_grad_(True)
        return wide, wide[:, case.slice_off:case.slice_off + case.cin], weight.requires_grad_(True), bias.requires_grad_(True), go
    feat.requires_grad_(True)
    return feat, feat, weight.requires_grad_(True), bias.requires_grad_(True), go


def run(case, dtype, ops):
    from generativedensification_amd import sparse_conv as S

    table = S.build_table(torch.as_tensor(case.indices).to(dev()), case.shape, case.batch, case.ksize)
    leaf, feat, weight, bias, go = gpu_inputs(case, dtype, ops)
    out = S.subm_conv3d(feat, table, weight, bias)
    gleaf, gw, gb = torch.autograd.grad(out, (leaf, weight, bias), go)
    if case.slice_of:
        outside = torch.ones(case.slice_of, dtype=torch.bool)
        outside[case.slice_off:case.slice_off + case.cin] = False
        assert not gleaf[:, outside.to(dev())].any()
        gleaf = gleaf[:, case.slice_off:case.slice_off + case.cin]
    torch.cuda.synchronize()
    return table, {"out": out.detach(), "grad_feat": gleaf, "grad_weight": gw, "grad_bias": gb}


@pytest.mark.parametrize("case", cases(), ids=repr)
def test_table_is_bit_equal_to_the_model(case):
    from generativedensification_amd import sparse_conv as S

    nbr, rep = model(case)
    table = S.build_table(torch.as_tensor(case.indices).to(dev()), case.shape, case.batch, case.ksize)
    assert table.nbr.dtype == torch.int32 and tuple(table.nbr.shape) == nbr.shape and table.ksize == case.ksize
    assert np.array_equal(table.nbr.cpu().numpy(), nbr)
    assert np.array_equal(table.rep.cpu().numpy(), rep)
    order = table.order.cpu().numpy()
    assert sorted(order.tolist()) == list(range(case.N))
    again = S.build_table(torch.as_tensor(case.indices).to(dev()), case.shape, case.batch, case.ksize)
    assert torch.equal(again.nbr, table.nbr) and torch.equal(again.rep, table.rep) and torch.equal(again.order, table.order)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("case", cases(), ids=repr)
def test_forward_and_gradients_meet_the_bar(case, dtype):
    ops, truth, err = reference(case, dtype)
    _, got = run(case, dtype, ops)
    failures = []
    for name in NAMES:
        g, t = got[name].double().cpu(), truth[name]
        assert g.shape == t.shape and got[name].dtype == dtype, name
        if not t.numel():
            continue
        tol = 2 * err[name] + 8 * EPS32 * float(t.abs().max()) + ULP[dtype] * t.abs()
        diff = (g - t).abs()
        worst = float((diff / tol).max())
        print(f"{case.name} {dtype} {name}: max|diff| {float(diff.max()):.3e} err_yardstick {err[name]:.3e} "
              f"max|truth| {float(t.abs().max()):.3e} worst diff/bar {worst:.3f}")
        if not bool((diff <= tol).all()):
            failures.append((name, worst))
    assert not failures, failures


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("name", ["n65_c40", "shared_2_5", "full_block_k135"])
def test_two_runs_are_bitwise_equal(name, dtype):
    case = by_name(name)
    ops, _, _ = reference(case, dtype)
    t1, a = run(case, dtype, ops)
    t2, b = run(case, dtype, ops)
    for k in NAMES:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(t1.nbr, t2.nbr) and torch.equal(t1.rep, t2.rep)


def test_shared_voxel_sites_get_identical_rows_and_zero_feature_gradient():
    case = by_name("shared_2_5")
    ops, _, _ = reference(case, torch.float16)
    table, got = run(case, torch.float16, ops)
    rep = table.rep.long()
    assert torch.equal(got["out"], got["out"][rep])
    assert not got["grad_feat"][rep != torch.arange(case.N, device=dev())].any()


def test_out_of_range_site_outputs_the_bias():
    case = by_name("out_of_range")
    ops, _, _ = reference(case, torch.float32)
    _, got = run(case, torch.float32, ops)
    bad = [i for i in range(case.N) if case.indices[i, 0] >= 1 or (case.indices[i, 1:] < 0).any() or (case.indices[i, 1:] >= 5).any()]
    assert torch.equal(got["out"][bad].cpu(), ops[2].float().expand(3, -1)) and not got["grad_feat"][bad].any()


def test_two_layers_with_one_indice_key_build_one_table():
    import spconv.pytorch as spconv
    from generativedensification_amd import sparse_conv as S

    case = by_name("n65_c40")
    torch.manual_seed(1)
    a = spconv.SubMConv3d(40, 24, 3, indice_key="stage0").to(dev())
    b = spconv.SubMConv3d(24, 40, 3, indice_key="stage0").to(dev())
    c = spconv.SubMConv3d(40, 24, (1, 3, 5), indice_key="other").to(dev())
    x = spconv.SparseConvTensor(torch.as_tensor(case.feat).float().to(dev()), torch.as_tensor(case.indices).to(dev()), case.shape,
                                case.batch)
    before = S.TABLES_BUILT
    y = a(x)
    assert S.TABLES_BUILT == before + 1
    z = b(y.replace_feature(torch.relu(y.features)))
    assert S.TABLES_BUILT == before + 1 and z.indice_dict is x.indice_dict and list(x.indice_dict) == ["stage0"]
    c(z)
    assert S.TABLES_BUILT == before + 2 and z.features.shape == (case.N, 40) and y.features.shape == (case.N, 24)
    with pytest.raises(ValueError, match="kernel size"):
        spconv.SubMConv3d(40, 24, 5, indice_key="stage0").to(dev())(x)
    # the module computes what the functional form computes
    nbr, _ = model(case)
    want = R.table_all(nbr, case.feat, a.weight.detach().double().cpu(), a.bias.detach().double().cpu())["out"]
    assert float((y.features.double().cpu() - want).abs().max()) <= 64 * EPS32 * float(want.abs().max())


def test_autocast_dtype_rule_and_parameter_gradient_dtypes():
    import spconv.pytorch as spconv

    case = by_name("n63")
    m = spconv.SubMConv3d(16, 32, 3, indice_key="k").to(dev())
    idx = torch.as_tensor(case.indices).to(dev())
    feat = torch.as_tensor(case.feat).float().to(dev()).requires_grad_(True)
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):       # fp16 whatever autocast's own dtype is
        y = m(spconv.SparseConvTensor(feat, idx, case.shape, case.batch)).features
    assert y.dtype == torch.float16
    y.float().square().sum().backward()
    assert feat.grad.dtype == torch.float32 and m.weight.grad.dtype == torch.float32 and m.bias.grad.dtype == torch.float32
    assert m.weight.grad.shape == m.weight.shape and bool(m.weight.grad.any())
    for dtype in DTYPES:                                                  # outside autocast: the features' dtype
        mm = spconv.SubMConv3d(16, 32, 3).to(dev()).to(dtype)
        f = feat.detach().to(dtype).requires_grad_(True)
        out = mm(spconv.SparseConvTensor(f, idx, case.shape, case.batch)).features
        assert out.dtype == dtype
        out.float().sum().backward()
        assert f.grad.dtype == dtype and mm.weight.grad.dtype == dtype and mm.bias.grad.dtype == dtype


def test_no_grad_call_keeps_no_backward_state_and_only_wanted_gradients_are_computed():
    from generativedensification_amd import sparse_conv as S

    case = by_name("n65_c40")
    ops, truth, _ = reference(case, torch.float32)
    table = S.build_table(torch.as_tensor(case.indices).to(dev()), case.shape, case.batch, case.ksize)
    feat, weight, bias, _ = (t.float().to(dev()) for t in ops)
    with torch.no_grad():
        out = S.subm_conv3d(feat, table, weight.requires_grad_(True), bias)
    assert out.grad_fn is None and not out.requires_grad
    out2 = S.subm_conv3d(feat, table, weight.detach(), bias)
    assert out2.grad_fn is None and torch.equal(out, out2)
    out3 = S.subm_conv3d(feat, table, weight.detach(), bias.requires_grad_(True))
    saved = out3.grad_fn.saved_tensors
    assert all(t is None for t in saved)                                  # the bias gradient needs neither features nor weight
    (gb,) = torch.autograd.grad(out3, (bias,), torch.ones_like(out3))
    assert torch.allclose(gb, torch.full_like(gb, float(case.N)))


def test_gradients_agree_with_central_differences_in_fp32():
    """16 -> 32 channels, N = 65.  The layer is linear in each input, so a central difference with a power-of-two step is
    exact up to the f32 rounding of the two forward passes: |FD - <grad, d>| <= (sum_i |R_i| (e_i+ + e_i-)) / (2 h) + the
    analytic side's own rounding, e_i <= (terms + 2) eps32 sum|products| (the worst case of any summation order)."""
    from generativedensification_amd import sparse_conv as S

    rng = np.random.default_rng(5)
    idx = np.concatenate([np.zeros((65, 1), np.int64), np.stack(np.unravel_index(rng.choice(125, 65, replace=False), (5, 5, 5)), 1)], 1)
    nbr, _ = R.table_model(idx, (5, 5, 5), 1, (3, 3, 3))
    table = S.build_table(torch.as_tensor(idx, dtype=torch.int32).to(dev()), (5, 5, 5), 1, 3)
    assert np.array_equal(table.nbr.cpu().numpy(), nbr)
    feat = torch.as_tensor(rng.standard_normal((65, 16)), dtype=torch.float32, device=dev()).requires_grad_(True)
    weight = torch.as_tensor(rng.standard_normal((32, 3, 3, 3, 16)) / 20, dtype=torch.float32, device=dev()).requires_grad_(True)
    bias = torch.as_tensor(rng.standard_normal(32), dtype=torch.float32, device=dev()).requires_grad_(True)
    Rw = torch.as_tensor(rng.standard_normal((65, 32)), dtype=torch.float32, device=dev())
    out = S.subm_conv3d(feat, table, weight, bias)
    grads = torch.autograd.grad(out, (feat, weight, bias), Rw)
    h = 2.0 ** -3
    terms = 27 * 16 + 1
    for which, (x, g) in enumerate(zip((feat, weight, bias), grads)):
        d = torch.as_tensor(rng.standard_normal(tuple(x.shape)), dtype=torch.float32, device=dev())
        args = [feat.detach(), weight.detach(), bias.detach()]
        vals, mags = [], []
        for sgn in (1.0, -1.0):
            a = list(args)
            a[which] = args[which] + sgn * h * d
            vals.append(float((S.subm_conv3d(a[0], table, a[1], a[2]).double() * Rw.double()).sum()))
            mags.append(R.table_all(nbr, a[0].abs().double().cpu(), a[1].abs().double().cpu(), a[2].abs().double().cpu())["out"])
        fd = (vals[0] - vals[1]) / (2 * h)
        analytic = float((g.double() * d.double()).sum())
        bound = float((Rw.abs().double().cpu() * (mags[0] + mags[1])).sum()) * (terms + 2) * EPS32 / (2 * h)
        bound += float((g.abs().double() * d.abs().double()).sum()) * (65 * 27 + 2) * EPS32
        print(f"input {which}: fd {fd:.6f} analytic {analytic:.6f} |diff| {abs(fd - analytic):.3e} bound {bound:.3e}")
        assert abs(fd - analytic) <= bound
