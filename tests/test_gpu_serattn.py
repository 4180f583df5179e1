"""GPU: the gather form of the HIP attention (generativedensification_amd/serattn.py, csrc/attn.hip gdr_attn_gather_*) on
the inputs of tests/serattn_cases.py.

Addressing, bit for bit: the forward equals the reference's line over this repository's own drop-in,
    flash_attn_varlen_qkvpacked_func(qkv[order].half().reshape(-1, 3, H, D), cu, patch, softmax_scale=s)
        .reshape(-1, C).to(qkv.dtype)[inverse],
for every case and dtype (the arithmetic is the same kernel's, only the addresses differ); for f16 qkv the backward equals that
composition's gradient on the rows the padding holds once (dQ, dK, dV) and in dQ on every row.

Accuracy, the bar of tests/test_gpu_attn.py as it stands: per tensor (out, dQ, dK, dV) err_hip <= 2 err_pt + ulp, err_hip
against the f64 restatement (tests/serattn_ref.py) computed from the same fp16-rounded inputs, err_pt the error of the
all-torch composition on the same device (serattn_ref.torch_composition), ulp the spacing of the tensor's dtype at its largest
magnitude.  Both errors are printed before the assertion.

patch_size as a hint: the same tables under a patch_size of a higher row tile give the same bits, so the gather kernels of the
three tiles check each other without a tolerance.

Then: two runs are bitwise equal and nothing synchronises with the host, through the op and through the bound forward with
the tables cached in the point; the bound forward under bf16 autocast at the bar of
test_gpu_attn.test_the_call_as_the_reference_makes_it_under_bf16_autocast; vjp and no_grad; the fall-backs.

Measured on an MI355X, worst err_hip / err_pt over the cases and out, dQ, dK, dV: 0.85 (f32 qkv), 1.02 (bf16), 2.58 (f16: dQ of
rp256_d64, delta from the fp16 result as the bitwise equality demands); the closest any tensor came to its bar was 0.90 of it
(that dQ), 0.42 for f32 and 0.26 for bf16.  Over the eight tile cases (serattn_cases.TILE_SHAPES): 1.00,
1.09 and 1.49 (f16 dQ of rp128_full_d8); closest 0.50, 0.28 and 0.54."""
import functools
import json
import os

import pytest
import torch

import attn_cases as AC
import attn_ref as R
import serattn_cases as SC
import serattn_ref as SR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _op(case, qkv=None, backward=True, patch=None):
    from generativedensification_amd import serattn as S

    qkv = (case["qkv"] if qkv is None else qkv).detach().requires_grad_(backward)
    out = S.serialized_attention(qkv, case["order"], case["inverse"], case["cu_t"], case["H"], patch or case["patch"],
                                 case["scale"])
    if backward:
        out.backward(case["dout"])
    return out.detach(), qkv.grad


def _drop_in(case):
    """the reference's line, with its autograd, over the drop-in"""
    from flash_attn import flash_attn_varlen_qkvpacked_func

    H, D, C = case["H"], case["D"], case["C"]
    qkv = case["qkv"].detach().requires_grad_(True)
    out = flash_attn_varlen_qkvpacked_func(qkv[case["order"]].half().reshape(-1, 3, H, D), case["cu_t"], case["patch"],
                                           softmax_scale=case["scale"]).reshape(-1, C).to(qkv.dtype)[case["inverse"]]
    out.backward(case["dout"])
    return out.detach(), qkv.grad


@functools.lru_cache(maxsize=None)
def _truth(name, dt):
    """the f64 restatement from the fp16-rounded inputs, once per case and dtype"""
    c = SC.make(name, dt)
    q64, d64 = c["qkv"].half().double(), c["dout"].half().double()
    out = SR.forward(q64, c["order"], c["inverse"], c["cu"], c["H"], c["scale"])
    dqkv = SR.backward(q64, c["order"], c["inverse"], c["cu"], c["H"], d64, c["scale"])
    return out, dqkv


def _report(what, got, truth, pt, dtype):
    err_hip = float((got.double() - truth).abs().max())
    err_pt = float((pt.double() - truth).abs().max())
    limit = AC.bar(err_pt, dtype, truth)
    print(f"{what}: err_hip {err_hip:.3e} err_pt {err_pt:.3e} ratio {err_hip / err_pt if err_pt else float('inf'):.3f} "
          f"ulp {AC.ulp(dtype, float(truth.abs().max())):.3e} bar {limit:.3e}")
    return err_hip, limit


@pytest.mark.parametrize("name,dt", SC.CASES)
def test_forward_is_the_composition_over_the_drop_in_bit_for_bit(name, dt):
    case = SC.make(name, dt, DEV)
    out, _ = _op(case, backward=False)
    want, _ = _drop_in(case)
    assert out.dtype == SC.DTYPES[dt] and out.shape == (case["N"], case["C"])
    assert torch.equal(out, want) and float(out.float().abs().max()) > 0
    # under no_grad, through a qkv that is neither dense nor aligned (one copy)
    wide = torch.zeros(case["N"], 3 * case["C"] + 1, dtype=SC.DTYPES[dt], device=DEV)
    wide[:, 1:] = case["qkv"]
    with torch.no_grad():
        out2, _ = _op(case, wide[:, 1:], backward=False)
    assert torch.equal(out2, want)


@pytest.mark.parametrize("name", list(SC.SHAPES))
def test_f16_backward_is_the_composition_bit_for_bit_where_the_padding_holds_a_row_once(name):
    case = SC.make(name, "f16", DEV)
    _, dqkv = _op(case)
    _, want = _drop_in(case)
    C, once = case["C"], ~case["has_copy"]
    assert dqkv.dtype == torch.float16 and dqkv.shape == want.shape
    assert torch.equal(dqkv[once], want[once]) and int(once.sum()) == case["N"] - SC.COPIES[name]
    assert torch.equal(dqkv[:, :C], want[:, :C])                      # dQ: a copy adds exactly zero
    assert float(dqkv.float().abs().max()) > 0
    if SC.COPIES[name]:   # the rows held twice do receive their second contribution (its size is the accuracy test's to judge)
        twice = case["has_copy"]
        t_dqkv = _truth(name, "f16")[1][twice.cpu()][:, C:]
        assert float((dqkv[twice][:, C:].double().cpu() - t_dqkv).abs().max()) < 0.05 * float(t_dqkv.abs().max())


@pytest.mark.parametrize("name,dt", SC.CASES)
def test_forward_and_gradients_against_f64(name, dt):
    dtype = SC.DTYPES[dt]
    case = SC.make(name, dt, DEV)
    out, dqkv = _op(case)
    assert dqkv.dtype == dtype and dqkv.shape == case["qkv"].shape
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(dqkv.float()).all())
    t_out, t_dqkv = _truth(name, dt)
    pt_out, pt_dqkv = SR.torch_composition(case["qkv"], case["order"], case["inverse"], case["cu"], case["H"], case["scale"],
                                           case["dout"])
    C = case["C"]
    results = [_report("out", out.cpu(), t_out, pt_out.cpu(), dtype)]
    for i, w in enumerate(("dq", "dk", "dv")):
        sl = slice(i * C, (i + 1) * C)
        results.append(_report(w, dqkv[:, sl].cpu(), t_dqkv[:, sl], pt_dqkv[:, sl].cpu(), dtype))
    for err, limit in results:
        assert err <= limit, (name, dt, results)


@pytest.mark.parametrize("name,dt", [(name, dt) for name in SC.SHAPES if SC.SHAPES[name][0] <= 128 for dt in SC.DTYPES])
def test_a_larger_patch_size_over_the_same_tables_gives_the_same_bits(name, dt):
    """patch_size only picks the row tile (64, 128 or 256 rows per head): the same tables under a patch_size of every higher
    tile give out and dqkv bit for bit, the borrowed rows' second contribution included.  The kernels of the three tiles are
    compared with each other, with no tolerance."""
    case = SC.make(name, dt, DEV)
    out, dqkv = _op(case)
    assert float(out.float().abs().max()) > 0 and float(dqkv.float().abs().max()) > 0
    higher = [p for p in (100, 128, 200, 256) if AC.row_tile(p) > AC.row_tile(case["patch"])]
    assert {AC.row_tile(p) for p in higher} == {rp for rp in (128, 256) if rp > AC.row_tile(case["patch"])}
    differ = 0
    for p in higher:
        out_p, dqkv_p = _op(case, patch=p)
        differ += AC.bits_differ(f"out at patch_size {p}", out_p, out)
        for i, w in enumerate(("dq", "dk", "dv")):
            sl = slice(i * case["C"], (i + 1) * case["C"])
            differ += AC.bits_differ(f"{w} at patch_size {p}", dqkv_p[:, sl], dqkv[:, sl])
    assert differ == 0, (name, dt)


def _bound(mod, point):
    from generativedensification_amd import serattn as S

    return S.serialized_attention_forward(mod, point)


def _stage0(C=160, H=20, dtype=torch.float32):
    patch, offsets, *_ = SC.SHAPES["cfg_stage0"]
    N = offsets[-1]
    order, inverse, cu, ser = SC.tables(offsets, patch, 11)
    g = torch.Generator().manual_seed(N)
    torch.manual_seed(N + 1)
    mod = SR.Module(C, H, patch, order_index=1).to(DEV)
    feat = (torch.randn(N, C, generator=g) * (1 + torch.arange(C) % 5)).to(DEV, dtype)
    w = (torch.randn(N, C, generator=g) * (0.5 + torch.arange(N).view(N, 1) % 3)).to(DEV)
    return mod, feat, w, offsets, patch, order.to(DEV), inverse.to(DEV), cu, ser


def test_two_runs_are_bitwise_equal_and_nothing_synchronises_with_the_host():
    for name, dt in (("borrow47_h3_d8", "bf16"), ("rp256_d64", "f32"), ("cfg_stage0", "f16")):
        case = SC.make(name, dt, DEV)
        runs = []
        for _ in range(2):
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                runs.append(_op(case))
            finally:
                torch.cuda.set_sync_debug_mode("default")
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    # the bound forward, the tables cached in the point by a first call
    mod, feat, w, offsets, patch, *_, ser = _stage0()
    point = SR.make_point(feat, offsets, ser, order_index=1)
    _bound(mod, point)
    assert all(k in point for k in ("pad", "unpad", "cu_seqlens_key"))
    runs = []
    for _ in range(2):
        x = feat.clone().requires_grad_(True)
        point.feat = x
        mod.zero_grad()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            with torch.autocast("cuda", torch.bfloat16):
                y = _bound(mod, point).feat
            (y.float() * w).sum().backward()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        runs.append((y.detach().clone(), x.grad.clone(), mod.qkv.weight.grad.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def _lines(mod, feat, order, inverse, cu_list, cu, mode):
    """the reference's lines with the attention by `mode`: the drop-in ("dropin"), f32 torch per patch ("f32") or the torch
    composition in fp16 per patch ("half")"""
    from flash_attn import flash_attn_varlen_qkvpacked_func

    H, C = mod.num_heads, mod.channels
    qkv = mod.qkv(feat)[order]
    packed = qkv.half().reshape(-1, 3, H, C // H)
    if mode == "dropin":
        x = flash_attn_varlen_qkvpacked_func(packed, cu, max_seqlen=mod.patch_size, dropout_p=0, softmax_scale=mod.scale)
    else:
        with torch.autocast("cuda", enabled=False):
            p = packed.float() if mode == "f32" else packed
            rows = []
            for a, b in zip(cu_list[:-1], cu_list[1:]):
                q, k, v = p[a:b].permute(1, 2, 0, 3).unbind(0)
                attn = torch.softmax((q * mod.scale) @ k.transpose(-2, -1), dim=-1)
                rows.append((attn @ v).transpose(0, 1))
            x = torch.cat(rows, 0).half()
    x = x.reshape(-1, C).to(qkv.dtype)
    return mod.proj_drop(mod.proj(x[inverse]))


def test_the_bound_forward_under_bf16_autocast():
    """err(bound forward) <= 2 err(fp16-composition lines) + ulp against the lines with f32 attention per patch, for the output
    and the gradients reaching qkv.weight and the input features; the output equals the lines over the drop-in bit for bit."""
    surface = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "serattn_surface.json")))
    mod, feat0, w, offsets, patch, order, inverse, cu, ser = _stage0()
    assert all(hasattr(mod, name) for name in surface["SerializedAttention"]["assigned"])
    res = {}
    for mode in ("f32", "half", "dropin", "bound"):
        feat = feat0.clone().requires_grad_(True)
        mod.zero_grad()
        with torch.autocast("cuda", torch.bfloat16):
            if mode == "bound":
                point = SR.make_point(feat, offsets, ser, order_index=1)      # no tables yet: patch_tables builds them
                y = _bound(mod, point).feat
                pad, unpad, cu_t = R.padded_patches(offsets, patch)
                assert torch.equal(point["pad"].cpu(), pad) and torch.equal(point["unpad"].cpu(), unpad)
                assert torch.equal(point["cu_seqlens_key"].cpu(), cu_t)
            else:
                y = _lines(mod, feat, order, inverse, cu.tolist(), cu.to(DEV), mode)
        assert y.dtype == torch.bfloat16
        (y.float() * w).sum().backward()
        res[mode] = (y.detach().clone(), mod.qkv.weight.grad.clone(), feat.grad.clone())
    assert torch.equal(res["bound"][0], res["dropin"][0])
    for what, t, pt, got in zip(("out", "d qkv.weight", "d feat"), res["f32"], res["half"], res["bound"]):
        err, limit = _report(what, got.cpu(), t.double().cpu(), pt.cpu(), t.dtype)
        assert float(t.abs().max()) > 0
        assert err <= limit, (what, err, limit)


def test_vjp_and_no_grad():
    from generativedensification_amd import serattn as S

    case = SC.make("borrow47_h3_d8", "f32", DEV)
    out, dqkv = _op(case)
    f = lambda x: S.serialized_attention(x, case["order"], case["inverse"], case["cu_t"], case["H"], case["patch"], case["scale"])  # noqa: E731
    o2, g2 = torch.autograd.functional.vjp(f, case["qkv"], case["dout"])
    assert torch.equal(o2, out) and torch.equal(g2, dqkv)
    with torch.no_grad():
        o3 = f(case["qkv"].detach().requires_grad_(True))
    assert torch.equal(o3, out) and not o3.requires_grad
    empty = S.serialized_attention(case["qkv"][:0], case["order"][:0], case["inverse"][:0], case["cu_t"][:1], case["H"], 48)
    assert empty.shape == (0, case["C"]) and empty.dtype == torch.float32


def test_fallbacks_give_the_composition():
    from generativedensification_amd import serattn as S

    mod, feat, w, offsets, patch, order, inverse, cu, ser = _stage0()
    with torch.no_grad():
        want = _lines(mod, feat, order, inverse, cu.tolist(), cu.to(DEV), "dropin")
        hip = _bound(mod, SR.make_point(feat, offsets, ser, order_index=1)).feat
        old = S.SERATTN_BACKEND
        try:
            S.SERATTN_BACKEND = "torch"
            torch_ = _bound(mod, SR.make_point(feat, offsets, ser, order_index=1)).feat
        finally:
            S.SERATTN_BACKEND = old
        assert torch.equal(hip, want) and torch.equal(torch_, want)
        # outside `covers`: the non-flash branch, patches of the smallest segment (30), against f32 attention per patch
        plain = SR.Module(160, 20, patch, enable_flash=False, order_index=1).to(DEV)
        plain.load_state_dict(mod.state_dict())
        assert not S.covers(plain)
        point = SR.make_point(feat, offsets, ser, order_index=1)
        got = _bound(plain, point).feat
        assert plain.patch_size == 30 and int(point["cu_seqlens_key"][1]) == 30
        order30, inverse30, cu30, _ = SC.tables(offsets, 30, 11)
        ref = _lines(plain, feat, order30.to(DEV), inverse30.to(DEV), cu30.tolist(), cu30.to(DEV), "f32")
        # (the lines round qkv and the result to fp16, 2^-11 each, the non-flash branch does neither: 4 x 2^-11 of the largest value)
        assert float((got - ref).abs().max()) <= 2e-3 * float(ref.abs().max())
