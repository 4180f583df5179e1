"""GPU: the HIP attention (csrc/attn.hip through the `flash_attn` drop-in) against the f64 restatement (tests/attn_ref.py)
on every input of tests/attn_cases.py, forward, lse and dQ, dK, dV; the rows nobody owns; bitwise reproducibility without
host synchronisation; the fixed-length entry point; and the call as the reference's SerializedAttention makes it.

The bar is measured against the reference arithmetic, per tensor:  err_hip <= 2 err_pt + ulp, where err_hip is the maximum
absolute difference to the f64 restatement (computed from the same half-rounded inputs), err_pt the same difference for the
plain torch composition in the same half dtype on the same device ((q * scale) @ k^T, softmax, @ v: the reference's
non-flash branch with upcasting off), and ulp the spacing of the output dtype at the tensor's largest f64 magnitude
(attn_cases.bar).  lse: twice the error of torch's f32 logsumexp of the f32 scores, plus one f32 ulp.  Every test prints
both errors before it asserts.

Measured on an MI355X, worst err_hip / err_pt over the cases: 1.35 (fp16) and 1.55 (bf16) over out, dQ, dK, dV, 1.34 and 1.81
for lse; the closest any tensor came to its bar was 0.62 of it."""
import pytest
import torch

import attn_cases as AC
import attn_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _hip(case, qkv=None):
    from flash_attn import flash_attn_varlen_qkvpacked_func

    qkv = (case["qkv"] if qkv is None else qkv).detach().requires_grad_(True)
    out = flash_attn_varlen_qkvpacked_func(qkv, case["cu_t"], case["max_seqlen"], softmax_scale=case["scale"])
    out.backward(case["dout"])
    return out.detach(), qkv.grad


def _report(what, got, truth, pt, dtype):
    err_hip = float((got.double() - truth).abs().max())
    err_pt = float((pt.double() - truth).abs().max())
    limit = AC.bar(err_pt, dtype, truth)
    print(f"{what}: err_hip {err_hip:.3e} err_pt {err_pt:.3e} ratio {err_hip / err_pt if err_pt else float('inf'):.3f} "
          f"ulp {AC.ulp(dtype, float(truth.abs().max())):.3e} bar {limit:.3e}")
    return err_hip, limit


@pytest.mark.parametrize("name,dt", AC.CASES)
def test_forward_lse_and_gradients_against_f64_on_symmetry_breaking_inputs(name, dt):
    from generativedensification_amd import _lib as L
    import ctypes as C

    dtype = AC.DTYPES[dt]
    case = AC.make(name, dtype, DEV)
    out, dqkv = _hip(case)
    assert out.dtype == dtype and dqkv.dtype == dtype and dqkv.shape == case["qkv"].shape
    cpu = AC.make(name, dtype)
    q64 = cpu["qkv"].double()
    t_out, t_lse = R.attention(q64, cpu["cu"], cpu["scale"])
    t_dqkv = R.attention_backward(q64, cpu["cu"], cpu["dout"].double(), cpu["scale"])
    pt_out, pt_dqkv = AC.torch_composition(case["qkv"], case["cu"], case["scale"], case["dout"])
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(dqkv.float()).all())
    results = [_report("out", out.cpu(), t_out, pt_out.cpu(), dtype)]
    for i, w in enumerate(("dq", "dk", "dv")):
        results.append(_report(w, dqkv[:, i].cpu(), t_dqkv[:, i], pt_dqkv[:, i].cpu(), dtype))
    # lse straight from the C entry point (the drop-in does not return it)
    H, D, total = case["qkv"].shape[2], case["qkv"].shape[3], case["qkv"].shape[0]
    a = L.GdrAttnArgs()
    a.total, a.batch, a.H, a.D, a.max_seqlen = total, len(case["cu"]) - 1, H, D, case["max_seqlen"]
    a.dtype, a.scale = (L.GDR_ATTN_BF16 if dtype == torch.bfloat16 else L.GDR_ATTN_F16), float(case["scale"] or D ** -0.5)
    lib = L.load()
    assert lib.gdr_attn_lse_bytes(C.byref(a)) == 4 * H * total
    o2 = torch.empty(total, H, D, dtype=dtype, device=DEV)
    lse = torch.full((H, total), float("nan"), dtype=torch.float32, device=DEV)
    st = (C.c_int64 * 4)(*case["qkv"].stride())
    L.check(lib.gdr_attn_forward(C.byref(a), case["qkv"].data_ptr(), st, case["cu_t"].data_ptr(), o2.data_ptr(), lse.data_ptr(),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)), "gdr_attn_forward")
    torch.cuda.synchronize()
    assert torch.equal(o2, out)
    results.append(_report("lse", lse.cpu(), t_lse, AC.f32_lse(case["qkv"], case["cu"], case["scale"]).cpu(), torch.float32))
    for err, limit in results:
        assert err <= limit, (name, dt, results)


@pytest.mark.parametrize("dt", list(AC.DTYPES))
def test_rows_nobody_owns_are_exactly_zero_and_an_empty_sequence_contributes_nothing(dt):
    dtype = AC.DTYPES[dt]
    case = AC.make("mixed_h3_d8", dtype, DEV)
    tail = case["cu"][-1]
    assert case["qkv"].shape[0] > tail
    poisoned = case["qkv"].clone()
    poisoned[tail:] = float("nan")          # nothing may be read from there either
    out, dqkv = _hip(case, poisoned)
    assert not out[tail:].any() and not dqkv[tail:].any()
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(dqkv.float()).all())
    # the same call without its zero-length sequence (a repeated boundary removed) gives the same bits
    cu = [c for i, c in enumerate(case["cu"]) if i == 0 or c != case["cu"][i - 1]]
    assert len(cu) == len(case["cu"]) - 1
    other = dict(case, cu_t=torch.tensor(cu, dtype=torch.int32, device=DEV))
    out2, dqkv2 = _hip(other, poisoned)
    assert torch.equal(out, out2) and torch.equal(dqkv, dqkv2)
    # an all-empty call: only zeros
    empty = dict(case, cu_t=torch.zeros(3, dtype=torch.int32, device=DEV))
    out3, dqkv3 = _hip(empty, poisoned)
    assert not out3.any() and not dqkv3.any()


def test_two_runs_are_bitwise_equal_and_nothing_synchronises_with_the_host():
    from flash_attn import flash_attn_varlen_qkvpacked_func

    runs = []
    for name, dt in (("mixed_h5_d64_scaled", "bf16"), ("ref48_h20_d8", "fp16"), ("mixed_h3_d8", "fp16")):
        case = AC.make(name, AC.DTYPES[dt], DEV)
        for _ in range(2):
            qkv = case["qkv"].detach().requires_grad_(True)
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                out = flash_attn_varlen_qkvpacked_func(qkv, case["cu_t"], case["max_seqlen"], softmax_scale=case["scale"])
                out.backward(case["dout"])
            finally:
                torch.cuda.set_sync_debug_mode("default")
            runs.append((out.detach().clone(), qkv.grad.clone()))
        assert torch.equal(runs[-1][0], runs[-2][0]) and torch.equal(runs[-1][1], runs[-2][1])


@pytest.mark.parametrize("dt", list(AC.DTYPES))
def test_fixed_length_entry_point_equals_the_varlen_call_bit_for_bit(dt):
    from flash_attn import flash_attn_qkvpacked_func, flash_attn_varlen_qkvpacked_func

    dtype = AC.DTYPES[dt]
    case = AC.make("ref48_h20_d8", dtype, DEV)
    B, Lq = 6, 48
    qkv = case["qkv"].detach().requires_grad_(True)
    out = flash_attn_varlen_qkvpacked_func(qkv, case["cu_t"], Lq, softmax_scale=case["scale"])
    out.backward(case["dout"])
    q5 = case["qkv"].reshape(B, Lq, 3, 20, 8).detach().requires_grad_(True)
    out5 = flash_attn_qkvpacked_func(q5, softmax_scale=case["scale"])
    assert out5.shape == (B, Lq, 20, 8)
    out5.backward(case["dout"].reshape(B, Lq, 20, 8))
    assert torch.equal(out5.reshape(-1, 20, 8), out) and torch.equal(q5.grad.reshape(-1, 3, 20, 8), qkv.grad)
    assert float(out.detach().float().abs().max()) > 0 and float(qkv.grad.float().abs().max()) > 0


# ---- the call as the reference's SerializedAttention makes it --------------------------------------------------------------
class _PatchAttention(torch.nn.Module):
    """Linear -> [order][pad] gather -> .half().reshape(-1, 3, H, C // H) -> attention per patch -> .reshape(-1, C) -> cast
    back -> [inverse] -> Linear, with the attention computed by `mode`: the drop-in ("hip"), f32 torch per patch ("f32") or
    the torch composition in fp16 per patch ("half")."""

    def __init__(self, C, H, patch):
        super().__init__()
        self.C, self.H, self.patch, self.scale = C, H, patch, (C // H) ** -0.5
        self.qkv = torch.nn.Linear(C, 3 * C)
        self.proj = torch.nn.Linear(C, C)

    def forward(self, feat, order, inverse, cu_list, cu, mode):
        from flash_attn import flash_attn_varlen_qkvpacked_func

        H, C = self.H, self.C
        qkv = self.qkv(feat)[order]
        packed = qkv.half().reshape(-1, 3, H, C // H)
        if mode == "hip":
            x = flash_attn_varlen_qkvpacked_func(packed, cu, max_seqlen=self.patch, dropout_p=0, softmax_scale=self.scale)
        else:
            with torch.autocast("cuda", enabled=False):
                p = packed.float() if mode == "f32" else packed
                rows = []
                for a, b in zip(cu_list[:-1], cu_list[1:]):
                    q, k, v = p[a:b].permute(1, 2, 0, 3).unbind(0)
                    attn = torch.softmax((q * self.scale) @ k.transpose(-2, -1), dim=-1)
                    rows.append((attn @ v).transpose(0, 1))
                x = torch.cat(rows, 0).half()
        x = x.reshape(-1, C).to(qkv.dtype)
        return self.proj(x[inverse])


@pytest.mark.parametrize("offsets,C,H", [((12000,), 160, 20), ((5003,), 256, 32), ((700, 730, 1500), 160, 20)])
def test_the_call_as_the_reference_makes_it_under_bf16_autocast(offsets, C, H):
    """err(hip module) <= 2 err(fp16-composition module) + ulp against the module with f32 attention per patch, for the
    output and the gradients reaching the first Linear's weight and the input features (pad duplicates tokens, so that
    gradient is an accumulation).  ulp: the spacing of the tensor's own dtype at its largest magnitude."""
    patch, N = 48, offsets[-1]
    pad, unpad, cu = R.padded_patches(offsets, patch)
    assert int(cu[-1]) == pad.numel() and (len(offsets) == 1 or min(b - a for a, b in zip((0,) + offsets, offsets)) < patch)
    g = torch.Generator().manual_seed(N)
    ser = torch.randperm(N, generator=g)                 # a serialisation order and its inverse
    order, inverse = ser[pad].to(DEV), unpad[torch.argsort(ser)].to(DEV)
    torch.manual_seed(N + 1)
    mod = _PatchAttention(C, H, patch).to(DEV)
    feat0 = (torch.randn(N, C, generator=g) * (1 + torch.arange(C) % 5)).to(DEV)
    w = (torch.randn(N, C, generator=g) * (0.5 + torch.arange(N).view(N, 1) % 3)).to(DEV)
    res = {}
    for mode in ("f32", "half", "hip"):
        feat = feat0.clone().requires_grad_(True)
        mod.zero_grad()
        with torch.autocast("cuda", torch.bfloat16):
            y = mod(feat, order, inverse, cu.tolist(), cu.to(DEV), mode)
        assert y.dtype == torch.bfloat16
        (y.float() * w).sum().backward()
        res[mode] = (y.detach().clone(), mod.qkv.weight.grad.clone(), feat.grad.clone())
    for what, t, pt, got in zip(("out", "d qkv.weight", "d feat"), res["f32"], res["half"], res["hip"]):
        err, limit = _report(what, got.cpu(), t.double().cpu(), pt.cpu(), t.dtype)
        assert float(t.abs().max()) > 0
        assert err <= limit, (what, err, limit)
