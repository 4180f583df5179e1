"""GPU: the HIP attention (csrc/attn.hip through the `flash_attn` drop-in) against the f64 restatement (tests/attn_ref.py)
on every input of tests/attn_cases.py, forward, lse and dQ, dK, dV; the rows nobody owns; bitwise reproducibility without
host synchronisation; the fixed-length entry point; max_seqlen as a hint (any upper bound gives the same bits, so the kernels
of the three row tiles check each other without a tolerance; one that is too small cuts the sequence at the tile); and the
call as the reference's SerializedAttention makes it.

The bar is measured against the reference arithmetic, per tensor:  err_hip <= 2 err_pt + ulp, where err_hip is the maximum
absolute difference to the f64 restatement (computed from the same half-rounded inputs), err_pt the same difference for the
plain torch composition in the same half dtype on the same device ((q * scale) @ k^T, softmax, @ v: the reference's
non-flash branch with upcasting off), and ulp the spacing of the output dtype at the tensor's largest f64 magnitude
(attn_cases.bar).  lse: twice the error of torch's f32 logsumexp of the f32 scores, plus one f32 ulp.  Every test prints
both errors before it asserts.

Measured on an MI355X, worst err_hip / err_pt over the cases: 1.35 (fp16) and 1.55 (bf16) over out, dQ, dK, dV, 1.34 and 1.81
for lse; the closest any tensor came to its bar was 0.62 of it.  Over the twelve tile shapes (t64_,
t128_, t256_): 2.01 and 2.07 (dQ both), 1.80 and 1.00 for lse; closest 0.79 (fp16 lse, D = 64 under 256 keys) and 0.77 (bf16
dQ of t256_h3_d8, where the CPU model of a correct kernel, tests/test_attn_cpu.py, stands at 0.77 too)."""
import ctypes as C

import pytest
import torch

import attn_cases as AC
import attn_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _hip(case, qkv=None, max_seqlen=None):
    from flash_attn import flash_attn_varlen_qkvpacked_func

    qkv = (case["qkv"] if qkv is None else qkv).detach().requires_grad_(True)
    out = flash_attn_varlen_qkvpacked_func(qkv, case["cu_t"], max_seqlen or case["max_seqlen"], softmax_scale=case["scale"])
    out.backward(case["dout"])
    return out.detach(), qkv.grad


def _args(qkv, batch, max_seqlen, scale):
    from generativedensification_amd import _lib as L

    a = L.GdrAttnArgs()
    a.total, a.batch, a.H, a.D, a.max_seqlen = qkv.shape[0], batch, qkv.shape[2], qkv.shape[3], max_seqlen
    a.dtype, a.scale = (L.GDR_ATTN_BF16 if qkv.dtype == torch.bfloat16 else L.GDR_ATTN_F16), float(scale or qkv.shape[3] ** -0.5)
    return a


def _c_forward(qkv, cu_t, max_seqlen, scale, out=None, lse=None):
    """gdr_attn_forward itself (the drop-in does not return lse), into `out` and `lse` if given -> out, lse"""
    from generativedensification_amd import _lib as L

    total, _, H, D = qkv.shape
    a, lib = _args(qkv, cu_t.numel() - 1, max_seqlen, scale), L.load()
    assert lib.gdr_attn_lse_bytes(C.byref(a)) == 4 * H * total
    out = torch.empty(total, H, D, dtype=qkv.dtype, device=DEV) if out is None else out
    lse = torch.full((H, total), float("nan"), dtype=torch.float32, device=DEV) if lse is None else lse
    L.check(lib.gdr_attn_forward(C.byref(a), qkv.data_ptr(), (C.c_int64 * 4)(*qkv.stride()), cu_t.data_ptr(), out.data_ptr(),
                                 lse.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "gdr_attn_forward")
    torch.cuda.synchronize()
    return out, lse


def _c_backward(qkv, cu_t, max_seqlen, scale, dout, out, lse, dqkv):
    """gdr_attn_backward itself, into `dqkv`"""
    from generativedensification_amd import _lib as L

    a = _args(qkv, cu_t.numel() - 1, max_seqlen, scale)
    L.check(L.load().gdr_attn_backward(C.byref(a), dout.data_ptr(), (C.c_int64 * 3)(*dout.stride()), qkv.data_ptr(),
                                       (C.c_int64 * 4)(*qkv.stride()), cu_t.data_ptr(), out.data_ptr(), lse.data_ptr(),
                                       dqkv.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "gdr_attn_backward")
    torch.cuda.synchronize()
    return dqkv


def _report(what, got, truth, pt, dtype):
    err_hip = float((got.double() - truth).abs().max())
    err_pt = float((pt.double() - truth).abs().max())
    limit = AC.bar(err_pt, dtype, truth)
    print(f"{what}: err_hip {err_hip:.3e} err_pt {err_pt:.3e} ratio {err_hip / err_pt if err_pt else float('inf'):.3f} "
          f"ulp {AC.ulp(dtype, float(truth.abs().max())):.3e} bar {limit:.3e}")
    return err_hip, limit


@pytest.mark.parametrize("name,dt", AC.CASES)
def test_forward_lse_and_gradients_against_f64_on_symmetry_breaking_inputs(name, dt):
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
    o2, lse = _c_forward(case["qkv"], case["cu_t"], case["max_seqlen"], case["scale"])
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


# ---- max_seqlen is a hint: it picks the row tile (RP = 64, 128 or 256 rows per head) and nothing of the arithmetic ----------
HINTS = {name: (64, 100, 128, 129, 256) for name in AC.TIERS if name.startswith("t64_")}
HINTS.update({name: (128, 200, 256) for name in AC.TIERS if name.startswith("t128_")})
HINTS["ref48_h20_d8"] = (48, 64, 65, 256)


@pytest.mark.parametrize("name,dt", [(name, dt) for name in HINTS for dt in AC.DTYPES])
def test_any_upper_bound_for_max_seqlen_gives_the_same_bits(name, dt):
    """The key loop runs over the sequence's own length and the sweeps of the backward over its own rows; the row tile only
    places rows in LDS.  So out, lse and dqkv under every larger hint equal those under the case's own, bit for bit: the
    kernels of the three row tiles are compared with each other, with no tolerance."""
    case = AC.make(name, AC.DTYPES[dt], DEV)
    hints = HINTS[name]
    assert hints[0] == case["max_seqlen"] and {AC.row_tile(m) for m in hints} == {rp for rp in (64, 128, 256) if rp >= hints[0]}
    out, dqkv = _hip(case)
    _, lse = _c_forward(case["qkv"], case["cu_t"], hints[0], case["scale"])
    assert float(out.float().abs().max()) > 0 and float(dqkv.float().abs().max()) > 0
    differ = 0
    for m in hints[1:]:
        out_m, dqkv_m = _hip(case, max_seqlen=m)
        o_m, lse_m = _c_forward(case["qkv"], case["cu_t"], m, case["scale"])
        assert torch.equal(o_m, out_m)
        differ += AC.bits_differ(f"out at max_seqlen {m}", out_m, out) + AC.bits_differ(f"lse at max_seqlen {m}", lse_m, lse)
        for i, w in enumerate(("dq", "dk", "dv")):
            differ += AC.bits_differ(f"{w} at max_seqlen {m}", dqkv_m[:, i], dqkv[:, i])
    assert differ == 0, (name, dt)


@pytest.mark.parametrize("dt", list(AC.DTYPES))
@pytest.mark.parametrize("name,Lq", [("t64_h5_d16", 64), ("t64_h5_d64", 64), ("t128_h5_d16", 128), ("t128_h5_d64", 128)])
def test_fixed_length_entry_point_with_full_tiles_equals_the_varlen_call_bit_for_bit(name, Lq, dt):
    """(B, L) = (3, 64) and (3, 128), H = 5: every lane of the tile is live and the last workgroup of a sequence has dead heads"""
    from flash_attn import flash_attn_qkvpacked_func, flash_attn_varlen_qkvpacked_func

    case = AC.make(name, AC.DTYPES[dt], DEV)
    B, (H, D) = 3, case["qkv"].shape[2:]
    assert H == 5 and case["qkv"].shape[0] >= B * Lq
    rows, dout = case["qkv"][:B * Lq], case["dout"][:B * Lq]
    cu_t = torch.arange(B + 1, dtype=torch.int32, device=DEV) * Lq
    qkv = rows.detach().requires_grad_(True)
    out = flash_attn_varlen_qkvpacked_func(qkv, cu_t, Lq, softmax_scale=case["scale"])
    out.backward(dout)
    q5 = rows.reshape(B, Lq, 3, H, D).detach().requires_grad_(True)
    out5 = flash_attn_qkvpacked_func(q5, softmax_scale=case["scale"])
    assert out5.shape == (B, Lq, H, D)
    out5.backward(dout.reshape(B, Lq, H, D))
    assert torch.equal(out5.reshape(-1, H, D), out) and torch.equal(q5.grad.reshape(-1, 3, H, D), qkv.grad)
    assert float(out.detach().float().abs().max()) > 0 and float(qkv.grad.float().abs().max()) > 0
    assert bool(out.detach()[-1].any()) and bool(qkv.grad[-1].any())            # the tile's last row is there


@pytest.mark.parametrize("dt", list(AC.DTYPES))
@pytest.mark.parametrize("name,hint,lengths", [("t256_h3_d8", 64, (10, 70, 0, 5)), ("t256_h3_d32", 64, (10, 70, 0, 5)),
                                               ("t256_h5_d16", 128, (7, 130, 20)), ("t256_h5_d64", 128, (7, 130, 20))])
def test_a_sequence_longer_than_max_seqlen_is_cut_at_the_tile_and_its_further_rows_are_not_written(name, hint, lengths, dt):
    """What the header of attention.py says of a hint that is too small, through the C entry points into buffers filled with
    a sentinel: the first RP rows of the long sequence are, bit for bit, a call on those RP tokens alone; its further rows keep
    the sentinel in out, lse and dqkv; every other sequence (and the rows behind the last) equals the call whose hint is large
    enough."""
    dtype = AC.DTYPES[dt]
    case = AC.make(name, dtype, DEV)
    cu = AC.cu_of(lengths)
    total, long = cu[-1] + 2, max(range(len(lengths)), key=lengths.__getitem__)
    a, b = cu[long], cu[long + 1]
    assert hint == AC.row_tile(hint) < b - a <= 256 and all(n <= hint for i, n in enumerate(lengths) if i != long)
    qkv, dout, scale = case["qkv"][:total], case["dout"][:total], case["scale"]
    cu_t = torch.tensor(cu, dtype=torch.int32, device=DEV)
    H, D = qkv.shape[2:]
    SENT, SENT_LSE = -1234.0, -7777.0

    def run(rows, drows, cu_rows, max_seqlen):
        n = rows.shape[0]
        out = torch.full((n, H, D), SENT, dtype=dtype, device=DEV)
        lse = torch.full((H, n), SENT_LSE, dtype=torch.float32, device=DEV)
        dqkv = torch.full((n, 3, H, D), SENT, dtype=dtype, device=DEV)
        _c_forward(rows, cu_rows, max_seqlen, scale, out, lse)
        return out, lse, _c_backward(rows, cu_rows, max_seqlen, scale, drows, out, lse, dqkv)

    out, lse, dqkv = run(qkv, dout, cu_t, hint)
    whole = run(qkv, dout, cu_t, 256)
    alone = run(qkv[a:a + hint], dout[a:a + hint], torch.tensor([0, hint], dtype=torch.int32, device=DEV), hint)
    for what, got, full, cut in zip(("out", "lse", "dqkv"), (out, lse.t(), dqkv), (whole[0], whole[1].t(), whole[2]),
                                    (alone[0], alone[1].t(), alone[2])):
        sentinel = torch.full_like(got[a + hint:b], SENT_LSE if what == "lse" else SENT)
        assert torch.equal(got[a:a + hint], cut) and bool(cut.any()), what
        assert torch.equal(got[a + hint:b], sentinel) and not torch.equal(full[a + hint:b], sentinel), what
        assert torch.equal(got[:a], full[:a]) and torch.equal(got[b:], full[b:]) and bool(full[:a].any()), what
        assert not got[cu[-1]:].any(), what


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
