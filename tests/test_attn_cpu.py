"""CPU: the plain-torch attention restatement (tests/attn_ref.py) against autograd; mutants of it against the inputs of
tests/attn_cases.py at the bars the GPU test applies; the (D, row tile, dtype) kernels the case table selects, and the room a
model of a correct kernel leaves under the bar on the tile cases; `padded_patches` on hand-worked examples; the `flash_attn` drop-in's
names, signatures and argument errors; the gdr_attn_* exports and their refusals."""
import ctypes as C
import functools
import inspect
import itertools
import os

import pytest
import torch

import attn_cases as AC
import attn_ref as R


def _truth(case, mut=None):
    """f64 (out, lse, dqkv) of the restatement on the half-rounded inputs of a case."""
    qkv, dout, rp = case["qkv"].double(), case["dout"].double(), AC.row_tile(case["max_seqlen"])
    out, lse = R.attention(qkv, case["cu"], case["scale"], mut=mut, rp=rp)
    return out, lse, R.attention_backward(qkv, case["cu"], dout, case["scale"], mut=mut, rp=rp)


@functools.lru_cache(maxsize=None)
def _judged(name, dt):
    """a case with what every judgement of it needs, computed once and left unchanged: the case, its f64 truth, and per tensor
    (out, dq, dk, dv) the pair (truth, bar), the bar of test_gpu_attn.py built from the torch half composition run on the CPU"""
    dtype = AC.DTYPES[dt]
    case = AC.make(name, dtype)
    out, lse, dqkv = _truth(case)
    pt_out, pt_dqkv = AC.torch_composition(case["qkv"], case["cu"], case["scale"], case["dout"])
    pairs = [("out", out, pt_out)] + [("dqkv"[0] + "qkv"[i], dqkv[:, i], pt_dqkv[:, i]) for i in range(3)]
    bars = {what: (t, AC.bar(float((pt.double() - t).abs().max()), dtype, t)) for what, t, pt in pairs}
    return case, (out, lse, dqkv), bars


def _beyond(name, dt, mut):
    """the tensors of a case in which the mutant misses the truth by more than the bar"""
    case, (out, lse, dqkv), bars = _judged(name, dt)
    out_m, lse_m, dqkv_m = _truth(case, mut)
    got = {"out": out_m, "dq": dqkv_m[:, 0], "dk": dqkv_m[:, 1], "dv": dqkv_m[:, 2]}
    hits = [(name, dt, what) for what, (t, limit) in bars.items() if float((got[what] - t).abs().max()) > limit]
    pt_lse = AC.f32_lse(case["qkv"], case["cu"], case["scale"])
    if float((lse_m - lse).abs().max()) > AC.bar(float((pt_lse.double() - lse).abs().max()), torch.float32, lse):
        hits.append((name, dt, "lse"))
    return hits


@pytest.mark.parametrize("name", ["mixed_h3_d8", "mixed_h5_d16_scaled", "short_h1_d8"])
def test_closed_form_backward_equals_autograd_through_the_forward(name):
    case = AC.make(name, torch.float16)
    qkv = case["qkv"].double().requires_grad_(True)
    out, lse = R.attention(qkv, case["cu"], case["scale"])
    out.backward(case["dout"].double())
    closed = R.attention_backward(qkv.detach(), case["cu"], case["dout"].double(), case["scale"])
    assert float(closed.abs().max()) > 0
    assert float((closed - qkv.grad).abs().max()) <= 1e-12 * float(closed.abs().max())
    tail = case["cu"][-1]
    assert not out[tail:].any() and not lse[:, tail:].any() and not closed[tail:].any()
    # softmax rows sum to one: exp(s - lse) does
    a, b = case["cu"][0], case["cu"][1]
    h = qkv.shape[2] - 1
    s = (qkv[a:b, 0, h] @ qkv[a:b, 1, h].t()).detach() * (case["scale"] or qkv.shape[-1] ** -0.5)
    assert torch.allclose(torch.exp(s - lse[h, a:b, None].detach()).sum(1), torch.ones(b - a, dtype=torch.float64), atol=1e-12)


def test_hot_head_overflows_f32_without_max_subtraction_and_has_one_key_rows():
    case = AC.make("mixed_h3_d8", torch.bfloat16)
    qkv = case["qkv"].float()
    a, b = case["cu"][7], case["cu"][8]      # the 256-token sequence
    s = (qkv[a:b, 0, 0] @ qkv[a:b, 1, 0].t()) * 8 ** -0.5
    assert float(s.max()) > 100 and float(s.max() - s.min()) > 150
    assert not torch.isfinite(torch.exp(s).sum(1)).all()
    assert float(torch.softmax(s.double(), 1).max(1).values.max()) > 1 - 1e-12


@pytest.mark.parametrize("mut", R.MUTANTS)
def test_every_mutant_is_beyond_the_gpu_bars_on_some_case(mut):
    """The bar of test_gpu_attn.py, built here from the SAME torch half composition run on the CPU: a mutant must miss the
    truth by more than 2 err_pt + ulp in at least one tensor of at least one case.  A mistake of the row tile (R.TILE_MUTANTS)
    must be that far off on one of the tile cases (AC.TIERS) of EVERY head dimension, since each D is a kernel of its own."""
    caught = []
    for name, dt in AC.CASES:
        caught = _beyond(name, dt, mut)
        if caught:
            break
    assert caught, mut
    if mut in R.TILE_MUTANTS:
        tiles = (64, 128) if mut == "group_reads_first_head" else (64, 128, 256)     # (one head per workgroup at RP = 256)
        by_kernel = {}
        for name in AC.TIERS:
            key = (AC.SHAPES[name][1], AC.row_tile(AC.max_seqlen(name)))
            for dt in AC.DTYPES:
                hits = _beyond(name, dt, mut)
                if hits and key not in by_kernel:
                    by_kernel[key] = hits
        for key in sorted(by_kernel):
            print(f"{mut}: D = {key[0]}, RP = {key[1]} caught by {by_kernel[key][0][:2]} in {[h[2] for h in by_kernel[key]]}")
        assert {k for k in by_kernel if k[1] in tiles} == set(itertools.product((8, 16, 32, 64), tiles)), (mut, by_kernel)


def test_the_case_table_reaches_every_head_dim_row_tile_and_dtype():
    """a (D, RP, dtype) is a kernel of its own, forward and backward: the cases, each at its own max_seqlen, select all 24"""
    reached = {(AC.SHAPES[name][1], AC.row_tile(AC.make(name, AC.DTYPES[dt])["max_seqlen"]), dt) for name, dt in AC.CASES}
    assert reached == set(itertools.product((8, 16, 32, 64), (64, 128, 256), AC.DTYPES))
    # ... and the tile cases alone do, with a full tile, one a row short of it and the smallest it holds (0 for the first tile)
    tiers = {(AC.SHAPES[n][1], AC.row_tile(AC.max_seqlen(n))) for n in AC.TIERS}
    assert tiers == set(itertools.product((8, 16, 32, 64), (64, 128, 256))) and len(AC.TIERS) == 12
    for name in AC.TIERS:
        H, _, lengths, *_ = AC.SHAPES[name]
        rp = AC.row_tile(max(lengths))
        assert {rp, rp - 1, rp // 2 + 1 if rp > 64 else 1, 0} <= set(lengths) and H % 2 and sum(lengths) <= 843
    for tier in ("t64_", "t128_", "t256_"):      # both values of every other setting under every tile
        rows = [AC.SHAPES[n] for n in AC.TIERS if n.startswith(tier)]
        assert {r[3] is None for r in rows} == {True, False} and {r[5] for r in rows} == {"dense", "sliced"}
        assert {r[4] == 0 for r in rows} == {True, False}


@pytest.mark.parametrize("name", AC.TIERS)
def test_a_correct_kernel_leaves_room_under_the_bar_on_every_tile_case(name):
    """A condition on the INPUTS, not a tolerance on the kernel: R.kernel_model (f32 arithmetic, out rounded to the dtype, delta
    from the rounded out, gradients rounded once) must stay within 0.8 of the bar in out, dQ, dK and dV, so that a correct
    kernel that only sums in another order is not a coin flip against the bar on the GPU.  dQ is the tensor that crowds it:
    delta comes from the rounded result.  A case over the cap gets another length order, never a wider cap."""
    worst = 0.0
    for dt in AC.DTYPES:
        case, _, bars = _judged(name, dt)
        out, dqkv = R.kernel_model(case["qkv"], case["cu"], case["dout"], case["scale"])
        dqkv = dqkv.to(AC.DTYPES[dt])
        got = {"out": out, "dq": dqkv[:, 0], "dk": dqkv[:, 1], "dv": dqkv[:, 2]}
        shares = {what: float((got[what].double() - t).abs().max()) / limit for what, (t, limit) in bars.items()}
        print(f"{name} {dt}: share of the bar " + " ".join(f"{w} {s:.2f}" for w, s in shares.items()))
        worst = max(worst, *shares.values())
    assert worst <= 0.8, (name, worst)


def test_padded_patches_on_hand_worked_examples():
    pad, unpad, cu = R.padded_patches([4], 4)            # exactly one patch
    assert pad.tolist() == [0, 1, 2, 3] and unpad.tolist() == [0, 1, 2, 3] and cu.tolist() == [0, 4]
    pad, unpad, cu = R.padded_patches([5], 4)            # patch + 1: the second sequence repeats tokens 1..3 of the first
    assert pad.tolist() == [0, 1, 2, 3, 4, 1, 2, 3] and unpad.tolist() == [0, 1, 2, 3, 4] and cu.tolist() == [0, 4, 8]
    pad, unpad, cu = R.padded_patches([3], 4)            # below the patch: one short sequence, nothing repeated
    assert pad.tolist() == [0, 1, 2] and unpad.tolist() == [0, 1, 2] and cu.tolist() == [0, 3]
    # three samples of 6, 2 and 9 points: 8 + 2 + 12 padded slots
    pad, unpad, cu = R.padded_patches([6, 8, 17], 4)
    assert pad.tolist() == [0, 1, 2, 3, 4, 5, 2, 3] + [6, 7] + [8, 9, 10, 11, 12, 13, 14, 15, 16, 13, 14, 15]
    assert unpad.tolist() == [0, 1, 2, 3, 4, 5] + [8, 9] + [10, 11, 12, 13, 14, 15, 16, 17, 18]
    assert cu.tolist() == [0, 4, 8, 10, 14, 18, 22] and cu.dtype == torch.int32
    assert torch.equal(pad[unpad], torch.arange(17))     # unpad inverts pad on the points
    pad, unpad, cu = R.padded_patches([48 * 3], 48)
    assert torch.equal(pad, torch.arange(144)) and cu.tolist() == [0, 48, 96, 144]


def test_dropin_package_names_signatures_and_version():
    import flash_attn
    from flash_attn import flash_attn_interface as FI

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert flash_attn.__file__.startswith(root) and flash_attn.__version__.startswith("2.")
    assert flash_attn.flash_attn_varlen_qkvpacked_func is FI.flash_attn_varlen_qkvpacked_func
    assert flash_attn.flash_attn_qkvpacked_func is FI.flash_attn_qkvpacked_func

    def sig(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]

    E = inspect.Parameter.empty
    common = [("dropout_p", 0.0), ("softmax_scale", None), ("causal", False), ("window_size", (-1, -1)), ("softcap", 0.0),
              ("alibi_slopes", None), ("deterministic", False), ("return_attn_probs", False)]
    assert sig(flash_attn.flash_attn_varlen_qkvpacked_func) == [("qkv", E), ("cu_seqlens", E), ("max_seqlen", E)] + common
    assert sig(flash_attn.flash_attn_qkvpacked_func) == [("qkv", E)] + common
    src = open(os.path.join(root, "generativedensification_amd", "attention.py")).read()
    assert "oracle" not in src


def test_unsupported_arguments_raise_naming_the_argument_and_cpu_tensors_have_no_fallback():
    from flash_attn import flash_attn_qkvpacked_func, flash_attn_varlen_qkvpacked_func

    qkv = torch.zeros(10, 3, 2, 8, dtype=torch.float16)
    cu = torch.tensor([0, 4, 10], dtype=torch.int32)
    for kw, word in ((dict(dropout_p=0.1), "dropout_p"), (dict(causal=True), "causal"), (dict(window_size=(4, 4)), "window_size"),
                     (dict(softcap=1.0), "softcap"), (dict(alibi_slopes=torch.zeros(2)), "alibi_slopes"),
                     (dict(return_attn_probs=True), "return_attn_probs")):
        with pytest.raises(NotImplementedError, match=word):
            flash_attn_varlen_qkvpacked_func(qkv, cu, 6, **kw)
        with pytest.raises(NotImplementedError, match=word):
            flash_attn_qkvpacked_func(qkv.reshape(2, 5, 3, 2, 8), **kw)
    with pytest.raises(RuntimeError, match="fp16 or bf16"):
        flash_attn_varlen_qkvpacked_func(qkv.float(), cu, 6)
    with pytest.raises(ValueError, match=r"\(8, 16, 32, 64\)"):
        flash_attn_varlen_qkvpacked_func(torch.zeros(10, 3, 2, 24, dtype=torch.float16), cu, 6)
    with pytest.raises(ValueError, match="256"):
        flash_attn_varlen_qkvpacked_func(qkv, cu, 257)
    with pytest.raises(ValueError, match="256"):
        flash_attn_qkvpacked_func(torch.zeros(1, 300, 3, 2, 8, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        flash_attn_varlen_qkvpacked_func(qkv, cu.long(), 6)
    with pytest.raises(ValueError):
        flash_attn_varlen_qkvpacked_func(qkv[:, :2], cu, 6)
    # inside the envelope the call goes on to the refusal of CPU tensors: dropout_p=0 as the reference passes in eval
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        flash_attn_varlen_qkvpacked_func(qkv, cu, max_seqlen=6, dropout_p=0, softmax_scale=0.3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        flash_attn_qkvpacked_func(qkv.bfloat16().reshape(2, 5, 3, 2, 8), deterministic=True)


def test_library_exports_the_attention_entry_points_and_refuses_bad_arguments_without_a_gpu():
    from generativedensification_amd import _lib as L

    lib = L.load()
    for n in ("gdr_attn_lse_bytes", "gdr_attn_forward", "gdr_attn_backward"):
        assert hasattr(lib, n) and n in L.EXPORTED_SYMBOLS
    assert lib.gdr_abi_version() == 17

    def args(**kw):
        a = L.GdrAttnArgs()
        a.total, a.batch, a.H, a.D, a.max_seqlen, a.fixed_len, a.dtype, a.scale = 1000, 20, 20, 8, 48, 0, L.GDR_ATTN_F16, 0.35
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    st4, st3 = (C.c_int64 * 4)(480, 160, 8, 1), (C.c_int64 * 3)(160, 8, 1)
    fake = 0x10000000          # never dereferenced: every call below is refused before any device work
    assert lib.gdr_attn_lse_bytes(C.byref(args())) == 20 * 1000 * 4
    assert lib.gdr_attn_lse_bytes(None) == 0
    for kw, word in ((dict(D=24), b"8, 16, 32 or 64"), (dict(D=128), b"8, 16, 32 or 64"), (dict(max_seqlen=257), b"256"),
                     (dict(max_seqlen=0), b"256"), (dict(H=0), b"H"), (dict(dtype=2), b"dtype"), (dict(total=-1), b"negative"),
                     (dict(scale=float("nan")), b"finite"), (dict(scale=float("inf")), b"finite")):
        a = args(**kw)
        assert lib.gdr_attn_lse_bytes(C.byref(a)) == 0 and word in lib.gdr_last_error(), kw
        assert lib.gdr_attn_forward(C.byref(a), fake, st4, fake, fake, fake, None) == -1 and word in lib.gdr_last_error(), kw
        assert lib.gdr_attn_backward(C.byref(a), fake, st3, fake, st4, fake, fake, fake, fake, None) == -1, kw
    a = args()
    assert lib.gdr_attn_forward(None, fake, st4, fake, fake, fake, None) == -1
    assert lib.gdr_attn_forward(C.byref(a), None, st4, fake, fake, fake, None) == -1 and b"NULL" in lib.gdr_last_error()
    assert lib.gdr_attn_forward(C.byref(a), fake, None, fake, fake, fake, None) == -1
    assert lib.gdr_attn_forward(C.byref(a), fake, st4, fake, None, fake, None) == -1
    assert lib.gdr_attn_forward(C.byref(a), fake, st4, fake, fake + 2, fake, None) == -1 and b"unaligned" in lib.gdr_last_error()
    assert lib.gdr_attn_backward(C.byref(a), None, st3, fake, st4, fake, fake, fake, fake, None) == -1
    assert lib.gdr_attn_backward(C.byref(a), fake, st3, fake, st4, fake, fake, None, fake, None) == -1
    # without cu_seqlens the implied boundaries must fit: fixed_len <= max_seqlen, batch * fixed_len <= total
    assert lib.gdr_attn_forward(C.byref(args(fixed_len=49)), fake, st4, None, fake, fake, None) == -1
    assert lib.gdr_attn_forward(C.byref(args(fixed_len=48, batch=21)), fake, st4, None, fake, fake, None) == -1
    assert b"exceeds total" in lib.gdr_last_error()
