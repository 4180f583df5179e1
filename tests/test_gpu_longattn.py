"""GPU: the tiled MFMA attention (generativedensification_amd/vitattn.py, csrc/attn_tiled.hip) on the cases of
tests/longattn_cases.py: out, lse, dq, dk and dv against the f64 restatement (tests/attn_ref.py) at the project's bar
(tests/attn_cases.py `bar`: err <= 2 err_torch + ulp, err_torch from torch's own half composition on the same device); what
must hold bit for bit (two runs, a batch against its first image, every layout against the dense one, three tensors against
the packed one, NaN around a sliced operand, guard bands behind every output); and `vit_attention_forward` bound to a mirror
of timm's Attention (tests/vitattn_ref.py) against an f64 run of the same module, with every fall-back of `covers`."""
import copy
import ctypes as C
import functools

import pytest
import torch

import attn_cases as AC
import longattn_cases as LC
import vitattn_ref as VR
from generativedensification_amd import vitattn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(case, packed=None):
    """forward + backward of a case -> dict(out, lse, dq, dk, dv); `packed`: through attn_tiled_qkvpacked (default: wherever
    the layout has a packed tensor)"""
    packed = case["qkv"] is not None if packed is None else packed
    if packed:
        leaf = case["qkv"].detach().requires_grad_(True)
        out = vitattn.attn_tiled_qkvpacked(leaf, case["scale"])
    else:
        leaves = [case[w].detach().requires_grad_(True) for w in "qkv"]
        out = vitattn.attn_tiled(*leaves, case["scale"])
    lse = out.grad_fn.saved_tensors[4]      # (q, k, v, out, lse) of the autograd node
    out.backward(case["dout"])
    if packed:
        assert leaf.grad.shape == case["qkv"].shape
        dq, dk, dv = leaf.grad.unbind(2)
    else:
        dq, dk, dv = (t.grad for t in leaves)
    return dict(out=out.detach(), lse=lse, dq=dq, dk=dk, dv=dv)


@functools.lru_cache(maxsize=None)
def _dense(name, dt):
    """the result of a case in the packed dense layout: computed once, compared against bit for bit, never written to"""
    return _run(LC.make(name, LC.DTYPES[dt], DEV, layout="packed"))


def _same_bits(a, b):
    return [w for w in ("out", "lse", "dq", "dk", "dv") if AC.bits_differ(w, a[w], b[w])]


@pytest.mark.parametrize("name,dt", LC.CASES)
def test_accuracy_against_the_f64_restatement_at_the_projects_bar(name, dt):
    got = _run(LC.make(name, LC.DTYPES[dt], DEV))
    assert got["out"].shape == (LC.SHAPES[name][0], LC.SHAPES[name][1], LC.SHAPES[name][2], LC.D)
    assert got["out"].dtype == LC.DTYPES[dt] and got["lse"].dtype == torch.float32
    assert LC.judge(name, dt, got, LC.torch_errors(name, dt, DEV)) == []


@pytest.mark.parametrize("name,dt", [("l129", "bf16"), ("l257", "fp16"), ("vit1025", "bf16")])
def test_two_runs_are_bitwise_equal(name, dt):
    case = LC.make(name, LC.DTYPES[dt], DEV, layout="packed")
    assert _same_bits(_run(case), _dense(name, dt)) == []


@pytest.mark.parametrize("name,dt", [("l65", "bf16"), ("l129", "fp16"), ("l257", "bf16")])
def test_the_first_image_of_a_batch_does_not_depend_on_the_rest(name, dt):
    case = LC.make(name, LC.DTYPES[dt], DEV, layout="packed")
    assert case["B"] > 1
    first = dict(case, qkv=case["qkv"][:1].contiguous(), dout=case["dout"][:1].contiguous())
    alone, batch = _run(first), _dense(name, dt)
    assert _same_bits(alone, {w: t[:1] for w, t in batch.items()}) == []


@pytest.mark.parametrize("layout", LC.LAYOUTS)
@pytest.mark.parametrize("name,dt", [("l17", "fp16"), ("l129", "bf16"), ("l193", "fp16")])
def test_every_layout_gives_the_bits_of_the_dense_one(name, dt, layout):
    """the sliced and misaligned layouts are surrounded by NaN: the result is finite and unchanged"""
    case = LC.make(name, LC.DTYPES[dt], DEV, layout=layout)
    got = _run(case)
    assert all(bool(torch.isfinite(t).all()) for t in got.values())
    assert _same_bits(got, _dense(name, dt)) == []
    if case["qkv"] is not None:      # three tensors (views of the packed one) against the packed entry point
        assert _same_bits(_run(case, packed=False), got) == []


def test_rows_are_read_in_place_where_they_are_aligned_and_copied_where_not():
    for layout, in_place in (("packed", True), ("linear", True), ("sliced", True), ("misaligned", False)):
        case = LC.make("l17", torch.bfloat16, DEV, layout=layout)
        assert (vitattn._rows(case["q"]).data_ptr() == case["q"].data_ptr()) == in_place, layout
        assert (vitattn._rows(case["dout"]).data_ptr() == case["dout"].data_ptr()) == in_place, layout


def test_guard_bands_behind_every_output_are_untouched():
    from generativedensification_amd import _lib as L
    from generativedensification_amd import _marshal as M

    lib = L.load()
    name, dt, G = "l129", "bf16", 4096
    case = LC.make(name, LC.DTYPES[dt], DEV, layout="packed")
    B, Lq, H = case["B"], case["L"], case["H"]
    a = L.GdrAttnTiledArgs()
    a.B, a.L, a.H, a.D, a.dtype, a.scale = B, Lq, H, LC.D, L.GDR_DTYPES[dt.replace("fp", "f")], LC.D ** -0.5
    n = B * Lq * H * LC.D

    def guarded(numel, dtype):
        return torch.full((numel + G,), -7.0, dtype=dtype, device=DEV)

    out, out_lo, dqkv = guarded(n, case["q"].dtype), guarded(n, case["q"].dtype), guarded(3 * n, case["q"].dtype)
    lse, scratch = guarded(B * H * Lq, torch.float32), guarded(B * H * Lq, torch.float32)
    q, k, v = case["q"], case["k"], case["v"]
    dense = (C.c_int64 * 4)(Lq * H * LC.D, H * LC.D, LC.D, 1)
    L.check(lib.gdr_attn_tiled_forward(C.byref(a), q.data_ptr(), vitattn._strides(q), k.data_ptr(), vitattn._strides(k),
                                       v.data_ptr(), vitattn._strides(v), out.data_ptr(), out_lo.data_ptr(), lse.data_ptr(),
                                       M.stream()), "forward")
    grads = dqkv[:3 * n].view(B, Lq, 3, H, LC.D).unbind(2)
    L.check(lib.gdr_attn_tiled_backward(C.byref(a), case["dout"].data_ptr(), dense, q.data_ptr(), vitattn._strides(q),
                                        k.data_ptr(), vitattn._strides(k), v.data_ptr(), vitattn._strides(v), out.data_ptr(),
                                        out_lo.data_ptr(), lse.data_ptr(), *(x for g in grads for x in (g.data_ptr(), vitattn._strides(g))),
                                        scratch.data_ptr(), M.stream()), "backward")
    for what, t, used in (("out", out, n), ("out_lo", out_lo, n), ("dqkv", dqkv, 3 * n), ("lse", lse, B * H * Lq), ("scratch", scratch, B * H * Lq)):
        assert bool((t[used:] == -7.0).all()), what
        assert not bool((t[:used] == -7.0).all()), what
    want = _dense(name, dt)
    got = dict(out=out[:n].view(B, Lq, H, LC.D), lse=lse[:B * H * Lq].view(B, H, Lq), dq=grads[0], dk=grads[1], dv=grads[2])
    assert _same_bits(got, want) == []


# ---- the bound module ------------------------------------------------------------------------------------------------------

def _module_run(m, x, dy, fn, autocast=True):
    """forward + backward of fn(m, x) -> [out, dx, d qkv.weight, d qkv.bias, d proj.weight, d proj.bias]"""
    m.zero_grad(set_to_none=True)
    x = x.detach().clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        out = fn(m, x)
    out.backward(dy.to(out.dtype))
    return [out.detach(), x.grad] + [p.grad.clone() for p in (m.qkv.weight, m.qkv.bias, m.proj.weight, m.proj.bias)]


NAMES = ("out", "dx", "d qkv.weight", "d qkv.bias", "d proj.weight", "d proj.bias")


@pytest.mark.parametrize("N", [65, 197])
def test_bound_forward_against_an_f64_run_of_the_same_module(N, monkeypatch):
    monkeypatch.setattr(vitattn, "VITATTN_BACKEND", "hip")
    m = VR.make(128, 2, seed=11).to(DEV)
    x, dy = (t.to(DEV) for t in VR.inputs(2, N, 128, seed=12 + N))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert vitattn.covers(m, x)
    truth = _module_run(copy.deepcopy(m).double(), x.double(), dy.double(), VR.Attention.forward, autocast=False)
    torch_ = _module_run(m, x, dy, VR.Attention.forward)
    hip = _module_run(m, x, dy, vitattn.vit_attention_forward)
    bad = []
    for what, t, pt, got in zip(NAMES, truth, torch_, hip):
        assert got.dtype == pt.dtype and got.shape == pt.shape
        err_pt, err = float((pt.double() - t).abs().max()), float((got.double() - t).abs().max())
        limit = AC.bar(err_pt, got.dtype, t)
        print(f"N={N} {what}: err {err:.3e}  torch {err_pt:.3e}  bar {limit:.3e}  ratio {err / limit:.2f}")
        if not err <= limit:
            bad.append(what)
    assert bad == []


def test_every_fall_back_of_covers_returns_torchs_bits(monkeypatch):
    monkeypatch.setattr(vitattn, "VITATTN_BACKEND", "hip")
    x, dy = (t.to(DEV) for t in VR.inputs(2, 65, 128, seed=21))
    mask = torch.rand(65, 65, device=DEV) > 0.2

    def check(m, autocast=True, mask=None, covered=False):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            assert vitattn.covers(m, x, mask) == covered
        torch.manual_seed(5)
        want = _module_run(m, x, dy, lambda mod, t: VR.Attention.forward(mod, t, mask), autocast)
        torch.manual_seed(5)
        got = _module_run(m, x, dy, lambda mod, t: vitattn.vit_attention_forward(mod, t, mask), autocast)
        return [w for w, a, b in zip(NAMES, want, got) if not torch.equal(a, b)]

    plain = VR.make(128, 2, seed=22).to(DEV)
    assert check(plain, mask=mask) == []                                     # a mask
    assert check(plain, autocast=False) == []                                # float32 projection
    assert check(VR.make(128, 4, seed=23).to(DEV)) == []                     # head_dim 32
    assert check(VR.make(128, 2, seed=24, qk_norm=True).to(DEV)) == []       # q_norm / k_norm
    assert check(VR.make(128, 2, seed=25, attn_drop=0.1).to(DEV).train()) == []      # dropout, training
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert vitattn.covers(VR.make(128, 2, seed=25, attn_drop=0.1).to(DEV).eval(), x)     # ... but not in eval
        assert vitattn.covers(plain.half(), x.half()) and vitattn.covers(plain, x)
    monkeypatch.setattr(vitattn, "VITATTN_BACKEND", "torch")
    assert check(VR.make(128, 2, seed=22).to(DEV)) == []                     # the backend switch
    monkeypatch.setattr(vitattn, "VITATTN_BACKEND", "hip")
    assert check(VR.make(128, 2, seed=22).to(DEV), covered=True) != []       # the fused path is another computation
