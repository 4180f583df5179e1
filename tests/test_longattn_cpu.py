"""CPU: the gdr_attn_tiled_* exports and every refusal of their envelope with fake pointers; the Python refusals of
generativedensification_amd/vitattn.py; its `covers` predicate and fall-back on CPU tensors; and the cases of
tests/longattn_cases.py against a CPU model of a correct tiled kernel (inside the bars the GPU test applies) and two broken
ones (each beyond a bar on at least one case, so the cases are known to be able to fail)."""
import ctypes as C
import functools

import pytest
import torch

import longattn_cases as LC
import vitattn_ref as VR
from generativedensification_amd import vitattn


@functools.lru_cache(maxsize=None)
def _err_pt(name, dt):
    return LC.torch_errors(name, dt)


def test_library_exports_the_tiled_attention_and_refuses_bad_arguments_without_a_gpu():
    from generativedensification_amd import _lib as L

    lib = L.load()
    for n in ("gdr_attn_tiled_scratch_bytes", "gdr_attn_tiled_forward", "gdr_attn_tiled_backward"):
        assert hasattr(lib, n) and n in L.EXPORTED_SYMBOLS
    assert lib.gdr_abi_version() == 17
    assert L.GDR_ATTN_TILED_MAX_SEQLEN == vitattn.MAX_SEQLEN == 16384 and L.GDR_ATTN_MAX_SEQLEN == 256

    def args(**kw):
        a = L.GdrAttnTiledArgs()
        a.B, a.L, a.H, a.D, a.dtype, a.scale = 12, 1025, 12, 64, L.GDR_DTYPES["bf16"], 0.125
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    packed = (C.c_int64 * 4)(1025 * 2304, 2304, 64, 1)
    dense = (C.c_int64 * 4)(1025 * 768, 768, 64, 1)
    fake = 0x10000000          # never dereferenced: every call below is refused before any device work

    def fwd(a, q=fake, qs=packed, k=fake + 1536, ks=packed, v=fake + 3072, vs=packed, out=fake, out_lo=fake, lse=fake):
        return lib.gdr_attn_tiled_forward(a, q, qs, k, ks, v, vs, out, out_lo, lse, None)

    def bwd(a, **kw):
        p = dict(dout=fake, douts=dense, q=fake, qs=packed, k=fake, ks=packed, v=fake, vs=packed, out=fake, out_lo=None, lse=fake,
                 dq=fake, dqs=packed, dk=fake, dks=packed, dv=fake, dvs=packed, scratch=fake)
        p.update(kw)
        return lib.gdr_attn_tiled_backward(a, *p.values(), None)

    assert lib.gdr_attn_tiled_scratch_bytes(C.byref(args())) == 12 * 12 * 1025 * 4
    assert lib.gdr_attn_tiled_scratch_bytes(None) == 0
    for kw, word in ((dict(D=32), b"D must be 64"), (dict(D=128), b"D must be 64"), (dict(dtype=2), b"dtype"),
                     (dict(L=0), b"16384"), (dict(L=16385), b"16384"), (dict(B=0), b"B must"), (dict(H=0), b"H must"),
                     (dict(B=1 << 12, H=1 << 10, L=1 << 9), b"2^31"), (dict(scale=float("nan")), b"finite"),
                     (dict(scale=float("inf")), b"finite")):
        a = args(**kw)
        assert lib.gdr_attn_tiled_scratch_bytes(C.byref(a)) == 0 and word in lib.gdr_last_error(), kw
        assert fwd(C.byref(a)) == -1 and word in lib.gdr_last_error(), kw
        assert bwd(C.byref(a)) == -1 and word in lib.gdr_last_error(), kw
    a = C.byref(args())
    assert fwd(None) == -1 and bwd(None) == -1
    # the operands: NULL, a channel stride other than 1, rows off 16 bytes (the base, or a stride that is no multiple of 8)
    chan2 = (C.c_int64 * 4)(1025 * 2304, 2304, 128, 2)
    odd = (C.c_int64 * 4)(1025 * 2308, 2308, 64, 1)
    for name in ("q", "k", "v"):
        assert fwd(a, **{name: None}) == -1 and name.encode() + b": NULL" in lib.gdr_last_error()
        assert fwd(a, **{name + "s": None}) == -1 and name.encode() + b": NULL" in lib.gdr_last_error()
        assert fwd(a, **{name + "s": chan2}) == -1 and name.encode() + b": channel stride" in lib.gdr_last_error()
        assert fwd(a, **{name + "s": odd}) == -1 and name.encode() + b": rows must be 16-byte aligned" in lib.gdr_last_error()
        assert fwd(a, **{name: fake + 8}) == -1 and name.encode() + b": rows must be 16-byte aligned" in lib.gdr_last_error()
    assert fwd(a, out=None) == -1 and b"NULL" in lib.gdr_last_error()
    assert fwd(a, lse=None) == -1 and b"NULL" in lib.gdr_last_error()
    assert fwd(a, out=fake + 2) == -1 and b"unaligned" in lib.gdr_last_error()
    assert fwd(a, out_lo=fake + 2) == -1 and b"unaligned" in lib.gdr_last_error()
    for name in ("dout", "q", "k", "v", "dq", "dk", "dv"):
        assert bwd(a, **{name: None}) == -1 and name.encode() + b": NULL" in lib.gdr_last_error()
        assert bwd(a, **{name + "s": chan2}) == -1 and name.encode() + b": channel stride" in lib.gdr_last_error()
        assert bwd(a, **{name: fake + 4}) == -1 and name.encode() + b": rows must be 16-byte aligned" in lib.gdr_last_error()
    for name in ("out", "lse", "scratch"):
        assert bwd(a, **{name: None}) == -1 and b"NULL" in lib.gdr_last_error()
    assert bwd(a, scratch=fake + 2) == -1 and b"unaligned" in lib.gdr_last_error()
    assert bwd(a, out_lo=fake + 2) == -1 and b"unaligned" in lib.gdr_last_error()


def test_python_entry_points_refuse_what_is_outside_the_envelope_by_name():
    qkv = torch.zeros(2, 5, 3, 2, 64, dtype=torch.float16)
    q = qkv[:, :, 0]
    with pytest.raises(ValueError, match=r"\(batch, seqlen, 3, nheads, headdim\)"):
        vitattn.attn_tiled_qkvpacked(qkv[:, :, :2])
    with pytest.raises(ValueError, match=r"\(batch, seqlen, 3, nheads, headdim\)"):
        vitattn.attn_tiled_qkvpacked(qkv[0])
    with pytest.raises(RuntimeError, match="fp16 or bf16 only, qkv is torch.float32"):
        vitattn.attn_tiled_qkvpacked(qkv.float())
    with pytest.raises(ValueError, match="qkv: head dimension 32"):
        vitattn.attn_tiled_qkvpacked(torch.zeros(2, 5, 3, 2, 32, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="qkv: sequence length 16385"):
        vitattn.attn_tiled_qkvpacked(torch.zeros(1, 16385, 3, 1, 64, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="qkv: sequence length 0"):
        vitattn.attn_tiled_qkvpacked(qkv[:, :0])
    with pytest.raises(ValueError, match="batch and nheads"):
        vitattn.attn_tiled_qkvpacked(qkv[:0])
    with pytest.raises(ValueError, match="finite"):
        vitattn.attn_tiled_qkvpacked(qkv, softmax_scale=float("nan"))
    with pytest.raises(ValueError, match=r"k must be \(batch, seqlen, nheads, headdim\)"):
        vitattn.attn_tiled(q, qkv, q)
    with pytest.raises(ValueError, match="v must have q's shape"):
        vitattn.attn_tiled(q, q, q[:, :4])
    with pytest.raises(RuntimeError, match="k must have q's dtype"):
        vitattn.attn_tiled(q, q.bfloat16(), q)
    with pytest.raises(RuntimeError, match="q is torch.float32"):
        vitattn.attn_tiled(q.float(), q.float(), q.float())
    with pytest.raises(ValueError, match="q: head dimension 8"):
        vitattn.attn_tiled(q[..., :8], q[..., :8], q[..., :8])
    # inside the envelope the call goes on to the refusal of CPU tensors
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vitattn.attn_tiled_qkvpacked(qkv, softmax_scale=0.3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vitattn.attn_tiled(q.bfloat16(), q.bfloat16(), q.bfloat16())


def test_covers_is_false_on_cpu_tensors_and_the_bound_forward_returns_the_mirrors_bits(monkeypatch):
    monkeypatch.setattr(vitattn, "VITATTN_BACKEND", "hip")
    m = VR.make(128, 2, seed=3)
    x, dy = VR.inputs(2, 9, 128, seed=4)
    assert m.head_dim == 64 and not vitattn.covers(m, x) and not vitattn.covers(m, x.bfloat16())
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert not vitattn.covers(m, x)
    want = m(x)
    got = vitattn.vit_attention_forward(m, x)
    assert torch.equal(got, want)
    mask = torch.rand(9, 9) > 0.3
    assert torch.equal(vitattn.vit_attention_forward(m, x, mask), m(x, mask)) and not torch.equal(m(x, mask), want)
    # the binding line of INTEGRATION.md, on the mirror class
    monkeypatch.setattr(VR.Attention, "forward", vitattn.vit_attention_forward)
    x1 = x.clone().requires_grad_(True)
    out = m(x1)
    assert torch.equal(out, want)
    out.backward(dy)
    assert x1.grad is not None and bool(torch.isfinite(x1.grad).all())
    assert vitattn.VITATTN_BACKEND == "hip" and set(vitattn.__all__) >= {"attn_tiled", "attn_tiled_qkvpacked", "covers"}


def test_case_table_covers_what_the_tiles_need():
    lengths = {s[1] for s in LC.SHAPES.values()}
    assert lengths >= {1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 193, 255, 256, 257, 1025}
    assert {s[0] for s in LC.SHAPES.values()} == {1, 2, 3} and {s[2] for s in LC.SHAPES.values()} >= {1, 3, 5}
    assert {s[4] for s in LC.SHAPES.values()} == set(LC.LAYOUTS)
    assert any(s[3] is None for s in LC.SHAPES.values()) and any(s[3] is not None for s in LC.SHAPES.values())
    assert LC.SHAPES["vit1025"][:3] == (1, 1025, 2)
    for layout in LC.LAYOUTS:      # every layout holds the same values
        case = LC.make("l17", torch.bfloat16, layout=layout)
        qkv, dout = LC.values("l17", torch.bfloat16)
        for i, w in enumerate("qkv"):
            assert torch.equal(case[w], qkv[:, :, i])
        assert torch.equal(case["dout"], dout)
    # head 0 is hot: its logits span over a hundred, and one key towers
    qkv, _ = LC.values("l129", torch.float16)
    s = (qkv[0, :, 0, 0].double() @ qkv[0, :, 1, 0].double().t()) * 64 ** -0.5
    assert float(s.max() - s.min()) > 100 and int(s.softmax(-1).max(-1).indices.mode().values) == 2


@pytest.mark.parametrize("name,dt", LC.CASES)
def test_model_of_a_correct_tiled_kernel_stays_inside_the_bars(name, dt):
    assert LC.judge(name, dt, LC.tiled_model(name, dt), _err_pt(name, dt)) == []


@pytest.mark.parametrize("mut", LC.MODEL_MUTANTS)
def test_each_broken_model_is_beyond_a_bar_on_some_case(mut):
    hits = [(name, dt, what) for name, dt in LC.CASES
            for what, _, _ in LC.judge(name, dt, LC.tiled_model(name, dt, mut), _err_pt(name, dt), show=False)]
    print(mut, hits)
    assert hits
    if mut == "tail_keys_unmasked":      # only a length that is no multiple of the key tile can show it
        assert all(LC.SHAPES[name][1] % LC.KEY_TILE for name, _, _ in hits)
    else:                                # only more than one key tile
        assert all(LC.SHAPES[name][1] > LC.KEY_TILE for name, _, _ in hits)
