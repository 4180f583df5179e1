"""CPU: the projections of generativedensification_amd/groupattn.py around the numpy core against nn.MultiheadAttention itself
in float64, the numpy gradient restatement against central differences, the patch row map against the reference's unfold /
einsum lines, what the seeded inputs are for, the recorded surface of the reference's GroupAttBlock against what
group_att_block_forward reads, and the argument checks (which raise before the library loads)."""
import ast
import inspect
import itertools

import numpy as np
import pytest
import torch
from torch import nn

import groupattn_cases as GC
import groupattn_ref as R

GRID = list(itertools.product(GC.MHA_GRID, (False, True), (False, True)))


def ga():
    from generativedensification_amd import groupattn as G

    return G


@pytest.mark.parametrize("shape,bias,packed", GRID, ids=str)
def test_projections_and_numpy_core_equal_multihead_attention_in_float64(shape, bias, packed):
    E, H, kdim, Lq, Lk = shape
    mha = GC.make_mha(E, H, kdim, bias, packed)
    assert (mha.in_proj_weight is not None) == packed and (mha.in_proj_bias is not None) == bias
    x, cond = (torch.from_numpy(a) for a in GC.mha_inputs(E, H, E if packed else kdim, Lq, Lk))
    with torch.no_grad():
        ref = mha(x, cond, cond, need_weights=False)[0].numpy()
        q, k, v, scale = ga().project_qkv(mha, x, cond)
        assert q.shape == x.shape and k.shape == v.shape == (x.shape[0], Lk, E) and scale == (E // H) ** -0.5
        # k and v are the two halves of one product: no copy was made for either
        assert k.stride() == v.stride() == (Lk * 2 * E, 2 * E, 1) and v.data_ptr() - k.data_ptr() == E * 8
        core = torch.from_numpy(R.group_cross_attention(q.numpy(), k.numpy(), v.numpy(), scale, H))
        out = mha.out_proj(core).numpy()
    err, top = np.abs(out - ref).max(), np.abs(ref).max()
    print(f"composition {shape} bias={bias} packed={packed}: max|d|={err:.3e} max|ref|={top:.3e}")
    assert err <= 1e-12 * top


def test_numpy_gradients_equal_central_differences():
    rng = np.random.default_rng(5)
    M, Lq, Lk, H, Dh, scale = 2, 3, 4, 2, 3, 0.7
    q, g = rng.standard_normal((M, Lq, H * Dh)), rng.standard_normal((M, Lq, H * Dh))
    k, v = rng.standard_normal((M, Lk, H * Dh)), rng.standard_normal((M, Lk, H * Dh))
    grads = R.group_cross_attention_grad(q, k, v, scale, H, g)
    ins = [q, k, v]

    def loss(args):
        return float((R.group_cross_attention(*args, scale, H) * g).sum())

    h = 1e-6
    for which, grad in enumerate(grads):
        num = np.zeros_like(ins[which])
        for idx in np.ndindex(num.shape):
            hi, lo = [a.copy() for a in ins], [a.copy() for a in ins]
            hi[which][idx] += h
            lo[which][idx] -= h
            num[idx] = (loss(hi) - loss(lo)) / (2 * h)
        # central differences in float64: truncation h^2 |f'''| ~ 1e-12, rounding eps |f| / h ~ 1e-9
        assert np.abs(num - grad).max() <= 1e-7 * max(1.0, np.abs(grad).max()), which
    # the torch restatement states the same function
    tq, tk, tv = (torch.from_numpy(a).requires_grad_(True) for a in ins)
    out = R.group_cross_attention_torch(tq, tk, tv, scale, H)
    out.backward(torch.from_numpy(g))
    assert np.abs(out.detach().numpy() - R.group_cross_attention(q, k, v, scale, H)).max() <= 1e-14
    for t, grad in zip((tq, tk, tv), grads):
        assert np.abs(t.grad.numpy() - grad).max() <= 1e-13


@pytest.mark.parametrize("name", list(GC.CASES))
def test_inputs_reach_near_uniform_and_near_one_hot_rows(name):
    """what the core cases are for: s spans about +-12, the first query near uniform, a near one-hot row in the last group"""
    M, Lq, Lk, H, Dh = GC.CASES[name]
    q, k, v, g = GC.inputs(name)
    assert q.shape == g.shape == (M, Lq, H * Dh) and k.shape == v.shape == (M, Lk, H * Dh)
    s = GC.scale_of(name) * np.einsum("mihd,mjhd->mhij", q.reshape(M, Lq, H, Dh), k.reshape(M, Lk, H, Dh))
    p = R.probabilities(q, k, GC.scale_of(name), H)
    print(f"inputs {name}: max|s|={np.abs(s).max():.2f} first-row max p * Lk={p[0, :, 0].max() * Lk:.3f} last-group max p={p[-1].max():.5f}")
    assert 8 <= np.abs(s).max() <= 25
    assert p[0, :, 0].max() <= 1.25 / Lk
    assert p[-1].max() > 0.99
    if name == GC.TWIN_KEYS:
        assert np.array_equal(k[:, 0], k[:, 1]) and not np.array_equal(v[:, 0], v[:, 1]) and np.array_equal(p[..., 0], p[..., 1])


@pytest.mark.parametrize("B,C,G,bs", [(2, 8, 3, 2), (1, 8, 2, 1)])
def test_row_map_equals_the_unfold_einsum_lines_and_their_inverse_bit_for_bit(B, C, G, bs):
    D = G * bs
    vol = np.random.default_rng(9).standard_normal((B, C, D, D, D))
    x = torch.from_numpy(vol)
    patches = R.patchify_torch(x, bs)
    assert patches.shape == (B * G ** 3, bs ** 3, C)
    assert np.array_equal(R.patchify(vol, bs), patches.numpy())
    assert np.array_equal(R.unpatchify(patches.numpy(), vol.shape, bs), R.unpatchify_torch(patches, x.shape, bs).numpy())
    assert np.array_equal(R.unpatchify(R.patchify(vol, bs), vol.shape, bs), vol)
    # with the volume stored channels-last both directions move whole C-element rows
    rows = x.contiguous(memory_format=torch.channels_last_3d).permute(0, 2, 3, 4, 1).reshape(-1, C)
    assert torch.equal(rows[torch.from_numpy(R.voxel_rows(B, D, D, D, bs))].view(patches.shape), patches)
    # a non-cubic volume: the map is a permutation
    idx = R.voxel_rows(2, 4, 6, 2, 2)
    assert np.array_equal(np.sort(idx), np.arange(2 * 4 * 6 * 2))


def test_surface_of_the_reference_is_what_group_att_block_forward_reads():
    S = R.surface()
    fn = ga().group_att_block_forward
    assert list(inspect.signature(fn).parameters) == S["forward"]["params"] == ["self", "x", "cond", "group_axis", "block_size"]
    tree = ast.parse(inspect.getsource(fn))
    reads = sorted({n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name)
                    and n.value.id == "self"})
    assert reads == S["forward"]["reads"] == ["cnn", "cross_attn", "mlp", "norm1", "norm2", "norm3"] == sorted(S["modules"])
    assert S["init"]["params"] == ["inner_dim", "cond_dim", "num_heads", "eps", "attn_drop", "attn_bias", "mlp_ratio", "mlp_drop",
                                   "norm_layer"]
    assert S["init"]["defaults"] == {"attn_drop": 0.0, "attn_bias": False, "mlp_ratio": 2.0, "mlp_drop": 0.0, "norm_layer": "nn.LayerNorm"}
    assert S["modules"]["cross_attn"] == {"constructor": "nn.MultiheadAttention", "args": [], "keywords": {
        "embed_dim": "inner_dim", "num_heads": "num_heads", "kdim": "cond_dim", "vdim": "cond_dim", "dropout": "attn_drop",
        "bias": "attn_bias", "batch_first": True}}
    # the three norms are built without eps: the constructor's `eps` does not reach them
    assert all(S["modules"][n] == {"constructor": "norm_layer", "args": ["inner_dim"], "keywords": {}} for n in ("norm1", "norm2", "norm3"))
    assert S["modules"]["cnn"]["keywords"] == {"kernel_size": 3, "padding": 1, "bias": False}
    assert S["modules"]["mlp"]["types"] == ["Linear", "GELU", "Dropout", "Linear", "Dropout"]
    # the patch order of the row map is the one of the recorded einsum subscripts
    assert S["forward"]["unfold_axes"] == [2, 3, 4] and S["forward"]["einsum"] == ["bcgl->bglc", "bdhwzyxc->bcdzhywx"]
    assert S["cond"] == {"unfold_axes": [3, 4, 5], "einsum": "bvcgl->bgvlc"}
    # the stand-in built from the record has the recorded parameter names, and the projections cover its attention
    m = R.make_group_att_block(32, 24, 4)
    assert sorted(n for n, _ in m.named_parameters()) == S["parameters"]
    assert m.norm1.eps == 1e-5 and m.cross_attn.in_proj_bias is None and m.cross_attn.out_proj.bias is None
    assert m.mlp[0].out_features == 64 and m.cnn.weight.shape == (32, 32, 3, 3, 3)
    q, k, v, scale = ga().project_qkv(m.cross_attn, torch.zeros(3, 8, 32), torch.zeros(3, 5, 24))
    assert q.shape == (3, 8, 32) and k.shape == v.shape == (3, 5, 32) and scale == 8 ** -0.5 and q.requires_grad and k.requires_grad
    # cond as the VolTransformer builds it: V views of the bs^3 voxels of a group
    feats = torch.arange(2 * 3 * 5 * 4 ** 3, dtype=torch.float32).view(2, 3, 5, 4, 4, 4)
    cond = R.cond_blocks(feats, 2)
    assert cond.shape == (2 * 8, 8 * 3, 5)
    assert torch.equal(cond[0, :8], R.patchify_torch(feats[:, 0], 2)[0]) and torch.equal(cond[9, 8:16], R.patchify_torch(feats[:, 1], 2)[9])


def test_projections_refuse_what_they_do_not_cover():
    G = ga()
    x, cond = torch.zeros(2, 3, 16), torch.zeros(2, 4, 16)
    refused = [nn.MultiheadAttention(16, 2, batch_first=False), nn.MultiheadAttention(16, 2, batch_first=True, add_bias_kv=True),
               nn.MultiheadAttention(16, 2, batch_first=True, add_zero_attn=True),
               nn.MultiheadAttention(16, 2, batch_first=True, dropout=0.1), nn.MultiheadAttention(16, 2, batch_first=True, kdim=16, vdim=4)]
    for m in refused:
        with pytest.raises(NotImplementedError):
            G.project_qkv(m, x, cond)
    G.project_qkv(nn.MultiheadAttention(16, 2, batch_first=True, dropout=0.1).eval(), x, cond)      # (no dropout in eval mode)
    with pytest.raises(TypeError):
        G.project_qkv(nn.Linear(4, 4), x, cond)
    m = nn.MultiheadAttention(16, 2, batch_first=True, kdim=8, vdim=8)
    for bad_x, bad_cond in ((x[0], cond), (x, cond), (torch.zeros(2, 3, 8), torch.zeros(2, 4, 8)), (x, torch.zeros(3, 4, 8))):
        with pytest.raises(ValueError):
            G.project_qkv(m, bad_x, bad_cond)


def test_argument_checks_raise_their_documented_types_before_the_library_is_loaded(monkeypatch):
    G = ga()
    from generativedensification_amd import _lib as L

    def no_load():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(L, "load", no_load)
    q, k = torch.zeros(5, 8, 64), torch.zeros(5, 4, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.group_cross_attention(q, k, k, 0.25, 4)
    for bad in ((q.double(), k, k), (q, k.double(), k), (q, k, k.long()), (q.numpy(), k, k), (q, None, k)):
        with pytest.raises(TypeError):
            G.group_cross_attention(*bad, 0.25, 4)
    for bad, heads in (((q[0], k, k), 4), ((q, k[:4], k), 4), ((q, k, k[:, :3]), 4), ((q, torch.zeros(5, 4, 32), k), 4),
                       ((q, k, k), 0), ((q, k, k), 65), ((q, k, k), 3), ((q, k, k), 16), ((q, k, k), 1),
                       ((torch.zeros(5, 65, 64), k, k), 4), ((torch.zeros(5, 0, 64), k, k), 4),
                       ((q, torch.zeros(5, 65, 64), torch.zeros(5, 65, 64)), 4), ((q, torch.zeros(5, 0, 64), torch.zeros(5, 0, 64)), 4)):
        with pytest.raises(ValueError):
            G.group_cross_attention(*bad, 0.25, heads)
    with pytest.raises(ValueError):
        G.group_cross_attention(q, k, k, float("nan"), 4)
    assert G.in_envelope(12288, 8, 4, 16, 16) and G.in_envelope(1, 64, 64, 64, 32)
    assert not any(G.in_envelope(*s) for s in ((24, 512, 256, 16, 16), (4, 8, 4, 16, 5), (4, 8, 65, 16, 16), (4, 8, 4, 65, 8), ((1 << 24) + 1, 8, 4, 16, 16)))

    vol, w = torch.zeros(2, 8, 4, 4, 4), torch.ones(8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.patchify_layer_norm(vol, 2, w, w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.layer_norm_unpatchify(torch.zeros(16, 8, 8), vol.shape, 2)
    for bad_vol, bs, bad_w in ((vol.double(), 2, w), (vol, 2, w.double()), (vol.numpy(), 2, w)):
        with pytest.raises(TypeError):
            G.patchify_layer_norm(bad_vol, bs, bad_w, None)
    with pytest.raises(TypeError):
        G.patchify_layer_norm(vol, 2, w, w, out_dtype=torch.float64)
    for bad_vol, bs, bad_w in ((vol[0], 2, w), (vol, 3, w), (vol, 0, w), (vol, 9, w), (torch.zeros(2, 12, 4, 4, 4), 2, None),
                               (torch.zeros(2, 1032, 2, 2, 2), 2, None), (vol, 2, torch.ones(16)), (vol, 2, torch.ones(8, 1)),
                               (torch.zeros(2, 8, 4, 4, 6), 4, w)):
        with pytest.raises(ValueError):
            G.patchify_layer_norm(bad_vol, bs, bad_w, None)
    for patches, shape, bs in ((torch.zeros(16, 8, 8), (2, 8, 4, 4), 2), (torch.zeros(16, 8, 4), vol.shape, 2),
                               (torch.zeros(16, 8), vol.shape, 2), (torch.zeros(16, 8, 8), (2, 8, 4, 4, 5), 2)):
        with pytest.raises(ValueError):
            G.layer_norm_unpatchify(patches, shape, bs)
    m = R.make_group_att_block(32, 24, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.group_att_block_forward(m, torch.zeros(1, 32, 4, 4, 4), torch.zeros(8, 3, 24), 2, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.grouped_cross_attention(m.cross_attn, torch.zeros(8, 8, 32), torch.zeros(8, 3, 24))


def test_library_refuses_what_lies_beyond_the_envelope_without_a_gpu():
    """the entry points check their arguments before any device work: -1 for invalid arguments, GDR_ERR_UNSUPPORTED (-3) beyond
    the envelope or for a misaligned / under-strided row"""
    from generativedensification_amd import _lib as L

    lib = L.load()
    fake = 0x1000                  # 16-byte aligned, never dereferenced
    f32 = L.GDR_NORM_DTYPES["f32"]

    def fwd(M=4, Lq=8, Lk=4, H=16, Dh=16, q=fake, qs=256, ks=512, vs=512, out=fake, dt=f32, scale=0.25):
        return lib.gdr_groupattn_forward(q, qs, dt, fake, ks, f32, fake + 1024, vs, f32, M, Lq, Lk, H, Dh, scale, out, f32, None)

    def bwd(M=4, Lq=8, Lk=4, H=16, Dh=16, gs=256, gq=fake, gk=fake, g=fake):
        return lib.gdr_groupattn_backward(g, gs, f32, fake, 256, f32, fake, 256, f32, fake, 256, f32, M, Lq, Lk, H, Dh, 0.25, gq, gk,
                                          fake, None)

    assert lib.gdr_abi_version() == 17
    assert fwd(M=0) == 0 and bwd(M=0) == 0
    for kw in ({"Dh": 4}, {"Dh": 24}, {"Dh": 64}, {"H": 65}, {"Lq": 65}, {"Lk": 65}, {"M": (1 << 24) + 1}, {"q": fake + 8}, {"qs": 260},
               {"qs": 248}, {"ks": 128}, {"vs": 516}, {"out": fake + 4}):
        assert fwd(**kw) == -3 and b"groupattn" in lib.gdr_last_error(), kw
    for kw in ({"Dh": 12}, {"H": 128}, {"Lk": 100}, {"gs": 12}, {"gq": fake + 4}, {"gk": fake + 8}):
        assert bwd(**kw) == -3 and b"groupattn" in lib.gdr_last_error(), kw
    for kw in ({"M": -1}, {"H": 0}, {"Lq": 0}, {"Lk": 0}, {"Dh": 0}, {"dt": 7}, {"q": None}, {"scale": float("nan")}):
        assert fwd(**kw) == -1, kw
    assert bwd(g=None) == -1

    def patchify(B=2, D=4, H=4, W=4, C=64, bs=2, vol=fake, dt=f32, eps=1e-5, patches=fake, pdt=f32):
        return lib.gdr_groupattn_patchify_norm_forward(vol, dt, fake, f32, None, f32, B, D, H, W, C, bs, eps, patches, pdt, fake, f32, None)

    def unpatchify(B=2, D=4, H=4, W=4, C=64, bs=2, vol=fake):
        return lib.gdr_groupattn_norm_unpatchify_forward(fake, f32, None, f32, fake, f32, B, D, H, W, C, bs, 1e-5, vol, f32, None)

    def norm_bwd(fn, B=2, D=4, H=4, W=4, C=64, bs=2, ws=0x10000, nbytes=1 << 20, gx=fake):
        patchify_side = fn is lib.gdr_groupattn_patchify_norm_backward          # two gradients, and the dtype of the patches
        head = (fake, f32, fake, f32, fake, f32, f32) if patchify_side else (fake, f32, fake, f32)
        return fn(*head, fake, f32, f32, B, D, H, W, C, bs, 1e-5, ws, nbytes, gx, fake, fake, None)

    assert patchify(B=0) == 0 and unpatchify(B=0) == 0
    for kw in ({"C": 4}, {"C": 12}, {"C": 1032}, {"bs": 9}, {"B": 1 << 20, "D": 64, "H": 64, "W": 64}, {"D": 1 << 16, "H": 1 << 16, "W": 1 << 16},
               {"vol": fake + 8}):
        assert patchify(**kw) == -3 and b"groupattn" in lib.gdr_last_error(), kw
        assert unpatchify(**kw) == -3 and b"groupattn" in lib.gdr_last_error(), kw
    for kw in ({"B": -1}, {"D": 0}, {"bs": 0}, {"D": 6, "bs": 4}, {"W": 5}, {"vol": None}):
        assert patchify(**kw) == -1 and unpatchify(**kw) == -1, kw
    assert patchify(dt=5) == -1 and patchify(pdt=3) == -1 and patchify(eps=-1.0) == -1 and patchify(patches=None) == -1
    assert lib.gdr_groupattn_norm_backward_bytes(128, 64) >= 2 * 2 * 64 * 4
    assert lib.gdr_groupattn_norm_backward_bytes(128, 12) == 0 and lib.gdr_groupattn_norm_backward_bytes(1 << 31, 64) == 0
    for fn in (lib.gdr_groupattn_patchify_norm_backward, lib.gdr_groupattn_norm_unpatchify_backward):
        for kw in ({"C": 20}, {"bs": 16}, {"gx": fake + 8}, {"ws": 0x10010}):
            assert norm_bwd(fn, **kw) == -3 and b"groupattn" in lib.gdr_last_error(), kw
        assert norm_bwd(fn, ws=None) == -1 and norm_bwd(fn, W=3) == -1
        assert norm_bwd(fn, nbytes=64) == L.GDR_ERR_WORKSPACE
