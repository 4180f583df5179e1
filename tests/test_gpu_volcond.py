"""GPU: the volume conditioning of csrc/volcond.hip (generativedensification_amd.volcond) against the float64 restatement
(tests/volcond_ref.py) and the reference's torch composition on the same GPU in the same dtypes (tests/volcond_torch.py).

Accuracy bar, for every output and gradient (the project's bar of tests/test_gpu_norm.py): with e_hip = max|hip - ref64| and
e_torch = max|torch - ref64| (ref64 on the inputs as rounded to their dtypes), e_hip <= 2 e_torch + half an ulp of the result
dtype at max|ref64|.  Every pair is printed before it is asserted.  Where torch has no answer (the pairs with a zero homogeneous
depth, which it divides by), the bound is derived in the test."""
import types

import numpy as np
import pytest
import torch

import norm_ref as NR
import volcond_cases as VC
import volcond_ref as R
import volcond_torch as T

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16


def volcond():
    from generativedensification_amd import volcond as V

    return V


def dev(a, dtype=F32):
    return None if a is None else NR.to_dtype(a, dtype).to(DEV)


def f64(t):
    return None if t is None else t.detach().double().cpu().numpy()


def bar(what, hip, tor, ref64):
    """prints the pair; settle asserts the bar"""
    assert hip.dtype == tor.dtype and hip.shape == tor.shape == ref64.shape, (what, hip.dtype, tor.dtype, hip.shape, tor.shape, ref64.shape)
    e_hip = float(np.abs(f64(hip) - ref64).max()) if ref64.size else 0.0
    e_torch = float(np.abs(f64(tor) - ref64).max()) if ref64.size else 0.0
    slack = NR.half_ulp(hip.dtype, float(np.abs(ref64).max()) if ref64.size else 0.0)
    print(f"volcond-bar {what}: e_hip={e_hip:.3e} e_torch={e_torch:.3e} half_ulp={slack:.3e}")
    assert np.isfinite(f64(hip)).all(), what
    return what, e_hip, e_torch, slack


def settle(results):
    bad = [(w, eh, et, s) for w, eh, et, s in results if not eh <= 2 * et + s]
    assert not bad, bad


class ctx:
    """autocast to bfloat16 or nothing"""

    def __init__(self, on):
        self.cm = torch.autocast("cuda", dtype=BF16) if on else torch.autocast("cuda", enabled=False)

    def __enter__(self):
        return self.cm.__enter__()

    def __exit__(self, *a):
        return self.cm.__exit__(*a)


# ---- ray_sh -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
def test_ray_sh(dtype):
    V = volcond()
    rays = dev(VC.ray_inputs(), dtype)
    results = []
    for silu in (False, True):
        hip = V.ray_sh(rays, silu=silu)
        assert hip.dtype == F32 and hip.shape == (37, 32) and not hip.requires_grad
        assert torch.equal(hip, V.ray_sh(rays, silu=silu))
        results.append(bar(f"ray_sh/{dtype}/silu={silu}", hip, T.ray_sh(rays.float(), silu), R.ray_sh(f64(rays), silu)))
    settle(results)
    shaped = V.ray_sh(rays.view(1, 37, 1, 6).expand(2, 37, 1, 6))
    assert shaped.shape == (2, 37, 1, 32) and torch.equal(shaped[1, :, 0], V.ray_sh(rays))
    with torch.autocast("cuda", dtype=BF16):
        assert V.ray_sh(rays).dtype == F32
    assert V.ray_sh(rays[:0]).shape == (0, 32)


# ---- mod_layer_norm -----------------------------------------------------------------------------------------------------------

# (x, shift_scale, parameters, autocast): the three pure ones and the pairs autocast produces (a bfloat16 encoder output and
# Linear product with float32 parameters; a float32 x with a bfloat16 product)
MOD_DTYPES = {"f32": (F32, F32, F32, False), "bf16": (BF16, BF16, BF16, False), "f16": (F16, F16, F16, False),
              "amp_bf16_x": (BF16, BF16, F32, True), "amp_f32_x": (F32, BF16, F32, True)}


def mod_leaves(name, x_dt, ss_dt, p_dt):
    x64, ss64, w64, b64, g64 = VC.mod_inputs(name)
    rows, c, _, layout = VC.MOD_CASES[name]
    x, ss = dev(x64, x_dt), dev(ss64, ss_dt)
    if layout == "tokens":          # the token slice of a (2, 1 + 12, C) encoder output as (2, 3, 4, C); ss a column slice
        full = torch.zeros(2, 13, c, dtype=x_dt, device=DEV)
        full[:, 1:] = x.view(2, 12, c)
        wide = torch.zeros(rows, 2 * c + 8, dtype=ss_dt, device=DEV)
        wide[:, :2 * c] = ss
        return full, wide, dev(w64, p_dt), dev(b64, p_dt), g64
    return x, ss, dev(w64, p_dt), dev(b64, p_dt), g64


def mod_call(fn, name, leaves, g64, amp):
    rows, c, _, layout = VC.MOD_CASES[name]
    x, ss, w, b = (None if t is None else t.clone().requires_grad_(True) for t in leaves)
    xin, ssin = (x[:, 1:].view(2, 3, 4, c), ss[:, :2 * c]) if layout == "tokens" else (x, ss)
    with ctx(amp):
        out = fn(xin, ssin, w, b, VC.EPS)
    out.backward(dev(g64, out.dtype).view(out.shape))
    gx = x.grad[:, 1:].reshape(rows, c) if layout == "tokens" else x.grad
    gss = ss.grad[:, :2 * c] if layout == "tokens" else ss.grad
    return out.reshape(rows, c), gx, gss, None if w is None else w.grad, None if b is None else b.grad


@pytest.mark.parametrize("dtypes", sorted(MOD_DTYPES))
@pytest.mark.parametrize("name", sorted(VC.MOD_CASES))
def test_mod_layer_norm(name, dtypes):
    V = volcond()
    x_dt, ss_dt, p_dt, amp = MOD_DTYPES[dtypes]
    *leaves, g64 = mod_leaves(name, x_dt, ss_dt, p_dt)
    hip = mod_call(V.mod_layer_norm, name, leaves, g64, amp)
    again = mod_call(V.mod_layer_norm, name, leaves, g64, amp)
    tor = mod_call(T.mod_layer_norm, name, leaves, g64, amp)
    want = F32 if amp else torch.promote_types(torch.promote_types(x_dt, ss_dt), p_dt if leaves[2] is not None else x_dt)
    assert hip[0].dtype == want
    for t, leaf_dt in zip(hip[1:], (x_dt, ss_dt, p_dt, p_dt)):
        assert t is None or t.dtype == leaf_dt
    for a, b in zip(hip, again):
        assert (a is None and b is None) or torch.equal(a, b)          # bitwise, forward and backward
    rows, c, _, layout = VC.MOD_CASES[name]
    x, ss, w, b = leaves
    x64 = f64(x[:, 1:].reshape(rows, c)) if layout == "tokens" else f64(x)
    ss64 = f64(ss[:, :2 * c]) if layout == "tokens" else f64(ss)
    g_used = f64(dev(g64, hip[0].dtype))
    refs = (R.mod_layer_norm(x64, ss64, f64(w), f64(b), VC.EPS),) + R.mod_layer_norm_grad(x64, ss64, f64(w), f64(b), VC.EPS, g_used)
    results = [bar(f"modln/{name}/{dtypes}/{what}", h, t, r) for what, h, t, r in zip(("out", "dx", "dss", "dw", "db"), hip, tor, refs)
               if h is not None]
    settle(results)
    if name == "constant_row":
        assert all(torch.isfinite(t).all() for t in hip if t is not None)
        if dtypes == "f32":
            row = VC.CONSTANT_ROW
            want_row = b * (1 + ss[row, c:]) + ss[row, :c]
            assert (hip[0][row] - want_row).abs().max() <= 2 ** -23 * float(want_row.abs().max())      # the two roundings of a * b + c


def test_mod_layer_norm_computes_only_the_gradients_needed():
    V = volcond()
    *leaves, g64 = mod_leaves("r67_c24", F32, F32, F32)
    full = mod_call(V.mod_layer_norm, "r67_c24", leaves, g64, False)
    x, ss, w, b = (t.clone() for t in leaves)
    x.requires_grad_(True)
    out = V.mod_layer_norm(x, ss, w, b, VC.EPS)
    out.backward(dev(g64))
    assert torch.equal(out, full[0]) and torch.equal(x.grad, full[1]) and ss.grad is None and w.grad is None and b.grad is None
    w.requires_grad_(True)
    x.grad = None
    V.mod_layer_norm(x.detach(), ss, w, b, VC.EPS).backward(dev(g64))
    assert torch.equal(w.grad, full[3]) and x.grad is None
    with torch.no_grad():
        assert torch.equal(V.mod_layer_norm(x, ss, w, b, VC.EPS), full[0])
    empty = V.mod_layer_norm(x[:0], ss[:0], w, b, VC.EPS)
    assert empty.shape == (0, 24)


# ---- sample_tokens ------------------------------------------------------------------------------------------------------------

# (rows, view_embed, out_dtype)
SAMPLE_DTYPES = {"f32": (F32, F32, None), "bf16": (BF16, BF16, None), "f16": (F16, F16, None), "bf16_rows_f32_embed": (BF16, F32, None),
                 "f32_to_bf16": (F32, F32, BF16)}


def sample_call(kind, name, rows, ve, out_dtype, grad64):
    V = volcond()
    Bn, Vn, hw, img_hw, r, g = VC.SAMPLE_CASES[name][:6]
    _, points, w2cs, ixts, _, _ = VC.sample_inputs(name)
    rows = rows.clone().requires_grad_(True)
    ve = None if ve is None else ve.clone().requires_grad_(True)
    cams = (dev(points), dev(w2cs), dev(ixts))
    if kind == "hip":
        out = V.sample_tokens(rows, *cams, img_hw, g, view_embed=ve, out_dtype=out_dtype, n_views=Vn)
    else:
        out = T.sample_tokens(rows, *cams, img_hw, g, Vn, ve)
        if out_dtype is not None:
            out = out.to(out_dtype)
    out.backward(dev(grad64, out.dtype))
    return out, rows.grad, None if ve is None else ve.grad


@pytest.mark.parametrize("dtypes", sorted(SAMPLE_DTYPES))
@pytest.mark.parametrize("name", [n for n in sorted(VC.SAMPLE_CASES) if n != "degenerate"])
def test_sample_tokens(name, dtypes):
    rows_dt, ve_dt, out_dtype = SAMPLE_DTYPES[dtypes]
    Bn, Vn, hw, img_hw, r, g, Cn, E, views, _ = VC.SAMPLE_CASES[name]
    rows64, points, w2cs, ixts, ve64, grad64 = VC.sample_inputs(name)
    rows, ve = dev(rows64, rows_dt), dev(ve64, ve_dt)
    hip = sample_call("hip", name, rows, ve, out_dtype, grad64)
    again = sample_call("hip", name, rows, ve, out_dtype, grad64)
    tor = sample_call("torch", name, rows, ve, out_dtype, grad64)
    want = out_dtype or (rows_dt if ve is None else torch.promote_types(rows_dt, ve_dt))
    assert hip[0].dtype == want and hip[0].shape == (Bn * g ** 3, Vn * (r // g) ** 3, Cn + E) and hip[0].is_contiguous()
    assert hip[1].dtype == rows_dt and (ve is None or hip[2].dtype == ve_dt)
    for a, b in zip(hip, again):
        assert (a is None and b is None) or torch.equal(a, b)          # bitwise, forward and backward
    cams32 = [f64(dev(a)) for a in (points, w2cs, ixts)]
    ref_out = R.sample_tokens(f64(rows), *cams32, img_hw, g, Vn, f64(ve))
    g_used = f64(dev(grad64, hip[0].dtype))
    ref_drows, ref_dve = R.sample_tokens_grad(rows.shape, *cams32, img_hw, g, Vn, None if ve is None else ve.shape, g_used)
    results = [bar(f"sample/{name}/{dtypes}/{what}", h, t, r_) for what, h, t, r_ in
               zip(("out", "drows", "dve"), hip, tor, (ref_out, ref_drows, ref_dve)) if h is not None]
    settle(results)
    if ve is not None:      # the embedding columns are copies
        per = hip[0].reshape(-1, Cn + E)[torch.as_tensor(R.cond_rows(Bn, Vn, r, g)).to(DEV)]
        assert torch.equal(per[..., Cn:], ve[0, :Vn, :, 0, 0, 0].to(want)[None, :, None, :].expand(Bn, Vn, r ** 3, E))
        assert views == Vn or not hip[2][0, Vn:].any()


def test_sample_tokens_autocast_and_no_grad():
    V = volcond()
    name = "b2v3_5x3_g2"
    Bn, Vn, hw, img_hw, r, g = VC.SAMPLE_CASES[name][:6]
    rows64, points, w2cs, ixts, ve64, grad64 = VC.sample_inputs(name)
    rows, ve, cams = dev(rows64), dev(ve64), (dev(points), dev(w2cs), dev(ixts))
    plain = V.sample_tokens(rows, *cams, img_hw, g, view_embed=ve, n_views=Vn)
    with torch.autocast("cuda", dtype=BF16):
        amp = V.sample_tokens(rows, *cams, img_hw, g, view_embed=ve, n_views=Vn)
    assert amp.dtype == F32 and torch.equal(amp, plain) and not plain.requires_grad
    only_ve = ve.clone().requires_grad_(True)
    V.sample_tokens(rows, *cams, img_hw, g, view_embed=only_ve, n_views=Vn).backward(dev(grad64))
    both = sample_call("hip", name, rows, ve, None, grad64)
    assert torch.equal(only_ve.grad, both[2])
    # cameras in float64 are converted, not refused
    assert torch.equal(V.sample_tokens(rows, *(c.double() for c in cams), img_hw, g, view_embed=ve, n_views=Vn), plain)


def test_degenerate_pairs_sample_zeros_and_send_finite_gradients():
    """torch divides by the zero depth, so the bound is derived: a position carries at most 4e-6 of absolute error in float32
    (the normalised coordinate in [-2, 2] rounds to 2^-23 and is scaled by w / 2 = 2.5; the projection adds as much again), a
    weight is a product of two factors in [0, 1] with that error each, and a sample or a texel gradient sums n such terms:
    |error| <= n * 1e-5 * max|value| with n = 4 taps forward and at most 4 * 64 entries backward."""
    V = volcond()
    name = "degenerate"
    Bn, Vn, hw, img_hw, r, g, Cn, E, views, _ = VC.SAMPLE_CASES[name]
    rows64, points, w2cs, ixts, ve64, grad64 = VC.sample_inputs(name)
    rows, ve = dev(rows64), dev(ve64)
    with torch.autograd.set_detect_anomaly(True):
        out, drows, dve = sample_call("hip", name, rows, ve, None, grad64)
    cams32 = [f64(dev(a)) for a in (points, w2cs, ixts)]
    ref_out = R.sample_tokens(f64(rows), *cams32, img_hw, g, Vn, f64(ve))
    ref_drows, ref_dve = R.sample_tokens_grad(rows.shape, *cams32, img_hw, g, Vn, ve.shape, f64(dev(grad64)))
    zero_depth = torch.as_tensor(points[:, 2] == 0.125).to(DEV)
    per = out.reshape(-1, Cn + E)[torch.as_tensor(R.cond_rows(Bn, Vn, r, g).reshape(-1)).to(DEV)]
    assert int(zero_depth.sum()) == 16 and not per[zero_depth, :Cn].any() and per[~zero_depth, :Cn].any()
    assert torch.isfinite(out).all() and torch.isfinite(drows).all() and torch.isfinite(dve).all()
    e_out, e_drows, e_dve = (float(np.abs(f64(a) - b).max()) for a, b in ((out, ref_out), (drows, ref_drows), (dve, ref_dve)))
    print(f"volcond-degenerate: e_out={e_out:.3e} e_drows={e_drows:.3e} e_dve={e_dve:.3e}")
    assert e_out <= 4 * 1e-5 * np.abs(rows64).max()
    assert e_drows <= 4 * 64 * 1e-5 * np.abs(grad64).max()
    assert e_dve <= 64 * 2.0 ** -23 * np.abs(grad64).max() * 2      # a float32 sum of 64 terms


# ---- bindings -----------------------------------------------------------------------------------------------------------------

def network(seed, Cn=24, E=8, r=4, n_groups=(2, 1), embed=16, layers=()):
    """stand-ins for Network / ModLN / VolTransformer with only the attributes the bindings read"""
    gen = torch.Generator().manual_seed(seed)
    norm = torch.nn.LayerNorm(Cn, eps=1e-6)
    mlp = torch.nn.Sequential(torch.nn.SiLU(), torch.nn.Linear(32, 2 * Cn))
    with torch.no_grad():
        norm.weight.copy_(1 + 0.3 * torch.randn(Cn, generator=gen))
        norm.bias.copy_(0.2 * torch.randn(Cn, generator=gen))
        mlp[1].weight.copy_(0.3 * torch.randn(2 * Cn, 32, generator=gen))
        mlp[1].bias.copy_(0.1 * torch.randn(2 * Cn, generator=gen))
    dec = types.SimpleNamespace(n_groups=list(n_groups), block_size=[r // g for g in n_groups],
                                pos_embed=torch.nn.Parameter(torch.randn(1, embed, r, r, r, generator=gen).to(DEV)), layers=list(layers),
                                norm=torch.nn.LayerNorm(embed, eps=1e-6).to(DEV),
                                deconv=torch.nn.ConvTranspose3d(embed, 8, kernel_size=2, stride=2, padding=0).to(DEV))
    return types.SimpleNamespace(volume_grid=dev(VC.grid_points(r)).view(r, r, r, 3), feat_vol_reso=r,
                                 dir_norm=types.SimpleNamespace(norm=norm.to(DEV), mlp=mlp.to(DEV)),
                                 view_embed=torch.nn.Parameter(torch.randn(1, 4, E, 1, 1, 1, generator=gen).to(DEV)),
                                 cfg=types.SimpleNamespace(model=types.SimpleNamespace(view_embed_dim=E)), vol_decoder=dec)


def batch_of(Bn, Vn, hw, img_hw, Cn, seed):
    rng = np.random.default_rng(seed)
    w2cs, ixts = VC.orbit_cameras(Bn * 4, img_hw)
    h, w = hw
    rays = np.concatenate([rng.standard_normal((Bn, 4, h, w, 3)) * 1.2, rng.standard_normal((Bn, 4, h, w, 3))], -1)
    batch = {"tar_w2c": dev(w2cs).view(Bn, 4, 4, 4), "tar_ixt": dev(ixts).view(Bn, 4, 3, 3), "tar_rays_down": dev(rays),
             "tar_rgb": torch.zeros(1, device=DEV).expand(Bn, 4, *img_hw, 3)}
    tokens = dev(rng.standard_normal((Bn * Vn, 1 + h * w, Cn)))          # an encoder output with a class token, token-major
    img_feats = torch.einsum('blc->bcl', tokens[:, 1:]).reshape(Bn * Vn, Cn, h, w)
    return batch, img_feats, rays, w2cs, ixts


@pytest.mark.parametrize("amp", [False, True], ids=["f32", "autocast"])
def test_build_feat_vol_binding(amp, monkeypatch):
    V = volcond()
    Bn, Vn, hw, img_hw, Cn, r = 2, 3, (3, 5), (48, 80), 24, 4
    net = network(3, Cn=Cn, r=r)
    batch, img_feats, rays, w2cs, ixts = batch_of(Bn, Vn, hw, img_hw, Cn, 5)
    src = torch.zeros(1, device=DEV).expand(Bn * Vn, 3, *img_hw)
    sel = lambda a: a.reshape(Bn, 4, *a.shape[1:])[:, :Vn].reshape(Bn * Vn, *a.shape[1:])      # noqa: E731
    cams = (dev(VC.grid_points(r)), dev(sel(w2cs)), dev(sel(ixts)))

    def reference(feats):
        """the reference's build_feat_vol restated with this file's composition"""
        with ctx(amp):
            sh = T.ray_sh(batch["tar_rays_down"][:, :Vn].reshape(-1, *hw, 6))
            x = T.mod_layer_norm(torch.einsum('bchw->bhwc', feats), net.dir_norm.mlp(sh), net.dir_norm.norm.weight, net.dir_norm.norm.bias, 1e-6)
            return T.feat_vol(torch.einsum('bhwc->bchw', x), *cams, img_hw, Vn)

    outs = {}
    for backend in ("hip", "torch"):
        monkeypatch.setattr(V, "COND_BACKEND", backend)
        leaf = img_feats.clone().requires_grad_(True)
        with ctx(amp):
            vol = V.build_feat_vol(net, src, leaf, Vn, batch)
        # (einsum is on autocast's lower-precision list: the reference's volume is bfloat16 there)
        assert vol.shape == (Bn, Vn, Cn, r, r, r) and vol.dtype == (BF16 if amp else F32)
        g = torch.randn(vol.shape, generator=torch.Generator().manual_seed(9)).to(DEV, vol.dtype)
        net.dir_norm.norm.zero_grad()
        net.dir_norm.mlp.zero_grad()
        vol.backward(g)
        outs[backend] = (vol, leaf.grad, net.dir_norm.norm.weight.grad.clone(), net.dir_norm.mlp[1].weight.grad.clone())
    leaf = img_feats.clone().requires_grad_(True)
    net.dir_norm.norm.zero_grad()
    net.dir_norm.mlp.zero_grad()
    vol = reference(leaf)
    vol.backward(g)
    tor = (vol, leaf.grad, net.dir_norm.norm.weight.grad.clone(), net.dir_norm.mlp[1].weight.grad.clone())
    # float64: the Linear in float64 from the float32 parameters
    lin = net.dir_norm.mlp[1]
    ss64 = R.ray_sh(f64(batch["tar_rays_down"][:, :Vn]).reshape(-1, 6), silu=True) @ f64(lin.weight).T + f64(lin.bias)
    x64 = f64(img_feats.permute(0, 2, 3, 1)).reshape(-1, Cn)
    rows64 = R.mod_layer_norm(x64, ss64, f64(net.dir_norm.norm.weight), f64(net.dir_norm.norm.bias), 1e-6).reshape(Bn * Vn, *hw, Cn)
    ref = R.sample_tokens(rows64, *(f64(c) for c in cams), img_hw, r, Vn).reshape(Bn, r, r, r, Vn, Cn).transpose(0, 4, 5, 1, 2, 3)
    results = [bar(f"build_feat_vol/{'amp' if amp else 'f32'}/{backend}", outs[backend][0], tor[0], ref) for backend in ("hip", "torch")]
    settle(results)
    # the gradients through the whole binding against the torch composition, same dtypes.  float32: other summation orders of a
    # few hundred float32 terms, 1e-5 of the largest entry.  bfloat16 autocast: the reference's projection matmuls run in
    # bfloat16 there, half an ulp at a pixel coordinate of up to 80 is 0.25 px = 1/64 of a texel of the 16 times smaller map, in
    # each factor of a tap weight (3.1e-2 of a gradient), and the Linear's product and its gradient round to bfloat16 (twice
    # 2^-8): 4e-2 of the largest entry
    for what, h, t in zip(("dfeats", "dln_weight", "dlinear_weight"), outs["hip"][1:], tor[1:]):
        err, top = float((h - t).abs().max()), float(t.abs().max())
        print(f"volcond-binding {what}: err={err:.3e} max={top:.3e}")
        assert h.dtype == t.dtype and err <= (4e-2 if amp else 1e-5) * top


def test_volume_conds_equal_build_feat_vol_cat_cond_bitwise(monkeypatch):
    from generativedensification_amd import deconv3d as D

    V = volcond()
    monkeypatch.setattr(D, "TAIL_BACKEND", "torch")
    Bn, Vn, hw, img_hw, Cn, r, E = 2, 3, (3, 5), (48, 80), 24, 4, 8
    mixing = lambda x, cond, n_group, block_size: x + 1e-3 * cond.float().sum()      # noqa: E731  (a layer that reads its cond)
    for layers in ((), (mixing, mixing, mixing)):
        net = network(4, Cn=Cn, E=E, r=r, n_groups=(2, 1, 4), layers=layers)
        batch, img_feats, *_ = batch_of(Bn, Vn, hw, img_hw, Cn, 6)
        src = torch.zeros(1, device=DEV).expand(Bn * Vn, 3, *img_hw)
        for backend in ("hip", "torch"):
            monkeypatch.setattr(V, "COND_BACKEND", backend)
            vol = V.build_feat_vol(net, src, img_feats, Vn, batch)
            vol = torch.cat((vol, net.view_embed[:, :Vn].expand(Bn, -1, -1, r, r, r)), dim=2)
            old = D.vol_transformer_forward(net.vol_decoder, vol)
            conds = V.volume_conds(net, img_feats, Vn, batch)
            new = D.vol_transformer_forward_from_conds(net.vol_decoder, conds, Bn)
            assert len(conds) == 3 and all(torch.equal(c, D._cond(vol, g_, r // g_)) for c, g_ in zip(conds, (2, 1, 4)))
            assert old.shape == (Bn, 2 * r, 2 * r, 2 * r, 8) and torch.equal(old, new)
    with pytest.raises(ValueError):
        D.vol_transformer_forward_from_conds(net.vol_decoder, conds[:2], Bn)
