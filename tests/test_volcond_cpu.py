"""CPU: the float64 restatement of the volume conditioning (tests/volcond_ref.py) against the recorded values of the reference's
rsh_cart_3 and against torch autograd on the reference's composition restated (tests/volcond_torch.py, with F.grid_sample and the
cond lines of VolTransformer.forward), which pins the sample position u = (x + 0.5) w / W - 0.5 and the cond row order; the argument
checks of generativedensification_amd.volcond, which raise before the library loads; the refusals of the C ABI of
csrc/volcond.hip without a device."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import volcond_cases as VC
import volcond_ref as R
import volcond_torch as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "volcond_rsh.npz")
F64 = torch.float64


def t64(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(F64)


def test_restatement_equals_the_recorded_rsh_cart_3():
    """the reference prints its constants with 14 to 15 digits: a relative 1e-13 of the largest term, |v|^3 for degree 3"""
    d = np.load(GOLDEN)
    v, want = d["vectors"], d["rsh"]
    assert v.shape == (64, 3) and want.shape == (64, 16)
    norms = np.linalg.norm(v, axis=1)
    assert (norms == 0).sum() == 1 and (np.abs(norms - 1) < 1e-12).sum() >= 24 and (np.abs(norms - 1) > 0.05).sum() >= 24
    got = R.rsh3(v)
    bound = 1e-13 * 10 * np.maximum(1.0, norms[:, None] ** 3)
    assert (np.abs(got - want) <= bound).all(), float(np.abs(got - want).max())
    assert np.abs(got - T.rsh3(t64(v)).numpy()).max() < 1e-13


def test_ray_sh_restatement_equals_torch():
    rays = VC.ray_inputs()
    assert rays.shape == (37, 6)
    for silu in (False, True):
        got, want = R.ray_sh(rays, silu), T.ray_sh(t64(rays), silu).numpy()
        assert np.isfinite(got).all() and np.abs(got - want).max() < 1e-12
    plain = R.ray_sh(rays)
    zero_sh = R.rsh3(np.zeros(3))
    assert np.array_equal(plain[5], np.concatenate([zero_sh, zero_sh]))          # zero direction: dh = 0, m = 0
    assert np.abs(plain[11, 16:] - zero_sh).max() < 1e-15                        # origin parallel to the direction: m = 0
    assert np.allclose(plain[23, :16], R.rsh3(np.array([0.6, 0.0, -0.8]) * 1e-8), rtol=1e-12, atol=0)   # |d| = 1e-20: divided by 1e-12


@pytest.mark.parametrize("name", sorted(VC.MOD_CASES))
def test_mod_layer_norm_restatement_equals_torch_autograd(name):
    x, ss, w, b, g = VC.mod_inputs(name)
    leaves = [t64(a).requires_grad_(True) if a is not None else None for a in (x, ss, w, b)]
    out = T.mod_layer_norm(*leaves, VC.EPS)
    out.backward(t64(g))
    assert np.abs(R.mod_layer_norm(x, ss, w, b, VC.EPS) - out.detach().numpy()).max() < 1e-11
    grads = R.mod_layer_norm_grad(x, ss, w, b, VC.EPS, g)
    for what, got, leaf in zip(("dx", "dss", "dw", "db"), grads, leaves):
        if leaf is not None:
            assert np.abs(got - leaf.grad.numpy()).max() < 1e-8 * max(1.0, np.abs(got).max()), (name, what)
    if name == "constant_row":
        c = x.shape[1]
        row = VC.CONSTANT_ROW
        assert np.array_equal(R.mod_layer_norm(x, ss, w, b, VC.EPS)[row], b * (1 + ss[row, c:]) + ss[row, :c])
        assert np.isfinite(grads[0]).all()


@pytest.mark.parametrize("name", sorted(VC.SAMPLE_CASES))
def test_sample_tokens_restatement_equals_torch_autograd(name):
    B, V, hw, img_hw, r, g, Cn, E, views, geometry = VC.SAMPLE_CASES[name]
    rows, points, w2cs, ixts, ve, grad = VC.sample_inputs(name)
    got = R.sample_tokens(rows, points, w2cs, ixts, img_hw, g, V, ve)
    drows, dve = R.sample_tokens_grad(rows.shape, points, w2cs, ixts, img_hw, g, V, None if ve is None else ve.shape, grad)
    assert got.shape == grad.shape == (B * g ** 3, V * (r // g) ** 3, Cn + E)
    if geometry == "dyadic":
        # torch divides by the zero depth; the rule of the kernels is checked by hand: pairs with a zero depth sample zeros
        zero_depth = np.isclose(points[:, 2], 0.125, atol=0)
        per = got.reshape(-1, Cn + E)[R.cond_rows(B, V, r, g).reshape(-1)].reshape(B * V, -1, Cn + E)
        assert zero_depth.sum() == 16 and np.array_equal(per[0, zero_depth, :Cn], np.zeros((16, Cn)))
        assert np.abs(per[0, ~zero_depth, :Cn]).max() > 0 and np.isfinite(drows).all()
        points = points[~zero_depth]
        keep = R.cond_rows(B, V, r, g).reshape(-1)[~zero_depth]
        # the other pairs (a negative depth among them) against torch, point by point
        leaf = t64(rows).requires_grad_(True)
        vol = T.feat_vol(torch.einsum('bhwc->bchw', leaf), t64(np.concatenate([points, points[:16]])), t64(w2cs), t64(ixts), img_hw, V)
        want = vol.reshape(Cn, -1)[:, :48].T.detach().numpy()
        assert np.abs(got.reshape(-1, Cn + E)[keep, :Cn] - want).max() < 1e-12
        return
    leaf = t64(rows).requires_grad_(True)
    ve_leaf = None if ve is None else t64(ve).requires_grad_(True)
    out = T.sample_tokens(leaf, t64(points), t64(w2cs), t64(ixts), img_hw, g, V, ve_leaf)
    out.backward(t64(grad))
    assert np.abs(got - out.detach().numpy()).max() < 1e-12
    assert np.abs(drows - leaf.grad.numpy()).max() < 1e-11
    if ve is not None:
        assert np.abs(dve - ve_leaf.grad.numpy()).max() < 1e-11
        assert views == V or np.array_equal(dve[0, V:], np.zeros_like(dve[0, V:]))


def test_unscaled_intrinsics_sample_somewhere_else():
    """the 16 times larger image the intrinsics refer to: sampling at the pixel itself (the unscaled recipe) misses the map"""
    name = "b1v3_3x5_g4"
    B, V, hw, img_hw, r, g = VC.SAMPLE_CASES[name][:6]
    rows, points, w2cs, ixts, _, _ = VC.sample_inputs(name)
    scaled = R.sample_tokens(rows, points, w2cs, ixts, img_hw, g, V)
    unscaled = R.sample_tokens(rows, points, w2cs, ixts, hw, g, V)
    assert np.abs(scaled - unscaled).max() > 0.1


def test_argument_checks_raise_before_the_library_loads(monkeypatch):
    from generativedensification_amd import _lib as L
    from generativedensification_amd import volcond as V

    def no_load():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(L, "load", no_load)
    with pytest.raises(TypeError):
        V.ray_sh(np.zeros((3, 6)))
    with pytest.raises(TypeError):
        V.ray_sh(torch.zeros(3, 6, dtype=F64))
    with pytest.raises(ValueError):
        V.ray_sh(torch.zeros(3, 5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.ray_sh(torch.zeros(3, 6))
    x, ss, w = torch.zeros(4, 16), torch.zeros(4, 32), torch.ones(16)
    with pytest.raises(TypeError):
        V.mod_layer_norm(x.double(), ss, w, w)
    with pytest.raises(TypeError):
        V.mod_layer_norm(x, ss, w, w, eps="1e-5")
    for bad in (dict(x=torch.zeros(4, 12), ss=torch.zeros(4, 24)), dict(x=torch.zeros(4, 1032), ss=torch.zeros(4, 2064)),
                dict(ss=torch.zeros(4, 16)), dict(ss=torch.zeros(3, 32)), dict(w=torch.ones(8)), dict(x=torch.zeros(16)),
                dict(eps=-1.0)):
        kw = dict(x=x, ss=ss, w=w, eps=1e-5)
        kw.update(bad)
        with pytest.raises(ValueError):
            V.mod_layer_norm(kw["x"], kw["ss"], kw["w"], None, kw["eps"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.mod_layer_norm(x, ss, w, w)
    rows, pts = torch.zeros(2, 3, 5, 8), torch.zeros(8, 3)
    w2c, ixt = torch.zeros(2, 4, 4), torch.zeros(2, 3, 3)
    ve = torch.zeros(1, 2, 8, 1, 1, 1)
    with pytest.raises(TypeError):
        V.sample_tokens(rows.double(), pts, w2c, ixt, (48, 80), 2)
    with pytest.raises(TypeError):
        V.sample_tokens(rows, pts, w2c, ixt, (48, 80), 2, out_dtype=F64)
    for bad in (dict(rows=torch.zeros(2, 3, 5, 12)), dict(rows=torch.zeros(2, 3, 5, 4104)), dict(rows=torch.zeros(2, 1025, 1, 8)),
                dict(rows=torch.zeros(3, 5, 8)), dict(pts=torch.zeros(9, 3)), dict(pts=torch.zeros(8, 2)), dict(n_group=3), dict(n_group=0),
                dict(w2c=torch.zeros(3, 4, 4)), dict(ixt=torch.zeros(2, 3, 4)), dict(img_hw=(0, 80)), dict(img_hw=48), dict(n_views=3),
                dict(ve=torch.zeros(1, 1, 8, 1, 1, 1)), dict(ve=torch.zeros(1, 2, 12, 1, 1, 1)), dict(ve=torch.zeros(2, 8))):
        kw = dict(rows=rows, pts=pts, w2c=w2c, ixt=ixt, img_hw=(48, 80), n_group=2, n_views=2, ve=ve)
        kw.update(bad)
        with pytest.raises(ValueError):
            V.sample_tokens(kw["rows"], kw["pts"], kw["w2c"], kw["ixt"], kw["img_hw"], kw["n_group"], view_embed=kw["ve"],
                            n_views=kw["n_views"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.sample_tokens(rows, pts, w2c, ixt, (48, 80), 2, view_embed=ve, n_views=2)
    monkeypatch.setattr(V, "COND_BACKEND", "cuda")
    with pytest.raises(ValueError, match="COND_BACKEND"):
        V.build_feat_vol(None, None, None, 2, {})
    assert V.SLAB_ROWS == VC.SLAB_ROWS == L.GDR_VOLCOND_SLAB_ROWS


def test_abi_symbols_and_refusals_without_a_gpu():
    from generativedensification_amd import _lib as L

    lib = L.load()
    names = ("gdr_volcond_ray_sh", "gdr_volcond_modln_forward", "gdr_volcond_modln_backward_bytes", "gdr_volcond_modln_backward",
             "gdr_volcond_sample_forward", "gdr_volcond_sample_backward_bytes", "gdr_volcond_sample_backward")
    for name in names:
        assert hasattr(lib, name) and name in L.EXPORTED_SYMBOLS
    assert lib.gdr_abi_version() == 17
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gdr.h")).read()
    for macro, value in (("GDR_VOLCOND_SLAB_ROWS", L.GDR_VOLCOND_SLAB_ROWS), ("GDR_VOLCOND_MAX_CHANNELS", L.GDR_VOLCOND_MAX_CHANNELS),
                         ("GDR_VOLCOND_MAX_SIDE", L.GDR_VOLCOND_MAX_SIDE)):
        assert f"#define {macro} {value}\n" in header
    assert "#define GDR_VOLCOND_MAX_ENTRIES (1 << 30)\n" in header and L.GDR_VOLCOND_MAX_ENTRIES == 1 << 30
    fake = 0x10000         # never dereferenced: every refusal comes before any device work
    INVALID, UNSUPPORTED, WORKSPACE = -1, -3, L.GDR_ERR_WORKSPACE      # include/gdr.h GDR_ERR_INVALID_ARG, GDR_ERR_UNSUPPORTED
    F32 = L.GDR_NORM_DTYPES["f32"]

    assert lib.gdr_volcond_ray_sh(fake, F32, 0, 0, fake, None) == L.GDR_OK              # n = 0: no launch
    assert lib.gdr_volcond_ray_sh(fake, F32, -1, 0, fake, None) == INVALID
    assert lib.gdr_volcond_ray_sh(fake, 7, 4, 0, fake, None) == INVALID
    assert lib.gdr_volcond_ray_sh(None, F32, 4, 0, fake, None) == INVALID
    assert lib.gdr_volcond_ray_sh(fake, F32, 4, 0, fake + 4, None) == INVALID
    assert lib.gdr_volcond_ray_sh(fake, F32, 1 << 27, 0, fake, None) == UNSUPPORTED

    def fwd(R_=4, Cn=16, x=fake, xs=16, inner=4, outer=0, ss=fake, sss=32, w=fake, out=fake, eps=1e-5, dt=F32):
        return lib.gdr_volcond_modln_forward(x, xs, inner, outer, dt, ss, sss, F32, w, F32, None, F32, R_, Cn, eps, out, F32, None)

    assert fwd(R_=0) == L.GDR_OK                                                        # R = 0: no launch
    assert fwd(Cn=12) == UNSUPPORTED and fwd(Cn=1032) == UNSUPPORTED and fwd(Cn=0) == UNSUPPORTED
    assert fwd(R_=-1) == INVALID and fwd(R_=1 << 31) == UNSUPPORTED
    assert fwd(x=None) == INVALID and fwd(ss=None) == INVALID and fwd(out=None) == INVALID
    assert fwd(xs=8) == INVALID and fwd(xs=20) == INVALID and fwd(sss=24) == INVALID and fwd(x=fake + 8) == INVALID
    assert fwd(inner=0) == INVALID and fwd(outer=-8) == INVALID and fwd(outer=12) == INVALID
    assert fwd(eps=-1.0) == INVALID and fwd(dt=5) == INVALID and fwd(w=fake + 2) == INVALID
    assert b"volcond" in lib.gdr_last_error()

    assert lib.gdr_volcond_modln_backward_bytes(100, 16) >= 4 * 2 * 16 * 4 and lib.gdr_volcond_modln_backward_bytes(100, 12) == 0

    def bwd(R_=4, Cn=16, g=fake, ws=fake, ws_bytes=1 << 20, dx=fake, dss=fake, dw=fake, db=fake):
        return lib.gdr_volcond_modln_backward(g, 16, F32, fake, 16, 4, 0, F32, fake, 32, F32, fake, F32, fake, F32, R_, Cn, 1e-5, ws,
                                              ws_bytes, dx, dss, dw, db, None)

    assert bwd(dx=None, dss=None, dw=None, db=None) == L.GDR_OK                         # nothing is wanted: no launch
    assert bwd(Cn=12) == UNSUPPORTED and bwd(g=None) == INVALID and bwd(ws=None) == INVALID
    assert bwd(R_=100, ws_bytes=256) == WORKSPACE and bwd(dx=fake + 4) == INVALID

    def sargs(**kw):
        a = L.GdrVolcondSampleArgs(B=1, V=2, h=3, w=5, C=8, E=8, r=4, n_group=2, img_h=48, img_w=80)
        for k, v in kw.items():
            setattr(a, k, v)
        return C.byref(a)

    def sfwd(a, rows=fake, ve=fake, cond=fake, keys=fake, wts=fake):
        return lib.gdr_volcond_sample_forward(a, rows, F32, fake, fake, fake, ve, 8, F32, cond, F32, keys, wts, None)

    assert sfwd(None) == INVALID and sfwd(sargs(B=0)) == INVALID and sfwd(sargs(n_group=3)) == INVALID
    assert sfwd(sargs(C=12)) == UNSUPPORTED and sfwd(sargs(C=4104)) == UNSUPPORTED and sfwd(sargs(E=4)) == UNSUPPORTED
    assert sfwd(sargs(h=1025)) == UNSUPPORTED and sfwd(sargs(r=1024, n_group=1)) == UNSUPPORTED      # 4 B V r^3 > 2^30
    assert sfwd(sargs(), rows=None) == INVALID and sfwd(sargs(), ve=None) == INVALID and sfwd(sargs(), keys=None) == INVALID
    assert sfwd(sargs(), rows=fake + 4) == INVALID and sfwd(sargs(), keys=fake + 4) == INVALID
    assert lib.gdr_volcond_sample_backward_bytes(sargs()) >= 2 * 8 * 4 * 2 * 64 and lib.gdr_volcond_sample_backward_bytes(sargs(C=12)) == 0

    def sbwd(a, g=fake, keys=fake, ws=fake, ws_bytes=1 << 30, drows=fake, dve=fake):
        return lib.gdr_volcond_sample_backward(a, g, F32, keys, fake, ws, ws_bytes, drows, F32, dve, F32, None)

    assert sbwd(sargs(), drows=None, dve=None) == L.GDR_OK                              # nothing is wanted: no launch
    assert sbwd(sargs(n_group=3)) == INVALID and sbwd(sargs(), g=None) == INVALID and sbwd(sargs(), keys=None) == INVALID
    assert sbwd(sargs(), ws_bytes=256) == WORKSPACE and sbwd(sargs(E=0), drows=None) == INVALID
