"""CPU: the restatement of the projected bilinear sampling (tests/pointfeat_ref.py) against hand-placed positions, the C ABI
of csrc/pointfeat.hip as far as it goes without a device, and the refusals of generativedensification_amd.pointfeat."""
import ctypes as C

import pytest
import torch

import pointfeat_ref as R

H, W = 5, 7
HAND_X = (-1.0, -0.5, 0.0, 0.25, W - 1.0, W - 0.5, float(W))
HAND_Y = (-1.0, -0.5, 0.0, 0.25, H - 1.0, H - 0.5, float(H))


def test_hand_bilinear_equals_grid_sample_at_hand_placed_positions():
    """the restatement samples through the reference's normalised coordinates; its un-normalised form is the pixel index:
    every border case by hand, on texels that are distinct integers"""
    image = torch.arange(2 * H * W, dtype=torch.float64).view(2, H, W) + 1
    xy = torch.tensor([[x, y] for y in HAND_Y for x in HAND_X], dtype=torch.float64)
    got = R.sample(image[None], xy[None])[0]                  # (C, P)
    want = torch.stack([R.hand_bilinear(image, float(x), float(y)) for x, y in xy], dim=1)
    assert (got - want).abs().max() <= 1e-12
    # spot values: the centre of texel (0, 0); half of it from half a texel outside; nothing from a whole texel outside
    assert R.hand_bilinear(image, 0.0, 0.0).tolist() == [1.0, 1.0 + H * W]
    assert R.hand_bilinear(image, -0.5, 0.0).tolist() == [0.5, 0.5 * (1 + H * W)]
    assert R.hand_bilinear(image, -1.0, 0.25).tolist() == [0.0, 0.0] and R.hand_bilinear(image, float(W), 2.0).tolist() == [0.0, 0.0]
    assert R.hand_bilinear(image, W - 0.5, H - 1.0).tolist() == [0.5 * H * W, 0.5 * 2 * H * W]


def test_restatement_projects_as_the_arithmetic_says():
    w2cs, ixts = R.cameras(3, 45, 61)
    assert not torch.equal(ixts[0, 0, 0], ixts[0, 1, 1]) and float(ixts[0, 0, 2]) % 1 != 0 and float(ixts[0, 1, 2]) % 1 != 0
    for v in range(3):       # rotations, eyes on the ring
        Rm = w2cs[v, :3, :3].double()
        assert (Rm @ Rm.T - torch.eye(3, dtype=torch.float64)).abs().max() < 1e-6
        assert abs(float((-Rm.T @ w2cs[v, :3, 3].double()).norm()) - 1.9) < 1e-5
    xy, z = R.project(torch.zeros(1, 3), w2cs, ixts)           # the origin lands on the principal point at depth 1.9
    assert (xy[:, 0] - ixts[:, :2, 2]).abs().max() < 1e-4 and (z - 1.9).abs().max() < 1e-5
    xy, z = R.project(torch.tensor([[0.1, 0.2, -3.0]]), torch.eye(4)[None], torch.eye(3)[None])     # behind: mirrored
    assert torch.allclose(xy[0, 0], torch.tensor([0.1 / -3.0, 0.2 / -3.0])) and float(z) == -3.0


def test_abi_symbols_and_refusals_without_a_gpu():
    from generativedensification_amd import _lib as L

    lib = L.load()
    for name in ("gdr_point_feats_forward", "gdr_point_feats_backward", "gdr_sample_views_forward", "gdr_sample_views_backward"):
        assert hasattr(lib, name) and name in L.EXPORTED_SYMBOLS
    assert lib.gdr_abi_version() == 17
    fake = 0x10000         # never dereferenced: every refusal comes before any device work
    s = (C.c_int64 * 4)(1, 1, 1, 1)

    def args(N=10, V=4, Cn=8, Hh=16, Ww=16):
        a = L.GdrPointfeatArgs()
        a.N, a.V, a.C, a.H, a.W = N, V, Cn, Hh, Ww
        return C.byref(a)

    def fwd(a, out=fake):
        return lib.gdr_point_feats_forward(a, fake, s, fake, s, fake, s, fake, s, fake, s, fake, fake, out, None)

    def views(a):
        return lib.gdr_sample_views_forward(a, fake, s, fake, s, fake, fake, fake, fake, None)

    for bad, word in ((dict(V=0), b"V"), (dict(V=L.GDR_PF_MAX_VIEWS + 1), b"V"), (dict(N=-1), b"N"), (dict(N=1 << 31), b"N"),
                      (dict(Hh=0), b"H"), (dict(Ww=L.GDR_PF_MAX_SIDE + 1), b"H")):
        assert fwd(args(**bad)) == -1 and word in lib.gdr_last_error()
        assert views(args(**bad)) == -1
        assert lib.gdr_point_feats_backward(args(**bad), fake, fake, s, fake, s, fake, s, fake, s, fake, s, fake, fake, fake, fake,
                                            fake, fake, fake, None) == -1
        assert lib.gdr_sample_views_backward(args(**bad), fake, fake, fake, s, fake, s, fake, fake, fake, fake, None) == -1
    for Cn in (0, L.GDR_PF_MAX_CHANNELS + 1):
        assert views(args(Cn=Cn)) == -1 and b"C must be" in lib.gdr_last_error()
    assert fwd(None) == -1
    assert fwd(args(), out=fake + 4) == -1 and b"unaligned" in lib.gdr_last_error()
    assert lib.gdr_point_feats_forward(args(), fake, None, fake, s, fake, s, fake, s, fake, s, fake, fake, fake, None) == -1
    assert lib.gdr_point_feats_forward(args(), None, s, fake, s, fake, s, fake, s, fake, s, fake, fake, fake, None) == -1
    assert lib.gdr_sample_views_backward(args(), fake, None, None, s, fake, s, fake, fake, None, fake, None) == -1
    assert b"reads the images" in lib.gdr_last_error()
    # empty inputs, and a backward nobody wants anything from, are answered without a launch
    assert fwd(args(N=0), out=None) == 0
    assert lib.gdr_sample_views_forward(args(N=0), None, s, None, s, None, None, None, None, None) == 0
    assert lib.gdr_point_feats_backward(args(), fake, fake, s, fake, s, fake, s, fake, s, fake, s, fake, fake, None, None, None,
                                        None, None, None) == 0
    assert lib.gdr_sample_views_backward(args(), fake, None, fake, s, fake, s, fake, fake, None, None, None) == 0


def test_python_surface_refuses_before_any_launch():
    from generativedensification_amd import pointfeat as P

    V, N = 2, 5
    ok = dict(img_ref=torch.zeros(V, 3, H, W), image=torch.zeros(V, H, W, 3), acc_map=torch.zeros(V, H, W),
              depth=torch.zeros(V, H, W, 1), points=torch.zeros(N, 3), w2cs=torch.eye(4).repeat(V, 1, 1),
              ixts=torch.eye(3).repeat(V, 1, 1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.point_feats(**ok)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.point_feats(**{**ok, "depth": torch.zeros(V, H, W)})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.sample_views(torch.zeros(V, 6, H, W), ok["points"], ok["w2cs"], ok["ixts"])
    for key, bad in (("img_ref", torch.zeros(V, 4, H, W)), ("image", torch.zeros(V, 3, H, W)), ("acc_map", torch.zeros(V, H, W, 1)),
                     ("depth", torch.zeros(V, H, W, 2)), ("points", torch.zeros(N, 2)), ("points", torch.zeros(3, N, 3)),
                     ("w2cs", torch.zeros(V, 3, 4)), ("ixts", torch.zeros(V + 1, 3, 3)), ("img_ref", torch.zeros(3, H, W))):
        with pytest.raises(ValueError, match=key):
            P.point_feats(**{**ok, key: bad})
    with pytest.raises(ValueError, match="images"):
        P.sample_views(torch.zeros(6, H, W), ok["points"], ok["w2cs"], ok["ixts"])
    with pytest.raises(ValueError, match="points"):
        P.sample_views(torch.zeros(V, 6, H, W), torch.zeros(N, 4), ok["w2cs"], ok["ixts"])
    with pytest.raises(ValueError, match="views"):
        P.sample_views(torch.zeros(17, 1, 2, 2), ok["points"], torch.eye(4).repeat(17, 1, 1), torch.eye(3).repeat(17, 1, 1))
    with pytest.raises(ValueError, match="channels"):
        P.sample_views(torch.zeros(1, 4097, 1, 1), ok["points"], torch.eye(4)[None], torch.eye(3)[None])
    with pytest.raises(TypeError, match="float32"):
        P.point_feats(**{**ok, "image": ok["image"].half()})
    with pytest.raises(TypeError, match="float32"):
        P.sample_views(torch.zeros(V, 6, H, W, dtype=torch.float64), ok["points"], ok["w2cs"], ok["ixts"])
    assert (P.MAX_VIEWS, P.MAX_CHANNELS, P.MAX_SIDE) == (16, 4096, 16384)
