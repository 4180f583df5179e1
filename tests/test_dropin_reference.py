"""CPU: the reference's caller modules (lightning/renderer.py, lightning/renderer_2dgs.py, lightning/utils.py) against this
repo's drop-in packages `diff_gaussian_rasterization`, `diff_surfel_rasterization` and `simple_knn` (the drop-in test of
SURVEY §0-3).  What those modules take from the packages — the names they import, the keyword names of their
GaussianRasterizationSettings / GaussianRasterizer / rasterizer calls, how many outputs they unpack, the parameters of the
methods their callers use — is recorded in tests/golden/dropin_surface.json (tests/golden/make_dropin_surface.py).  Here
that surface is exercised on the product packages (HIP only: a loud failure on CPU tensors) and on the oracle stand-ins,
together with the repo's mirrors of the reference's Renderer and MiniCam, whose numbers tests/test_golden*_cpu.py pin."""
import importlib
import inspect
import json
import math
import os
import sys

import pytest
import torch

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dropin_surface.json")) as _f:
    SURFACE = json.load(_f)
R3, R2, UTILS = (SURFACE[m] for m in ("lightning/renderer.py", "lightning/renderer_2dgs.py", "lightning/utils.py"))


def _cam(w, h, znear, zfar):
    from generativedensification_amd.camera import MiniCam

    c2w = torch.eye(4)
    c2w[2, 3] = -2.0
    return MiniCam(c2w, w, h, torch.tensor(0.75), torch.tensor(0.75), znear, zfar, "cpu")


def _imported(surface):
    """{name: object} of the caller's `from <package> import ...` lines, resolved as Python resolves them now."""
    out = {}
    for pkg, names in surface["imports"].items():
        mod = importlib.import_module(pkg)
        for name in names:
            out[name] = getattr(mod, name)
    return out


def _rasterizer(surface, names, cam, sh_degree):
    """The caller's set_rasterizer: settings built BY KEYWORD with exactly its names, the module built by keyword."""
    values = dict(image_height=int(cam.image_height), image_width=int(cam.image_width), tanfovx=math.tan(cam.FoVx * 0.5),
                  tanfovy=math.tan(cam.FoVy * 0.5), bg=torch.ones(3), scale_modifier=1.0, viewmatrix=cam.world_view_transform,
                  projmatrix=cam.full_proj_transform, sh_degree=sh_degree, campos=cam.camera_center, prefiltered=False,
                  debug=False)
    assert sorted(surface["settings_keywords"]) == sorted(values)
    rs = names["GaussianRasterizationSettings"](**{k: values[k] for k in surface["settings_keywords"]})
    (kw,) = surface["rasterizer_keywords"]
    return names["GaussianRasterizer"](**{kw: rs})


def _call(surface, rasterizer, inputs):
    """The caller's rasterizer(...) call with exactly its keyword names; as many outputs as it unpacks."""
    out = rasterizer(**{k: inputs[k] for k in surface["call_keywords"]})
    assert len(out) == surface["call_outputs"]
    return out


def _inputs(n, scale_dims, scene=None):
    if scene is None:
        return dict(means3D=torch.zeros(n, 3), means2D=torch.zeros(n, 4, requires_grad=True), shs=torch.zeros(n, 4, 3),
                    opacities=torch.full((n, 1), 0.5), scales=torch.full((n, scale_dims), 0.01),
                    rotations=torch.tensor([1.0, 0.0, 0.0, 0.0]).repeat(n, 1), cov3D_precomp=None)
    return dict(means3D=scene["centers"], means2D=torch.zeros(n, 4, requires_grad=True), shs=scene["shs"],
                opacities=torch.sigmoid(scene["opacity"]), scales=torch.exp(scene["scales"][:, :scale_dims]).contiguous(),
                rotations=torch.nn.functional.normalize(scene["rotations"]), cov3D_precomp=None)


def _assert_mirror_signatures(surface, renderer_cls):
    """Every parameter the caller's methods take, in the same order, at the head of the mirror's parameters."""
    from generativedensification_amd.camera import MiniCam

    for meth, params in dict(surface["signatures"], **UTILS["signatures"]).items():
        cls, name = meth.split(".")
        got = list(inspect.signature(getattr(renderer_cls if cls == "Renderer" else MiniCam, name)).parameters)
        assert got[:len(params)] == params, (meth, got, params)


def test_reference_renderer_imports_against_product_package_and_fails_loudly_on_cpu():
    sys.modules.pop("diff_gaussian_rasterization", None)
    import diff_gaussian_rasterization as D  # the PRODUCT package (HIP only)
    from generativedensification_amd.renderer import Renderer

    assert not getattr(D, "__oracle_standin__", False)
    names = _imported(R3)
    assert names == {"GaussianRasterizationSettings": D.GaussianRasterizationSettings,
                     "GaussianRasterizer": D.GaussianRasterizer}
    cam = _cam(32, 32, 0.5, 2.5)
    rast = _rasterizer(R3, names, cam, 1)
    assert rast.raster_settings.image_height == 32 and rast.raster_settings.sh_degree == 1
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _call(R3, rast, _inputs(16, 3))
    # the repo's mirror of the caller's Renderer: same parameters, same loud failure, same settings
    _assert_mirror_signatures(R3, Renderer)
    r = Renderer(sh_degree=1)
    n = 16
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r.render_img(cam, None, torch.zeros(n, 3), torch.zeros(n, 4, 3), torch.zeros(n, 1), torch.zeros(n, 3),
                     torch.ones(n, 4), "cpu")
    rs = r.set_rasterizer(cam, device="cpu").raster_settings
    assert rs.image_height == 32 and rs.sh_degree == 1 and sorted(rs._fields) == sorted(R3["settings_keywords"])


def test_reference_renderer_runs_on_cpu_with_oracle_standin(oracle_built, monkeypatch):
    from generativedensification_amd import renderer as R
    from generativedensification_amd.synthetic import make_scene
    from oracle.gdr_oracle import make_standin_module

    st = make_standin_module("f32")
    monkeypatch.setitem(sys.modules, "diff_gaussian_rasterization", st)
    names = _imported(R3)
    assert names["GaussianRasterizer"] is st.GaussianRasterizer
    sc = make_scene(300, 4, sh_degree=3, sigma0=(0.03,))
    cam = _cam(48, 32, 0.5, 3.5)
    image, radii, depth, alpha = _call(R3, _rasterizer(R3, names, cam, 3), _inputs(300, 3, sc))
    assert image.shape == (3, 32, 48) and depth.shape == (1, 32, 48) and alpha.shape == (1, 32, 48)
    assert radii.shape == (300,) and int((radii > 0).sum()) > 0
    # the mirror's render_img on the stand-in, as the caller's Renderer runs it
    monkeypatch.setattr(R, "GaussianRasterizationSettings", st.GaussianRasterizationSettings)
    monkeypatch.setattr(R, "GaussianRasterizer", st.GaussianRasterizer)
    out = R.Renderer(sh_degree=3).render_img(cam, None, sc["centers"], sc["shs"], sc["opacity"], sc["scales"], sc["rotations"],
                                             "cpu", prex="_fine")
    assert out["image_fine"].shape == (32, 48, 3) and out["depth_fine"].shape == (32, 48, 1)
    assert out["acc_map_fine"].shape == (32, 48)
    assert 0.0 <= float(out["image_fine"].detach().min()) and float(out["image_fine"].detach().max()) <= 1.0


# ---- 2DGS adaptor (lightning/renderer_2dgs.py) against the product `diff_surfel_rasterization` ---------------
def test_reference_2dgs_adaptor_imports_against_product_package_and_fails_loudly_on_cpu():
    """No stand-ins at all: the names lightning/renderer_2dgs.py imports resolve to the PRODUCT `diff_surfel_rasterization`
    and the PRODUCT `simple_knn._C.distCUDA2` (both HIP only)."""
    sys.modules.pop("diff_surfel_rasterization", None)
    for k in [k for k in sys.modules if k.startswith("simple_knn")]:
        del sys.modules[k]
    import diff_surfel_rasterization as D  # the PRODUCT package (HIP only)
    from generativedensification_amd import renderer_2dgs
    from generativedensification_amd.knn import dist2

    assert not getattr(D, "__oracle_standin__", False)
    names = _imported(R2)
    assert names == {"GaussianRasterizationSettings": D.GaussianRasterizationSettings,
                     "GaussianRasterizer": D.GaussianRasterizer, "distCUDA2": dist2}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        names["distCUDA2"](torch.zeros(8, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        renderer_2dgs._activation_scale(torch.zeros(8, 3))
    cam = _cam(32, 32, 0.5, 2.5)
    rast = _rasterizer(R2, names, cam, 1)
    assert rast.raster_settings.image_width == 32 and rast.raster_settings.sh_degree == 1
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _call(R2, rast, _inputs(16, 2))
    _assert_mirror_signatures(R2, renderer_2dgs.Renderer)
    r = renderer_2dgs.Renderer(sh_degree=1)
    n = 16
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r.render_img(cam, None, torch.zeros(n, 3), torch.zeros(n, 4, 3), torch.zeros(n, 1), torch.zeros(n, 2),
                     torch.ones(n, 4), "cpu")
    rs = r.set_rasterizer(cam, device="cpu").raster_settings
    assert rs.image_width == 32 and rs.sh_degree == 1 and sorted(rs._fields) == sorted(R2["settings_keywords"])


def test_reference_2dgs_adaptor_runs_on_cpu_with_oracle_standin(oracle_built, monkeypatch):
    from generativedensification_amd import renderer_2dgs as R
    from generativedensification_amd.camera import build_rays
    from generativedensification_amd.synthetic import make_scene
    from oracle.gsr_oracle import make_simple_knn_stub, make_surfel_standin_module

    st = make_surfel_standin_module("f32")
    knn, knn_c = make_simple_knn_stub()
    monkeypatch.setitem(sys.modules, "diff_surfel_rasterization", st)
    monkeypatch.setitem(sys.modules, "simple_knn", knn)
    monkeypatch.setitem(sys.modules, "simple_knn._C", knn_c)
    names = _imported(R2)
    assert names["GaussianRasterizer"] is st.GaussianRasterizer and names["distCUDA2"] is knn_c.distCUDA2
    sc = make_scene(300, 4, sh_degree=3, sigma0=(0.03,))
    assert names["distCUDA2"](sc["centers"]).shape == (300,)
    cam = _cam(48, 32, 0.5, 3.5)
    image, radii, allmap = _call(R2, _rasterizer(R2, names, cam, 3), _inputs(300, 2, sc))
    assert image.shape == (3, 32, 48) and allmap.shape == (7, 32, 48) and radii.shape == (300,)
    # the mirror's render_img on the stand-in, as the caller's Renderer runs it
    monkeypatch.setattr(R, "GaussianRasterizationSettings", st.GaussianRasterizationSettings)
    monkeypatch.setattr(R, "GaussianRasterizer", st.GaussianRasterizer)
    c2w = torch.eye(4)
    c2w[2, 3] = -2.0
    out = R.Renderer(sh_degree=3, fused=False).render_img(cam, build_rays(c2w, 0.75, 0.75, 32, 48), sc["centers"], sc["shs"],
                                                          sc["opacity"], sc["scales"][:, :2].contiguous(), sc["rotations"],
                                                          "cpu", prex="_fine")
    assert out["image_fine"].shape == (32, 48, 3) and out["depth_fine"].shape == (32, 48, 1)
    assert out["rend_normal_fine"].shape == (32, 48, 3) and out["rend_dist_fine"].shape == (32, 48)
    assert float(out["acc_map_fine"].detach().max()) > 0.1 and torch.isfinite(out["depth_normal_fine"]).all()
