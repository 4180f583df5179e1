"""-m gpu: the surfel path's multi-view preprocess entries (gsr_preprocess_forward_views = K1s of V views in one launch,
gsr_preprocess_backward_views = K9s of V views in one launch) on tiny scenes, against the single-view entries
(gsr_forward_view, gsr_backward) on the same inputs, through the ctypes layer.  The surfel counterpart of
test_gpu_preprocess_views_small.py: same cameras, same three-times-frustum scene with one hidden surfel, same bars.

K1s: every per-view array it leaves (radius, depth, 96-byte render record, rect, tiles, clamp mask, block sums, duplicate
count) is compared BIT FOR BIT with the single-view K1s of that view.

K9s: fed the gradient records the single-view backward of each view leaves (K7s' output), it must give the sum over the
views, in view order, of the single-view K9s outputs:
  * every output within util.elem_stats' bar (per element 1e-4 |ref| + 1e-6 max|ref|, fewer than util.MAX_OUTSIDE of the
    elements outside, max-norm relative error < 1e-4);
  * bit for bit where the multi-view kernel adds the per-view terms in that same order: the SH gradient and the
    screen-space signal always, the opacity gradient unless the sigmoid is folded in; and equal in value (a zero's sign
    aside) for every output when V == 1.  (means3D / scales / rotations of V > 1 are sums of the same terms in another
    association: the kernel sums the gradients of the world-space vectors that build T over the views before they go
    through the scale / rotation chain once.)
accumulate = 1 adds onto noise, accumulate = 0 writes onto NaN; a surfel no view sees gets exact zeros or is left as it
was."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import util as U

pytestmark = pytest.mark.gpu

H = W = U.SMALL_HW
RAW_ALL = 1 | 2 | 4          # GDR_IN_RAW_OPACITY | GDR_IN_RAW_SCALES | GDR_IN_RAW_ROTATIONS
MAX_VIEWS = U.SMALL_MAX_VIEWS
NS = (1, 63, 255, 256, 257, 513)   # partial last wave, partial last workgroup, a wave wholly past the end of the rows
_bits, _cams, _hidden_point = U.bits, U.small_cams, U.small_hidden_point

GRAD_KEYS = ("means3D", "means2D", "shs", "opacities", "scales", "rotations")
REC_WORDS = 24               # GSR_REC_FLOATS
GRAD_WORDS = 32              # GSR_GRAD_FLOATS

# (N, V, active degree, M, flags): degree 3 and 1 take the staged SH rows in K9s, degree 2 (27-float rows) does not
CASES = [(n, v, deg, m, f) for deg, m in ((3, 16), (1, 4), (2, 9)) for n in NS for v in (1, 3, MAX_VIEWS)
         for f in (RAW_ALL, 0)]


def _scene(N, M, flags, dev):
    """test_gpu_preprocess_views_small._scene with (N,2) scales: raw attributes over three times the scene cube, activated
    on the host where the raw flag is off; surfel 0 is out of every camera's sight."""
    from generativedensification_amd.synthetic import make_scene

    sc = make_scene(N, 40 + N, sh_degree=int(math.isqrt(M)) - 1, sigma0=(0.06, 0.02))
    means = 3.0 * sc["centers"]
    means[0] = _hidden_point()
    op = sc["opacity"] if flags & 1 else torch.sigmoid(sc["opacity"])
    scales = sc["scales"][:, :2] if flags & 2 else torch.exp(sc["scales"][:, :2])
    rot = sc["rotations"] if flags & 4 else torch.nn.functional.normalize(sc["rotations"])
    return {k: v.contiguous().to(dev) for k, v in dict(means3D=means, shs=sc["shs"], opacities=op, scales=scales,
                                                        rotations=rot).items()}


def _structs(sc, cam, deg, flags, dev, keep):
    from generativedensification_amd import _lib as L
    from generativedensification_amd import rasterizer as R

    rs = R.GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=math.tan(U.FOV * 0.5), tanfovy=math.tan(U.FOV * 0.5),
        bg=torch.ones(3, device=dev), scale_modifier=1.0, viewmatrix=cam.world_view_transform,
        projmatrix=cam.full_proj_transform, sh_degree=deg, campos=cam.camera_center, prefiltered=False, debug=False)
    s = R._settings_struct(rs, dev, keep)
    N, M = sc["shs"].shape[:2]
    inp = L.GsrInputs(N, M, sc["means3D"].data_ptr(), sc["opacities"].data_ptr(), sc["shs"].data_ptr(), None,
                      sc["scales"].data_ptr(), sc["rotations"].data_ptr(), None, flags, 0)
    return s, inp


def _geom_arrays(buf, g, N):
    """The arrays K1s leaves in a gdr_geom, as numpy."""
    def view(ptr, dtype, count):
        off = ptr - buf.data_ptr()
        return buf[off:off + count * torch.empty(0, dtype=dtype).element_size()].view(dtype).cpu().numpy()

    blocks = (N + 255) // 256
    return dict(depths=view(g.depths, torch.int32, N), rec=view(g.rec, torch.int32, REC_WORDS * N),
                rect=view(g.rect, torch.int32, 4 * N), tiles_touched=view(g.tiles_touched, torch.int32, N),
                clamped=view(g.clamped, torch.uint8, N), block_sums=view(g.block_sums, torch.int32, blocks),
                num_rendered=view(g.num_rendered, torch.int32, 1))


_REF = {}


def _single_view(N, deg, M, flags, v, dev):
    """Single-view forward + backward of view v (once per scene and view): K1s' arrays, the gradient records K7s leaves
    for K9s, and K9s' outputs."""
    key = (N, deg, M, flags, v)
    if key not in _REF:
        from generativedensification_amd import _lib as L
        from generativedensification_amd import rasterizer as R

        lib = L.load()
        sc, keep = _scene(N, M, flags, dev), []
        s, inp = _structs(sc, _cams(dev)[v], deg, flags, dev, keep)
        f32 = dict(dtype=torch.float32, device=dev)
        color, allmap = torch.empty(3, H, W, **f32), torch.empty(7, H, W, **f32)
        radii = torch.empty(N, dtype=torch.int32, device=dev)
        out = L.GsrOutputs(color.data_ptr(), allmap.data_ptr(), radii.data_ptr())
        ws, vs = R.forward_view_native(lib.gsr_forward_view, C.byref(s), C.byref(inp), N, H, W, True, C.byref(out), None,
                                       dev, R._stream())
        gen = torch.Generator().manual_seed(1000 + v)
        gc, ga = (torch.randn(c, H, W, generator=gen).to(dev) for c in (3, 7))
        g = dict(means3D=torch.empty(N, 3, **f32), means2D=torch.empty(N, 4, **f32), shs=torch.empty(N, M, 3, **f32),
                 opacities=torch.empty(N, 1, **f32), scales=torch.empty(N, 2, **f32), rotations=torch.empty(N, 4, **f32))
        rec = torch.empty(N * GRAD_WORDS, **f32)
        gin = L.GsrGradInputs(gc.data_ptr(), ga.data_ptr())
        gout = L.GsrGradOutputs(g["means3D"].data_ptr(), g["means2D"].data_ptr(), g["shs"].data_ptr(), None,
                                g["opacities"].data_ptr(), g["scales"].data_ptr(), g["rotations"].data_ptr(), None,
                                rec.data_ptr(), 0, 0)
        L.check(lib.gsr_backward(C.byref(s), C.byref(inp), C.byref(vs.geom), C.byref(vs.bin), C.byref(vs.img), int(vs.D),
                                 radii.data_ptr(), C.byref(gin), C.byref(gout), R._stream()), "gsr_backward")
        torch.cuda.synchronize()
        _REF[key] = dict(geom=_geom_arrays(ws, vs.geom, N), radii=radii.cpu().numpy(), rec=rec.cpu(),
                         grads={k: t.cpu().numpy() for k, t in g.items()})
    return _REF[key]


@pytest.mark.parametrize("N,V,deg,M,flags", CASES)
def test_surfel_multiview_preprocess_equals_the_single_view_entries(N, V, deg, M, flags):
    from generativedensification_amd import _lib as L
    from generativedensification_amd import rasterizer as R

    dev = torch.device("cuda:0")
    lib = L.load()
    ref = [_single_view(N, deg, M, flags, v, dev) for v in range(V)]
    sc, keep = _scene(N, M, flags, dev), []
    cams = _cams(dev)
    structs = [_structs(sc, cams[v], deg, flags, dev, keep) for v in range(V)]
    s_arr = (L.GdrSettings * V)(*[s for s, _ in structs])
    inp = structs[0][1]

    # ---- K1s of the V views in one launch --------------------------------------------------------------------------
    gbytes = (int(lib.gsr_geom_bytes(N)) + 255) // 256 * 256
    gbuf = torch.zeros(V * gbytes, dtype=torch.uint8, device=dev)
    g_arr = (L.GdrGeom * V)()
    for v in range(V):
        L.check(lib.gsr_geom_carve(C.c_void_p(gbuf.data_ptr() + v * gbytes), N, C.byref(g_arr[v])), "gsr_geom_carve")
    radii = torch.full((V, N), -1, dtype=torch.int32, device=dev)
    r_arr = (C.c_void_p * V)(*[radii[v].data_ptr() for v in range(V)])
    L.check(lib.gsr_preprocess_forward_views(V, s_arr, C.byref(inp), g_arr, r_arr, R._stream()),
            "gsr_preprocess_forward_views")
    torch.cuda.synchronize()
    rad = radii.cpu().numpy()
    for v in range(V):
        got = _geom_arrays(gbuf, g_arr[v], N)
        np.testing.assert_array_equal(rad[v], ref[v]["radii"], err_msg=f"radii of view {v}")
        for k in ("depths", "rec", "rect", "tiles_touched", "clamped", "block_sums", "num_rendered"):
            np.testing.assert_array_equal(got[k], ref[v]["geom"][k], err_msg=f"{k} of view {v}")
    seen = rad > 0
    assert not seen[:, 0].any()                                   # the hidden surfel
    if V > 1 and N >= 63:
        assert (seen.any(0) & ~seen.all(0)).any()                 # radius 0 in some views, not in others
    if N >= 63:
        assert seen.any()

    # ---- K9s of the V views in one launch, on the records the single-view backward left ------------------------------
    recs = [ref[v]["rec"].to(dev) for v in range(V)]
    rec_arr = (C.c_void_p * V)(*[r.data_ptr() for r in recs])
    shapes = dict(means3D=(N, 3), means2D=(N, 4), shs=(N, M, 3), opacities=(N, 1), scales=(N, 2), rotations=(N, 4))
    total = {k: np.zeros(shapes[k], np.float32) for k in GRAD_KEYS}
    for v in range(V):                                            # float32, view order, from zero
        for k in GRAD_KEYS:
            total[k] = total[k] + ref[v]["grads"][k]
    gen = torch.Generator().manual_seed(7)
    for accumulate in (0, 1):
        base = {k: (torch.randn(shapes[k], generator=gen) if accumulate else torch.full(shapes[k], float("nan")))
                for k in GRAD_KEYS}
        g = {k: t.clone().to(dev) for k, t in base.items()}
        gout = L.GsrGradOutputs(g["means3D"].data_ptr(), g["means2D"].data_ptr(), g["shs"].data_ptr(), None,
                                g["opacities"].data_ptr(), g["scales"].data_ptr(), g["rotations"].data_ptr(), None, None,
                                accumulate, 0)
        L.check(lib.gsr_preprocess_backward_views(V, s_arr, C.byref(inp), g_arr, r_arr, rec_arr, C.byref(gout), R._stream()),
                "gsr_preprocess_backward_views")
        torch.cuda.synchronize()
        what = f"N={N} V={V} deg={deg} M={M} flags={flags} accumulate={accumulate}"
        for k in GRAD_KEYS:
            got = g[k].cpu().numpy()
            want = total[k] + base[k].numpy() if accumulate else total[k]
            outside, worst, maxn = U.elem_stats(got, want)
            bits_equal = bool((_bits(got) == _bits(want)).all())
            print(f"[{what}] {k:10s} outside {outside:.2e} worst/tol {worst:.2f} max-norm rel {maxn:.2e} "
                  f"max|diff| {float(np.abs(got - want).max()):.3e} bits equal {bits_equal}")
            assert np.isfinite(got).all(), (what, k)
            assert outside < U.MAX_OUTSIDE and maxn < 1e-4, (what, k, outside, maxn)
            if k in ("shs", "means2D") or (k == "opacities" and not flags & 1):
                np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=f"{what}: {k} bit for bit")
            elif V == 1:
                np.testing.assert_array_equal(got, want, err_msg=f"{what}: {k}")
            # the surfel no view sees: exact zeros, or left as it was
            hidden = base[k].numpy()[0] if accumulate else np.zeros(shapes[k][1:], np.float32)
            np.testing.assert_array_equal(_bits(got[0]), _bits(hidden), err_msg=f"{what}: {k} of the hidden surfel")
