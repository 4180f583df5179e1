"""Cameras x scenes that break the symmetries of the rasterizer's camera handling: shared by tests/test_camera_cases_cpu.py
(the oracle alone: reach floors, autograd, finite differences, mutants) and tests/test_gpu_camera.py (HIP against the oracle).

Every other rasterizer test looks through `orbit_cameras` (radius 1.9, looking at the origin, fovx == fovy, scale_modifier 1):
no visible Gaussian is ever in the frustum clamp of the EWA Jacobian, none is near the near plane, and tan(fovx/2) and
tan(fovy/2) are the same number.  The cameras here stand inside / on the edge of / next to the scene cube, look past its
centre, have fovx != fovy in both orders with W > H and W < H, and scale_modifier on both sides of 1.

`branches` of a case = what it is FOR; tests/test_camera_cases_cpu.py asserts that the f32 oracle shows at least `FLOOR`
visible Gaussians with a non-zero means3D gradient in each claimed branch:
  clamp_x / clamp_y  |t.x / t.z| > 1.3 tan(fovx/2)  (resp. y): Jacobian evaluated at the clamped point, xmul / ymul = 0 backward
  near               view depth in (0.2, 0.4): just behind the near cull, large radii, rects cut by the image edges
  edges              rect cut by each of the four image edges (counted per edge; the floor holds for the rarest edge)
"""
from __future__ import annotations

import math

import numpy as np
import torch

import util as U
from generativedensification_amd.camera import MiniCam, look_at_c2w
from generativedensification_amd.synthetic import make_scene

FLOOR = 16           # visible Gaussians with a non-zero gradient per claimed branch (full-size case)
FLOOR_REDUCED = 8    # the same on the reduced-N version used by the f64 autograd / finite-difference tests
ZNEAR, ZFAR = 0.1, 5.0
NEAR_CULL, NEAR_BAND = 0.2, 0.4

# H, W are never multiples of 16.  where: position of the eye relative to the scene cube [-0.5, 0.5]^3.
CAMERAS = {
    # fovx > fovy, W > H; eye inside the cube; SH degree 3
    "inside_wide_x": dict(eye=(0.35, 0.2, 0.1), target=(-0.3, -0.1, 0.05), fovx=1.1, fovy=0.45, H=110, W=206, N=6000, seed=11,
                          deg=3, sigma0=(0.04, 0.01), scale_modifier=1.3, bg=(1.0, 0.5, 0.2), where="inside",
                          branches=("clamp_x", "clamp_y", "near", "edges"), surfel=True,
                          reduced=dict(N=700, H=55, W=103)),
    # fovx < fovy, W < H; eye on an edge of the cube; SH degree 1
    "edge_tall_y": dict(eye=(0.5, -0.5, 0.1), target=(0.0, 0.1, 0.0), fovx=0.4, fovy=0.8, H=174, W=94, N=6000, seed=12,
                        deg=1, sigma0=(0.04, 0.01), scale_modifier=1.0, bg=(0.0, 0.0, 0.0), where="edge",
                        branches=("clamp_x", "clamp_y", "near", "edges"), surfel=True,
                        reduced=dict(N=700, H=87, W=47)),
    # fovx > fovy, W < H; eye outside, looking past the centre; SH degree 2; scale_modifier above 1
    "outside_offaxis": dict(eye=(1.0, 0.7, 0.4), target=(0.35, -0.2, 0.1), fovx=0.7, fovy=0.3, H=206, W=142, N=8000, seed=13,
                            deg=2, sigma0=(0.03, 0.008), scale_modifier=1.7, bg=(1.0, 1.0, 1.0), where="outside",
                            branches=("clamp_x", "clamp_y", "edges"), surfel=True,
                            reduced=dict(N=900, H=103, W=71)),
    # fovx < fovy, W > H; eye just outside a face, Gaussians on both sides of the near plane; SH degree 0; scale_modifier below 1
    "near_face": dict(eye=(0.62, 0.3, 0.2), target=(-0.3, -0.1, 0.05), fovx=0.5, fovy=1.0, H=106, W=202, N=6000, seed=14,
                      deg=0, sigma0=(0.01, 0.004), scale_modifier=0.6, bg=(0.2, 0.7, 0.4), where="outside",
                      branches=("near", "edges"), surfel=True,
                      reduced=dict(N=900, H=53, W=101)),
    # colors_precomp + cov3D_precomp; fovx > fovy, W > H; eye inside
    "inside_precomp": dict(eye=(-0.3, 0.35, -0.2), target=(0.4, -0.1, 0.1), fovx=0.9, fovy=0.5, H=118, W=166, N=5000, seed=15,
                           deg=0, sigma0=(0.04, 0.01), scale_modifier=0.8, bg=(0.5, 0.5, 0.5), where="inside",
                           branches=("clamp_x", "clamp_y", "near", "edges"), surfel=False, precomp=True,
                           reduced=dict(N=700, H=59, W=83)),
}
NAMES = tuple(CAMERAS)
SURFEL_NAMES = tuple(n for n, c in CAMERAS.items() if c["surfel"])


def camera(spec, device="cpu", H=None, W=None):
    """MiniCam of a table entry (MiniCam takes fovy BEFORE fovx)."""
    c2w = look_at_c2w(torch.tensor(spec["eye"]), torch.tensor(spec["target"]))
    return MiniCam(c2w, W or spec["W"], H or spec["H"], torch.tensor(spec["fovy"]), torch.tensor(spec["fovx"]), ZNEAR, ZFAR, device)


def _with_camera(case, cam, fovx, fovy):
    case.update(view=cam.world_view_transform.contiguous(), proj=cam.full_proj_transform.contiguous(),
                campos=cam.camera_center.contiguous(), tanfovx=math.tan(0.5 * fovx), tanfovy=math.tan(0.5 * fovy))
    return case


def make_camera_case(name, reduced=False):
    """A case dict in util.make_case's format for CAMERAS[name]; reduced=True: the few-hundred-Gaussian, half-size image
    version of the f64 autograd / finite-difference tests (same camera, same scene statistics)."""
    spec = dict(CAMERAS[name])
    if reduced:
        spec.update(spec["reduced"])
    pre = bool(spec.get("precomp"))
    case = U.make_case(spec["N"], spec["H"], spec["W"], spec["seed"], deg=spec["deg"], sigma0=spec["sigma0"], bg=spec["bg"],
                       scale_modifier=spec["scale_modifier"], colors_precomp=pre, cov_precomp=pre)
    case = _with_camera(case, camera(spec), spec["fovx"], spec["fovy"])
    case["name"], case["branches"] = name, spec["branches"]
    return case


def as_surfel(case):
    """The same camera and scene as a 2DGS case (util.make_surfel_case's format: (N,2) scales)."""
    c = dict(case)
    c["scales"] = case["scales"][:, :2].contiguous()
    c["transMat_precomp"] = None
    return c


def view_geometry(case):
    """float64, from the case alone: view depth, t.x / t.z, t.y / t.z of every Gaussian."""
    p = case["means3D"].double().numpy()
    v = case["view"].double().numpy()
    pv = p @ v[:3, :3] + v[3, :3]
    z = pv[:, 2]
    zs = np.where(z == 0, 1e-300, z)
    return z, pv[:, 0] / zs, pv[:, 1] / zs


def branch_masks(case, out):
    """Boolean (N,) masks of the VISIBLE Gaussians of each branch (out: forward dict of the oracle on `case`)."""
    z, rx, ry = view_geometry(case)
    vis = np.asarray(out["radii"]) > 0
    px, py = np.asarray(out["xy"], np.float64)[:, 0], np.asarray(out["xy"], np.float64)[:, 1]
    r = np.asarray(out["radii"], np.float64)
    H, W = case["H"], case["W"]
    return dict(
        clamp_x=vis & (np.abs(rx) > 1.3 * case["tanfovx"]), clamp_y=vis & (np.abs(ry) > 1.3 * case["tanfovy"]),
        near=vis & (z > NEAR_CULL) & (z < NEAR_BAND),
        cut_left=vis & (px - r < 0), cut_right=vis & (px + r > W - 1), cut_top=vis & (py - r < 0), cut_bottom=vis & (py + r > H - 1))


def reach(case, out, g_means3D=None):
    """Counts of what the case reaches.  With g_means3D (the oracle's gradient w.r.t. means3D) the branch counts are of
    Gaussians whose gradient is non-zero."""
    z, _, _ = view_geometry(case)
    m = branch_masks(case, out)
    if g_means3D is not None:
        nz = np.abs(np.asarray(g_means3D).reshape(-1, 3)).max(axis=1) > 0
        m = {k: v & nz for k, v in m.items()}
    rg = np.asarray(out["ranges"]).astype(np.int64).reshape(-1, 2)
    d = {k: int(v.sum()) for k, v in m.items()}
    d.update(visible=int((np.asarray(out["radii"]) > 0).sum()), near_culled=int((z <= NEAR_CULL).sum()), edges=min(d["cut_left"], d["cut_right"], d["cut_top"], d["cut_bottom"]),
             max_radius=int(np.asarray(out["radii"]).max()), longest_list=int((rg[:, 1] - rg[:, 0]).max()),
             num_rendered=int(out["num_rendered"]))
    return d


# ---- multi-view sets: ONE image size, ONE Gaussian set, every view its own (fovx, fovy) and bg -----------------------------
MV = dict(H=102, W=150, N=6000, seed=21, deg=2, sigma0=(0.015, 0.004))
_MV_FOVS = [(1.0, 0.5), (0.45, 0.95), (0.8, 0.35), (0.4, 1.1), (1.15, 0.6), (0.55, 0.9), (0.7, 0.4), (0.5, 1.2), (0.9, 0.55)]
_MV_BGS = [(1.0, 1.0, 1.0), (0.5, 0.5, 0.5), (0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.3, 0.6, 0.9),
           (0.9, 0.6, 0.3), (0.2, 0.2, 0.8)]


def multiview_specs(V):
    """V (<= 9) cameras on a tilted ring of radius 0.45 (inside the cube), each looking across the cube at a point of the
    opposite side, off the centre."""
    specs = []
    for j in range(V):
        th = 2 * math.pi * j / V + 0.3
        eye = (0.45 * math.cos(th), 0.45 * math.sin(th), 0.25 * math.sin(2 * th + 0.5))
        target = (-0.3 * math.cos(th + 0.4), -0.3 * math.sin(th + 0.4), -0.1 * math.sin(th))
        specs.append(dict(eye=eye, target=target, fovx=_MV_FOVS[j][0], fovy=_MV_FOVS[j][1], H=MV["H"], W=MV["W"], bg=_MV_BGS[j]))
    return specs


def make_multiview_set(V, device="cpu"):
    """(raw scene dict of make_scene, [MiniCam], [bg tensors], [case dict per view in util.make_case's format]); the cases
    share the activated tensors, so the sum of their oracle gradients is the gradient of the multi-view node."""
    sc = make_scene(MV["N"], MV["seed"], sh_degree=MV["deg"], sigma0=MV["sigma0"])
    specs = multiview_specs(V)
    base = U.make_case(MV["N"], MV["H"], MV["W"], MV["seed"], deg=MV["deg"], sigma0=MV["sigma0"])
    cams = [camera(s, device) for s in specs]
    cases = []
    for s in specs:
        c = _with_camera(dict(base), camera(s), s["fovx"], s["fovy"])
        c["bg"] = torch.tensor(s["bg"], dtype=torch.float32)
        cases.append(c)
    return sc, cams, [torch.tensor(s["bg"], dtype=torch.float32, device=device) for s in specs], cases
