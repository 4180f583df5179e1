"""CPU (-m "not gpu"): the camera table of tests/camera_cases.py, checked with the oracle alone before the GPU tests lean
on it — (a) every case reaches the branches it claims, (b) the f64 C oracle equals autograd in those branches, (c) finite
differences on Gaussians taken from the branches, (d) the cases tell a wrong camera from a right one and the orbit camera
of the rest of the suite does not, (e) MiniCam with fovx != fovy against the reference's class (golden fixtures)."""
import numpy as np
import pytest
import torch

import camera_cases as CC
import util as U
from oracle import torch_ref
from oracle import torch_ref_surfel as TS
from oracle.gdr_oracle import Oracle
from oracle.gsr_oracle import SurfelOracle

GRAD_KEYS = ("means3D", "means2D", "shs", "opacities", "scales", "rotations")
PRECOMP_KEYS = ("means3D", "means2D", "colors_precomp", "opacities", "cov3D_precomp")


def _keys(case):
    return PRECOMP_KEYS if case["cov3D_precomp"] is not None else GRAD_KEYS


# ---- (a) reach ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduced", [False, True])
@pytest.mark.parametrize("name", CC.NAMES)
def test_case_reaches_the_branches_it_claims(oracle_built, name, reduced):
    """Floors, not measurements: >= 16 (reduced: 8) visible Gaussians with a non-zero oracle gradient w.r.t. means3D in
    every branch the case claims; no Gaussian within 1e-6 of the near cull (so markVisible can be compared exactly)."""
    case = CC.make_camera_case(name, reduced=reduced)
    out, g = U.run_oracle(case, "f32", U.rand_grads(case), nthreads=4)
    r = CC.reach(case, out, g["means3D"])
    print(name, "reduced" if reduced else "full", r)
    floor = CC.FLOOR_REDUCED if reduced else CC.FLOOR
    assert case["branches"], name
    for b in case["branches"]:
        assert r[b] >= floor, (name, b, r)
    z, _, _ = CC.view_geometry(case)
    assert not (np.abs(z - CC.NEAR_CULL) < 1e-6).any()
    assert case["H"] % 16 and case["W"] % 16
    assert case["tanfovx"] != case["tanfovy"]


def test_table_covers_every_branch_twice_and_every_camera_kind():
    for b in ("clamp_x", "clamp_y", "near", "edges"):
        assert sum(b in c["branches"] for c in CC.CAMERAS.values()) >= 2, b
    kinds = {(c["fovx"] > c["fovy"], c["W"] > c["H"]) for c in CC.CAMERAS.values()}
    assert kinds == {(True, True), (True, False), (False, True), (False, False)}
    assert {c["where"] for c in CC.CAMERAS.values()} == {"inside", "edge", "outside"}
    sm = [c["scale_modifier"] for c in CC.CAMERAS.values() if not c.get("precomp")]
    assert min(sm) < 1.0 < max(sm)
    assert {c["deg"] for c in CC.CAMERAS.values()} == {0, 1, 2, 3}
    assert sum(bool(c.get("precomp")) for c in CC.CAMERAS.values()) == 1
    assert len(CC.SURFEL_NAMES) >= 3
    for spec in CC.CAMERAS.values():     # the eye is where the table says it is
        m = max(abs(x) for x in spec["eye"])
        assert {"inside": m < 0.5, "edge": m == 0.5, "outside": m > 0.5}[spec["where"]]


@pytest.mark.parametrize("V", [3, 9])
def test_multiview_sets_have_clamped_gaussians_in_every_view(oracle_built, V):
    sc, cams, bgs, cases = CC.make_multiview_set(V)
    assert len({(c["tanfovx"], c["tanfovy"]) for c in cases}) == V and len({tuple(b.tolist()) for b in bgs}) == V
    assert len({c["tanfovx"] for c in cases}) == V and len({c["tanfovy"] for c in cases}) == V
    for j, c in enumerate(cases):
        assert (c["H"], c["W"]) == (CC.MV["H"], CC.MV["W"]) and c["tanfovx"] != c["tanfovy"]
        out, _ = U.run_oracle(c, "f32", nthreads=4)
        m = CC.branch_masks(c, out)
        assert int((m["clamp_x"] | m["clamp_y"]).sum()) >= CC.FLOOR, (V, j)
        assert int(m["clamp_x"].sum()) >= CC.FLOOR and int(m["clamp_y"].sum()) >= CC.FLOOR, (V, j)


# ---- (b) f64 C oracle == autograd in these branches -------------------------------------------------------------------------
@pytest.mark.parametrize("name", CC.NAMES)
def test_c_oracle_matches_autograd_on_camera_case(oracle_built, name):
    """The bars of test_oracle_cpu.py::test_c_oracle_backward_matches_autograd (forward 1e-12, radii equal, gradients 1e-10
    relative) on the reduced version of every case."""
    case = CC.make_camera_case(name, reduced=True)
    dt = torch.float64
    s = U.settings_np(case)
    out, og = U.run_oracle({k: (v.to(dt) if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in case.items()},
                           "f64", [g.to(dt) for g in U.rand_grads(case)])
    names = [k for k in ("means3D", "shs", "colors_precomp", "opacities", "scales", "rotations", "cov3D_precomp") if case[k] is not None]
    ins = {k: case[k].to(dt).requires_grad_(True) for k in names}
    probe = torch.zeros(case["N"], 4, dtype=dt, requires_grad=True)
    kw = {k: v for k, v in ins.items() if k not in ("means3D", "opacities")}
    c, r, d, a = torch_ref.render(ins["means3D"], ins["opacities"], means2D_probe=probe, **kw, **torch_ref.settings_kwargs(s))
    assert np.abs(c.detach().numpy() - out["color"]).max() < 1e-12
    assert np.abs(d.detach().numpy() - out["depth"]).max() < 1e-12
    assert np.abs(a.detach().numpy() - out["alpha"]).max() < 1e-12
    np.testing.assert_array_equal(r.numpy(), out["radii"])
    gc, gd, ga = [g.to(dt) for g in U.rand_grads(case)]
    gt = torch.autograd.grad((c * gc).sum() + (d * gd).sum() + (a * ga).sum(), list(ins.values()) + [probe])
    for k, g in zip(names + ["means2D"], gt):
        ref = g.numpy()
        got = og[k] if k == "means2D" else og[k].reshape(ref.shape)
        if k == "means2D":
            ref, got = ref[:, :2], got[:, :2]
        assert np.abs(ref).max() > 0, k
        assert np.abs(got - ref).max() <= 1e-10 * max(1.0, np.abs(ref).max()), k


@pytest.mark.parametrize("name", CC.SURFEL_NAMES)
def test_c_surfel_oracle_matches_autograd_on_camera_case(oracle_built, name):
    """The bars of test_oracle_surfel_cpu.py::test_c_surfel_oracle_matches_autograd on the reduced version of every case
    that is used for 2DGS."""
    case = CC.as_surfel(CC.make_camera_case(name, reduced=True))
    dt = torch.float64
    s = U.settings_np(case)
    ins = {k: case[k].to(dt).clone().requires_grad_(True) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    targs = {k: v for k, v in ins.items() if k not in ("means3D", "opacities")}
    c, r, am = TS.render(ins["means3D"], ins["opacities"], **targs, **torch_ref.settings_kwargs(s))
    o = SurfelOracle("f64")
    out = o.forward(ins["means3D"].detach().numpy(), ins["opacities"].detach().numpy(), s,
                    **{k: v.detach().numpy() for k, v in targs.items()})
    assert int((out["radii"] > 0).sum()) > 100
    m = CC.branch_masks(case, out)        # reach of the SURFEL projection: its own radii
    for b in case["branches"]:
        if b != "edges":
            assert int(m[b].sum()) >= CC.FLOOR_REDUCED, (name, b, int(m[b].sum()))
    assert np.abs(c.detach().numpy() - out["color"]).max() < 1e-12
    assert np.abs(am.detach().numpy() - out["allmap"]).max() < 1e-12
    np.testing.assert_array_equal(r.numpy(), out["radii"])
    gc, ga = [g.to(dt) for g in U.rand_surfel_grads(case)]
    gt = torch.autograd.grad((c * gc).sum() + (am * ga).sum(), list(ins.values()))
    og = o.backward(out, gc.numpy(), ga.numpy())
    for k, gg in zip(ins, gt):
        ref = gg.numpy()
        assert np.abs(og[k].reshape(ref.shape) - ref).max() <= 1e-10 * max(1.0, np.abs(ref).max()), k


# ---- (c) finite differences on Gaussians taken from the branches --------------------------------------------------------
@pytest.mark.parametrize("name", CC.NAMES)
def test_finite_differences_fp64_in_the_branches(oracle_built, name):
    """The pattern, tolerances and skip rule of test_oracle_cpu.py::test_finite_differences_fp64, the Gaussians drawn from the
    clamp branches and the near band instead of from all visible ones.  On a clamped Gaussian every input but means3D is
    perturbed at a random element.  For means3D the 3DGS backward is by convention NOT the derivative of the forward there
    (the clamped t.x = +-limx t.z is held constant: xmul = 0 and no d/dt.z term), so a clamped Gaussian is moved along the
    camera axis of its clamp, which leaves t.z — hence the clamped Jacobian — unchanged: the true directional derivative
    is then the one with xmul = 0, and a backward that kept the unclamped d/dt.x term fails this check.  means3D at a random
    element is checked on the unclamped Gaussians of the near band.
    A second skip rule (see `check`) drops a perturbation whose fd(eps) and fd(eps / 2) disagree.  It drops few: of 19-24
    attempts per case it skipped 1, 1, 0, 0, 1 (table order) and 23, 23, 24, 10, 19 checks survived; a case where it
    skipped more than a quarter of the attempts fails."""
    case = CC.make_camera_case(name, reduced=True)
    o = Oracle("f64")
    s = U.settings_np(case)
    gc, gd, ga = [g.numpy().astype(np.float64) for g in U.rand_grads(case)]
    names = [k for k in ("means3D", "shs", "colors_precomp", "opacities", "scales", "rotations", "cov3D_precomp") if case[k] is not None]
    base = {k: case[k].numpy().astype(np.float64) for k in names}

    def loss(inp):
        out = o.forward(inp["means3D"], inp["opacities"], s, **{k: v for k, v in inp.items() if k not in ("means3D", "opacities")})
        return float((out["color"] * gc).sum() + (out["depth"] * gd).sum() + (out["alpha"] * ga).sum()), out

    l0, out0 = loss(base)
    g = o.backward(out0, gc, gd, ga)
    m = CC.branch_masks(case, out0)
    nz = np.abs(g["means3D"]).max(axis=1) > 0
    clamped = {"x": np.nonzero(m["clamp_x"] & ~m["clamp_y"] & nz)[0], "y": np.nonzero(m["clamp_y"] & ~m["clamp_x"] & nz)[0]}
    any_clamped = np.nonzero((m["clamp_x"] | m["clamp_y"]) & nz)[0]
    near_free = np.nonzero(m["near"] & ~m["clamp_x"] & ~m["clamp_y"] & nz)[0]
    free = near_free if near_free.size else np.nonzero((out0["radii"] > 0) & ~m["clamp_x"] & ~m["clamp_y"] & nz)[0]
    rng = np.random.default_rng(0)
    eps = 1e-6
    cam_axis = case["view"].double().numpy()[:3, :3]        # column a = world direction of camera axis a
    checked, skipped = dict(clamped=0, other=0), dict(clamped=0, other=0)

    def fd_of(k, i, direction, h):
        p, q = {kk: v.copy() for kk, v in base.items()}, {kk: v.copy() for kk, v in base.items()}
        p[k][i] += h * direction
        q[k][i] -= h * direction
        lp, op = loss(p)
        lq, oq = loss(q)
        same = (np.array_equal(op["n_contrib"], out0["n_contrib"]) and np.array_equal(oq["n_contrib"], out0["n_contrib"])
                and np.array_equal(op["radii"], out0["radii"]) and np.array_equal(oq["radii"], out0["radii"]))
        return (lp - lq) / (2 * h), same

    def check(kind, k, i, direction):
        fd, same = fd_of(k, i, direction, eps)
        if not same:
            return  # perturbation crossed a discontinuity (skip rule): FD not meaningful
        # The Gaussians of these branches cover thousands of pixels, and a pixel whose alpha crosses 1/255 in the MIDDLE of
        # a list changes neither n_contrib nor the radii.  Such a jump J shows as fd(eps) - fd(eps / 2) = -J / (2 eps); a
        # smooth loss gives O(eps^2).  The decision does not look at the analytic gradient.
        fd_half, same = fd_of(k, i, direction, 0.5 * eps)
        if not same or abs(fd - fd_half) > 1e-5 * max(1.0, abs(fd_half)) + 1e-6:
            skipped[kind] += 1
            return
        an = float((g[k].reshape(base[k].shape)[i] * direction).sum())
        assert abs(fd - an) <= 1e-5 * max(1.0, abs(an)) + 1e-6, (name, kind, k, i, fd, an)
        checked[kind] += 1

    def unit(shape):
        d = np.zeros(shape)
        d[tuple(int(rng.integers(0, n)) for n in shape)] = 1.0
        return d

    for axis, col in (("x", 0), ("y", 1)):                  # means3D of clamped Gaussians, along the axis of the clamp
        for i in clamped[axis][:3]:
            check("clamped", "means3D", int(i), cam_axis[:, col].copy())
    for k in names:
        if k != "means3D" and any_clamped.size:
            for _ in range(2):
                check("clamped", k, int(rng.choice(any_clamped)), unit(base[k].shape[1:]))
        for _ in range(2):
            check("other", k, int(rng.choice(free)), unit(base[k].shape[1:]))
    print(name, "checked", checked, "alpha-threshold skips", skipped, "clamped x only / y only:", clamped["x"].size, clamped["y"].size, "near unclamped:", near_free.size)
    assert checked["clamped"] + checked["other"] >= 10
    assert 4 * (skipped["clamped"] + skipped["other"]) <= checked["clamped"] + checked["other"]
    if "clamp_x" in case["branches"] or "clamp_y" in case["branches"]:
        assert checked["clamped"] >= 4
    if "near" in case["branches"]:
        assert near_free.size > 0 and checked["other"] >= 4


# ---- (d) the cases discriminate ---------------------------------------------------------------------------------------
def _fails(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def _straight_through_clamp_term(case, out64, g64):
    """d(means3D) that a backward with xmul = ymul = 1 would ADD: the un-clamped variant of torch_ref's EWA projection
    (the clamped t.x, t.y carry the gradient of the unclamped ones), differentiated against the oracle's own dL/dconic."""
    dt = torch.float64
    means = case["means3D"].to(dt).requires_grad_(True)
    V = case["view"].to(dt)
    if case["cov3D_precomp"] is None:
        Mm = torch_ref.quat_to_R(case["rotations"].to(dt)) * (case["scale_modifier"] * case["scales"].to(dt))[:, None, :]
        Sigma = Mm @ Mm.transpose(1, 2)
    else:
        c = case["cov3D_precomp"].to(dt)
        Sigma = torch.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]], 1).reshape(-1, 3, 3)
    vis = torch.from_numpy(out64["radii"] > 0)
    dconic = torch.from_numpy(np.asarray(g64["_partial"]["conic"], np.float64)[:, :3])

    def grad(straight_through):
        pv = means @ V[:3, :3] + V[3, :3]
        tz = pv[:, 2]
        t = []
        for a, lim in ((0, 1.3 * case["tanfovx"]), (1, 1.3 * case["tanfovy"])):
            r = (pv[:, a] / tz).detach()
            held = (r.clamp(-lim, lim) * tz).detach()
            if straight_through:
                held = held + pv[:, a] - pv[:, a].detach()
            t.append(torch.where(r.abs() > lim, held, pv[:, a]))
        fx, fy = case["W"] / (2 * case["tanfovx"]), case["H"] / (2 * case["tanfovy"])
        zero = torch.zeros_like(tz)
        J = torch.stack([fx / tz, zero, -fx * t[0] / (tz * tz), zero, fy / tz, -fy * t[1] / (tz * tz)], 1).reshape(-1, 2, 3)
        A = J @ V[:3, :3].T
        cov2 = A @ Sigma @ A.transpose(1, 2)
        a_, b_, c_ = cov2[:, 0, 0] + 0.3, cov2[:, 0, 1], cov2[:, 1, 1] + 0.3
        det = a_ * c_ - b_ * b_
        conic = torch.stack([c_ / det, -b_ / det, a_ / det], 1)
        return torch.autograd.grad((conic * dconic)[vis].sum(), means)[0].numpy()

    return grad(True) - grad(False)


def _mutant_results(case):
    """{mutant: (fails the bit-exact radii comparison, fails util.assert_grads)} against the correct oracle."""
    grads = U.rand_grads(case)
    keys = _keys(case)
    o32, g32 = U.run_oracle(case, "f32", grads, nthreads=4)
    o64, g64 = U.run_oracle(case, "f64", grads, nthreads=4)
    res = {}

    def judge(tag, om, gm):
        res[tag] = (om is not None and not np.array_equal(om["radii"], o32["radii"]),
                    _fails(lambda: U.assert_grads(gm, g64, g32, keys, f"{case.get('name', 'orbit')} {tag}")))

    swapped = dict(case, tanfovx=case["tanfovy"], tanfovy=case["tanfovx"])
    judge("tanfov exchanged", *U.run_oracle(swapped, "f32", grads, nthreads=4))
    judge("scale_modifier = 1", *U.run_oracle(dict(case, scale_modifier=1.0), "f32", grads, nthreads=4))
    extra = _straight_through_clamp_term(case, o64, g64)
    gm = dict(g32, means3D=(g32["means3D"].astype(np.float64) + extra).astype(np.float32))
    judge("xmul = ymul = 1", None, gm)
    res["_extra_rel"] = float(np.abs(extra).max() / np.abs(g64["means3D"]).max())
    return res


@pytest.mark.parametrize("name", CC.NAMES)
def test_cases_tell_a_wrong_camera_from_a_right_one(oracle_built, name):
    """Three wrong rasterizers, emulated with the oracle: tan(fovx/2) and tan(fovy/2) exchanged, scale_modifier ignored, and
    the frustum clamp's xmul / ymul left at 1 in the backward.  Each must FAIL against the correct oracle — the first two
    both the bit-exact radii comparison and util.assert_grads, the third util.assert_grads — or the case is not doing its
    job.  (scale_modifier: on the cases where it is not 1 and acts, i.e. not with cov3D_precomp; xmul / ymul: on the cases
    that claim a clamp branch.)  With the orbit camera of the rest of the suite none of them is noticed: see
    test_orbit_camera_does_not_tell_them_apart."""
    case = CC.make_camera_case(name)
    res = _mutant_results(case)
    print(name, res)
    assert res["tanfov exchanged"] == (True, True)
    if case["scale_modifier"] != 1.0 and case["cov3D_precomp"] is None:
        assert res["scale_modifier = 1"] == (True, True)
    if "clamp_x" in case["branches"] or "clamp_y" in case["branches"]:
        assert res["xmul = ymul = 1"][1]


def test_orbit_camera_does_not_tell_them_apart(oracle_built):
    """The same three mutants on test_gpu_parity.py's case (3000, 250, 190, seed 3) — orbit camera, fovx == fovy,
    scale_modifier 1: all three pass every check (radii identical, 0 gradient elements outside; the xmul / ymul term is
    exactly 0.0 because no visible Gaussian is in the clamp), which is why the suite could not see such an error before.
    On the table's cases that claim a clamp branch the xmul / ymul term alone is 1.2e-2 to 7.8e-2 of the largest means3D
    gradient, against a bar of 1e-4."""
    case = U.make_case(3_000, 250, 190, 3, deg=3, sigma0=(0.03, 0.01))
    res = _mutant_results(case)
    print("orbit", res)
    assert res["tanfov exchanged"] == (False, False)
    assert res["scale_modifier = 1"] == (False, False)
    assert res["xmul = ymul = 1"] == (False, False) and res["_extra_rel"] == 0.0
