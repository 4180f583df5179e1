"""GPU: simple_knn._C.distCUDA2 (generativedensification_amd/knn.py -> csrc/knn.hip) on the clouds of knn_cases.py:
exact against the f64 brute force, independent of the grid bit for bit, the drop-in's contract, and the WORK of the
search (candidates examined per point, reported by the kernel) bounded against the uniform cloud's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import knn_cases as KC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (4, 5, 255, 256, 257, 20_000)


def _dist2(pts, **kw):
    from generativedensification_amd.knn import dist2

    return dist2(torch.from_numpy(pts).to(DEV) if isinstance(pts, np.ndarray) else pts, **kw)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("family", KC.FAMILIES)
def test_exact_against_f64_brute_force(oracle_built, family, N):
    """Every family at the launch edges and at 20 000 points == the f64 brute force of the float32-rounded points, at the
    bar of test_gpu_surfel.py (rtol 1e-5, atol 1e-12); exact zeros where three other points coincide with a point."""
    from oracle.gsr_oracle import knn_mean_dist2
    from simple_knn._C import distCUDA2

    pts = KC.make(family, N)
    ref = knn_mean_dist2(pts, "f64", nthreads=16)
    got = distCUDA2(torch.from_numpy(pts).to(DEV)).cpu().numpy()
    assert got.shape == (N,) and got.dtype == np.float32
    err = np.abs(got - ref) / np.maximum(ref, 1e-30)
    print(f"{family} N={N}: max rel err {err.max():.2e}")
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-12)
    zero = KC.multiplicity(pts) >= 4
    assert (got[zero] == 0).all() and (ref[zero] == 0).all()
    if family == "coincident":
        assert zero.all()
    if family == "duplicates" and N >= 255:
        assert zero.any() and not zero.all() and (got[~zero] > 0).all()


@pytest.mark.parametrize("N", (0, 1, 3))
@pytest.mark.parametrize("family", ("uniform", "coincident", "plane"))
def test_fewer_than_four_points(family, N):
    """N < 4: inf (the lineage's `best = FLT_MAX` left in place); N = 0: an empty tensor."""
    got, work = _dist2(KC.make(family, N), return_work=True)
    assert got.shape == (N,) and got.dtype == torch.float32 and work.shape == (N,)
    assert torch.isinf(got).all() and (got > 0).all()
    assert (work.cpu() == max(N - 1, 0)).all()


@pytest.mark.parametrize("family", KC.FAMILIES)
def test_result_does_not_depend_on_the_grid(family):
    """cells_per_axis in {1, 7, default, 64}: bitwise equal.  The search is exact and every distance is the same
    expression of the same floats, so no tolerance applies.  (One cell = brute force: only at N = 5000.)"""
    for N, grids in ((20_000, (7, None, 64)), (5_000, (1, 7, None, 64))):
        pts = torch.from_numpy(KC.make(family, N)).to(DEV)
        outs = {g: _dist2(pts, cells_per_axis=g).cpu().numpy() for g in grids}
        for g in grids:
            assert np.array_equal(outs[g].view(np.uint32), outs[None].view(np.uint32)), (family, N, g, np.abs(
                outs[g] - outs[None]).max())


def test_contract_dtypes_layout_grad_stream_determinism():
    from simple_knn._C import distCUDA2

    base = KC.make("uniform", 3001) * 4.0
    f32 = torch.from_numpy(base).to(DEV)
    ref = distCUDA2(f32)
    assert ref.dtype == torch.float32 and ref.device == f32.device and ref.shape == (3001,) and not ref.requires_grad
    assert torch.equal(distCUDA2(f32), ref)                                   # two runs, bit for bit
    # other dtypes == the result for the input rounded to float32
    f64 = torch.from_numpy(base.astype(np.float64) * (1 + 2.0 ** -30)).to(DEV)
    assert f64.dtype == torch.float64 and torch.equal(distCUDA2(f64), distCUDA2(f64.to(torch.float32)))
    for dt in (torch.float16, torch.bfloat16):
        h = f32.to(dt)
        got = distCUDA2(h)
        assert got.dtype == torch.float32 and torch.equal(got, distCUDA2(h.to(torch.float32)))
    # a non-contiguous (N, 3) slice
    wide = torch.zeros(3001, 7, device=DEV)
    wide[:, 1:7:2] = f32
    sl = wide[:, 1:7:2]
    assert not sl.is_contiguous() and torch.equal(distCUDA2(sl), ref)
    # requires_grad in, no grad out
    leaf = f32.clone().requires_grad_(True)
    got = distCUDA2(leaf)
    assert torch.equal(got, ref) and not got.requires_grad and got.grad_fn is None
    # a non-default stream
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        on_s = distCUDA2(f32)
    s.synchronize()
    assert torch.equal(on_s, ref)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        distCUDA2(f32.cpu())


def test_non_finite_points_return_and_leave_finite_clouds_alone():
    """NaN / Inf coordinates are outside the contract (upstream's behaviour is unspecified): the call returns, and a finite
    cloud gives the same result before and after."""
    pts = KC.make("uniform", 64)
    before = _dist2(pts)
    bad = pts.copy()
    bad[3, 1], bad[17, 0], bad[40, 2] = np.nan, np.inf, -np.inf
    got = _dist2(bad)
    torch.cuda.synchronize()
    assert got.shape == (64,)
    assert torch.equal(_dist2(pts), before)


def _work_child(N, timeout):
    p = subprocess.run([sys.executable, os.path.join(HERE, "knn_work.py"), str(N)], capture_output=True, text=True,
                       timeout=timeout)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("KNN_WORK ")][-1]
    return json.loads(line[len("KNN_WORK "):])


def test_work_is_bounded():
    """W(family, N) = mean over the points of the candidates the kernel examined.  At N = 20 000 and 160 000:
      * offset_*, aniso, plane, near_plane, line, outliers_*: W <= (125 / 27) W(uniform, N), the uniform cloud measured in
        the same run; 125 / 27 = one cubic shell more than the 3 x 3 x 3 block the uniform cloud needs, the only slack;
      * coincident and duplicates: a point with three other points at its own location examines no more candidates than
        its own cell holds (the scan starts there and leaves at the third zero).  The points of `duplicates` with fewer
        copies have a non-zero answer, which no exact search finds inside one cell of ~2 points; they are covered by the
        exactness test, not by this bound;
      * coincident: W does not grow with N;
      * clusters, lattice: no cap (a uniform grid cannot serve two scales); printed.
    Each N runs in a child process under a time limit: a quadratic search at 160 000 points is 2.6e10 distance
    evaluations in one kernel."""
    res = {}
    for N in (20_000, 160_000):
        res[N] = r = _work_child(N, timeout=420)
        for fam in KC.FAMILIES:
            print(f"W({fam}, {N}) = {r[fam]['W']:.1f}  max {r[fam]['max']}  cells {r[fam]['gdim']}  "
                  f"[points with 3 copies elsewhere: {r[fam]['zero_points']}, W {r[fam]['W_zero']:.1f}, "
                  f"own cell {r[fam]['pop_zero']:.1f}]")
    for N, r in res.items():
        cap = KC.WORK_SLACK * r["uniform"]["W"]
        for fam in KC.CAPPED:
            assert r[fam]["W"] <= cap, (fam, N, r[fam]["W"], cap)
        for fam in ("coincident", "duplicates"):
            assert r[fam]["zero_points"] > 0 and r[fam]["zero_over_cell"] == 0 and r[fam]["out_zero_wrong"] == 0, (fam, N, r[fam])
            assert r[fam]["W_zero"] <= r[fam]["pop_zero"]
        assert r["coincident"]["zero_points"] == N
    assert res[160_000]["coincident"]["W"] <= res[20_000]["coincident"]["W"]
