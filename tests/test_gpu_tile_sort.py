"""-m gpu: the per-tile depth sort of lists of up to 4096 entries (csrc/binning.hip tile_sort_kernel) under both of its
modes — K.TILE_SORT_MODE 1: stable 8-bit radix passes + tie pass; 2: one counting pass on 4096 depth buckets + in-bucket
fix-up, radix for a list that puts more than 16 entries into one bucket — against the float32 oracle: ranges, point_list
and keys_sorted bit for bit, under both scatter modes (the order in which a tile's entries arrive differs between them).

Every case is one to three 16 x 16 tiles under an identity camera (view depth = the Gaussian's z, bit for bit); the
Gaussians are as small as the rasterizer makes them (the 0.3 px^2 dilation gives a 2 px radius) and sit on the centre of
their tile, so a tile's list is exactly the Gaussians placed on it, with the depths the case chose.  Which path a tile must
take is computed here from the ORACLE's depth keys with the bucket map of binning.hip, and the library's debug counter of
lists that left the bucket path has to agree: a case meant for the bucket path shows 0, so a silent fallback cannot hide a
broken bucket path."""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest
import torch

import util as U

pytestmark = pytest.mark.gpu

BUCKETS_LOG2 = 12       # binning.hip GDR_TSORT_BUCKETS = 4096
BUCKET_MAX = 16         # binning.hip GDR_TSORT_BUCKET_MAX
LDS_LIST = 4096         # GDR_TSORT_MEDIUM: longer lists belong to the long class (radix, not counted)
ONE = 0x3F800000        # float bits of 1.0: 2^23 ulps to 2.0, another 2^23 to 4.0


def _z(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def make_tile_case(tile_depths, seed=0):
    """One Gaussian per entry of tile_depths[t] (float32 view depths, in id order) on the centre of tile t of a
    (16 * len(tile_depths)) x 16 image, ids running tile after tile."""
    from generativedensification_amd.camera import MiniCam

    T = len(tile_depths)
    W, H = 16 * T, 16
    z = np.concatenate([np.asarray(d, np.float32) for d in tile_depths])
    n = int(z.size)
    case = U.make_case(n, H, W, seed, deg=0, sigma0=(1e-4,))
    tile = np.concatenate([np.full(len(d), t) for t, d in enumerate(tile_depths)])
    ndc = (2.0 * (16 * tile + 7.5) + 1.0) / W - 1.0
    means = np.zeros((n, 3), np.float32)
    means[:, 0] = (ndc * math.tan(U.FOV * 0.5) * z.astype(np.float64)).astype(np.float32)
    means[:, 2] = z
    cam = MiniCam(torch.eye(4), W, H, U.FOV, U.FOV, 0.5, 10.0, "cpu")
    case.update(means3D=torch.from_numpy(means), scales=torch.full((n, 3), 1e-4),
                opacities=torch.full((n, 1), 0.05),
                view=cam.world_view_transform.contiguous(), proj=cam.full_proj_transform.contiguous(),
                campos=cam.camera_center.contiguous())
    return case


def _depth_keys(o):
    """The oracle's depth bits in list order."""
    if "keys_sorted" in o:
        return (np.asarray(o["keys_sorted"]).view(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return np.asarray(o["depths"], np.float32).view(np.uint32)[np.asarray(o["point_list"]).astype(np.int64)].astype(np.int64)


def largest_buckets(o):
    """Per tile: (list length, largest bucket count under binning.hip's map b = (key - kmin) >> max(0, bits(span) - 12))."""
    keys, out = _depth_keys(o), []
    for lo, hi in np.asarray(o["ranges"]).astype(np.int64):
        k = keys[lo:hi]
        if k.size == 0:
            out.append((0, 0))
            continue
        span = int(k.max() - k.min())
        shift = max(0, span.bit_length() - BUCKETS_LOG2)
        b = (k - k.min()) >> shift
        assert b.max() < (1 << BUCKETS_LOG2)
        out.append((int(k.size), int(np.bincount(b).max())))
    return out


def expected_fallbacks(o):
    return sum(1 for n, big in largest_buckets(o) if 0 < n <= LDS_LIST and big > BUCKET_MAX)


class _knobs:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        from generativedensification_amd import rasterizer as R

        self.saved = {k: getattr(R.K, k) for k in self.kw}
        for k, v in self.kw.items():
            setattr(R.K, k, v)

    def __exit__(self, *a):
        from generativedensification_amd import rasterizer as R

        for k, v in self.saved.items():
            setattr(R.K, k, v)


def _assert_equal(h, o, tag):
    assert h["num_rendered"] == o["num_rendered"], tag
    np.testing.assert_array_equal(h["ranges"].view(np.uint32), o["ranges"], err_msg=f"ranges, {tag}")
    np.testing.assert_array_equal(h["point_list"].view(np.uint32), o["point_list"], err_msg=f"point_list, {tag}")
    np.testing.assert_array_equal(h["keys_sorted"].view(np.uint64), o["keys_sorted"], err_msg=f"keys_sorted, {tag}")


def check(case, o, run=None, equal=_assert_equal, **knobs):
    """Both sort modes x both scatter modes against the oracle; the fallback counter against the oracle's bucket map
    (bucket mode: the lists with an overfull bucket; radix mode never tries the bucket path: 0).  The first call of a scene
    shape has no history and is planned twice (the lists may be sorted twice): it is not counted."""
    from generativedensification_amd import _debug as K

    run = run or (lambda c: [U.run_hip(c)[0]])
    oracles = o if isinstance(o, list) else [o]
    want = sum(expected_fallbacks(x) for x in oracles)
    with _knobs(**knobs):
        run(case)
        for sort_mode in (1, 2):
            for scatter_mode in (1, 2):
                with _knobs(TILE_SORT_MODE=sort_mode, SCATTER_MODE=scatter_mode):
                    K.tile_sort_fallbacks(reset=True)
                    hs = run(case)
                    got = K.tile_sort_fallbacks(reset=True)
                tag = f"sort mode {sort_mode}, scatter mode {scatter_mode}"
                for v, (h, x) in enumerate(zip(hs, oracles)):
                    equal(h, x, f"{tag}, view {v}")
                print(f"{tag}: fallbacks {got}, expected {want if sort_mode == 2 else 0}; (length, largest bucket) "
                      f"{[largest_buckets(x) for x in oracles]}")
                assert got == (want if sort_mode == 2 else 0), tag
    return want


def _uniform(rng, n, lo=1.4, hi=2.4):
    return rng.uniform(lo, hi, n).astype(np.float32)


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097])
def test_list_lengths(oracle_built, n):
    """Around the wave, the short / medium boundary (2048) and the LDS capacity (4096); 4097 stays on the long class
    (launch hints off, so that the long class is launched whatever earlier tests saw).  Uniform depths: bucket path."""
    case = make_tile_case([_uniform(np.random.default_rng(n), n)], seed=n)
    o, _ = U.run_oracle(case, "f32")
    assert largest_buckets(o)[0][0] == n
    assert check(case, o, LAUNCH_HINTS=n <= LDS_LIST) == 0


def test_all_depths_equal(oracle_built):
    """Span 0: everything in bucket 0, the tile falls back and the ids ascend."""
    case = make_tile_case([np.full(300, 1.75, np.float32)])
    o, _ = U.run_oracle(case, "f32")
    assert largest_buckets(o) == [(300, 300)]
    np.testing.assert_array_equal(o["point_list"], np.arange(300))
    assert check(case, o) == 1


def test_all_depths_equal_short_enough_for_one_bucket(oracle_built):
    """Span 0 with 16 entries: one bucket at the threshold, sorted by id by the fix-up alone."""
    case = make_tile_case([np.full(16, 1.75, np.float32)])
    o, _ = U.run_oracle(case, "f32")
    assert largest_buckets(o) == [(16, 16)]
    assert check(case, o) == 0


def test_span_below_the_bucket_count(oracle_built):
    """Span < 4096 ulps: shift 0, one key value per bucket.  Equal depths go to ids in DESCENDING memory order (depths
    descend with the id), so the fix-up has to reverse every bucket."""
    rng = np.random.default_rng(3)
    off = np.sort(rng.integers(0, 3000, 1000))[::-1]
    case = make_tile_case([_z(ONE + (1 << 22) + off)])
    o, _ = U.run_oracle(case, "f32")
    (n, big), = largest_buckets(o)
    keys = _depth_keys(o)
    assert n == 1000 and 2 <= big <= BUCKET_MAX and keys.max() - keys.min() < 4096 and (keys[1:] == keys[:-1]).sum() > 50
    assert check(case, o) == 0


@pytest.mark.parametrize("span", [4095, 4096, 4097, 1 << 23])
def test_power_of_two_span_edges(oracle_built, span):
    """The span decides the shift: exactly 4095 (shift 0, last bucket 4095), 4096 and 4097 (shift 1), 2^23 (shift 12; from
    1.0 to 2.0 exactly)."""
    rng = np.random.default_rng(span)
    off = np.concatenate([[0, span], rng.integers(0, span + 1, 1498)])
    case = make_tile_case([_z(ONE + rng.permutation(off))], seed=span % 97)
    o, _ = U.run_oracle(case, "f32")
    keys = _depth_keys(o)
    assert keys.max() - keys.min() == span
    assert check(case, o) == 0


def test_binade_crossing(oracle_built):
    """Depths on both sides of 2.0, where the float bits change their step."""
    z = _uniform(np.random.default_rng(5), 1200, 1.9, 2.1)
    assert (z < 2.0).sum() > 100 and (z >= 2.0).sum() > 100
    case = make_tile_case([z], seed=5)
    o, _ = U.run_oracle(case, "f32")
    assert check(case, o) == 0


@pytest.mark.parametrize("full", [16, 17])
def test_threshold_edge(oracle_built, full):
    """One bucket holds exactly 16 / 17 entries, every other at most one: 16 stays on the bucket path, 17 falls back."""
    rng = np.random.default_rng(full)
    shift = 12                                            # span 2^24 - 1: 24 bits, buckets of 4096 ulps
    others = rng.choice(np.arange(1, 4095), 1001, replace=False)
    crowded, others = others[0], others[1:]
    off = np.concatenate([[0, (1 << 24) - 1],
                          (others << shift) + rng.integers(0, 1 << shift, others.size),
                          (crowded << shift) + rng.choice(1 << shift, full, replace=False)])
    case = make_tile_case([_z(ONE + rng.permutation(off))], seed=full)
    o, _ = U.run_oracle(case, "f32")
    assert largest_buckets(o) == [(1002 + full, full)]
    assert check(case, o) == (0 if full == 16 else 1)


def test_two_clusters_and_a_far_outlier(oracle_built):
    """Two tight clusters share the first bucket because one far entry stretches the span: about L / 2 in it."""
    rng = np.random.default_rng(8)
    off = np.concatenate([rng.integers(0, 50, 500), 2000 + rng.integers(0, 50, 499), [1 << 24]])
    case = make_tile_case([_z(ONE + rng.permutation(off))], seed=8)
    o, _ = U.run_oracle(case, "f32")
    (n, big), = largest_buckets(o)
    assert n == 1000 and big == 999
    assert check(case, o) == 1


@functools.lru_cache(maxsize=None)
def _mixed():
    rng = np.random.default_rng(9)
    case = make_tile_case([_uniform(rng, 800), np.full(100, 2.0, np.float32), np.zeros(0, np.float32)], seed=9)
    return case, U.run_oracle(case, "f32")[0]


def test_bucket_fallback_and_empty_tile_in_one_launch(oracle_built):
    case, o = _mixed()
    lb = largest_buckets(o)
    assert lb[0][0] == 800 and lb[0][1] <= BUCKET_MAX and lb[1] == (100, 100) and lb[2] == (0, 0)
    assert check(case, o) == 1


def test_two_array_input(oracle_built):
    """The radix partition on the tile bits hands the sort keys and ids in two arrays instead of packed words."""
    case, o = _mixed()
    assert check(case, o, FORCE_RADIX_PARTITION=True) == 1


def test_three_views_in_one_node(oracle_built):
    """blockIdx.y = view: three cameras along the view axis, a uniform tile and a clustered tile in each."""
    from generativedensification_amd import rasterizer as R
    from generativedensification_amd.camera import MiniCam

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(11)
    clustered = np.concatenate([_z(ONE + (1 << 22) + rng.integers(0, 40, 399)), [np.float32(2.4)]]).astype(np.float32)
    case = make_tile_case([_uniform(rng, 600), clustered], seed=11)
    sets = []
    for tz in (0.0, -0.25, 0.125):
        c2w = torch.eye(4)
        c2w[2, 3] = tz
        c = MiniCam(c2w, case["W"], case["H"], U.FOV, U.FOV, 0.5, 10.0, "cpu")
        sets.append(dict(case, view=c.world_view_transform.contiguous(), proj=c.full_proj_transform.contiguous(),
                         campos=c.camera_center.contiguous()))
    oracles = [U.run_oracle(cc, "f32")[0] for cc in sets]
    for o in oracles:
        assert [n for n, _ in largest_buckets(o)] == [600, 400]
    t = lambda k: case[k].to(dev)

    def run(_):
        out = R._forward_views_impl(t("means3D"), torch.zeros(case["N"], 4, device=dev), t("shs"), t("opacities"), t("scales"),
                                    t("rotations"), [U.settings_torch(cc, dev) for cc in sets], 0)
        torch.cuda.synchronize()
        return [{k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in st.tensors().items()}
                for st in out[4]]

    assert check(case, oracles, run=run) >= 3


def test_surfel_lists(oracle_built):
    """The surfel path shares the binning stage."""
    case = U.make_surfel_case(3_000, 80, 112, 19, deg=1, sigma0=(0.01, 0.002))
    o, _ = U.run_surfel_oracle(case, "f32")
    assert max(n for n, _ in largest_buckets(o)) > 64

    def equal(h, x, tag):
        np.testing.assert_array_equal(h["ranges"].view(np.uint32), x["ranges"], err_msg=f"ranges, {tag}")
        np.testing.assert_array_equal(h["point_list"].view(np.uint32), x["point_list"], err_msg=f"point_list, {tag}")
        np.testing.assert_array_equal(h["keys_sorted"].view(np.uint64) & np.uint64(0xFFFFFFFF),
                                      _depth_keys(x).astype(np.uint64), err_msg=f"depth keys, {tag}")

    check(case, o, run=lambda c: [U.run_surfel_hip(c)[0]], equal=equal)
