"""-m gpu: the two ways tile_scatter (csrc/binning.hip) writes the tile-partitioned list — direct (one store per entry,
K.SCATTER_MODE 1) and staged in LDS and written out in runs (2) — against the float32 oracle.  The partition may differ by a
permutation within a tile; the per-tile sort orders by (depth, Gaussian id), so the sorted lists, keys and ranges must be
the oracle's bit for bit under either mode.  Every case asserts, from the oracle, the property it is there for."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest
import torch

import util as U

pytestmark = pytest.mark.gpu

CHUNK = 1024      # Gaussians per workgroup of tile_count / tile_scatter at these sizes (N <= 256 * 1024: bin_geometry)


def stage_capacity(tiles):
    """Entries the staged kernel can hold for an image of `tiles` tiles (binning.hip stage_capacity: what the two per-tile
    tables leave of 160 KB - 256 B of LDS, 8 bytes per entry)."""
    return (160 * 1024 - 256 - 8 * tiles) // 8


def _tiles(case):
    return ((case["W"] + 15) // 16) * ((case["H"] + 15) // 16)


def _chunk_entries(o, n):
    """Duplicates per workgroup chunk, from the oracle's tiles_touched (0 for a culled Gaussian)."""
    tt = np.where(np.asarray(o["radii"]) > 0, np.asarray(o["tiles_touched"]).astype(np.int64), 0)
    pad = (-n) % CHUNK
    return np.concatenate([tt, np.zeros(pad, np.int64)]).reshape(-1, CHUNK).sum(1)


def _run_mode(case, mode):
    from generativedensification_amd import rasterizer as R

    saved = R.K.SCATTER_MODE
    R.K.SCATTER_MODE = mode
    try:
        return U.run_hip(case)[0]
    finally:
        R.K.SCATTER_MODE = saved


def _assert_lists(case, o):
    for mode in (1, 2):
        h = _run_mode(case, mode)
        assert h["num_rendered"] == o["num_rendered"], mode
        np.testing.assert_array_equal(h["ranges"].view(np.uint32), o["ranges"], err_msg=f"ranges, mode {mode}")
        np.testing.assert_array_equal(h["point_list"].view(np.uint32), o["point_list"], err_msg=f"point_list, mode {mode}")
        np.testing.assert_array_equal(h["keys_sorted"].view(np.uint64), o["keys_sorted"], err_msg=f"keys_sorted, mode {mode}")


def _behind_camera(case, ids):
    """Move the Gaussians `ids` far behind the camera (culled by K1: radius 0, no tile)."""
    axis = case["view"][:3, 2].clone()
    axis = axis / axis.norm()
    m = case["means3D"].clone()
    m[ids] = case["campos"][None, :] - 5.0 * axis[None, :] + 0.01 * m[ids]
    case["means3D"] = m.contiguous()


@functools.lru_cache(maxsize=None)
def _several():
    case = U.make_case(5_000, 112, 160, 3, deg=1)
    return case, U.run_oracle(case, "f32")[0]


@pytest.mark.parametrize("n", [1_500, 1_025])
def test_two_workgroups_and_a_ragged_tile_count(oracle_built, n):
    """5 x 3 tiles (not a multiple of 64), two workgroups; the second chunk is partly empty — at N = 1025 it holds ONE
    Gaussian, and its counts come from the totals row."""
    case = U.make_case(n, 40, 72, 7, deg=0, sigma0=(0.004,))
    o, _ = U.run_oracle(case, "f32")
    per = _chunk_entries(o, n)
    assert _tiles(case) == 15 and per.size == 2 and per[0] > 0 and per.sum() == o["num_rendered"]
    if n == 1_025:      # the one Gaussian of the last workgroup must be visible, or that workgroup has nothing to place
        if o["radii"][1024] <= 0 or o["tiles_touched"][1024] == 0:
            case["means3D"][1024] = case["means3D"][int(np.argmax(np.asarray(o["tiles_touched"]) * (np.asarray(o["radii"]) > 0)))]
            o, _ = U.run_oracle(case, "f32")
            per = _chunk_entries(o, n)
        assert per[1] == o["tiles_touched"][1024] > 0
    else:
        assert 0 < per[1] < per[0]
    assert per.max() <= stage_capacity(15)
    _assert_lists(case, o)


def test_several_workgroups(oracle_built):
    """70 tiles (row stride 128), 5 workgroups: with the XCD row map the grid is 8 workgroups, 3 of them without a row."""
    case, o = _several()
    per = _chunk_entries(o, case["N"])
    assert _tiles(case) == 70 and per.size == 5 and (per > 0).all() and per.max() <= stage_capacity(70)
    _assert_lists(case, o)


def test_staged_and_direct_chunks_in_one_launch(oracle_built):
    """The first workgroup's Gaussians cover every tile: its entries exceed the staging buffer and it takes the direct
    route; the other four workgroups stage theirs."""
    base, _ = _several()
    case = dict(base)
    sc = case["scales"].clone()
    sc[:CHUNK] = 1.5
    case["scales"] = sc.contiguous()
    op = case["opacities"].clone()
    op[:CHUNK] = 0.02       # (keeps the images from saturating after a handful of contributors)
    case["opacities"] = op.contiguous()
    o, _ = U.run_oracle(case, "f32")
    per = _chunk_entries(o, case["N"])
    cap = stage_capacity(70)
    assert per[0] > cap and (per[1:] <= cap).all() and (per[1:] > 0).all(), (per, cap)
    _assert_lists(case, o)


def test_nothing_to_do_empty_tiles_and_a_tile_of_the_last_workgroup(oracle_built):
    """Culled Gaussians (behind the camera: radius 0) between visible ones, a tile no Gaussian touches, and a tile only the
    last workgroup feeds."""
    n = 3_000
    case = U.make_case(n, 64, 96, 13, deg=0, sigma0=(0.003,))
    o, _ = U.run_oracle(case, "f32")
    r = np.asarray(o["ranges"]).astype(np.int64)
    pl = np.asarray(o["point_list"]).astype(np.int64)
    length = r[:, 1] - r[:, 0]
    order = np.argsort(length, kind="stable")
    order = order[length[order] > 0]
    a = int(order[0])                                   # shortest non-empty list: this tile is emptied
    last_lo = (n - 1) // CHUNK * CHUNK
    b = next(int(t) for t in order[1:] if (pl[r[t, 0]:r[t, 1]] >= last_lo).any())
    ids_a = pl[r[a, 0]:r[a, 1]]
    ids_b = pl[r[b, 0]:r[b, 1]]
    gone = np.unique(np.concatenate([ids_a, ids_b[ids_b < last_lo], np.arange(5, n, 17)]))
    keep_b = np.setdiff1d(ids_b[ids_b >= last_lo], ids_a)
    gone = np.setdiff1d(gone, keep_b)
    _behind_camera(case, torch.from_numpy(gone))
    o, _ = U.run_oracle(case, "f32")
    r = np.asarray(o["ranges"]).astype(np.int64)
    pl = np.asarray(o["point_list"]).astype(np.int64)
    rad = np.asarray(o["radii"])
    assert (rad[gone] == 0).all() and (rad > 0).sum() > n // 2
    assert r[a, 1] == r[a, 0]                                           # an empty tile
    assert r[b, 1] > r[b, 0] and (pl[r[b, 0]:r[b, 1]] >= last_lo).all()   # a tile of the last workgroup alone
    assert _chunk_entries(o, n).size == 3
    _assert_lists(case, o)


def test_equal_depths_under_the_staged_scatter(oracle_built):
    """The constant-depth plane of test_equal_depth_ties_keep_gaussian_index_order: ties are broken by Gaussian id whatever
    order the partition arrives in."""
    case = U.make_case(3_000, 64, 64, 5, deg=0, sigma0=(0.02,))
    axis = case["view"][:3, 2].clone()
    axis = axis / axis.norm()
    m = case["means3D"]
    case["means3D"] = (m - (m @ axis)[:, None] * axis[None, :]).contiguous()
    o, _ = U.run_oracle(case, "f32")
    keys = o["keys_sorted"]
    assert (keys[1:] == keys[:-1]).mean() > 0.01
    h = _run_mode(case, 2)
    np.testing.assert_array_equal(h["point_list"].view(np.uint32), o["point_list"])
    np.testing.assert_array_equal(h["keys_sorted"].view(np.uint64), o["keys_sorted"])


def test_three_views_in_one_node_under_the_staged_scatter(oracle_built):
    """blockIdx.y = view: three views through the multi-view node, radii and images per view against the oracle."""
    from generativedensification_amd import rasterizer as R
    from generativedensification_amd.camera import orbit_cameras

    dev = torch.device("cuda:0")
    case = U.make_case(20_000, 208, 176, 41, deg=3, sigma0=(0.0052, 0.00065))
    sets = [dict(case, view=c.world_view_transform.contiguous(), proj=c.full_proj_transform.contiguous(),
                 campos=c.camera_center.contiguous()) for c in orbit_cameras(3, 176, 208)]
    t = lambda k: case[k].to(dev)
    saved = R.K.SCATTER_MODE
    R.K.SCATTER_MODE = 2
    try:
        colors, radii, depths, alphas = R.render_views_raw(t("means3D"), torch.zeros(case["N"], 4, device=dev), t("shs"),
                                                           t("opacities"), t("scales"), t("rotations"),
                                                           [U.settings_torch(cc, dev) for cc in sets], flags=0)
        torch.cuda.synchronize()
    finally:
        R.K.SCATTER_MODE = saved
    for v, cc in enumerate(sets):
        o, _ = U.run_oracle(cc, "f32")
        assert _chunk_entries(o, case["N"]).size == 20
        np.testing.assert_array_equal(radii[v].cpu().numpy(), o["radii"])
        U.assert_rendered_parity(colors[v].cpu().numpy(), depths[v].cpu().numpy(), alphas[v].cpu().numpy(), o, f"view {v}")


def test_capacity_guard_keeps_the_staged_copy_inside_the_key_buffer(oracle_built):
    """A device-sized binning call (gdr_binning.d_dev) whose buffers were carved for a third of the real duplicate count:
    neither mode may write a word beyond `capacity` entries of the key buffer.  The key buffer is the test's own, with a
    sentinel behind it long enough to take every entry an unguarded store could write; the call answers GDR_OK and leaves the
    real count on the device, above the capacity, which is how the caller learns of the shortfall (direct path: the same)."""
    from generativedensification_amd import _lib as L
    from generativedensification_amd import rasterizer as R

    dev = torch.device("cuda:0")
    lib = L.load()
    case, o = _several()
    N, H, W, tiles = case["N"], case["H"], case["W"], _tiles(case)
    D = int(o["num_rendered"])
    cap = D // 3
    assert cap > 1000
    rs = U.settings_torch(case, dev)
    e = torch.empty(0, device=dev)
    t = lambda k: e if case[k] is None else case[k].to(dev)
    _, radii, _, _, st, keep = R.forward_raw(t("means3D"), t("shs"), t("colors_precomp"), t("opacities"), t("scales"),
                                             t("rotations"), t("cov3D_precomp"), rs)      # K1's outputs: st.geom
    torch.cuda.synchronize()
    assert st.D == D
    s = keep[-1]
    counter = torch.zeros(2, dtype=torch.int32, device=dev)
    SENT = -0x5A5A5A5A5A5A5A5B
    seen = {}
    for mode in (1, 2):
        need = int(lib.gdr_binning_bytes_for(cap, 256, N, tiles))
        ws = torch.zeros(need, dtype=torch.uint8, device=dev)
        ibuf = torch.zeros(int(lib.gdr_image_bytes(H, W)), dtype=torch.uint8, device=dev)
        kbuf = torch.full((cap + D + 4096,), SENT, dtype=torch.int64, device=dev)
        bb, img = L.GdrBinning(), L.GdrImage()
        L.check(lib.gdr_binning_carve_for(ws.data_ptr(), cap, 256, N, tiles, C.byref(bb)), "gdr_binning_carve_for")
        L.check(lib.gdr_image_carve(ibuf.data_ptr(), H, W, C.byref(img)), "gdr_image_carve")
        assert bb.tile_hist and bb.scatter_mode == 0
        counter[0] = D
        bb.keys[0] = kbuf.data_ptr()
        bb.d_dev = counter.data_ptr()
        bb.scatter_mode = mode
        rc = lib.gdr_binning_forward(C.byref(s), N, C.byref(st.geom), C.byref(bb), C.byref(img), cap, radii.data_ptr(),
                                     R._stream())
        torch.cuda.synchronize()
        assert rc == L.GDR_OK, (mode, rc)
        assert bool((kbuf[cap:] == SENT).all()), f"mode {mode}: a store beyond the capacity"
        assert bool((kbuf[:cap] != SENT).any())                   # (the guarded part of the list was written)
        seen[mode] = (rc, int(counter[0]))
        assert seen[mode][1] == D > cap                           # the shortfall, as the caller reads it
    assert seen[1] == seen[2]


def test_surfel_images_equal_under_both_modes(oracle_built):
    """The surfel path shares the binning stage: same images under either mode."""
    from generativedensification_amd import rasterizer as R

    case = U.make_surfel_case(3_000, 80, 112, 19, deg=1, sigma0=(0.01, 0.002))
    outs = {}
    saved = R.K.SCATTER_MODE
    try:
        for mode in (1, 2):
            R.K.SCATTER_MODE = mode
            outs[mode] = U.run_surfel_hip(case)[0]
    finally:
        R.K.SCATTER_MODE = saved
    assert outs[1]["num_rendered"] > CHUNK
    for k in ("color", "allmap", "radii", "ranges", "point_list"):
        np.testing.assert_array_equal(outs[1][k], outs[2][k], err_msg=k)
    o, _ = U.run_surfel_oracle(case, "f32")
    np.testing.assert_array_equal(outs[2]["point_list"].view(np.uint32), o["point_list"])
