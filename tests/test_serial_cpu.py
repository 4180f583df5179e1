"""CPU: the numpy restatement of the point serialization (tests/serial_ref.py) against the codes recorded from the
reference's serialization module (tests/golden/serial_*.npz, tests/golden/make_golden_serial.py), its decode round trips,
the defining properties of the patch tables (and the tables recorded from the reference's get_padding_and_inverse), and
the C ABI of csrc/serialize.hip as far as it goes without a device."""
import ctypes as C
import os

import numpy as np
import pytest

import serial_ref as R
from serial_cases import CASES, GOLDEN, PATCH_SIZES, golden, segment_sizes


def test_the_golden_set_is_the_one_the_cases_were_chosen_for():
    assert CASES == sorted(["n1", "n2_same_cell", "n63", "n64", "n65", "d1", "d2", "d8", "d9", "d16", "b3_d7", "b3_d16"])
    for case in CASES:
        g = golden(case)
        grid, depth = g["grid_coord"], int(g["depth"])
        assert grid.dtype == np.int32 and grid.min() >= 0 and grid.max() < 1 << depth
        assert os.path.getsize(os.path.join(GOLDEN, f"serial_{case}.npz")) < 100_000
        if depth >= 2 and grid.shape[0] > 2:      # ranges differ per axis: a -trans row cannot equal its plain row
            assert grid[:, 0].max() > grid[:, 1].max() > grid[:, 2].max()
            assert (g["code_z"] != g["code_z_trans"]).any() and (g["code_hilbert"] != g["code_hilbert_trans"]).any()
    g = golden("n2_same_cell")
    assert (g["grid_coord"][0] == g["grid_coord"][1]).all()
    for case in ("b3_d7", "b3_d16"):
        assert sorted(set(golden(case)["batch"].tolist())) == [0, 2]           # three segments, the middle one empty
    assert int(golden("b3_d16")["code_z"].max()).bit_length() == 50           # batch 2 above 48 cell bits
    assert golden("n1")["code_hilbert"].shape == (1,)


@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_the_reference_codes_bit_for_bit(case):
    g = golden(case)
    grid, batch, depth = g["grid_coord"], g["batch"], int(g["depth"])
    for order in R.ORDERS:
        mine = R.encode(grid, batch, depth, order)
        want = g["code_" + order.replace("-", "_")]
        assert mine.dtype == np.int64 and mine.shape == want.shape and (mine == want).all(), order
    dg, db = R.decode(g["code_hilbert"], depth, "hilbert")
    assert (dg == g["decode_grid"]).all() and (db == g["decode_batch"]).all()
    assert (dg == grid).all() and (db == batch).all()
    zg, zb = R.decode(g["code_z"], depth, "z")                                 # (the reference's z decode raises: round trip)
    assert (zg == grid).all() and (zb == batch).all()


@pytest.mark.parametrize("depth", range(1, 17))
def test_decode_inverts_encode_for_both_curves(depth):
    rng = np.random.default_rng(depth)
    n = 200
    grid = np.stack([rng.integers(0, max(1, (1 << depth) >> s), n) for s in (0, 1, 2)], axis=1)
    grid[0] = (1 << depth) - 1
    batch = rng.integers(0, 5, n)
    for order in ("z", "hilbert"):
        code = R.encode(grid, batch, depth, order)
        assert code.min() >= 0 and int(code.max()).bit_length() <= 3 * depth + 3
        dg, db = R.decode(code, depth, order)
        assert (dg == grid).all() and (db == batch).all(), order
    # the curve property that makes it a Hilbert curve: consecutive indices are neighbouring cells
    if depth <= 3:
        cells, _ = R.decode(np.arange(1 << (3 * depth)), depth, "hilbert")
        assert (np.abs(np.diff(cells, axis=0)).sum(1) == 1).all()
        assert len({tuple(c) for c in cells.tolist()}) == 1 << (3 * depth)


def test_stable_order_and_inverse_of_the_restatement():
    g = golden("b3_d7")
    grid = np.concatenate([g["grid_coord"], g["grid_coord"][:20]])            # 20 duplicate cells
    batch = np.concatenate([g["batch"], g["batch"][:20]])
    code, order, inverse = R.serialize(grid, batch, 7, R.ORDERS)
    n = grid.shape[0]
    for r in range(4):
        s = code[r][order[r]]
        assert (np.diff(s) >= 0).all() and sorted(order[r].tolist()) == list(range(n))
        assert (inverse[r][order[r]] == np.arange(n)).all()
        ties = np.diff(s) == 0
        assert ties.sum() >= 20 and (np.diff(order[r])[ties] > 0).all()


@pytest.mark.parametrize("P", PATCH_SIZES)
def test_patch_tables_satisfy_their_defining_properties(P):
    sizes = segment_sizes(P)
    offset = np.cumsum(sizes)
    pad, unpad, cu = R.patch_tables(offset, P)
    n = int(offset[-1])
    assert pad.dtype == unpad.dtype == np.int64 and cu.dtype == np.int32
    assert unpad.shape == (n,) and (pad[unpad] == np.arange(n)).all()
    starts = np.concatenate([[0], offset])
    seg_of_point = np.repeat(np.arange(len(sizes)), sizes)
    padded = [s if s <= P else -(-s // P) * P for s in sizes]
    seg_of_slot = np.repeat(np.arange(len(sizes)), padded)
    assert pad.shape == seg_of_slot.shape and (seg_of_point[pad] == seg_of_slot).all()       # every slot: a point of its own segment
    assert ((pad >= starts[seg_of_slot]) & (pad < starts[seg_of_slot + 1])).all()
    assert cu[0] == 0 and cu[-1] == pad.shape[0] and (np.diff(cu) > 0).all() and (np.diff(cu) <= P).all()
    for a, b in zip(cu[:-1], cu[1:]):                                                         # a sequence never spans two segments
        assert len(set(seg_of_slot[a:b].tolist())) == 1


@pytest.mark.parametrize("P", PATCH_SIZES)
def test_patch_tables_equal_the_reference_tables(P):
    """tests/golden/serial_patch.npz: get_padding_and_inverse of the reference's autoencoder.py, which loads with stand-in
    modules for the packages that method does not use"""
    g = np.load(os.path.join(GOLDEN, "serial_patch.npz"))
    assert g[f"offset_{P}"].tolist() == np.cumsum(segment_sizes(P)).tolist()
    pad, unpad, cu = R.patch_tables(g[f"offset_{P}"], P)
    for mine, key in ((pad, "pad"), (unpad, "unpad"), (cu, "cu_seqlens")):
        want = g[f"{key}_{P}"]
        assert mine.dtype == want.dtype and mine.shape == want.shape and (mine == want).all(), key


def test_abi_symbols_and_refusals_without_a_gpu():
    from generativedensification_amd import _lib as L

    lib = L.load()
    for name in ("gdr_serial_encode", "gdr_serial_decode", "gdr_serial_sort_bytes", "gdr_serial_sort", "gdr_serial_patch_tables"):
        assert hasattr(lib, name) and name in L.EXPORTED_SYMBOLS
    assert lib.gdr_abi_version() == 17
    # the workspace query: two key and two index buffers per row plus the (256, tiles) count matrix
    for k, n in ((1, 1), (4, 12_000), (4, 48_000), (8, 1 << 20)):
        tiles = -(-n // L.GDR_SERIAL_SORT_TILE)
        b = lib.gdr_serial_sort_bytes(k, n)
        assert k * n * 24 + k * 256 * tiles * 4 <= b <= k * n * 24 + k * 256 * tiles * 4 + 8 * 256
    assert lib.gdr_serial_sort_bytes(0, 10) == 0 and b"serial_sort_bytes" in lib.gdr_last_error()
    assert lib.gdr_serial_sort_bytes(L.GDR_SERIAL_MAX_ORDERS + 1, 10) == 0
    fake = 0x10000         # never dereferenced: every refusal comes before any device work
    strides = (C.c_int64 * 2)(3, 1)
    orders = (C.c_int32 * 2)(0, 2)
    for depth in (0, 17):
        assert lib.gdr_serial_encode(fake, strides, 0, None, 10, depth, 2, orders, fake, None) == -1
        assert b"depth" in lib.gdr_last_error()
        assert lib.gdr_serial_decode(fake, 10, depth, 0, fake, fake, None) == -1
    assert lib.gdr_serial_encode(fake, strides, 0, None, 10, 8, 2, (C.c_int32 * 2)(0, 4), fake, None) == -1
    assert b"unknown order" in lib.gdr_last_error()
    assert lib.gdr_serial_encode(fake, strides, 0, None, -1, 8, 2, orders, fake, None) == -1
    assert lib.gdr_serial_encode(fake, strides, 0, None, 10, 8, 0, orders, fake, None) == -1
    assert lib.gdr_serial_decode(fake, 10, 8, 1, fake, fake, None) == -1                       # z-trans has no decode
    assert lib.gdr_serial_sort(fake, 4, 10, 0, fake, 1 << 20, fake, fake, None) == -1
    assert lib.gdr_serial_sort(fake, 4, 10, 64, fake, 1 << 20, fake, fake, None) == -1
    assert lib.gdr_serial_sort(fake, 4, 10, 21, fake, 16, fake, fake, None) == L.GDR_ERR_WORKSPACE
    assert lib.gdr_serial_patch_tables(fake, 0, 48, 0, 0, 0, fake, fake, fake, None) == -1
    assert lib.gdr_serial_patch_tables(fake, L.GDR_SERIAL_MAX_SEGMENTS + 1, 48, 0, 0, 0, fake, fake, fake, None) == -1
    assert lib.gdr_serial_patch_tables(fake, 3, 0, 10, 10, 1, fake, fake, fake, None) == -1
    # empty inputs are answered without a launch
    assert lib.gdr_serial_encode(None, strides, 0, None, 0, 8, 2, orders, None, None) == 0
    assert lib.gdr_serial_sort(None, 2, 0, 24, None, 0, None, None, None) == 0


def test_python_surface_refuses_before_any_launch():
    import torch
    from generativedensification_amd import serialization as S

    grid = torch.zeros(4, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.encode(grid, None, 8, "z")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.serialize(grid, None, 8, ["z", "hilbert"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.decode(torch.zeros(4, dtype=torch.int64), 8, "z")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.patch_tables(torch.tensor([3, 9]), 4)
    with pytest.raises(ValueError, match="unknown order"):
        S.serialize(grid, None, 8, ["z", "morton"])
    with pytest.raises(ValueError, match="orders per call"):
        S.serialize(grid, None, 8, [])
    with pytest.raises(ValueError, match=r"\(N, 3\)"):
        S.encode(torch.zeros(4, 2, dtype=torch.int32), None, 8, "z")
    with pytest.raises(ValueError, match="'z' and 'hilbert'"):
        S.decode(torch.zeros(4, dtype=torch.int64), 8, "z-trans")
    assert S.ORDERS == R.ORDERS and S.SORT_TILE == 1024
