"""GPU: the HIP point serialization (csrc/serialize.hip through generativedensification_amd.serialization) against the codes
recorded from the reference (tests/golden/serial_*.npz) and the numpy restatement (tests/serial_ref.py): encode / decode,
the stable sort with its inverse at sizes around the sort's tile, the mapping-level `serialization`, the patch tables, and
one call in the shape of SerializedAttention.forward down to the HIP attention.  Everything is integer: equality is exact."""
import os

import numpy as np
import pytest
import torch

import attn_cases as AC
import attn_ref
import serial_ref as R
from serial_cases import CASES, GOLDEN, PATCH_SIZES, cloud, golden, segment_sizes

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TILE = 1024


def S():
    from generativedensification_amd import serialization

    return serialization


def dev(a, dtype=None):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def check_rows(code, order, inverse):
    """the properties that define (order, inverse) of every row, on host copies"""
    k, n = code.shape
    for r in range(k):
        assert (np.diff(code[r][order[r]]) >= 0).all()
        assert (np.sort(order[r]) == np.arange(n)).all()
        assert (inverse[r][order[r]] == np.arange(n)).all()


@pytest.mark.parametrize("case", CASES)
def test_encode_and_decode_equal_the_reference_codes(case):
    g = golden(case)
    grid, batch, depth = g["grid_coord"], g["batch"], int(g["depth"])
    n = grid.shape[0]
    wide = torch.zeros(n, 7, dtype=torch.int32)
    wide[:, 1::2] = torch.from_numpy(grid)
    wide = wide.to(DEV)
    layouts = {"int32": dev(grid), "int64": dev(grid, torch.int64), "strided": wide[:, 1::2],
               "transposed": dev(grid.T.copy()).T}
    assert not layouts["strided"].is_contiguous() and layouts["transposed"].stride() == (1, n)
    for name, t in layouts.items():
        for order in R.ORDERS:
            code = S().encode(t, dev(batch), depth, order)
            assert code.dtype == torch.int64 and code.shape == (n,)
            assert (code.cpu().numpy() == g["code_" + order.replace("-", "_")]).all(), (name, order)
    nb = S().encode(layouts["int32"], None, depth, "hilbert")                # without batch: the cell bits alone
    assert (nb.cpu().numpy() == g["code_hilbert"] & ((1 << (3 * depth)) - 1)).all()
    for order in ("z", "hilbert"):
        dg, db = S().decode(dev(g["code_" + order]), depth, order)
        assert dg.dtype == db.dtype == torch.int64 and dg.shape == (n, 3) and db.shape == (n,)
        assert (dg.cpu().numpy() == grid).all() and (db.cpu().numpy() == batch).all(), order
    dg, db = S().decode(dev(g["code_hilbert"]), depth, "hilbert")
    assert (dg.cpu().numpy() == g["decode_grid"]).all() and (db.cpu().numpy() == g["decode_batch"]).all()


@pytest.mark.parametrize("case", CASES)
def test_serialize_equals_the_restatement_on_the_goldens(case):
    g = golden(case)
    grid, batch, depth = g["grid_coord"], g["batch"], int(g["depth"])
    segments = int(batch.max()) + 1
    code, order, inverse = (t.cpu().numpy() for t in S().serialize(dev(grid), dev(batch), depth, R.ORDERS, num_segments=segments))
    rc, ro, ri = R.serialize(grid, batch, depth, R.ORDERS)
    for r, name in enumerate(R.ORDERS):
        assert (code[r] == g["code_" + name.replace("-", "_")]).all()
    assert (code == rc).all() and (order == ro).all() and (inverse == ri).all()
    check_rows(code, order, inverse)


# N = 0, one sort tile - 1 / exactly / + 1, three tiles and a bit, and the decoder's first shape (12 000 points at depth 7,
# ~30 points in a cell that another point has too)
@pytest.mark.parametrize("n,depth,segments", [(0, 7, 1), (TILE - 1, 7, 1), (TILE, 5, 1), (TILE + 1, 7, 3), (3 * TILE + 77, 6, 5),
                                              (12_000, 7, 1), (2 * TILE + 5, 16, 6)])
def test_serialize_equals_the_restatement_on_random_clouds(n, depth, segments):
    assert S().SORT_TILE == TILE
    grid, batch = cloud(n, depth, 7000 + n + depth, segments, full=n == 12_000)
    if n == 12_000:      # 12 000 points in 128^3 cells: n^2 / (2 * 2^21) = 34 expected collisions
        cells = {tuple(c) for c in grid.tolist()}
        assert 10 <= n - len(cells) <= 80, n - len(cells)
    code, order, inverse = (t.cpu().numpy() for t in S().serialize(dev(grid), dev(batch), depth, R.ORDERS, num_segments=segments))
    assert code.shape == order.shape == inverse.shape == (4, n) and code.dtype == order.dtype == inverse.dtype == np.int64
    rc, ro, ri = R.serialize(grid, batch, depth, R.ORDERS)
    assert (code == rc).all()
    check_rows(code, order, inverse)
    assert (order == ro).all() and (inverse == ri).all()


def test_many_duplicates_and_an_unknown_segment_count():
    """3000 points in 40 cells (long runs of equal codes across tiles), and the sort over all 63 bits when the caller cannot
    say how many segments there are"""
    grid, batch = cloud(3000, 9, 5, segments=4, cells=40)
    rc, ro, ri = R.serialize(grid, batch, 9, R.ORDERS)
    for segments in (4, None):
        code, order, inverse = (t.cpu().numpy() for t in S().serialize(dev(grid), dev(batch), 9, R.ORDERS, num_segments=segments))
        assert (code == rc).all() and (order == ro).all() and (inverse == ri).all(), segments


def test_points_of_one_cell_keep_their_order():
    grid = np.tile(np.array([[5, 2, 1]], np.int32), (300, 1))
    code, order, inverse = S().serialize(dev(grid), None, 4, R.ORDERS)
    for r in range(4):
        assert (order[r].cpu().numpy() == np.arange(300)).all() and (inverse[r].cpu().numpy() == np.arange(300)).all()
        assert len(set(code[r].tolist())) == 1


def test_row_lists_with_repeats_and_fewer_than_four_rows():
    grid, batch = cloud(1500, 8, 11, segments=2)
    for orders in (["hilbert"], ["z-trans", "z-trans", "hilbert"], ["hilbert-trans", "z", "hilbert-trans", "z", "hilbert", "z-trans"]):
        code, order, inverse = (t.cpu().numpy() for t in S().serialize(dev(grid), dev(batch), 8, orders, num_segments=2))
        rc, ro, ri = R.serialize(grid, batch, 8, orders)
        assert code.shape == (len(orders), 1500)
        assert (code == rc).all() and (order == ro).all() and (inverse == ri).all(), orders


def _point(n=2500, seed=3):
    g = torch.Generator().manual_seed(seed)
    coord = (torch.rand(n, 3, generator=g) * torch.tensor([6.0, 3.0, 1.5]) - 1.0).to(DEV)
    sizes = [n // 3, 0, n - n // 3]
    offset = torch.tensor(sizes).cumsum(0).to(DEV)
    batch = torch.repeat_interleave(torch.arange(3), torch.tensor(sizes)).to(DEV)
    return {"coord": coord, "grid_size": 0.05, "batch": batch, "offset": offset}


def _expect(point, orders, depth):
    grid = point["grid_coord"].cpu().numpy()          # the cells torch computed on the device
    return R.serialize(grid, point["batch"].cpu().numpy(), depth, orders)


def test_serialization_fills_the_mapping_like_the_reference():
    point = _point()
    S().serialization(point, order=list(R.ORDERS))                         # depth=None: measured from the coordinates
    want_grid = torch.div(point["coord"] - point["coord"].min(0)[0], 0.05, rounding_mode="trunc").int()
    assert point["grid_coord"].dtype == torch.int32 and torch.equal(point["grid_coord"], want_grid)
    depth = int(want_grid.max()).bit_length()
    assert type(point["serialized_depth"]) is int and point["serialized_depth"] == depth == 7
    rc, ro, ri = _expect(point, R.ORDERS, depth)
    for key, want in (("serialized_code", rc), ("serialized_order", ro), ("serialized_inverse", ri)):
        assert point[key].dtype == torch.int64 and point[key].device == DEV and (point[key].cpu().numpy() == want).all(), key
    # a grid_coord that is already there is used as it is; a single order name gives one row
    given = {"grid_coord": point["grid_coord"].long() // 2, "batch": point["batch"], "offset": point["offset"]}
    S().serialization(given, order="hilbert", depth=9)
    rc, ro, ri = _expect(given, ["hilbert"], 9)
    assert given["serialized_depth"] == 9 and set(given) == {"grid_coord", "batch", "offset", "serialized_depth",
                                                             "serialized_code", "serialized_order", "serialized_inverse"}
    assert (given["serialized_code"].cpu().numpy() == rc).all() and (given["serialized_order"].cpu().numpy() == ro).all()
    with pytest.raises(ValueError):
        S().serialization({"grid_coord": torch.zeros(5, 3, dtype=torch.int32, device=DEV), "batch": torch.zeros(5, dtype=torch.long, device=DEV)})


@pytest.mark.parametrize("seed", [0, 1, 12345])
def test_shuffled_rows_follow_the_global_generator(seed):
    torch.manual_seed(seed)
    perm = torch.randperm(4).tolist()
    after = torch.rand(1)
    point = _point(700)
    torch.manual_seed(seed)
    S().serialization(point, order=list(R.ORDERS), depth=8, shuffle_orders=True)
    assert torch.equal(torch.rand(1), after)                               # exactly one draw was taken
    names = [R.ORDERS[i] for i in perm]
    rc, ro, ri = _expect(point, names, 8)
    assert (point["serialized_code"].cpu().numpy() == rc).all() and (point["serialized_order"].cpu().numpy() == ro).all()
    assert (point["serialized_inverse"].cpu().numpy() == ri).all()


def test_a_given_depth_never_synchronises_with_the_host():
    probe = torch.ones(1, device=DEV)
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            detects = False
        except RuntimeError:
            detects = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not detects:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not make .item() raise on this build")
    point = _point(1300)
    S().serialization(dict(point), order=list(R.ORDERS), depth=8)          # warm: library load, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        S().serialization(point, order=list(R.ORDERS), depth=8)
        code = S().encode(point["grid_coord"], point["batch"], 8, "hilbert")
        S().decode(code, 8, "hilbert")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    rc, ro, ri = _expect(point, R.ORDERS, 8)
    assert (point["serialized_order"].cpu().numpy() == ro).all() and (code.cpu().numpy() == rc[2]).all()


@pytest.mark.parametrize("P", PATCH_SIZES)
def test_patch_tables_equal_the_restatement_and_the_reference(P):
    sizes = segment_sizes(P)
    offset = np.cumsum(sizes)
    want = R.patch_tables(offset, P)
    ref = np.load(os.path.join(GOLDEN, "serial_patch.npz"))
    for given in (dev(offset), [int(v) for v in offset], dev(offset, torch.int32)):
        got = S().patch_tables(given, P)
        assert got[0].dtype == got[1].dtype == torch.int64 and got[2].dtype == torch.int32
        for mine, w, key in zip(got, want, ("pad", "unpad", "cu_seqlens")):
            assert mine.device == DEV and mine.shape == w.shape and (mine.cpu().numpy() == w).all(), key
            assert (mine.cpu().numpy() == ref[f"{key}_{P}"]).all(), key


def test_patch_tables_of_the_decoder_sizes_and_of_empty_input():
    for sizes, P in (([12_000], 48), ([12_000, 24_001, 0, 5], 48), ([0], 48), ([0, 0], 4), ([3] * 300, 2)):
        offset = np.cumsum(sizes)
        got = S().patch_tables([int(v) for v in offset], P)
        for mine, w in zip(got, R.patch_tables(offset, P)):
            assert mine.shape == w.shape and (mine.cpu().numpy() == w).all(), (sizes[:4], P)


def test_serialized_attention_call_end_to_end():
    """SerializedAttention.forward's indexing on our tables, down to the HIP attention: qkv[order[r][pad]] through
    flash_attn_varlen_qkvpacked_func on cu_seqlens, back through unpad[inverse[r]] — against attention per patch by plain
    torch on the same gathered rows, to the bar of tests/attn_cases.py (err <= 2 err_torch + ulp against f64)."""
    from flash_attn import flash_attn_varlen_qkvpacked_func

    H, D, P, dtype = 4, 8, 48, torch.float16
    sizes = [500, 30, 0, 131]
    n = sum(sizes)
    grid, _ = cloud(n, 7, 99)
    batch = np.repeat(np.arange(len(sizes)), sizes).astype(np.int64)
    offset = np.cumsum(sizes)
    point = {"grid_coord": dev(grid), "batch": dev(batch), "offset": dev(offset)}
    S().serialization(point, order=list(R.ORDERS), depth=7)
    pad, unpad, cu_seqlens = S().patch_tables(point["offset"], P)
    g = torch.Generator().manual_seed(5)
    feat = (torch.randn(n, 3, H, D, generator=g) * (0.5 + torch.arange(H).view(1, 1, H, 1))).to(dtype).to(DEV)
    rpad, runpad, rcu = R.patch_tables(offset, P)
    _, ro, ri = R.serialize(grid, batch, 7, R.ORDERS)
    for r in (0, 3):
        order = point["serialized_order"][r][pad]
        inverse = unpad[point["serialized_inverse"][r]]
        assert (order.cpu().numpy() == ro[r][rpad]).all() and (inverse.cpu().numpy() == runpad[ri[r]]).all()
        assert torch.equal(order[inverse], torch.arange(n, device=DEV))
        qkv = feat[order]
        out = flash_attn_varlen_qkvpacked_func(qkv, cu_seqlens, max_seqlen=P, dropout_p=0, softmax_scale=D ** -0.5)
        got = out[inverse]
        cu = [int(v) for v in rcu]
        truth, _ = attn_ref.attention(qkv.cpu().double(), cu, D ** -0.5)
        pt, _ = AC.torch_composition(qkv, cu, D ** -0.5)
        err = float((out.cpu().double() - truth).abs().max())
        err_pt = float((pt.cpu().double() - truth).abs().max())
        limit = AC.bar(err_pt, dtype, truth)
        print(f"row {r}: err_hip {err:.3e} err_pt {err_pt:.3e} bar {limit:.3e}")
        assert err <= limit
        assert torch.equal(got, out[dev(runpad[ri[r]])]) and got.shape == (n, H, D)
        # every point attends inside its own segment: the patch of point i holds only points of batch[i]
        seq_of_slot = np.repeat(np.arange(len(cu) - 1), np.diff(cu))
        slot = inverse.cpu().numpy()
        for s in range(len(cu) - 1):
            members = order.cpu().numpy()[cu[s]:cu[s + 1]]
            assert len(set(batch[members].tolist())) == 1
        assert (batch[order.cpu().numpy()[slot]] == batch).all() and seq_of_slot.shape[0] == order.shape[0]


def test_envelope_violations_raise_before_any_launch():
    grid = torch.zeros(10, 3, dtype=torch.int32, device=DEV)
    batch = torch.zeros(10, dtype=torch.long, device=DEV)
    for depth in (0, 17):
        with pytest.raises(ValueError, match="depth"):
            S().encode(grid, batch, depth, "z")
        with pytest.raises(ValueError, match="depth"):
            S().serialize(grid, batch, depth, R.ORDERS)
        with pytest.raises(ValueError, match="depth"):
            S().decode(batch, depth, "z")
        with pytest.raises(ValueError, match="depth"):
            S().serialization({"grid_coord": grid, "batch": batch, "offset": batch[:1] + 10}, order=["z"], depth=depth)
    with pytest.raises(ValueError, match="63-bit"):
        S().serialize(grid, batch, 16, R.ORDERS, num_segments=1 << 15)       # 48 + 16 bits
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S().serialize(grid.cpu(), None, 8, R.ORDERS)
    with pytest.raises(RuntimeError, match="device"):
        S().serialize(grid, batch.cpu(), 8, R.ORDERS)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S().patch_tables(torch.tensor([10]), 48)
    for bad in (torch.zeros(10, 2, dtype=torch.int32, device=DEV), torch.zeros(10, dtype=torch.int32, device=DEV),
                torch.zeros(3, 10, dtype=torch.int32, device=DEV)):
        with pytest.raises(ValueError, match=r"\(N, 3\)"):
            S().serialize(bad, None, 8, R.ORDERS)
    with pytest.raises(TypeError, match="int32 or int64"):
        S().serialize(grid.float(), None, 8, R.ORDERS)
    with pytest.raises(ValueError, match="one entry per point"):
        S().serialize(grid, batch[:5], 8, R.ORDERS)
    with pytest.raises(ValueError, match="unknown order"):
        S().serialize(grid, batch, 8, ["z", "peano"])
    with pytest.raises(ValueError, match="unknown order"):
        S().encode(grid, batch, 8, "hilbert_trans")
    with pytest.raises(ValueError, match="orders per call"):
        S().serialize(grid, batch, 8, ["z"] * 9)
    with pytest.raises(ValueError, match="patch_size"):
        S().patch_tables([10], 0)
    with pytest.raises(ValueError, match="non-decreasing"):
        S().patch_tables([10, 5], 4)
