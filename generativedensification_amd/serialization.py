"""Point-cloud serialization for the point decoder on the MI355X (csrc/serialize.hip, include/gdr.h gdr_serial_*): what the
reference computes with tensor ops in `Point.serialization` (lightning/point_decoder/utils/structure.py) before any
SerializedAttention block runs, and the pad / unpad / cu_seqlens tables of `SerializedAttention.get_padding_and_inverse`
(lightning/point_decoder/autoencoder.py) that the `flash_attn` package of this repository consumes.

`encode` / `decode` carry the names, argument order and return types of the reference's `serialization.encode` / `decode`;
`serialization` can be bound as `Point.serialization`.  GPU tensors only (no CPU fallback); anything outside the envelope
raises before a kernel is launched: 1 <= depth <= 16, 3 * depth + bit_length(B) <= 63, grid_coord (N, 3) int32 or int64
with any strides, at most 8 orders per call.  Coordinates outside [0, 2^depth) give unspecified codes.

Equal codes are ordered by ascending point index (the reference's torch.argsort leaves their order open).  Nothing here
synchronises with the host except where said: `depth=None` (one read of the coordinate maximum) and a device `offset` given
to `patch_tables` (one read of its B values).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from . import _marshal as M

__all__ = ["encode", "decode", "serialize", "serialization", "patch_tables", "ORDERS", "SORT_TILE"]

ORDERS = tuple(L.GDR_SERIAL_ORDERS)
SORT_TILE = L.GDR_SERIAL_SORT_TILE     # keys per workgroup of the sort


def _order_ids(orders):
    if isinstance(orders, str):
        orders = [orders]
    orders = list(orders)
    if not 1 <= len(orders) <= L.GDR_SERIAL_MAX_ORDERS:
        raise ValueError(f"between 1 and {L.GDR_SERIAL_MAX_ORDERS} orders per call, got {len(orders)}")
    for o in orders:
        if o not in L.GDR_SERIAL_ORDERS:
            raise ValueError(f"unknown order {o!r}: one of {ORDERS}")
    return orders, (C.c_int32 * len(orders))(*(L.GDR_SERIAL_ORDERS[o] for o in orders))


def _check_depth(depth, segments: int):
    if isinstance(depth, bool) or not isinstance(depth, int):
        raise TypeError(f"depth must be an int, got {type(depth).__name__}")
    if not 1 <= depth <= L.GDR_SERIAL_MAX_DEPTH:
        raise ValueError(f"depth {depth} is outside 1..{L.GDR_SERIAL_MAX_DEPTH}")
    if depth * 3 + int(segments).bit_length() > 63:
        raise ValueError(f"depth {depth} with {segments} segments does not fit a 63-bit code")


def _check_grid(grid_coord):
    if not isinstance(grid_coord, torch.Tensor) or grid_coord.dim() != 2 or grid_coord.shape[1] != 3:
        raise ValueError(f"grid_coord must be an (N, 3) tensor, got {tuple(getattr(grid_coord, 'shape', ()))}")
    if grid_coord.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"grid_coord must be int32 or int64, not {grid_coord.dtype}")
    if not grid_coord.is_cuda:
        raise RuntimeError("the HIP serialization runs on ROCm/HIP tensors only (no CPU fallback)")
    if grid_coord.shape[0] > L.GDR_SERIAL_MAX_POINTS:
        raise ValueError(f"more than {L.GDR_SERIAL_MAX_POINTS} points")


def _check_batch(batch, grid_coord):
    if batch is None:
        return None
    if not isinstance(batch, torch.Tensor) or batch.dim() != 1 or batch.shape[0] != grid_coord.shape[0]:
        raise ValueError("batch must be a 1-D tensor with one entry per point")
    if batch.device != grid_coord.device:
        raise RuntimeError("batch must live on grid_coord's device")
    if batch.dtype.is_floating_point or batch.dtype.is_complex or batch.dtype == torch.bool:
        raise TypeError(f"batch must be an integer tensor, not {batch.dtype}")
    return batch.long().contiguous()


def _encode(grid_coord, batch, depth, names, ids):
    """checked arguments -> (k, N) int64"""
    N, k, dev = grid_coord.shape[0], len(names), grid_coord.device
    with torch.cuda.device(dev):
        code = torch.empty(k, N, dtype=torch.int64, device=dev)
        L.check(L.load().gdr_serial_encode(grid_coord.data_ptr(), M.strides(grid_coord),
                                           int(grid_coord.dtype == torch.int64), None if batch is None else batch.data_ptr(),
                                           N, depth, k, ids, code.data_ptr(), M.stream()), "gdr_serial_encode")
    return code


@torch.no_grad()
def encode(grid_coord, batch=None, depth=16, order="z"):
    """The reference's serialization.encode: (N, 3) grid cells (+ batch) -> N int64 codes under one order."""
    if not isinstance(order, str):
        raise ValueError(f"order must be one of {ORDERS}")
    names, ids = _order_ids(order)
    _check_grid(grid_coord)
    batch = _check_batch(batch, grid_coord)
    _check_depth(depth, 1)
    return _encode(grid_coord, batch, depth, names, ids)[0]


@torch.no_grad()
def decode(code, depth=16, order="z"):
    """The reference's serialization.decode for "z" and "hilbert": N codes -> (grid_coord (N, 3) int64, batch (N) int64)."""
    if order not in ("z", "hilbert"):
        raise ValueError(f"decode takes the orders 'z' and 'hilbert', not {order!r}")
    if not isinstance(code, torch.Tensor) or code.dim() != 1 or code.dtype != torch.int64:
        raise ValueError("code must be a 1-D int64 tensor")
    if not code.is_cuda:
        raise RuntimeError("the HIP serialization runs on ROCm/HIP tensors only (no CPU fallback)")
    _check_depth(depth, 1)
    code = code.contiguous()
    N, dev = code.shape[0], code.device
    with torch.cuda.device(dev):
        grid = torch.empty(N, 3, dtype=torch.int64, device=dev)
        batch = torch.empty(N, dtype=torch.int64, device=dev)
        L.check(L.load().gdr_serial_decode(code.data_ptr(), N, depth, L.GDR_SERIAL_ORDERS[order], grid.data_ptr(),
                                           batch.data_ptr(), M.stream()), "gdr_serial_decode")
    return grid, batch


@torch.no_grad()
def serialize(grid_coord, batch, depth, orders, num_segments=None):
    """Codes under every order of `orders` (row r = orders[r]; names may repeat), their stable argsort and its inverse:
    (code, order, inverse), each (k, N) int64 with inverse[r, order[r, j]] = j.  num_segments: B, an upper bound of
    batch.max() + 1 that the caller knows on the host (len(point.offset)); it limits the sort to the 3 * depth +
    bit_length(B - 1) bits that can differ.  Without it (and with a batch) every bit above the cell code is sorted."""
    names, ids = _order_ids(orders)
    _check_grid(grid_coord)
    batch = _check_batch(batch, grid_coord)
    if num_segments is None:
        _check_depth(depth, 1)
        bits = 3 * depth if batch is None else 63
    else:
        if int(num_segments) < 1:
            raise ValueError("num_segments must be >= 1")
        _check_depth(depth, int(num_segments))
        bits = 3 * depth + (int(num_segments) - 1).bit_length()
    N, k, dev = grid_coord.shape[0], len(names), grid_coord.device
    lib = L.load()
    code = _encode(grid_coord, batch, depth, names, ids)
    with torch.cuda.device(dev):
        order = torch.empty(k, N, dtype=torch.int64, device=dev)
        inverse = torch.empty(k, N, dtype=torch.int64, device=dev)
        nbytes = lib.gdr_serial_sort_bytes(k, N)
        if nbytes == 0:
            L.check(-1, "gdr_serial_sort_bytes")
        ws, base, usable = M.workspace(nbytes, dev)
        L.check(lib.gdr_serial_sort(code.data_ptr(), k, N, bits, base, usable, order.data_ptr(), inverse.data_ptr(), M.stream()),
                "gdr_serial_sort")
    return code, order, inverse


@torch.no_grad()
def serialization(point, order="z", depth=None, shuffle_orders=False):
    """The reference's Point.serialization on any mutable mapping (bind it with `Point.serialization = serialization`): needs
    "batch" and "grid_coord" or "coord" + "grid_size"; fills "grid_coord" if absent, "serialized_depth" (int),
    "serialized_code", "serialized_order", "serialized_inverse" ((k, N) int64).  "offset", which Point always carries, tells
    the number of segments.  depth=None reads the coordinate maximum back once; with depth given nothing synchronises."""
    if "batch" not in point:
        raise KeyError("serialization needs point['batch']")
    if "grid_coord" not in point:
        if "grid_size" not in point or "coord" not in point:
            raise KeyError("serialization needs point['grid_coord'] or point['coord'] and point['grid_size']")
        coord = point["coord"]
        # the reference's own expression, by torch on the caller's device: a kernel that divided differently would move
        # points across cell borders
        point["grid_coord"] = torch.div(coord - coord.min(0)[0], point["grid_size"], rounding_mode="trunc").int()
    grid_coord = point["grid_coord"]
    _check_grid(grid_coord)
    if depth is None:
        depth = int(grid_coord.max()).bit_length()
        if depth == 0:
            raise ValueError("every grid coordinate is 0: the serialization depth would be 0")
    segments = len(point["offset"]) if "offset" in point else None
    names = [order] if isinstance(order, str) else list(order)
    if shuffle_orders:
        # the reference permutes the finished rows by one torch.randperm(k) of the global CPU generator; the same draw,
        # applied to the row order of the encode (row j = order perm[j]) instead of three gathers
        perm = torch.randperm(len(names))
        names = [names[i] for i in perm.tolist()]
    code, order_, inverse = serialize(grid_coord, point["batch"], depth, names, num_segments=segments)
    point["serialized_depth"] = depth
    point["serialized_code"] = code
    point["serialized_order"] = order_
    point["serialized_inverse"] = inverse


@torch.no_grad()
def patch_tables(offset, patch_size, device=None):
    """pad, unpad (int64) and cu_seqlens (int32) of SerializedAttention.get_padding_and_inverse in one launch.  offset: the B
    segment ends (the reference's point.offset) as a device tensor — one read-back of its B values sizes the outputs — or as a
    sequence of ints (no read-back; `device` then says where the tables go, default: the current device).  A segment longer
    than patch_size is padded to a multiple of it with the points one patch before its end."""
    P = int(patch_size)
    if P < 1:
        raise ValueError("patch_size must be >= 1")
    if isinstance(offset, torch.Tensor):
        if not offset.is_cuda:
            raise RuntimeError("the HIP serialization runs on ROCm/HIP tensors only (no CPU fallback)")
        if offset.dim() != 1 or offset.dtype.is_floating_point:
            raise ValueError("offset must be a 1-D integer tensor of segment ends")
        dev = offset.device
        ends = [int(v) for v in offset.tolist()]
        off_dev = offset.long().contiguous()
    else:
        ends = [int(v) for v in offset]
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("the HIP serialization runs on ROCm/HIP tensors only (no CPU fallback)")
        off_dev = None
    B = len(ends)
    if not 1 <= B <= L.GDR_SERIAL_MAX_SEGMENTS:
        raise ValueError(f"between 1 and {L.GDR_SERIAL_MAX_SEGMENTS} segments, got {B}")
    total = n_seq = prev = 0
    for e in ends:
        n = e - prev
        if n < 0:
            raise ValueError("offset must be non-decreasing and start at or above 0")
        total += n if n <= P else -(-n // P) * P
        n_seq += 0 if n == 0 else (1 if n <= P else -(-n // P))
        prev = e
    if total >= 1 << 31:
        raise ValueError("the padded length does not fit cu_seqlens (int32)")
    if off_dev is None:
        off_dev = torch.tensor(ends, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        pad = torch.empty(total, dtype=torch.int64, device=dev)
        unpad = torch.empty(prev, dtype=torch.int64, device=dev)
        cu = torch.empty(n_seq + 1, dtype=torch.int32, device=dev)
        L.check(L.load().gdr_serial_patch_tables(off_dev.data_ptr(), B, P, prev, total, n_seq, pad.data_ptr(), unpad.data_ptr(),
                                                 cu.data_ptr(), M.stream()), "gdr_serial_patch_tables")
    return pad, unpad, cu
