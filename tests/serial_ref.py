"""Plain-integer numpy restatement of the point serialization (csrc/serialize.hip, include/gdr.h gdr_serial_*): the four
space-filling-curve codes, their decode, the stable order with its inverse, and the patch index tables.  Written from the
specification, one bit at a time — deliberately not the word-parallel arithmetic of the kernels — and checked bit for bit
against codes recorded from the reference's serialization module (tests/golden/serial_*.npz, tests/test_serial_cpu.py)."""
import numpy as np

ORDERS = ("z", "z-trans", "hilbert", "hilbert-trans")


def _axes(grid_coord, depth, trans):
    g = np.asarray(grid_coord).astype(np.int64).reshape(-1, 3) & ((1 << depth) - 1)
    cols = (1, 0, 2) if trans else (0, 1, 2)
    return [g[:, c].copy() for c in cols]


def _interleave(X, depth):
    """per bit level from the most significant: dimension 0, 1, 2"""
    code = np.zeros(X[0].shape, np.int64)
    for level in range(depth - 1, -1, -1):
        for d in range(3):
            code = (code << 1) | ((X[d] >> level) & 1)
    return code


def _deinterleave(code, depth):
    X = [np.zeros(code.shape, np.int64) for _ in range(3)]
    for level in range(depth):
        for d in range(3):
            X[d] |= ((code >> (3 * level + 2 - d)) & 1) << level
    return X


def _walk_step(X, d, level):
    """dimension d at bit `level`: bit set -> invert the lower bits of dimension 0; clear -> exchange with dimension 0 the
    lower bits in which the two differ"""
    low = (1 << level) - 1
    on = ((X[d] >> level) & 1).astype(bool)
    t = np.where(on, 0, (X[0] ^ X[d]) & low)
    X[0] ^= np.where(on, low, 0)
    X[0] ^= t
    X[d] ^= t


def encode(grid_coord, batch=None, depth=16, order="z"):
    assert order in ORDERS and 1 <= depth <= 16
    X = _axes(grid_coord, depth, order.endswith("-trans"))
    if order.startswith("hilbert"):
        for level in range(depth - 1, -1, -1):
            for d in range(3):
                _walk_step(X, d, level)
        gray = _interleave(X, depth)
        code = np.zeros_like(gray)
        run = np.zeros_like(gray)
        for b in range(3 * depth - 1, -1, -1):        # prefix XOR from the most significant bit
            run ^= (gray >> b) & 1
            code |= run << b
    else:
        code = _interleave(X, depth)
    if batch is not None:
        code = (np.asarray(batch).astype(np.int64) << (3 * depth)) | code
    return code


def decode(code, depth=16, order="z"):
    assert order in ("z", "hilbert") and 1 <= depth <= 16
    code = np.asarray(code).astype(np.int64)
    batch = code >> (3 * depth)
    low = code & ((1 << (3 * depth)) - 1)
    if order == "hilbert":
        X = _deinterleave(low ^ (low >> 1), depth)
        for level in range(depth):
            for d in (2, 1, 0):
                _walk_step(X, d, level)
    else:
        X = _deinterleave(low, depth)
    return np.stack(X, axis=-1), batch


def serialize(grid_coord, batch, depth, orders):
    """(code, order, inverse), each (k, N) int64; equal codes keep ascending point index"""
    code = np.stack([encode(grid_coord, batch, depth, o) for o in orders]).reshape(len(orders), -1)
    order = np.argsort(code, axis=1, kind="stable").astype(np.int64)
    inverse = np.empty_like(order)
    n = code.shape[1]
    for r in range(len(orders)):
        inverse[r, order[r]] = np.arange(n)
    return code, order, inverse


def patch_tables(offset, patch_size):
    """offset: the B segment ends (the reference's point.offset) -> pad, unpad (int64), cu_seqlens (int32)"""
    P = int(patch_size)
    off = [0] + [int(v) for v in offset]
    pad, unpad, cu = [], [], []
    poff = 0
    for i in range(len(off) - 1):
        n = off[i + 1] - off[i]
        m = n if n <= P else -(-n // P) * P
        for j in range(n):
            unpad.append(off[i] + j + poff - off[i])
        for l in range(m):
            pad.append(off[i] + (l if l < n else l - P))
        cu.extend(range(poff, poff + m, P))
        poff += m
    cu.append(poff)
    return np.asarray(pad, np.int64), np.asarray(unpad, np.int64), np.asarray(cu, np.int32)
