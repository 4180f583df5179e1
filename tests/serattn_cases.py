"""Inputs for the tests of the gather form of the attention (generativedensification_amd/serattn.py): the five smallest
batches that reach every path of the kernels, as the reference's SerializedAttention would see them.

  - each segment of the batch is serialized in an order of its own (a seeded permutation INSIDE the segment), and the padded
    slots come from tests/attn_ref.py padded_patches: a segment longer than a patch repeats the tail of its last full
    sequence in the next one;
  - Q, K and V come from different distributions, every head has its own magnitude, rows and channels of qkv and of the
    upstream gradient are scaled (as attn_cases.make does it), so a swapped table, a transposition or a missed copy shows;
  - N <= 1500.

name -> (patch, offsets, H, D, softmax_scale):
  borrow47_h3_d8  segments of 49 (47 copies), 96 (none), 30 (one short sequence), 0 (empty), 97 (47 copies behind two full
                  patches); H = 3 is no multiple of the 4 heads of a workgroup
  cfg_stage0      the config's head layout (20 x 8); 20 and 46 copies
  rp128_d16       128 rows per head, 50 copies, a non-default scale
  rp256_d64       256 rows per head, 16-bit LDS rows, 199 copies, then a segment with none
  exact_d32       no copies at all
"""
import functools

import torch

import attn_ref as R

SHAPES = {
    "borrow47_h3_d8": (48, (49, 145, 175, 175, 272), 3, 8, None),
    "cfg_stage0": (48, (700, 730, 1500), 20, 8, 8 ** -0.5),
    "rp128_d16": (100, (250,), 2, 16, 0.2),
    "rp256_d64": (200, (201, 601), 2, 64, None),
    "exact_d32": (48, (96, 144), 5, 32, None),
}
COPIES = {"borrow47_h3_d8": 94, "cfg_stage0": 66, "rp128_d16": 50, "rp256_d64": 199, "exact_d32": 0}
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
CASES = [(name, dt) for name in SHAPES for dt in DTYPES]


def tables(offsets, patch, seed):
    """-> order (Tp,), inverse (N,) int64, cu (batch + 1,) int32, the serialization order (N,): CPU tensors"""
    pad, unpad, cu = R.padded_patches(offsets, patch)
    g = torch.Generator().manual_seed(seed)
    ser, prev = [], 0
    for end in offsets:
        ser.append(prev + torch.randperm(end - prev, generator=g))
        prev = end
    ser = torch.cat(ser)
    return ser[pad], unpad[torch.argsort(ser)], cu, ser


@functools.lru_cache(maxsize=None)
def _make(name, dt):
    patch, offsets, H, D, scale = SHAPES[name]
    dtype = DTYPES[dt]
    N, C = offsets[-1], H * D
    seed = 2000 + sum(map(ord, name))
    order, inverse, cu, _ = tables(offsets, patch, seed)
    assert order.numel() - N == COPIES[name] and bool((order[inverse] == torch.arange(N)).all())
    g = torch.Generator().manual_seed(seed + 1)
    mag = 0.6 + 0.45 * torch.arange(H, dtype=torch.float32)
    mag = (mag / mag.max() * min(float(mag.max()), 3.0)).view(1, H, 1)
    row = (0.5 + torch.arange(N, dtype=torch.float32) % 5 / 4).view(N, 1, 1)
    q = torch.randn(N, H, D, generator=g) * mag * row
    k = (torch.rand(N, H, D, generator=g) * 2 - 0.7) * mag.flip(1)
    v = -torch.log(torch.rand(N, H, D, generator=g).clamp_min(1e-3)) * (0.3 + 0.2 * torch.arange(H).view(1, H, 1))
    chan = 1.0 + 0.5 * torch.cos(torch.arange(C, dtype=torch.float32) * 1.3)
    tok = (0.25 + torch.arange(N, dtype=torch.float32) % 7 / 4).view(N, 1)
    qkv = torch.stack([q, k, v], dim=1).reshape(N, 3 * C).to(dtype)
    dout = (torch.randn(N, C, generator=g) * tok * chan).to(dtype)
    has_copy = torch.zeros(N, dtype=torch.bool)
    seen = torch.bincount(order, minlength=N)
    has_copy[seen > 1] = True
    assert int(has_copy.sum()) == COPIES[name] and int(seen.max()) <= 2 and int(seen.min()) == 1
    return dict(qkv=qkv, dout=dout, order=order, inverse=inverse, cu=cu.tolist(), cu_t=cu, patch=patch, H=H, D=D, C=C, N=N,
                scale=scale, has_copy=has_copy)


def make(name, dt, device="cpu"):
    """-> dict(qkv (N, 3 C), dout (N, C) in the dtype `dt` names, order, inverse, cu (list), cu_t, patch, H, D, C, N, scale,
    has_copy (N,) bool: the points the padding holds twice), tensors on `device`.  Built once per (name, dt) and copied."""
    case = _make(name, dt)
    return {k: (v.clone().to(device) if isinstance(v, torch.Tensor) else v) for k, v in case.items()}
