"""Inputs for the attention tests that break the symmetries of the kernels' index arithmetic, and the bars both the GPU test
(tests/test_gpu_attn.py) and the mutant test (tests/test_attn_cpu.py) apply.

  - Q, K and V come from different distributions (normal, shifted uniform, skewed positive), so a swap of two of them shows;
  - every head has its own magnitude, so a head / token or head / channel transposition shows;
  - the upstream gradient differs per token and per channel;
  - lengths are mixed in one call (48, 48, 1, 7, 33, 0, 64, 256, 5), with a zero-length sequence in the middle;
  - every head dimension runs under every row tile of the kernels (the `t64_`, `t128_` and `t256_` shapes), with sequences that
    fill the tile, miss it by one row, are the smallest it can hold, and sit on and beside a multiple of the 8-key block;
  - the reference's layouts are there: sequences of 48, D = 8 with H = 20 and H = 32;
  - every D of the envelope appears with an H that is a multiple of nothing convenient (3, 5);
  - default and non-default softmax scales;
  - head 0 is "hot": its logits span well over a hundred, so a softmax without max-subtraction overflows in f32 (exp(88.8)),
    and its rows are dominated by a single key;
  - `total` is larger than cu_seqlens[-1] (rows nobody owns);
  - one layout reads qkv as a slice of a wider buffer, at an offset that breaks 16-byte alignment, with a dout whose rows are
    strided too;
  - fp16 and bf16.
"""
import math

import torch

MIXED = (48, 48, 1, 7, 33, 0, 64, 256, 5)
# one tuple per row tile of the kernels (RP = 64, 128 or 256 rows per head, picked from max_seqlen): a sequence that fills the
# tile, one that is one short of it, the smallest the tile can hold, lengths on and just past a multiple of the 8-key block
T64 = (64, 63, 57, 56, 9, 8, 1, 0, 17, 48)
T128 = (65, 127, 128, 0, 96, 1, 121)
T256 = (129, 255, 256, 0, 200)

# name -> (H, D, lengths, softmax_scale, rows beyond cu_seqlens[-1], layout)
SHAPES = {
    "mixed_h3_d8": (3, 8, MIXED, None, 5, "dense"),
    "mixed_h5_d16_scaled": (5, 16, MIXED, 0.2, 3, "sliced"),
    "mixed_h3_d32": (3, 32, MIXED, None, 0, "dense"),
    "mixed_h5_d64_scaled": (5, 64, MIXED, 0.09, 7, "sliced"),
    "ref48_h20_d8": (20, 8, (48,) * 6, 8 ** -0.5, 0, "dense"),        # the call site passes its scale explicitly
    "ref48_h32_d8_sliced": (32, 8, (48,) * 5, None, 2, "sliced"),
    "short_h1_d8": (1, 8, (3, 1, 0, 2), None, 1, "dense"),
    # every head dimension under every row tile; H is a multiple of neither 4 nor 2, the heads a workgroup holds at RP = 64 and
    # 128; each tier has both scales, both layouts and both kinds of tail
    "t64_h3_d8": (3, 8, T64, None, 0, "dense"),
    "t64_h5_d16": (5, 16, T64, 0.2, 3, "sliced"),
    "t64_h3_d32": (3, 32, T64, None, 5, "sliced"),
    "t64_h5_d64": (5, 64, T64, 0.09, 0, "dense"),
    "t128_h3_d8": (3, 8, T128, 0.3, 2, "sliced"),
    "t128_h5_d16": (5, 16, T128, None, 0, "dense"),
    "t128_h3_d32": (3, 32, T128, 0.15, 0, "sliced"),
    "t128_h5_d64": (5, 64, T128, None, 4, "dense"),
    "t256_h3_d8": (3, 8, T256, None, 3, "dense"),
    "t256_h5_d16": (5, 16, T256, 0.2, 0, "sliced"),
    "t256_h3_d32": (3, 32, T256, None, 0, "sliced"),
    "t256_h5_d64": (5, 64, T256, 0.1, 6, "dense"),
}
TIERS = [name for name in SHAPES if name.startswith(("t64_", "t128_", "t256_"))]
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
CASES = [(name, dt) for name in SHAPES for dt in DTYPES]
MANT_BITS = {torch.float16: 10, torch.bfloat16: 7, torch.float32: 23}


def max_seqlen(name):
    return max(SHAPES[name][2])


def row_tile(max_seqlen):
    """RP, the rows per head of a workgroup: the kernels' selection (csrc/attn.hip attn_launch)"""
    return 64 if max_seqlen <= 64 else 128 if max_seqlen <= 128 else 256


def cu_of(lengths):
    cu = [0]
    for n in lengths:
        cu.append(cu[-1] + n)
    return cu


def make(name, dtype, device="cpu"):
    """-> dict(qkv, dout, cu (list), cu_t (int32 tensor), scale, max_seqlen): qkv (total, 3, H, D) and dout (total, H, D)
    in `dtype` on `device`, laid out as the case says."""
    H, D, lengths, scale, extra, layout = SHAPES[name]
    cu = cu_of(lengths)
    total = cu[-1] + extra
    g = torch.Generator().manual_seed(1000 + sum(map(ord, name)))
    mag = 0.6 + 0.45 * torch.arange(H, dtype=torch.float32)        # a magnitude per head
    mag = mag / mag.max() * min(mag.max(), 3.0)
    q = torch.randn(total, H, D, generator=g) * mag.view(1, H, 1)
    k = (torch.rand(total, H, D, generator=g) * 2 - 0.7) * mag.flip(0).view(1, H, 1)
    v = -torch.log(torch.rand(total, H, D, generator=g).clamp_min(1e-3)) * (0.3 + 0.2 * torch.arange(H).view(1, H, 1))
    # head 0 is hot: q and k aligned per channel, key j scaled by r_j ~ N(0, 1) -> logits ~ 50 r_j, beyond +-100 in a sequence
    hot = (50.0 / ((scale or D ** -0.5) * D)) ** 0.5
    sign = torch.where(torch.arange(D) % 3 == 0, -1.0, 1.0)
    q[:, 0] = hot * sign * (1 + 0.3 * torch.randn(total, D, generator=g))
    k[:, 0] = hot * sign * torch.randn(total, 1, generator=g) * (1 + 0.1 * torch.randn(total, D, generator=g))
    for a, b in zip(cu[:-1], cu[1:]):       # ... and its third key towers over the rest: rows dominated by a single key
        if b - a > 2:
            k[a + 2, 0] = hot * sign * 4.5
    tok = 0.25 + torch.arange(total, dtype=torch.float32).view(total, 1, 1) % 7 / 4
    chan = 1.0 + 0.5 * torch.cos(torch.arange(H * D, dtype=torch.float32).view(1, H, D) * 1.3)
    dout = torch.randn(total, H, D, generator=g) * tok * chan
    qkv = torch.stack([q, k, v], dim=1).to(dtype)
    dout = dout.to(dtype)
    if layout == "sliced":       # a slice of wider buffers: rows keep unit stride, nothing else is dense or 16-byte aligned
        wide = torch.zeros(total, 3, H + 1, D + 4, dtype=dtype)
        wide[:, :, 1:, 4:] = qkv
        wide_d = torch.zeros(total, 2 * H, D + 2, dtype=dtype)
        wide_d[:, ::2, 2:] = dout
        wide, wide_d = wide.to(device), wide_d.to(device)
        qkv, dout = wide[:, :, 1:, 4:], wide_d[:, ::2, 2:]
        assert not qkv.is_contiguous() and not dout.is_contiguous()
    else:
        qkv, dout = qkv.to(device), dout.to(device)
    return dict(qkv=qkv, dout=dout, cu=cu, cu_t=torch.tensor(cu, dtype=torch.int32, device=device), scale=scale,
                max_seqlen=max(max(lengths), 1))


def ulp(dtype, magnitude):
    """The spacing of `dtype` at `magnitude` (> 0)."""
    return 2.0 ** (math.floor(math.log2(magnitude)) - MANT_BITS[dtype]) if magnitude > 0 else 0.0


def bar(err_pt, dtype, truth):
    """err <= 2 err_pt + ulp: two correct half-precision implementations round at different points (the factor 2 is
    upstream flash-attention's convention); the ulp floor (the output dtype's spacing at the tensor's largest f64
    magnitude) keeps the bar meaningful where the composition happens to be exact."""
    return 2.0 * err_pt + ulp(dtype, float(truth.abs().max()))


def torch_composition(qkv, cu, scale, dout=None):
    """The arithmetic of the reference's own non-flash branch with upcasting off, in qkv's (half) dtype on qkv's device,
    per sequence: (q * scale) @ k^T, softmax, @ v.  -> out (total, H, D), and dqkv by autograd if dout is given."""
    total, _, H, D = qkv.shape
    scale = D ** -0.5 if scale is None else scale
    leaf = qkv.detach().clone().requires_grad_(dout is not None)
    out = torch.zeros(total, H, D, dtype=qkv.dtype, device=qkv.device)
    pieces = []
    for a, b in zip(cu[:-1], cu[1:]):
        if b <= a:
            continue
        q, k, v = leaf[a:b].permute(1, 2, 0, 3).unbind(0)       # (H, L, D) each
        attn = torch.softmax((q * scale) @ k.transpose(-2, -1), dim=-1)
        pieces.append((a, b, (attn @ v).transpose(0, 1)))
    if pieces:
        out = _assemble(pieces, total, H, D, qkv)
    if dout is None:
        return out.detach(), None
    out.backward(dout)
    return out.detach(), leaf.grad


def _assemble(pieces, total, H, D, like):
    rows, at = [], 0
    for a, b, o in pieces:
        if a > at:
            rows.append(torch.zeros(a - at, H, D, dtype=like.dtype, device=like.device))
        rows.append(o)
        at = b
    if total > at:
        rows.append(torch.zeros(total - at, H, D, dtype=like.dtype, device=like.device))
    return torch.cat(rows, 0)


def f32_lse(qkv, cu, scale):
    """torch's f32 logsumexp of the f32 scores of the half-rounded inputs: (H, total), zero where no sequence owns the row."""
    total, _, H, D = qkv.shape
    scale = D ** -0.5 if scale is None else scale
    lse = torch.zeros(H, total, dtype=torch.float32, device=qkv.device)
    for a, b in zip(cu[:-1], cu[1:]):
        if b <= a:
            continue
        q, k = qkv[a:b, 0].float().transpose(0, 1), qkv[a:b, 1].float().transpose(0, 1)
        lse[:, a:b] = torch.logsumexp((q * scale) @ k.transpose(-2, -1), dim=-1)
    return lse


def bits_differ(what, a, b):
    """0 if a and b are equal bit for bit; else the number of elements that differ, after printing it with the largest
    distance in units of the last place (the bit patterns read as sign-magnitude integers)"""
    if torch.equal(a, b):
        return 0
    ints = []
    for t in (a, b):
        i = t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).to(torch.int64)
        ints.append(torch.where(i < 0, (-32768 if t.element_size() == 2 else -(1 << 31)) - i, i))
    n = int((ints[0] != ints[1]).sum())
    print(f"{what}: {n} of {a.numel()} elements differ, by at most {int((ints[0] - ints[1]).abs().max())} ulp")
    return n
