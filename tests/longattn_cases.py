"""Inputs for the tests of the tiled MFMA attention (generativedensification_amd/vitattn.py, csrc/attn_tiled.hip), with the
symmetry-breaking properties of tests/attn_cases.py `make`, for fixed-length batches (B, L, H, 64):

  - Q, K and V come from different distributions (normal, shifted uniform, skewed positive), so a swap of two of them shows;
  - every head has its own magnitude, so a head / token or head / channel transposition shows;
  - head 0 is "hot": its logits span well over a hundred, so a softmax without max-subtraction overflows in f32, and its third
    key towers over the rest: rows dominated by a single key, which sits in the FIRST key tile, so every later tile rescales
    nothing and a missing rescale of an EARLIER tile (the other heads) shows;
  - the upstream gradient differs per token and per channel;
  - lengths are the smallest at which a boundary of the kernels' tiles (16-row MFMA blocks, 64 swept rows per LDS tile, 128
    stationary rows per workgroup) can go wrong: on it, one short of it and one past it, and the image encoder's own 1025;
  - B in {1, 2, 3}, H in {1, 3, 5}, default and explicit softmax scales, fp16 and bf16;
  - five layouts of the same values (so results can be compared bit for bit): one packed dense tensor, three separate tensors,
    the view of a Linear's (B, L, 3 H D) output, a slice of a wider NaN-filled buffer with gaps between images, tokens and
    heads whose rows are still 16-byte aligned (read in place), and one whose rows are not (the copy path).

The bars are tests/attn_cases.py's (`bar`, `ulp`, `torch_composition`, `f32_lse`) on the batch flattened to (B L, 3, H, D) with
cu = [0, L, 2L, ...]; the truth is tests/attn_ref.py in f64 on the same.  `tiled_model` is a CPU model of a correct tiled kernel
and of two broken ones."""
import functools

import torch

import attn_cases as AC
import attn_ref as R

D = 64
KEY_TILE = 64
LAYOUTS = ("packed", "separate", "linear", "sliced", "misaligned")
DTYPES = AC.DTYPES

# name -> (B, L, H, softmax_scale, layout)
SHAPES = {
    "l1": (2, 1, 3, None, "packed"),
    "l15": (3, 15, 1, 0.2, "separate"),
    "l16": (1, 16, 5, None, "linear"),
    "l17": (2, 17, 3, 0.09, "sliced"),
    "l63": (3, 63, 5, None, "misaligned"),
    "l64": (1, 64, 3, 0.15, "packed"),
    "l65": (2, 65, 5, None, "sliced"),
    "l127": (1, 127, 3, None, "separate"),
    "l128": (2, 128, 1, 0.2, "linear"),
    "l129": (3, 129, 3, None, "sliced"),
    "l193": (1, 193, 5, 0.1, "misaligned"),
    "l255": (2, 255, 3, None, "packed"),
    "l256": (1, 256, 5, 0.11, "sliced"),
    "l257": (2, 257, 3, None, "linear"),
    "vit1025": (1, 1025, 2, None, "linear"),
}
CASES = [(name, dt) for name in SHAPES for dt in DTYPES]


def values(name, dtype):
    """-> (qkv (B, L, 3, H, D), dout (B, L, H, D)) dense CPU tensors of `dtype`: the values of a case, whatever its layout"""
    B, L, H, scale, _ = SHAPES[name]
    g = torch.Generator().manual_seed(7000 + sum(map(ord, name)))
    mag = 0.6 + 0.45 * torch.arange(H, dtype=torch.float32)
    mag = mag / mag.max() * min(mag.max(), 3.0)
    q = torch.randn(B, L, H, D, generator=g) * mag.view(1, 1, H, 1)
    k = (torch.rand(B, L, H, D, generator=g) * 2 - 0.7) * mag.flip(0).view(1, 1, H, 1)
    v = -torch.log(torch.rand(B, L, H, D, generator=g).clamp_min(1e-3)) * (0.3 + 0.2 * torch.arange(H).view(1, 1, H, 1))
    hot = (50.0 / ((scale or D ** -0.5) * D)) ** 0.5
    sign = torch.where(torch.arange(D) % 3 == 0, -1.0, 1.0)
    q[:, :, 0] = hot * sign * (1 + 0.3 * torch.randn(B, L, D, generator=g))
    k[:, :, 0] = hot * sign * torch.randn(B, L, 1, generator=g) * (1 + 0.1 * torch.randn(B, L, D, generator=g))
    if L > 2:
        k[:, 2, 0] = hot * sign * 4.5
    tok = 0.25 + torch.arange(B * L, dtype=torch.float32).view(B, L, 1, 1) % 7 / 4
    chan = 1.0 + 0.5 * torch.cos(torch.arange(H * D, dtype=torch.float32).view(1, 1, H, D) * 1.3)
    dout = torch.randn(B, L, H, D, generator=g) * tok * chan
    return torch.stack([q, k, v], dim=2).to(dtype), dout.to(dtype)


def lay(qkv, dout, layout, device):
    """the values in a layout on `device` -> dict(qkv = the packed (B, L, 3, H, D) tensor or None, q, k, v, dout)"""
    B, L, _, H, _ = qkv.shape
    nan = float("nan")
    if layout == "packed":
        p = qkv.to(device)
    elif layout == "linear":      # what timm's Attention makes of self.qkv(x)
        p = qkv.reshape(B, L, 3 * H * D).to(device).view(B, L, 3, H, D)
    elif layout == "separate":
        q, k, v = (qkv[:, :, i].contiguous().to(device) for i in range(3))
        return dict(qkv=None, q=q, k=k, v=v, dout=dout.to(device))
    elif layout == "sliced":      # rows stay 16-byte aligned; gaps between images, tokens and heads, all NaN
        wide = torch.full((B + 1, L + 2, 3, H + 1, D + 8), nan, dtype=qkv.dtype)
        wide[:B, 1:L + 1, :, 1:, 8:] = qkv
        wide_d = torch.full((B, L + 1, 2 * H, D + 8), nan, dtype=qkv.dtype)
        wide_d[:, :L, ::2, 8:] = dout
        p, dout = wide.to(device)[:B, 1:L + 1, :, 1:, 8:], wide_d.to(device)[:, :L, ::2, 8:]
        assert not p.is_contiguous() and p.stride(4) == 1 and p.data_ptr() % 16 == 0 and p.stride(0) != L * p.stride(1)
        return dict(qkv=p, q=p[:, :, 0], k=p[:, :, 1], v=p[:, :, 2], dout=dout)
    elif layout == "misaligned":      # rows at an 8-byte offset: the copy path
        wide = torch.full((B, L, 3, H + 1, D + 4), nan, dtype=qkv.dtype)
        wide[:, :, :, 1:, 4:] = qkv
        wide_d = torch.full((B, L, H, D + 2), nan, dtype=qkv.dtype)
        wide_d[..., 2:] = dout
        p, dout = wide.to(device)[:, :, :, 1:, 4:], wide_d.to(device)[..., 2:]
        assert p.data_ptr() % 16 or p.stride(3) % 8
        return dict(qkv=p, q=p[:, :, 0], k=p[:, :, 1], v=p[:, :, 2], dout=dout)
    else:
        raise KeyError(layout)
    return dict(qkv=p, q=p[:, :, 0], k=p[:, :, 1], v=p[:, :, 2], dout=dout.to(device))


def make(name, dtype, device="cpu", layout=None):
    """a case in its own layout (or `layout`): lay()'s dict plus scale, B, L, H"""
    B, L, H, scale, own = SHAPES[name]
    qkv, dout = values(name, dtype)
    return dict(lay(qkv, dout, layout or own, device), scale=scale, B=B, L=L, H=H)


def cu_of(B, L):
    return [b * L for b in range(B + 1)]


@functools.lru_cache(maxsize=None)
def truth(name, dt):
    """f64 (out (B, L, H, D), lse (B, H, L), dqkv (B, L, 3, H, D)) of tests/attn_ref.py on the half-rounded values of a case;
    computed once, shared, never written to"""
    B, L, H, scale, _ = SHAPES[name]
    qkv, dout = values(name, DTYPES[dt])
    flat, cu = qkv.double().reshape(B * L, 3, H, D), cu_of(B, L)
    out, lse = R.attention(flat, cu, scale)
    dqkv = R.attention_backward(flat, cu, dout.double().reshape(B * L, H, D), scale)
    return out.reshape(B, L, H, D), lse.reshape(H, B, L).transpose(0, 1).contiguous(), dqkv.reshape(B, L, 3, H, D)


def torch_errors(name, dt, device="cpu"):
    """the errors against truth() of what the bars are built from, on `device`: torch's composition in the case's half dtype
    (out, dq, dk, dv) and torch's f32 log-sum-exp (lse) -> dict of floats"""
    B, L, H, scale, _ = SHAPES[name]
    qkv, dout = values(name, DTYPES[dt])
    flat, cu = qkv.reshape(B * L, 3, H, D).to(device), cu_of(B, L)
    out, dqkv = AC.torch_composition(flat, cu, scale, dout.reshape(B * L, H, D).to(device))
    lse = AC.f32_lse(flat, cu, scale).reshape(H, B, L).transpose(0, 1)
    t_out, t_lse, t_dqkv = truth(name, dt)
    err = lambda got, t: float((got.double().cpu().reshape(t.shape) - t).abs().max())     # noqa: E731
    return dict(out=err(out, t_out), lse=err(lse, t_lse), dq=err(dqkv[:, 0], t_dqkv[:, :, 0]),
                dk=err(dqkv[:, 1], t_dqkv[:, :, 1]), dv=err(dqkv[:, 2], t_dqkv[:, :, 2]))


def judge(name, dt, got, err_pt, show=True):
    """got: dict(out, lse, dq, dk, dv) tensors -> [(what, err, bar)] for every tensor beyond its bar, after printing each pair
    of errors.  The bars: 2 err_pt + one ulp of the output dtype (f32 for lse) at the truth's largest magnitude."""
    t_out, t_lse, t_dqkv = truth(name, dt)
    truths = dict(out=t_out, lse=t_lse, dq=t_dqkv[:, :, 0], dk=t_dqkv[:, :, 1], dv=t_dqkv[:, :, 2])
    beyond = []
    for what, t in truths.items():
        g = got[what].detach().double().cpu()
        err = float((g - t).abs().max()) if bool(torch.isfinite(g).all()) else float("inf")
        limit = AC.bar(err_pt[what], torch.float32 if what == "lse" else DTYPES[dt], t)
        if show:
            print(f"{name} {dt} {what}: err {err:.3e}  torch {err_pt[what]:.3e}  bar {limit:.3e}  ratio {err / limit if limit else float(err > 0):.2f}")
        if not err <= limit:
            beyond.append((what, err, limit))
    return beyond


MODEL_MUTANTS = ("tail_keys_unmasked", "no_rescale")


def tiled_model(name, dt, mut=None):
    """What a correct kernel of csrc/attn_tiled.hip's design gives on the CPU, in f32 on the half-rounded values: online
    softmax over tiles of 64 keys, P rounded to the half dtype per tile relative to the running max and only as the operand of
    P V, the row sum from the unrounded P; backward with P from lse, delta from the result as TWO half words (the rounded one
    and what its rounding dropped: with delta from the rounded word alone this model is 1.6 to 1.9 times BEYOND the dq bar at
    L = 1025, because K has a mean and the error of delta does not average out over the keys), P and dS rounded once as
    operands.  -> dict(out, lse, dq, dk, dv).  `mut`: one mistake of such a kernel:
      tail_keys_unmasked  the rows behind the sequence in the last key tile (zeros in LDS) take part with score 0;
      no_rescale          the output accumulator is not rescaled when the running max moves."""
    B, L, H, scale, _ = SHAPES[name]
    dtype = DTYPES[dt]
    qkv, dout = values(name, dtype)
    scale = D ** -0.5 if scale is None else scale
    q, k, v = (qkv[:, :, i].float().transpose(1, 2) for i in range(3))      # (B, H, L, D)
    g = dout.float().transpose(1, 2)
    m = torch.full((B, H, L), float("-inf"))
    l = torch.zeros(B, H, L)
    o = torch.zeros(B, H, L, D)
    for k0 in range(0, L, KEY_TILE):
        kt, vt = k[:, :, k0:k0 + KEY_TILE], v[:, :, k0:k0 + KEY_TILE]
        if mut == "tail_keys_unmasked" and kt.shape[2] < KEY_TILE:
            pad = torch.zeros(B, H, KEY_TILE - kt.shape[2], D)
            kt, vt = torch.cat([kt, pad], 2), torch.cat([vt, pad], 2)
        s = (q @ kt.transpose(-1, -2)) * scale
        mn = torch.maximum(m, s.max(-1).values)
        alpha = torch.exp(m - mn)
        p = torch.exp(s - mn[..., None])
        l = l * alpha + p.sum(-1)
        if mut != "no_rescale":
            o = o * alpha[..., None]
        o = o + p.to(dtype).float() @ vt
        m = mn
    o = o / l[..., None]
    out = o.to(dtype)
    out_lo = (o - out.float()).to(dtype)      # what out's rounding dropped, kept in the half dtype for delta
    lse = m + torch.log(l)
    # delta and dP are the same kind of product (a kernel forms both with the same MFMA steps): where O = V they are equal
    delta = (g.unsqueeze(-2) @ (out.float() + out_lo.float()).unsqueeze(-1)).reshape(B, H, L)
    dp = (g.unsqueeze(-2) @ v.unsqueeze(-1)).reshape(B, H, L, 1) if L == 1 else g @ v.transpose(-1, -2)
    p = torch.exp((q @ k.transpose(-1, -2)) * scale - lse[..., None])
    ds = (p * (dp - delta[..., None])).to(dtype).float()
    p = p.to(dtype).float()
    back = lambda t: t.transpose(1, 2).to(dtype)     # noqa: E731
    return dict(out=out.transpose(1, 2), lse=lse, dq=back(scale * (ds @ k)), dk=back(scale * (ds.transpose(-1, -2) @ q)),
                dv=back(p.transpose(-1, -2) @ g))
