"""Plain-torch restatement of the variable-length packed-QKV attention of generativedensification_amd/csrc/attn.hip (what
flash_attn_varlen_qkvpacked_func computes with dropout 0 and no mask), dtype-generic and written as a loop over sequences
and heads: forward, the per-row log-sum-exp, and the closed-form backward.  Run in f64 it is the truth the GPU tests
measure against; autograd through `attention` cross-checks the closed form (tests/test_attn_cpu.py).

`mut` switches ONE deliberate mistake on, each of a kind an index or a formula in a kernel could have; the CPU tests show
that the inputs of tests/attn_cases.py expose every one of them at the bars the GPU test applies.

`padded_patches` restates, in our own words, how the reference's SerializedAttention turns batch offsets into the gather
`pad`, its inverse `unpad` and `cu_seqlens`."""
import torch

# mistakes of the row tile: a 256-thread workgroup holds G = 256 / RP heads of RP rows each (RP = 64, 128 or 256, the smallest
# that holds max_seqlen) and walks the keys in blocks of 8; `rp` tells these mutants the tile of the call
TILE_MUTANTS = ("full_tile_loses_last_row", "pad_keys_score_zero", "partial_block_dropped", "group_reads_first_head")
MUTANTS = ("dk_no_scale", "softmax_query_axis", "no_delta", "boundary_off_by_one", "kv_swapped", "heads_d_transposed",
           "lse_total_major", "scale_from_hd") + TILE_MUTANTS
KEY_BLOCK = 8


def _bounds(cu, total, mut, rp=256):
    cu = [int(c) for c in cu]
    if mut == "boundary_off_by_one":      # every inner boundary one row late
        cu = [cu[0]] + [min(c + 1, cu[-1]) for c in cu[1:-1]] + [cu[-1]]
    if mut == "full_tile_loses_last_row":     # a sequence of exactly RP rows: its last row is neither a query nor a key
        return [(a, b - 1 if b - a == rp else b) for a, b in zip(cu[:-1], cu[1:])]
    return list(zip(cu[:-1], cu[1:]))


def _kv_head(h, mut, rp):
    """the head whose K and V rows head h reads: its own, or (the `g * RP` term missing from an LDS row index) those of the
    first head of its workgroup"""
    return h - h % (256 // rp) if mut == "group_reads_first_head" else h


def _scale(qkv, scale, mut):
    H, D = qkv.shape[2:]
    if scale is not None:
        return float(scale)
    return float((H * D) ** -0.5) if mut == "scale_from_hd" else float(D ** -0.5)


def _probs(q, k, scale, mut):
    """(P, lse) of one head: q, k (L, D)."""
    s = (q @ k.t()) * scale
    L = k.shape[0]
    if mut == "partial_block_dropped" and L > KEY_BLOCK and L % KEY_BLOCK:      # the key loop stops at the last full block
        s = torch.cat([s[:, :L - L % KEY_BLOCK], torch.full_like(s[:, L - L % KEY_BLOCK:], float("-inf"))], 1)
    if mut == "pad_keys_score_zero" and L % KEY_BLOCK:      # the zero rows behind the sequence take part with score 0 (V = 0)
        s = torch.cat([s, torch.zeros_like(s[:, :KEY_BLOCK - L % KEY_BLOCK])], 1)
    axis = 0 if mut == "softmax_query_axis" else 1
    m = s.max(dim=axis, keepdim=True).values
    e = torch.exp(s - m)
    z = e.sum(dim=axis, keepdim=True)
    lse = (m + torch.log(z)).reshape(-1)
    return (e / z)[:, :L], lse


def attention(qkv, cu_seqlens, softmax_scale=None, mut=None, rp=256):
    """qkv (total, 3, H, D), cu_seqlens (batch + 1) ints -> out (total, H, D), lse (H, total), in qkv's dtype.  Rows no
    sequence owns are zero in both.  `rp`: the row tile of the call, read by TILE_MUTANTS only."""
    total, _, H, D = qkv.shape
    scale = _scale(qkv, softmax_scale, mut)
    out = torch.zeros(total, H, D, dtype=qkv.dtype)
    lse = torch.zeros(H, total, dtype=qkv.dtype)
    for a, b in _bounds(cu_seqlens, total, mut, rp):
        if b <= a:
            continue
        for h in range(H):
            hk = _kv_head(h, mut, rp)
            q, k, v = qkv[a:b, 0, h], qkv[a:b, 1, hk], qkv[a:b, 2, hk]
            if mut == "kv_swapped":
                k, v = v, k
            P, l = _probs(q, k, scale, mut)
            out[a:b, h] = P @ v        # (autograd follows slice assignment)
            lse[h, a:b] = l
    if mut == "heads_d_transposed":
        out = out.transpose(1, 2).reshape(total, H, D)
    if mut == "lse_total_major":
        lse = lse.t().reshape(H, total)
    return out, lse


def attention_backward(qkv, cu_seqlens, dout, softmax_scale=None, mut=None, rp=256, out=None):
    """The closed form: dV = P^T dO, dS = P o (dO V^T - delta), dQ = scale dS K, dK = scale dS^T Q, delta = rowsum(dO o O).
    dqkv (total, 3, H, D); rows no sequence owns are zero.  `out` (total, H, D): the forward's result as the backward finds it
    (rounded, say), for delta; by default O is formed again here."""
    total, _, H, D = qkv.shape
    scale = _scale(qkv, softmax_scale, mut)
    dqkv = torch.zeros_like(qkv)
    for a, b in _bounds(cu_seqlens, total, mut, rp):
        if b <= a:
            continue
        for h in range(H):
            hk = _kv_head(h, mut, rp)
            q, k, v = qkv[a:b, 0, h], qkv[a:b, 1, hk], qkv[a:b, 2, hk]
            ki, vi = (2, 1) if mut == "kv_swapped" else (1, 2)
            if mut == "kv_swapped":
                k, v = v, k
            do = dout[a:b, h]
            if mut == "heads_d_transposed":
                do = dout.transpose(1, 2).reshape(total, H, D)[a:b, h]
            P, _ = _probs(q, k, scale, mut)
            o = P @ v if out is None else out[a:b, h]
            delta = (do * o).sum(dim=1, keepdim=True)
            dP = do @ v.t()
            if mut == "softmax_query_axis":
                delta = (P * dP).sum(dim=0, keepdim=True)
            dS = P * dP if mut == "no_delta" else P * (dP - delta)
            dqkv[a:b, 0, h] = scale * (dS @ k)
            dqkv[a:b, ki, h] = (1.0 if mut == "dk_no_scale" else scale) * (dS.t() @ q)
            dqkv[a:b, vi, h] = P.t() @ do
    return dqkv


def kernel_model(qkv, cu_seqlens, dout, softmax_scale=None, out_dtype=None, delta_from_rounded=True):
    """What a CORRECT kernel of csrc/attn.hip's design gives, whatever its summation order: f32 arithmetic from the inputs as
    they are (rounded by the caller), the result rounded to `out_dtype` (default: qkv's), delta from that rounded result (or
    from the f32 one), and gradients that the caller rounds once.  -> out (out_dtype), dqkv (f32).  Its distance to the f64
    restatement, set against a bar, says how much of the bar the roundings every correct kernel shares already use up."""
    q32, out_dtype = qkv.float(), out_dtype or qkv.dtype
    out32, _ = attention(q32, cu_seqlens, softmax_scale)
    out = out32.to(out_dtype)
    dqkv = attention_backward(q32, cu_seqlens, dout.float(), softmax_scale, out=out.float() if delta_from_rounded else out32)
    return out, dqkv


def padded_patches(offset, patch):
    """offset: the cumulative point counts of the samples of a batch (sample i owns points [offset[i-1], offset[i])).
    Returns (pad, unpad, cu_seqlens) as int64, int64, int32 CPU tensors:
      - a sample with MORE than `patch` points is cut into sequences of exactly `patch` tokens; its last, incomplete
        sequence is filled up at the END with the tokens that sit `patch` positions earlier (the tail of its previous
        sequence), so tokens are duplicated, never invented;
      - a sample with at most `patch` points is one short sequence (none at all if it is empty);
      - pad[j] = the point that padded slot j holds, unpad[i] = the padded slot where point i sits (its first copy),
        cu_seqlens = the starts of all sequences and the padded total."""
    offset = [int(o) for o in offset]
    pad, unpad, cu = [], [], []
    p0 = s0 = 0
    for end in offset:
        n = end - s0
        n_pad = -(-n // patch) * patch if n > patch else n
        slots = list(range(n_pad))
        for j in range(n, n_pad):
            slots[j] = j - patch
        pad += [s0 + j for j in slots]
        unpad += [p0 + j for j in range(n)]
        cu += list(range(p0, p0 + n_pad, patch))
        p0, s0 = p0 + n_pad, end
    cu.append(p0)
    return (torch.tensor(pad, dtype=torch.int64), torch.tensor(unpad, dtype=torch.int64), torch.tensor(cu, dtype=torch.int32))
