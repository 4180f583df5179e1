"""Plain-torch restatement of the variable-length packed-QKV attention of generativedensification_amd/csrc/attn.hip (what
flash_attn_varlen_qkvpacked_func computes with dropout 0 and no mask), dtype-generic and written as a loop over sequences
and heads: forward, the per-row log-sum-exp, and the closed-form backward.  Run in f64 it is the truth the GPU tests
measure against; autograd through `attention` cross-checks the closed form (tests/test_attn_cpu.py).

`mut` switches ONE deliberate mistake on, each of a kind an index or a formula in a kernel could have; the CPU tests show
that the inputs of tests/attn_cases.py expose every one of them at the bars the GPU test applies.

`padded_patches` restates, in our own words, how the reference's SerializedAttention turns batch offsets into the gather
`pad`, its inverse `unpad` and `cu_seqlens`."""
import torch

MUTANTS = ("dk_no_scale", "softmax_query_axis", "no_delta", "boundary_off_by_one", "kv_swapped", "heads_d_transposed",
           "lse_total_major", "scale_from_hd")


def _bounds(cu, total, mut):
    cu = [int(c) for c in cu]
    if mut == "boundary_off_by_one":      # every inner boundary one row late
        cu = [cu[0]] + [min(c + 1, cu[-1]) for c in cu[1:-1]] + [cu[-1]]
    return list(zip(cu[:-1], cu[1:]))


def _scale(qkv, scale, mut):
    H, D = qkv.shape[2:]
    if scale is not None:
        return float(scale)
    return float((H * D) ** -0.5) if mut == "scale_from_hd" else float(D ** -0.5)


def _probs(q, k, scale, mut):
    """(P, lse) of one head: q, k (L, D)."""
    s = (q @ k.t()) * scale
    axis = 0 if mut == "softmax_query_axis" else 1
    m = s.max(dim=axis, keepdim=True).values
    e = torch.exp(s - m)
    z = e.sum(dim=axis, keepdim=True)
    lse = (m + torch.log(z)).reshape(-1)
    return e / z, lse


def attention(qkv, cu_seqlens, softmax_scale=None, mut=None):
    """qkv (total, 3, H, D), cu_seqlens (batch + 1) ints -> out (total, H, D), lse (H, total), in qkv's dtype.  Rows no
    sequence owns are zero in both."""
    total, _, H, D = qkv.shape
    scale = _scale(qkv, softmax_scale, mut)
    out = torch.zeros(total, H, D, dtype=qkv.dtype)
    lse = torch.zeros(H, total, dtype=qkv.dtype)
    for a, b in _bounds(cu_seqlens, total, mut):
        if b <= a:
            continue
        for h in range(H):
            q, k, v = qkv[a:b, 0, h], qkv[a:b, 1, h], qkv[a:b, 2, h]
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


def attention_backward(qkv, cu_seqlens, dout, softmax_scale=None, mut=None):
    """The closed form: dV = P^T dO, dS = P o (dO V^T - delta), dQ = scale dS K, dK = scale dS^T Q, delta = rowsum(dO o O).
    dqkv (total, 3, H, D); rows no sequence owns are zero."""
    total, _, H, D = qkv.shape
    scale = _scale(qkv, softmax_scale, mut)
    dqkv = torch.zeros_like(qkv)
    for a, b in _bounds(cu_seqlens, total, mut):
        if b <= a:
            continue
        for h in range(H):
            q, k, v = qkv[a:b, 0, h], qkv[a:b, 1, h], qkv[a:b, 2, h]
            ki, vi = (2, 1) if mut == "kv_swapped" else (1, 2)
            if mut == "kv_swapped":
                k, v = v, k
            do = dout[a:b, h]
            if mut == "heads_d_transposed":
                do = dout.transpose(1, 2).reshape(total, H, D)[a:b, h]
            P, _ = _probs(q, k, scale, mut)
            o = P @ v
            delta = (do * o).sum(dim=1, keepdim=True)
            dP = do @ v.t()
            if mut == "softmax_query_axis":
                delta = (P * dP).sum(dim=0, keepdim=True)
            dS = P * dP if mut == "no_delta" else P * (dP - delta)
            dqkv[a:b, 0, h] = scale * (dS @ k)
            dqkv[a:b, ki, h] = (1.0 if mut == "dk_no_scale" else scale) * (dS.t() @ q)
            dqkv[a:b, vi, h] = P.t() @ do
    return dqkv


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
