"""The packed-QKV entry points of flash_attn 2.x, with its signatures, on the HIP attention of this repository."""
from generativedensification_amd import attention as _A


def _refuse(dropout_p, causal, window_size, softcap, alibi_slopes, return_attn_probs):
    if dropout_p != 0:
        raise NotImplementedError("dropout_p != 0 is not supported by the HIP attention (the reference passes attn_drop 0.0)")
    if causal:
        raise NotImplementedError("causal=True is not supported by the HIP attention")
    if tuple(window_size) != (-1, -1):
        raise NotImplementedError("a finite window_size is not supported by the HIP attention")
    if softcap != 0:
        raise NotImplementedError("softcap != 0 is not supported by the HIP attention")
    if alibi_slopes is not None:
        raise NotImplementedError("alibi_slopes is not supported by the HIP attention")
    if return_attn_probs:
        raise NotImplementedError("return_attn_probs=True is not supported by the HIP attention")


def flash_attn_varlen_qkvpacked_func(qkv, cu_seqlens, max_seqlen, dropout_p=0.0, softmax_scale=None, causal=False,
                                     window_size=(-1, -1), softcap=0.0, alibi_slopes=None, deterministic=False,
                                     return_attn_probs=False):
    """qkv (total, 3, nheads, headdim), cu_seqlens (batch + 1) int32 -> (total, nheads, headdim).  `deterministic` is
    accepted and has nothing to switch: the backward is always bitwise reproducible."""
    _refuse(dropout_p, causal, window_size, softcap, alibi_slopes, return_attn_probs)
    return _A.attn_varlen_qkvpacked(qkv, cu_seqlens, max_seqlen, softmax_scale)


def flash_attn_qkvpacked_func(qkv, dropout_p=0.0, softmax_scale=None, causal=False, window_size=(-1, -1), softcap=0.0,
                              alibi_slopes=None, deterministic=False, return_attn_probs=False):
    """qkv (batch, seqlen, 3, nheads, headdim) -> (batch, seqlen, nheads, headdim)."""
    _refuse(dropout_p, causal, window_size, softcap, alibi_slopes, return_attn_probs)
    return _A.attn_qkvpacked(qkv, softmax_scale)
