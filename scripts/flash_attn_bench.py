#!/usr/bin/env python3
"""The point decoder's patch attention at the reference's call shapes: the HIP path (csrc/attn.hip through the flash_attn
drop-in) against two torch baselines on the same GPU in the same session.  One JSON line per shape.

Shapes (configs/base.yaml, per sample of the batch; patches of dec_patch_size = 48 tokens, head dimension 8):
  stage 0   T = k_num = 12 000 selected points, 160 channels / 20 heads;
  stage 1   T = 12 000 x upscale_factor[0] (2) x non_leaf_ratio[0] (0.8) = 19 200 tokens, 256 channels / 32 heads;
  stage 1*  T = 24 000: the same stage with the mask off (non_leaf_ratio 1.0), the upper bound.
This is a reading of the configuration, not a trace of the reference (which cannot run here without its other extensions).

Baselines, on the same fp16 data viewed as (patches, 48, 3, H, 8):
  torch     the composition of the reference's non-flash branch, batched over patches: (q * scale) @ k^T, softmax, @ v;
  sdpa      torch.nn.functional.scaled_dot_product_attention on the (patches, H, 48, 8) views.
Times are device events over --iters calls after --warmup calls of the same shape, repeated --repeats times (median and
min..max reported); forward alone runs without autograd.  Bytes are the algorithmic ones: forward reads qkv and writes out
and lse; backward additionally reads dout, out, lse and qkv and writes dqkv.  The fraction is against the 8.0 TB/s HBM3E
peak (a float4 copy reaches 6.3 TB/s on this part).

    python scripts/flash_attn_bench.py [--shape T,H,D] [--dtype fp16] [--iters 200] [--warmup 20] [--repeats 5]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from flash_attn import flash_attn_varlen_qkvpacked_func  # noqa: E402

HBM_PEAK = 8.0e12
PATCH = 48


def timed(fn, iters, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def run(T, H, D, dtype, iters, warmup, repeats):
    dev = torch.device("cuda:0")
    T = T // PATCH * PATCH
    P = T // PATCH
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = torch.randn(T, 3, H, D, generator=g, device=dev).to(dtype).requires_grad_(True)
    dout = torch.randn(T, H, D, generator=g, device=dev).to(dtype)
    cu = torch.arange(0, T + 1, PATCH, dtype=torch.int32, device=dev)
    scale = D ** -0.5

    def hip(x):
        return flash_attn_varlen_qkvpacked_func(x, cu, max_seqlen=PATCH, dropout_p=0, softmax_scale=scale)

    def composition(x):
        q, k, v = x.reshape(P, PATCH, 3, H, D).permute(2, 0, 3, 1, 4).unbind(0)
        attn = torch.softmax((q * scale) @ k.transpose(-2, -1), dim=-1)
        return (attn @ v).transpose(1, 2).reshape(T, H, D)

    def sdpa(x):
        q, k, v = x.reshape(P, PATCH, 3, H, D).permute(2, 0, 3, 1, 4).unbind(0)
        return F.scaled_dot_product_attention(q, k, v, scale=scale).transpose(1, 2).reshape(T, H, D)

    def fwd(f):
        def step():
            with torch.no_grad():
                f(qkv)
        return step

    def fwd_bwd(f):
        def step():
            qkv.grad = None
            f(qkv).backward(dout)
        return step

    e = qkv.element_size()
    bytes_fwd = T * 3 * H * D * e + T * H * D * e + T * H * 4
    bytes_bwd = T * H * D * e * 2 + T * H * 4 + T * 3 * H * D * e * 2
    res = {"T": T, "patches": P, "H": H, "D": D, "dtype": str(dtype), "iters": iters, "warmup": warmup, "repeats": repeats,
           "model_bytes_fwd": bytes_fwd, "model_bytes_bwd": bytes_bwd, "hbm_peak": HBM_PEAK}
    with torch.no_grad():
        ref = composition(qkv).float()
        res["max_abs_diff_hip_vs_torch"] = float((hip(qkv).float() - ref).abs().max())
        res["max_abs_diff_sdpa_vs_torch"] = float((sdpa(qkv).float() - ref).abs().max())
    for name, f in (("hip", hip), ("torch", composition), ("sdpa", sdpa)):
        res[f"{name}_fwd"] = timed(fwd(f), iters, warmup, repeats)
        res[f"{name}_fwd_bwd"] = timed(fwd_bwd(f), iters, warmup, repeats)
    for k in ("fwd", "fwd_bwd"):
        best = min(res[f"torch_{k}"]["median_ms"], res[f"sdpa_{k}"]["median_ms"])
        res[f"speedup_{k}_vs_better_baseline"] = best / res[f"hip_{k}"]["median_ms"]
    res["hbm_frac_fwd"] = bytes_fwd / (HBM_PEAK * res["hip_fwd"]["median_ms"] * 1e-3)
    res["hbm_frac_fwd_bwd"] = (bytes_fwd + bytes_bwd) / (HBM_PEAK * res["hip_fwd_bwd"]["median_ms"] * 1e-3)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shape", action="append", help="T,H,D (repeatable); default the three decoder shapes")
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("flash_attn_bench.py measures on the GPU only")
    dtype = torch.float16 if a.dtype == "fp16" else torch.bfloat16
    for s in a.shape or ["12000,20,8", "19200,32,8", "24000,32,8"]:
        T, H, D = (int(v) for v in s.split(","))
        run(T, H, D, dtype, a.iters, a.warmup, a.repeats)


if __name__ == "__main__":
    main()
