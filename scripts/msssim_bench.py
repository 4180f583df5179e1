#!/usr/bin/env python3
"""MS-SSIM at the reference's training shape: the fused HIP path (csrc/ssim.hip) against the torch composition that
pytorch_msssim runs (grouped separable F.conv2d + F.avg_pool2d, fp32).  One JSON line per shape.

Both paths read the reference's layout: X, Y = permuted (B, H, V*W, 3) views, NCHW with channel stride 1
(lightning/loss.py passes image.permute(0, 3, 1, 2)); only X requires grad, as there.  Times are device events over
--iters iterations after --warmup.  The byte model counts the fused path's unavoidable HBM traffic per call (levels,
pyramid, coefficient maps, gradients; halo re-reads not counted) against the 8 TB/s HBM peak.

    python scripts/msssim_bench.py [--shape 3,3,512,4096] [--shape 1,3,512,512] [--iters 20] [--warmup 5]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from generativedensification_amd.ssim import ms_ssim  # noqa: E402

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
HBM_PEAK = 8.0e12


def torch_ms_ssim(X, Y, data_range=1.0, win_size=11, win_sigma=1.5, K=(0.01, 0.03)):
    """pytorch_msssim's composition: per level 5 grouped separable convolutions + elementwise terms, avg_pool2d between."""
    Ch = X.shape[1]
    coords = torch.arange(win_size, dtype=torch.float32) - win_size // 2
    g = torch.exp(-(coords ** 2) / (2 * win_sigma ** 2))
    g = (g / g.sum()).to(X.device)
    wh, ww = g.view(1, 1, -1, 1).repeat(Ch, 1, 1, 1), g.view(1, 1, 1, -1).repeat(Ch, 1, 1, 1)

    def filt(t):
        return F.conv2d(F.conv2d(t, wh, groups=Ch), ww, groups=Ch)

    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    w = torch.tensor(WEIGHTS, device=X.device)
    mcs = []
    for lvl in range(len(WEIGHTS)):
        mu1, mu2 = filt(X), filt(Y)
        s11, s22, s12 = filt(X * X) - mu1 ** 2, filt(Y * Y) - mu2 ** 2, filt(X * Y) - mu1 * mu2
        cs_map = (2 * s12 + C2) / (s11 + s22 + C2)
        ssim_map = (2 * mu1 * mu2 + C1) / (mu1 ** 2 + mu2 ** 2 + C1) * cs_map
        if lvl < len(WEIGHTS) - 1:
            mcs.append(torch.relu(cs_map.flatten(2).mean(-1)))
            pad = [s % 2 for s in X.shape[2:]]
            X, Y = F.avg_pool2d(X, kernel_size=2, padding=pad), F.avg_pool2d(Y, kernel_size=2, padding=pad)
    v = torch.prod(torch.stack(mcs + [torch.relu(ssim_map.flatten(2).mean(-1))]) ** w.view(-1, 1, 1), dim=0)
    return v.mean()


def byte_model(B, C, H, W, k=11, levels=5):
    P, fwd, bwd = B * C, 0, 0
    h, w = H, W
    for lvl in range(levels):
        n, nv = P * h * w, P * (h - k + 1) * (w - k + 1)
        h2, w2 = (h + h % 2) // 2, (w + w % 2) // 2
        n2 = P * h2 * w2
        fwd += 8 * n                                    # tile kernel reads X, Y
        if lvl < levels - 1:
            fwd += 8 * n + 8 * n2                       # pool reads X, Y, writes the next level
        bwd += 8 * n + 16 * nv                          # coefficient kernel: X, Y in, float4 map out
        bwd += 16 * nv + 8 * n + 4 * n                  # gradient kernel: map, X, Y in, dX out
        if lvl < levels - 1:
            bwd += 4 * n2                               # + the coarser level's dX
        h, w = h2, w2
    return fwd, bwd


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def run(shape, iters, warmup):
    B, C, H, W = shape
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    img = torch.rand(B, H, W, C, generator=g, device=dev)
    tar = (img + 0.1 * torch.randn(B, H, W, C, generator=g, device=dev)).clamp(0, 1)
    X0, Y = img.permute(0, 3, 1, 2), tar.permute(0, 3, 1, 2)
    X = img.clone().requires_grad_(True)

    def fwd(f):
        return lambda: f(X.detach().permute(0, 3, 1, 2), Y)

    def fwd_bwd(f):
        def step():
            X.grad = None
            f(X.permute(0, 3, 1, 2), Y).backward()
        return step

    hip = lambda a, b: ms_ssim(a, b, data_range=1.0)   # noqa: E731
    res = {"shape": list(shape), "layout": "permuted NHWC view (channel stride 1)", "iters": iters, "warmup": warmup}
    res["hip_fwd_ms"] = timed(fwd(hip), iters, warmup)
    res["hip_fwd_bwd_ms"] = timed(fwd_bwd(hip), iters, warmup)
    res["torch_fwd_ms"] = timed(fwd(torch_ms_ssim), iters, warmup)
    res["torch_fwd_bwd_ms"] = timed(fwd_bwd(torch_ms_ssim), iters, warmup)
    res["speedup_fwd_bwd"] = res["torch_fwd_bwd_ms"] / res["hip_fwd_bwd_ms"]
    v_h, v_t = float(hip(X0, Y)), float(torch_ms_ssim(X0, Y))
    res["value_hip"], res["value_torch"] = v_h, v_t
    fb, bb = byte_model(B, C, H, W)
    res["model_bytes_fwd"], res["model_bytes_bwd"] = fb, bb
    res["hbm_frac_fwd"] = fb / (HBM_PEAK * res["hip_fwd_ms"] * 1e-3)
    res["hbm_frac_fwd_bwd"] = (fb + bb) / (HBM_PEAK * res["hip_fwd_bwd_ms"] * 1e-3)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shape", action="append", help="B,C,H,W (repeatable); default 3,3,512,4096")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("msssim_bench.py measures on the GPU only")
    for s in a.shape or ["3,3,512,4096"]:
        run(tuple(int(v) for v in s.split(",")), a.iters, a.warmup)


if __name__ == "__main__":
    main()
