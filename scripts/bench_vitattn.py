#!/usr/bin/env python
"""scripts/bench_vitattn.py — time of the tiled MFMA attention (generativedensification_amd.vitattn, csrc/attn_tiled.hip)
against torch's scaled_dot_product_attention on the same GPU in the same process, at the image encoder's shapes: 12 images of
1025 tokens, head dimension 64, 12 heads (ViT-B/16) and 6 heads (ViT-S/16).

  core    attn_tiled_qkvpacked on one packed (B, L, 3, H, D) tensor against F.scaled_dot_product_attention on the three
          permuted views of the same tensor (what timm hands it), bf16 and fp16; forward alone (no_grad) and forward + backward
          with the gradient of the packed tensor.
  module  one attention module (tests/vitattn_ref.py, the mirror of timm's Attention) at dim 768 and dim 384 under bf16
          autocast with float32 parameters, through vitattn.vit_attention_forward with VITATTN_BACKEND "hip" against its own
          torch forward; forward alone, and forward + backward with the gradients of x and every parameter.

Operands are random, not zero.  Every pair is compared before it is timed.  Timing: warm-up of every shape, then `--repeats`
windows per contender, alternating; a window is as many calls as fill `--window` seconds, between two device events;
microseconds per call, median and range.  TFLOP/s counts 4 B H L^2 D forward and 10 B H L^2 D backward over the device time,
`peak_share` is that over the MI355X's 2.5 PFLOP/s dense bf16 / fp16 MFMA peak.  `recommend` is "hip" only where its median is
lower and the two ranges do not overlap; `default` is the recommendation of the module's forward + backward at dim 768, the
rule VITATTN_BACKEND ships by.  The parent process never touches the GPU: it starts one child under
`timeout -k 10` and relays its output.

Usage: python scripts/bench_vitattn.py [--out profiles/vitattn_bench.json] [--timeout 400]
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORE = ((12, 1025, 12, 64), (12, 1025, 6, 64))      # B, L, H, D
DIMS = (768, 384)
PEAK = 2.5e15


def window(fn, iters):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def timed(fns, seconds, repeats, warmup=3):
    import torch

    iters = {}
    for k, fn in fns.items():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        iters[k] = max(5, math.ceil(seconds * 1e6 / max(window(fn, 5), 1.0)))
    per = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            per[k].append(window(fn, iters[k]))
            torch.cuda.synchronize()
    return {k: {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1),
                "iters": iters[k]} for k, v in per.items()}


def verdict(times, flops=None, a="hip", b="torch"):
    """'hip' only where its median is lower and the two ranges over the windows do not overlap"""
    times[f"{b}_over_{a}"] = round(times[b]["median_us"] / times[a]["median_us"], 2)
    times["recommend"] = "hip" if times[a]["median_us"] < times[b]["median_us"] and times[a]["max_us"] < times[b]["min_us"] else "torch"
    if flops:
        for k in (a, b):
            times[k]["tflops"] = round(flops / times[k]["median_us"] / 1e6, 1)
            times[k]["peak_share"] = round(flops / (times[k]["median_us"] * 1e-6) / PEAK, 3)
    return times


def child(args):
    import torch
    import torch.nn.functional as F

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import vitattn_ref as VR
    from generativedensification_amd import vitattn as V

    assert torch.cuda.is_available(), "bench_vitattn needs the GPU (no CPU fallback)"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)

    def emit(row):
        print(json.dumps(row), flush=True)

    def rel(xs, ys):
        return [float((s.double() - t.double()).norm()) / max(float(t.double().norm()), 1e-30) for s, t in zip(xs, ys)]

    def no_grad(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    for B, L, H, D in CORE:
        for name, dtype in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
            qkv = torch.randn(B, L, 3, H, D, generator=g).to(dev, dtype).requires_grad_(True)
            gout = torch.randn(B, L, H, D, generator=g).to(dev, dtype)
            fns = {"hip": lambda: V.attn_tiled_qkvpacked(qkv),
                   "torch": lambda: F.scaled_dot_product_attention(*qkv.permute(2, 0, 3, 1, 4).unbind(0)).transpose(1, 2)}
            both = {k: (lambda fn: lambda: torch.autograd.grad(fn(), qkv, gout))(fn) for k, fn in fns.items()}
            r = rel([no_grad(fns["hip"])()] + list(both["hip"]()), [no_grad(fns["torch"])()] + list(both["torch"]()))
            tag = f"core_b{B}_l{L}_h{H}_d{D}_{name}"
            emit(dict(case=f"{tag}_output_and_gradient_hip_against_torch_relative_norm", values=[float(f"{v:.3e}") for v in r]))
            assert max(r) <= 2e-2, r      # (a sanity bound: the tests hold the bar)
            f = 4.0 * B * H * L * L * D
            emit(dict(case=f"{tag}_forward", **verdict(timed({k: no_grad(fn) for k, fn in fns.items()}, args.window, args.repeats), f)))
            emit(dict(case=f"{tag}_forward_backward", **verdict(timed(both, args.window, args.repeats), 3.5 * f)))
            del qkv, gout

    default = None
    for dim in DIMS:
        m = VR.make(dim, dim // 64, seed=1).to(dev)
        x = torch.randn(12, 1025, dim, generator=g).to(dev).requires_grad_(True)
        gout = torch.randn(12, 1025, dim, generator=g).to(dev, torch.bfloat16)
        leaves = [x] + list(m.parameters())

        def forward(backend):
            def run():
                V.VITATTN_BACKEND = backend
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    if backend == "hip":
                        assert V.covers(m, x)
                        return V.vit_attention_forward(m, x)
                    return VR.Attention.forward(m, x)
            return run

        both = {k: (lambda fn: lambda: torch.autograd.grad(fn(), leaves, gout))(forward(k)) for k in ("hip", "torch")}
        r = rel([no_grad(forward("hip"))()] + list(both["hip"]()), [no_grad(forward("torch"))()] + list(both["torch"]()))
        emit(dict(case=f"module_dim{dim}_output_and_gradients_hip_against_torch_relative_norm", values=[float(f"{v:.3e}") for v in r]))
        assert max(r) <= 5e-2, r
        emit(dict(case=f"module_dim{dim}_forward", **verdict(timed({k: no_grad(forward(k)) for k in ("hip", "torch")}, args.window,
                                                                   args.repeats))))
        row = verdict(timed(both, args.window, args.repeats))
        emit(dict(case=f"module_dim{dim}_forward_backward", **row))
        if dim == 768:
            default = row["recommend"]
        V.VITATTN_BACKEND = "torch"
    emit(dict(case="default", VITATTN_BACKEND=default))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vitattn_bench.json"))
    ap.add_argument("--timeout", type=int, default=400, help="seconds for the child")
    ap.add_argument("--window", type=float, default=0.25, help="seconds of calls per window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    results = {"core_shapes": [dict(zip(("B", "L", "H", "D"), sh)) for sh in CORE], "module_dims": list(DIMS), "window_s": args.window,
               "repeats": args.repeats, "peak_flops": PEAK, "rows": []}
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--window", str(args.window),
           "--repeats", str(args.repeats)]
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    for line in proc.stdout.splitlines():
        print(line, flush=True)
        if line.startswith("{"):
            results["rows"].append(json.loads(line))
    if proc.returncode:
        print(f"bench_vitattn: the child ended with status {proc.returncode}", file=sys.stderr)
        return proc.returncode
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
