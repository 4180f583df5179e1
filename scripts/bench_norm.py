#!/usr/bin/env python
"""scripts/bench_norm.py — GPU time of the fused row normalisations (generativedensification_amd.norm) against two torch
forms on the same GPU in the same process, at the decoder's shapes of the base config:

  A  ada_layer_norm(feat, scale, offset), B = 1, at (N, C) = (12 000, 160), (24 000, 256), (19 200, 256), (76 800, 256)
       reference   torch_scatter.gather_csr(scale, pad(offset)) * layer_norm(feat)   (this repository's drop-in: one read-back)
       torch       scale.repeat_interleave(counts, 0, output_size=N) * layer_norm(feat)   (no read-back)
  B  pe_concat_layer_norm(x, feat, frequencies, S) at (P, S, C, F) = (12 000, 2, 160, 15), (19 200, 4, 256, 15)
       reference   layer_norm(cat([positional_encoding(f, x), gather_csr(feat, arange(P + 1) * S)]))
       torch       the same with feat.repeat_interleave(S, 0)

fp32 inputs, and bf16 inputs under bf16 autocast (the trainer's state: the results are float32).  Forward alone and forward +
backward.  Every pair is compared before it is timed.  Timing: warm-up, then `--repeats` windows of `--iters` calls per
method, alternating, each window between two device events; microseconds per call, median and range, host work included.
Each row also carries the bytes the call must move (inputs read once, the output written once; for the backward the gradient
and feat read and dfeat written) and the share of the HBM peak (8 TB/s) the fused call reaches with them.  `trig_probe` rows
time the B forward at the same shapes with one frequency: the same rows-to-lanes mapping, 1/15 of the sin / cos evaluations
and fewer output bytes (the row carries its byte count); these times include host work, the kernel times alone come from
scripts/norm_kernel_times.py.
There is no pass bar.  The parent process never touches the GPU: it starts one child under a time limit and relays its output.

Usage: python scripts/bench_norm.py [--out FILE.json] [--timeout 500]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADA_SHAPES = ((12_000, 160), (24_000, 256), (19_200, 256), (76_800, 256))
PE_SHAPES = ((12_000, 2, 160, 15), (19_200, 4, 256, 15))
TRIG_PROBES = ((12_000, 2, 160, 1), (19_200, 4, 256, 1))     # PE_SHAPES with one frequency: the same C, so the same lane mapping
HBM_PEAK = 8.0e12


def window(fn, iters):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def timed(fns, iters, repeats, warmup=5):
    import torch

    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    per = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            per[k].append(window(fn, iters))
    return {k: {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}
            for k, v in per.items()}


def with_share(times, nbytes):
    times["bytes"] = nbytes
    times["hip_share_of_hbm_peak"] = round(nbytes / (times["hip"]["median_us"] * 1e-6) / HBM_PEAK, 3)
    return times


def child(args):
    import torch
    import torch.nn.functional as F

    sys.path.insert(0, ROOT)
    import torch_scatter
    from generativedensification_amd import norm as N

    assert torch.cuda.is_available(), "bench_norm needs the GPU (no CPU fallback)"
    dev = torch.device("cuda:0")
    results = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "repeats": args.repeats, "rows": []}

    def emit(row):
        print(json.dumps(row), flush=True)
        results["rows"].append(row)

    def both(fwd, leaves, gout):
        """(forward alone, forward + backward) of one form"""
        return (lambda: fwd()), (lambda: torch.autograd.grad(fwd(), leaves, gout))

    for dtype, autocast in ((torch.float32, False), (torch.bfloat16, True)):
        es = torch.empty(0, dtype=dtype).element_size()
        ctx = lambda: torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast)      # noqa: E731
        for n, c in ADA_SHAPES:
            g = torch.Generator().manual_seed(n + c)
            feat = torch.randn(n, c, generator=g).to(dtype).to(dev).requires_grad_(True)
            scale = torch.randn(1, c, generator=g).to(dtype).to(dev).requires_grad_(True)
            offset = torch.tensor([n], device=dev)
            counts = torch.tensor([n], device=dev)
            gout = torch.randn(n, c, generator=g).to(dev)
            if not autocast:
                gout = gout.to(dtype)

            def hip():
                with ctx():
                    return N.ada_layer_norm(feat, scale, offset)

            def reference():
                with ctx():
                    return torch_scatter.gather_csr(scale, F.pad(offset, (1, 0), "constant", 0)) * F.layer_norm(feat, (c,))

            def plain():
                with ctx():
                    return scale.repeat_interleave(counts, 0, output_size=n) * F.layer_norm(feat, (c,))

            a, b, d = hip(), reference(), plain()
            assert a.dtype == b.dtype == d.dtype and torch.allclose(a, b, atol=1e-4, rtol=1e-4) and torch.allclose(a, d, atol=1e-4, rtol=1e-4)
            forms = {"hip": both(hip, (feat, scale), gout), "reference": both(reference, (feat, scale), gout),
                     "torch": both(plain, (feat, scale), gout)}
            os_ = a.element_size()
            fwd_bytes = n * c * (es + os_) + c * es + 8
            emit({"case": "ada_forward", "N": n, "C": c, "dtype": str(dtype), "autocast": autocast,
                  **with_share(timed({k: v[0] for k, v in forms.items()}, args.iters, args.repeats), fwd_bytes)})
            emit({"case": "ada_forward_backward", "N": n, "C": c, "dtype": str(dtype), "autocast": autocast,
                  **with_share(timed({k: v[1] for k, v in forms.items()}, args.iters, args.repeats),
                               fwd_bytes + n * c * (os_ + 2 * es) + 2 * c * es)})
        for p, s, c, f in PE_SHAPES + TRIG_PROBES:
            g = torch.Generator().manual_seed(p + c)
            x = (0.004 * torch.tanh(torch.randn(p * s, 3, generator=g))).to(dtype).to(dev).requires_grad_(True)
            feat = torch.randn(p, c, generator=g).to(dtype).to(dev).requires_grad_(True)
            freq = (2.0 ** torch.arange(f)).to(dev)
            ptr = torch.arange(p + 1, dtype=torch.int64, device=dev) * s
            w = 6 * f + c
            gout = torch.randn(p * s, w, generator=g).to(dev)

            def positional_encoding(fr, xx):
                fx = torch.flatten(fr[None, :, None] * xx[:, None, :], -2, -1)
                return torch.cat([torch.sin(fx), torch.cos(fx)], dim=-1)

            def hip():
                with ctx():
                    return N.pe_concat_layer_norm(x, feat, freq, s)

            def reference():
                with ctx():
                    return F.layer_norm(torch.cat([positional_encoding(freq, x), torch_scatter.gather_csr(feat, ptr)], dim=-1), (w,))

            def plain():
                with ctx():
                    return F.layer_norm(torch.cat([positional_encoding(freq, x), feat.repeat_interleave(s, 0)], dim=-1), (w,))

            a, b, d = hip(), reference(), plain()
            assert a.dtype == b.dtype == d.dtype == torch.float32
            assert torch.allclose(a, b, atol=1e-4, rtol=1e-4) and torch.allclose(a, d, atol=1e-4, rtol=1e-4)
            wp = a.stride(0)
            fwd_bytes = p * s * 3 * es + p * c * es + f * 4 + p * s * wp * 4
            if f == 1:
                emit({"case": "trig_probe_pe_forward", "P": p, "S": s, "C": c, "F": f, "dtype": str(dtype), "autocast": autocast,
                      **with_share(timed({"hip": hip}, args.iters, args.repeats), fwd_bytes)})
                continue
            forms = {"hip": both(hip, (x, feat), gout), "reference": both(reference, (x, feat), gout),
                     "torch": both(plain, (x, feat), gout)}
            emit({"case": "pe_forward", "P": p, "S": s, "C": c, "F": f, "dtype": str(dtype), "autocast": autocast,
                  **with_share(timed({k: v[0] for k, v in forms.items()}, args.iters, args.repeats), fwd_bytes)})
            emit({"case": "pe_forward_backward", "P": p, "S": s, "C": c, "F": f, "dtype": str(dtype), "autocast": autocast,
                  **with_share(timed({k: v[1] for k, v in forms.items()}, args.iters, args.repeats),
                               fwd_bytes + p * s * w * 4 + p * s * 3 * es * 2 + 2 * p * c * es)})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=500)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--iters", str(args.iters), "--repeats", str(args.repeats)]
    if args.out:
        cmd += ["--out", args.out]
    try:
        return subprocess.run(cmd, timeout=args.timeout).returncode
    except subprocess.TimeoutExpired:
        print(f"bench_norm: the GPU process did not finish in {args.timeout} s", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
