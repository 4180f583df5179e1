#!/usr/bin/env python
"""scripts/bench_scatter.py — GPU time of the segment reductions (generativedensification_amd.segment, the torch_scatter /
torch_geometric drop-ins) against the torch composition a user without the package would write, on the same GPU in the same
process.  At N = 12 000 / 24 000 / 96 000, C = 160 / 256 (fp16), B = 1 and 4:

  global_pooling      segment_csr(feat, pad(offset), "mean")             vs torch.segment_reduce(feat, "mean", lengths)
  serialized_pooling  segment_csr(feat[indices], idx_ptr, "max") and segment_csr(coord[indices], idx_ptr, "mean"), on the
                      clusters torch.unique gives for the z-order codes of a seeded cloud shifted by one level
                                                                          vs index_reduce_("amax") and index_add_ / count
  upscale             gather_csr(x, arange(N / 4 + 1) * 4) forward + backward  vs repeat_interleave(4) forward + backward
  top_k_count         torch_geometric.utils.scatter(ones, batch, "sum")  vs zeros(B).index_add_(0, batch, ones)

Every pair is compared before it is timed (global_pooling: each against float64, both errors recorded).  Timing: warm-up,
then `--repeats` windows of `--iters` calls per method, alternating, each window between two device events; microseconds per call, median and range, host work included.  There is
no pass bar.  The parent process never touches the GPU: it starts one child under a time limit and relays its output.

Usage: python scripts/bench_scatter.py [--out FILE.json] [--timeout 500]
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (12_000, 24_000, 96_000)
CHANNELS = (160, 256)
BATCHES = (1, 4)


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


def morton(grid, depth):
    import torch

    code = torch.zeros(grid.shape[0], dtype=torch.int64)
    for b in range(depth):
        for axis in range(3):
            code |= ((grid[:, axis] >> b) & 1) << (3 * b + 2 - axis)
    return code


def child(args):
    import torch

    sys.path.insert(0, ROOT)
    import torch_scatter
    from torch_geometric.utils import scatter as pyg_scatter

    assert torch.cuda.is_available(), "bench_scatter needs the GPU (no CPU fallback)"
    dev = torch.device("cuda:0")
    results = {"device": torch.cuda.get_device_name(0), "dtype": "float16", "iters": args.iters, "repeats": args.repeats, "rows": []}

    def emit(row):
        print(json.dumps(row), flush=True)
        results["rows"].append(row)

    for n in SIZES:
        g = torch.Generator().manual_seed(n)
        coord = torch.rand(n, 3, generator=g)
        depth = 1 + max(1, round(math.log2((n / 3) ** (1 / 3))))     # about 3 points per cell of the pooled grid: short clusters
        code = morton((coord * (1 << depth)).long(), depth) >> 3
        _, cluster, counts = torch.unique(code.to(dev), sorted=True, return_inverse=True, return_counts=True)
        _, indices = torch.sort(cluster)
        idx_ptr = torch.cat([counts.new_zeros(1), torch.cumsum(counts, dim=0)])
        S = counts.numel()
        coord_d = coord.to(dev)
        for C in CHANNELS:
            feat = torch.randn(n, C, generator=g).half().to(dev)
            # SerializedPooling pair
            def hip_pool():
                return (torch_scatter.segment_csr(feat[indices], idx_ptr, reduce="max"),
                        torch_scatter.segment_csr(coord_d[indices], idx_ptr, reduce="mean"))

            def torch_pool():
                f = torch.empty(S, C, dtype=feat.dtype, device=dev).index_reduce_(0, cluster, feat, "amax", include_self=False)
                c = torch.zeros(S, 3, device=dev).index_add_(0, cluster, coord_d) / counts.unsqueeze(1)
                return f, c

            a, b = hip_pool(), torch_pool()
            assert torch.equal(a[0], b[0]) and torch.allclose(a[1], b[1], atol=1e-5), "serialized_pooling differs"
            emit({"case": "serialized_pooling", "N": n, "C": C, "segments": S, "longest": int(counts.max()), **timed({"hip": hip_pool, "torch": torch_pool},
                                                                                     args.iters, args.repeats)})
            # upscale: N / 4 parents to N children, forward + backward
            x = feat[: n // 4].clone().requires_grad_(True)
            ptr4 = torch.arange(n // 4 + 1, dtype=torch.int64, device=dev) * 4
            gout = torch.randn(n // 4 * 4, C, generator=g).half().to(dev)

            def hip_up():
                return torch.autograd.grad(torch_scatter.gather_csr(x, ptr4), x, gout)[0]

            def torch_up():
                return torch.autograd.grad(x.repeat_interleave(4, dim=0), x, gout)[0]

            assert torch.allclose(hip_up().float(), torch_up().float(), atol=2e-2, rtol=2e-3), "upscale differs"
            emit({"case": "upscale_fwd_bwd", "N": n // 4 * 4, "C": C, **timed({"hip": hip_up, "torch": torch_up}, args.iters, args.repeats)})
            for B in BATCHES:
                sizes = [n // B + (1 if i < n % B else 0) for i in range(B)]
                lengths = torch.tensor(sizes, device=dev)
                padded = torch.nn.functional.pad(torch.cumsum(lengths, 0), (1, 0))

                def hip_gp():
                    return torch_scatter.segment_csr(src=feat, indptr=padded, reduce="mean")

                def torch_gp():
                    return torch.segment_reduce(feat, "mean", lengths=lengths, axis=0)

                truth = torch.segment_reduce(feat.double(), "mean", lengths=lengths, axis=0)
                err = {k: float((f().double() - truth).abs().max()) for k, f in (("hip", hip_gp), ("torch", torch_gp))}
                assert err["hip"] <= 1e-4, ("global_pooling differs from float64", err)     # (means of ~1e-2: half an fp16 ulp is 4e-6)
                emit({"case": "global_pooling", "N": n, "C": C, "B": B, "max_err_vs_f64": err,
                      **timed({"hip": hip_gp, "torch": torch_gp}, args.iters, args.repeats)})
        for B in BATCHES:
            batch = torch.randint(0, B, (n,), generator=g).to(dev)
            ones = batch.new_ones(n)

            def hip_count():
                return pyg_scatter(ones, batch, dim_size=B, reduce="sum")

            def torch_count():
                return torch.zeros(B, dtype=torch.int64, device=dev).index_add_(0, batch, ones)

            assert torch.equal(hip_count(), torch_count()), "top_k_count differs"
            emit({"case": "top_k_count", "N": n, "B": B, **timed({"hip": hip_count, "torch": torch_count}, args.iters, args.repeats)})
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
        print(f"bench_scatter: the GPU process did not finish in {args.timeout} s", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
