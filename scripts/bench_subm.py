#!/usr/bin/env python
"""scripts/bench_subm.py — GPU time of the submanifold sparse convolution (generativedensification_amd.sparse_conv) against
a torch composition of the same arithmetic on the same GPU in the same process: per tap one `index_select`, one `matmul`
and one `index_add_` over the rows that have a neighbour, on the table the HIP build made (so both do the same sums).

Shapes: N = 24 000 at C = 160 and N = 76 800 at C = 256, kernel size 3, fp16.  Coordinates are made the way the decoder's
upscale step makes them: parents on a surface-like shell, 4 children jittered within half a parent cell of each, re-gridded at
half the cell size — so some children share a voxel.  Per shape the script prints the share of sites that share a voxel and
the mean number of taps that fire per site, then forward alone (no_grad) and forward + backward (features, weight, bias) for
both methods, timed alternately window by window: warm-up, then `--repeats` windows of `--iters` calls, each window between
two device events; microseconds per call, median and range, host work included.  The table build is timed on its own.  The
outputs and gradients of the two methods are compared before anything is timed.  No pass / fail beyond that comparison.

The parent process never touches the GPU: it starts one child under a time limit and relays its output.

Usage: python scripts/bench_subm.py [--out FILE.json] [--timeout 500]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((24_000, 160), (76_800, 256))


def decoder_like_sites(n, seed):
    """(n, 4) int32 (batch 0) and the grid extent: n / 4 parents on a sphere shell in a grid of G cells, 4 children each
    within half a parent cell, re-gridded at half the cell size"""
    import torch

    g = torch.Generator().manual_seed(seed)
    parents = n // 4
    G = max(8, int(1.1 * parents ** 0.5))                   # a shell of radius 0.4 G crosses ~ 2 G^2 cells: ~ 0.4 parents per cell
    d = torch.randn(parents * 6, 3, generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    cell = torch.unique(torch.floor((0.5 + 0.4 * d) * G).long(), dim=0)
    cell = cell[torch.randperm(cell.shape[0], generator=g)[:parents]]
    centre = cell.float() + 0.5
    child = centre.repeat_interleave(4, 0) + (torch.rand(cell.shape[0] * 4, 3, generator=g) - 0.5)
    grid = torch.floor(child * 2).long().clamp_(0, 2 * G - 1)
    idx = torch.cat([torch.zeros(grid.shape[0], 1, dtype=torch.long), grid], 1).int()
    return idx, 2 * G


def torch_subm(feat, nbr_rows, weight, bias):
    """nbr_rows: per tap (rows with a neighbour, their neighbours), made once from the table"""
    import torch

    Cout, Cin = weight.shape[0], weight.shape[-1]
    wk = weight.reshape(Cout, -1, Cin)
    out = bias.unsqueeze(0).repeat(feat.shape[0], 1)
    for k, (rows, src) in enumerate(nbr_rows):
        if rows.numel():
            out.index_add_(0, rows, torch.matmul(feat.index_select(0, src), wk[:, k].t()))
    return out


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
    return {k: {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1),
                "iters": iters, "repeats": repeats} for k, v in per.items()}


def rel_l2(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-30))


def child(args):
    import torch

    sys.path.insert(0, ROOT)
    from generativedensification_amd import sparse_conv as S

    assert torch.cuda.is_available(), "bench_subm needs the GPU (no CPU fallback)"
    dev = torch.device("cuda:0")
    results = {"device": torch.cuda.get_device_name(0), "dtype": "float16", "kernel_size": 3, "shapes": []}
    for n, C in SHAPES:
        idx, G = decoder_like_sites(n, n)
        N = idx.shape[0]
        idx = idx.to(dev)
        table = S.build_table(idx, (G, G, G), 1, 3)
        shared = float((torch.bincount(table.rep.long(), minlength=N)[table.rep.long()] > 1).float().mean())
        taps = float((table.nbr >= 0).float().sum() / N)
        g = torch.Generator().manual_seed(C)
        feat = torch.randn(N, C, generator=g).half().to(dev).requires_grad_(True)
        weight = (torch.randn(C, 3, 3, 3, C, generator=g) / (27 * C) ** 0.5).half().to(dev).requires_grad_(True)
        bias = torch.randn(C, generator=g).half().to(dev).requires_grad_(True)
        gout = torch.randn(N, C, generator=g).half().to(dev)
        rows = []
        for k in range(27):
            r = torch.nonzero(table.nbr[k] >= 0).squeeze(1)
            rows.append((r, table.nbr[k, r].long()))
        leaves = (feat, weight, bias)

        def run(hip, backward):
            f = (lambda: S.subm_conv3d(feat, table, weight, bias)) if hip else (lambda: torch_subm(feat, rows, weight, bias))
            if not backward:
                with torch.no_grad():
                    return f()
            return torch.autograd.grad(f(), leaves, gout)

        row = {"N": N, "C": C, "grid": G, "share_of_sites_sharing_a_voxel": round(shared, 4), "mean_taps_per_site": round(taps, 2),
               "rel_l2_diff_forward": rel_l2(run(True, False), run(False, False)),
               "rel_l2_diff_grads": [rel_l2(a, b) for a, b in zip(run(True, True), run(False, True))]}
        print(json.dumps(row), flush=True)
        assert row["rel_l2_diff_forward"] < 5e-3 and max(row["rel_l2_diff_grads"]) < 5e-3, row
        row["table_build"] = timed({"hip": lambda: S.build_table(idx, (G, G, G), 1, 3)}, args.iters, args.repeats)
        row["forward"] = timed({"hip": lambda: run(True, False), "torch": lambda: run(False, False)}, args.iters, args.repeats)
        row["forward_backward"] = timed({"hip": lambda: run(True, True), "torch": lambda: run(False, True)}, args.iters,
                                        args.repeats)
        print(json.dumps(row), flush=True)
        results["shapes"].append(row)
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
        print(f"bench_subm: the GPU process did not finish in {args.timeout} s", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
