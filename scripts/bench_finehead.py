#!/usr/bin/env python
"""scripts/bench_finehead.py — GPU time of the fused fine Gaussian head and of the fine-set assembly
(generativedensification_amd.finehead) against the reference's lines on the same GPU in the same process, at the base config's
shapes: C 256, sh_dim 12 (20 attribute columns), decoder levels of 4 800 and 76 800 rows, 262 144 coarse Gaussians, k_num 12 000.

  head      a module with GaussianModule's surface (tests/finehead_ref.py make_module) with forward bound to
            gaussian_module_forward: HEAD_BACKEND "hip" against "torch".  "torch" runs the reference's lines, which is the path of
            the parent commit.  Forward alone, and forward + backward (the gradients of the rows and of the four parameters), at
            each of the two row counts.
  assembly  assemble_fine_gaussians (with the survivor count the caller knows) against `_union_gaussians` and the five
            concatenations (tests/finehead_ref.py reference_assemble), forward alone and forward + backward (level coords and
            attributes, the four coarse tensors, shs_fine).  The script draws `mask` and prints n_masked.

Every row carries the bytes the call has to move at least (each operand read once, each result written once) and its time over
the time of those bytes at --peak-tbs TB/s.  fp32, and bf16 autocast (the trainer's state: float32 parameters, bfloat16 rows and
attributes).  Operands are random, not zero.  Every pair is compared before it is timed.  Timing: warm-up, then `--repeats` windows
of `--iters` calls per method, alternating, each window between two device events; microseconds per call, median and range.  There
is no pass bar.  The parent process never touches the GPU: it starts one child per mode, each under its own `timeout -k 10`, and
relays their output.

Usage: python scripts/bench_finehead.py [--out profiles/finehead_bench.json] [--timeout 240]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, SH, SH_DEGREE = 256, 12, 1
LEVELS = (4800, 76800)
NC, K_NUM, MASK_SHARE = 262144, 12000, 0.5
OPACITY_SHIFT, SCALING_SHIFT = -2.1792, -4.3
MODES = ("fp32", "bf16-autocast")


def window(fn, iters):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def timed(fns, iters, repeats, warmup=3):
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


def verdict(times, least_bytes, peak_tbs, a="hip", b="torch"):
    """'hip' only where its median is lower and the two ranges over the windows do not overlap"""
    times[f"{b}_over_{a}"] = round(times[b]["median_us"] / times[a]["median_us"], 2)
    times["recommend"] = "hip" if times[a]["median_us"] < times[b]["median_us"] and times[a]["max_us"] < times[b]["min_us"] else "torch"
    floor_us = least_bytes / (peak_tbs * 1e12) * 1e6
    times.update(least_bytes=least_bytes, floor_us=round(floor_us, 2), hip_over_floor=round(times[a]["median_us"] / floor_us, 1),
                 torch_over_floor=round(times[b]["median_us"] / floor_us, 1))
    return times


def child(args):
    import torch

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import finehead_ref as R                 # the module built from tests/golden/finehead_surface.json, and the reference's lines
    from generativedensification_amd import finehead as H

    assert torch.cuda.is_available(), "bench_finehead needs the GPU (no CPU fallback)"
    dev = torch.device("cuda:0")
    bf16 = torch.bfloat16
    mode = args.child
    autocast = mode != "fp32"
    dtype = bf16 if autocast else torch.float32
    es, P = (2 if autocast else 4), SH + 8
    tol = 5e-2 if autocast else 1e-4

    def emit(row):
        row["mode"] = mode
        print(json.dumps(row), flush=True)

    g = torch.Generator().manual_seed(0)
    m = R.make_module("GaussianModule", C, SH_DEGREE).to(dev)
    type(m).forward = H.gaussian_module_forward
    params = tuple(m.feat2attr.parameters())
    param_bytes = sum(t.numel() for t in params) * 4

    # ---- the head ----
    for rows in LEVELS:
        # the rows as the decoder's last stage hands them over: dense, in the autocast dtype under autocast
        x = (torch.randn(rows, C, generator=g) * 1.5 + 0.3).to(dev, dtype).requires_grad_(True)
        gout = torch.randn(rows, P, generator=g).to(dev, dtype)
        ins = (x,) + params

        def forward(backend):
            def run():
                H.HEAD_BACKEND = backend
                with torch.autocast("cuda", dtype=bf16, enabled=autocast):
                    return m(R.Point(leaf_point=R.Point(feat=x))).leaf_point.attribute
            return run

        def both(backend):
            fwd = forward(backend)

            def run():
                return torch.autograd.grad(fwd(), ins, gout)
            return run

        with torch.no_grad():
            a, b = forward("hip")(), forward("torch")()
            assert a.dtype == b.dtype and a.shape == b.shape and float((a.float() - b.float()).abs().max()) <= tol * float(b.float().abs().max())
        ga, gb = both("hip")(), both("torch")()
        rel = [float((s.double() - t.double()).norm()) / float(t.double().norm()) for s, t in zip(ga, gb)]
        emit(dict(case=f"head_{rows}_gradients_hip_against_torch_relative_norm", values=[float(f"{r:.3e}") for r in rel]))
        assert all(s.dtype == t.dtype for s, t in zip(ga, gb)) and max(rel) <= 4 * tol
        del a, b, ga, gb

        def no_grad(fn):
            def run():
                with torch.no_grad():
                    return fn()
            return run

        fwd_bytes = rows * (C + P) * es + param_bytes
        emit(dict(case=f"head_{rows}_forward", **verdict(timed({"hip": no_grad(forward("hip")), "torch": no_grad(forward("torch"))}, args.iters, args.repeats),
                                                         fwd_bytes, args.peak_tbs)))
        emit(dict(case=f"head_{rows}_forward_backward", **verdict(timed({"hip": both("hip"), "torch": both("torch")}, args.iters, args.repeats),
                                                                  fwd_bytes + rows * (2 * C + P) * es + 2 * param_bytes, args.peak_tbs)))
    H.HEAD_BACKEND = "hip"

    # ---- the assembly ----
    mask = torch.rand(NC, generator=g) < MASK_SHARE
    n_masked = int(mask.sum())
    selected = torch.zeros(n_masked, dtype=torch.bool)
    selected[torch.randperm(n_masked, generator=g)[:K_NUM]] = True
    n_survivors = n_masked - K_NUM
    emit(dict(case="assembly_shape", Nc=NC, n_masked=n_masked, k_num=K_NUM, n_survivors=n_survivors, levels=list(LEVELS)))
    mask, selected = mask.to(dev), selected.to(dev)
    rand = lambda *s: torch.randn(*s, generator=g).to(dev).requires_grad_(True)      # noqa: E731
    levels = [(rand(n, 3), torch.randn(n, P, generator=g).to(dev, dtype).requires_grad_(True)) for n in LEVELS]
    coarse = [rand(NC, w) for w in (3, 1, 3, 4)]
    fine = rand(n_masked, SH // 3, 3)
    leaves = [t for level in levels for t in level] + coarse + [fine]
    T = sum(LEVELS) + n_survivors
    gouts = [torch.randn(T, *s, generator=g).to(dev) for s in ((3,), (SH // 3, 3), (1,), (3,), (4,))]

    def hip():
        return H.assemble_fine_gaussians(levels, *coarse, fine, mask, selected, SH, OPACITY_SHIFT, SCALING_SHIFT, n_survivors=n_survivors)

    def tor():
        return R.reference_assemble(levels, coarse, fine, mask, selected, SH, OPACITY_SHIFT, SCALING_SHIFT)

    def both(fn):
        def run():
            return torch.autograd.grad(fn(), leaves, gouts)
        return run

    with torch.no_grad():
        assert all(torch.equal(s, t) for s, t in zip(hip(), tor()))
    assert all(s.dtype == t.dtype and torch.equal(s, t) for s, t in zip(both(hip)(), both(tor)()))

    def no_grad(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    L_rows = sum(LEVELS)
    fwd_bytes = T * (P + 3) * 4 + L_rows * (12 + P * es) + n_survivors * (P + 3) * 4 + NC + n_masked
    bwd_bytes = T * (P + 3) * 4 + L_rows * (12 + P * es) + NC * 11 * 4 + n_masked * SH * 4
    emit(dict(case="assembly_forward", **verdict(timed({"hip": no_grad(hip), "torch": no_grad(tor)}, args.iters, args.repeats), fwd_bytes, args.peak_tbs)))
    emit(dict(case="assembly_forward_backward", **verdict(timed({"hip": both(hip), "torch": both(tor)}, args.iters, args.repeats), fwd_bytes + bwd_bytes,
                                                          args.peak_tbs)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "finehead_bench.json"))
    ap.add_argument("--timeout", type=int, default=240, help="seconds for each mode's child")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--peak-tbs", type=float, default=8.0, help="the HBM rate the byte floor is turned into time with")
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    results = {"shape": {"C": C, "sh_dim": SH, "levels": list(LEVELS), "Nc": NC, "k_num": K_NUM}, "iters": args.iters, "repeats": args.repeats,
               "peak_tbs": args.peak_tbs, "rows": []}
    for mode in MODES:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", mode, "--iters", str(args.iters),
               "--repeats", str(args.repeats), "--peak-tbs", str(args.peak_tbs)]
        proc = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        for line in proc.stdout.splitlines():
            print(line, flush=True)
            if line.startswith("{"):
                results["rows"].append(json.loads(line))
        if proc.returncode:
            print(f"bench_finehead: the {mode} child ended with status {proc.returncode}; nothing more is started", file=sys.stderr)
            return proc.returncode
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
