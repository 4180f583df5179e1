#!/usr/bin/env python
"""scripts/bench_upscale.py — GPU time of UpscaleModule's fused glue (generativedensification_amd.upscale) against the
reference's lines on the same GPU in the same process, at the two UpscaleModule shapes of the base config: 12 000 parents x
S = 2 at C = 160 -> 256, and 19 200 parents x S = 4 at C = 256 -> 256; F = 15, B = 1.

  module    a module with UpscaleModule's surface (tests/upscale_ref.py make_module, its norms bound to the fused AdaLayerNorm as
            INTEGRATION §12 binds them) with forward bound to upscale_module_forward: UPSCALE_BACKEND "hip" against "torch".
            "torch" runs the reference's lines over this repository's drop-ins, which is the path of the parent commit.  Forward
            alone, and forward + backward with every gradient (feat, coord, global_feat and all parameters).  Host work and
            allocations are included.
  pieces    expand and merge alone, forward and forward + backward, against the torch compositions without a read-back
            (tests/upscale_ref.py torch_expand / torch_merge), each with the bytes the call has to move at least (each operand
            read once, each result written once) and its time over the time of those bytes at --peak-tbs TB/s.

fp32, and bf16 autocast (the trainer's state: float32 parameters).  Operands are random, not zero.  Every pair is compared
before it is timed.  Timing: warm-up, then `--repeats` windows of `--iters` calls per method, alternating, each window between
two device events; microseconds per call, median and range.  `recommend` is "hip" only where its median is lower and the two
ranges do not overlap; UPSCALE_BACKEND ships as "hip" only if that holds for bf16-autocast forward + backward at both shapes.
The parent process never touches the GPU: it starts one child per mode, each under its own `timeout -k 10`, and relays their
output.

Usage: python scripts/bench_upscale.py [--out profiles/upscale_bench.json] [--timeout 240]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((12000, 2, 160, 256), (19200, 4, 256, 256))      # parents, S, C, Cout
F, B, GLOBAL, GRID = 15, 1, 24, 0.008
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
    if least_bytes:
        floor_us = least_bytes / (peak_tbs * 1e12) * 1e6
        times.update(least_bytes=least_bytes, floor_us=round(floor_us, 2), hip_over_floor=round(times[a]["median_us"] / floor_us, 1),
                     torch_over_floor=round(times[b]["median_us"] / floor_us, 1))
    return times


def child(args):
    import torch

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import upscale_ref as R
    from generativedensification_amd import norm as N
    from generativedensification_amd import upscale as U

    assert torch.cuda.is_available(), "bench_upscale needs the GPU (no CPU fallback)"
    dev = torch.device("cuda:0")
    bf16 = torch.bfloat16
    mode = args.child
    autocast = mode != "fp32"
    lo = bf16 if autocast else torch.float32
    es = 2 if autocast else 4
    tol = 5e-2 if autocast else 1e-4

    def emit(row):
        row["mode"] = mode
        print(json.dumps(row), flush=True)

    def close(a, b):
        return a.dtype == b.dtype and a.shape == b.shape and float((a.float() - b.float()).abs().max()) <= tol * max(float(b.float().abs().max()), 1e-30)

    def rel(xs, ys):
        return [float((s.double() - t.double()).norm()) / max(float(t.double().norm()), 1e-30) for s, t in zip(xs, ys)]

    def no_grad(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    g = torch.Generator().manual_seed(0)
    rand = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    for n, s, c, co in SHAPES:
        tag = f"{n}x{s}_c{c}"
        rows, w = n * s, 6 * F + c
        wp = (w + 7) // 8 * 8

        # ---- the bound forward ----
        m = R.make_module(c, co, s, F, global_channels=GLOBAL, ada_forward=N.ada_layer_norm_forward).to(dev)
        m.eval()                                 # (the base config's drop_path is 0: no draw)
        type(m).forward = U.upscale_module_forward
        coord = (torch.rand(n, 3, generator=g) - 0.5).to(dev).requires_grad_(True)
        feat = (rand(n, c) * 1.5 + 0.3).to(dev).requires_grad_(True)
        glob = rand(B, GLOBAL).to(dev).requires_grad_(True)
        offset = torch.tensor([n], device=dev)
        leaves = [feat, coord, glob] + list(m.parameters())

        def forward(backend):
            def run():
                U.UPSCALE_BACKEND = backend
                with torch.autocast("cuda", dtype=bf16, enabled=autocast):
                    p = m(R.Point(coord=coord, feat=feat, global_feat=glob, offset=offset, grid_size=GRID))
                return p.feat, p.coord
            return run

        gouts = None

        def both(backend):
            fwd = forward(backend)

            def run():
                return torch.autograd.grad(fwd(), leaves, gouts)
            return run

        with torch.no_grad():
            a, b = forward("hip")(), forward("torch")()
            # (by the norm: one tanh that rounds the other way moves a sin(2^14 x) column by up to 0.3 under bf16)
            assert all(x.dtype == y.dtype for x, y in zip(a, b)) and max(rel(a, b)) <= tol, rel(a, b)
            gouts = [rand(*t.shape).to(dev, t.dtype) for t in a]
        ga, gb = both("hip")(), both("torch")()
        r = rel(ga, gb)
        emit(dict(case=f"module_{tag}_gradients_hip_against_torch_relative_norm", values=[float(f"{v:.3e}") for v in r]))
        assert all(x.dtype == y.dtype for x, y in zip(ga, gb)) and max(r) <= (0.5 if autocast else 1e-2)      # (a sanity bound: the tests hold the bar)
        del a, b, ga, gb
        x_es, h_es, o_es = 4, 4 if autocast else es, 4 if autocast else es      # coord and, under autocast, the norms' results are f32
        expand_bytes = n * 3 * s * es + n * 3 * 4 + n * c * 4 + rows * 3 * x_es + rows * wp * h_es + F * 4
        merge_bytes = n * co * es + rows * co * es + B * co * es + rows * co * o_es + B * 8
        emit(dict(case=f"module_{tag}_forward", **verdict(timed({"hip": no_grad(forward("hip")), "torch": no_grad(forward("torch"))}, args.iters,
                                                                args.repeats), 0, args.peak_tbs)))
        emit(dict(case=f"module_{tag}_forward_backward", **verdict(timed({"hip": both("hip"), "torch": both("torch")}, args.iters, args.repeats), 0,
                                                                 args.peak_tbs)))
        U.UPSCALE_BACKEND = "torch"

        # ---- the pieces ----
        t = (rand(n, 3 * s) * 1.5).to(dev, lo).requires_grad_(True)
        freq = (2.0 ** torch.arange(F)).to(dev)
        e_leaves = [t, coord, feat]

        def expand(fn):
            def run():
                with torch.autocast("cuda", dtype=bf16, enabled=autocast):
                    return fn(t, coord, feat, freq, s, GRID, False)
            return run

        hip_e, tor_e = expand(U.expand), expand(R.torch_expand)
        with torch.no_grad():
            a, b = hip_e(), tor_e()
            # (h sits behind sin(2^14 x): compared loosely here, bitwise against pe_concat_layer_norm in tests/test_gpu_upscale.py)
            assert close(a[0], b[0]) and a[1].dtype == b[1].dtype and a[1].shape == b[1].shape
            e_gouts = [rand(*v.shape).to(dev, v.dtype) for v in a]
        del a, b
        emit(dict(case=f"expand_{tag}_forward", **verdict(timed({"hip": no_grad(hip_e), "torch": no_grad(tor_e)}, args.iters, args.repeats),
                                                          expand_bytes, args.peak_tbs)))
        e_bwd_bytes = expand_bytes + rows * 3 * x_es + rows * w * h_es + n * 3 * s * es + n * 3 * 4 + n * c * 4
        emit(dict(case=f"expand_{tag}_forward_backward",
                  **verdict(timed({"hip": lambda: torch.autograd.grad(hip_e(), e_leaves, e_gouts),
                                   "torch": lambda: torch.autograd.grad(tor_e(), e_leaves, e_gouts)}, args.iters, args.repeats), e_bwd_bytes, args.peak_tbs)))

        skip = rand(n, co).to(dev, lo).requires_grad_(True)
        branch = rand(rows, co).to(dev, lo).requires_grad_(True)
        scale = rand(B, co).to(dev, lo).requires_grad_(True)
        m_leaves = [skip, branch, scale]

        def merge(fn):
            def run():
                with torch.autocast("cuda", dtype=bf16, enabled=autocast):
                    return fn(skip, branch, None, scale, offset, s)
            return run

        hip_m, tor_m = merge(U.merge), merge(R.torch_merge)
        with torch.no_grad():
            a, b = hip_m(), tor_m()
            assert close(a, b), float((a.float() - b.float()).abs().max())
            m_gout = rand(*a.shape).to(dev, a.dtype)
        ga, gb = torch.autograd.grad(hip_m(), m_leaves, m_gout), torch.autograd.grad(tor_m(), m_leaves, m_gout)
        r = rel(ga, gb)
        emit(dict(case=f"merge_{tag}_gradients_hip_against_torch_relative_norm", values=[float(f"{v:.3e}") for v in r]))
        assert max(r) <= (0.5 if autocast else 1e-2)      # (torch's bf16 grad_scale is itself a quarter off: tests/test_gpu_upscale.py)
        del a, b, ga, gb
        emit(dict(case=f"merge_{tag}_forward", **verdict(timed({"hip": no_grad(hip_m), "torch": no_grad(tor_m)}, args.iters, args.repeats),
                                                         merge_bytes, args.peak_tbs)))
        m_bwd_bytes = merge_bytes + rows * co * o_es + n * co * es + rows * co * es + B * co * es
        emit(dict(case=f"merge_{tag}_forward_backward",
                  **verdict(timed({"hip": lambda: torch.autograd.grad(hip_m(), m_leaves, m_gout),
                                   "torch": lambda: torch.autograd.grad(tor_m(), m_leaves, m_gout)}, args.iters, args.repeats), m_bwd_bytes, args.peak_tbs)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upscale_bench.json"))
    ap.add_argument("--timeout", type=int, default=240, help="seconds for each mode's child")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--peak-tbs", type=float, default=8.0, help="the HBM rate the byte floor is turned into time with")
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    results = {"shapes": [dict(zip(("parents", "S", "C", "Cout"), sh)) for sh in SHAPES], "F": F, "B": B, "iters": args.iters,
               "repeats": args.repeats, "peak_tbs": args.peak_tbs, "rows": []}
    for mode in MODES:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", mode, "--iters", str(args.iters),
               "--repeats", str(args.repeats), "--peak-tbs", str(args.peak_tbs)]
        proc = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        for line in proc.stdout.splitlines():
            print(line, flush=True)
            if line.startswith("{"):
                results["rows"].append(json.loads(line))
        if proc.returncode:
            print(f"bench_upscale: the {mode} child ended with status {proc.returncode}; nothing more is started", file=sys.stderr)
            return proc.returncode
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
