#!/usr/bin/env python
"""scripts/bench_serattn.py — time of SerializedAttention.forward with the fused gather-attention
(generativedensification_amd.serattn) against the reference's lines on the same GPU in the same process, at the two block
shapes of the base config: N = 12 000 points at C = 160 in 20 heads, and N = 19 200 at C = 256 in 32 heads; patches of 48, B = 1.

  module    a module with SerializedAttention's surface (tests/serattn_ref.py Module) and a point whose tables are cached,
            through serattn.serialized_attention_forward: SERATTN_BACKEND "hip" against "torch".  "torch" runs the reference's
            lines over serialization.patch_tables' tables and the flash_attn drop-in, which is the best path of the parent
            commit.  Forward alone (no_grad), and forward + backward with the gradients of the features and every parameter.
  op        serialized_attention alone against the line it replaces (gather, .half(), the drop-in, cast, gather), on a qkv of the
            mode's dtype: forward alone and forward + backward.

fp32, and bf16 autocast (the trainer's state: float32 parameters).  Operands are random, not zero.  Every pair is compared
before it is timed.  Timing: warm-up, then `--repeats` windows of `--iters` calls per method, alternating; each window lies
between two device events (device time per call) and the host clock is read before the first call and after the last one is
issued (host time per call, no synchronisation inside); microseconds per call, median and range.  `recommend` is "hip" only
where its device median is lower and the two ranges do not overlap.  The parent process never touches the GPU: it starts one
child per mode, each under its own `timeout -k 10`, and relays their output.

Usage: python scripts/bench_serattn.py [--out profiles/serattn_bench.json] [--timeout 240]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((12000, 160, 20), (19200, 256, 32))      # N, C, H
PATCH = 48
MODES = ("fp32", "bf16-autocast")


def window(fn, iters):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    t1 = time.perf_counter()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters, (t1 - t0) * 1e6 / iters


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
            torch.cuda.synchronize()
    res = {}
    for k, v in per.items():
        dev, host = [x[0] for x in v], [x[1] for x in v]
        res[k] = {"median_us": round(statistics.median(dev), 1), "min_us": round(min(dev), 1), "max_us": round(max(dev), 1),
                  "host_median_us": round(statistics.median(host), 1), "host_min_us": round(min(host), 1),
                  "host_max_us": round(max(host), 1)}
    return res


def verdict(times, a="hip", b="torch"):
    """'hip' only where its median is lower and the two ranges over the windows do not overlap"""
    times[f"{b}_over_{a}"] = round(times[b]["median_us"] / times[a]["median_us"], 2)
    times["recommend"] = "hip" if times[a]["median_us"] < times[b]["median_us"] and times[a]["max_us"] < times[b]["min_us"] else "torch"
    return times


def child(args):
    import torch

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import serattn_cases as SC
    import serattn_ref as SR
    from flash_attn import flash_attn_varlen_qkvpacked_func
    from generativedensification_amd import serattn as S

    assert torch.cuda.is_available(), "bench_serattn needs the GPU (no CPU fallback)"
    dev = torch.device("cuda:0")
    bf16 = torch.bfloat16
    mode = args.child
    autocast = mode != "fp32"
    lo = bf16 if autocast else torch.float32

    def emit(row):
        row["mode"] = mode
        print(json.dumps(row), flush=True)

    def rel(xs, ys):
        return [float((s.double() - t.double()).norm()) / max(float(t.double().norm()), 1e-30) for s, t in zip(xs, ys)]

    def no_grad(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    g = torch.Generator().manual_seed(0)
    for n, c, h in SHAPES:
        tag = f"{n}_c{c}_h{h}"
        order, inverse, cu, ser = SC.tables((n,), PATCH, 5)
        order, inverse, cu = order.to(dev), inverse.to(dev), cu.to(dev)

        # ---- the bound forward ----
        torch.manual_seed(1)
        m = SR.Module(c, h, PATCH).to(dev)
        feat = (torch.randn(n, c, generator=g) * 1.5 + 0.3).to(dev).requires_grad_(True)
        point = SR.make_point(feat, (n,), ser)
        S.serialized_attention_forward(m, point)      # caches the tables
        leaves = [feat] + list(m.parameters())

        def forward(backend):
            def run():
                S.SERATTN_BACKEND = backend
                point.feat = feat
                with torch.autocast("cuda", dtype=bf16, enabled=autocast):
                    return S.serialized_attention_forward(m, point).feat
            return run

        gout = None

        def both(backend):
            fwd = forward(backend)

            def run():
                return torch.autograd.grad(fwd(), leaves, gout)
            return run

        with torch.no_grad():
            a, b = forward("hip")(), forward("torch")()
            assert a.dtype == b.dtype and torch.equal(a, b)      # the forward is the same arithmetic
            gout = torch.randn(*a.shape, generator=g).to(dev, a.dtype)
        ga, gb = both("hip")(), both("torch")()
        r = rel(ga, gb)
        emit(dict(case=f"module_{tag}_gradients_hip_against_torch_relative_norm", values=[float(f"{v:.3e}") for v in r]))
        assert max(r) <= (5e-2 if autocast else 1e-2)      # (a sanity bound: the tests hold the bar)
        del a, b, ga, gb
        emit(dict(case=f"module_{tag}_forward", **verdict(timed({"hip": no_grad(forward("hip")), "torch": no_grad(forward("torch"))},
                                                                args.iters, args.repeats))))
        emit(dict(case=f"module_{tag}_forward_backward", **verdict(timed({"hip": both("hip"), "torch": both("torch")}, args.iters,
                                                                         args.repeats))))
        S.SERATTN_BACKEND = "hip"

        # ---- the op ----
        qkv = torch.randn(n, 3 * c, generator=g).to(dev, lo).requires_grad_(True)
        scale = (c // h) ** -0.5

        def hip_op():
            return S.serialized_attention(qkv, order, inverse, cu, h, PATCH, scale)

        def torch_op():
            return flash_attn_varlen_qkvpacked_func(qkv[order].half().reshape(-1, 3, h, c // h), cu, PATCH,
                                                    softmax_scale=scale).reshape(-1, c).to(qkv.dtype)[inverse]

        with torch.no_grad():
            a = hip_op()
            assert torch.equal(a, torch_op())
            og = torch.randn(*a.shape, generator=g).to(dev, a.dtype)
        emit(dict(case=f"op_{tag}_forward", **verdict(timed({"hip": no_grad(hip_op), "torch": no_grad(torch_op)}, args.iters,
                                                            args.repeats))))
        emit(dict(case=f"op_{tag}_forward_backward",
                  **verdict(timed({"hip": lambda: torch.autograd.grad(hip_op(), [qkv], og),
                                   "torch": lambda: torch.autograd.grad(torch_op(), [qkv], og)}, args.iters, args.repeats))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "serattn_bench.json"))
    ap.add_argument("--timeout", type=int, default=240, help="seconds for each mode's child")
    ap.add_argument("--iters", type=int, default=100, help="calls per window (windows of 20 host-bound calls scatter)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    results = {"shapes": [dict(zip(("N", "C", "H"), sh)) for sh in SHAPES], "patch": PATCH, "iters": args.iters,
               "repeats": args.repeats, "rows": []}
    for mode in MODES:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", mode, "--iters",
               str(args.iters), "--repeats", str(args.repeats)]
        proc = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        for line in proc.stdout.splitlines():
            print(line, flush=True)
            if line.startswith("{"):
                results["rows"].append(json.loads(line))
        if proc.returncode:
            print(f"bench_serattn: the {mode} child ended with status {proc.returncode}; nothing more is started", file=sys.stderr)
            return proc.returncode
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
