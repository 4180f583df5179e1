#!/usr/bin/env python
"""scripts/bench_viewattn.py — GPU time of the folded view cross attention (generativedensification_amd.viewattn) against the
torch path on the same GPU in the same process, at the fine decoder's shapes: E = 80, H = 16, Ck = 8, sh = 12,
N = 16 384 / 65 536 / 131 072 / 262 144 points with V = 4 and 2 views.

  forward_fine   a module with the decoder's norm / cross_att / mlp_fine (tests/viewattn_ref.py make_decoder):
       reference   the module's torch path (tests/viewattn_ref.py torch_forward_fine), which is what the reference runs
       hip         viewattn.decoder_forward_fine bound onto the same module
  core           view_attention_pool(t, cond, scale) alone:
       torch       softmax(scale * einsum(t, cond)) and the second einsum, in the same dtypes
       hip         the one launch

fp32, and bf16 autocast (the trainer's state; the core is fp32 in both, so its rows are measured once).  Forward alone and
forward + backward (the gradients of the inputs and of every parameter).  Every pair is compared before it is timed.  Timing:
warm-up, then `--repeats` windows of `--iters` calls per method, alternating, each window between two device events;
microseconds per call, median and range, host work included.  The core rows also carry the bytes the call must move (t and
cond read once, u written once; for the backward grad_out, t and cond read, both gradients written; the forward +
backward row is the sum) and the share of the HBM peak (8 TB/s) the fused calls reach with them.
A shape at which torch's own attention refuses a launch (`HIP error: invalid argument`; any other error ends the run) carries
`reference_error` and the time of the HIP path alone.  The share is a rate over the CALL's time: it includes host work, and
up to N = 131 072 the tensors of a shape (at most 151 MB, reused by every call) fit the 256 MiB Infinity Cache, so only the
N = 262 144 rows say anything about HBM.  Kernel times come from a profiler run of their own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o core -- python scripts/bench_viewattn.py --child --core-only --rows 262144
There is no pass bar.  The parent process never touches the GPU: it starts one child under a time limit and relays its output.

Usage: python scripts/bench_viewattn.py [--out FILE.json] [--timeout 500] [--core-only] [--rows N [N ...]]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = (16_384, 65_536, 131_072, 262_144)
VIEWS = (4, 2)
E, H, CK, SH = 80, 16, 8, 12
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

    sys.path.insert(0, ROOT)
    from generativedensification_amd import viewattn as VA

    assert torch.cuda.is_available(), "bench_viewattn needs the GPU (no CPU fallback)"
    dev = torch.device("cuda:0")
    results = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "repeats": args.repeats, "rows": []}

    def emit(row):
        print(json.dumps(row), flush=True)
        results["rows"].append(row)

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import viewattn_ref as R                # the stand-in module built from tests/golden/viewattn_surface.json

    torch.manual_seed(0)
    m = R.make_decoder(E, SH).to(dev)

    def reference(vol, pts):
        return R.torch_forward_fine(m, vol, pts)

    def bound(vol, pts):
        return VA.decoder_forward_fine(m, vol, pts)

    params = tuple(m.parameters())
    scale = (E // H) ** -0.5

    for n in args.rows:
        for v in VIEWS:
            g = torch.Generator().manual_seed(n + v)
            vol = torch.randn(n, E, generator=g).to(dev).requires_grad_(True)
            pts = torch.randn(n, v, CK, generator=g).to(dev).requires_grad_(True)
            g_feat, g_sh = torch.randn(n, 1, E, generator=g).to(dev), torch.randn(n, 1, SH, generator=g).to(dev)
            for autocast in (() if args.core_only else (False, True)):
                def run(fn):
                    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                        return fn(vol, pts)

                def fb(fn):
                    return torch.autograd.grad(run(fn), (vol, pts) + params, (g_feat, g_sh))

                tag = {"N": n, "V": v, "autocast": autocast}
                with torch.no_grad():
                    a = run(bound)
                    torch.cuda.synchronize()
                    try:                    # (a launch torch's own attention refuses is a result of this comparison, not its end)
                        b = run(reference)
                        torch.cuda.synchronize()
                    except RuntimeError as exc:
                        if "invalid argument" not in str(exc):      # anything but the refused launch ends the run here
                            raise
                        b = None
                        tag["reference_error"] = str(exc).splitlines()[0]
                forward, both = {"hip": lambda: run(bound)}, {"hip": lambda: fb(bound)}
                if b is not None:
                    tol = 1e-1 if autocast else 1e-4          # (of the largest value: a check of sanity, the tests hold the bar)
                    assert a[0].shape == b[0].shape and a[1].shape == b[1].shape and a[0].dtype == b[0].dtype == torch.float32
                    assert all(float((x - y).abs().max()) <= tol * float(y.abs().max()) for x, y in zip(a, b))
                    forward["reference"], both["reference"] = (lambda: run(reference)), (lambda: fb(reference))
                emit({"case": "forward_fine_forward", **tag, **timed(forward, args.iters, args.repeats)})
                emit({"case": "forward_fine_forward_backward", **tag, **timed(both, args.iters, args.repeats)})
            t = (2.0 * torch.randn(n, H, CK, generator=g)).to(dev).requires_grad_(True)
            gout = torch.randn(n, H, CK, generator=g).to(dev)

            def hip():
                return VA.view_attention_pool(t, pts, scale)

            def plain():
                p = torch.softmax(scale * torch.einsum("nhc,nvc->nhv", t, pts), dim=-1)
                return torch.einsum("nhv,nvc->nhc", p, pts)

            with torch.no_grad():
                assert torch.allclose(hip(), plain(), atol=1e-4, rtol=1e-4)
            fwd_bytes = 4 * n * (2 * H * CK + v * CK)
            bwd_bytes = 4 * n * (3 * H * CK + 2 * v * CK)
            emit({"case": "core_forward", "N": n, "V": v, **with_share(timed({"hip": hip, "torch": plain}, args.iters, args.repeats), fwd_bytes)})
            emit({"case": "core_forward_backward", "N": n, "V": v,
                  **with_share(timed({"hip": lambda: torch.autograd.grad(hip(), (t, pts), gout),
                                      "torch": lambda: torch.autograd.grad(plain(), (t, pts), gout)}, args.iters, args.repeats),
                               fwd_bytes + bwd_bytes)})
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
    ap.add_argument("--core-only", action="store_true", help="time view_attention_pool alone")
    ap.add_argument("--rows", type=int, nargs="+", default=list(ROWS))
    args = ap.parse_args()
    if args.child:
        child(args)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--iters", str(args.iters), "--repeats", str(args.repeats), "--rows", *map(str, args.rows)]
    if args.core_only:
        cmd.append("--core-only")
    if args.out:
        cmd += ["--out", args.out]
    try:
        return subprocess.run(cmd, timeout=args.timeout).returncode
    except subprocess.TimeoutExpired:
        print(f"bench_viewattn: the GPU process did not finish in {args.timeout} s", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
