#!/usr/bin/env python
"""scripts/bench_coarsehead.py — GPU time of the fused coarse Gaussian head (generativedensification_amd.coarsehead) against the
reference's lines on the same GPU in the same process, at the reference shape: batch 3, a 64^3 volume of 80-channel rows
(786 432 rows), K 1, sh_dim 12 (23 output columns).

  bound    a module with the Decoder's surface (tests/coarsehead_ref.py make_decoder) with forward_coarse bound to
           decoder_forward_coarse: HEAD_BACKEND "hip" against "torch".  "torch" runs the reference's lines, which is the path of
           the parent commit.  Forward alone, and forward + backward (the gradients of the rows and of the six parameters).
  launches through the C ABI, on buffers of the same sizes: the forward, the backward and the fold launch on their own, with
           the bytes each has to move at least (each operand read once, each result written once; the forward's floor is
           rows x (C x sizeof(dtype) + 4 x 23 K)) and its time over the time of those bytes at --peak-tbs TB/s

fp32, and bf16 autocast (the trainer's state: float32 parameters, bfloat16 rows).  Operands are random, not zero.  Every pair is
compared before it is timed.  Timing: warm-up, then `--repeats` windows of `--iters` calls per method, alternating, each window
between two device events; microseconds per call, median and range.  There is no pass bar.  The parent process never touches
the GPU: it starts one child per mode, each under its own `timeout -k 10`, and relays their output.

Usage: python scripts/bench_coarsehead.py [--out profiles/coarsehead_bench.json] [--timeout 240]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH, VOL, C, K, SH = 3, 64, 80, 1, 12
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


def verdict(times, a="hip", b="torch"):
    """'hip' only where its median is lower and the two ranges over the windows do not overlap"""
    times[f"{b}_over_{a}"] = round(times[b]["median_us"] / times[a]["median_us"], 2)
    times["recommend"] = "hip" if times[a]["median_us"] < times[b]["median_us"] and times[a]["max_us"] < times[b]["min_us"] else "torch"
    return times


def child(args):
    import torch

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import coarsehead_ref as R               # the module built from tests/golden/coarsehead_surface.json
    from generativedensification_amd import _lib as L
    from generativedensification_amd import _marshal as M
    from generativedensification_amd import coarsehead as H

    assert torch.cuda.is_available(), "bench_coarsehead needs the GPU (no CPU fallback)"
    dev = torch.device("cuda:0")
    bf16 = torch.bfloat16
    mode = args.child
    autocast = mode != "fp32"
    dtype = bf16 if autocast else torch.float32
    rows = BATCH * VOL ** 3
    P = SH + 11

    def emit(row):
        row["mode"] = mode
        print(json.dumps(row), flush=True)

    g = torch.Generator().manual_seed(0)
    dec = R.make_decoder(C, K, SH).to(dev)
    with torch.no_grad():
        for lin in (dec.mlp_coarse[0], dec.mlp_coarse[2], dec.mlp_coarse[4]):
            lin.bias.copy_(0.3 * torch.randn(lin.bias.shape, generator=g))
    type(dec).forward_coarse = H.decoder_forward_coarse
    # the rows as deconv3d hands them over: dense, in the autocast dtype under autocast
    x = (torch.randn(BATCH, VOL, VOL, VOL, C, generator=g) * 1.5 + 0.3).to(dev, dtype).requires_grad_(True)
    gouts = [torch.randn(s, generator=g).to(dev) for s in ((BATCH, VOL ** 3 * K, 3), (BATCH, VOL ** 3 * K, SH // 3, 3), (BATCH, VOL ** 3 * K, 3),
                                                             (BATCH, VOL ** 3 * K, 4), (BATCH, VOL ** 3 * K, 1))]
    ins = (x,) + tuple(dec.mlp_coarse.parameters())

    def forward(backend):
        def run():
            H.HEAD_BACKEND = backend
            with torch.autocast("cuda", dtype=bf16, enabled=autocast):
                return dec.forward_coarse(x, OPACITY_SHIFT, SCALING_SHIFT)
        return run

    def both(backend):
        fwd = forward(backend)

        def run():
            return torch.autograd.grad(fwd(), ins, gouts)
        return run

    tol = 5e-2 if autocast else 1e-4
    with torch.no_grad():
        a, b = forward("hip")(), forward("torch")()
        for s, t in zip(a, b):
            assert s.shape == t.shape and float((s - t).abs().max()) <= tol * float(t.abs().max())
        del a, b
    ga, gb = both("hip")(), both("torch")()
    # in the norm, not the maximum: on random rows a unit with a pre-activation next to 0 may be gated differently by the two,
    # and the gradient of that row then differs by a whole term (tests/coarsehead_cases.py settles the gates; this does not)
    # (about 1e-6 of 126 M units flip in fp32, each moving its row's gradient by about a tenth: 1e-3 of the norm)
    rel = [float((s.double() - t.double()).norm()) / float(t.double().norm()) for s, t in zip(ga, gb)]
    emit(dict(case="gradients_hip_against_torch_relative_norm", values=[float(f"{r:.3e}") for r in rel]))
    assert all(s.dtype == t.dtype for s, t in zip(ga, gb)) and max(rel) <= max(4 * tol, 1e-2)
    del ga, gb

    def no_grad(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    emit(dict(case="bound_forward", **verdict(timed({"hip": no_grad(forward("hip")), "torch": no_grad(forward("torch"))}, args.iters, args.repeats))))
    emit(dict(case="bound_forward_backward", **verdict(timed({"hip": both("hip"), "torch": both("torch")}, args.iters, args.repeats))))
    H.HEAD_BACKEND = "hip"

    # ---- the launches on their own ----
    lib, dt, es = L.load(), H._DTYPES[dtype], (2 if autocast else 4)
    params = [t.detach() for t in H._params(dec)]
    xr = x.detach().view(rows, C)
    f32 = dict(dtype=torch.float32, device=dev)
    outs = [torch.empty(rows * K, w, **f32) for w in (3, SH, 3, 4, 1)]
    pws, pbase = H._packed(lib, params[0::2], False, dt, C, K, SH, dev)
    bws, bbase = H._packed(lib, params[0::2], True, dt, C, K, SH, dev)
    ws, base, usable = H._workspace(lib, L.GDR_COARSEHEAD_WS_PARTIALS, dt, rows, C, K, SH, dev)
    grad_x = torch.empty_like(xr)
    grads = [torch.empty_like(t) for t in params]
    flat = [g_.reshape(rows * K, -1) for g_ in gouts]
    bias = [a for b in params[1::2] for a in (b.data_ptr(), H._DTYPES[b.dtype])]

    def fwd_launch():
        L.check(lib.gdr_coarsehead_forward(xr.data_ptr(), dt, pbase, *bias, rows, 1, C, K, SH, OPACITY_SHIFT, SCALING_SHIFT, None, 0.0, 0.0,
                                           *[o.data_ptr() for o in outs], None, None, M.stream()), "gdr_coarsehead_forward")

    def bwd_launch(with_params):
        def run():
            L.check(lib.gdr_coarsehead_backward(xr.data_ptr(), dt, bbase, *bias[:4], rows, C, K, SH, outs[0].data_ptr(),
                                                *[t.data_ptr() for t in flat], None, 0.0, grad_x.data_ptr(), base if with_params else None,
                                                usable if with_params else 0, M.stream()), "gdr_coarsehead_backward")
        return run

    def fold_launch():
        out = [a for i in (0, 1, 2, 3, 4, 5) for a in (grads[i].data_ptr(), H._DTYPES[grads[i].dtype])]
        L.check(lib.gdr_coarsehead_fold(base, usable, dt, rows, C, K, SH, *out, M.stream()), "gdr_coarsehead_fold")

    slabs = min(1024, -(-rows // H.SLAB_MIN))
    part = (2 * C * C + K * P * C + 2 * C + K * P) * (8 if not autocast else 4)
    floors = {"forward": rows * (C * es + 4 * P * K), "backward_x_only": rows * (2 * C * es + 4 * 3 * K + 4 * P * K),
              "backward": rows * (2 * C * es + 4 * 3 * K + 4 * P * K) + slabs * part, "fold": slabs * part}
    fwd_launch()
    times = timed({"forward": fwd_launch, "backward_x_only": bwd_launch(False), "backward": bwd_launch(True), "fold": fold_launch},
                  args.iters, args.repeats)
    for name, t in times.items():
        floor_us = floors[name] / (args.peak_tbs * 1e12) * 1e6
        emit(dict(case="launch_" + name, **t, least_bytes=floors[name], floor_us=round(floor_us, 1),
                  time_over_floor=round(t["median_us"] / floor_us, 2), achieved_tbs=round(floors[name] / t["median_us"] / 1e6, 3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coarsehead_bench.json"))
    ap.add_argument("--timeout", type=int, default=240, help="seconds for each mode's child")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--peak-tbs", type=float, default=8.0, help="the HBM rate the byte floor is turned into time with")
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    results = {"shape": {"batch": BATCH, "volume": VOL, "C": C, "K": K, "sh_dim": SH}, "iters": args.iters, "repeats": args.repeats,
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
            print(f"bench_coarsehead: the {mode} child ended with status {proc.returncode}; nothing more is started", file=sys.stderr)
            return proc.returncode
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
