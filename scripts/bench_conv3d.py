#!/usr/bin/env python
"""scripts/bench_conv3d.py — GPU time of the channels-last 3x3x3 convolution (generativedensification_amd.conv3d) against torch's
on the same GPU in the same process, at the volume transformer's shape: batch 3, 256 channels, a 32^3 volume stored
channels_last_3d (98 304 voxels), weight (256, 256, 3, 3, 3), no bias.

  conv     the tail of the GroupAttBlock on the same tensors:
       hip        conv3d(vol, w, add_input=True): one pack launch + one product launch
       torch      vol + F.conv3d(vol.contiguous(), w, padding=1): the path group_att_block_forward takes by default
       torch_cl   vol + F.conv3d(vol, w, padding=1): torch's convolution fed the channels-last volume directly (for the record)
     with TFLOP/s = 2 x 27 x Cin x Cout x voxels over the call time (x 3 for forward + backward) and its share of the dense
     peak (157 TFLOP/s f32, 2.5 PFLOP/s bf16).  The rate is over the CALL's time: host work, the pack and the allocation of the
     results are in it.
  block    a module with the GroupAttBlock's children (tests/groupattn_ref.py make_group_att_block), group_att_block_forward
           bound, groupattn.CONV_BACKEND "hip" against "torch", n_groups 16
  parts    through the C ABI, on buffers of the same sizes: the weight pack alone, the whole weight gradient (slab partials
           + fold), the bias gradient.  The fold's own time is a kernel time: see the profiler run below.

fp32, and bf16 autocast (the trainer's state: float32 parameters, a bfloat16 volume).  Forward alone and forward + backward
(the gradients of the volume and of the weight).  Operands are random, not zero.  Every pair is compared before it is timed.
Timing: warm-up, then `--repeats` windows of `--iters` calls per method, alternating, each window between two device events;
microseconds per call, median and range.  Kernel times come from a profiler run of their own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o conv -- python scripts/bench_conv3d.py --child --only conv
There is no pass bar.  The parent process never touches the GPU: it starts one child under a time limit and relays its output.

Usage: python scripts/bench_conv3d.py [--out profiles/conv3d_bench.json] [--timeout 500] [--only conv block parts]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, HEADS, COND, BATCH, VOL, FEAT, VIEWS, N_GROUP = 256, 16, 800, 3, 32, 16, 4, 16
PEAK = {"fp32": 157.3e12, "bf16-autocast": 2.5e15}
PARTS = ("conv", "block", "parts")


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


def close(a, b, tol):
    return float((a.float() - b.float()).abs().max()) <= tol * float(b.float().abs().max())


def child(args):
    import ctypes

    import torch
    import torch.nn.functional as F

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import groupattn_ref as R                # the stand-in module built from tests/golden/groupattn_surface.json
    from generativedensification_amd import _lib as L
    from generativedensification_amd import _marshal as M
    from generativedensification_amd import conv3d as C3
    from generativedensification_amd import groupattn as GA

    assert torch.cuda.is_available(), "bench_conv3d needs the GPU (no CPU fallback)"
    dev = torch.device("cuda:0")
    bf16, cl = torch.bfloat16, torch.channels_last_3d
    shape = (BATCH, C, VOL, VOL, VOL)
    voxels = BATCH * VOL ** 3
    flop = 2.0 * 27 * C * C * voxels
    results = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "repeats": args.repeats, "shape": list(shape), "rows": []}

    def emit(row):
        print(json.dumps(row), flush=True)
        results["rows"].append(row)

    g = torch.Generator().manual_seed(0)
    w = (torch.randn(C, C, 3, 3, 3, generator=g) / (27 * C) ** 0.5).to(dev).requires_grad_(True)
    for mode in ("fp32", "bf16-autocast"):
        autocast = mode != "fp32"
        dtype = bf16 if autocast else torch.float32
        tol = 5e-2 if autocast else 1e-4

        def amp(fn):
            def run():
                with torch.autocast("cuda", dtype=bf16, enabled=autocast):
                    return fn()
            return run

        if "conv" in args.only:
            # the volume as norm3 hands it over: channels-last, in the autocast dtype under autocast
            vol = torch.randn(shape, generator=g).to(dev, dtype).contiguous(memory_format=cl).requires_grad_(True)
            gout = torch.randn(shape, generator=g).to(dev, dtype).contiguous(memory_format=cl)
            fns = {"hip": amp(lambda: C3.conv3d(vol, w, add_input=True)),
                   "torch": amp(lambda: vol + F.conv3d(vol.contiguous(), w, padding=1)),
                   "torch_cl": amp(lambda: vol + F.conv3d(vol, w, padding=1))}
            with torch.no_grad():
                a, b, c = (fn() for fn in fns.values())
                assert a.dtype == b.dtype == dtype and close(a, b, tol) and close(c, b, tol)
                del a, b, c
            for case, mult, run in (("conv_forward", 1, fns),
                                    ("conv_forward_backward", 3, {k: (lambda fn=fn: torch.autograd.grad(fn(), (vol, w), gout)) for k, fn in fns.items()})):
                with torch.no_grad() if mult == 1 else torch.enable_grad():
                    times = verdict(timed(run, args.iters, args.repeats))
                for k in fns:
                    tf = mult * flop / (times[k]["median_us"] * 1e-6)
                    times[k]["tflops"] = round(tf / 1e12, 1)
                    times[k]["share_of_peak"] = round(tf / PEAK[mode], 3)
                emit({"case": case, "mode": mode, **times})
            del vol, gout, fns, run

        if "block" in args.only:
            m = R.make_group_att_block(C, COND, HEADS).to(dev)
            bs, fbs = VOL // N_GROUP, FEAT // N_GROUP
            x = torch.randn(shape, generator=g).to(dev).contiguous(memory_format=cl).requires_grad_(True)
            cond = torch.randn(BATCH * N_GROUP ** 3, fbs ** 3 * VIEWS, COND, generator=g).to(dev).requires_grad_(True)
            gv = torch.randn(shape, generator=g).to(dev, dtype).contiguous(memory_format=cl)
            ins = (x, cond) + tuple(m.parameters())

            def block(backend):
                def run():
                    saved = GA.CONV_BACKEND
                    GA.CONV_BACKEND = backend
                    try:
                        return GA.group_att_block_forward(m, x, cond, N_GROUP, bs)
                    finally:
                        GA.CONV_BACKEND = saved
                return amp(run)

            fns = {"hip": block("hip"), "torch": block("torch")}
            with torch.no_grad():
                a, b = fns["hip"](), fns["torch"]()
                assert a.shape == b.shape and a.dtype == b.dtype and close(a, b, tol)
                del a, b
                emit({"case": "block_forward", "mode": mode, **verdict(timed(fns, args.iters, args.repeats))})
            emit({"case": "block_forward_backward", "mode": mode,
                  **verdict(timed({k: (lambda fn=fn: torch.autograd.grad(fn(), ins, gv)) for k, fn in fns.items()}, args.iters, args.repeats))})
            del m, x, cond, gv, ins, fns

        if "parts" in args.only:
            lib = L.load()
            dt, f32 = L.GDR_NORM_DTYPES["bf16" if autocast else "f32"], L.GDR_NORM_DTYPES["f32"]
            rows = torch.randn(voxels, C, generator=g).to(dev, dtype)
            grows = torch.randn(voxels, C, generator=g).to(dev, dtype)
            packed = torch.empty(27 * C * C, dtype=dtype, device=dev)
            gw, gb = torch.empty_like(w), torch.empty(C, device=dev)
            ws_w = M.workspace(lib.gdr_conv3d_workspace_bytes(L.GDR_CONV3D_WS_GRAD_WEIGHT, dt, voxels, C, C) + 256, dev)
            ws_b = M.workspace(lib.gdr_conv3d_workspace_bytes(L.GDR_CONV3D_WS_GRAD_BIAS, dt, voxels, C, C) + 256, dev)
            wd = w.detach()

            def pack():
                L.check(lib.gdr_conv3d_pack_weight(wd.data_ptr(), f32, C, C, 0, packed.data_ptr(), dt, M.stream()), "pack")

            def grad_weight():
                L.check(lib.gdr_conv3d_grad_weight(rows.data_ptr(), grows.data_ptr(), dt, BATCH, VOL, VOL, VOL, C, C, ws_w[1], ws_w[2],
                                                   gw.data_ptr(), f32, M.stream()), "grad_weight")

            def grad_bias():
                L.check(lib.gdr_conv3d_grad_bias(grows.data_ptr(), dt, voxels, C, ws_b[1], ws_b[2], gb.data_ptr(), f32, M.stream()), "grad_bias")

            emit({"case": "parts", "mode": mode, "workspace_grad_weight_bytes": ws_w[0].numel(),
                  **timed({"pack": pack, "grad_weight": grad_weight, "grad_bias": grad_bias}, args.iters, args.repeats)})
            del rows, grows, packed, gw, gb, ws_w, ws_b
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=500)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--only", nargs="+", default=list(PARTS), choices=PARTS)
    args = ap.parse_args()
    if args.child:
        child(args)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--iters", str(args.iters), "--repeats", str(args.repeats), "--only", *args.only]
    if args.out:
        cmd += ["--out", args.out]
    try:
        return subprocess.run(cmd, timeout=args.timeout).returncode
    except subprocess.TimeoutExpired:
        print(f"bench_conv3d: the GPU process did not finish in {args.timeout} s", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
