#!/usr/bin/env python
"""scripts/bench_deconv3d.py — GPU time of the fused LayerNorm + 2x transposed convolution (generativedensification_amd.deconv3d)
against the reference's four lines on the same GPU in the same process, at the volume transformer's shape: batch 3, 256
channels, a 32^3 volume stored channels_last_3d (98 304 voxels) -> 64^3 x 80 (786 432 rows).

  tail     the tail of VolTransformer.forward on the same tensors:
       hip        conv_transpose3d_2x_of(deconv, x, norm).permute(0, 2, 3, 4, 1): pack + one forward launch
       torch      the reference's four lines (einsum, LayerNorm, einsum, ConvTranspose3d, einsum + contiguous): what the
                  parent commit ran
  model    a module with VolTransformer's attributes (tests/deconv3d_ref.py make_mirror), 12 blocks with the GroupAttBlock's
           children (tests/groupattn_ref.py) bound to group_att_block_forward with CONV_BACKEND "hip", vol_transformer_forward
           with TAIL_BACKEND "hip" against "torch", n_groups [16]
  launches through the C ABI, on buffers of the same sizes: every entry point on its own, with the bytes it has to move at
           least (each operand read once, each result written once) and the rate that makes of its time

fp32, and bf16 autocast (the trainer's state: float32 parameters, a bfloat16 volume).  Forward alone and forward + backward
(the gradients of the volume and of the four parameters).  Operands are random, not zero.  Every pair is compared before it is
timed.  Timing: warm-up, then `--repeats` windows of `--iters` calls per method, alternating, each window between two device
events; microseconds per call, median and range.  There is no pass bar.  The parent process never touches the GPU: it starts
one child under a time limit and relays its output.

Usage: python scripts/bench_deconv3d.py [--out profiles/deconv3d_bench.json] [--timeout 500] [--only tail model launches]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, OUT, HEADS, COND, BATCH, VOL, FEAT, VIEWS, N_GROUP, LAYERS = 256, 80, 16, 800, 3, 32, 16, 4, 16, 12
PARTS = ("tail", "model", "launches")


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
    import torch

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import deconv3d_ref as R                 # the mirror built from tests/golden/voltransformer_surface.json
    import groupattn_ref as GR               # the blocks' stand-in built from tests/golden/groupattn_surface.json
    from generativedensification_amd import _lib as L
    from generativedensification_amd import _marshal as M
    from generativedensification_amd import deconv3d as D3
    from generativedensification_amd import groupattn as GA

    assert torch.cuda.is_available(), "bench_deconv3d needs the GPU (no CPU fallback)"
    dev = torch.device("cuda:0")
    bf16 = torch.bfloat16
    shape = (BATCH, C, VOL, VOL, VOL)
    rows = BATCH * VOL ** 3
    results = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "repeats": args.repeats, "shape": list(shape), "out_dim": OUT,
               "rows": []}

    def emit(row):
        print(json.dumps(row), flush=True)
        results["rows"].append(row)

    def rows_cl(t):
        return t.permute(0, 2, 3, 4, 1).clone(memory_format=torch.contiguous_format).permute(0, 4, 1, 2, 3)

    g = torch.Generator().manual_seed(0)
    tail = R.make_mirror([], embed_dim=C, vol_low_res=VOL, n_groups=(N_GROUP,), out_dim=OUT).to(dev)
    for mode in ("fp32", "bf16-autocast"):
        autocast = mode != "fp32"
        dtype = bf16 if autocast else torch.float32
        tol = 5e-2 if autocast else 1e-4

        def amp(fn):
            def run():
                with torch.autocast("cuda", dtype=bf16, enabled=autocast):
                    return fn()
            return run

        if "tail" in args.only:
            # the volume as the last bound block hands it over: channels-last, in the autocast dtype under autocast
            x = rows_cl(torch.randn(shape, generator=g).to(dev, dtype)).requires_grad_(True)
            gout = torch.randn(BATCH, 2 * VOL, 2 * VOL, 2 * VOL, OUT, generator=g).to(dev, dtype)

            def four_lines():
                y = tail.norm(torch.einsum('bcdhw->bdhwc', x))
                y = torch.einsum('bdhwc->bcdhw', y)
                return torch.einsum('bcdhw->bdhwc', tail.deconv(y)).contiguous()

            fns = {"hip": amp(lambda: D3.conv_transpose3d_2x_of(tail.deconv, x, tail.norm).permute(0, 2, 3, 4, 1)), "torch": amp(four_lines)}
            with torch.no_grad():
                a, b = (fn() for fn in fns.values())
                assert a.dtype == b.dtype == dtype and a.shape == b.shape and a.is_contiguous() and close(a, b, tol)
                del a, b
            ins = (x,) + tuple(tail.norm.parameters()) + tuple(tail.deconv.parameters())
            for case, run in (("tail_forward", fns),
                              ("tail_forward_backward", {k: (lambda fn=fn: torch.autograd.grad(fn(), ins, gout)) for k, fn in fns.items()})):
                with torch.no_grad() if case == "tail_forward" else torch.enable_grad():
                    emit({"case": case, "mode": mode, **verdict(timed(run, args.iters, args.repeats))})
            del x, gout, fns, run, ins

        if "model" in args.only:
            layers = []
            for i in range(LAYERS):
                blk = GR.make_group_att_block(C, COND, HEADS, seed=i)
                type(blk).forward = GA.group_att_block_forward           # the binding (every stand-in has a class of its own)
                layers.append(blk)
            model = R.make_mirror(layers, embed_dim=C, vol_low_res=VOL, n_groups=(N_GROUP,), out_dim=OUT).to(dev)
            feats = torch.randn(BATCH, VIEWS, COND, FEAT, FEAT, FEAT, generator=g).to(dev)
            gv = torch.randn(BATCH, 2 * VOL, 2 * VOL, 2 * VOL, OUT, generator=g).to(dev, dtype)
            params = tuple(model.parameters())

            def whole(backend):
                def run():
                    saved = GA.CONV_BACKEND, D3.TAIL_BACKEND
                    GA.CONV_BACKEND, D3.TAIL_BACKEND = "hip", backend
                    try:
                        return D3.vol_transformer_forward(model, feats)
                    finally:
                        GA.CONV_BACKEND, D3.TAIL_BACKEND = saved
                return amp(run)

            fns = {"hip": whole("hip"), "torch": whole("torch")}
            iters = max(1, args.iters // 2)
            with torch.no_grad():
                a, b = fns["hip"](), fns["torch"]()
                assert a.shape == b.shape and a.dtype == b.dtype and a.is_contiguous() and close(a, b, tol)
                del a, b
                emit({"case": "model_forward", "mode": mode, **verdict(timed(fns, iters, args.repeats, warmup=1))})
            emit({"case": "model_forward_backward", "mode": mode,
                  **verdict(timed({k: (lambda fn=fn: torch.autograd.grad(fn(), params, gv)) for k, fn in fns.items()}, iters, args.repeats,
                                  warmup=1))})
            del model, layers, feats, gv, params, fns

        if "launches" in args.only:
            lib = L.load()
            dt, f32 = L.GDR_NORM_DTYPES["bf16" if autocast else "f32"], L.GDR_NORM_DTYPES["f32"]
            es = 2 if autocast else 4
            x = torch.randn(rows, C, generator=g).to(dev, dtype)
            gy = torch.randn(8 * rows, OUT, generator=g).to(dev, dtype)
            y, gx = torch.empty_like(gy), torch.empty_like(x)
            w, b, lw, lb = (p.detach() for p in (tail.deconv.weight, tail.deconv.bias, tail.norm.weight, tail.norm.bias))
            gw, gb, glw, glb = (torch.empty_like(p) for p in (w, b, lw, lb))
            packed, packed_t = (torch.empty(8 * C * OUT, dtype=dtype, device=dev) for _ in range(2))
            stats = torch.empty(rows, 2, dtype=torch.float64, device=dev)

            def ws(what):
                return M.workspace(lib.gdr_deconv3d_workspace_bytes(what, dt, rows, C, OUT) + 256, dev)

            ws_w, ws_b, ws_i = ws(L.GDR_DECONV3D_WS_GRAD_WEIGHT), ws(L.GDR_DECONV3D_WS_GRAD_BIAS), ws(L.GDR_DECONV3D_WS_GRAD_INPUT)
            dims = (BATCH, VOL, VOL, VOL, C, OUT)

            def pack():
                L.check(lib.gdr_deconv3d_pack_weight(w.data_ptr(), f32, C, OUT, 0, packed.data_ptr(), dt, M.stream()), "pack")

            def forward():
                L.check(lib.gdr_deconv3d_forward(x.data_ptr(), dt, packed.data_ptr(), b.data_ptr(), f32, 1, lw.data_ptr(), f32, lb.data_ptr(), f32,
                                                 1e-6, *dims, stats.data_ptr(), y.data_ptr(), M.stream()), "forward")

            def forward_no_norm():
                L.check(lib.gdr_deconv3d_forward(x.data_ptr(), dt, packed.data_ptr(), b.data_ptr(), f32, 0, None, f32, None, f32, 0.0, *dims,
                                                 None, y.data_ptr(), M.stream()), "forward")

            def grad_input():
                L.check(lib.gdr_deconv3d_grad_input(gy.data_ptr(), dt, packed_t.data_ptr(), x.data_ptr(), stats.data_ptr(), 1, lw.data_ptr(), f32,
                                                    *dims, ws_i[1], ws_i[2], gx.data_ptr(), glw.data_ptr(), f32, glb.data_ptr(), f32, M.stream()),
                        "grad_input")

            def grad_weight():
                L.check(lib.gdr_deconv3d_grad_weight(x.data_ptr(), stats.data_ptr(), 1, lw.data_ptr(), f32, lb.data_ptr(), f32, gy.data_ptr(), dt,
                                                     *dims, ws_w[1], ws_w[2], gw.data_ptr(), f32, M.stream()), "grad_weight")

            def grad_bias():
                L.check(lib.gdr_deconv3d_grad_bias(gy.data_ptr(), dt, 8 * rows, OUT, ws_b[1], ws_b[2], gb.data_ptr(), f32, M.stream()), "grad_bias")

            L.check(lib.gdr_deconv3d_pack_weight(w.data_ptr(), f32, C, OUT, 1, packed_t.data_ptr(), dt, M.stream()), "pack")
            pack()
            forward()
            xb, yb = rows * C * es, 8 * rows * OUT * es
            least = {"pack": 8 * C * OUT * (4 + es), "forward": xb + yb + rows * 16, "forward_no_norm": xb + yb,
                     "grad_input": yb + 2 * xb + rows * 16, "grad_weight": xb + yb + rows * 16, "grad_bias": yb}
            times = timed({"pack": pack, "forward": forward, "forward_no_norm": forward_no_norm, "grad_input": grad_input,
                           "grad_weight": grad_weight, "grad_bias": grad_bias}, args.iters, args.repeats)
            for k, t in times.items():
                t["least_bytes"] = least[k]
                t["gb_per_s"] = round(least[k] / (t["median_us"] * 1e-6) / 1e9, 1)
            emit({"case": "launches", "mode": mode, **times})
            del x, gy, y, gx, packed, packed_t, stats, ws_w, ws_b, ws_i
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
        print(f"bench_deconv3d: the GPU process did not finish in {args.timeout} s", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
