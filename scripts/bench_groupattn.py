#!/usr/bin/env python
"""scripts/bench_groupattn.py — GPU time of the group cross attention (generativedensification_amd.groupattn) against the torch
path on the same GPU in the same process, at the volume transformer's shapes (embedding 256, 16 heads, cond width 800, batch 3,
a 32^3 volume, 4 views of a 16^3 feature volume):

    n_groups 16   M = 12 288 groups, Lq = 8 queries, Lk = 4 keys, block_size 2
    n_groups 8    M =  1 536 groups, Lq = 64, Lk = 32, block_size 4

  core        group_cross_attention(q, k, v) alone, k and v the halves of one 2E-wide product:
       torch    F.scaled_dot_product_attention on the head views of the same tensors (what nn.MultiheadAttention runs)
       hip      the one launch
  patchify    patchify_layer_norm against the reference's unfold / einsum lines + F.layer_norm
  unpatchify  layer_norm_unpatchify against F.layer_norm + the reference's view / einsum lines
  block       a module with the GroupAttBlock's children (tests/groupattn_ref.py make_group_att_block):
       torch    the module's torch path (tests/groupattn_ref.py torch_forward), which is what the reference runs
       hip      groupattn.group_att_block_forward bound onto the same module

fp32, and bf16 (the core on bf16 tensors; the norms and the block under bf16 autocast, the trainer's state).  Forward alone and
forward + backward (the gradients of the inputs and of every parameter).  Every pair is compared before it is timed.  Timing:
warm-up, then `--repeats` windows of `--iters` calls per method, alternating, each window between two device events;
microseconds per call, median and range, host work included.  The core and norm rows also carry the bytes the call must move
(every input read once, every output written once; the forward + backward row is the sum of both directions) and the share
of the HBM peak (8 TB/s) the fused calls reach with them.  The share is a rate over the CALL's time: it includes host work and
the allocation of the results.  Kernel times come from a profiler run of their own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o core -- python scripts/bench_groupattn.py --child --only core
There is no pass bar.  The parent process never touches the GPU: it starts one child under a time limit and relays its output.

Usage: python scripts/bench_groupattn.py [--out FILE.json] [--timeout 500] [--only core patchify unpatchify block] [--groups 16 8]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, H, COND, BATCH, VOL, FEAT, VIEWS = 256, 16, 800, 3, 32, 16, 4
HBM_PEAK = 8.0e12
PARTS = ("core", "patchify", "unpatchify", "block")


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


def with_share(times, nbytes):
    times["bytes"] = nbytes
    times["hip_share_of_hbm_peak"] = round(nbytes / (times["hip"]["median_us"] * 1e-6) / HBM_PEAK, 3)
    times["torch_over_hip"] = round(times["torch"]["median_us"] / times["hip"]["median_us"], 2)
    return times


def close(a, b, tol):
    return float((a.float() - b.float()).abs().max()) <= tol * float(b.float().abs().max())


def child(args):
    import torch
    import torch.nn.functional as F

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import groupattn_ref as R                # the stand-in module built from tests/golden/groupattn_surface.json
    from generativedensification_amd import groupattn as GA

    assert torch.cuda.is_available(), "bench_groupattn needs the GPU (no CPU fallback)"
    dev = torch.device("cuda:0")
    bf16 = torch.bfloat16
    results = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "repeats": args.repeats, "rows": []}

    def emit(row):
        print(json.dumps(row), flush=True)
        results["rows"].append(row)

    torch.manual_seed(0)
    m = R.make_group_att_block(E, COND, H).to(dev)
    params = tuple(m.parameters())
    scale = (E // H) ** -0.5
    for n_group in args.groups:
        bs, fbs = VOL // n_group, FEAT // n_group
        M, lq, lk = BATCH * n_group ** 3, bs ** 3, fbs ** 3 * VIEWS
        shape = (BATCH, E, VOL, VOL, VOL)
        rows = BATCH * VOL ** 3
        g = torch.Generator().manual_seed(n_group)
        tag0 = {"n_groups": n_group, "M": M, "Lq": lq, "Lk": lk}

        if "core" in args.only:
            for dtype in (torch.float32, bf16):
                es = 4 if dtype == torch.float32 else 2
                q = torch.randn(M, lq, E, generator=g).to(dev, dtype).requires_grad_(True)
                kv = torch.randn(M, lk, 2 * E, generator=g).to(dev, dtype).requires_grad_(True)
                gout = torch.randn(M, lq, E, generator=g).to(dev, dtype)

                def hip():
                    return GA.group_cross_attention(q, kv[..., :E], kv[..., E:], scale, H)

                def sdpa():
                    heads = [t.reshape(M, t.shape[1], H, E // H).transpose(1, 2) for t in (q, kv[..., :E], kv[..., E:])]
                    return F.scaled_dot_product_attention(*heads, scale=scale).transpose(1, 2).reshape(M, lq, E)

                with torch.no_grad():
                    assert close(hip(), sdpa(), 1e-4 if dtype == torch.float32 else 2e-2)
                tag = {**tag0, "dtype": str(dtype).replace("torch.", "")}
                fwd_bytes = es * M * E * (2 * lq + 2 * lk)
                bwd_bytes = es * M * E * (3 * lq + 4 * lk)
                emit({"case": "core_forward", **tag, **with_share(timed({"hip": hip, "torch": sdpa}, args.iters, args.repeats), fwd_bytes)})
                emit({"case": "core_forward_backward", **tag,
                      **with_share(timed({"hip": lambda: torch.autograd.grad(hip(), (q, kv), gout),
                                          "torch": lambda: torch.autograd.grad(sdpa(), (q, kv), gout)}, args.iters, args.repeats),
                                   fwd_bytes + bwd_bytes)})
                del q, kv, gout

        if not {"patchify", "unpatchify", "block"} & set(args.only):
            continue
        # the volume as a block hands it to the next: channels-last (the first block's input is made so by one copy)
        x = torch.randn(shape, generator=g).to(dev).contiguous(memory_format=torch.channels_last_3d).requires_grad_(True)
        cond = torch.randn(M, lk, COND, generator=g).to(dev).requires_grad_(True)
        gvol = torch.randn(shape, generator=g).to(dev).contiguous(memory_format=torch.channels_last_3d)
        for autocast in (False, True):
            cast = bf16 if autocast else None
            tag = {**tag0, "autocast": autocast}
            tol = 5e-2 if autocast else 1e-4

            def amp(fn):
                def run():
                    with torch.autocast("cuda", dtype=bf16, enabled=autocast):
                        return fn()
                return run

            n1, n3 = m.norm1, m.norm3
            if "patchify" in args.only:
                def hip():
                    return GA.patchify_layer_norm(x, bs, n1.weight, n1.bias, n1.eps, out_dtype=cast, patches_dtype=cast)

                def plain():
                    patches = R.patchify_torch(x, bs)
                    return patches, n1(patches)

                with torch.no_grad():
                    a, b = amp(hip)(), amp(plain)()
                    assert torch.equal(a[0], b[0]) and close(a[1], b[1], tol)
                    gp, gn = torch.randn_like(a[0]), torch.randn_like(a[1])
                    tgn = torch.randn_like(b[1])
                es_p, es_n = a[0].element_size(), a[1].element_size()
                fwd_bytes = rows * E * (4 + es_p + es_n)
                bwd_bytes = rows * E * (4 + es_p + es_n + 4)
                ins = (x, n1.weight, n1.bias)
                emit({"case": "patchify_forward", **tag, **with_share(timed({"hip": amp(hip), "torch": amp(plain)}, args.iters, args.repeats), fwd_bytes)})
                emit({"case": "patchify_forward_backward", **tag,
                      **with_share(timed({"hip": lambda: torch.autograd.grad(amp(hip)(), ins, (gp, gn)),
                                          "torch": lambda: torch.autograd.grad(amp(plain)(), ins, (gp, tgn))}, args.iters, args.repeats),
                                   fwd_bytes + bwd_bytes)})
                del a, b, gp, gn, tgn
            if "unpatchify" in args.only:
                with torch.no_grad():
                    patches = R.patchify_torch(x, bs).to(cast or torch.float32).contiguous()
                patches.requires_grad_(True)

                def hip():
                    return GA.layer_norm_unpatchify(patches, shape, bs, n3.weight, n3.bias, n3.eps, out_dtype=cast)

                def plain():
                    return R.unpatchify_torch(n3(patches), shape, bs)

                with torch.no_grad():
                    a, b = amp(hip)(), amp(plain)()
                    assert a.dtype == b.dtype and close(a, b, tol)
                    gv = gvol.to(a.dtype)
                es_p, es_v = patches.element_size(), a.element_size()
                fwd_bytes = rows * E * (es_p + es_v)
                bwd_bytes = rows * E * (es_p + es_v + es_p)
                ins = (patches, n3.weight, n3.bias)
                emit({"case": "unpatchify_forward", **tag, **with_share(timed({"hip": amp(hip), "torch": amp(plain)}, args.iters, args.repeats), fwd_bytes)})
                emit({"case": "unpatchify_forward_backward", **tag,
                      **with_share(timed({"hip": lambda: torch.autograd.grad(amp(hip)(), ins, gv),
                                          "torch": lambda: torch.autograd.grad(amp(plain)(), ins, gv)}, args.iters, args.repeats),
                                   fwd_bytes + bwd_bytes)})
                del a, b, gv, patches
            if "block" in args.only:
                def hip():
                    return GA.group_att_block_forward(m, x, cond, n_group, bs)

                def plain():
                    return R.torch_forward(m, x, cond, n_group, bs)

                with torch.no_grad():
                    a, b = amp(hip)(), amp(plain)()
                    assert a.shape == b.shape and a.dtype == b.dtype and close(a, b, tol)
                    gv = gvol.to(a.dtype)
                    del a, b
                ins = (x, cond) + params
                times = timed({"hip": amp(hip), "torch": amp(plain)}, args.iters, args.repeats)
                times["torch_over_hip"] = round(times["torch"]["median_us"] / times["hip"]["median_us"], 2)
                emit({"case": "block_forward", **tag, **times})
                times = timed({"hip": lambda: torch.autograd.grad(amp(hip)(), ins, gv),
                               "torch": lambda: torch.autograd.grad(amp(plain)(), ins, gv)}, args.iters, args.repeats)
                times["torch_over_hip"] = round(times["torch"]["median_us"] / times["hip"]["median_us"], 2)
                emit({"case": "block_forward_backward", **tag, **times})
        del x, cond, gvol
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=500)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--only", nargs="+", default=list(PARTS), choices=PARTS)
    ap.add_argument("--groups", type=int, nargs="+", default=[16, 8], help="n_groups values (divisors of 16)")
    args = ap.parse_args()
    if args.child:
        child(args)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--iters", str(args.iters), "--repeats", str(args.repeats),
           "--only", *args.only, "--groups", *map(str, args.groups)]
    if args.out:
        cmd += ["--out", args.out]
    try:
        return subprocess.run(cmd, timeout=args.timeout).returncode
    except subprocess.TimeoutExpired:
        print(f"bench_groupattn: the GPU process did not finish in {args.timeout} s", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
