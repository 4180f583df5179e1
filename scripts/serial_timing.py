#!/usr/bin/env python
"""scripts/serial_timing.py — GPU time of the point serialization at the point decoder's three shapes (12 000, 24 000 and
48 000 points at depths 7, 8, 9; four orders, one segment): `serialize` (encode + sort + inverse), `patch_tables` at P = 48,
and for context a torch composition on the same device — the same word-parallel arithmetic written with torch ops, then
torch.argsort and scatter_ as the reference's Point.serialization does them.  The reference's own Hilbert encoder (one
byte per bit, 2620 aten ops per encode of 12 000 points at depth 8, counted on CPU torch) is not part of this repository
and is not timed here.

The parent process never touches the GPU: it starts one child under a time limit and relays its output.  Per shape and
method: warm-up, then `--repeats` windows of `--iters` calls each, a window timed with device events around the whole
window; the figures are microseconds per call, median and range over the windows.  The composition's codes and (stable)
order are compared with `serialize` before anything is timed.

Usage: python scripts/serial_timing.py [--out FILE.json] [--timeout 300]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((12_000, 7), (24_000, 8), (48_000, 9))
ORDERS = ("z", "z-trans", "hilbert", "hilbert-trans")


def spread3(v):
    x = v & 0x1FFFFF
    x = (x | (x << 32)) & 0x001F00000000FFFF
    x = (x | (x << 16)) & 0x001F0000FF0000FF
    x = (x | (x << 8)) & 0x100F00F00F00F00F
    x = (x | (x << 4)) & 0x10C30C30C30C30C3
    x = (x | (x << 2)) & 0x1249249249249249
    return x


def interleave3(a, b, c):
    return (spread3(a) << 2) | (spread3(b) << 1) | spread3(c)


def hilbert_torch(a, b, c, depth):
    import torch

    q = 1 << (depth - 1)
    while q > 1:
        p = q - 1
        a = torch.where((a & q) != 0, a ^ p, a)
        for other in (0, 1):
            d = c if other else b
            on = (d & q) != 0
            t = torch.where(on, torch.zeros_like(a), (a ^ d) & p)
            a = torch.where(on, a ^ p, a ^ t)
            d = d ^ t
            if other:
                c = d
            else:
                b = d
        q >>= 1
    h = interleave3(a, b, c)
    for s in (1, 2, 4, 8, 16, 32):
        h = h ^ (h >> s)
    return h


def torch_serialize(grid, depth):
    import torch

    x, y, z = grid[:, 0].long(), grid[:, 1].long(), grid[:, 2].long()
    code = torch.stack([interleave3(x, y, z), interleave3(y, x, z), hilbert_torch(x, y, z, depth), hilbert_torch(y, x, z, depth)])
    order = torch.argsort(code)
    inverse = torch.zeros_like(order).scatter_(dim=1, index=order,
                                               src=torch.arange(0, code.shape[1], device=order.device).repeat(code.shape[0], 1))
    return code, order, inverse


def timed(fn, iters, repeats, warmup):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        per_call.append(a.elapsed_time(b) * 1e3 / iters)
    return {"median_us": round(statistics.median(per_call), 2), "min_us": round(min(per_call), 2),
            "max_us": round(max(per_call), 2), "iters": iters, "repeats": repeats}


def child(args):
    import torch

    sys.path.insert(0, ROOT)
    from generativedensification_amd import serialization as S

    assert torch.cuda.is_available(), "serial_timing needs the GPU (no CPU fallback)"
    dev = torch.device("cuda:0")
    results = {"device": torch.cuda.get_device_name(0), "shapes": []}
    for n, depth in SHAPES:
        g = torch.Generator().manual_seed(n)
        grid = torch.randint(0, 1 << depth, (n, 3), generator=g, dtype=torch.int32).to(dev)
        batch = torch.zeros(n, dtype=torch.long, device=dev)
        code, order, inverse = S.serialize(grid, batch, depth, ORDERS, num_segments=1)
        tc, _, _ = torch_serialize(grid, depth)
        assert torch.equal(tc, code), "the torch composition and the kernels disagree on the codes"
        assert torch.equal(torch.argsort(tc, dim=1, stable=True), order), "the stable order differs"
        assert torch.equal(torch.gather(inverse, 1, order), torch.arange(n, device=dev).repeat(4, 1))
        row = {"N": n, "depth": depth, "orders": len(ORDERS)}
        row["serialize"] = timed(lambda: S.serialize(grid, batch, depth, ORDERS, num_segments=1), args.iters, args.repeats, 20)
        row["encode_only"] = timed(lambda: S.encode(grid, batch, depth, "hilbert"), args.iters, args.repeats, 20)
        row["patch_tables_P48"] = timed(lambda: S.patch_tables([n], 48), args.iters, args.repeats, 20)
        off = torch.tensor([n], device=dev)
        row["patch_tables_P48_device_offset"] = timed(lambda: S.patch_tables(off, 48), args.iters, args.repeats, 20)
        row["torch_composition"] = timed(lambda: torch_serialize(grid, depth), max(args.iters // 10, 5), args.repeats, 5)
        print(json.dumps(row), flush=True)
        results["shapes"].append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=7)
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
        print(f"serial_timing: the GPU process did not finish in {args.timeout} s", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
