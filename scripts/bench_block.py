#!/usr/bin/env python
"""scripts/bench_block.py — time of the decoder's Block.forward with the fused residual junctions
(generativedensification_amd.block) against the reference's lines on the same GPU in the same process, at the two block shapes
of the base config: N = 12 000 points at C = 160 in 20 heads, and N = 19 200 at C = 256 in 32 heads; patches of 48, B = 1.

  module     one bound Block (tests/block_ref.py make_block over the spconv drop-in and the bound SerializedAttention, tables
             cached), through block.block_forward: BLOCK_BACKEND "hip" against "torch".  "torch" runs the reference's lines over
             this repository's drop-ins, which is the parent commit's behaviour.  Forward alone (no_grad), and forward +
             backward with the gradients of the features and every parameter.  Both norm kinds: "ln", the plain
             nn.LayerNorm(elementwise_affine=False) that Network builds (the case the default is decided on), and "ada", the
             AdaLayerNorm of AutoEncoder (bound to norm.ada_layer_norm_forward on the torch side, as the parent binds it).
  junctions  the three junctions of that Block alone against the torch lines they replace, on tensors of the dtypes the Block
             hands them in the mode: forward alone and forward + backward.

fp32, and bf16 autocast (the trainer's state: float32 parameters).  Operands are random, not zero; eval mode (drop_path is
the identity, as at the base config's drop_path = 0).  Every pair is compared before it is timed.  Timing: warm-up, then
`--repeats` windows of `--iters` calls per method (`--junction-iters` for the short junctions rows), alternating; each window
lies between two device events (device time per call) and the host clock is read before the first call and after the last one is issued (host time per call, no
synchronisation inside); microseconds per call, median and range.  `recommend` is "hip" only where its device median is lower
and the two ranges do not overlap.  The parent process never touches the GPU: it starts one child per (mode, norm kind), each
under its own `timeout -k 10`, and relays their output.

Usage: python scripts/bench_block.py [--out profiles/block_bench.json] [--timeout 240]
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
KINDS = ("ln", "ada")


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


def sites(n, extent):
    """n distinct voxels of an extent^3 grid as (n, 4) int32 rows (0, c0, c1, c2), from a seeded draw"""
    import numpy as np

    cells = np.random.default_rng(3).choice(extent ** 3, size=n, replace=False)
    return np.stack([np.zeros(n, dtype=np.int64), cells // extent ** 2, cells // extent % extent, cells % extent], 1).astype(np.int32)


def child(args):
    import torch

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import block_ref as BR
    import serattn_cases as SC
    from generativedensification_amd import block as B
    from generativedensification_amd import norm as NM
    from generativedensification_amd import serattn as S
    from generativedensification_amd.sparse_conv import SparseConvTensor

    assert torch.cuda.is_available(), "bench_block needs the GPU (no CPU fallback)"
    dev = torch.device("cuda:0")
    bf16 = torch.bfloat16
    mode, kind = args.child.split(",")
    autocast = mode != "fp32"
    lo = bf16 if autocast else torch.float32

    def emit(row):
        row["mode"], row["norm"] = mode, kind
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
        _, _, _, ser = SC.tables((n,), PATCH, 5)
        m = BR.make_block(c, h, PATCH, norm=kind, conv="hip", seed=1, ada_forward=NM.ada_layer_norm_forward,
                          attn_forward=S.serialized_attention_forward).to(dev)
        m.eval()
        assert B.covers(m)
        feat = (torch.randn(n, c, generator=g) * 1.5 + 0.3).to(dev).requires_grad_(True)
        glob = torch.randn(1, 24, generator=g).to(dev)
        indices = torch.from_numpy(sites(n, 48)).to(dev)
        so = torch.stack([ser.cpu(), torch.arange(n).flip(0)]).to(dev)
        point = BR.Point(feat=feat, offset=torch.tensor([n], dtype=torch.int64, device=dev), global_feat=glob, serialized_order=so,
                         serialized_inverse=torch.argsort(so, dim=1))
        indice_dict = {}
        leaves = [feat] + list(m.parameters())

        def forward(backend):
            def run():
                B.BLOCK_BACKEND = backend
                point.feat = feat
                point.sparse_conv_feat = SparseConvTensor(feat, indices, (48, 48, 48), 1, indice_dict)      # (the conv's table stays cached)
                with torch.autocast("cuda", dtype=bf16, enabled=autocast):
                    return B.block_forward(m, point).feat
            return run

        gout = None

        def both(backend):
            fwd = forward(backend)

            def run():
                return torch.autograd.grad(fwd(), leaves, gout)
            return run

        with torch.no_grad():
            a, b = forward("hip")(), forward("torch")()
            assert a.dtype == b.dtype and a.shape == b.shape
            gout = torch.randn(*a.shape, generator=g).to(dev, a.dtype)
        r = rel([a], [b]) + rel(both("hip")(), both("torch")())
        emit(dict(case=f"module_{tag}_output_and_gradients_hip_against_torch_relative_norm", values=[float(f"{v:.3e}") for v in r]))
        assert max(r) <= (5e-2 if autocast else 1e-2)      # (a sanity bound: the tests hold the bar)
        del a, b
        emit(dict(case=f"module_{tag}_forward", **verdict(timed({"hip": no_grad(forward("hip")), "torch": no_grad(forward("torch"))},
                                                                args.iters, args.repeats))))
        emit(dict(case=f"module_{tag}_forward_backward", **verdict(timed({"hip": both("hip"), "torch": both("torch")}, args.iters,
                                                                         args.repeats))))
        B.BLOCK_BACKEND = "torch"

        # ---- the three junctions alone: skip float32, branches as the Linears hand them over in the mode ----
        off = point.offset
        skip = torch.randn(n, c, generator=g).to(dev).requires_grad_(True)
        branches = [torch.randn(n, c, generator=g).to(dev, lo).requires_grad_(True) for _ in range(3)]
        if kind == "ada":
            scales = [torch.randn(1, c, generator=g).to(dev, lo).requires_grad_(True) for _ in range(3)]
            specs = [("ada", s, 1e-5) for s in scales]
        else:
            scales, specs = [], [("ln", None, None, 1e-5)] * 3
        jleaves = [skip] + branches + scales

        def chain(fn):
            def run():
                with torch.autocast("cuda", dtype=bf16, enabled=autocast):
                    y, n1 = fn(skip, branches[0], None, specs[0], specs[1], off)
                    y, n2 = fn(y, branches[1], None, None, specs[2], off)
                    y, _ = fn(y, branches[2], None, None, None, None)
                return y, n1, n2
            return run

        with torch.no_grad():
            outs = chain(B.junction)()
            r = rel(outs, chain(BR.torch_junction)())
            assert max(r) <= (1e-2 if autocast else 1e-4), r
            gouts = [torch.randn(*o.shape, generator=g).to(dev, o.dtype) for o in outs]
        emit(dict(case=f"junctions_{tag}_forward", **verdict(timed({"hip": no_grad(chain(B.junction)), "torch": no_grad(chain(BR.torch_junction))},
                                                                   args.junction_iters, args.repeats))))
        emit(dict(case=f"junctions_{tag}_forward_backward",
                  **verdict(timed({"hip": lambda: torch.autograd.grad(chain(B.junction)(), jleaves, gouts),
                                   "torch": lambda: torch.autograd.grad(chain(BR.torch_junction)(), jleaves, gouts)}, args.junction_iters,
                                  args.repeats))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_bench.json"))
    ap.add_argument("--timeout", type=int, default=240, help="seconds for each child")
    ap.add_argument("--iters", type=int, default=100, help="calls per window of a module row")
    ap.add_argument("--junction-iters", type=int, default=400, help="calls per window of a junctions row (60-2000 us a call)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    results = {"shapes": [dict(zip(("N", "C", "H"), sh)) for sh in SHAPES], "patch": PATCH, "iters": args.iters,
               "junction_iters": args.junction_iters, "repeats": args.repeats, "rows": []}
    for mode in MODES:
        for kind in KINDS:
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", f"{mode},{kind}",
                   "--iters", str(args.iters), "--junction-iters", str(args.junction_iters), "--repeats", str(args.repeats)]
            proc = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            for line in proc.stdout.splitlines():
                print(line, flush=True)
                if line.startswith("{"):
                    results["rows"].append(json.loads(line))
            if proc.returncode:
                print(f"bench_block: the {mode} / {kind} child ended with status {proc.returncode}; nothing more is started", file=sys.stderr)
                return proc.returncode
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
