#!/usr/bin/env python
"""scripts/bench_pointfeat.py — GPU time of the projected bilinear sampling (generativedensification_amd.pointfeat) against
the torch composition of the same step on the same GPU in the same process: `projection`, two `cat`s, one `einsum` copy,
`F.grid_sample` and the |depth - z| channel for `point_feats`; `projection` and `F.grid_sample` for `sample_views`.

Shapes: `point_feats` at N = 262 144 and N = 100 000 with V = 4 views of 512 x 512; `sample_views` at V = 12, C = 768,
32 x 32 and N = 4096 (the 16^3 feature-volume grid).  Per shape and method: forward alone (under no_grad) and forward +
backward (gradients towards the coarse renders and the points for `point_feats`, as upstream; towards the images only for
`sample_views`, whose grid never needs one).  The two methods are timed alternately, window by window: warm-up, then
`--repeats` windows of `--iters` calls each, a window timed with device events around the whole window; the figures are
microseconds per call, median and range over the windows, host work of the call included.  The forward (max-norm) and the
gradients (L2 norm) of the two methods are compared before anything is timed, and for every gradient the number of elements
that lie further apart than 1e-3 of the tensor's largest magnitude is printed with the result.

The parent process never touches the GPU: it starts one child under a time limit and relays its output.

Usage: python scripts/bench_pointfeat.py [--out FILE.json] [--timeout 500]
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEAT_SHAPES = ((262_144, 4, 512, 512), (100_000, 4, 512, 512))
VIEWS_SHAPES = ((4096, 12, 768, 32, 32),)


def cameras(V, H, W, dev):
    """eyes on a ring of radius 1.9 looking at the origin, ~43 degrees of view: the +-0.5 cube fills most of the image"""
    import torch

    w2cs, ixts = [], []
    for i in range(V):
        a, e = 2 * math.pi * (i + 0.37) / V, 0.4 * math.sin(1.7 * i + 0.4)
        eye = 1.9 * torch.tensor([math.cos(a) * math.cos(e), math.sin(a) * math.cos(e), math.sin(e)])
        fwd = -eye / eye.norm()
        right = torch.linalg.cross(fwd, torch.tensor([0.0, 0.0, 1.0]))
        right = right / right.norm()
        R = torch.stack((right, torch.linalg.cross(fwd, right), fwd))
        m = torch.eye(4)
        m[:3, :3], m[:3, 3] = R, -R @ eye
        f = 0.5 / math.tan(0.375)
        w2cs.append(m)
        ixts.append(torch.tensor([[f * W, 0, W / 2], [0, f * H, H / 2], [0, 0, 1.0]]))
    return torch.stack(w2cs).to(dev), torch.stack(ixts).to(dev)


def torch_projection(points, w2cs, ixts):
    p = points.reshape(1, -1, 3) @ w2cs[:, :3, :3].transpose(1, 2) + w2cs[:, :3, 3][:, None]
    p = p @ ixts.transpose(1, 2)
    return p[..., :2] / p[..., -1:], p[..., -1:]


def torch_point_feats(img_ref, image, acc_map, depth, points, w2cs, ixts):
    """the composition as the call site writes it, ending in the (N, V, 8) layout the cross attention takes"""
    import torch
    import torch.nn.functional as F

    V, n = img_ref.shape[0], points.shape[0]
    h, w = img_ref.shape[-2:]
    xy, z = torch_projection(points, w2cs, ixts)
    xy = (xy + 0.5) / torch.tensor([w, h], device=points.device) * 2 - 1.0
    coarse = torch.cat((image, acc_map.unsqueeze(-1), depth), dim=-1)
    coarse = torch.cat((img_ref, torch.einsum("bhwc->bchw", coarse)), dim=1)
    feats = F.grid_sample(coarse, xy.unsqueeze(1), align_corners=False).view(V, -1, n)
    z_diff = (feats[:, -1:] - z.view(V, -1, n)).abs()
    return torch.einsum("lcb->blc", torch.cat((feats[:, :-1], z_diff), dim=1))


def torch_sample_views(images, points, w2cs, ixts):
    import torch
    import torch.nn.functional as F

    h, w = images.shape[-2:]
    xy, z = torch_projection(points, w2cs, ixts)
    xy = (xy + 0.5) / torch.tensor([w, h], device=points.device) * 2 - 1.0
    return F.grid_sample(images, xy.unsqueeze(1), align_corners=False)[:, :, 0], z[..., 0]


def window(fn, iters):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def timed_pair(fns, iters, repeats, warmup):
    """{name: stats} of several methods timed alternately, window by window"""
    import torch

    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    per = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            per[k].append(window(fn, iters))
    return {k: {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1),
                "iters": iters, "repeats": repeats} for k, v in per.items()}


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def rel_l2(a, b):
    """gradients: |depth - z| and the bilinear weights have kinks, and among 10^6 pairs a few sit on one within f32 rounding
    and fall to different sides in two correct implementations — a max-norm would report those few"""
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def apart(a, b, tol=1e-3):
    """[elements with |a - b| > tol max|b|, all elements]: how localised the difference that rel_l2 lets through is"""
    return [int(((a - b).abs() > tol * b.abs().max()).sum()), a.numel()]


def child(args):
    import torch

    sys.path.insert(0, ROOT)
    from generativedensification_amd import pointfeat as P

    assert torch.cuda.is_available(), "bench_pointfeat needs the GPU (no CPU fallback)"
    dev = torch.device("cuda:0")
    results = {"device": torch.cuda.get_device_name(0), "point_feats": [], "sample_views": []}
    for N, V, H, W in FEAT_SHAPES:
        g = torch.Generator().manual_seed(N)
        w2cs, ixts = cameras(V, H, W, dev)
        img_ref = torch.rand(V, 3, H, W, generator=g).to(dev)
        # the renders in the layout the rasterizer returns: CHW storage behind a permute
        image = torch.rand(V, 3, H, W, generator=g).to(dev).permute(0, 2, 3, 1).requires_grad_(True)
        acc = torch.rand(V, H, W, generator=g).to(dev).requires_grad_(True)
        depth = (1.2 + 1.4 * torch.rand(V, 1, H, W, generator=g)).to(dev).permute(0, 2, 3, 1).requires_grad_(True)
        points = (torch.rand(N, 3, generator=g) - 0.5).to(dev).requires_grad_(True)
        gout = torch.randn(N, V, 8, generator=g).to(dev)
        leaves = (image, acc, depth, points)

        def run(f, backward):
            if not backward:
                with torch.no_grad():
                    return f(img_ref, image, acc, depth, points, w2cs, ixts)
            return torch.autograd.grad(f(img_ref, image, acc, depth, points, w2cs, ixts), leaves, gout)

        out_h, out_t = run(P.point_feats, False), run(torch_point_feats, False)
        g_h, g_t = run(P.point_feats, True), run(torch_point_feats, True)
        row = {"N": N, "V": V, "H": H, "W": W, "rel_diff_forward": rel(out_h, out_t),
               "rel_l2_diff_grads": [rel_l2(a, b) for a, b in zip(g_h, g_t)],
               "rel_max_diff_grads": [rel(a, b) for a, b in zip(g_h, g_t)],
               "grad_elements_apart": [apart(a, b) for a, b in zip(g_h, g_t)]}
        assert row["rel_diff_forward"] < 1e-4 and max(row["rel_l2_diff_grads"]) < 1e-2, row
        row["forward"] = timed_pair({"hip": lambda: run(P.point_feats, False), "torch": lambda: run(torch_point_feats, False)},
                                    args.iters, args.repeats, 10)
        row["forward_backward"] = timed_pair({"hip": lambda: run(P.point_feats, True), "torch": lambda: run(torch_point_feats, True)},
                                             args.iters, args.repeats, 10)
        print(json.dumps(row), flush=True)
        results["point_feats"].append(row)
    for N, V, C, H, W in VIEWS_SHAPES:
        g = torch.Generator().manual_seed(N + C)
        w2cs, ixts = cameras(V, H, W, dev)
        images = torch.randn(V, C, H, W, generator=g).to(dev).requires_grad_(True)
        r = 16
        ax = (torch.arange(r, dtype=torch.float32) + 0.5) / r - 0.5
        points = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), dim=-1).reshape(-1, 3)[:N].to(dev)
        gfeat = torch.randn(V, C, points.shape[0], generator=g).to(dev)

        def run_v(f, backward):
            if not backward:
                with torch.no_grad():
                    return f(images, points, w2cs, ixts)[0]
            return torch.autograd.grad(f(images, points, w2cs, ixts)[0], (images,), gfeat)

        gv_h, gv_t = run_v(P.sample_views, True)[0], run_v(torch_sample_views, True)[0]
        row = {"N": points.shape[0], "V": V, "C": C, "H": H, "W": W,
               "rel_diff_forward": rel(run_v(P.sample_views, False), run_v(torch_sample_views, False)),
               "rel_l2_diff_grads": [rel_l2(gv_h, gv_t)], "rel_max_diff_grads": [rel(gv_h, gv_t)],
               "grad_elements_apart": [apart(gv_h, gv_t)]}
        del gv_h, gv_t
        assert row["rel_diff_forward"] < 1e-4 and row["rel_l2_diff_grads"][0] < 1e-2, row
        row["forward"] = timed_pair({"hip": lambda: run_v(P.sample_views, False), "torch": lambda: run_v(torch_sample_views, False)},
                                    args.iters, args.repeats, 10)
        row["forward_backward"] = timed_pair({"hip": lambda: run_v(P.sample_views, True),
                                              "torch": lambda: run_v(torch_sample_views, True)}, args.iters, args.repeats, 10)
        print(json.dumps(row), flush=True)
        results["sample_views"].append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=500)
    ap.add_argument("--iters", type=int, default=100)
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
        print(f"bench_pointfeat: the GPU process did not finish in {args.timeout} s", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
