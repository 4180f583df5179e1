#!/usr/bin/env python
"""bench.py — views/sec forward+backward @ 800x800 of the Gaussian-splatting render path
(BASELINE.json `metric`), on N GPUs of one node, one rank per GPU.

    python bench.py [--gpus N --steps K --warmup W]

N>1: one rank per GPU over RCCL.  Either launched by `python -m torch.distributed.run --nproc-per-node N ...
bench.py --gpus N` (RANK / LOCAL_RANK / WORLD_SIZE in the environment), or — when WORLD_SIZE is unset — bench.py
re-executes ITSELF under torch.distributed.run with N ranks.  WORLD_SIZE != --gpus is an error, never a silent
one-GPU run.

A "step" = one pass of the hot path over one batch: every view of this rank's shard is
rendered through the reference boundary (`Renderer.render_img` -> `GaussianRasterizer`,
lightning/renderer.py:209-272 semantics) and back-propagated (MSE + 0.1 mean(depth) + 0.1
mean(alpha)) into the Gaussian attributes; per-view losses are all-gathered
(RCCL over xGMI).  Weak scaling: views_per_gpu is fixed, the Gaussians are replicated.

Workload (config.workload):
  c4  (default) BASELINE.json configs[3] per-GPU share: 2M densified-like Gaussians
      (sigma0 = 0.00065), 4 views/GPU at 800x800, SH degree 3 — the configuration the
      metric's target (">= 2M Gaussians ... >= 120 views/s on 1 x MI355X") is quoted on.
  c2  BASELINE.json configs[1]: 200k Gaussians (50/50 sigma0 mix), 4 views 800x800.

Prints ONE JSON line (rank 0) with the contract fields (`metric`, `value`, `unit`,
`higher_is_better`, `dtype`, `ms_per_step`, ...).  Inputs are resident in HBM before the
timed region starts.  A plain run sets up, warms up, times the K steps and prints the line;
everything else is measured only with `--full`: `roofline` (dominant kernel, HIP-event
timed on the launch stream in a second pass of the same K steps), the `per_view` and
`images_out` headlines, the collectives' own times (`comm_ms`), `cpu_baseline` (the
oracle's C restatement on the host cores, bounded sample, rank 0, N=1 only), the PyTorch-CPU
baseline, `psnr_vs_oracle`, `loss_mean` and `grad_l1`.

    --dump-outputs DIR   after the timed steps, what the timed path computed in its last
                         step (per-view losses, the Gaussians' gradients on a fixed seeded
                         sample of rows) as DIR/<name>.npy, for output-by-output comparison
                         of two builds on identical (seeded) inputs
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch
import torch.distributed as dist

K7_SETTLE_STEPS = 13   # untimed steps in front of --warmup: the K7 choice of a launch shape is made after its 12th launch
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6.3 TB/s achievable
ATOMIC_PEAK_LINES = 21.0e9   # float-atomic 64-byte record lines / s the device sustains (measured: scripts/atomic_probe.hip)
DUMP_ROWS = 65_536     # --dump-outputs: rows (Gaussians, pixels) of a larger output kept, a fixed seeded sample
DUMP_LIMIT = 64 * 2**20   # --dump-outputs: bytes written at most


def sample_rows(n, k=DUMP_ROWS, seed=0):
    """Sorted indices of a fixed, seeded sample of k of n rows (all n rows when n <= k)."""
    if n <= k:
        return torch.arange(n)
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:k].sort().values


def dump_outputs(out_dir, arrays):
    """--dump-outputs: every array as out_dir/<name>.npy, float64 where given so and float32 otherwise."""
    import numpy as np

    res = {}
    for name, a in arrays.items():
        a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        res[name] = a.astype(np.float64 if a.dtype == np.float64 else np.float32)
    total = sum(a.nbytes for a in res.values())
    if total > DUMP_LIMIT:
        raise SystemExit(f"bench.py: --dump-outputs would write {total} bytes, more than {DUMP_LIMIT}")
    os.makedirs(out_dir, exist_ok=True)
    for name, a in res.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    print(f"[bench] wrote {len(res)} arrays ({total} bytes) to {out_dir}", file=sys.stderr, flush=True)


def gaussian_outputs(grads, n_rows):
    """The per-Gaussian outputs of a step (gradients, leading dimension n_rows) on a fixed seeded sample of rows, plus
    the sample's row indices (float64: exact)."""
    idx = sample_rows(n_rows)
    out = {"gaussian_rows": idx.double()}
    for name, g in grads.items():
        if g is not None:
            out["grad_" + name] = g.detach().reshape(n_rows, -1)[idx.to(g.device)]
    return out

WORKLOADS = {
    "c4": dict(n=2_000_000, sigma0=(0.00065,), seed=3, views_per_gpu=4, h=800, w=800, deg=3,
               desc="BASELINE configs[3] per-GPU share: 2M densified-like Gaussians, 4 views/GPU 800x800, SH3, fwd+bwd"),
    "c3": dict(n=262_144 + 81_600, sigma0=None, seed=2, views_per_gpu=8, h=512, w=512, deg=1,
               desc="BASELINE configs[2] stand-in: 262144 coarse (sigma0 0.0052) + 81600 fine (0.00065) Gaussians with the "
                    "statistics of network.py's decoder output, 8 views 512x512, SH1 (configs/base.yaml), fwd+bwd"),
    "c2": dict(n=200_000, sigma0=(0.0052, 0.00065), seed=1, views_per_gpu=4, h=800, w=800, deg=3,
               desc="BASELINE configs[1]: 200k Gaussians (50/50 sigma0 mix), 4 views 800x800, SH3, fwd+bwd"),
    "c3step": dict(n=262_144, n_fine=81_600, k_num=12_000, samples=3, sigma0=(0.0052,), seed=2, views_per_gpu=8, v_sel=4,
                   h=512, w=512, deg=1,
                   desc="BASELINE configs[2] call pattern: the reference's train-step render sequence per sample "
                        "(network.py:826-972): 8 coarse renders of 262144 Gaussians -> vjp of the image MSE over 4 views "
                        "w.r.t. the (N,4) carrier + top-k 12000 -> 8 fine renders of 81600 new + the unselected coarse "
                        "Gaussians; B = 3 samples (configs/base.yaml:122), 512x512, SH1; loss on image + image_fine with "
                        "the coarse depth / alpha carrying gradient; ONE backward per step"),
    "c5": dict(n=500_000, sigma0=(0.0052, 0.00065), seed=5, views_per_gpu=4, h=800, w=800, deg=3, surfel=True,
               desc="BASELINE configs[4]: 2DGS surfel path (renderer_2dgs.render_img: image + depth/normal/distortion "
                    "maps), 500k surfels (50/50 sigma0 mix), 4 views 800x800, SH3, fwd+bwd"),
}


def algorithmic_bytes(n, d, p, m, tiles, v=1):
    """Per-kernel ALGORITHMIC HBM bytes per launch (stated in DESIGN.md).
    A = input attribute bytes / Gaussian, S = saved state, G = partial grads, K = key+value."""
    A = 12 + 12 + 16 + 4 + 12 * m
    S, G, K = 75, 52, 12
    R9 = 4 + 48 + 1
    bits = 32 + max(1, math.ceil(math.log2(max(tiles, 2))))
    passes = (bits + 7) // 8
    return dict(
        preprocess_fwd=n * (A + S),
        scan_block_sums=n * 8 // 256,
        duplicate_with_keys=n * 20 + d * K,
        sort_hist=d * 8,                # per pass
        sort_rowscan=0,
        sort_scatter=d * 2 * K,         # per pass
        tile_ranges=d * 8,
        tile_order=tiles * 12,
        # direct tile binning (round 3; replaces duplicate + 2 x (hist, row scan, scatter) + ranges): a counting sort on the
        # tile id straight from the rects.  W = workgroups of the count / scatter kernels = columns of the count matrix
        tile_count=n * 24 + tiles * min(1024, -(-n // 512)) * 4,
        tile_scan=2 * tiles * min(1024, -(-n // 512)) * 4 + tiles * 12,
        tile_scatter=n * 28 + d * 8 + tiles * min(1024, -(-n // 512)) * 4,
        tile_sort=d * (8 + 4),          # (split over the size-class launches by the entries each handles)
        tile_sort_long=0,
        render_fwd=d * 44 + p * 28,
        render_bwd=d * (44 + G) + p * 28,
        # K8+K9 as BUILT: it recomputes the projection from the inputs instead of reading K1's saved state, so per view it
        # reads radius 4 + the 12 used floats of the gradient record 48 + clamp mask 1 (= R9), plus cov3D 24 once; the
        # SURVEY formula n (A + S + G) + n (A + 16) charges S = 75 saved bytes it never reads and sat ABOVE the counters
        # (round-2 verdict).  The path-level figure `_bytes_view` below keeps the SURVEY formula (the contract's).
        preprocess_bwd=n * (A + 24 + R9) + n * (A + 16),
        # multi-view kernels (v views per launch): inputs read once, per-view state v times, outputs written once
        preprocess_fwd_views=n * (A + v * S),
        preprocess_bwd_views=n * (A + 24 + v * R9) + n * (A + 16),
        _passes=passes,
        _bytes_view=n * (A + S) + n * 28 + d * K + d * (8 + passes * 2 * K) + d * 8 + d * 44 + p * 28
        + d * (44 + G) + p * 28 + n * (A + S + G) + n * (A + 16),
    )


def surfel_algorithmic_bytes(n, d, p, m, tiles, v=1):
    """2DGS path: A = 12 + 8 + 16 + 4 + 12 M input bytes / surfel, S = 96-byte render record + depth, rect, tiles,
    clamp (25), G = 20 partial gradients (80), K = key + value; per pixel 15 floats out (image 3, allmap 7, final
    T/M1/M2 3, n_contrib 2) and 15 in (10 gradients + 5 state)."""
    A = 12 + 8 + 16 + 4 + 12 * m
    S, G, K = 96 + 25, 80, 12
    bits = 32 + max(1, math.ceil(math.log2(max(tiles, 2))))
    passes = (bits + 7) // 8
    out = algorithmic_bytes(n, d, p, m, tiles, v)
    R9 = 4 + 80 + 48 + 1   # K9s per view as built: radius, the 20 used floats of the gradient record, Tu/Tv/Tw of the render record, clamp mask
    out.update(preprocess_fwd=n * (A + S), render_fwd=d * (4 + 96) + p * 60, render_bwd=d * (4 + 96 + G) + p * 60,
               preprocess_bwd=n * (A + R9) + n * (A + 16), preprocess_fwd_views=n * (A + v * S),
               preprocess_bwd_views=n * (A + v * R9) + n * (A + 16), _passes=passes)
    out["_bytes_view"] = (out["preprocess_fwd"] + n * 28 + d * K + d * (8 + passes * 2 * K) + d * 8 + out["render_fwd"]
                          + out["render_bwd"] + n * (A + S + 128) + n * (A + 16))   # (path level: the SURVEY-style formula)
    return out


def run_c3step(args, wl, dev, rank, world, use_dist, barrier_fn):
    """The reference's per-sample render sequence as a timed workload (see WORKLOADS["c3step"]); every rank runs its own
    B samples (the reference's own strategy: DDP over scenes, train_lightning.py:71-76).  Reported through the fused entry
    points (`value`) and through the unchanged caller's pattern (`per_view`): renders/s, a render = one view forward +
    backward (the 4 vjp views of a sample count: they are rendered and differentiated)."""
    import gc
    from torch.autograd.functional import vjp
    from generativedensification_amd import _lib as L
    from generativedensification_amd.camera import orbit_cameras
    from generativedensification_amd.renderer import Renderer
    from generativedensification_amd.synthetic import make_scene, make_targets

    B, V, VS, K = wl["samples"], wl["views_per_gpu"], wl["v_sel"], wl["k_num"]
    n, nf, h, w, deg = args.n or wl["n"], wl["n_fine"], wl["h"], wl["w"], wl["deg"]
    keys = ("centers", "shs", "opacity", "scales", "rotations")
    coarse = [make_scene(n, wl["seed"] + 10 * (rank * B + b), sh_degree=deg, sigma0=wl["sigma0"], device=dev, layout=args.layout)
              for b in range(B)]
    fine = [make_scene(nf, wl["seed"] + 10 * (rank * B + b) + 1, sh_degree=deg, sigma0=(0.00065,), device=dev, layout=args.layout)
            for b in range(B)]
    # the decoder's outputs are batched tensors the loops index per sample (network.py:821-836)
    lc = {k: torch.stack([c[k] for c in coarse]).requires_grad_(True) for k in keys}
    lf = {k: torch.stack([f[k] for f in fine]).requires_grad_(True) for k in keys}
    leaves = list(lc.values()) + list(lf.values())
    cams = orbit_cameras(V, w, h, device=dev)
    tg = make_targets(V, h, w, wl["seed"]).to(dev)
    tg_chw = tg.permute(0, 3, 1, 2).contiguous()
    three = ([1.0, 1.0, 1.0], [0.5, 0.5, 0.5], [0.0, 0.0, 0.0])      # dataLoader/gobjverse.py:112-117
    bgs = [torch.tensor(three[j % 3], device=dev) for j in range(V)]
    r_caller = Renderer(sh_degree=deg, fused=False)
    r_fused = Renderer(sh_degree=deg)
    L.load()

    from generativedensification_amd.camera import MiniCam
    batch_cam = [(c.c2w.to(dev), torch.tensor(float(c.FoVy), device=dev), torch.tensor(float(c.FoVx), device=dev),
                  torch.tensor(float(c.znear), device=dev), torch.tensor(float(c.zfar), device=dev)) for c in cams]
    fresh = {"on": not args.prebuilt_cams}

    def cam_of(j):          # network.py:832,851,970: a new MiniCam per render call from the batch's device tensors (utils.py:22-48)
        if not fresh["on"]:
            return cams[j]
        c2w, fy, fx, zn, zf = batch_cam[j]
        return MiniCam(c2w, w, h, fy, fx, zn, zf, dev)

    def caller_step():      # the render sequence of lightning/network.py:813-972 + renderer.py:209-272 (cameras: see cam_of)
        for p in leaves:
            p.grad = None
        total = 0
        for i in range(B):
            centers = lc["centers"][i]
            oc = []
            for j in range(V):
                r_caller.set_bg_color(bgs[j])
                oc.append(r_caller.render_img(cam_of(j), None, centers, lc["shs"][i], lc["opacity"][i], lc["scales"][i],
                                              lc["rotations"][i], dev))

            def fn(ssp):
                fr = []
                for j in range(VS):
                    r_caller.set_bg_color(bgs[j])
                    fr.append(r_caller.render_img(cam_of(j), None, centers, lc["shs"][i], lc["opacity"][i], lc["scales"][i],
                                                  lc["rotations"][i], dev, screenspace_points=ssp))
                return ((torch.stack([f["image"] for f in fr]) - tg[:VS]) ** 2).mean()
            _, grad = vjp(fn, torch.zeros(n, 4, device=dev))
            score = torch.norm(grad[:, 2:4], dim=-1)
            sel = torch.zeros(n, dtype=torch.bool, device=dev)
            sel[torch.topk(score, K, dim=0).indices] = True
            fs = [torch.cat([lf[k][i], lc[k][i][~sel]], dim=0) for k in keys]
            of = []
            for j in range(V):
                r_caller.set_bg_color(bgs[j])
                of.append(r_caller.render_img(cam_of(j), None, *fs, dev, prex="_fine"))
            img_c = torch.cat([o["image"] for o in oc], dim=1)          # views concatenated along the width (network.py:974)
            img_f = torch.cat([o["image_fine"] for o in of], dim=1)
            gt = torch.cat(list(tg), dim=1)
            total = total + ((img_c - gt) ** 2).mean() + ((img_f - gt) ** 2).mean() \
                + 0.1 * torch.cat([o["depth"] for o in oc], dim=1).mean() + 0.1 * torch.cat([o["acc_map"] for o in oc], dim=1).mean()
        total.backward()
        return total.detach()

    def fused_step():       # the same sample through the multi-view entries: 3 nodes per sample instead of 20
        for p in leaves:
            p.grad = None
        total = 0
        for i in range(B):
            a = [lc[k][i] for k in keys]
            lv_c = r_fused.render_views_loss(cams, bgs, tg_chw, *a, dev, w_depth=0.1, w_alpha=0.1)
            _, grad, idx = r_fused.screenspace_absgrad(cams[:VS], bgs[:VS], tg[:VS], *[x.detach() for x in a], dev, topk=K)
            sel = torch.zeros(n, dtype=torch.bool, device=dev)
            sel[idx] = True
            fs = [torch.cat([lf[k][i], lc[k][i][~sel]], dim=0) for k in keys]
            lv_f = r_fused.render_views_loss(cams, bgs, tg_chw, *fs, dev, w_depth=0.0, w_alpha=0.0)
            total = total + (lv_c.sum() + lv_f.sum()) / V
        total.backward()
        return total.detach()

    renders = B * (2 * V + VS) * world

    def timed(fn, k, warm):
        for _ in range(warm):
            fn()
        barrier_fn()
        gc.collect()
        gc.disable()
        t0 = time.perf_counter()
        for _ in range(k):
            last = fn()
        barrier_fn()
        el = time.perf_counter() - t0
        gc.enable()
        if use_dist:
            t = torch.tensor([el], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        return el, float(last)

    el_f, loss_f = timed(fused_step, args.steps, args.warmup)
    if args.dump_outputs and rank == 0:     # the last timed step: its loss and the gradients of both Gaussian sets
        outs = {"loss": torch.tensor([loss_f], dtype=torch.float64)}
        for tag, leaf_set in (("coarse", lc), ("fine", lf)):
            rows = leaf_set["centers"].shape[0] * leaf_set["centers"].shape[1]      # (B samples x N Gaussians)
            outs.update({f"{tag}_{k}": v for k, v in gaussian_outputs({k: p.grad for k, p in leaf_set.items()}, rows).items()})
        dump_outputs(args.dump_outputs, outs)
    k_c = max(1, min(args.steps, 10))
    el_c = loss_c = el_c_prebuilt = None
    if args.full:           # second headline: the unchanged caller's sequence
        el_c, loss_c = timed(caller_step, k_c, max(1, min(args.warmup, 3)))
    if args.full and fresh["on"]:   # the same sequence from cameras built once: what the per-call MiniCam costs the caller
        fresh["on"] = False
        el_c_prebuilt, _ = timed(caller_step, k_c, 2)
        fresh["on"] = True
    kernels = {}
    roofline = None
    if args.full and not args.no_roofline:
        L.profile_enable(True)
        L.profile_collect(reset=True)
        for _ in range(min(args.steps, 3)):
            fused_step()
        torch.cuda.synchronize()
        prof = L.profile_collect(reset=True)
        L.profile_enable(False)
        ks = min(args.steps, 3)
        kernels = {nm: dict(avg_us=round(1e3 * ms / c, 2), launches_per_step=round(c / ks, 1), ms_per_step=round(ms / ks, 3))
                   for nm, (ms, c) in prof.items() if c}
        if kernels:
            # Algorithmic bytes per STEP and kernel: a sample is three nodes over two Gaussian sets — the coarse set (n, V views,
            # loss folded in), the abs-grad pass over it (VS views, K7 producing the (N,4) carrier gradient only, no K9) and the
            # fine set (n_f = n_fine_new + n - k_num, V views) — so one kernel id covers launches of different sizes; the
            # figures below are sums over the step's launches with each set's measured duplicate count
            from generativedensification_amd import rasterizer as R

            def dups(tensors, cs):
                out = []
                with torch.no_grad():
                    e = torch.empty(0, device=dev)
                    for cam in cs:
                        rs = r_caller.set_rasterizer(cam, device=dev).raster_settings
                        out.append(R.forward_raw(tensors[0], tensors[1], e, torch.sigmoid(tensors[2]), torch.exp(tensors[3]),
                                                 torch.nn.functional.normalize(tensors[4]), e, rs)[-2].D)
                return sum(out) / len(out)
            with torch.no_grad():
                a0 = [lc[k][0].detach() for k in keys]
                _, _, idx0 = r_fused.screenspace_absgrad(cams[:VS], bgs[:VS], tg[:VS], *a0, dev, topk=K)
                sel0 = torch.zeros(n, dtype=torch.bool, device=dev)
                sel0[idx0] = True
                f0 = [torch.cat([lf[k][0].detach(), lc[k][0].detach()[~sel0]], dim=0) for k in keys]
            d_c, d_f, n_f = dups(a0, cams), dups(f0, cams), int(f0[0].shape[0])
            tiles, m, P = ((w + 15) // 16) * ((h + 15) // 16), (deg + 1) ** 2, h * w
            ac, af, av = (algorithmic_bytes(n, d_c, P, m, tiles, V), algorithmic_bytes(n_f, d_f, P, m, tiles, V),
                          algorithmic_bytes(n, d_c, P, m, tiles, VS))
            per_view_ids = ("tile_count", "tile_scan", "tile_order", "tile_scatter", "tile_sort", "render_fwd")
            step_bytes = {q: B * ((V + VS) * ac[q] + V * af[q]) for q in per_view_ids}
            step_bytes["preprocess_fwd"] = B * (ac["preprocess_fwd_views"] + av["preprocess_fwd_views"] + af["preprocess_fwd_views"])
            step_bytes["preprocess_bwd"] = B * (ac["preprocess_bwd_views"] + af["preprocess_bwd_views"])
            step_bytes["render_bwd"] = B * (V * ac["render_bwd"] + VS * (d_c * (44 + 16) + P * 20) + V * af["render_bwd"])
            for q, bts in step_bytes.items():
                if q in kernels and kernels[q]["ms_per_step"] > 0:
                    kernels[q]["alg_bytes_per_step"] = int(bts)
                    kernels[q]["alg_GBs"] = round(bts / (kernels[q]["ms_per_step"] * 1e-3) / 1e9, 1)
                    kernels[q]["frac"] = round(kernels[q]["alg_GBs"] / HBM_PEAK_GBS, 4)
            dom = max(kernels, key=lambda q: kernels[q]["ms_per_step"])
            built = sum(q.get("alg_bytes_per_step", 0) for q in kernels.values()) + B * (2 * V) * 64 * (n + n_f) // 2
            roofline = dict(bound="hbm", kernel=dom, peak=HBM_PEAK_GBS, unit="GB/s", achieved=kernels[dom].get("alg_GBs"),
                            frac=kernels[dom].get("frac"), traffic=None, avg_launch_us=kernels[dom]["avg_us"],
                            alg_bytes_per_step=kernels[dom].get("alg_bytes_per_step"),
                            path_bytes_step_built=int(built),
                            path_frac_built=round(built / (el_f / args.steps) / 1e9 / HBM_PEAK_GBS, 4),
                            sets={"coarse": {"n": n, "num_rendered_per_view": int(d_c)},
                                  "fine": {"n": n_f, "num_rendered_per_view": int(d_f)}},
                            note="achieved / frac: the dominant kernel's algorithmic bytes summed over the step's launches "
                                 "(two Gaussian sets, three nodes per sample) over its summed launch time")
    cpu_baseline = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        import numpy as np
        from oracle.gdr_oracle import Oracle, Settings
        cores = os.cpu_count() or 1
        o = Oracle("f32", nthreads=cores)
        cam = cams[0]
        ss = Settings(h, w, math.tan(0.375), math.tan(0.375), np.ones(3, np.float32), 1.0, cam.world_view_transform.cpu().numpy(),
                      cam.full_proj_transform.cpu().numpy(), deg, cam.camera_center.cpu().numpy())
        c0 = {k: lc[k][0].detach().cpu() for k in keys}
        g = np.random.default_rng(0)
        gcol, gdep, galp = (g.standard_normal((3, h, w), dtype=np.float32), g.standard_normal((1, h, w), dtype=np.float32),
                            g.standard_normal((1, h, w), dtype=np.float32))
        t0, reps = time.perf_counter(), 0
        while True:
            ctx = o.forward(c0["centers"].numpy(), torch.sigmoid(c0["opacity"]).numpy(), ss, shs=c0["shs"].numpy(),
                            scales=torch.exp(c0["scales"]).numpy(), rotations=torch.nn.functional.normalize(c0["rotations"]).numpy())
            o.backward(ctx, gcol, gdep, galp)
            reps += 1
            if time.perf_counter() - t0 > 10.0 or reps >= 8:
                break
        tc = (time.perf_counter() - t0) / reps
        cpu_baseline = dict(value=round(1.0 / tc, 4), unit="renders/s", cores=cores, kind="port",
                            sample=f"oracle C restatement (OpenMP, {cores} threads), {reps} x fwd+bwd of 1 coarse view {h}x{w}, "
                                   f"{n} Gaussians ({tc:.3f} s each); a render of the fine set costs about the same")
    v_f = renders * args.steps / el_f
    per_view = None
    if el_c is not None:
        v_c = renders * k_c / el_c
        per_view = {"value": round(v_c, 2), "unit": "renders/s", "ms_per_step": round(1e3 * el_c / k_c, 3),
                    "ms_per_sample": round(1e3 * el_c / k_c / B, 3), "steps": k_c, "of_fused": round(v_c / v_f, 3),
                    "entry": "the unchanged caller: render_img per view (torch activations, new settings + carrier per call), "
                             "torch.autograd.functional.vjp + torch.topk, losses on the width-concatenated views, one backward",
                    "cameras": ("built once (--prebuilt-cams)" if args.prebuilt_cams else
                                "a MiniCam built on the device in front of every render call (network.py:832,851,970 -> utils.py:22-48)"),
                    "value_prebuilt_cams": None if el_c_prebuilt is None else round(renders * k_c / el_c_prebuilt, 2),
                    "ms_per_sample_prebuilt_cams": None if el_c_prebuilt is None else round(1e3 * el_c_prebuilt / k_c / B, 3),
                    "host_boundary": "compiled (csrc/boundary.cpp)" if L.boundary() is not None else "python + ctypes"}
    return {
        "metric": "renders/sec fwd+bwd @ 512x512, reference train-step sequence", "value": round(v_f, 2), "unit": "renders/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * el_f / args.steps, 3),
        "ms_per_sample": round(1e3 * el_f / args.steps / B, 3), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic (seeded random Gaussians with the decoder's statistics, random targets)",
        "config": {"workload": f"c3step: {wl['desc']}", "n_coarse": n, "n_fine_new": nf, "k_num": K, "samples_per_step": B,
                   "renders_per_sample": 2 * V + VS, "image": [h, w], "sh_degree": deg, "layout": args.layout,
                   "parallelism": f"scene-sharded x{world} (the reference's DDP)", "peak_mem_gb": round(torch.cuda.max_memory_allocated(dev) / 2**30, 2),
                   "entry": "render_views_loss (coarse, fine) + screenspace_absgrad(topk) per sample: 3 rasterizer nodes"},
        "per_view": per_view,
        "loss_fused": loss_f, "loss_per_view": loss_c, "roofline": roofline, "cpu_baseline": cpu_baseline, "kernels": kernels,
        "spread": "same box run-to-run +-0.3 %, box-to-box +-4 % (BASELINE.md section 4)",
        "gc": "Python's cyclic collector disabled inside the timed regions (timeit convention; collected right before)",
    }


def run_forward_only(args, wl, dev, rank, world, use_dist, barrier_fn):
    """Evaluation throughput: the reference renders a turntable of ONE Gaussian set under no_grad, one `render_img` per
    frame (/root/reference/evaluation.py:169-193: 120 frames; tools/meshExtractor.py:73-106 does the same for its depth
    maps).  A step = `--eval-views` views of the workload's scene, forward only.  `value` = through `render_views` (chunks of
    <= 8 views per K1 launch, the inputs read once per chunk); `per_view` = the unchanged caller (`render_img` per view with
    torch activations: one native gdr_forward_view / gsr_forward_view call each)."""
    import gc
    from generativedensification_amd import _lib as L
    from generativedensification_amd.camera import orbit_cameras
    from generativedensification_amd.synthetic import make_scene

    n, h, w, deg = args.n or wl["n"], wl["h"], wl["w"], wl["deg"]
    surfel = bool(wl.get("surfel"))
    V = args.eval_views
    if args.workload == "c3" and not args.n:
        a = make_scene(262_144, wl["seed"], sh_degree=deg, sigma0=(0.0052,), device=dev, layout=args.layout)
        b = make_scene(81_600, wl["seed"] + 1, sh_degree=deg, sigma0=(0.00065,), device=dev, layout=args.layout)
        scene = {k: torch.cat([a[k], b[k]]).contiguous() for k in a}
        n = scene["centers"].shape[0]
    else:
        scene = make_scene(n, wl["seed"], sh_degree=deg, sigma0=wl["sigma0"] or (0.0052,), device=dev, layout=args.layout)
    if surfel:
        scene["scales"] = scene["scales"][:, :2].contiguous()
    cams = orbit_cameras(V, w, h, device=dev)
    rays = [None] * V
    if surfel:
        from generativedensification_amd.camera import build_rays
        from generativedensification_amd.renderer_2dgs import Renderer as Rd
        rays = [build_rays(torch.inverse(c.world_view_transform.T.cpu()), 0.75, 0.75, h, w).to(dev) for c in cams]
    else:
        from generativedensification_amd.renderer import Renderer as Rd
    r_fused, r_caller = Rd(sh_degree=deg, white_background=True), Rd(sh_degree=deg, white_background=True, fused=False)
    for r in (r_fused, r_caller):
        r.set_bg_color(torch.ones(3, device=dev))
    a = (scene["centers"], scene["shs"], scene["opacity"], scene["scales"], scene["rotations"], dev)
    L.load()

    def views_step():
        with torch.no_grad():
            acc = 0.0
            for lo in range(0, V, 8):
                cs = cams[lo:lo + 8]
                outs = (r_fused.render_views(cs, rays[lo:lo + 8], None, *a) if surfel else r_fused.render_views(cs, None, *a))
                acc = acc + outs[-1]["image"][0, 0, 0]      # (every frame is consumed, as the video writer does)
            return outs     # (the last chunk's frames: what --dump-outputs writes)

    def caller_step():
        with torch.no_grad():
            acc = 0.0
            for j, cam in enumerate(cams):
                acc = acc + r_caller.render_img(cam, rays[j], *a)["image"][0, 0, 0]
            return acc

    def timed(fn, k, warm):
        for _ in range(warm):
            fn()
        barrier_fn()
        gc.collect()
        gc.disable()
        t0 = time.perf_counter()
        for _ in range(k):
            last = fn()
        barrier_fn()
        el = time.perf_counter() - t0
        gc.enable()
        if use_dist:
            t = torch.tensor([el], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        return el, last

    k = args.steps
    el_v, last_outs = timed(views_step, k, max(1, min(args.warmup, 2)))
    if args.dump_outputs and rank == 0:     # the maps of the last chunk's views in the last timed step, a seeded pixel sample
        px = sample_rows(h * w)
        maps = {f"{key}_last_views": torch.stack([o[key].reshape(h * w, -1)[px.to(dev)] for o in last_outs]) for key in last_outs[0]}
        dump_outputs(args.dump_outputs, dict(maps, pixel_rows=px.double()))
    v_v, per_view = V * k * world / el_v, None
    if args.full:           # second headline: the unchanged caller
        k_c = max(1, min(args.steps, 5))
        el_c, _ = timed(caller_step, k_c, 1)
        v_c = V * k_c * world / el_c
        per_view = {"value": round(v_c, 2), "unit": "views/s", "ms_per_step": round(1e3 * el_c / k_c, 3), "of_fused": round(v_c / v_v, 3),
                    "entry": "the unchanged caller: render_img per frame under no_grad (torch activations, one native forward call)"}
    # per-kernel times of the fused leg and the algorithmic bytes of the forward kernels
    kernels, roofline = {}, None
    if args.full and not args.no_roofline:
        from generativedensification_amd import rasterizer as R
        from generativedensification_amd import surfel_rasterizer as SR
        with torch.no_grad():
            rs = r_caller.set_rasterizer(cams[0], device=dev).raster_settings
            e = torch.empty(0, device=dev)
            st = (SR if surfel else R).forward_raw(scene["centers"], scene["shs"], e, torch.sigmoid(scene["opacity"]),
                                                   torch.exp(scene["scales"]), torch.nn.functional.normalize(scene["rotations"]),
                                                   e, rs)[-2]
            d0 = st.D
            del st
        tiles = ((w + 15) // 16) * ((h + 15) // 16)
        alg = (surfel_algorithmic_bytes if surfel else algorithmic_bytes)(n, d0, h * w, (deg + 1) ** 2, tiles, 8)
        alg["preprocess_fwd"] = alg["preprocess_fwd_views"]
        alg["render_fwd_deep"] = alg["render_fwd"]
        L.profile_enable(True)
        L.profile_collect(reset=True)
        views_step()
        torch.cuda.synchronize()
        prof = L.profile_collect(reset=True)
        L.profile_enable(False)
        for nm, (ms, c) in prof.items():
            if c:
                kk = dict(avg_us=round(1e3 * ms / c, 2), launches=c, total_ms=round(ms, 3))
                if alg.get(nm) and nm not in ("tile_sort_long",):
                    kk["alg_bytes"] = int(alg[nm])
                    kk["frac"] = round(alg[nm] / (kk["avg_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)
                kernels[nm] = kk
        if kernels:
            dom = max(kernels, key=lambda q: kernels[q]["total_ms"])
            ab = kernels[dom].get("alg_bytes", 0)
            built = sum(q["launches"] * q.get("alg_bytes", 0) for q in kernels.values())
            roofline = dict(bound="hbm", kernel=dom, achieved=round(ab / (kernels[dom]["avg_us"] * 1e-6) / 1e9, 1), peak=HBM_PEAK_GBS,
                            unit="GB/s", frac=kernels[dom].get("frac"), traffic=None, alg_bytes_per_launch=ab,
                            avg_launch_us=kernels[dom]["avg_us"], path_bytes_step_built=int(built),
                            path_frac_built=round(built / (el_v / k) / 1e9 / HBM_PEAK_GBS, 4), num_rendered_view0=int(d0))
    cpu_baseline = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        import numpy as np
        from oracle.gdr_oracle import Oracle, Settings
        from oracle.gsr_oracle import SurfelOracle
        cores = os.cpu_count() or 1
        o = (SurfelOracle if surfel else Oracle)("f32", nthreads=cores)
        cam = cams[0]
        ss = Settings(h, w, math.tan(0.375), math.tan(0.375), np.ones(3, np.float32), 1.0, cam.world_view_transform.cpu().numpy(),
                      cam.full_proj_transform.cpu().numpy(), deg, cam.camera_center.cpu().numpy())
        c = {kk: v.cpu() for kk, v in scene.items()}
        op, sc = torch.sigmoid(c["opacity"]).numpy(), torch.exp(c["scales"]).numpy()
        ro = torch.nn.functional.normalize(c["rotations"]).numpy()
        t0, reps = time.perf_counter(), 0
        while True:
            o.forward(c["centers"].numpy(), op, ss, shs=c["shs"].numpy(), scales=sc, rotations=ro)
            reps += 1
            if time.perf_counter() - t0 > 10.0 or reps >= 5:
                break
        tc = (time.perf_counter() - t0) / reps
        cpu_baseline = dict(value=round(1.0 / tc, 4), unit="views/s", cores=cores, kind="port",
                            sample=f"oracle C restatement (OpenMP, {cores} threads), {reps} x forward of 1 view {h}x{w}, all {n} "
                                   f"Gaussians ({tc:.2f} s each)")
    return {
        "metric": f"views/sec forward only (no_grad) @ {h}x{w}", "value": round(v_v, 2), "unit": "views/s", "n_gpus": world,
        "steps": k, "warmup": args.warmup, "ms_per_step": round(1e3 * el_v / k, 3), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic (seeded random Gaussians with the decoder's statistics)",
        "config": {"workload": f"{args.workload} forward-only: {V}-frame turntable of one Gaussian set under no_grad "
                               f"(evaluation.py:169-193), scene of {wl['desc']}", "n_gaussians": n, "views_per_step": V,
                   "image": [h, w], "sh_degree": deg, "layout": args.layout, "parallelism": f"replicas x{world}",
                   "entry": "render_views, <= 8 views per K1 launch, activations fused into K1",
                   "peak_mem_gb": round(torch.cuda.max_memory_allocated(dev) / 2**30, 2)},
        "per_view": per_view, "roofline": roofline, "cpu_baseline": cpu_baseline, "kernels": kernels,
        "gc": "Python's cyclic collector disabled inside the timed regions (timeit convention; collected right before)",
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=13,
                    help="untimed steps (default 13: the library settles on a K7 variant per scene shape after timing launches "
                         "8..11 of the shape, include/gdr.h gdr_k7_tune_get)")
    ap.add_argument("--workload", default="c4", choices=sorted(WORKLOADS))
    ap.add_argument("--n", type=int, default=0, help="override the number of Gaussians")
    ap.add_argument("--views-per-gpu", type=int, default=0)
    ap.add_argument("--grad-allreduce", action="store_true",
                    help="also sum the Gaussian attribute grads over ranks each step (SURVEY §8e)")
    ap.add_argument("--torch-loss", action="store_true",
                    help="take the loss with torch ops on the clamped HWC dicts (default: the fused HIP loss kernel, "
                         "same value and gradients, generativedensification_amd/losses.py)")
    ap.add_argument("--loss-kernels", action="store_true",
                    help="separate fused loss kernels after K6 / before K7 (losses.view_loss_fused) instead of the loss "
                         "folded into K6/K7 (default)")
    ap.add_argument("--stacked-loss", action="store_true",
                    help="take the loss on the view-stacked tensors (measured slower: dim-wise means on strided views)")
    ap.add_argument("--per-view", action="store_true",
                    help="the reference's call pattern as the timed entry: one render_img per view (network.py:827-838), "
                         "the losses summed, ONE backward through all views (the default run reports this pattern as its "
                         "second headline `per_view` anyway)")
    ap.add_argument("--backward-per-view", action="store_true",
                    help="like --per-view but with a backward() after every view (what --per-view meant in rounds 1-2)")
    ap.add_argument("--no-per-view-leg", action="store_true", help="skip the second and third headline (`per_view`, `images_out`)")
    ap.add_argument("--no-settle", action="store_true", help="no K7-settling steps in front of --warmup (A/B of the tuner itself)")
    ap.add_argument("--unfused", action="store_true",
                    help="torch activations before the rasterizer, op for op as lightning/renderer.py:225-230")
    ap.add_argument("--dist-backend", default=None,
                    help="torch.distributed backend (default nccl = RCCL on ROCm; gloo with --single-device, because RCCL "
                         "refuses two ranks on one device)")
    ap.add_argument("--layout", default="cube", choices=["cube", "shell"],
                    help="scene layout: cube = the BASELINE workloads (uniform in the reference's scene cube); shell = "
                         "object-like stand-in with skewed tile lists (not a BASELINE number)")
    ap.add_argument("--order", default="random", choices=["random", "morton"],
                    help="memory order of the Gaussians: random (default, the worst case) or 3D Morton order")
    ap.add_argument("--host-profile", action="store_true",
                    help="cProfile of the host side of the timed steps (top entries to stderr; slows the run)")
    ap.add_argument("--overlap-comm", action="store_true",
                    help="with --grad-allreduce: issue the reduce-scatter + all-gather asynchronously and join them before the "
                         "next step's backward (they overlap the next forward)")
    ap.add_argument("--force-dist", action="store_true",
                    help="initialise torch.distributed even at WORLD_SIZE=1 (exercises the RCCL barrier / all-gather / "
                         "all-reduce calls of the N>1 path on a one-GPU box)")
    ap.add_argument("--single-device", action="store_true",
                    help="developer smoke test of the N>1 code path on a 1-GPU box: every rank uses cuda:0")
    ap.add_argument("--keep-grads", action="store_true",
                    help="with --grad-allreduce: keep the Gaussians' .grad tensors (the views of the persistent packed buffer "
                         "allreduce_gaussian_grads leaves behind) and zero them each step instead of dropping them: autograd then "
                         "accumulates into the buffer (one fill + one read-modify-write of the gradients) instead of the "
                         "one copy_ into the buffer that fresh gradients cost")
    ap.add_argument("--forward-only", action="store_true",
                    help="evaluation throughput (evaluation.py:169-193: a 120-frame turntable of ONE Gaussian set under no_grad): "
                         "views/s through render_img per view and through render_views, no backward")
    ap.add_argument("--eval-views", type=int, default=120)
    ap.add_argument("--image-loss", action="store_true",
                    help="the loss of the reference's fine-stage renders and of its first 1000 iterations "
                         "(lightning/loss.py:35-50): image MSE only, in torch — no gradient reaches depth / alpha / the 2DGS "
                         "maps, and the surfel backward takes the image-only K7s")
    ap.add_argument("--separate-loss-gather", action="store_true",
                    help="with --grad-allreduce: the per-view losses in a collective of their own (rounds 1-5) instead of in the tail "
                         "of the packed gradient buffer (A/B of the one-collective step)")
    ap.add_argument("--prebuilt-cams", action="store_true",
                    help="the unchanged-caller legs (`per_view`, c3step's caller_step, --per-view) render from cameras built once "
                         "instead of building a MiniCam on the device in front of every render call as "
                         "/root/reference/lightning/network.py:832,851,970 do (default: per call, the reference's loop)")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beyond the headline: roofline / per-kernel pass, the per_view and images_out "
                         "headlines, the collectives' own times, the CPU baselines, PSNR vs the oracle, loss_mean / grad_l1 "
                         "(the --no-* options below switch single parts of it off)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path computed in its last step as DIR/<name>.npy "
                         "(float32 / float64, at most 64 MB: a fixed seeded sample of the rows of larger outputs)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--traffic-json", default=os.path.join(ROOT, "profiles", "pmc_traffic.json"),
                    help="per-kernel HBM bytes per launch measured with rocprofv3 --pmc (scripts/gpu_pmc.sh); "
                         "{workload: {kernel: bytes}}; missing file/entry -> traffic null")
    args = ap.parse_args()
    if args.dist_backend is None:
        args.dist_backend = "gloo" if args.single_device else "nccl"

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # not under a launcher: become N ranks (one per GPU; --single-device: N ranks on cuda:0 over gloo)
        import socket
        import subprocess
        sk = socket.socket()
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
        sk.close()
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), "--", os.path.abspath(__file__)] + sys.argv[1:]
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        raise SystemExit(subprocess.call(cmd, env=env))

    # stdout carries exactly ONE line (the JSON result).  Libraries that write to file descriptor 1 from C (RCCL
    # prints a version banner on rank 0 when the first communicator is created) are sent to stderr instead.
    sys.stdout.flush()
    result_fd = os.dup(1)
    os.dup2(2, 1)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: refusing to report a {world}-rank run "
                         f"as a {args.gpus}-GPU number")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a ROCm GPU (no CPU fallback for the product path)")
    if args.single_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    use_dist = world > 1 or args.force_dist
    if args.force_dist:
        os.environ["GDR_FORCE_COLLECTIVES"] = "1"
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29517")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        if args.dist_backend == "nccl":
            try:
                dist.init_process_group("nccl", device_id=dev)  # RCCL over xGMI
            except TypeError:  # older torch: no device_id argument
                dist.init_process_group("nccl")
        else:
            dist.init_process_group(args.dist_backend)
    if use_dist and dist.get_world_size() != args.gpus:
        raise SystemExit(f"bench.py: process group has {dist.get_world_size()} ranks, --gpus {args.gpus}")
    if world > 1 and not args.single_device and torch.cuda.device_count() < world:
        raise SystemExit(f"bench.py: {world} ranks but only {torch.cuda.device_count()} visible GPUs "
                         "(--single-device runs every rank on cuda:0 for a smoke test)")

    from generativedensification_amd import _lib as L
    from generativedensification_amd.camera import orbit_cameras
    from generativedensification_amd.multiview import (allreduce_gaussian_grads, gather_view_losses,
                                                       render_views, shard_views)
    from generativedensification_amd.renderer import Renderer
    from generativedensification_amd.losses import view_loss_fused
    from generativedensification_amd.synthetic import make_scene, make_targets, view_loss, views_loss

    wl = dict(WORKLOADS[args.workload])
    if args.forward_only:
        if args.workload == "c3step":
            raise SystemExit("bench.py: --forward-only applies to the scene workloads (c2, c3, c4, c5)")
        out = run_forward_only(args, wl, dev, rank, world, use_dist, barrier_fn=lambda: (dist.barrier() if use_dist else None,
                                                                                          torch.cuda.synchronize()))
        if rank == 0:
            os.write(result_fd, (json.dumps(out) + "\n").encode())
        if use_dist:
            dist.destroy_process_group()
        return
    if args.workload == "c3step":
        out = run_c3step(args, wl, dev, rank, world, use_dist, barrier_fn=lambda: (dist.barrier() if use_dist else None,
                                                                                    torch.cuda.synchronize()))
        if rank == 0:
            os.write(result_fd, (json.dumps(out) + "\n").encode())
        if use_dist:
            dist.destroy_process_group()
        return
    if args.n:
        wl["n"] = args.n
    if args.views_per_gpu:
        wl["views_per_gpu"] = args.views_per_gpu
    n, h, w, deg, vpg = wl["n"], wl["h"], wl["w"], wl["deg"], wl["views_per_gpu"]
    total_views = vpg * world
    if args.workload == "c3" and not args.n:  # two populations of different size (coarse grid + densified points)
        a = make_scene(262_144, wl["seed"], sh_degree=deg, sigma0=(0.0052,), device=dev, layout=args.layout,
                       order=args.order)
        b = make_scene(81_600, wl["seed"] + 1, sh_degree=deg, sigma0=(0.00065,), device=dev, layout=args.layout,
                       order=args.order)
        scene = {k: torch.cat([a[k], b[k]]).contiguous() for k in a}
    else:
        scene = make_scene(n, wl["seed"], sh_degree=deg, sigma0=wl["sigma0"] or (0.0052,), device=dev,
                           layout=args.layout, order=args.order)
    surfel = bool(wl.get("surfel"))
    if surfel:
        scene["scales"] = scene["scales"][:, :2].contiguous()
    params = {k: v.requires_grad_(True) for k, v in scene.items()}
    all_cams = orbit_cameras(total_views, w, h, device=dev)
    mine = shard_views(total_views, rank, world)
    cams = [all_cams[i] for i in mine]
    targets = make_targets(total_views, h, w, wl["seed"])[list(mine)].to(dev)
    # same strides as the HWC views of the rasterizer's CHW images: elementwise kernels stay on the dense path
    targets_chw = targets.permute(0, 3, 1, 2).contiguous()
    targets = targets_chw.permute(0, 2, 3, 1)
    rays = Renderer2D = surfel_view_loss_fused = surfel_loss = None
    if surfel:
        from generativedensification_amd.camera import build_rays
        from generativedensification_amd.renderer_2dgs import Renderer as Renderer2D
        from generativedensification_amd.losses import surfel_view_loss_fused
        from generativedensification_amd.synthetic import surfel_loss

        renderer = Renderer2D(sh_degree=deg, white_background=True, fused=not args.unfused)
        rays = [build_rays(torch.inverse(c.world_view_transform.T.cpu()), 0.75, 0.75, h, w).to(dev) for c in cams]
    else:
        renderer = Renderer(sh_degree=deg, white_background=True, fused=not args.unfused)
    renderer.set_bg_color(torch.ones(3, device=dev))
    plist = list(params.values())
    L.load()

    # The reference builds its camera in front of EVERY render call (lightning/network.py:832,851,970 ->
    # lightning/utils.py:22-48) from tensors of the batch, which live on the device: torch.inverse(c2w), a CPU projection
    # matrix filled entry by entry from device scalars (four implicit device -> host reads), its upload, a 4x4 matmul; and
    # set_rasterizer's math.tan(FoV / 2) reads two more device scalars (lightning/renderer.py:109-110).  The unchanged-caller
    # legs do the same (round-5 verdict, missing #4) unless --prebuilt-cams; both figures are reported.
    dev_scalars = {}

    def fresh_cam(c):
        from generativedensification_amd.camera import MiniCam
        k = id(c)
        if k not in dev_scalars:     # the batch's tensors: c2w, fovx / fovy, near / far on the device
            dev_scalars[k] = (c.c2w.to(dev), torch.tensor(float(c.FoVy), device=dev), torch.tensor(float(c.FoVx), device=dev),
                              torch.tensor(float(c.znear), device=dev), torch.tensor(float(c.zfar), device=dev))
        c2w, fy, fx, zn, zf = dev_scalars[k]
        return MiniCam(c2w, c.image_width, c.image_height, fy, fx, zn, zf, dev)
    prebuilt_override = {"on": False}

    def make_step(per_view, unfused, torch_loss=False, loss_kernels=False, stacked_loss=False, backward_per_view=False):
        """One pass of the hot path over the rank's views.  per_view: the reference's call pattern — one
        `render_img` per view (lightning/network.py:827-838), the losses summed, ONE backward through all the views'
        graphs (Lightning's loss.backward()); backward_per_view: a backward() after every view instead (round 2's
        `--per-view`).  Otherwise the fused multi-view entry points."""
        rnd = renderer if not unfused or not renderer.fused else (
            Renderer2D(sh_degree=deg, white_background=True, fused=False) if surfel else
            Renderer(sh_degree=deg, white_background=True, fused=False))
        if rnd is not renderer:
            rnd.set_bg_color(torch.ones(3, device=dev))
        a = (params["centers"], params["shs"], params["opacity"], params["scales"], params["rotations"], dev)

        fresh = per_view and not (args.prebuilt_cams or prebuilt_override["on"])

        def step():
            steps_run[0] += 1
            for p in plist:
                if args.keep_grads and p.grad is not None:
                    p.grad.zero_()
                else:
                    p.grad = None
            if per_view:
                losses = []
                for j, cam in enumerate(cams):
                    if fresh:       # network.py:832: a new MiniCam per render call, built on the device from the batch's tensors
                        cam = fresh_cam(cam)
                    out = rnd.render_img(cam, rays[j] if surfel else None, *a)
                    loss = (((out["image"] - targets[j]) ** 2).mean() if args.image_loss
                            else (surfel_loss if surfel else view_loss)(out, targets[j]))
                    if backward_per_view:
                        wait_pending()
                        loss.backward()
                        loss = loss.detach()
                    losses.append(loss)
                losses = torch.stack(losses)
                if not backward_per_view:
                    wait_pending()
                    losses.sum().backward()
                    losses = losses.detach()
            elif args.image_loss:
                outs = (rnd.render_views(cams, rays, None, *a, raw=True) if surfel
                        else render_views(rnd, cams, None, params, dev, raw=True))
                lv = torch.stack([((o["color"] - targets_chw[j]) ** 2).mean() for j, o in enumerate(outs)])
                wait_pending()
                lv.sum().backward()
                losses = lv.detach()
            elif surfel:
                if not (torch_loss or unfused or loss_kernels):
                    # all views of the shard AND their fused loss kernels in one surfel node (the loss kernels of a view
                    # run on its side stream, next to the other views' render kernels; maps never materialised)
                    lv = rnd.render_views_loss(cams, rays, None, targets_chw, *a)
                elif not (torch_loss or unfused):   # one surfel node + one fused-loss autograd node per view
                    outs = rnd.render_views(cams, rays, None, *a, raw=True)
                    lv = torch.stack([surfel_view_loss_fused(o["color"], o["allmap"], rays[j], cams[j].world_view_transform,
                                                             targets_chw[j]) for j, o in enumerate(outs)])
                else:
                    outs = rnd.render_views(cams, rays, None, *a)
                    lv = torch.stack([surfel_loss(o, targets[j]) for j, o in enumerate(outs)])
                wait_pending()
                lv.sum().backward()
                losses = lv.detach()
            else:               # multi-view entry point: all views of the shard in one rasterizer node
                if not (stacked_loss or torch_loss or unfused or loss_kernels):
                    # loss folded into K6's epilogue / K7's prologue: no loss kernels, no dL/dimage tensors
                    lv = rnd.render_views_loss(cams, None, targets_chw, *a)
                elif not (stacked_loss or torch_loss or unfused):
                    outs = render_views(rnd, cams, None, params, dev, raw=True)
                    lv = torch.stack([view_loss_fused(o["color"], o["depth"], o["alpha"], targets_chw[j])
                                      for j, o in enumerate(outs)])
                elif not stacked_loss:
                    outs = render_views(rnd, cams, None, params, dev)
                    lv = torch.stack([view_loss(o, targets[j]) for j, o in enumerate(outs)])
                else:
                    out = render_views(rnd, cams, None, params, dev, stacked=True)
                    lv = views_loss(out, targets)  # (V,) per-view losses on the view-stacked tensors
                wait_pending()
                lv.sum().backward()
                losses = lv.detach()
            ev = None
            if comm_events is not None:     # (the timed collectives of the roofline pass: events on the caller's stream)
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                ev[0].record()
            if args.grad_allreduce and not args.separate_loss_gather:
                # ONE pair of collectives per step (round 6): the V per-view losses ride in the tail of the packed gradient
                # buffer (the reference's DDP issues one bucketed all-reduce per step, train_lightning.py:71-76)
                if ev:
                    ev[1].record()
                h_ = allreduce_gaussian_grads(plist, async_op=bool(args.overlap_comm), view_losses=losses, n_views=total_views)
                if args.overlap_comm:   # RS + AG on the process group's stream, next to the NEXT step's forward; joined before
                    pending_box["h"] = h_                                                 # its backward writes the buffer again
                    all_losses = losses      # (the gathered losses are read where they are logged: h_.losses joins)
                else:
                    all_losses = h_.losses
            else:
                all_losses = gather_view_losses(losses, total_views)
                if ev:
                    ev[1].record()
                if args.grad_allreduce:
                    if args.overlap_comm:
                        pending_box["h"] = allreduce_gaussian_grads(plist, async_op=True)
                    else:
                        allreduce_gaussian_grads(plist)
            if ev:
                ev[2].record()
                comm_events.append(ev)
            return all_losses
        return step

    steps_run = [0]         # steps executed so far, every leg: the timed region's count is read from it, not from --steps
    comm_events = None      # a list while the collectives are being timed
    pending_box: dict = {}

    def wait_pending():
        h = pending_box.pop("h", None)
        if h is not None:
            h.wait()

    step = make_step(args.per_view or args.backward_per_view, args.unfused, args.torch_loss, args.loss_kernels,
                     args.stacked_loss, args.backward_per_view)

    def barrier():
        wait_pending()
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    # The library settles on a K7 variant per launch shape with ONE timed round (launches 8..11 of the shape, include/gdr.h
    # gdr_k7_tune_get) and keeps it: that round runs here, before the W warm-up steps, whatever --warmup says — so every
    # timed step runs the chosen kernel (round-4 verdict: with --warmup 5 the round fell inside the timed region).
    settle = 0 if args.no_settle else K7_SETTLE_STEPS
    for _ in range(settle):
        step()
    for _ in range(args.warmup):
        step()
    barrier()
    # Python's cyclic collector is off inside the timed regions (the `timeit` convention): one generation-2 pass over this
    # process's ~170 k objects takes 35 ms — 10 steps of the C4 workload — and whether one lands in a 30-60 ms timed region
    # is chance (measured: the same per-view run 790 or 1380 views/s).  Collected right before, re-enabled right after.
    import gc
    gc.collect()
    gc.disable()
    prof_host = None
    if args.host_profile:
        import cProfile
        prof_host = cProfile.Profile()
        prof_host.enable()
    n_before = steps_run[0]
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last_losses = step()
    barrier()
    elapsed = time.perf_counter() - t0
    timed_steps = steps_run[0] - n_before
    gc.enable()
    if prof_host is not None:
        import io
        import pstats
        prof_host.disable()
        buf = io.StringIO()
        pstats.Stats(prof_host, stream=buf).sort_stats("tottime").print_stats(40)
        print(buf.getvalue(), file=sys.stderr)
    rank_ms = None
    if use_dist:     # the slowest rank is the job's time; every rank's own time is reported so that a straggler shows
        mine_t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        all_t = [torch.zeros_like(mine_t) for _ in range(dist.get_world_size())]
        dist.all_gather(all_t, mine_t)
        per_rank = [float(x.item()) for x in all_t]
        elapsed = max(per_rank)
        rank_ms = [round(1e3 * x / timed_steps, 3) for x in per_rank]
    views_per_sec = total_views * timed_steps / elapsed
    ms_per_step = 1e3 * elapsed / timed_steps

    def note(msg):
        if rank == 0:
            print(f"[bench] {msg} (t+{time.perf_counter() - t0:.1f}s)", file=sys.stderr, flush=True)

    note(f"timed region done: {views_per_sec:.1f} views/s")
    # ---- what the last timed step computed: the per-view losses and the Gaussians' gradients (a seeded sample of rows)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, dict(gaussian_outputs({k: p.grad for k, p in params.items()}, n),
                                             view_losses=last_losses))
    # ---- the collectives on their own (HIP events around each, a short extra pass; inside `value` they are part of the step)
    comm_ms = None
    if use_dist and args.full:
        comm_events = []
        for _ in range(max(1, min(args.steps, 5))):
            step()
        torch.cuda.synchronize()
        k_ev = len(comm_events)
        ones = torch.ones(1, device=dev)
        dist.all_reduce(ones)                     # how many ranks the collectives really span (1 per process of the group)
        G_, B_ = dist.get_world_size(), sum(p.numel() * p.element_size() for p in plist)
        link = 153e9                              # one xGMI link, one direction (MI355X_MICROARCH.md: 7 links x ~153 GB/s per GPU)
        comm_ms = dict(ranks_seen=int(ones.item()), backend=dist.get_backend(),     # ("nccl" = RCCL over xGMI; "gloo" = the CPU test backend)
                       grad_bytes=B_, overlap=bool(args.overlap_comm),
                       expected_grad_allreduce_ms=(None if G_ < 2 else dict(
                           direct_all_links=round(2e3 * (B_ / G_) / link, 3), ring_one_link=round(2e3 * B_ * (G_ - 1) / G_ / link, 3),
                           note="reduce-scatter + all-gather of the packed gradients over xGMI: every peer pair moves 1/G of the "
                                "buffer per phase when all 7 point-to-point links carry traffic at once; a ring is bound by one link")),
                       collectives_per_step=(2 if args.grad_allreduce and not args.separate_loss_gather else
                                             (3 if args.grad_allreduce else 1)),
                       losses=("in the tail of the packed gradient buffer: no collective of their own" if args.grad_allreduce and
                               not args.separate_loss_gather else "all-gather of V floats"),
                       loss_gather=round(sum(e[0].elapsed_time(e[1]) for e in comm_events) / k_ev, 4),
                       grad_allreduce=(round(sum(e[1].elapsed_time(e[2]) for e in comm_events) / k_ev, 4) if args.grad_allreduce else None),
                       grads="kept (zeroed each step: autograd accumulates into the packed buffer)" if args.keep_grads
                       else "dropped each step; from the second step on K9 writes them straight into the packed buffer (gradient sinks, "
                            "rasterizer.register_grad_sink): no copy in front of the collectives",
                       note="ms per step on this rank, HIP events on the caller's stream around gather_view_losses / "
                            "allreduce_gaussian_grads (packing included); rank 0")
        comm_events = None
    # ---- D (num_rendered) per view, measured (--full: one more forward per view) ---------------------
    from generativedensification_amd import rasterizer as R
    from generativedensification_amd import surfel_rasterizer as SR
    d_views, pair_views, class_entries = [], [], [0, 0, 0]
    with torch.no_grad():
        for cam in (cams if args.full else ()):
            rs = renderer.set_rasterizer(cam, device=dev).raster_settings
            e = torch.empty(0, device=dev)
            fr = (SR if surfel else R).forward_raw(params["centers"].detach(), params["shs"].detach(), e,
                                                   torch.sigmoid(params["opacity"].detach()),
                                                   torch.exp(params["scales"].detach()),
                                                   torch.nn.functional.normalize(params["rotations"].detach()), e, rs)
            st = fr[-2]
            d_views.append(st.D)
            # pixel-Gaussian evaluations of the reference algorithm for this view: every pixel walks its tile's list up to
            # its last contributor -> sum of n_contrib; the backward walks the same entries again
            try:
                tt = st.tensors()
                nc = tt["n_contrib"]
                pair_views.append(int((nc if nc.dim() == 2 else nc.reshape(-1, h, w)[0]).long().sum()))
                ll = (tt["ranges"][:, 1].long() - tt["ranges"][:, 0].long()).clamp_min(0)
                for c, (lo_, hi_) in enumerate(((0, 2048), (2048, 4096), (4096, 1 << 40))):   # the tile sort's size classes
                    class_entries[c] += int(ll[(ll > lo_) & (ll <= hi_)].sum())
            except Exception:
                pass
            del st, fr
    d_mean = sum(d_views) / max(1, len(d_views))
    tiles = ((w + 15) // 16) * ((h + 15) // 16)
    m = (deg + 1) ** 2
    alg = (surfel_algorithmic_bytes if surfel else algorithmic_bytes)(n, d_mean, h * w, m, tiles, min(vpg, 8))
    # the deep forward takes the cut tiles of an object-like scene (nearly every pair where it runs at all): K6's bytes
    alg["render_fwd_deep"] = alg["render_fwd"]
    if sum(class_entries):   # the tile sort's D * 24 bytes split over its launches by the entries each size class handles:
        # `tile_sort` = the <= 2048-entry class (one launch per view), `tile_sort_long` = the medium + long class launches
        alg["tile_sort"] = class_entries[0] / len(d_views) * 12
        # bytes PER VIEW of the medium + long class launches; per launch = this x views / launches of the step (one launch of
        # the medium class per view, one of the long class where the shape's recent calls saw lists beyond 4096 entries)
        alg["_tile_sort_long_view"] = (class_entries[1] + class_entries[2]) / len(d_views) * 12
        alg["tile_sort_long"] = alg["_tile_sort_long_view"]

    # ---- roofline: per-kernel HIP-event timing, second pass of the same K steps -----------
    roofline = None
    k7_variant = None
    kernels = {}

    def profiled(fn, k):
        L.profile_enable(True)
        L.profile_collect(reset=True)
        for _ in range(k):
            fn()
        torch.cuda.synchronize()
        prof = L.profile_collect(reset=True)
        L.profile_enable(False)
        return prof

    if args.full and not args.no_roofline:
        prof = profiled(step, args.steps)
        # PMC tables (rocprofv3 --pmc passes, scripts/gpu_pmc.sh -> scripts/make_pmc_traffic.py) hold for ONE scene: the
        # figures are used only when the table's recorded scene is the one being run; otherwise traffic is null and no
        # measured path fraction is printed (round 2 printed 1.135 for a 0.5 M scene against the 2 M table)
        try:
            pmc = json.load(open(args.traffic_json))
        except Exception:
            pmc = {}
        meta = pmc.get(args.workload + "_meta", {})
        pmc_ok = (meta.get("n") == n and meta.get("layout", "cube") == args.layout and meta.get("order", "random") == args.order
                  and meta.get("views_per_gpu") == vpg and meta.get("abi") == L.ABI_VERSION
                  and not (args.per_view or args.backward_per_view or args.unfused or args.image_loss))
        tj, vj = (pmc.get(args.workload, {}), pmc.get(args.workload + "_valu", {})) if pmc_ok else ({}, {})
        # which K7 the library settled on for this shape (include/gdr.h gdr_k7_tune_get: rows, or row pairs where they pay)
        k7_variant = None
        if True:
            import ctypes as _C
            ch, u0, u1 = _C.c_int32(0), _C.c_float(0), _C.c_float(0)
            for kind in ((3,) if surfel else (1, 0, 2)):
                if L.load().gdr_k7_tune_get(n, h, w, min(vpg, 8), kind, _C.byref(ch), _C.byref(u0), _C.byref(u1)) == 0:
                    rd, us4 = _C.c_int32(0), (_C.c_float * 4)()
                    L.load().gdr_k7_tune_get_rounds(n, h, w, min(vpg, 8), kind, None, _C.byref(rd), us4)
                    k7_variant = dict(chosen={1: "pairs", 0: "rows"}.get(ch.value, "undecided (rows so far)"),
                                      us_rows=round(u0.value, 1), us_pairs=round(u1.value, 1),
                                      rounds_done=rd.value,
                                      confirmation=(dict(us_rows=round(us4[2], 1), us_pairs=round(us4[3], 1)) if rd.value >= 2 else
                                                    "at launches 64..67 of the shape (not reached in this run)"),
                                      timed_steps_on_chosen=(args.steps if ch.value >= 0 and (settle or args.warmup >= 13) else None),
                                      settle_steps=settle,
                                      note="render_bwd_kernel (one record line per 4x4 block) or render_bwd_pairs_kernel (8x4 where "
                                           "that saves lines): one timed round per launch shape (its launches 8..11, here inside the "
                                           "settle steps in front of --warmup), the faster serves; ONE confirmation round at launches "
                                           "64..67 overturns it only if it loses by > 5 %, then the choice is final; GDR_K7_PAIRS=0/1 pins it")
                    break
        aj = pmc.get(args.workload + "_atomic", {}) if pmc_ok else {}

        def pmc_name(name):   # bench kernel id -> kernel symbol in the rocprofv3 summaries
            if name == "render_bwd" and k7_variant and k7_variant["chosen"] == "pairs":
                pk = ("surfel_" if surfel else "") + "render_bwd_pairs_kernel"
                if pk in tj or pk in vj:
                    return pk
            alias = {"duplicate_with_keys": "duplicate", "tile_ranges": "ranges", "tile_sort_long": "tile_sort"}
            base = ("surfel_" if surfel and name in ("preprocess_fwd", "preprocess_bwd", "render_fwd", "render_bwd") else "") \
                + alias.get(name, name)
            for cand in (base + "_views_kernel", base + "_kernel"):
                if cand in tj or cand in vj:
                    return cand
            return base + "_kernel"

        for name, (ms, cnt) in prof.items():
            if cnt:
                k = dict(avg_us=round(1e3 * ms / cnt, 2), launches=cnt, total_ms=round(ms, 3))
                if alg.get(name):      # algorithmic bytes per launch against the 8 TB/s HBM peak, per kernel
                    multi = name in ("preprocess_fwd", "preprocess_bwd") and cnt < args.steps * vpg   # views kernels
                    per_launch = alg[name + "_views"] if multi else alg[name]
                    if name == "tile_sort_long" and alg.get("_tile_sort_long_view") is not None:
                        per_launch = alg["_tile_sort_long_view"] * vpg * args.steps / cnt
                    if name == "render_bwd" and cnt < args.steps * vpg:     # K7 of all views in one launch (round 4)
                        per_launch = alg[name] * vpg * args.steps / cnt
                    k["alg_bytes"] = int(per_launch)
                    k["alg_GBs"] = round(per_launch / (k["avg_us"] * 1e-6) / 1e9, 1)
                    k["frac"] = round(k["alg_GBs"] / HBM_PEAK_GBS, 4)
                if pmc_name(name) in tj and name != "tile_sort_long":   # (the PMC summary merges the tile-sort classes)
                    k["traffic"] = tj[pmc_name(name)]
                kernels[name] = k
        # The kernels of different views run on side streams, several launches at a time: each launch then takes
        # longer than it does alone (its event pair brackets time it shares with the other views' kernels), and the
        # per-launch figures shrink although the work per second does not.  A short extra pass with every kernel on ONE
        # stream gives each kernel's duration on its own.
        if kernels and R.K.RENDER_SIDE and vpg > 1 and not (args.per_view or args.backward_per_view or args.torch_loss and surfel):
            R.K.RENDER_SIDE = 0
            try:
                prof1 = profiled(step, min(args.steps, 3))
            finally:
                R.K.RENDER_SIDE = 1
            for name, (ms1, cnt1) in prof1.items():
                if cnt1 and name in kernels:
                    a1 = 1e3 * ms1 / cnt1
                    kernels[name]["avg_us_serial"] = round(a1, 2)
                    if kernels[name].get("alg_bytes"):
                        kernels[name]["frac_serial"] = round(kernels[name]["alg_bytes"] / (a1 * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)
        if kernels:
            # dominant = the largest share of the step's GPU time.  Summed event time overstates kernels that run several at
            # a time (four concurrent K6 on four streams: 4 x 354 us of events for 4 x 138 us of work), so a kernel's share
            # is launches x its duration ALONE where the serial pass measured it
            dom = max(kernels, key=lambda k: kernels[k]["launches"] * kernels[k].get("avg_us_serial", kernels[k]["avg_us"]))
            avg_s = kernels[dom]["avg_us"] * 1e-6
            achieved = kernels[dom].get("alg_bytes", alg[dom]) / avg_s / 1e9
            traffic = kernels[dom].get("traffic")
            roofline = dict(bound="hbm", kernel=dom, achieved=round(achieved, 1), peak=HBM_PEAK_GBS,
                            unit="GB/s", frac=round(achieved / HBM_PEAK_GBS, 4),
                            traffic=traffic, traffic_scene=(meta if pmc_ok else None),
                            alg_bytes_per_launch=int(kernels[dom].get("alg_bytes", alg[dom])),
                            avg_launch_us=kernels[dom]["avg_us"],
                            path_bytes_view=int(alg["_bytes_view"]),
                            path_frac=round(views_per_sec / world * alg["_bytes_view"] / 1e9 / HBM_PEAK_GBS, 4))
            # the path AS BUILT: sum over the kernels of launches x the algorithmic bytes of that launch (the multi-view K1 / K9
            # read the per-Gaussian inputs once per node, not once per view as the contract formula `path_frac` charges) plus
            # the gradient-record fills, per step, against the same peak
            built = sum(k["launches"] * k.get("alg_bytes", 0) for k in kernels.values()) / args.steps
            if not (args.per_view or args.backward_per_view):
                built += vpg * n * (128 if surfel else 64)
            roofline.update(path_bytes_step_built=int(built),
                            path_frac_built=round(built / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                            path_note="path_frac: SURVEY 8(d)'s per-view formula x views/s (the contract's figure); "
                                      "path_frac_built: the algorithmic bytes of the kernels as launched; "
                                      "path_frac_measured: rocprofv3 PMC bytes of the same launches")
            if pmc_ok and tj:
                # what the counters say the whole path moves per step (sum over kernels of launches x PMC bytes per
                # launch; kernels without a PMC figure count with their algorithmic bytes), against the same peak: the
                # algorithmic path_frac charges the per-Gaussian bytes of K1 / K9 once per view although the multi-view
                # kernels read the inputs once per node — this one does not
                moved = sum(k["launches"] * (k.get("traffic") or k.get("alg_bytes") or 0) for nm, k in kernels.items()) / args.steps
                if not surfel:    # gradient-record memsets: 64 B per Gaussian and view (hipMemsetAsync, not a library kernel)
                    moved += vpg * n * 64
                roofline.update(path_bytes_step_measured=int(moved),
                                path_frac_measured=round(moved / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 4))
            # K6 / K7 are not HBM bound: K6 sits against the VALU issue rate, K7 against the VALU issue rate AND the
            # device's float-atomic line rate (atomic_frac below): pixel-Gaussian evaluations, VALU instructions, atomic lines
            if pair_views:
                pairs = sum(pair_views) / len(pair_views)
                roofline.update(pairs_per_view=int(pairs), pairs_per_s=round(2 * pairs * views_per_sec / world, 1),
                                pairs_note="sum over pixels of n_contrib = list entries the reference's per-pixel loops "
                                           "evaluate in the forward; x2 for the backward; per GPU")
            iv = vj.get(pmc_name(dom))
            if iv:      # SQ_INSTS_VALU per launch (rocprofv3 --pmc): one wave64 VALU instruction issues in >= 2 cycles
                simds, clk = 1024, 2.4e9            # on a SIMD32 (v_mul_f32 class, scripts/ubench/valu_rate.hip)
                roofline.update(valu_insts_per_launch=int(iv),
                                valu_issue_frac=round(iv * 2 / (kernels[dom]["avg_us"] * 1e-6 * simds * clk), 4),
                                valu_note="SQ_INSTS_VALU x 2 cycles / (launch time x 1024 SIMDs x 2.4 GHz): fraction of the "
                                          "peak VALU issue rate; the kernel's own mix (DPP, compares, 3-source fma, exp: "
                                          "3.5-8 cycles each) averages ~3.6 cycles per instruction")
            if dom == "render_bwd" and k7_variant:
                roofline["k7_variant"] = k7_variant
            ia = aj.get(pmc_name(dom))
            if ia:      # K7: one float-atomic record line per (entry, 4x4 block) hit; they execute outside the L2s
                roofline.update(atomic_lines_per_launch=int(ia), atomic_peak_lines_per_s=ATOMIC_PEAK_LINES,
                                atomic_frac=round(ia / (kernels[dom]["avg_us"] * 1e-6) / ATOMIC_PEAK_LINES, 4),
                                atomic_note="TCC_EA0_ATOMIC per launch (rocprofv3 --pmc; == TCC_ATOMIC: every float atomic "
                                            "leaves the L2) / launch time, against the device's measured rate of 64-byte "
                                            "atomic lines (scripts/atomic_probe.hip, profiles/r04_atomic_probe.txt: 20.9-21.0 G/s "
                                            "whatever the lanes per line; hidden behind VALU work when there is enough of it)")
            if kernels[dom].get("avg_us_serial"):
                avg1 = kernels[dom]["avg_us_serial"]
                if roofline.get("valu_insts_per_launch"):
                    roofline["valu_issue_frac_serial"] = round(roofline["valu_insts_per_launch"] * 2 / (avg1 * 1e-6 * 1024 * 2.4e9), 4)
                if roofline.get("atomic_lines_per_launch"):
                    roofline["atomic_frac_serial"] = round(roofline["atomic_lines_per_launch"] / (avg1 * 1e-6) / ATOMIC_PEAK_LINES, 4)
                roofline.update(avg_launch_us_serial=avg1, frac_serial=kernels[dom].get("frac_serial"),
                                launch_overlap=round(kernels[dom]["avg_us"] / avg1, 2))
    note("roofline pass done")
    # ---- second headline: the UNCHANGED caller's pattern, timed in the same run ------------------------------------------
    # lightning/network.py:827-838 renders the views one `render_img` at a time (torch activations, a new settings tuple
    # and a new (N,4) carrier per call, lightning/renderer.py:209-272), sums the losses and back-propagates ONCE through
    # all the graphs.  `value` above is the fused multi-view entry a modified caller can use; this is what the reference's
    # files get as they are.
    per_view = None
    if args.full and not (args.per_view or args.backward_per_view or args.no_per_view_leg):
        pv_step = make_step(True, True)
        for _ in range(max(1, min(args.warmup, 13))):     # (13: the K7 choice of this launch shape settles after 12 launches)
            pv_step()
        barrier()
        k_pv = max(1, min(args.steps, 10))
        gc.collect()
        gc.disable()
        t1 = time.perf_counter()
        for _ in range(k_pv):
            pv_step()
        barrier()
        el = time.perf_counter() - t1
        gc.enable()
        if use_dist:
            t = torch.tensor([el], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        pv = total_views * k_pv / el
        per_view = dict(value=round(pv, 2), unit="views/s", ms_per_step=round(1e3 * el / k_pv, 3), steps=k_pv,
                        entry=("renderer_2dgs.render_img" if surfel else "render_img") + " per view, torch activations "
                              "(lightning/renderer.py:225-230 op for op), torch loss, one backward through all views",
                        cameras=("built once (--prebuilt-cams)" if args.prebuilt_cams else
                                 "a MiniCam built on the device in front of every render call (lightning/network.py:832 -> "
                                 "lightning/utils.py:22-48: torch.inverse + a CPU projection matrix filled from device scalars)"),
                        host_boundary=("compiled (csrc/boundary.cpp)" if L.boundary() is not None else "python + ctypes"),
                        path_frac=round(pv / world * alg["_bytes_view"] / 1e9 / HBM_PEAK_GBS, 4),
                        of_fused=round(pv / views_per_sec, 3))
        if not args.prebuilt_cams:      # the same loop from cameras built once: what the camera construction costs the caller
            prebuilt_override["on"] = True
            pv2_step = make_step(True, True)
            prebuilt_override["on"] = False
            for _ in range(3):
                pv2_step()
            barrier()
            gc.collect()
            gc.disable()
            t1 = time.perf_counter()
            for _ in range(k_pv):
                pv2_step()
            barrier()
            el2 = time.perf_counter() - t1
            gc.enable()
            if use_dist:
                t = torch.tensor([el2], device=dev, dtype=torch.float64)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                el2 = float(t.item())
            per_view["value_prebuilt_cams"] = round(total_views * k_pv / el2, 2)
            per_view["ms_per_step_prebuilt_cams"] = round(1e3 * el2 / k_pv, 3)
        note(f"per-view leg done: {pv:.1f} views/s")
    # ---- third headline: the fused node with the IMAGES out and a torch loss on them ----------------------------------
    # /root/reference/lightning/loss.py:37-48 is MSE + 0.5 (1 - MS-SSIM) on the image: MS-SSIM needs the materialised image,
    # so the reference's main loss cannot use the loss fold behind `value` (its vjp stage, network.py:859, can).  This leg is
    # what a caller gets that switches its per-view loop to ONE render_views call and keeps its own loss: images (and depth /
    # alpha maps) written, torch ops for the loss, dL/dimage tensors read by K7.
    images_out = None
    if args.full and not (args.per_view or args.backward_per_view or args.no_per_view_leg or args.torch_loss or args.image_loss):
        io_step = make_step(False, False, torch_loss=True)
        for _ in range(max(1, min(args.warmup, 13)) if args.no_settle else K7_SETTLE_STEPS):
            io_step()
        barrier()
        k_io = max(1, min(args.steps, 10))
        gc.collect()
        gc.disable()
        t1 = time.perf_counter()
        for _ in range(k_io):
            io_step()
        barrier()
        el = time.perf_counter() - t1
        gc.enable()
        if use_dist:
            t = torch.tensor([el], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        io = total_views * k_io / el
        images_out = dict(value=round(io, 2), unit="views/s", ms_per_step=round(1e3 * el / k_io, 3), steps=k_io,
                          entry=("renderer_2dgs.render_views" if surfel else "render_views") + " (all views of the shard, one node), "
                                "images / maps materialised, torch loss on them (what lightning/loss.py:37-48 needs), one backward",
                          of_fused=round(io / views_per_sec, 3))
        note(f"images-out leg done: {io:.1f} views/s")
    # ---- CPU baseline: oracle (C restatement, OpenMP) on a bounded sample ------------------
    cpu_baseline = None
    psnr_vs_oracle = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        import numpy as np
        from oracle.gdr_oracle import Oracle, Settings
        from oracle.gsr_oracle import SurfelOracle

        cores = os.cpu_count() or 1
        o = (SurfelOracle if surfel else Oracle)("f32", nthreads=cores)
        cam = cams[0]
        s = Settings(h, w, math.tan(0.375), math.tan(0.375), np.ones(3, np.float32), 1.0,
                     cam.world_view_transform.cpu().numpy(), cam.full_proj_transform.cpu().numpy(), deg,
                     cam.camera_center.cpu().numpy())
        n_s = n  # bounded sample: 1 of the rank's views, full Gaussian set (~6 s on 8 cores)
        c = {k: v.detach()[:n_s].cpu() for k, v in params.items()}
        op = torch.sigmoid(c["opacity"]).numpy()
        sc = torch.exp(c["scales"]).numpy()
        ro = torch.nn.functional.normalize(c["rotations"]).numpy()
        g = np.random.default_rng(0)
        gc = g.standard_normal((3, h, w), dtype=np.float32)
        gd = g.standard_normal((1, h, w), dtype=np.float32)
        ga = g.standard_normal((1, h, w), dtype=np.float32)
        gm = g.standard_normal((7, h, w), dtype=np.float32)
        tc0 = time.perf_counter()
        reps = 0
        while True:
            ctx = o.forward(c["centers"].numpy(), op, s, shs=c["shs"].numpy(), scales=sc, rotations=ro)
            o.backward(ctx, gc, gm) if surfel else o.backward(ctx, gc, gd, ga)
            reps += 1
            if time.perf_counter() - tc0 > 10.0 or reps >= 5:
                break
        tc = (time.perf_counter() - tc0) / reps
        cpu_baseline = dict(value=round(1.0 / tc * (n_s / n), 4), unit="views/s", cores=cores, kind="port",
                            sample=f"oracle C restatement (OpenMP, {cores} threads), {reps} x fwd+bwd of 1 view {h}x{w}, "
                                   f"all {n} Gaussians ({tc:.2f} s each)")
        # BASELINE.json's metric ends in "PSNR vs ref": the oracle's render against the HIP render of the same view at the
        # benchmark's own size, on IDENTICAL inputs (torch activations for both: the rasterizer boundary of renderer.py:250-259),
        # for every view of the rank (the oracle as the checker, outside every timed region).  Threshold flips counted: an alpha
        # on the other side of 1/255 (a guard that re-evaluates near-threshold lanes in the oracle's order was built and
        # measured in round 5 — render.hip GDR_THRESHOLD_GUARD, profiles/r05_ab_threshold_guard.txt: -2..-4 %, 5 -> 3 flips —
        # and is NOT in the product build) or a transmittance on the other side of 1e-4 (T carries the accumulated rounding
        # of all earlier factors) adds or drops one contributor of one pixel: flips of both kinds remain expected.
        per_view_psnr = []
        try:
            act = (params["centers"].detach(), params["shs"].detach(), torch.sigmoid(params["opacity"].detach()),
                   torch.exp(params["scales"].detach()), torch.nn.functional.normalize(params["rotations"].detach()))
            e0 = torch.empty(0, device=dev)
            rend_u = (Renderer2D if surfel else Renderer)(sh_degree=deg, white_background=True, fused=False)
            rend_u.set_bg_color(torch.ones(3, device=dev))
            for vi, cam_v in enumerate(cams[:4]):
                if vi == 0:
                    ctx_v = ctx
                else:
                    s_v = Settings(h, w, math.tan(0.375), math.tan(0.375), np.ones(3, np.float32), 1.0,
                                   cam_v.world_view_transform.cpu().numpy(), cam_v.full_proj_transform.cpu().numpy(), deg,
                                   cam_v.camera_center.cpu().numpy())
                    ctx_v = o.forward(c["centers"].numpy(), op, s_v, shs=c["shs"].numpy(), scales=sc, rotations=ro)
                with torch.no_grad():
                    rs = rend_u.set_rasterizer(cam_v, device=dev).raster_settings
                    res = (SR if surfel else R).forward_raw(act[0], act[1], e0, act[2], act[3], act[4], e0, rs)
                    st0 = res[-2]
                    tt = st0.tensors()
                    img_h = res[0].clamp(0, 1).cpu().numpy()
                    nc_h = tt["n_contrib"].cpu().numpy().reshape(-1, h, w)[0].astype(np.int64)
                    ft_h = tt["final_T"].cpu().numpy().reshape(-1, h, w)[0]
                img_o = np.clip(ctx_v["color"], 0.0, 1.0)
                nc_o = np.asarray(ctx_v["n_contrib"]).reshape(-1, h, w)[0].astype(np.int64)
                ft_o = np.asarray(ctx_v["final_T"]).reshape(-1, h, w)[0]
                d_rgb = np.abs(img_h - img_o).max(axis=0)
                mse_v = float(((img_h - img_o) ** 2).mean())
                per_view_psnr.append(dict(
                    view=vi, psnr_db=round(10 * math.log10(1.0 / max(mse_v, 1e-20)), 1), max_abs_rgb=float(d_rgb.max()),
                    n_contrib_mismatch_pixels=int((nc_h != nc_o).sum()),
                    final_T_outlier_pixels=int((np.abs(ft_h - ft_o) > 1e-4 * np.abs(ft_o) + 1e-6).sum()),
                    rgb_outlier_pixels=int((d_rgb > 1e-4).sum())))
                del st0, tt, res
            worst = min(per_view_psnr, key=lambda q: q["psnr_db"])
            flips = dict(n_contrib_mismatch_pixels=sum(q["n_contrib_mismatch_pixels"] for q in per_view_psnr),
                         final_T_outlier_pixels=sum(q["final_T_outlier_pixels"] for q in per_view_psnr),
                         rgb_outlier_pixels=sum(q["rgb_outlier_pixels"] for q in per_view_psnr),
                         pixels=int(h * w) * len(per_view_psnr))
            psnr_vs_oracle = dict(psnr_db=worst["psnr_db"], max_abs_rgb=max(q["max_abs_rgb"] for q in per_view_psnr),
                                  threshold_flips=flips, per_view=per_view_psnr,
                                  view=f"the rank's first {len(per_view_psnr)} views (psnr_db = the worst of them), full size, all "
                                       "Gaussians, identical activated inputs; oracle = f32 C restatement (parity unpinned: DESIGN 0)")
        except Exception as ex:     # (a statistic: never fails the bench)
            psnr_vs_oracle = dict(error=f"{type(ex).__name__}: {ex}")

    # ---- the literal "PyTorch-CPU" baseline of north_star: the vectorised torch restatement with autograd
    # (oracle/torch_ref.py), all host cores, on a bounded sample (a prefix of the Gaussian set at the full image size;
    # the cost per view is linear in the number of Gaussians at fixed tile occupancy, so the rate is scaled by n_s / n)
    note("C-oracle baseline done")
    cpu_baseline_torch = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline and not surfel and args.workload != "c3":
        import subprocess
        thr = min(os.cpu_count() or 1, 16)   # torch's intra-op pool degrades on small per-tile tensors beyond this
        cmd = [sys.executable, os.path.join(ROOT, "scripts", "torch_cpu_baseline.py"), "--n", str(n), "--seed", str(wl["seed"]),
               "--sigma0", ",".join(str(x) for x in (wl["sigma0"] or (0.0052,))), "--h", str(h), "--w", str(w), "--deg", str(deg),
               "--layout", args.layout, "--threads", str(thr)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=150)
            res = json.loads(r.stdout.strip().splitlines()[-1])
            cpu_baseline_torch = dict(
                value=round(1.0 / res["seconds"] * (res["n_sample"] / n), 6), unit="views/s", cores=res["threads"], kind="port",
                sample=f"oracle/torch_ref.py (vectorised PyTorch forward + autograd backward, {res['threads']} threads), 1 x "
                       f"fwd+bwd of 1 view {h}x{w} on the first {res['n_sample']} of {n} Gaussians ({res['seconds']:.1f} s); "
                       f"rate scaled by {res['n_sample']}/{n} (cost is linear in N at fixed image size)")
        except Exception as ex:   # a baseline leg must never stall or fail the bench
            cpu_baseline_torch = dict(value=None, unit="views/s", kind="port", sample=f"not measured: {type(ex).__name__}")

    if rank == 0:
        out = {
            "metric": "views/sec fwd+bwd @ 800x800", "value": round(views_per_sec, 2), "unit": "views/s",
            "n_gpus": world, "world_size": dist.get_world_size() if use_dist else 1,
            "dist_backend": (dist.get_backend() if use_dist else None), "steps": args.steps, "timed_steps": timed_steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3),
            "ms_per_step_ranks": rank_ms, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
            "data": "synthetic (seeded random Gaussians with the decoder's statistics, random targets)",
            "config": {"workload": f"{args.workload}: {wl['desc']}", "n_gaussians": n, "layout": args.layout, "order": args.order,
                       "views_per_gpu": vpg, "image": [h, w], "sh_degree": deg,
                       "num_rendered_per_view": int(d_mean) if d_views else None, "parallelism": f"view-sharded x{world}",
                       "grad_allreduce": bool(args.grad_allreduce),
                       "peak_mem_gb": round(torch.cuda.max_memory_allocated(dev) / 2**30, 2),
                       "entry": ("renderer_2dgs.render_views (all views of the shard, one node)" if surfel and not (args.per_view or args.backward_per_view or args.torch_loss or args.unfused)
                                 else "renderer_2dgs.render_img per view" if surfel else ("render_img per view, backward per view" if args.backward_per_view else "render_img per view, one backward") if (args.per_view or args.backward_per_view)
                                 else "render_views (all views of the shard, one node)")
                       + (", torch activations" if args.unfused else ", activations fused into K1/K9"),
                       "loss": ("torch image MSE only (the reference's fine-stage / first-1000-iterations loss: no gradient for "
                                "depth, alpha or the 2DGS maps)" if args.image_loss else
                                "fused HIP kernels inside the render node, on the views' side streams "
                                "(MSE + 1000 distortion + 0.2 normal consistency + 0.1 depth + 0.1 alpha)"
                                if surfel and not (args.per_view or args.backward_per_view or args.torch_loss or args.unfused or args.loss_kernels)
                                else "fused HIP kernels, one autograd node per view "
                                "(MSE + 1000 distortion + 0.2 normal consistency + 0.1 depth + 0.1 alpha)"
                                if surfel and not (args.per_view or args.backward_per_view or args.torch_loss or args.unfused)
                                else "torch ops (MSE + 1000 distortion + 0.2 normal consistency + 0.1 depth + 0.1 alpha)" if surfel
                                else "torch ops" if (args.per_view or args.backward_per_view or args.stacked_loss or args.torch_loss or args.unfused)
                                else "fused HIP loss kernels (clamp+MSE+0.1 mean depth+0.1 mean alpha)" if args.loss_kernels
                                else "folded into K6 epilogue / K7 prologue (clamp+MSE+0.1 mean depth+0.1 mean alpha)")},
            "roofline": roofline, "k7_variant": k7_variant, "per_view": per_view, "images_out": images_out, "comm_ms": comm_ms,
            "spread": "same box run-to-run +-0.3 %, box-to-box +-4 % (BASELINE.md section 4: measured over 6 boxes)",
            "gc": "Python's cyclic collector disabled inside the timed regions (timeit convention; collected right before)",
            "cpu_baseline": cpu_baseline, "cpu_baseline_torch": cpu_baseline_torch,
            "psnr_vs_oracle": psnr_vs_oracle, "kernels": kernels,
            "loss_mean": float(last_losses.mean()) if args.full else None,
            # L1 norms of the Gaussians' gradients after the last step (with --grad-allreduce: of the sum over all ranks'
            # views) — lets a 2-rank run be compared with one rank rendering the same views (tests/test_gpu_multirank.py)
            "grad_l1": ({k: (float(p.grad.double().abs().sum()) if p.grad is not None else None) for k, p in params.items()}
                        if args.full else None),
        }
        os.write(result_fd, (json.dumps(out) + "\n").encode())
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
