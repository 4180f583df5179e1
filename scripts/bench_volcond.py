#!/usr/bin/env python
"""scripts/bench_volcond.py — GPU time of the fused volume conditioning (generativedensification_amd.volcond) against the torch
routes on the same GPU in the same process, at the reference shape: batch 3, 4 and 2 views, 32 x 32 token maps of 768 channels
under intrinsics of a 512 x 512 image, view_embed 32, a 16^3 grid, n_groups [16].

  candidates, from the (B V, 1 + L, C) encoder output and the batch's cameras and rays to the cond (B g^3, V bs^3, C + E):
    reference  the reference's composition restated (ray_to_plucker, rsh_cart_3, ModLN, einsum copies, grid_sample, cat, the
               cond lines of VolTransformer.forward)
    documented the path the repository documented before this module: torch ModLN, pointfeat.sample_views with the intrinsics
               rescaled to the token map, cat, deconv3d._cond
    fused      volcond.volume_conds (ray_sh, the Linear, mod_layer_norm, sample_tokens)
  launches     through the C ABI on buffers of the same sizes: every launch of the fused path on its own, with the bytes it has
               to move at least (each operand read once, each result written once) and its time over the time of those bytes
               at --peak-tbs TB/s

fp32, and bf16 autocast (float32 parameters).  Operands are random, not zero.  The candidates are compared before they are timed.
Timing: warm-up, then `--repeats` windows of `--iters` calls per candidate, alternating, each window between two device events;
microseconds per call, median and range.  There is no pass bar.  The parent process never touches the GPU: it starts one child
per (mode, views), each under its own `timeout -k 10`, and relays their output.

Usage: python scripts/bench_volcond.py [--out profiles/volcond_bench.json] [--timeout 240]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH, TOK, C, E, RESO, IMG, N_GROUPS = 3, 32, 768, 32, 16, 512, (16,)
MODES = ("fp32", "bf16-autocast")
VIEWS = (4, 2)


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


def verdict(times):
    """'hip' only where the fused path's median is below both others' and its range over the windows overlaps neither"""
    f = times["fused"]
    for other in ("reference", "documented"):
        times[f"{other}_over_fused"] = round(times[other]["median_us"] / f["median_us"], 2)
    times["recommend"] = "hip" if all(f["median_us"] < times[o]["median_us"] and f["max_us"] < times[o]["min_us"]
                                      for o in ("reference", "documented")) else "torch"
    return times


def child(args):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import volcond_cases as VC               # the orbit cameras and the grid of the tests
    import volcond_torch as T                # the reference's composition restated
    from generativedensification_amd import _lib as L
    from generativedensification_amd import _marshal as M
    from generativedensification_amd import deconv3d as D
    from generativedensification_amd import pointfeat as PF
    from generativedensification_amd import volcond as V

    assert torch.cuda.is_available(), "bench_volcond needs the GPU (no CPU fallback)"
    dev = torch.device("cuda:0")
    bf16, f32 = torch.bfloat16, torch.float32
    mode, Vn = args.child, args.views
    autocast = mode != "fp32"
    BV, L_tok, r = BATCH * Vn, TOK * TOK, RESO

    def emit(row):
        row["mode"], row["views"] = mode, Vn
        print(json.dumps(row), flush=True)

    gen = torch.Generator().manual_seed(0)
    rng = np.random.default_rng(0)
    norm = torch.nn.LayerNorm(C, eps=1e-6).to(dev)
    mlp = torch.nn.Sequential(torch.nn.SiLU(), torch.nn.Linear(32, 2 * C)).to(dev)
    with torch.no_grad():
        norm.weight.copy_(1 + 0.3 * torch.randn(C, generator=gen))
        norm.bias.copy_(0.2 * torch.randn(C, generator=gen))
    view_embed = torch.nn.Parameter(torch.randn(1, 4, E, 1, 1, 1, generator=gen).to(dev))
    grid = torch.from_numpy(VC.grid_points(r)).to(dev, f32)
    net = types.SimpleNamespace(volume_grid=grid.view(r, r, r, 3), feat_vol_reso=r, dir_norm=types.SimpleNamespace(norm=norm, mlp=mlp),
                                view_embed=view_embed, cfg=types.SimpleNamespace(model=types.SimpleNamespace(view_embed_dim=E)),
                                vol_decoder=types.SimpleNamespace(n_groups=list(N_GROUPS)))
    w2cs, ixts = VC.orbit_cameras(BV, (IMG, IMG))
    w2cs, ixts = torch.from_numpy(w2cs).to(dev, f32), torch.from_numpy(ixts).to(dev, f32)
    rays = torch.from_numpy(np.concatenate([rng.standard_normal((BATCH, Vn, TOK, TOK, 3)) * 1.2,
                                            rng.standard_normal((BATCH, Vn, TOK, TOK, 3))], -1)).to(dev, f32)
    batch = {"tar_w2c": w2cs.view(BATCH, Vn, 4, 4), "tar_ixt": ixts.view(BATCH, Vn, 3, 3), "tar_rays_down": rays,
             "tar_rgb": torch.zeros(1, device=dev).expand(BATCH, Vn, IMG, IMG, 3)}
    # the encoder's output: token-major with a class token, in the autocast dtype under autocast
    tokens = torch.randn(BV, 1 + L_tok, C, generator=gen).to(dev, bf16 if autocast else f32).requires_grad_(True)
    scale = torch.tensor([[TOK / IMG, 0, (TOK / IMG - 1) / 2], [0, TOK / IMG, (TOK / IMG - 1) / 2], [0, 0, 1]], device=dev)
    ixts_tok = scale @ ixts

    def img_feats():
        return torch.einsum('blc->bcl', tokens[:, 1:]).reshape(BV, C, TOK, TOK)

    def torch_modln(feats):
        sh = T.ray_sh(rays.reshape(-1, TOK, TOK, 6))
        x = T.mod_layer_norm(torch.einsum('bchw->bhwc', feats), mlp(sh), norm.weight, norm.bias, norm.eps)
        return torch.einsum('bhwc->bchw', x)

    def embed(vol):
        return torch.cat((vol, view_embed[:, :Vn].expand(BATCH, -1, -1, r, r, r)), dim=2)

    def reference():
        vol = T.feat_vol(torch_modln(img_feats()), grid, w2cs, ixts, (IMG, IMG), Vn)
        return [T.cond_of(embed(vol), g) for g in N_GROUPS]

    def documented():
        x = torch_modln(img_feats())
        vol = PF.sample_views(x.float(), grid, w2cs, ixts_tok)[0].to(x).view(BATCH, Vn, C, r, r, r)
        return [D._cond(embed(vol), g, r // g) for g in N_GROUPS]

    def fused():
        return V.volume_conds(net, img_feats(), Vn, batch, img_hw=(IMG, IMG))

    cands = {"reference": reference, "documented": documented, "fused": fused}
    ins = (tokens, norm.weight, norm.bias, mlp[1].weight, mlp[1].bias, view_embed)
    gouts = [torch.randn(BATCH * g ** 3, Vn * (r // g) ** 3, C + E, generator=gen).to(dev) for g in N_GROUPS]

    def forward(name):
        def run():
            with torch.no_grad(), torch.autocast("cuda", dtype=bf16, enabled=autocast):
                return cands[name]()
        return run

    def both(name):
        def run():
            with torch.autocast("cuda", dtype=bf16, enabled=autocast):
                out = cands[name]()
            return torch.autograd.grad(out, ins, [g.to(o.dtype) for g, o in zip(gouts, out)])
        return run

    # fused against documented: both project in float32.  Against the reference the differences are reported only: under
    # autocast its projection matmuls run in bfloat16 and move the sample positions by up to a pixel of the full image
    tol = 5e-2 if autocast else 1e-4
    outs = {k: forward(k)() for k in cands}
    for k, base in (("documented", "reference"), ("fused", "reference"), ("fused", "documented")):
        for s, t in zip(outs[k], outs[base]):
            assert s.shape == t.shape, (k, base, s.shape, t.shape)      # (under autocast the reference's cond einsum leaves bfloat16)
            err = float((s.float() - t.float()).abs().max())
            emit(dict(case=f"forward_{k}_against_{base}_max_abs", value=float(f"{err:.3e}"), dtypes=[str(s.dtype), str(t.dtype)]))
            assert base == "reference" or err <= tol * float(t.float().abs().max()), (k, base, err)
    grads = {k: both(k)() for k in cands}
    for k, base in (("documented", "reference"), ("fused", "reference"), ("fused", "documented")):
        rel = [float((s.double() - t.double()).norm()) / max(float(t.double().norm()), 1e-30) for s, t in zip(grads[k], grads[base])]
        emit(dict(case=f"gradients_{k}_against_{base}_relative_norm", values=[float(f"{x:.3e}") for x in rel]))
        assert base == "reference" or max(rel) <= max(4 * tol, 1e-2), (k, base, rel)
    del outs, grads

    emit(dict(case="forward", **verdict(timed({k: forward(k) for k in cands}, args.iters, args.repeats))))
    emit(dict(case="forward_backward", **verdict(timed({k: both(k) for k in cands}, args.iters, args.repeats))))

    # ---- the launches of the fused path on their own ----
    lib = L.load()
    x_dt = bf16 if autocast else f32
    es, ss_es = (2 if autocast else 4), (2 if autocast else 4)
    R = BV * L_tok
    N, g = r ** 3, N_GROUPS[0]
    W = C + E
    dt = V._DTYPES
    tok = tokens.detach()
    x = tok[:, 1:]
    ss = torch.randn(R, 2 * C, generator=gen).to(dev, x_dt)
    rows = torch.empty(R, C, dtype=f32, device=dev)
    sh = torch.empty(R, 32, dtype=f32, device=dev)
    grad_rows = torch.randn(R, C, generator=gen).to(dev)
    dx, dss = torch.empty(R, C, dtype=x_dt, device=dev), torch.empty_like(ss)
    dw, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
    mws, mbase, musable = M.queried_workspace(lib.gdr_volcond_modln_backward_bytes, "gdr_volcond_modln_backward_bytes", dev, R, C)
    a = L.GdrVolcondSampleArgs(BATCH, Vn, TOK, TOK, C, E, r, g, IMG, IMG)
    import ctypes
    ar = ctypes.byref(a)
    cond = torch.empty(BATCH * g ** 3, Vn * (r // g) ** 3, W, dtype=f32, device=dev)
    keys = torch.empty(4 * BV * N, dtype=torch.int64, device=dev)
    wts = torch.empty(4 * BV * N, dtype=f32, device=dev)
    ve = view_embed.detach()[0, :, :, 0, 0, 0]
    sws, sbase, susable = M.queried_workspace(lib.gdr_volcond_sample_backward_bytes, "gdr_volcond_sample_backward_bytes", dev, ar)
    drows, dve = torch.empty(R, C, device=dev), torch.empty(Vn, E, device=dev)
    F = dt[f32]

    def ray_sh_launch():
        L.check(lib.gdr_volcond_ray_sh(rays.data_ptr(), F, R, 1, sh.data_ptr(), M.stream()), "gdr_volcond_ray_sh")

    def modln_fwd():
        L.check(lib.gdr_volcond_modln_forward(x.data_ptr(), C, L_tok, (1 + L_tok) * C, dt[x_dt], ss.data_ptr(), 2 * C, dt[x_dt], norm.weight.data_ptr(),
                                              F, norm.bias.data_ptr(), F, R, C, 1e-6, rows.data_ptr(), F, M.stream()), "gdr_volcond_modln_forward")

    def modln_bwd():
        L.check(lib.gdr_volcond_modln_backward(grad_rows.data_ptr(), C, F, x.data_ptr(), C, L_tok, (1 + L_tok) * C, dt[x_dt], ss.data_ptr(), 2 * C,
                                               dt[x_dt], norm.weight.data_ptr(), F, norm.bias.data_ptr(), F, R, C, 1e-6, mbase, musable,
                                               dx.data_ptr(), dss.data_ptr(), dw.data_ptr(), db.data_ptr(), M.stream()),
                "gdr_volcond_modln_backward")

    def sample_fwd():
        L.check(lib.gdr_volcond_sample_forward(ar, rows.data_ptr(), F, grid.data_ptr(), w2cs.data_ptr(), ixts.data_ptr(), ve.data_ptr(), E, F,
                                               cond.data_ptr(), F, keys.data_ptr(), wts.data_ptr(), M.stream()), "gdr_volcond_sample_forward")

    def sample_bwd():
        L.check(lib.gdr_volcond_sample_backward(ar, gouts[0].data_ptr(), F, keys.data_ptr(), wts.data_ptr(), sbase, susable, drows.data_ptr(), F,
                                                dve.data_ptr(), F, M.stream()), "gdr_volcond_sample_backward")

    pairs = BV * N
    floors = {"ray_sh": R * (6 * 4 + 32 * 4), "modln_forward": R * (C * es + 2 * C * ss_es + C * 4),
              "modln_backward": R * (C * 4 + C * es + 2 * C * ss_es + C * es + 2 * C * ss_es),
              # a sample reads at most min(4 pairs, texels) rows of the map and writes the cond and the tap table
              "sample_forward": min(4 * pairs, R) * C * 4 + pairs * W * 4 + 4 * pairs * 12,
              "sample_backward": pairs * W * 4 + 4 * pairs * 12 + R * C * 4}
    sample_fwd()
    times = timed({"ray_sh": ray_sh_launch, "modln_forward": modln_fwd, "modln_backward": modln_bwd, "sample_forward": sample_fwd,
                   "sample_backward": sample_bwd}, args.iters, args.repeats)
    for name, t in times.items():
        floor_us = floors[name] / (args.peak_tbs * 1e12) * 1e6
        emit(dict(case="launch_" + name, **t, least_bytes=floors[name], floor_us=round(floor_us, 2),
                  time_over_floor=round(t["median_us"] / floor_us, 2), achieved_tbs=round(floors[name] / t["median_us"] / 1e6, 3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volcond_bench.json"))
    ap.add_argument("--timeout", type=int, default=240, help="seconds for each child")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--peak-tbs", type=float, default=8.0, help="the HBM rate the byte floor is turned into time with")
    ap.add_argument("--child", default=None)
    ap.add_argument("--views", type=int, default=4)
    args = ap.parse_args()
    if args.child:
        return child(args)
    results = {"shape": {"batch": BATCH, "views": list(VIEWS), "tokens": [TOK, TOK], "C": C, "E": E, "r": RESO, "n_groups": list(N_GROUPS),
                         "image": [IMG, IMG]}, "iters": args.iters, "repeats": args.repeats, "peak_tbs": args.peak_tbs, "rows": []}
    for mode in MODES:
        for views in VIEWS:
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", mode, "--views", str(views),
                   "--iters", str(args.iters), "--repeats", str(args.repeats), "--peak-tbs", str(args.peak_tbs)]
            proc = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            for line in proc.stdout.splitlines():
                print(line, flush=True)
                if line.startswith("{"):
                    results["rows"].append(json.loads(line))
            if proc.returncode:
                print(f"bench_volcond: the {mode} / {views} views child ended with status {proc.returncode}; nothing more is started",
                      file=sys.stderr)
                return proc.returncode
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
