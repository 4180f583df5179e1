#!/usr/bin/env python
"""scripts/bench_densify.py — GPU time of the densification masks (generativedensification_amd.densify) bound as the forwards
of MaskModule / MaskResModule, against a torch restatement of the two forwards over this repository's drop-ins
(torch_geometric.utils.scatter / softmax / cumsum, torch_scatter.segment_csr) on the same GPU in the same process.

  shapes   N = 12 000 B points for B in {1, 3, 4}, C = 160, non_leaf_ratio 0.8, temperature 1
  scores   float32, and bfloat16 under bf16 autocast (the trainer's state: MaskModule's sigmoid is bf16 then)
  modes    top-k at every shape.  top-p against the restatement at 2 000 points per segment only (its triangular matrix holds
           sum n_b^2 / 2 index pairs); the fused call is also timed at 12 000 per segment.  (MaskModule's sigmoid scores put
           the top-p cut behind the first point or two of a segment; the work of both forms does not depend on where it falls.)
  timed    forward alone, and forward + backward to the parameters of `net` and to `feat`

The torch restatement: two global sorts (descending by score, then stable by segment), the rank of every point inside its segment
against ceil(ratio * n_b); for top-p a sparse lower-triangular matmul as the segmented prefix sum; the reference's
`assert sum(mask) == new_offset[-1]`; boolean indexing for the split.  Every pair is compared before it is timed (masks equal
where the scores are distinct).  Host synchronisations per forward are counted with torch.cuda.set_sync_debug_mode("warn").
Timing: warm-up, then `--repeats` windows of `--iters` calls per method, alternating, each window between two device events;
microseconds per call, median and range, host work included.  There is no pass bar.  The parent process never touches the GPU:
it starts one child under a time limit and relays its output.

Usage: python scripts/bench_densify.py [--out FILE.json] [--timeout 500]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import types
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEGMENTS = (1, 3, 4)
POINTS, TOP_P_POINTS, CHANNELS, RATIO = 12_000, 2_000, 160, 0.8


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


def host_syncs(fn):
    """the number of synchronising calls torch reports during fn()"""
    import torch

    torch.cuda.synchronize()
    previous = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode(previous)
    return sum("synchroniz" in str(w.message).lower() and "prototype" not in str(w.message).lower() for w in seen)


class Point(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def child(args):
    import torch
    import torch.nn.functional as F

    sys.path.insert(0, ROOT)
    import torch_scatter
    from torch_geometric.utils import cumsum as pyg_cumsum
    from torch_geometric.utils import scatter as pyg_scatter
    from torch_geometric.utils import softmax as pyg_softmax
    from generativedensification_amd import densify as D

    assert torch.cuda.is_available(), "bench_densify needs the GPU (no CPU fallback)"
    dev = torch.device("cuda:0")
    results = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "repeats": args.repeats, "rows": []}

    def emit(row):
        print(json.dumps(row), flush=True)
        results["rows"].append(row)

    def ranked_rows(score, batch):
        _, perm = torch.sort(score.view(-1), descending=True)
        sorted_batch, bperm = torch.sort(batch[perm], descending=False, stable=True)
        return perm[bperm], sorted_batch

    @torch.no_grad()
    def torch_top_k(score, ratio, offset):
        n = score.shape[0]
        batch = torch.repeat_interleave(torch.arange(offset.shape[0], device=dev), torch.diff(F.pad(offset, (1, 0))))
        counts = pyg_scatter(batch.new_ones(n), batch, reduce="sum")
        k = (float(ratio) * counts.to(score.dtype)).ceil().to(torch.long)
        rows, sorted_batch = ranked_rows(score, batch)
        rank = torch.arange(n, device=dev) - pyg_cumsum(counts)[sorted_batch]
        mask = torch.zeros(n, dtype=torch.bool, device=dev)
        mask[rows[rank < k[sorted_batch]]] = True
        return mask, torch.cumsum(k, dim=0)

    @torch.no_grad()
    def torch_top_p(score, ratio, offset):
        n = score.shape[0]
        ptr = F.pad(offset, (1, 0))
        batch = torch.repeat_interleave(torch.arange(offset.shape[0], device=dev), torch.diff(ptr))
        rows, _ = ranked_rows(score, batch)
        pairs = torch.cat([torch.tril_indices(int(e - a), int(e - a), device=dev) + a for a, e in zip(ptr[:-1], ptr[1:])], dim=-1)
        lower = torch.sparse_coo_tensor(pairs, torch.ones(pairs.shape[1], device=dev), (n, n))
        with torch.autocast("cuda", enabled=False):
            prefix = torch.mm(lower, score.view(-1)[rows][:, None].float())
        mask = torch.zeros(n, dtype=torch.bool, device=dev)
        mask[rows[prefix.to(score.dtype).flatten() <= ratio]] = True
        return mask, torch_scatter.segment_csr(mask.to(offset.dtype), ptr, reduce="sum").cumsum(0)

    def torch_select(self, prob, offset):
        return (torch_top_k if self.mask_sampling_type == "topk" else torch_top_p)(prob, self.non_leaf_ratio, offset)

    def torch_mask_module(self, point):
        feat = point.feat
        prob = torch.sigmoid(self.net(feat))
        non_leaf, non_leaf_offset = torch_select(self, prob, point.offset)
        assert torch.sum(non_leaf) == non_leaf_offset[-1]
        leaf = ~non_leaf
        gate = (feat - feat * prob).detach() + feat * prob
        return Point(coord=point.coord[non_leaf], feat=gate[non_leaf], global_feat=point.global_feat, offset=non_leaf_offset,
                     grid_size=point.grid_size,
                     leaf_point=Point(coord=point.coord[leaf], feat=gate[leaf], offset=point.offset - non_leaf_offset,
                                      grid_size=point.grid_size))

    def hip_mask_module(self, point):
        return D.mask_module_forward(self, point)

    def torch_mask_res_module(self, point):
        feat = point.feat
        raw_prob = self.net(feat)
        prob = pyg_softmax(src=raw_prob.to(torch.float32) / self.temperature, ptr=F.pad(point.offset, (1, 0)), dim=0)
        non_leaf, non_leaf_offset = torch_select(self, prob, point.offset)
        assert torch.sum(non_leaf) == non_leaf_offset[-1]
        out = Point(point)
        out.feat = (feat * non_leaf[:, None] - feat * prob).detach() + feat * prob
        out.update({"raw_prob": raw_prob, "prob": prob, "non_leaf": non_leaf, "non_leaf_offset": non_leaf_offset, "leaf": ~non_leaf,
                    "leaf_offset": point.offset - non_leaf_offset})
        return out

    def hip_mask_res_module(self, point):
        return D.mask_res_module_forward(self, Point(point))

    modules = {"MaskModule": (hip_mask_module, torch_mask_module, lambda o: (o.feat, o.leaf_point.feat)),
               "MaskResModule": (hip_mask_res_module, torch_mask_res_module, lambda o: (o.feat,))}
    cases = [("topk", POINTS, b, True) for b in SEGMENTS] + [("topp", TOP_P_POINTS, 3, True), ("topp", POINTS, 3, False)]
    for autocast in (False, True):
        ctx = lambda: torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast)      # noqa: E731
        for mode, per_segment, b, against_torch in cases:
            n, c = per_segment * b, CHANNELS
            g = torch.Generator().manual_seed(n + b)
            net = torch.nn.Sequential(torch.nn.Linear(c, c), torch.nn.GELU(), torch.nn.Linear(c, 1)).to(dev)
            feat = torch.randn(n, c, generator=g).to(dev).requires_grad_(True)
            point = Point(coord=torch.randn(n, 3, generator=g).to(dev), feat=feat, global_feat=torch.randn(b, 24, generator=g).to(dev),
                          offset=torch.arange(1, b + 1, device=dev) * per_segment, grid_size=0.01)
            leaves = tuple(net.parameters()) + (feat,)
            for name, (hip_fwd, torch_fwd, feats_of) in modules.items():
                self = types.SimpleNamespace(net=net, non_leaf_ratio=RATIO, temperature=1.0, mask_sampling_type=mode)

                def run(fwd):
                    with ctx():
                        return fwd(self, point)

                def both(fwd):
                    def fwd_bwd():
                        outs = feats_of(run(fwd))
                        return torch.autograd.grad(outs, leaves, [torch.ones_like(o) for o in outs], allow_unused=True)
                    return (lambda: run(fwd)), fwd_bwd

                forms = {"hip": both(hip_fwd)}
                row = {"module": name, "mode": mode, "N": n, "B": b, "C": c, "autocast": autocast}
                a = run(hip_fwd)
                row["score_dtype"] = str((a.prob if name == "MaskResModule" else run(lambda s, p: torch.sigmoid(s.net(p.feat)))).dtype)
                row["selected"] = int((a.non_leaf_offset if name == "MaskResModule" else a.offset)[-1])
                if against_torch:
                    try:
                        t = run(torch_fwd)
                        if name == "MaskResModule":
                            row["masks_differ_in"] = int((a.non_leaf != t.non_leaf).sum())
                        else:
                            row["selected_torch"] = int(t.offset[-1])
                        forms["torch"] = both(torch_fwd)
                    except Exception as exc:      # noqa: BLE001 — a torch form that cannot run at this shape is reported, not fatal
                        row["torch_error"] = f"{type(exc).__name__}: {str(exc)[:200]}"
                row["host_syncs_per_forward"] = {k: host_syncs(v[0]) for k, v in forms.items()}
                emit({"case": "forward", **row, **timed({k: v[0] for k, v in forms.items()}, args.iters, args.repeats)})
                emit({"case": "forward_backward", **row, **timed({k: v[1] for k, v in forms.items()}, args.iters, args.repeats)})
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
        print(f"bench_densify: the GPU process did not finish in {args.timeout} s", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
