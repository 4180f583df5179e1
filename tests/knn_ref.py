"""A numpy float32 restatement of the shell search of csrc/knn.hip, for the grid it is given (box and cells per axis):
-> the result and the number of candidates examined per point.  Exact values never come from here: they come from the
f64 brute force oracle.gsr_oracle.knn_mean_dist2.  The model exists to count work without a GPU, to keep the parent
algorithm's quadratic counts on record (`algo="parent"`), and to show that the cases of knn_cases.py catch a wrong search
(`mutant=`).

  algo = "product"  faces and cells both from u = p - lo, slack + 0.9999 margin, leaves the scan at three zeros
  algo = "parent"   the search before the per-axis grid: faces as lo + x * cs against p, 0.9999 margin only, no zero exit
  mutant (product): "no_margin"        no slack, no 0.9999
                    "skip_end_cell"    interior shell rows visit one end cell, not two
                    "wrong_face"       the bound is taken from the face one cell beyond the searched cube
                    "self_not_skipped" j == i is a candidate
                    "ties_dropped"     a distance equal to one already held is dropped
"""
import numpy as np

F = np.float32
TRIM_SHIFT = 8          # generativedensification_amd/knn.py
SLACK = F(1e-6)         # csrc/knn.hip KNN_SLACK
MARGIN = F(0.9999)


def parent_grid(pts):
    """The grid of the parent algorithm: exact bounding box, round((N / 2)^(1/3)) cells on every axis."""
    N = len(pts)
    G = max(1, min(256, int(round((N / 2.0) ** (1.0 / 3.0)))))
    return np.concatenate([pts.min(0), pts.max(0)]).astype(F), (G, G, G)


def product_grid(pts, cells_per_axis=None):
    """The grid generativedensification_amd/knn.py and knn_grid_kernel choose: per-axis quantile box, near-cubic cells,
    about N / 2 of them, one cell on an axis thinner than a cell."""
    N = len(pts)
    srt = np.sort(pts, axis=0)
    k = N >> TRIM_SHIFT
    bbox = np.concatenate([srt[k], srt[N - 1 - k]]).astype(F)
    if cells_per_axis:
        return bbox, (int(cells_per_axis),) * 3
    cap, M = N + 8, float(max(1, N // 2))
    e = bbox[3:].astype(np.float64) - bbox[:3].astype(np.float64)
    e = np.where(np.isfinite(e) & (e > 0), e, 0.0)
    e3, e2, e1 = np.sort(e)
    G = [1, 1, 1]
    if e1 > 0:
        s = np.cbrt(e1 * e2 * e3 / M)
        if not (s > 0 and e3 >= s):
            s = np.sqrt(e1 * e2 / M)
        if not (s > 0 and e2 >= s):
            s = e1 / M
        G = [int(min(max(e[k] / s + 0.5, 1.0), cap)) if e[k] >= s else 1 for k in range(3)]
    while G[0] * G[1] * G[2] > cap:
        k = int(np.argmax(G))
        others = G[(k + 1) % 3] * G[(k + 2) % 3]
        G[k] = max(1, min(G[k] - 1, cap // others))
    return bbox, tuple(G)


def search(pts, bbox, gdim, algo="product", mutant=None):
    """pts (N, 3) float32 -> (out (N,) float32, work (N,) int64) in the order of pts."""
    assert algo in ("product", "parent") and mutant in (None, "no_margin", "skip_end_cell", "wrong_face",
                                                        "self_not_skipped", "ties_dropped")
    pts = np.ascontiguousarray(pts, dtype=F)
    N = len(pts)
    out, work = np.full(N, np.inf, F), np.zeros(N, np.int64)
    if N == 0:
        return out, work
    G = np.asarray(gdim, dtype=np.int64)
    lo = np.asarray(bbox[:3], dtype=F)
    ext = np.maximum(np.asarray(bbox[3:], dtype=F) - lo, F(1e-20))
    Gf = G.astype(F)
    with np.errstate(over="ignore", invalid="ignore"):
        cs, ic = ext / Gf, Gf / ext
        slack = SLACK * ext
        u_all = pts - lo
        t = np.nan_to_num(u_all * ic, nan=0.0, posinf=3e9, neginf=-3e9)
    coord = np.clip(np.trunc(t).astype(np.int64), 0, G - 1)
    cid = (coord[:, 2] * G[1] + coord[:, 1]) * G[0] + coord[:, 0]
    order = np.argsort(cid, kind="stable")
    P, U, Cc = pts[order], u_all[order], coord[order]
    start = np.searchsorted(cid[order], np.arange(int(G.prod()) + 1))
    zero_exit = algo == "product"
    R = int(G.max())
    res, cnt = np.empty(N, F), np.zeros(N, np.int64)
    for i in range(N):
        p, u, c = P[i], U[i], Cc[i]
        best = np.full(3, np.inf, F)
        seen, done = 0, False

        def visit(x, y, z):
            nonlocal best, seen, done
            cell = (z * G[1] + y) * G[0] + x
            a, b = start[cell], start[cell + 1]
            if a == b:
                return
            j = np.arange(a, b)
            if mutant != "self_not_skipped":
                j = j[j != i]
            d = P[j] - p
            d = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
            if zero_exit:       # the scan leaves at the candidate that completes three zeros
                z_at = np.cumsum(d == 0) + np.count_nonzero(best == 0)
                hit = np.nonzero(z_at >= 3)[0]
                if len(hit):
                    d, done = d[: hit[0] + 1], True
            seen += len(d)
            if mutant == "ties_dropped":
                best = np.concatenate([np.unique(np.concatenate([best[np.isfinite(best)], d])), np.full(3, np.inf, F)])[:3]
            else:
                best = np.sort(np.concatenate([best, d]))[:3]

        for r in range(R):
            l, h = c - r, c + r
            for z in range(max(l[2], 0), min(h[2], G[2] - 1) + 1):
                for y in range(max(l[1], 0), min(h[1], G[1] - 1) + 1):
                    if done:
                        break
                    if z == l[2] or z == h[2] or y == l[1] or y == h[1]:
                        for x in range(max(l[0], 0), min(h[0], G[0] - 1) + 1):
                            if not done:
                                visit(x, y, z)
                    else:
                        if l[0] >= 0:
                            visit(l[0], y, z)
                        if h[0] < G[0] and h[0] != l[0] and not done and mutant != "skip_end_cell":
                            visit(h[0], y, z)
            if done:
                break
            bound = F(np.inf)
            for k in range(3):
                fl, fh = l[k], h[k] + 1
                if mutant == "wrong_face":
                    fl, fh = fl - 1, fh + 1
                if l[k] > 0:
                    if algo == "parent":
                        bk = p[k] - (lo[k] + F(fl) * cs[k])
                    else:
                        bk = u[k] - F(fl) * cs[k] - (F(0) if mutant == "no_margin" else slack[k])
                    bound = min(bound, F(bk))
                if h[k] < G[k] - 1:
                    if algo == "parent":
                        bk = (lo[k] + F(fh) * cs[k]) - p[k]
                    else:
                        bk = F(fh) * cs[k] - u[k] - (F(0) if mutant == "no_margin" else slack[k])
                    bound = min(bound, F(bk))
            if bound == np.inf:
                break
            bound = max(bound, F(0)) * (F(1) if mutant == "no_margin" else MARGIN)
            if best[2] <= F(bound) * F(bound):
                break
        res[i] = (best[0] + best[1] + best[2]) / F(3)
        cnt[i] = seen
    out[order], work[order] = res, cnt
    return out, work
