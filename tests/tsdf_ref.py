"""Vectorised numpy restatement of the TSDF fusion and marching-cubes extraction of csrc/tsdf.hip (include/gdr.h gdr_tsdf_*).

The semantics are those of Open3D's ScalableTSDFVolume (RGB8 colour) as published; parity with Open3D itself is unpinned.
All arithmetic is fp32 in the order written below, so the HIP kernels (built with -ffp-contract=off) reproduce it bit for bit.

Depth      D(v, u) is set to 0 where it is not finite, <= 0 or > depth_trunc.  Colour is uint8; float input is staged as
           p = rgb * 255 in fp32, truncated toward zero, then clipped to 0..255, and NaN gives 0 (floor(rgb * 255) on [0, 1]).
Allocation pixels with u % S == 0, v % S == 0 (S = depth_sampling_stride) and d > 0: q = ((u - cx) d / fx, (v - cy) d / fy, d),
           p = c2w q (c2w = inverse of E in f64, cast to f32); every block b with floor((p - trunc) / L) <= b <= floor((p + trunc) / L)
           per axis (L = R * voxel) is marked as touched by the view.  Blocks are ordered by (bz, by, bx).
Integration view by view, only into the blocks the view touched: voxel g (global integer index) has centre x = (g + 0.5) voxel,
           xc = E x; if z > 0: u = floor(xc.x fx / z + cx + 0.5) (v likewise), inside the image, d = D(v, u) > 0,
           sdf = (d - z) sqrt(1 + ((u - cx) / fx)^2 + ((v - cy) / fy)^2); if sdf > -trunc: t = min(1, sdf (1 / trunc)),
           T = (T w + t) / (w + 1), C = (C w + c) / (w + 1), w += 1.
Extraction a cube (lower corner voxel g) is valid when its 8 corners have w > 0; bit i of its case is T_i < 0; cases 0 and 255
           emit nothing.  A grid edge (a, a + e_axis) carries a vertex when its end points differ in sign, both have w > 0 and one of
           the (up to 4) cubes around it is valid: position centre(a) + (|Ta| / (|Ta| + |Tb|)) voxel along the axis, colour
           ((|Tb| Ca + |Ta| Cb) / (|Ta| + |Tb|)) / 255.  Vertices are ordered by owning voxel (block order, then the voxel's linear
           index x + R (y + R z)), then axis x < y < z; triangles by cube (same order), then table slot.
Post       crop (drop a triangle with any vertex outside the AABB, compared in f64), clusters of triangles sharing an edge, keep the
           clusters with count >= sorted(counts)[-min(#clusters, 10)], then drop unreferenced vertices (order kept).

The case table is derived here from first principles (TRI_TABLE): on every cube face the crossed edges are joined by segments, an
ambiguous face (two diagonal corners below zero) separating its negative corners; each segment is oriented so that the
negative side lies on its right seen from outside; the closed loops are fanned from their lowest edge.  csrc/tsdf.hip holds the
same table as a literal (test_tsdf_cpu.py checks the two agree).
"""
from __future__ import annotations

import numpy as np

f32 = np.float32

# corner i of a cube at offset CORNERS[i] (x, y, z); edge e joins corners EDGES[e] = (lower, upper)
CORNERS = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)], np.int64)
EDGES = ((0, 1), (1, 2), (3, 2), (0, 3), (4, 5), (5, 6), (7, 6), (4, 7), (0, 4), (1, 5), (2, 6), (3, 7))
EDGE_AXIS = tuple(int(np.argmax(CORNERS[b] - CORNERS[a])) for a, b in EDGES)
EDGE_OFFSET = tuple(tuple(int(c) for c in CORNERS[a]) for a, _ in EDGES)
_FACES = (((0, 3, 7, 4), (-1, 0, 0)), ((1, 2, 6, 5), (1, 0, 0)), ((0, 1, 5, 4), (0, -1, 0)), ((3, 2, 6, 7), (0, 1, 0)),
          ((0, 1, 2, 3), (0, 0, -1)), ((4, 5, 6, 7), (0, 0, 1)))


def _edge(a, b):
    return next(e for e, (p, q) in enumerate(EDGES) if {p, q} == {a, b})


def _build_tri_table():
    mid = [(CORNERS[a] + CORNERS[b]) / 2.0 for a, b in EDGES]
    table = []
    for case in range(256):
        neg = [bool((case >> i) & 1) for i in range(8)]
        nxt = {}
        for cs, n in _FACES:
            k = sum(neg[c] for c in cs)
            if k in (0, 4):
                continue
            centre = CORNERS[list(cs)].mean(0)
            segs = []
            for i, c in enumerate(cs):   # segments cutting off one corner: the lone negative (k = 1, or each of a diagonal
                prev, nxt_c = cs[i - 1], cs[(i + 1) % 4]   # pair), or the lone positive (k = 3)
                lone = (neg[c] and not neg[prev] and not neg[nxt_c]) if k != 3 else not neg[c]
                if lone:
                    g = (centre - CORNERS[c]) if neg[c] else (CORNERS[c] - centre)   # points from negative to positive
                    segs.append((_edge(c, prev), _edge(c, nxt_c), g))
            if not segs:   # two adjacent negatives: one segment across the face
                cr = [_edge(cs[i], cs[(i + 1) % 4]) for i in range(4) if neg[cs[i]] != neg[cs[(i + 1) % 4]]]
                g = CORNERS[[c for c in cs if not neg[c]]].mean(0) - CORNERS[[c for c in cs if neg[c]]].mean(0)
                segs.append((cr[0], cr[1], g))
            for e1, e2, g in segs:
                if np.dot(mid[e2] - mid[e1], np.cross(g, np.array(n, float))) < 0:
                    e1, e2 = e2, e1
                nxt[e1] = e2
        tris = []
        while nxt:
            s = min(nxt)
            loop, e = [s], nxt.pop(s)
            while e != s:
                loop.append(e)
                e = nxt.pop(e)
            tris += [(loop[0], loop[i], loop[i + 1]) for i in range(1, len(loop) - 1)]
        table.append(tuple(tris))
    return tuple(table)


TRI_TABLE = _build_tri_table()
MAX_TRIS = max(len(t) for t in TRI_TABLE)   # 5


# ---- views --------------------------------------------------------------------------------------------------------------
def make_view(depth, rgb, fx, fy, cx, cy, extrinsic, depth_trunc):
    """One staged view: sanitised f32 depth (H, W), uint8 colour (H, W, 3), f32 intrinsics, E and c2w (f32 3x4 rows)."""
    d = np.array(depth, dtype=f32).reshape(np.shape(depth)[0], np.shape(depth)[1])
    with np.errstate(invalid="ignore"):
        d = np.where(np.isfinite(d) & (d > 0) & (d <= f32(depth_trunc)), d, f32(0)).astype(f32)
    rgb = np.asarray(rgb)
    if rgb.dtype == np.uint8:
        c = rgb
    else:   # truncate, then clip to 0..255; NaN gives 0 (astype(uint8) alone is undefined out of range)
        with np.errstate(invalid="ignore", over="ignore"):
            p = rgb.astype(f32) * f32(255)
            c = np.where(np.isnan(p), f32(0), np.clip(np.trunc(p), f32(0), f32(255))).astype(np.uint8)
    E = np.asarray(extrinsic, dtype=np.float64)
    return dict(depth=d, rgb=c.reshape(d.shape[0], d.shape[1], 3), fx=f32(fx), fy=f32(fy), cx=f32(cx), cy=f32(cy),
                E=E.astype(f32), c2w=np.linalg.inv(E).astype(f32))


def _mat(M, x, y, z):
    return M[0] * x + M[1] * y + M[2] * z + M[3]


# ---- allocation ---------------------------------------------------------------------------------------------------------
def allocate(views, voxel, trunc, R=16, stride=4):
    """Sorted (nb, 3) int block coordinates (x, y, z) in (bz, by, bx) order and the (nb, V) bool touched-by-view matrix."""
    voxel, trunc = f32(voxel), f32(trunc)
    L = f32(R) * voxel
    touched = {}
    for k, v in enumerate(views):
        d = v["depth"][::stride, ::stride]
        vv, uu = np.nonzero(d > 0)
        d = d[vv, uu]
        u, w = (uu * stride).astype(f32), (vv * stride).astype(f32)
        qx, qy = (u - v["cx"]) * d / v["fx"], (w - v["cy"]) * d / v["fy"]
        M = v["c2w"]
        p = [_mat(M[i], qx, qy, d) for i in range(3)]
        lo = [np.floor((p[i] - trunc) / L).astype(np.int64) for i in range(3)]
        hi = [np.floor((p[i] + trunc) / L).astype(np.int64) for i in range(3)]
        span = max(int((hi[i] - lo[i]).max(initial=0)) for i in range(3))
        keys = set()
        for dz in range(span + 1):
            for dy in range(span + 1):
                for dx in range(span + 1):
                    bx, by, bz = lo[0] + dx, lo[1] + dy, lo[2] + dz
                    ok = (bx <= hi[0]) & (by <= hi[1]) & (bz <= hi[2])
                    keys.update(zip(bx[ok].tolist(), by[ok].tolist(), bz[ok].tolist()))
        for key in keys:
            touched.setdefault(key, set()).add(k)
    blocks = sorted(touched, key=lambda b: (b[2], b[1], b[0]))
    mask = np.zeros((len(blocks), len(views)), bool)
    for i, b in enumerate(blocks):
        mask[i, sorted(touched[b])] = True
    return np.array(blocks, np.int64).reshape(-1, 3), mask


# ---- integration --------------------------------------------------------------------------------------------------------
def _local(R):
    i = np.arange(R ** 3)
    return np.stack([i % R, (i // R) % R, i // (R * R)], 1)   # x fastest


def integrate(views, blocks, mask, voxel, trunc, R=16):
    """(T, W, C): (nb, R^3), (nb, R^3), (nb, R^3, 3) f32, colour in 0..255."""
    voxel, trunc = f32(voxel), f32(trunc)
    inv_trunc = f32(1) / trunc
    nb, n = len(blocks), R ** 3
    T = np.zeros((nb, n), f32)
    Wt = np.zeros((nb, n), f32)
    C = np.zeros((nb, n, 3), f32)
    loc = _local(R)
    for k, v in enumerate(views):
        sel = np.nonzero(mask[:, k])[0]
        if len(sel) == 0:
            continue
        g = blocks[sel][:, None, :] * R + loc[None]                       # (s, n, 3)
        x = [(g[..., i].astype(f32) + f32(0.5)) * voxel for i in range(3)]
        E = v["E"]
        xc = [_mat(E[i], *x) for i in range(3)]
        z = xc[2]
        H, Wd = v["depth"].shape
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            uf = np.floor(xc[0] * v["fx"] / z + v["cx"] + f32(0.5))
            vf = np.floor(xc[1] * v["fy"] / z + v["cy"] + f32(0.5))
            ok = (z > 0) & (uf >= 0) & (uf < Wd) & (vf >= 0) & (vf < H)
        ui = np.where(ok, uf, 0).astype(np.int64)
        vi = np.where(ok, vf, 0).astype(np.int64)
        d = v["depth"][vi, ui]
        ok &= d > 0
        a = (ui.astype(f32) - v["cx"]) / v["fx"]
        b = (vi.astype(f32) - v["cy"]) / v["fy"]
        with np.errstate(invalid="ignore", over="ignore"):
            sdf = (d - z) * np.sqrt(f32(1) + a * a + b * b)
            ok &= sdf > -trunc
        t = np.minimum(f32(1), sdf * inv_trunc)
        col = v["rgb"][vi, ui].astype(f32)
        Tb, Wb, Cb = T[sel], Wt[sel], C[sel]
        wn = Wb + f32(1)
        Tn = (Tb * Wb + t) / wn
        Cn = (Cb * Wb[..., None] + col) / wn[..., None]
        T[sel] = np.where(ok, Tn, Tb)
        C[sel] = np.where(ok[..., None], Cn, Cb)
        Wt[sel] = np.where(ok, wn, Wb)
    return T, Wt, C


# ---- marching cubes -----------------------------------------------------------------------------------------------------
def _dense(blocks, T, Wt, C, R):
    """Dense padded volume over the blocks' bounding box (+1 voxel of weight 0 on the high side)."""
    lo = blocks.min(0)
    dims = (blocks.max(0) - lo + 1) * R + 1
    Td = np.zeros(dims[::-1], f32)
    Wd = np.zeros(dims[::-1], f32)
    Cd = np.zeros(tuple(dims[::-1]) + (3,), f32)
    loc = _local(R)
    for i, b in enumerate(blocks):
        o = (b - lo) * R
        Td[o[2] + loc[:, 2], o[1] + loc[:, 1], o[0] + loc[:, 0]] = T[i]
        Wd[o[2] + loc[:, 2], o[1] + loc[:, 1], o[0] + loc[:, 0]] = Wt[i]
        Cd[o[2] + loc[:, 2], o[1] + loc[:, 1], o[0] + loc[:, 0]] = C[i]
    return lo * R, Td, Wd, Cd


def extract(blocks, T, Wt, C, voxel, R=16):
    """(vertices f32 (V, 3), triangles int32 (F, 3), colours f32 (V, 3)) in the canonical order."""
    voxel = f32(voxel)
    if len(blocks) == 0:
        return np.zeros((0, 3), f32), np.zeros((0, 3), np.int32), np.zeros((0, 3), f32)
    g0, Td, Wd, Cd = _dense(blocks, T, Wt, C, R)
    Z, Y, X = Td.shape
    # per owning voxel (in canonical order): global index of every voxel of every block
    loc = _local(R)
    own = (blocks - blocks.min(0))[:, None, :] * R + loc[None]          # (nb, n, 3) dense coordinates
    own = own.reshape(-1, 3)

    def at(A, p, dflt=0):
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        ok = (x >= 0) & (y >= 0) & (z >= 0) & (x < X) & (y < Y) & (z < Z)
        out = np.full(len(p), dflt, A.dtype) if A.ndim == 3 else np.zeros((len(p), 3), A.dtype)
        out[ok] = A[z[ok], y[ok], x[ok]]
        return out

    def cube_valid(p):
        ok = np.ones(len(p), bool)
        for c in CORNERS:
            ok &= at(Wd, p + c) > 0
        return ok

    # vertices: per owning voxel, axes x < y < z
    Ta, Wa, Ca = at(Td, own), at(Wd, own), at(Cd, own)
    vid = np.full((len(own), 3), -1, np.int64)
    flags = np.zeros((len(own), 3), bool)
    for ax in range(3):
        e = np.zeros(3, np.int64)
        e[ax] = 1
        Tb, Wb = at(Td, own + e), at(Wd, own + e)
        f = (Wa > 0) & (Wb > 0) & ((Ta < 0) != (Tb < 0))
        j, k = [a for a in range(3) if a != ax]
        anyv = np.zeros(len(own), bool)
        for dj in (0, 1):
            for dk in (0, 1):
                o = np.zeros(3, np.int64)
                o[j], o[k] = -dj, -dk
                anyv |= cube_valid(own + o)
        flags[:, ax] = f & anyv
    vid[flags] = np.arange(int(flags.sum()))
    oi, ax = np.nonzero(flags)
    pa = own[oi]
    pb = pa + np.eye(3, dtype=np.int64)[ax]
    ta, tb = np.abs(at(Td, pa)), np.abs(at(Td, pb))
    ca, cb = at(Cd, pa), at(Cd, pb)
    gpos = pa + g0
    verts = np.stack([(gpos[:, i].astype(f32) + f32(0.5)) * voxel for i in range(3)], 1)
    s = ta + tb
    r = ta / s
    verts[np.arange(len(oi)), ax] = verts[np.arange(len(oi)), ax] + r * voxel
    cols = ((tb[:, None] * ca + ta[:, None] * cb) / s[:, None]) / f32(255)
    # triangles: per cube (same order as the owning voxels), table slots in order
    valid = cube_valid(own)
    case = np.zeros(len(own), np.int64)
    for i, c in enumerate(CORNERS):
        case |= (at(Td, own + c) < 0).astype(np.int64) << i
    index = {tuple(p): i for i, p in enumerate(own.tolist())}
    tris = []
    for ci in np.nonzero(valid & (case != 0) & (case != 255))[0]:
        for tri in TRI_TABLE[case[ci]]:
            t = []
            for e in tri:
                o = own[ci] + np.array(EDGE_OFFSET[e])
                t.append(vid[index[tuple(o.tolist())], EDGE_AXIS[e]])
            tris.append(t)
    tris = np.array(tris, np.int64).reshape(-1, 3)
    assert (tris >= 0).all()
    return verts.astype(f32), tris.astype(np.int32), cols.astype(f32)


# ---- post-processing ----------------------------------------------------------------------------------------------------
def crop(verts, tris, aabb):
    aabb = np.asarray(aabb, np.float64).reshape(2, 3)
    v = verts.astype(np.float64)
    outside = ~((v >= aabb[0]).all(-1) & (v <= aabb[1]).all(-1))
    return tris[~outside[tris].any(-1)] if len(tris) else tris


def clusters(tris, n_verts):
    """(per-triangle cluster label numbered by the cluster's smallest triangle index, per-cluster counts)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    F = len(tris)
    if F == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    a = np.concatenate([tris[:, 0], tris[:, 1], tris[:, 2]]).astype(np.int64)
    b = np.concatenate([tris[:, 1], tris[:, 2], tris[:, 0]]).astype(np.int64)
    key = np.minimum(a, b) * n_verts + np.maximum(a, b)
    tid = np.tile(np.arange(F), 3)
    order = np.argsort(key, kind="stable")
    k, t = key[order], tid[order]
    same = k[1:] == k[:-1]
    g = coo_matrix((np.ones(int(same.sum())), (t[1:][same], t[:-1][same])), shape=(F, F))
    _, lab = connected_components(g, directed=False)
    first = np.full(lab.max() + 1, F)
    np.minimum.at(first, lab, np.arange(F))
    rank = np.argsort(np.argsort(first))
    lab = rank[lab]
    return lab, np.bincount(lab)


def keep_mask(counts, k=10):
    counts = np.asarray(counts)
    if len(counts) == 0:
        return np.zeros(0, bool)
    n = np.sort(counts)[-min(len(counts), k)]
    return counts >= n


def remove_unreferenced(verts, cols, tris):
    used = np.zeros(len(verts), bool)
    used[tris.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    return verts[used], cols[used], remap[tris].astype(np.int32)


def postprocess(verts, tris, cols, aabb=None):
    if aabb is not None:
        tris = crop(verts, tris, aabb)
    lab, cnt = clusters(tris, len(verts))
    tris = tris[keep_mask(cnt)[lab]] if len(tris) else tris
    return remove_unreferenced(verts, cols, tris)


def fuse(views, voxel, trunc, R=16, stride=4):
    blocks, mask = allocate(views, voxel, trunc, R, stride)
    T, Wt, C = integrate(views, blocks, mask, voxel, trunc, R)
    return blocks, mask, T, Wt, C


# ---- analytic test scene ------------------------------------------------------------------------------------------------
def sphere_depth(c2w, fx, fy, cx, cy, H, W, radius, centre=(0.0, 0.0, 0.0)):
    """(H, W) f32 view depth (camera z) of the pixel-centre rays hitting a sphere, 0 where they miss (f64 intersection)."""
    c2w = np.asarray(c2w, np.float64)
    u, v = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1) @ c2w[:3, :3].T
    o = c2w[:3, 3] - np.asarray(centre, np.float64)
    a, b, c = (d * d).sum(-1), d @ o, o @ o - radius * radius
    disc = b * b - a * c
    t = (-b - np.sqrt(np.maximum(disc, 0))) / a
    return np.where(disc > 0, t, 0).astype(f32)


def mesh_checks(verts, tris, radius, voxel):
    """The geometric bars of the sphere tests: (max | |v| - r | / voxel, max triangles per edge, outward share, clusters)."""
    r_err = float(np.abs(np.linalg.norm(verts.astype(np.float64), axis=1) - radius).max()) / voxel
    t = tris.astype(np.int64)
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), 1)
    _, per_edge = np.unique(e, axis=0, return_counts=True)
    v = verts.astype(np.float64)
    n = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    outward = float((np.einsum("ij,ij->i", n, v[t].mean(1)) > 0).mean())
    _, counts = clusters(tris, len(verts))
    return r_err, int(per_edge.max()), outward, len(counts)
