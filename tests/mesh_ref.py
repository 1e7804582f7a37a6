"""Float64 numpy reference of the mesh overlay's contract, written straight from the formulas: test
infrastructure only, the product never imports it.

rasterize_ref solves the 3x3 clip-space barycentric system per (pixel, triangle) inside the triangle's pixel bbox; antialias_ref applies
the analytic silhouette blend pair by pair.  edge_neighbours_ref is the brute-force dictionary form of the edge adjacency."""
from __future__ import annotations

import math
from collections import defaultdict

import numpy as np


def pixel_ndc(H, W):
    """NDC of the pixel centres: (px[x], py[y]) = ((2x+1)/W - 1, (2y+1)/H - 1); row 0 is NDC y = -1."""
    return (2.0 * np.arange(W) + 1.0) / W - 1.0, (2.0 * np.arange(H) + 1.0) / H - 1.0


def _bbox(Cv, H, W):
    """Pixel range that holds every covered pixel centre: the projected vertices' box (plus a pixel), or the image when a w <= 0."""
    if np.all(Cv[:, 3] > 0):
        X = (Cv[:, 0] / Cv[:, 3] + 1.0) * 0.5 * W - 0.5
        Y = (Cv[:, 1] / Cv[:, 3] + 1.0) * 0.5 * H - 0.5
        x0, x1 = max(math.floor(X.min()) - 1, 0), min(math.ceil(X.max()) + 1, W - 1)
        y0, y1 = max(math.floor(Y.min()) - 1, 0), min(math.ceil(Y.max()) + 1, H - 1)
        return x0, x1, y0, y1
    return 0, W - 1, 0, H - 1


def rasterize_ref(pos, tri, H, W):
    """pos (B,V,4), tri (F,3) -> dict of (B,H,W) arrays: id (triangle index, -1 empty), u, v, z (float64), bmin (the winner's smallest
    barycentric), gap (second-smallest minus smallest covering depth, inf with one layer), and rast (B,H,W,4) float32 in the product's
    layout."""
    pos = np.asarray(pos, np.float64)
    tri = np.asarray(tri, np.int64)
    B = pos.shape[0]
    pxs, pys = pixel_ndc(H, W)
    out = {k: np.zeros((B, H, W)) for k in ("u", "v", "z")}
    out["id"] = np.full((B, H, W), -1, np.int64)
    out["bmin"] = np.full((B, H, W), np.inf)
    best = np.full((B, H, W), np.inf)
    second = np.full((B, H, W), np.inf)
    for b in range(B):
        for t in range(tri.shape[0]):
            Cv = pos[b, tri[t]]                       # (3, 4) clip-space vertices
            if not np.all(np.isfinite(Cv)):
                continue
            M = np.stack([Cv[:, 0], Cv[:, 1], Cv[:, 3]])   # columns: (x, y, w) of each vertex
            if np.linalg.det(M) == 0.0:
                continue
            x0, x1, y0, y1 = _bbox(Cv, H, W)
            if x0 > x1 or y0 > y1:
                continue
            PX, PY = np.meshgrid(pxs[x0:x1 + 1], pys[y0:y1 + 1])
            # sum b_i = 1, sum b_i (x_i - px w_i) = 0, sum b_i (y_i - py w_i) = 0
            A = np.empty(PX.shape + (3, 3))
            A[..., 0, :] = 1.0
            A[..., 1, :] = Cv[:, 0] - PX[..., None] * Cv[:, 3]
            A[..., 2, :] = Cv[:, 1] - PY[..., None] * Cv[:, 3]
            rhs = np.broadcast_to(np.array([1.0, 0.0, 0.0]), PX.shape + (3,))
            with np.errstate(all="ignore"):
                ok = np.abs(np.linalg.det(A)) > 0
                bary = np.zeros(PX.shape + (3,))
                bary[ok] = np.linalg.solve(A[ok], rhs[ok][..., None])[..., 0]
                c = bary @ Cv                              # (h, w, 4)
                z = c[..., 2] / c[..., 3]
            cov = ok & np.all(bary >= 0, -1) & (c[..., 3] > 0) & (-c[..., 3] <= c[..., 2]) & (c[..., 2] <= c[..., 3])
            sl = (b, slice(y0, y1 + 1), slice(x0, x1 + 1))
            bst, sec = best[sl], second[sl]
            upd = cov & (z < bst)                         # strict: on an exact tie the lower index (earlier t) stays
            sec[...] = np.where(upd, bst, np.where(cov, np.minimum(sec, z), sec))
            bst[...] = np.where(upd, z, bst)
            for k, val in (("id", t), ("u", bary[..., 0]), ("v", bary[..., 1]), ("z", z), ("bmin", bary.min(-1))):
                view = out[k][sl]
                view[...] = np.where(upd, val, view)
    with np.errstate(invalid="ignore"):
        out["gap"] = second - best                    # nan (not < eps) where nothing covers
    rast = np.zeros((B, H, W, 4), np.float32)
    m = out["id"] >= 0
    rast[..., 0][m], rast[..., 1][m], rast[..., 2][m] = out["u"][m], out["v"][m], out["z"][m]
    rast[..., 3][m] = out["id"][m] + 1
    out["rast"] = rast
    return out


def ambiguous(ref, bmin_eps=1e-5, gap_eps=1e-6):
    """Pixels whose winner is not well defined in float arithmetic: on an edge, or two depths within gap_eps."""
    return ((ref["id"] >= 0) & (ref["bmin"] < bmin_eps)) | (ref["gap"] < gap_eps)


def edge_neighbours_ref(tri):
    """(F,3): for edge k = (tri[f,k], tri[f,(k+1)%3]) the other triangle on it, -1 boundary, -2 shared by more than two triangles."""
    tri = np.asarray(tri, np.int64)
    owners = defaultdict(list)
    for f, t in enumerate(tri):
        for k in range(3):
            a, b = int(t[k]), int(t[(k + 1) % 3])
            owners[(min(a, b), max(a, b))].append(f)
    nb = np.full(tri.shape, -1, np.int64)
    for f, t in enumerate(tri):
        for k in range(3):
            a, b = int(t[k]), int(t[(k + 1) % 3])
            o = owners[(min(a, b), max(a, b))]
            nb[f, k] = -1 if len(o) == 1 else (-2 if len(o) > 2 else (o[0] if o[1] == f else o[1]))
    return nb


def _orient(pos_b, tri):
    Cv = pos_b[tri]                                   # (F, 3, 4)
    M = np.stack([Cv[..., 0], Cv[..., 1], Cv[..., 3]], -2)
    return np.sign(np.linalg.det(M))


def antialias_ref(color, rast, pos, tri, neighbours):
    """color (B,H,W,C), rast (B,H,W,4) -> (B,H,W,C) float64.  Deltas are summed per pixel in the order left, right, below (y-1),
    above (y+1); pixels without a qualifying pair are returned unchanged."""
    color = np.asarray(color, np.float64)
    rast = np.asarray(rast, np.float64)
    pos = np.asarray(pos, np.float64)
    tri = np.asarray(tri, np.int64)
    nbr = np.asarray(neighbours, np.int64)
    B, H, W, _ = color.shape
    F = tri.shape[0]
    out = color.copy()
    wv = rast[..., 3]
    ids = np.where((wv >= 1) & (wv <= F) & (wv == np.floor(wv)), wv - 1, -1).astype(np.int64)
    for b in range(B):
        orient = _orient(pos[b], tri) if F else np.zeros(0)
        for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)):   # the summation order
            ys, xs = np.mgrid[0:H, 0:W]
            xn, yn = xs + dx, ys + dy
            inside = (xn >= 0) & (xn < W) & (yn >= 0) & (yn < H)
            ys, xs, xn, yn = ys[inside], xs[inside], xn[inside], yn[inside]
            ia, ib = ids[b, ys, xs], ids[b, yn, xn]
            sel = ia != ib
            ys, xs, xn, yn, ia, ib = ys[sel], xs[sel], xn[sel], yn[sel], ia[sel], ib[sel]
            za, zb = rast[b, ys, xs, 2], rast[b, yn, xn, 2]
            me_front = (ib < 0) | ((ia >= 0) & ((za < zb) | ((za == zb) & (ia < ib))))
            f = np.where(me_front, ia, ib)
            xp, yp = np.where(me_front, xs, xn), np.where(me_front, ys, yn)
            xq, yq = np.where(me_front, xn, xs), np.where(me_front, yn, ys)
            t = np.full(f.shape, np.nan)
            for k in range(3):                              # first qualifying edge: v0v1, v1v2, v2v0
                todo = np.isnan(t)
                A, Cc = pos[b, tri[f, k]], pos[b, tri[f, (k + 1) % 3]]
                nb = nbr[f, k]
                sil = (nb < 0) | (orient[f] * orient[np.maximum(nb, 0)] < 0)
                use = todo & sil & (A[:, 3] > 0) & (Cc[:, 3] > 0)
                with np.errstate(all="ignore"):
                    ax, ay = (A[:, 0] / A[:, 3] + 1) * 0.5 * W - 0.5, (A[:, 1] / A[:, 3] + 1) * 0.5 * H - 0.5
                    cx, cy = (Cc[:, 0] / Cc[:, 3] + 1) * 0.5 * W - 0.5, (Cc[:, 1] / Cc[:, 3] + 1) * 0.5 * H - 0.5
                    horiz = yp == yq
                    a_al, a_ac = np.where(horiz, ax, ay), np.where(horiz, ay, ax)
                    c_al, c_ac = np.where(horiz, cx, cy), np.where(horiz, cy, cx)
                    p_al, q_al, line = np.where(horiz, xp, yp), np.where(horiz, xq, yq), np.where(horiz, yp, xp)
                    s = (line - a_ac) / (c_ac - a_ac)
                    tt = (a_al + s * (c_al - a_al) - p_al) / (q_al - p_al)
                ok = use & (c_ac != a_ac) & (s >= 0) & (s <= 1) & (tt >= 0) & (tt <= 1)
                t = np.where(ok, tt, t)
            hit = ~np.isnan(t)
            cs, cn = color[b, ys, xs], color[b, yn, xn]
            wgt = np.where(me_front & (t < 0.5), 0.5 - t, np.where(~me_front & (t > 0.5), t - 0.5, 0.0))
            wgt = np.where(hit, wgt, 0.0)
            out[b, ys, xs] += wgt[:, None] * (cn - cs)
    return out
