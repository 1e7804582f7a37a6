"""Analytic inputs of the mesh overlay tests (tests/test_mesh_raster_cpu.py, tests/test_mesh_raster_gpu.py): clip-space vertices
(B=1, V, 4) float32 and int32 triangles."""
from __future__ import annotations

import numpy as np


def _clip(v):
    return np.asarray(v, np.float32)[None]


def flat_triangle():
    """w = 1, z = 0: coverage is the 2D triangle, (u, v) are linear in NDC."""
    return _clip([[-0.6, -0.5, 0.0, 1.0], [0.7, -0.4, 0.0, 1.0], [0.1, 0.6, 0.0, 1.0]]), np.array([[0, 1, 2]], np.int32)


def perspective_triangle():
    """Different w per vertex: (u, v) are perspective-correct (not linear in NDC), z/w varies."""
    return _clip([[-0.5, -0.5, 0.2, 1.0], [2.0, -1.0, 3.0, 4.0], [0.2, 1.2, 1.0, 2.0]]), np.array([[0, 1, 2]], np.int32)


def quad_crossing_w0():
    """A ground-plane quad from in front of the camera to behind it (w < 0): only the part with w > 0 and |z| <= w is drawn."""
    v = []
    for zc in (2.0, -2.0):      # camera-space depth: one edge in front of the camera, the other behind it
        for xc in (-1.0, 1.0):
            x, y, w = xc, -0.2, zc
            v.append([x, y, 0.9 * w - 0.1, w])   # z = a w + b: near plane at w ~ 0.1
    return _clip(v), np.array([[0, 1, 3], [0, 3, 2]], np.int32)


def near_far_clipped():
    """Two triangles whose depth runs through the near plane (z < -w) and through the far plane (z > w) inside the viewport."""
    v = [[-0.8, -0.8, -2.0, 1.0], [0.8, -0.8, 0.0, 1.0], [0.0, 0.8, 0.5, 1.0],
         [-0.8, 0.8, 2.0, 1.0], [0.8, 0.8, 0.0, 1.0], [0.0, -0.8, 0.5, 1.0]]
    return _clip(v), np.array([[0, 1, 2], [3, 4, 5]], np.int32)


def interpenetrating():
    """Two triangles that cross in depth: the winner switches along their intersection line."""
    v = [[-0.8, -0.6, -0.5, 1.0], [0.8, -0.6, 0.5, 1.0], [0.0, 0.8, 0.0, 1.0],
         [-0.8, 0.6, 0.513, 1.0], [0.8, 0.6, -0.487, 1.0], [0.0, -0.8, 0.013, 1.0]]
    return _clip(v), np.array([[0, 1, 2], [3, 4, 5]], np.int32)


def back_face():
    """The flat triangle with the opposite winding: no culling, it rasterizes the same."""
    pos, _ = flat_triangle()
    return pos, np.array([[0, 2, 1]], np.int32)


def vertical_edge(W=32, H=16, x_edge=10.3):
    """A w = 1 quad whose left edge is the vertical line x = x_edge in pixel units (pixel i spans [i, i + 1]), the background to its
    left: pixel 10 is covered by 0.7, so antialias blends it 0.3 towards pixel 9."""
    xn = x_edge * 2.0 / W - 1.0
    v = [[xn, -2.0, 0.0, 1.0], [3.0, -2.0, 0.0, 1.0], [3.0, 2.0, 0.0, 1.0], [xn, 2.0, 0.0, 1.0]]
    return _clip(v), np.array([[0, 1, 2], [0, 2, 3]], np.int32), H, W


def plane_grid(H, W, nx, ny, xs=None, ys=None):
    """A regular grid of nx * ny quads (two triangles each) spanning NDC x-coordinates xs and y-coordinates ys (default: the whole
    viewport, then beyond it by one cell), w = 1, z = 0."""
    xs = np.linspace(-1.0, 1.0, nx + 1) if xs is None else np.asarray(xs)
    ys = np.linspace(-1.0, 1.0, ny + 1) if ys is None else np.asarray(ys)
    X, Y = np.meshgrid(xs, ys)
    v = np.stack([X.ravel(), Y.ravel(), np.zeros(X.size), np.ones(X.size)], 1)
    idx = lambda i, j: j * len(xs) + i
    tri = []
    for j in range(len(ys) - 1):
        for i in range(len(xs) - 1):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i, j + 1), idx(i + 1, j + 1)
            tri += [(a, b, d), (a, d, c)] if (i + j) % 2 == 0 else [(a, b, c), (b, d, c)]
    return _clip(v), np.asarray(tri, np.int32)


ANALYTIC = {"flat": flat_triangle, "perspective": perspective_triangle, "quad_w0": quad_crossing_w0, "near_far": near_far_clipped,
            "interpenetrating": interpenetrating, "back_face": back_face}
