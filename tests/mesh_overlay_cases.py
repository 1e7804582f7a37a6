"""Inputs of the shaded mesh overlay tests (tests/test_mesh_overlay_cpu.py, tests/test_mesh_overlay_gpu.py) and of the generator of their
pins (tests/golden/make_mesh_overlay_pins.py): four small meshes, the case table and the exclusion mask.  Test infrastructure only.

Meshes (world space, sized to fill most of orbit_camera's 20 degree view from r = 1):
    cube          closed, 12 triangles
    pole_fan      an open cone: 9 triangles around one pole vertex
    non_manifold  three triangles on one edge (its adjacency entry is -2) and a fourth on another edge of the first
    head200       synthetic.head_mesh() decimated on its own lat/long grid: 13 of its rings x 8 of its segments and the pole, 200 faces

Each mesh is drawn under four of the sixteen combinations of (size, lighting, face colours, background kind); the four meshes together
cover all sixteen.  `through` is one more camera, so close to the cube that vertices lie behind it (w <= 0)."""
from __future__ import annotations

import numpy as np

SIZES = ((64, 48), (53, 77))                      # (W, H): no resize; renders 48 x 72 and resizes up
LIGHTS = ("constant", "front")
CONST_BG = [0.25, 0.5, 0.75]


def cube():
    s = 0.11
    v = np.array([[x, y, z] for x in (-s, s) for y in (-s, s) for z in (-s, s)], np.float32)   # index = 4 ix + 2 iy + iz
    f = [(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4), (1, 5, 7), (1, 7, 3)]
    return v, np.asarray(f, np.int64)


def pole_fan(n=9):
    v = [(0.0, 0.13, 0.02)]
    for j in range(n):
        a = 2 * np.pi * (j + 0.3) / n
        v.append((0.14 * np.cos(a), -0.09 + 0.02 * np.sin(3 * a), 0.14 * np.sin(a)))
    f = [(0, 1 + (j + 1) % n, 1 + j) for j in range(n)]
    return np.asarray(v, np.float32), np.asarray(f, np.int64)


def non_manifold():
    v = [(-0.02, -0.13, 0.0), (0.03, 0.13, 0.01), (0.15, 0.02, 0.05), (-0.14, 0.04, 0.08), (-0.05, -0.02, -0.15), (0.16, 0.14, -0.06)]
    f = [(0, 1, 2), (1, 0, 3), (0, 1, 4), (2, 1, 5)]
    return np.asarray(v, np.float32), np.asarray(f, np.int64)


def head200():
    from gaussianavatars_amd import synthetic as S

    verts, _ = S.head_mesh()
    rings, seg = 53, 97
    keep_r = np.round(np.linspace(1, rings - 2, 13)).astype(int)
    keep_s = np.round(np.arange(8) * seg / 8).astype(int)
    idx = [0] + [1 + (i - 1) * seg + j for i in keep_r for j in keep_s]
    v = verts[idx]
    ring = lambda i, j: 1 + i * 8 + (j % 8)
    f = [(0, ring(0, j + 1), ring(0, j)) for j in range(8)]
    for i in range(12):
        for j in range(8):
            a, b, c, d = ring(i, j), ring(i, j + 1), ring(i + 1, j), ring(i + 1, j + 1)
            f += [(a, b, d), (a, d, c)]
    f = np.asarray(f, np.int64)
    assert f.shape == (200, 3) and v.shape == (105, 3)
    return np.ascontiguousarray(v, np.float32), f


MESHES = {"cube": cube, "pole_fan": pole_fan, "non_manifold": non_manifold, "head200": head200}
# (yaw, pitch) of the orbit camera per mesh, chosen by make_mesh_overlay_pins.py's search: no ambiguous pixel at either size
POSES = {"cube": (27.0, -18.0), "pole_fan": (14.37, 21.61), "non_manifold": (-31.0, 9.0), "head200": (17.0, -11.0)}
THROUGH = dict(mesh="cube", r=0.16, yaw=23.0, pitch=-14.0, fovy=70.0)


def case_table():
    """[(name, mesh, size index, lighting, face colours?, image background?, through?)]"""
    out = []
    for m, mesh in enumerate(MESHES):
        for s in (0, 1):
            for l in (0, 1):
                c, g = s ^ (m & 1), l ^ (m >> 1)
                out.append((f"{mesh}-{SIZES[s][0]}x{SIZES[s][1]}-{LIGHTS[l]}-{'colors' if c else 'white'}-{'image' if g else 'const'}",
                            mesh, s, LIGHTS[l], bool(c), bool(g), False))
    out.append(("cube-through-64x48-front-colors-const", "cube", 0, "front", True, False, True))
    return out


def camera(name_or_through, W, H):
    from gaussianavatars_amd import synthetic as S

    if isinstance(name_or_through, dict):
        t = name_or_through
        return S.orbit_camera(W, H, r=t["r"], fovy_deg=t["fovy"], yaw_deg=t["yaw"], pitch_deg=t["pitch"])
    yaw, pitch = POSES[name_or_through]
    return S.orbit_camera(W, H, yaw_deg=yaw, pitch_deg=pitch)


def face_colors(F):
    """(1, F, 3): multiples of 1/16 in [1/16, 1], different per face and channel"""
    k = np.arange(F)[:, None] * np.array([3, 5, 7]) + np.array([1, 6, 11])
    return ((k % 16 + 1) / 16.0).astype(np.float32)[None]


def background_image(h, w):
    """(1, h, w, 3) at the render size: blocks of multiples of 1/8, not symmetric under a vertical or horizontal flip"""
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([((x // 4 + 3 * (y // 4) + c) % 8) / 8.0 for c in range(3)], -1)
    return img.astype(np.float32)[None]


def render_hw(W, H):
    return H // 8 * 8, W // 8 * 8


def excluded(amb, H, W):
    """Output pixels (H, W) left out of the comparison, from the ambiguity mask `amb` (h, w) of the float64 reference in render orientation
    (row 0 = NDC y -1): the ambiguous pixels and their 4-neighbours, flipped to image orientation, and with a resize every output pixel whose
    bilinear footprint (the two source rows x two source columns of align_corners=False sampling) touches one."""
    a = np.asarray(amb, bool)
    grown = a.copy()
    grown[1:] |= a[:-1]
    grown[:-1] |= a[1:]
    grown[:, 1:] |= a[:, :-1]
    grown[:, :-1] |= a[:, 1:]
    grown = grown[::-1]
    h, w = grown.shape
    if (h, w) == (H, W):
        return grown

    def taps(n_out, n_in):
        s = np.maximum((n_in / n_out) * (np.arange(n_out) + 0.5) - 0.5, 0.0)
        i0 = np.minimum(np.floor(s).astype(int), n_in - 1)
        return np.maximum(i0 - 1, 0), np.minimum(i0 + 2, n_in - 1)   # one more tap on either side: the index may round either way

    ylo, yhi = taps(H, h)
    xlo, xhi = taps(W, w)
    out = np.zeros((H, W), bool)
    for Y in range(H):
        rows = grown[ylo[Y]:yhi[Y] + 1].any(0)
        for X in range(W):
            out[Y, X] = rows[xlo[X]:xhi[X] + 1].any()
    return out
