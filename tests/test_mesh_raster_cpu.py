"""CPU tests of the mesh overlay (gaussianavatars_amd.mesh_raster, include/gmr.h): the float64 reference against analytic cases, the edge
adjacency builder against a brute-force dictionary, every argument check on host tensors, and the library's C ABI.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import mesh_cases as MC
import mesh_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference against analytic cases -------------------------------------------------------------------------------------------
def _inside_2d(P, x, y):
    (x0, y0), (x1, y1), (x2, y2) = P
    d = lambda ax, ay, bx, by, px, py: (bx - ax) * (py - ay) - (by - ay) * (px - ax)
    s = [d(x0, y0, x1, y1, x, y), d(x1, y1, x2, y2, x, y), d(x2, y2, x0, y0, x, y)]
    return (min(s) > 1e-9) or (max(s) < -1e-9)


def test_ref_flat_triangle_coverage_and_linear_uv():
    pos, tri = MC.flat_triangle()
    H, W = 24, 32
    r = R.rasterize_ref(pos, tri, H, W)
    pxs, pys = R.pixel_ndc(H, W)
    P = pos[0, :, :2].astype(np.float64)
    for y in range(H):
        for x in range(W):
            if _inside_2d(P, pxs[x], pys[y]):
                assert r["id"][0, y, x] == 0
                # w = 1: (u, v) are the 2D barycentrics of the pixel centre
                T = np.array([[P[0, 0], P[1, 0], P[2, 0]], [P[0, 1], P[1, 1], P[2, 1]], [1, 1, 1]])
                b = np.linalg.solve(T, [pxs[x], pys[y], 1.0])
                assert abs(r["u"][0, y, x] - b[0]) < 1e-12 and abs(r["v"][0, y, x] - b[1]) < 1e-12 and r["z"][0, y, x] == 0
            elif r["id"][0, y, x] == 0:
                assert r["bmin"][0, y, x] < 1e-9     # only on the boundary
    assert (r["rast"][..., 3] == 1).sum() == (r["id"] == 0).sum() > 50
    assert np.all(r["rast"][r["id"] < 0] == 0)


def test_ref_perspective_triangle_is_perspective_correct():
    pos, tri = MC.perspective_triangle()
    H, W = 24, 32
    r = R.rasterize_ref(pos, tri, H, W)
    pxs, pys = R.pixel_ndc(H, W)
    Cv = pos[0].astype(np.float64)
    ys, xs = np.nonzero(r["id"][0] == 0)
    assert len(ys) > 30
    for y, x in zip(ys, xs):
        u, v = r["u"][0, y, x], r["v"][0, y, x]
        c = u * Cv[0] + v * Cv[1] + (1 - u - v) * Cv[2]       # the clip-space point projects to the pixel centre
        assert abs(c[0] / c[3] - pxs[x]) < 1e-12 and abs(c[1] / c[3] - pys[y]) < 1e-12
        assert abs(c[2] / c[3] - r["z"][0, y, x]) < 1e-12
    # not affine in NDC: the screen-space barycentric differs from u somewhere by a lot
    assert np.ptp(r["u"][0][r["id"][0] == 0]) > 0.3


def test_ref_quad_through_w0_draws_only_the_front_part():
    pos, tri = MC.quad_crossing_w0()
    H, W = 24, 32
    r = R.rasterize_ref(pos, tri, H, W)
    cov = r["id"][0] >= 0
    assert 0 < cov.sum() < H * W
    # the plane y_clip = -0.2 with w > 0 projects below NDC y = -0.1 only: rows above are empty
    pxs, pys = R.pixel_ndc(H, W)
    assert not cov[pys > -0.1].any() and cov[pys < -0.3].all()
    assert np.all(np.abs(r["z"][0][cov]) <= 1)


def test_ref_near_and_far_planes_clip_per_pixel():
    pos, tri = MC.near_far_clipped()
    H, W = 24, 32
    r = R.rasterize_ref(pos, tri, H, W)
    full = R.rasterize_ref(np.concatenate([pos[..., :2], np.zeros_like(pos[..., :1]), pos[..., 3:]], -1), tri, H, W)
    for t in (0, 1):
        assert 0 < (r["id"] == t).sum() < (full["id"] == t).sum()     # clipped, but not away
    cov = r["id"] >= 0
    assert np.all(np.abs(r["z"][cov]) <= 1)


def test_ref_interpenetrating_triangles_switch_at_the_intersection():
    pos, tri = MC.interpenetrating()
    H, W = 24, 32
    r = R.rasterize_ref(pos, tri, H, W)
    assert (r["id"] == 0).sum() > 20 and (r["id"] == 1).sum() > 20
    # where both cover, the winner is the nearer one
    pxs, pys = R.pixel_ndc(H, W)
    for t in (0, 1):
        other = R.rasterize_ref(pos, tri[[1 - t]], H, W)
        both = (r["id"] >= 0) & (other["id"] == 0)
        assert both.any()
        z_other = other["z"][both]
        assert np.all(r["z"][both] <= z_other)


def test_ref_back_face_rasterizes():
    pos, tri = MC.back_face()
    r = R.rasterize_ref(pos, tri, 24, 32)
    f = R.rasterize_ref(*MC.flat_triangle(), 24, 32)
    assert np.array_equal(r["id"] >= 0, f["id"] >= 0) and (r["id"] >= 0).sum() > 50


def test_ref_antialias_vertical_edge_blends_by_the_covered_fraction():
    pos, tri, H, W = MC.vertical_edge()
    r = R.rasterize_ref(pos, tri, H, W)
    assert np.all(r["id"][0, :, :10] < 0) and np.all(r["id"][0, :, 10:] >= 0)
    color = np.zeros((1, H, W, 2))
    color[..., 0] = np.where(r["id"] >= 0, 1.0, 0.0)[0]
    color[..., 1] = 5.0
    out = R.antialias_ref(color, r["rast"], pos, tri, R.edge_neighbours_ref(tri))
    assert np.allclose(out[0, :, 10, 0], 0.7, atol=1e-12)          # pixel 10 is 0.7 covered
    assert np.array_equal(out[0, :, 9, 0], color[0, :, 9, 0])     # t = 0.2 < 0.5: Q unchanged
    mask = np.ones(W, bool)
    mask[10] = False
    assert np.array_equal(out[0][:, mask], color[0][:, mask])
    assert np.array_equal(out[..., 1], color[..., 1])              # a constant channel stays constant


# ---- edge adjacency ------------------------------------------------------------------------------------------------------------------
def test_edge_neighbours_match_the_dictionary_on_the_head_mesh():
    from gaussianavatars_amd import mesh_raster
    from gaussianavatars_amd import synthetic as S

    verts, faces = S.head_mesh()
    tri = torch.from_numpy(faces.astype(np.int32))
    got = mesh_raster.edge_neighbours(tri, verts.shape[0])
    want = R.edge_neighbours_ref(faces)
    assert got.dtype == torch.int32 and tuple(got.shape) == (faces.shape[0], 3)
    assert np.array_equal(got.numpy(), want)
    assert (want == -1).sum() > 0      # the neck hole: boundary edges


def test_edge_neighbours_non_manifold_fan():
    from gaussianavatars_amd import mesh_raster

    # three triangles on the edge (0, 1), one more on (1, 2) of the first
    faces = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4], [2, 1, 5]], np.int32)
    got = mesh_raster.edge_neighbours(torch.from_numpy(faces), 6).numpy()
    want = R.edge_neighbours_ref(faces)
    assert np.array_equal(got, want)
    assert got[0, 0] == got[1, 0] == got[2, 0] == -2
    assert got[0, 1] == 3 and got[3, 0] == 0
    assert mesh_raster.edge_neighbours(torch.zeros((0, 3), dtype=torch.int32), 0).shape == (0, 3)


# ---- argument checks, on host tensors ------------------------------------------------------------------------------------------------
def _ok():
    pos = torch.zeros(1, 3, 4)
    tri = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    return pos, tri


def test_rasterize_argument_checks():
    from gaussianavatars_amd.mesh_raster import rasterize

    pos, tri = _ok()
    cases = [
        (dict(pos=pos.double()), TypeError, "float32"),
        (dict(pos=pos[0]), ValueError, "range mode"),
        (dict(pos=pos[None]), ValueError, "rank 3"),
        (dict(pos=torch.zeros(1, 3, 3)), ValueError, r"\(B, V, 4\)"),
        (dict(tri=tri.long()), TypeError, "int32"),
        (dict(tri=tri[0]), ValueError, "rank 2"),
        (dict(tri=torch.tensor([[0, 1, 3]], dtype=torch.int32)), ValueError, "outside"),
        (dict(tri=torch.tensor([[0, -1, 2]], dtype=torch.int32)), ValueError, "outside"),
        (dict(tri=torch.zeros(1, 3, dtype=torch.int32).expand(1 << 24, 3)), ValueError, "2\\^24"),
        (dict(ranges=torch.zeros(1, 2, dtype=torch.int32)), ValueError, "range mode"),
        (dict(resolution=(0, 8)), ValueError, "at least 1"),
        (dict(resolution=(8, -1)), ValueError, "at least 1"),
        (dict(resolution=(1 << 16, 1 << 15)), ValueError, "2\\^31"),
        (dict(resolution="ab"), TypeError, "resolution"),
        (dict(pos="x"), TypeError, "torch.Tensor"),
        (dict(), ValueError, "CUDA"),     # everything else valid: the host tensor is refused last
    ]
    for kw, exc, msg in cases:
        args = dict(pos=pos, tri=tri, resolution=(8, 8), ranges=None)
        args.update(kw)
        with pytest.raises(exc, match=msg):
            rasterize(None, args["pos"], args["tri"], args["resolution"], ranges=args["ranges"])
    with pytest.raises(ValueError, match="2\\^31"):
        rasterize(None, torch.zeros(4, 3, 4), tri, (1 << 14, 1 << 15))


def test_antialias_argument_checks():
    from gaussianavatars_amd.mesh_raster import antialias

    pos, tri = _ok()
    color, rast = torch.zeros(1, 8, 8, 3), torch.zeros(1, 8, 8, 4)
    cases = [
        (dict(topology_hash=object()), ValueError, "topology_hash"),
        (dict(color=color.half()), TypeError, "float32"),
        (dict(color=color[0]), ValueError, "rank 4"),
        (dict(color=torch.zeros(1, 8, 8, 0)), ValueError, "channel"),
        (dict(rast=torch.zeros(1, 8, 8, 3)), ValueError, "does not match"),
        (dict(rast=torch.zeros(1, 8, 9, 4)), ValueError, "does not match"),
        (dict(rast=rast.int()), TypeError, "float32"),
        (dict(pos=torch.zeros(2, 3, 4)), ValueError, "batch"),
        (dict(pos=pos[0]), ValueError, "range mode"),
        (dict(tri=torch.tensor([[0, 1, 5]], dtype=torch.int32)), ValueError, "outside"),
        (dict(tri=tri.long()), TypeError, "int32"),
        (dict(tri=torch.zeros(1, 3, dtype=torch.int32).expand(1 << 24, 3)), ValueError, "2\\^24"),
        (dict(), ValueError, "CUDA"),
    ]
    for kw, exc, msg in cases:
        args = dict(color=color, rast=rast, pos=pos, tri=tri, topology_hash=None)
        args.update(kw)
        with pytest.raises(exc, match=msg):
            antialias(args["color"], args["rast"], args["pos"], args["tri"], topology_hash=args["topology_hash"])


def test_shim_forwards_and_keeps_the_rest_raising():
    from gaussianavatars_amd import shims

    shims.install()
    import nvdiffrast.torch as dr

    dr.RasterizeCudaContext()
    dr.RasterizeGLContext()
    pos, tri = _ok()
    with pytest.raises(ValueError, match="CUDA"):      # reaches mesh_raster's checks, no longer a blanket RuntimeError
        dr.rasterize(dr.RasterizeCudaContext(), pos, tri, (8, 8))
    with pytest.raises(ValueError, match="topology_hash"):
        dr.antialias(torch.zeros(1, 8, 8, 4), torch.zeros(1, 8, 8, 4), pos, tri, topology_hash=1)
    for name in ("interpolate", "texture"):
        with pytest.raises(RuntimeError, match="CUDA-only"):
            getattr(dr, name)()


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_gmr_library_exports_every_declared_symbol():
    from gaussianavatars_amd import _lib

    txt = open(os.path.join(ROOT, "include", "gmr.h")).read()
    abi = int(re.search(r"#define\s+GMR_ABI_VERSION\s+(\d+)", txt).group(1))
    names = sorted(set(re.findall(r"\b(gmr_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))))
    assert len(names) == 5
    lib = _lib.gmr()
    for n in names:
        assert hasattr(lib, n) and n in _lib.GMR_SYMBOLS, n
    assert lib.gmr_abi_version() == _lib.GMR_ABI_VERSION == abi
    assert int(re.search(r"#define\s+GMR_MAX_TRIANGLES\s+(\d+)", txt).group(1)) == _lib.GMR_MAX_TRIANGLES
    # host-side argument checks of the C entry points (nothing is launched)
    assert lib.gmr_workspace_bytes(1, 10144) == 10144 * 7 * 16 + 40 * 16
    one = C.c_void_p(16)
    assert lib.gmr_rasterize(1, 3, 1, 0, 8, one, one, one, one, None) < 0 and b"bad arguments" in lib.gmr_last_error()
    assert lib.gmr_rasterize(1, 3, 1, 8, 8, None, one, one, one, None) < 0 and b"NULL" in lib.gmr_last_error()
    assert lib.gmr_antialias(1, 3, 1, 8, 8, 0, one, one, one, one, one, one, None) < 0 and b"bad arguments" in lib.gmr_last_error()
    assert lib.gmr_antialias(1, 3, 1, 8, 8, 4, one, one, one, one, one, one, None) < 0 and b"alias" in lib.gmr_last_error()


def test_mesh_raster_imports_neither_oracle_nor_tests():
    for f in ("mesh_raster.py", os.path.join("shims", "nvdiffrast", "torch.py")):
        txt = open(os.path.join(ROOT, "gaussianavatars_amd", f)).read()
        assert not re.search(r"^\s*(from|import)\s+(oracle|tests|mesh_ref|mesh_cases)\b", txt, flags=re.M), f
