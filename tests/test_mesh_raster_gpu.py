"""The mesh overlay on the MI355X (gaussianavatars_amd.mesh_raster, include/gmr.h) against the float64 reference of tests/mesh_ref.py:
rasterize on analytic cases and the FLAME-sized head mesh, watertightness, antialias on the GPU's own rast, determinism, the nvdiffrast
shim in the reference's call pattern, and the forward-only autograd node."""
import numpy as np
import pytest
import torch

import mesh_cases as MC
import mesh_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _raster(pos, tri, H, W):
    from gaussianavatars_amd import mesh_raster

    rast, db = mesh_raster.rasterize(None, _t(pos), _t(tri), (H, W))
    torch.cuda.synchronize()
    assert rast.shape == (pos.shape[0], H, W, 4) and rast.dtype == torch.float32 and db.shape == (pos.shape[0], H, W, 0)
    return rast.cpu().numpy()


def _compare(got, ref, what):
    """Ids equal except at ambiguous pixels (< 0.5 % of the image); where ids match u, v and z within 1e-6 (measured: 3e-8, the float32
    rounding of the output; the winner's values are evaluated in double)."""
    gid = np.rint(got[..., 3]).astype(np.int64) - 1
    assert np.array_equal(got[..., 3], gid + 1.0), what
    amb = R.ambiguous(ref)
    assert amb.mean() < 0.005, f"{what}: {amb.mean():.4f} of the pixels are ambiguous"
    bad = (gid != ref["id"]) & ~amb
    assert not bad.any(), f"{what}: {bad.sum()} unambiguous pixels with a different triangle, first at {np.argwhere(bad)[:3].tolist()}"
    m = (gid == ref["id"]) & (gid >= 0)
    assert np.all(got[~(gid >= 0)] == 0), f"{what}: empty pixels must be all zeros"
    if m.any():
        du = np.abs(got[..., 0][m] - ref["u"][m]).max()
        dv = np.abs(got[..., 1][m] - ref["v"][m]).max()
        dz = np.abs(got[..., 2][m] - ref["z"][m]).max()
        assert du <= 1e-6 and dv <= 1e-6 and dz <= 1e-6, f"{what}: max |du| {du:.2e} |dv| {dv:.2e} |dz| {dz:.2e}"
        return du, dv, dz
    return 0.0, 0.0, 0.0


def _head_clip(W, H, yaw=0.0, pitch=0.0):
    from gaussianavatars_amd import synthetic as S

    verts, faces = S.head_mesh()
    cam = S.orbit_camera(W, H, yaw_deg=yaw, pitch_deg=pitch)
    vh = np.concatenate([verts.astype(np.float32), np.ones((verts.shape[0], 1), np.float32)], 1)
    clip = (vh @ cam.full_proj_transform).astype(np.float32)   # row vectors: what world_to_clip's bmm computes
    return clip[None], faces.astype(np.int32)


@pytest.mark.parametrize("case", sorted(MC.ANALYTIC))
def test_rasterize_analytic_cases_match_the_reference(case):
    pos, tri = MC.ANALYTIC[case]()
    for H, W in ((24, 32), (37, 53)):
        _compare(_raster(pos, tri, H, W), R.rasterize_ref(pos, tri, H, W), f"{case} {H}x{W}")


@pytest.mark.parametrize("H,W", [(544, 800), (547, 801)])
def test_rasterize_head_mesh_matches_the_reference(H, W):
    pos, tri = _head_clip(W, H)
    assert tri.shape == (10144, 3) and pos.shape == (1, 5143, 4)
    ref = R.rasterize_ref(pos, tri, H, W)
    got = _raster(pos, tri, H, W)
    err = _compare(got, ref, f"head {H}x{W}")
    assert (ref["id"] >= 0).mean() > 0.2
    print(f"head {H}x{W}: ambiguous {R.ambiguous(ref).mean():.5f}, max |du| |dv| |dz| = {err[0]:.2e} {err[1]:.2e} {err[2]:.2e}")


def test_rasterize_batch_of_two_poses():
    H, W = 272, 400
    p0, tri = _head_clip(W, H, yaw=0.0)
    p1, _ = _head_clip(W, H, yaw=35.0, pitch=-15.0)
    pos = np.concatenate([p0, p1], 0)
    got = _raster(pos, tri, H, W)
    ref = R.rasterize_ref(pos, tri, H, W)
    _compare(got, ref, "B=2")
    assert not np.array_equal(got[0], got[1])
    assert np.array_equal(got[0], _raster(p0, tri, H, W)[0])   # batch elements are independent


def test_rasterize_one_triangle_over_2048_squared():
    H = W = 2048
    pos = np.array([[[-1.5, -1.5, -0.5, 1.0], [4.0, -1.5, 0.25, 1.0], [-1.5, 4.0, 0.5, 1.0]]], np.float32)
    got = _raster(pos, np.array([[0, 1, 2]], np.int32), H, W)
    assert np.all(got[..., 3] == 1.0)
    pxs, pys = R.pixel_ndc(H, W)
    X, Y = np.meshgrid(pxs, pys)
    T = np.array([[-1.5, 4.0, -1.5], [-1.5, -1.5, 4.0], [1.0, 1.0, 1.0]])
    b = np.linalg.solve(T, np.stack([X.ravel(), Y.ravel(), np.ones(X.size)]))   # w = 1: 2D barycentrics
    u, v = b[0].reshape(H, W), b[1].reshape(H, W)
    z = -0.5 * u + 0.25 * v + 0.5 * (1 - u - v)
    assert np.abs(got[0, ..., 0] - u).max() <= 1e-6 and np.abs(got[0, ..., 1] - v).max() <= 1e-6
    assert np.abs(got[0, ..., 2] - z).max() <= 1e-6


def test_rasterize_empty_inputs():
    got = _raster(np.zeros((1, 0, 4), np.float32), np.zeros((0, 3), np.int32), 40, 30)
    assert np.all(got == 0)
    off = np.array([[[2.0, 2.0, 0.0, 1.0], [3.0, 2.0, 0.0, 1.0], [2.0, 3.0, 0.0, 1.0],        # right of the viewport
                     [-0.5, -0.5, 0.0, -1.0], [0.5, -0.5, 0.0, -1.0], [0.0, 0.5, 0.0, -1.0],  # behind the camera
                     [-0.5, -0.5, 2.0, 1.0], [0.5, -0.5, 2.0, 1.0], [0.0, 0.5, 2.0, 1.0]]],   # beyond the far plane
                   np.float32)
    got = _raster(off, np.arange(9, dtype=np.int32).reshape(3, 3), 40, 30)
    assert np.all(got == 0)


def _grid_coords(n):
    """NDC grid lines for an n-pixel axis: alternately exactly on pixel centres and on pixel corners, and beyond the viewport at both ends."""
    cuts = np.unique(np.linspace(0, n - 1, max(n // 6, 3)).astype(int))
    xs = [(2.0 * c + 1.0) / n - 1.0 if i % 2 == 0 else 2.0 * c / n - 1.0 for i, c in enumerate(cuts[1:-1])]
    return np.array([-1.25] + xs + [1.25], np.float32)


@pytest.mark.parametrize("H,W", [(64, 64), (48, 80), (37, 53)])
def test_rasterize_is_watertight(H, W):
    xs, ys = _grid_coords(W), _grid_coords(H)
    pos, tri = MC.plane_grid(H, W, 0, 0, xs=xs, ys=ys)
    got = _raster(pos, tri, H, W)
    gid = np.rint(got[0, ..., 3]).astype(np.int64) - 1
    assert np.all(gid >= 0), f"{(gid < 0).sum()} holes"
    pxs, pys = R.pixel_ndc(H, W)
    P = pos[0].astype(np.float64)
    for y in range(H):
        for x in range(W):
            a, b, c = P[tri[gid[y, x]]]
            T = np.array([[a[0], b[0], c[0]], [a[1], b[1], c[1]], [1.0, 1.0, 1.0]])
            bc = np.linalg.solve(T, [pxs[x], pys[y], 1.0])
            # the grid's vertices are float32: "on the edge" holds to their rounding
            assert bc.min() >= -1e-6, f"pixel ({x}, {y}) given to triangle {gid[y, x]} whose closure does not contain it"


def _rgba_from_normals(pos, tri, rast):
    """The caller's RGBA: a face-normal shade on covered pixels, alpha 1; white background with alpha 0."""
    P = pos[0, :, :3].astype(np.float64)
    n = np.cross(P[tri[:, 1]] - P[tri[:, 0]], P[tri[:, 2]] - P[tri[:, 0]])
    n /= np.linalg.norm(n, axis=1, keepdims=True) + 1e-30
    gid = np.rint(rast[..., 3]).astype(np.int64) - 1
    rgb = 0.5 + 0.5 * n[np.maximum(gid, 0)]
    fg = (gid >= 0)[..., None]
    rgba = np.concatenate([np.where(fg, rgb, 1.0), fg.astype(np.float64)], -1)
    return rgba.astype(np.float32)


def test_antialias_matches_the_reference_on_the_gpu_rast():
    from gaussianavatars_amd import mesh_raster

    H, W = 544, 800
    pos, tri = _head_clip(W, H, yaw=20.0)
    rast = _raster(pos, tri, H, W)
    nb = R.edge_neighbours_ref(tri)
    rgba = _rgba_from_normals(pos, tri, rast)
    for color in (rgba, rgba[..., 1:2].copy()):
        out = mesh_raster.antialias(_t(color), _t(rast), _t(pos), _t(tri)).cpu().numpy()
        ref = R.antialias_ref(color, rast, pos, tri, nb)
        d = np.abs(out - ref).max()
        assert d <= 1e-5, f"C={color.shape[-1]}: max |diff| {d:.2e}"
        changed = np.any(ref != color, -1)
        assert changed.sum() > 50                         # the silhouette is blended
        assert np.array_equal(out[~changed], color[~changed])   # everything else is copied bit for bit
        print(f"antialias C={color.shape[-1]}: max |diff| {d:.2e}, {changed.sum()} pixels blended")


def test_antialias_leaves_a_viewport_filling_plane_unchanged():
    from gaussianavatars_amd import mesh_raster

    H, W = 48, 80
    pos, tri = MC.plane_grid(H, W, 0, 0, xs=_grid_coords(W), ys=_grid_coords(H))
    rast = _raster(pos, tri, H, W)
    color = np.random.default_rng(0).random((1, H, W, 3), np.float32)
    out = mesh_raster.antialias(_t(color), _t(rast), _t(pos), _t(tri)).cpu().numpy()
    assert np.array_equal(out, color)


def test_rasterize_and_antialias_are_deterministic():
    from gaussianavatars_amd import mesh_raster

    H, W = 544, 800
    pos, tri = (_t(a) for a in _head_clip(W, H, yaw=10.0))
    r1, _ = mesh_raster.rasterize(None, pos, tri, (H, W))
    r2, _ = mesh_raster.rasterize(None, pos, tri, (H, W))
    assert torch.equal(r1, r2)
    color = torch.rand(1, H, W, 4, device=DEV)
    a1 = mesh_raster.antialias(color, r1, pos, tri)
    a2 = mesh_raster.antialias(color, r2, pos, tri)
    assert torch.equal(a1, a2)


def test_through_the_nvdiffrast_shim_in_the_reference_call_pattern():
    from gaussianavatars_amd import shims
    from gaussianavatars_amd import synthetic as S

    shims.install()
    import nvdiffrast.torch as dr

    glctx = dr.RasterizeCudaContext()
    cam = S.orbit_camera(802, 550, yaw_deg=-25.0)
    H, W = cam.image_height // 8 * 8, cam.image_width // 8 * 8          # the CUDA-context branch of NVDiffRenderer.render
    verts, faces_np = S.head_mesh()
    verts = torch.from_numpy(verts).to(DEV)[None]
    faces = torch.from_numpy(faces_np).to(DEV)                           # int64, as FLAME keeps them
    mvp = torch.from_numpy(cam.full_proj_transform).to(DEV)[None]
    verts_h = torch.cat([verts, torch.ones_like(verts[..., :1])], -1)
    verts_clip = torch.bmm(verts_h, mvp)
    tri = faces.int()
    rast_out, rast_out_db = dr.rasterize(glctx, verts_clip, tri, (H, W))
    assert rast_out.shape == (1, H, W, 4) and rast_out.dtype == torch.float32 and rast_out.device == verts_clip.device
    assert rast_out_db.shape == (1, H, W, 0)
    ids = rast_out[..., 3]
    assert torch.equal(ids, ids.round()) and ids.min() >= 0 and ids.max() <= faces.shape[0]
    fg_mask = torch.clamp(rast_out[..., -1:], 0, 1).bool()
    rgba = torch.cat([torch.where(fg_mask, torch.full_like(rast_out[..., :3], 0.3), torch.ones_like(rast_out[..., :3])),
                      fg_mask.float()], -1)
    rgba_aa = dr.antialias(rgba, rast_out, verts_clip, faces.int())
    assert rgba_aa.shape == rgba.shape and rgba_aa.dtype == torch.float32 and rgba_aa.device == rgba.device
    assert torch.all(rgba_aa[..., 3] >= 0) and torch.all(rgba_aa[..., 3] <= 1)
    ref = R.rasterize_ref(verts_clip.cpu().numpy(), faces_np, H, W)
    amb = R.ambiguous(ref)
    fg = fg_mask[..., 0].cpu().numpy()
    assert np.array_equal(fg[~amb], (ref["id"] >= 0)[~amb])


def test_backward_through_the_overlay_raises():
    from gaussianavatars_amd import mesh_raster

    pos, tri = MC.flat_triangle()
    p = _t(pos).requires_grad_()
    rast, _ = mesh_raster.rasterize(None, p, _t(tri), (24, 32))
    assert (rast[..., 3] > 0).any() and rast.requires_grad
    with pytest.raises(NotImplementedError, match="forward-only"):
        rast.sum().backward()
    color = torch.rand(1, 24, 32, 4, device=DEV, requires_grad=True)
    out = mesh_raster.antialias(color, rast.detach(), p, _t(tri))
    assert out.shape == color.shape and out.requires_grad
    with pytest.raises(NotImplementedError, match="forward-only"):
        out.sum().backward()
    with torch.no_grad():   # no node: plain tensors
        r2, _ = mesh_raster.rasterize(None, p, _t(tri), (24, 32))
    assert not r2.requires_grad and torch.equal(r2, rast.detach())
