"""The shaded mesh overlay on the MI355X (gaussianavatars_amd.mesh_renderer, include/gmr_overlay.h) against the pins of
tests/golden/mesh_overlay_pins.npz (the reference's own NVDiffRenderer on the CPU, rasterize / antialias in float64), gmr_resize_flip
against F.interpolate on the same device, compose_overlay against the torch expression's bits, and the smaller contracts.

Measured on the MI355X: see DESIGN.md section 16."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mesh_overlay_cases as OC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("albedo", "normal", "diffuse", "rgba")
CASES = OC.case_table()


@pytest.fixture(scope="module")
def pins():
    return np.load(os.path.join(ROOT, "tests", "golden", "mesh_overlay_pins.npz"))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _Cam:
    def __init__(self, P, name):
        self.image_width, self.image_height = (int(v) for v in P[name + "/size"])
        self.world_view_transform = _t(P[name + "/world_view_transform"])
        self.full_proj_transform = _t(P[name + "/full_proj_transform"])


def _inputs(P, case):
    name, mesh, s, light, colors, image_bg, through = case
    W, H = OC.SIZES[s]
    faces = _t(P[name + "/faces"])
    h, w = OC.render_hw(W, H)
    bg = _t(OC.background_image(h, w)) if image_bg else list(OC.CONST_BG)
    fc = _t(OC.face_colors(faces.shape[0])) if colors else None
    return _t(P[name + "/verts"])[None], faces, _Cam(P, name), bg, fc


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_render_from_camera_matches_the_pins(pins, case):
    """All four maps within 1e-5 of the pins outside the pixels the float64 reference calls ambiguous (with their 4-neighbours and, after a
    resize, every output pixel whose bilinear footprint touches one): at most 0.1 % of each image."""
    from gaussianavatars_amd.mesh_renderer import MeshRenderer

    name, _, s, light = case[:4]
    W, H = OC.SIZES[s]
    verts, faces, cam, bg, fc = _inputs(pins, case)
    out = MeshRenderer(use_opengl=False, lighting_type=light).render_from_camera(verts, faces, cam, background_color=bg, face_colors=fc)
    torch.cuda.synchronize()
    ex = OC.excluded(pins[name + "/amb"], H, W)
    assert ex.mean() <= 1e-3, f"{name}: {ex.mean():.5f} of the image is left out"
    worst = {}
    for k in KEYS:
        got, want = out[k].cpu().numpy(), pins[name + "/" + k]
        assert got.shape == want.shape and got.dtype == np.float32, (name, k, got.shape)
        worst[k] = float(np.abs(got - want)[0][~ex].max())
    print(f"{name}: max |diff| " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert all(v <= 1e-5 for v in worst.values()), (name, worst)


@pytest.mark.parametrize("case", [c for c in CASES if c[2] == 0], ids=[c[0] for c in CASES if c[2] == 0])
def test_use_opengl_branch_equals_the_no_resize_pins(pins, case):
    from gaussianavatars_amd.mesh_renderer import MeshRenderer

    name, _, s, light = case[:4]
    W, H = OC.SIZES[s]
    verts, faces, cam, bg, fc = _inputs(pins, case)
    gl = MeshRenderer(use_opengl=True, lighting_type=light).render_from_camera(verts, faces, cam, background_color=bg, face_colors=fc)
    cuda = MeshRenderer(use_opengl=False, lighting_type=light).render_from_camera(verts, faces, cam, background_color=bg, face_colors=fc)
    ex = OC.excluded(pins[name + "/amb"], H, W)
    for k in KEYS:
        assert torch.equal(gl[k], cuda[k]), (name, k)          # a multiple of 8: both branches render at the image size
        assert np.abs(gl[k].cpu().numpy() - pins[name + "/" + k])[0][~ex].max() <= 1e-5, (name, k)


def test_render_mesh_with_row_major_matrices_equals_render_from_camera(pins):
    from gaussianavatars_amd.mesh_renderer import MeshRenderer

    case = CASES[1]
    verts, faces, cam, bg, fc = _inputs(pins, case)
    r = MeshRenderer(lighting_type=case[3])
    want = r.render_from_camera(verts, faces, cam, background_color=bg, face_colors=fc)
    wvt, fpt = cam.world_view_transform.clone(), cam.full_proj_transform.clone()
    wvt[:, 1], wvt[:, 2], fpt[:, 1] = -wvt[:, 1], -wvt[:, 2], -fpt[:, 1]
    for RT in (wvt.T[None], wvt.T[None][:, :3]):               # (1, 4, 4) and (1, 3, 4)
        got = r.render_mesh(verts, faces, RT, fpt.T[None], (cam.image_height, cam.image_width), bg, fc)
        for k in KEYS:
            assert torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("shape", [(16, 24, 19, 29), (48, 72, 53, 77)], ids=["16x24-19x29", "48x72-53x77"])
@pytest.mark.parametrize("C", [1, 3, 4])
def test_resize_flip_matches_interpolate_on_the_device(shape, C):
    """Values in [0, 1]: a four-term weighted sum in fp32, the weights possibly formed in another order than torch's: 2e-6."""
    from gaussianavatars_amd.mesh_renderer import resize_flip

    w, h, W, H = shape
    x = torch.rand(2, h, w, C, device=DEV, generator=torch.Generator(DEV).manual_seed(7 + C))
    got = resize_flip(x, (H, W))
    want = F.interpolate(x.flip(1).permute(0, 3, 1, 2), (H, W), mode="bilinear").permute(0, 2, 3, 1)
    assert got.shape == (2, H, W, C) and got.is_contiguous()
    d = float((got - want).abs().max())
    print(f"resize_flip {w}x{h} -> {W}x{H} C={C}: max |diff| {d:.2e}")
    assert d <= 2e-6, d


@pytest.mark.parametrize("C", [1, 3, 4])
def test_resize_flip_at_equal_sizes_is_the_bitwise_flip(C):
    from gaussianavatars_amd.mesh_renderer import resize_flip

    x = torch.randn(2, 8, 8, C, device=DEV, generator=torch.Generator(DEV).manual_seed(C))
    x[0, 0, 0, 0], x[1, 3, 2, 0], x[0, 7, 7, C - 1] = -0.0, float("inf"), float("nan")
    got = resize_flip(x, (8, 8))
    assert torch.equal(got.view(torch.int32), x.flip(1).contiguous().view(torch.int32))


def test_compose_overlay_has_the_bits_of_the_torch_expression():
    from gaussianavatars_amd.mesh_renderer import compose_overlay

    H, W = 37, 53
    g = torch.Generator(DEV).manual_seed(3)
    rgba = torch.rand(1, H, W, 4, device=DEV, generator=g) * 1.5 - 0.25       # values outside [0, 1] too
    rgba[0, :10, :, 3], rgba[0, 10:20, :, 3] = 0.0, 1.0                        # alpha exactly 0 and exactly 1
    splat = torch.rand(3, H, W, device=DEV, generator=g) * 1.5 - 0.25
    send = lambda img: (torch.clamp(img, min=0, max=1.0) * 255).byte().permute(1, 2, 0).contiguous()
    rgba_mesh = rgba.squeeze(0).permute(2, 0, 1)
    rgb_mesh, alpha_mesh = rgba_mesh[:3, :, :], rgba_mesh[3:, :, :]
    for mesh_opacity in (0, 0.5, 1, 0.3):
        net_image = rgb_mesh * alpha_mesh * mesh_opacity + splat * (alpha_mesh * (1 - mesh_opacity) + (1 - alpha_mesh))
        got = compose_overlay(splat, rgba, mesh_opacity)
        assert got.shape == (3, H, W) and torch.equal(got.view(torch.int32), net_image.contiguous().view(torch.int32)), mesh_opacity
        assert torch.equal(compose_overlay(splat, rgba[0], mesh_opacity, as_bytes=True), send(net_image)), mesh_opacity
    assert torch.equal(compose_overlay(None, rgba, 0.5).view(torch.int32), rgb_mesh.contiguous().view(torch.int32))
    assert torch.equal(compose_overlay(None, rgba, 0.5, as_bytes=True), send(rgb_mesh))


def test_two_calls_give_identical_bits(pins):
    from gaussianavatars_amd.mesh_renderer import MeshRenderer

    case = CASES[-2]                                                           # head200 through the resize
    verts, faces, cam, bg, fc = _inputs(pins, case)
    r = MeshRenderer(lighting_type="front")
    a = r.render_from_camera(verts, faces, cam, background_color=bg, face_colors=fc)
    b = r.render_from_camera(verts, faces, cam, background_color=bg, face_colors=fc)
    for k in KEYS:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


def test_cached_adjacency_equals_a_fresh_build(pins):
    from gaussianavatars_amd import mesh_raster
    from gaussianavatars_amd import mesh_renderer as M

    M.clear_topology_cache()
    case = CASES[12]
    verts, faces, cam, bg, fc = _inputs(pins, case)
    r = M.MeshRenderer(lighting_type=case[3])
    first = r.render_from_camera(verts, faces, cam, background_color=bg, face_colors=fc)
    topo = M.topology(faces)
    assert len(M._TOPOLOGY) == 1 and topo.faces is faces
    assert torch.equal(topo.neighbours, mesh_raster.edge_neighbours(faces.int(), verts.shape[1]))
    again = r.render_from_camera(verts, faces, cam, background_color=bg, face_colors=fc)       # the cached entry
    fresh = r.render_from_camera(verts, faces.clone(), cam, background_color=bg, face_colors=fc)   # another tensor: a fresh build
    assert len(M._TOPOLOGY) == 2
    for k in KEYS:
        assert torch.equal(first[k], again[k]) and torch.equal(first[k], fresh[k]), k


def test_backward_through_rgba_raises(pins):
    from gaussianavatars_amd.mesh_renderer import MeshRenderer

    verts, faces, cam, bg, fc = _inputs(pins, CASES[0])
    v = verts.clone().requires_grad_()
    out = MeshRenderer().render_from_camera(v, faces, cam)
    assert out["rgba"].requires_grad
    with pytest.raises(NotImplementedError, match="forward-only"):
        out["rgba"].sum().backward()
    with torch.no_grad():
        plain = MeshRenderer().render_from_camera(v, faces, cam)
    assert not plain["rgba"].requires_grad and torch.equal(plain["rgba"], out["rgba"].detach())


def test_an_empty_mesh_returns_the_background(pins):
    from gaussianavatars_amd.mesh_renderer import MeshRenderer

    verts, _, cam, _, _ = _inputs(pins, CASES[2])                              # 53 x 77: through the resize
    faces = torch.zeros((0, 3), dtype=torch.int64, device=DEV)
    H, W = cam.image_height, cam.image_width
    out = MeshRenderer(lighting_type="front").render_from_camera(verts, faces, cam, background_color=list(OC.CONST_BG))
    bgc = torch.tensor(OC.CONST_BG, device=DEV)
    assert torch.all(out["albedo"] == 1) and out["rgba"].shape == (1, H, W, 4)
    for k in ("normal", "diffuse"):
        assert torch.allclose(out[k], bgc.expand(1, H, W, 3), atol=2e-6), k
    assert torch.allclose(out["rgba"][..., :3], bgc.expand(1, H, W, 3), atol=2e-6) and torch.all(out["rgba"][..., 3] == 0)
    img = _t(OC.background_image(*OC.render_hw(W, H)))
    gl = MeshRenderer(use_opengl=True).render_mesh(verts, faces, torch.eye(4, device=DEV)[None], torch.eye(4, device=DEV)[None],
                                                   OC.render_hw(W, H), img)
    assert torch.equal(gl["normal"], img) and torch.equal(gl["rgba"][..., :3], img)   # flipped on the way in and on the way out
