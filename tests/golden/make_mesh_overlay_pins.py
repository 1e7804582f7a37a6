"""Writes tests/golden/mesh_overlay_pins.npz: the reference's own NVDiffRenderer.render_mesh / render_from_camera on the cases of
tests/mesh_overlay_cases.py, run on the CPU with `dr.rasterize` / `dr.antialias` backed by the float64 reference of tests/mesh_ref.py.

    python tests/golden/make_mesh_overlay_pins.py [--reference /path/to/reference/checkout]

Needs a checkout of the reference (its mesh_renderer, utils and scene packages); tests/ref_cpu_env.py neutralises its `cuda` literals.
Per case the file holds the inputs (verts, faces, the camera's two matrices, the image size), the four output maps, and `amb`: the pixels
of the float64 rasterization that are ambiguous by the rule of tests/test_mesh_raster_gpu.py (mesh_ref.ambiguous), at the render size.
The poses in mesh_overlay_cases.POSES are accepted only when the pixels left out because of `amb` stay within 0.1 % of every image.
Face colours and the background image are not stored: mesh_overlay_cases.face_colors / background_image rebuild them."""
import argparse
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

import mesh_overlay_cases as OC  # noqa: E402
import mesh_ref as R  # noqa: E402
import ref_cpu_env  # noqa: E402


def _install_float64_nvdiffrast(record):
    m = types.ModuleType("nvdiffrast.torch")

    class _Ctx:
        def __init__(self, *a, **k):
            pass

    def rasterize(glctx, pos, tri, resolution, ranges=None, grad_db=True):
        H, W = (int(r) for r in resolution)
        ref = R.rasterize_ref(pos.numpy(), tri.numpy(), H, W)
        record["amb"] = R.ambiguous(ref)[0]
        return torch.from_numpy(ref["rast"]), torch.zeros(pos.shape[0], H, W, 0)

    def antialias(color, rast, pos, tri, topology_hash=None, pos_gradient_boost=1.0):
        out = R.antialias_ref(color.numpy(), rast.numpy(), pos.numpy(), tri.numpy(), R.edge_neighbours_ref(tri.numpy()))
        return torch.from_numpy(out.astype(np.float32))

    m.RasterizeCudaContext = m.RasterizeGLContext = _Ctx
    m.rasterize, m.antialias = rasterize, antialias
    pkg = types.ModuleType("nvdiffrast")
    pkg.torch = m
    sys.modules["nvdiffrast"], sys.modules["nvdiffrast.torch"] = pkg, m


class _Cam:
    def __init__(self, c):
        self.image_height, self.image_width = c.image_height, c.image_width
        self.world_view_transform = torch.from_numpy(c.world_view_transform.copy())
        self.full_proj_transform = torch.from_numpy(c.full_proj_transform.copy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("GAA_REFERENCE_ROOT", ""))
    ap.add_argument("--out", default=os.path.join(HERE, "mesh_overlay_pins.npz"))
    args = ap.parse_args()
    if not os.path.isdir(os.path.join(args.reference, "mesh_renderer")):
        sys.exit("pass --reference: a checkout of the reference with its mesh_renderer package")
    from gaussianavatars_amd import shims

    shims.install()
    sys.path.insert(0, args.reference)
    ref_cpu_env._no_cuda()
    record = {}
    _install_float64_nvdiffrast(record)
    from mesh_renderer import NVDiffRenderer

    pins, worst = {}, 0.0
    names = []
    for name, mesh, s, light, colors, image_bg, through in OC.case_table():
        W, H = OC.SIZES[s]
        verts_np, faces_np = OC.MESHES[mesh]()
        cam = OC.camera(OC.THROUGH if through else mesh, W, H)
        verts, faces = torch.from_numpy(verts_np)[None], torch.from_numpy(faces_np)
        h, w = OC.render_hw(W, H)
        bg = torch.from_numpy(OC.background_image(h, w)) if image_bg else list(OC.CONST_BG)
        fc = torch.from_numpy(OC.face_colors(faces_np.shape[0])) if colors else None
        renderer = NVDiffRenderer(use_opengl=False, lighting_type=light)
        out = renderer.render_from_camera(verts, faces, _Cam(cam), background_color=bg, face_colors=fc)
        amb = record["amb"]
        assert amb.shape == (h, w)
        ex = OC.excluded(amb, H, W)
        worst = max(worst, ex.mean())
        assert ex.mean() <= 1e-3, f"{name}: {ex.sum()} of {ex.size} pixels would be left out: choose another pose"
        if through:
            pos = np.concatenate([verts_np, np.ones((verts_np.shape[0], 1), np.float32)], 1) @ cam.full_proj_transform
            assert (pos[:, 3] <= 0).any() and (pos[:, 3] > 0).any(), "the through camera must leave vertices on both sides of w = 0"
        fg = out["rgba"][..., 3] > 0.5
        assert 0.05 < fg.float().mean() < (1.01 if through else 0.98), f"{name}: covered fraction {fg.float().mean():.3f}"
        names.append(name)
        pins[name + "/verts"], pins[name + "/faces"] = verts_np, faces_np
        pins[name + "/world_view_transform"], pins[name + "/full_proj_transform"] = cam.world_view_transform, cam.full_proj_transform
        pins[name + "/size"] = np.array([W, H], np.int32)
        pins[name + "/amb"] = amb
        for k in ("albedo", "normal", "diffuse", "rgba"):
            assert out[k].shape == (1, H, W, 4 if k == "rgba" else 3) and out[k].dtype == torch.float32
            pins[name + "/" + k] = out[k].numpy()
        print(f"{name}: covered {fg.float().mean():.3f}, ambiguous {int(amb.sum())}, left out {int(ex.sum())}", flush=True)
        if s == 0 and not through:   # render_mesh itself (what the use_opengl branch returns): same inputs, no resize
            wvt = torch.from_numpy(cam.world_view_transform.copy())
            fpt = torch.from_numpy(cam.full_proj_transform.copy())
            wvt[:, 1], wvt[:, 2], fpt[:, 1] = -wvt[:, 1], -wvt[:, 2], -fpt[:, 1]
            direct = renderer.render_mesh(verts, faces, wvt.T[None].contiguous(), fpt.T[None].contiguous(), (H, W), bg, fc)
            for k in ("albedo", "normal", "diffuse", "rgba"):   # at a size that is a multiple of 8 the resize is the identity
                assert torch.allclose(direct[k], out[k], atol=1e-6), (name, k)
    pins["names"] = np.array(names)
    np.savez_compressed(args.out, **pins)
    print(f"wrote {args.out}: {len(names)} cases, {os.path.getsize(args.out)} bytes, at most {worst:.5f} of an image left out")


if __name__ == "__main__":
    main()
