"""Time per frame of the shaded mesh overlay (gaussianavatars_amd.mesh_renderer) at FLAME size: one render_from_camera of
synthetic.head_mesh() (5143 vertices, 10144 faces) through synthetic.orbit_camera at 800 x 544 and at 802 x 550 (which renders 800 x 544 and
resizes), through MeshRenderer and through the composed-torch way it replaces: the same statements around mesh_raster.rasterize / antialias,
restated here from the published formulae (world-to-camera, world-to-clip, face normals, gather, shade, background, where, flip, bilinear
resize).  Also each launch of the new path alone, the cached against the uncached adjacency, and compose_overlay against its torch
expression.  Device events around `iters` back-to-back calls after `warmup` calls, and the host clock around the same window ending in a
synchronise; one process, one JSON line per resolution.

    python tools/overlay_timing.py [--iters 200] [--warmup 20]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gaussianavatars_amd import _lib, mesh_raster  # noqa: E402
from gaussianavatars_amd import mesh_renderer as M  # noqa: E402
from gaussianavatars_amd import synthetic as S  # noqa: E402


def _ms(fn, iters, warmup):
    """(device ms, wall ms) per call"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters, 1e3 * (time.perf_counter() - t0) / iters


class Cam:
    def __init__(self, c, dev):
        self.image_height, self.image_width = c.image_height, c.image_width
        self.world_view_transform = torch.from_numpy(c.world_view_transform).to(dev)
        self.full_proj_transform = torch.from_numpy(c.full_proj_transform).to(dev)


def composed(verts, faces, cam, background_color, lighting_type):
    """The overlay as composed torch around the two mesh_raster calls: what a frame cost before mesh_renderer.py."""
    view = cam.world_view_transform.clone().to(verts)
    view[:, 1], view[:, 2] = -view[:, 1], -view[:, 2]
    proj = cam.full_proj_transform.clone().to(verts)
    proj[:, 1] = -proj[:, 1]
    H, W = cam.image_height, cam.image_width
    h, w = (2048, 2048) if max(H, W) > 2048 else (H // 8 * 8, W // 8 * 8)
    hom = torch.cat([verts, torch.ones_like(verts[..., :1])], -1)
    v_cam = torch.bmm(hom, view[None])[..., :3]
    v_clip = torch.bmm(hom, proj[None])
    tri = faces.int()
    rast, _ = mesh_raster.rasterize(None, v_clip, tri, (h, w))
    covered = rast[..., 3:].clamp(0, 1).bool()
    fid = (rast[..., 3].long() - 1).clamp(min=0)
    p0, p1, p2 = (v_cam[:, faces[:, k]] for k in range(3))
    n = torch.cross(p1 - p0, p2 - p0, dim=-1)
    n = n / torch.sqrt((n * n).sum(-1, keepdim=True).clamp(min=1e-20))
    normal = n[0][fid]
    albedo = torch.ones_like(normal)
    diffuse = torch.ones_like(normal) if lighting_type == "constant" else normal[..., 2:].clamp(0, 1)
    rgba = torch.cat([albedo * diffuse, covered.float()], -1)
    bg = torch.tensor(list(background_color) + [0.0], device=verts.device).expand_as(rgba).flip(1)
    normal = torch.where(covered, normal, bg[..., :3])
    diffuse = torch.where(covered, diffuse, bg[..., :3])
    rgba = mesh_raster.antialias(torch.where(covered, rgba, bg), rast, v_clip, tri)
    out = {"albedo": albedo.flip(1), "normal": normal.flip(1), "diffuse": diffuse.flip(1), "rgba": rgba.flip(1)}
    return {k: F.interpolate(v.permute(0, 3, 1, 2), (H, W), mode="bilinear").permute(0, 2, 3, 1) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    verts_np, faces_np = S.head_mesh()
    verts = torch.from_numpy(verts_np).to(dev)[None]
    faces = torch.from_numpy(faces_np).to(dev)          # int64, a persistent buffer like gaussians.faces
    bg = [1.0, 1.0, 1.0]
    t = lambda fn: _ms(fn, args.iters, args.warmup)
    for W, H in ((800, 544), (802, 550)):
        cam = Cam(S.orbit_camera(W, H, yaw_deg=20.0), dev)
        r = M.MeshRenderer(lighting_type="front")
        new = r.render_from_camera(verts, faces, cam, bg)
        old = composed(verts, faces, cam, bg, "front")
        row = {"image": [H, W], "render": list(M.render_size(H, W)), "V": int(verts.shape[1]), "F": int(faces.shape[0]),
               "max_abs_diff_new_vs_composed": {k: float((new[k] - old[k]).abs().max()) for k in new},
               "fraction_over_1e-5": {k: float(((new[k] - old[k]).abs() > 1e-5).float().mean()) for k in new}}
        row["new_ms"], row["new_wall_ms"] = t(lambda: r.render_from_camera(verts, faces, cam, bg))
        row["composed_ms"], row["composed_wall_ms"] = t(lambda: composed(verts, faces, cam, bg, "front"))
        row["new_uncached_topology_ms"], row["new_uncached_topology_wall_ms"] = t(lambda: r.render_from_camera(verts, faces.clone(), cam, bg))
        # each launch of the new path alone, on the tensors of one frame
        h, w = M.render_size(H, W)
        topo = M.topology(faces)
        stream = C.c_void_p(_lib.raw_stream(dev))
        rt, mvp = cam.world_view_transform[None].contiguous(), cam.full_proj_transform[None].contiguous()
        pos, normals = M._prepare(verts, topo.tri, rt, mvp, _lib.GMR_MAT_CAMERA, dev, stream)
        rast, _ = mesh_raster._rasterize(pos, topo.tri, h, w, dev)
        maps = M._shade(rast, normals, None, _lib.GMR_LIGHT_FRONT, (1.0, 1.0, 1.0), None, dev, stream)
        aa = M._antialias(maps[3], rast, pos, topo.tri, topo.neighbours, dev, stream)
        row["stage_ms"] = {
            "prepare": t(lambda: M._prepare(verts, topo.tri, rt, mvp, _lib.GMR_MAT_CAMERA, dev, stream))[0],
            "rasterize": t(lambda: mesh_raster._rasterize(pos, topo.tri, h, w, dev))[0],
            "shade": t(lambda: M._shade(rast, normals, None, _lib.GMR_LIGHT_FRONT, (1.0, 1.0, 1.0), None, dev, stream))[0],
            "antialias": t(lambda: M._antialias(maps[3], rast, pos, topo.tri, topo.neighbours, dev, stream))[0],
            "resize_flip": t(lambda: M._resize_flip([maps[0], maps[1], maps[2], aa], H, W, dev, stream))[0],
            "adjacency_build": t(lambda: mesh_raster.edge_neighbours(topo.tri, verts.shape[1]))[0],
        }
        splat = torch.rand(3, H, W, device=dev)
        m = new["rgba"].squeeze(0).permute(2, 0, 1)
        row["compose_ms"] = t(lambda: M.compose_overlay(splat, new["rgba"], 0.5))[0]
        row["compose_torch_ms"] = t(lambda: m[:3] * m[3:] * 0.5 + splat * (m[3:] * (1 - 0.5) + (1 - m[3:])))[0]
        row["iters"], row["warmup"] = args.iters, args.warmup
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
