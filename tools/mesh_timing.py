"""Time per call of the mesh overlay (gaussianavatars_amd.mesh_raster) at FLAME size: rasterize, antialias and the edge adjacency build
alone, B = 1, the head mesh of synthetic.head_mesh() (5143 vertices, 10144 faces) through synthetic.orbit_camera, at 800 x 544 and
2048 x 2048.  Device events around `iters` back-to-back calls after `warmup` calls; one JSON line per resolution.  Kernel times: run it
under `rocprofv3 --kernel-trace --stats` (a run of its own).

    python tools/mesh_timing.py [--iters 200] [--warmup 20]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gaussianavatars_amd import mesh_raster  # noqa: E402
from gaussianavatars_amd import synthetic as S  # noqa: E402


def _ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    verts, faces = S.head_mesh()
    for W, H in ((800, 544), (2048, 2048)):
        cam = S.orbit_camera(W, H, yaw_deg=20.0)
        vh = np.concatenate([verts, np.ones((verts.shape[0], 1), np.float32)], 1)
        pos = torch.from_numpy((vh @ cam.full_proj_transform).astype(np.float32)[None]).to(dev)
        tri = torch.from_numpy(faces.astype(np.int32)).to(dev)
        rast, _ = mesh_raster.rasterize(None, pos, tri, (H, W))
        color = torch.rand(1, H, W, 4, device=dev)
        row = {"resolution": [H, W], "B": 1, "V": int(pos.shape[1]), "F": int(tri.shape[0]),
               "covered": float((rast[..., 3] > 0).float().mean()),
               "rasterize_ms": _ms(lambda: mesh_raster.rasterize(None, pos, tri, (H, W)), args.iters, args.warmup),
               "antialias_ms": _ms(lambda: mesh_raster.antialias(color, rast, pos, tri), args.iters, args.warmup),
               "adjacency_ms": _ms(lambda: mesh_raster.edge_neighbours(tri, pos.shape[1]), args.iters, args.warmup),
               "iters": args.iters, "warmup": args.warmup}
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
