"""Time per call of the landmarks of a posed FLAME mesh (flame_model/lbs.py:60-98), forward and forward + backward, on the full-size synthetic
rig (V = 5143, F = 10144) with a seeded 70-landmark embedding in which eye-like landmarks share faces, as the reference's does.

Legs, in one process:
    torch   the reference's composed expression (index_select + fancy index + einsum; autograd's index_put backward)
    gab     gaussianavatars_amd.binding.landmarks (include/gab.h: gab_landmarks_forward / gab_landmarks_backward): one launch each way

Two timings per leg and direction, each the median of `--steps` calls after `--warmup`:
    gpu_us   device events around every single call
    wall_us  host wall time per call of loops of 20 calls closed by one synchronize
One JSON line; --out writes it to a file.

    python tools/landmark_timing.py [--steps 200] [--warmup 20] [--out profiles/landmark_timing.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gaussianavatars_amd import binding as B  # noqa: E402
from gaussianavatars_amd import synthetic as S  # noqa: E402
from gaussianavatars_amd import unfused as U  # noqa: E402

L = 70


class Head:
    def __init__(self, dev):
        rig = S.flame_rig(4)
        g = np.random.default_rng(0)
        idx = g.integers(0, rig["faces"].shape[0], L)
        idx[60:] = idx[50:60]                                   # ten pairs on one face each
        bary = g.uniform(0.05, 1.0, (L, 3))
        self.v_template = torch.as_tensor(rig["v_template"], device=dev)
        self.faces = torch.as_tensor(rig["faces"], device=dev)
        self.full_lmk_faces_idx = torch.as_tensor(idx, device=dev)
        self.full_lmk_bary_coords = torch.as_tensor((bary / bary.sum(1, keepdims=True)).astype(np.float32), device=dev)


def make_steps(head, verts, w):
    def torch_fwd():
        return U.landmarks(verts, head.faces, head.full_lmk_faces_idx, head.full_lmk_bary_coords)

    def gab_fwd():
        return B.landmarks(head, verts)

    def both(fwd):
        def step():
            verts.grad = None
            (fwd() * w).sum().backward()
        return step

    return {"torch": (torch_fwd, both(torch_fwd)), "gab": (gab_fwd, both(gab_fwd))}


def time_step(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        step()
        b.record()
    torch.cuda.synchronize()
    gpu = [1e3 * a.elapsed_time(b) for a, b in ev]
    wall, block = [], 20
    for _ in range(max(1, steps // block)):
        t0 = time.perf_counter()
        for _ in range(block):
            step()
        torch.cuda.synchronize()
        wall.append(1e6 * (time.perf_counter() - t0) / block)
    return {"gpu_us": statistics.median(gpu), "wall_us": statistics.median(wall), "gpu_us_min": min(gpu), "wall_us_min": min(wall)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    head = Head(dev)
    g = torch.Generator(device="cpu").manual_seed(0)
    verts = (head.v_template.cpu() + 1e-3 * torch.randn(head.v_template.shape, generator=g))[None].to(dev).requires_grad_(True)
    w = torch.randn((1, L, 3), generator=g).to(dev)
    row = {"vertices": int(verts.shape[1]), "faces": int(head.faces.shape[0]), "landmarks": L, "steps": args.steps, "warmup": args.warmup}
    for leg, (fwd, both) in make_steps(head, verts, w).items():
        with torch.no_grad():
            row[leg] = {"forward": time_step(fwd, args.steps, args.warmup)}
        row[leg]["forward_backward"] = time_step(both, args.steps, args.warmup)
    for k in ("forward", "forward_backward"):
        row[f"wall_ratio_torch_over_gab_{k}"] = row["torch"][k]["wall_us"] / row["gab"][k]["wall_us"]
        row[f"gpu_ratio_torch_over_gab_{k}"] = row["torch"][k]["gpu_us"] / row["gab"][k]["gpu_us"]
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
