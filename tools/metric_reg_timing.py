"""Time per call, forward + backward, of the two METRIC-SPACE splat regularisers of a mesh-bound run (train.py:136 and :143: --metric_xyz,
--metric_scale) at 10 k and 100 k splats bound to F = 10 144 faces, about 60 % of them visible, with face_scaling requiring a gradient (a run
that fine-tunes the FLAME parameters).  Inputs are seeded: xyz ~ N(0, 0.8) per axis, log-scales ~ N(log 0.4, 0.5), face_scaling in [0.5, 1.5),
a uniform binding; thresholds and lambdas are the reference's defaults (arguments/__init__.py:100-105).

Legs, in one process:
    torch   the reference's composed lines (face_scaling[binding] gather, boolean-mask gather, exp / mul / sub / relu / norm / mean, and their
            backward with its index_put into face_scaling); get_scaling is spelled out as exp(_scaling) * face_scaling[binding]
    gms     gaussianavatars_amd.loss.metric_regularizers (include/gms.h): one launch forward, two backward

Two timings per leg, each the median of `--steps` calls after `--warmup`:
    gpu_us   device events around every single call
    wall_us  host wall time per call of loops of 20 calls closed by one synchronize: the stream is kept busy, a host wait inside a call
             (the composed leg's nonzero) drains it
and the device activities of one call (torch.profiler).  For the gms leg also each kernel's own time (gms_profile_*) and whether one call runs
under torch.cuda.set_sync_debug_mode("error"), i.e. without a host wait.  One JSON line per size; --out writes them all to a file.

    python tools/metric_reg_timing.py [--steps 200] [--warmup 20] [--sizes 10000,100000] [--faces 10144] [--out profiles/metric_reg_timing.json]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gaussianavatars_amd import _lib  # noqa: E402
from gaussianavatars_amd.loss import metric_regularizers  # noqa: E402

T_XYZ, T_S, L_XYZ, L_S = 1.0, 0.6, 1e-2, 1.0


def inputs(n, faces, dev):
    g = torch.Generator(device="cpu").manual_seed(0)
    xyz = (torch.randn(n, 3, generator=g) * 0.8).to(dev).requires_grad_(True)
    ls = (torch.randn(n, 3, generator=g) * 0.5 + math.log(0.4)).to(dev).requires_grad_(True)
    fs = (torch.rand(faces, 1, generator=g) + 0.5).to(dev).requires_grad_(True)
    binding = torch.randint(0, faces, (n,), generator=g).to(dev)
    vis = (torch.rand(n, generator=g) < 0.6).to(dev)
    return xyz, ls, fs, binding, vis


def step_torch(xyz, ls, fs, binding, vis):
    xyz.grad = ls.grad = fs.grad = None
    a = F.relu((xyz * fs[binding])[vis] - T_XYZ).norm(dim=1).mean() * L_XYZ
    b = F.relu((torch.exp(ls) * fs[binding])[vis] - T_S).norm(dim=1).mean() * L_S
    (a + b).backward()


def step_gms(xyz, ls, fs, binding, vis):
    xyz.grad = ls.grad = fs.grad = None
    a, b = metric_regularizers(xyz, ls, fs, binding, vis, T_XYZ, T_S)
    (a * L_XYZ + b * L_S).backward()


def count_launches(step, args):
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step(*args)
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if getattr(e, "device_type", None) == torch.autograd.DeviceType.CUDA)
    except Exception as e:   # the profiler is a convenience here: a build without it reports null
        print(f"# torch.profiler unavailable: {e!r}", file=sys.stderr)
        return None


def runs_without_host_wait(step, args):
    """One call under the sync debug mode that turns every host wait into an error; None where this torch has no such mode."""
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        return None
    torch.cuda.synchronize()
    was = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        step(*args)
        return True
    except RuntimeError as e:
        print(f"# host wait: {e}", file=sys.stderr)
        return False
    finally:
        torch.cuda.set_sync_debug_mode(was)
        torch.cuda.synchronize()


def time_leg(leg, n, faces, dev, steps, warmup):
    args = inputs(n, faces, dev)
    step = step_gms if leg == "gms" else step_torch
    for _ in range(warmup):
        step(*args)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        step(*args)
        b.record()
    torch.cuda.synchronize()
    gpu = [1e3 * a.elapsed_time(b) for a, b in ev]
    wall, block = [], 20
    for _ in range(max(1, steps // block)):
        t0 = time.perf_counter()
        for _ in range(block):
            step(*args)
        torch.cuda.synchronize()
        wall.append(1e6 * (time.perf_counter() - t0) / block)
    row = {"gpu_us": statistics.median(gpu), "wall_us": statistics.median(wall), "gpu_us_min": min(gpu), "wall_us_min": min(wall)}
    row["launches"] = count_launches(step, args)   # (every device activity of one call: kernels, fills and copies)
    row["no_host_wait"] = runs_without_host_wait(step, args)
    if leg == "gms":
        reps = 20
        _lib.gms_profile_enable(True)
        for _ in range(reps):
            step(*args)
        torch.cuda.synchronize()
        prof = _lib.gms_profile_read()
        _lib.gms_profile_enable(False)
        row["gms_launches"] = sum(k for _, k in prof.values()) / reps
        row["kernel_us"] = {name.split("::")[-1]: 1e3 * ms / k for name, (ms, k) in prof.items()}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", default="10000,100000")
    ap.add_argument("--faces", type=int, default=10144)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for n in (int(s) for s in args.sizes.split(",")):
        row = {"splats": n, "faces": args.faces, "steps": args.steps, "warmup": args.warmup}
        for leg in ("torch", "gms"):
            row[leg] = time_leg(leg, n, args.faces, dev, args.steps, args.warmup)
            torch.cuda.empty_cache()
        row["wall_ratio_torch_over_gms"] = row["torch"]["wall_us"] / row["gms"]["wall_us"]
        row["gpu_ratio_torch_over_gms"] = row["torch"]["gpu_us"] / row["gms"]["gpu_us"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
