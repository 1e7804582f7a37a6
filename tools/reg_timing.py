"""Time per call, forward + backward, of the two splat regularisers of a mesh-bound run (train.py:134-146 with the metric flags off) at
10 k, 100 k and 1 M splats, about half of them visible.  Inputs are seeded: xyz ~ N(0, 0.8) per axis, log-scales ~ N(log 0.4, 0.5);
thresholds and lambdas are the reference's defaults (arguments/__init__.py:100-105).

Legs, in one process:
    torch   the reference's composed expressions (boolean-mask gather, norm / exp / sub / relu / mean and their backward)
    grl     gaussianavatars_amd.loss.splat_regularizers (include/grl.h): one launch each way

Two timings per leg, each the median of `--steps` calls after `--warmup`:
    gpu_us   device events around every single call
    wall_us  host wall time per call of loops of 20 calls closed by one synchronize: the stream is kept busy, a host wait inside a call
             (the composed leg's nonzero) drains it
and the kernel launches of one call (torch.profiler for the composed leg; libgrl's own launch table for the other).  For the grl leg also the
two kernels' own times (grl_profile_*) and the backward's achieved bytes/s -- 25 B read and 24 B written per splat -- beside the 6.29 TB/s of
a float4 copy on the MI355X.  One JSON line per size; --out writes them all to a file.

    python tools/reg_timing.py [--steps 200] [--warmup 20] [--sizes 10000,100000,1000000] [--out profiles/reg_timing.json]
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
from gaussianavatars_amd.loss import splat_regularizers  # noqa: E402

COPY_TBS = 6.29
T_XYZ, T_S, L_XYZ, L_S = 1.0, 0.6, 1e-2, 1.0
BWD_BYTES_PER_SPLAT = 12 + 12 + 1 + 12 + 12


def inputs(n, dev):
    g = torch.Generator(device="cpu").manual_seed(0)
    xyz = (torch.randn(n, 3, generator=g) * 0.8).to(dev).requires_grad_(True)
    ls = (torch.randn(n, 3, generator=g) * 0.5 + math.log(0.4)).to(dev).requires_grad_(True)
    vis = (torch.rand(n, generator=g) < 0.5).to(dev)
    return xyz, ls, vis


def step_torch(xyz, ls, vis):
    xyz.grad = ls.grad = None
    a = F.relu(xyz[vis].norm(dim=1) - T_XYZ).mean() * L_XYZ
    b = F.relu(torch.exp(ls[vis]) - T_S).norm(dim=1).mean() * L_S
    (a + b).backward()


def step_grl(xyz, ls, vis):
    xyz.grad = ls.grad = None
    a, b = splat_regularizers(xyz, ls, vis, T_XYZ, T_S)
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


def time_leg(leg, n, dev, steps, warmup):
    args = inputs(n, dev)
    step = step_grl if leg == "grl" else step_torch
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
    if leg == "grl":
        reps = 20
        _lib.grl_profile_enable(True)
        for _ in range(reps):
            step(*args)
        torch.cuda.synchronize()
        prof = _lib.grl_profile_read()
        _lib.grl_profile_enable(False)
        row["grl_launches"] = sum(k for _, k in prof.values()) / reps
        for name, (ms, k) in prof.items():
            row["forward_kernel_us" if "fwd" in name else "backward_kernel_us"] = 1e3 * ms / k
        row["backward_tb_per_s"] = BWD_BYTES_PER_SPLAT * n / (row["backward_kernel_us"] * 1e-6) / 1e12
        row["backward_fraction_of_copy_rate"] = row["backward_tb_per_s"] / COPY_TBS
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for n in (int(s) for s in args.sizes.split(",")):
        row = {"splats": n, "steps": args.steps, "warmup": args.warmup, "copy_tb_per_s": COPY_TBS, "backward_bytes": BWD_BYTES_PER_SPLAT * n}
        for leg in ("torch", "grl"):
            row[leg] = time_leg(leg, n, dev, args.steps, args.warmup)
            torch.cuda.empty_cache()
        row["wall_ratio_torch_over_grl"] = row["torch"]["wall_us"] / row["grl"]["wall_us"]
        row["gpu_ratio_torch_over_grl"] = row["torch"]["gpu_us"] / row["grl"]["gpu_us"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
