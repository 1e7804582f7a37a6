"""Time per optimizer step of the reference's nine Adam groups (twelve tensors: N splats with SH 3, 59 floats each, and T = 300 timesteps of
FLAME parameters) at 10 k, 100 k (bench.py's cfg3) and 1 M splats.  Only the optimizer is stepped; random gradients are written once.

Legs:
    torch        torch.optim.Adam built the way the reference builds it (scene/gaussian_model.py:213-222 + three add_param_group calls)
    torch_fused  the same with torch's own fused=True (device-side step tensors, one launch per group: not what the reference runs)
    gop          gaussianavatars_amd.optim.FusedAdam (include/gop.h)

Two timings per leg, each the median of `--steps` steps after `--warmup`:
    gpu_us   device events around every single step
    wall_us  host wall time per step of loops of 20 steps closed by one synchronize -- what a host-paced training loop sees
and the kernel launches of one step (torch.profiler; libgop's own launch counter for the gop leg).  For the gop leg also the kernel's own
time (gop_profile_*) and the achieved bytes/s from 28 B per element, beside the 6.29 TB/s of a float4 copy on the MI355X.  One JSON line per size; --out writes them all to a file.

    python tools/adam_timing.py [--steps 200] [--warmup 20] [--sizes 10000,100000,1000000] [--out profiles/adam_timing.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gaussianavatars_amd import _lib  # noqa: E402
from gaussianavatars_amd.optim import FusedAdam  # noqa: E402

LRS = dict(xyz=0.005, f_dc=0.0025, f_rest=0.0025 / 20.0, opacity=0.05, scaling=0.017, rotation=0.001, pose=1e-5, trans=1e-6, expr=1e-3)
COPY_TBS = 6.29


def build(leg, n, t, dev):
    g = torch.Generator(device="cpu").manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g).to(dev).requires_grad_(True)
    splat = [("xyz", [r(n, 3)]), ("f_dc", [r(n, 1, 3)]), ("f_rest", [r(n, 15, 3)]), ("opacity", [r(n, 1)]), ("scaling", [r(n, 3)]),
             ("rotation", [r(n, 4)])]
    flame = [("pose", [r(t, 3), r(t, 3), r(t, 3), r(t, 6)]), ("trans", [r(t, 3)]), ("expr", [r(t, 100)])]
    kw = dict(fused=True) if leg == "torch_fused" else {}
    opt = (FusedAdam if leg == "gop" else torch.optim.Adam)([{"params": ps, "lr": LRS[k], "name": k} for k, ps in splat], lr=0.0, eps=1e-15, **kw)
    for k, ps in flame:
        opt.add_param_group({"params": ps, "lr": LRS[k], "name": k})
    params = [p for grp in opt.param_groups for p in grp["params"]]
    for p in params:
        p.grad = torch.randn_like(p) * 1e-3
    return opt, sum(p.numel() for p in params)


def count_launches(opt):
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            opt.step()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if getattr(e, "device_type", None) == torch.autograd.DeviceType.CUDA)
    except Exception as e:   # the profiler is a convenience here: a build without it reports null
        print(f"# torch.profiler unavailable: {e!r}", file=sys.stderr)
        return None


def time_leg(leg, n, t, dev, steps, warmup):
    opt, elements = build(leg, n, t, dev)
    for _ in range(warmup):
        opt.step()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        opt.step()
        b.record()
    torch.cuda.synchronize()
    gpu = [1e3 * a.elapsed_time(b) for a, b in ev]
    wall, block = [], 20
    for _ in range(max(1, steps // block)):
        t0 = time.perf_counter()
        for _ in range(block):
            opt.step()
        torch.cuda.synchronize()
        wall.append(1e6 * (time.perf_counter() - t0) / block)
    row = {"gpu_us": statistics.median(gpu), "wall_us": statistics.median(wall), "gpu_us_min": min(gpu), "wall_us_min": min(wall)}
    if leg == "gop":
        _lib.gop_profile_enable(True)
        opt.step()
        torch.cuda.synchronize()
        prof = _lib.gop_profile_read()
        _lib.gop_profile_enable(False)
        row["launches"] = sum(k for _, k in prof.values())
        row["kernel_us"] = 1e3 * sum(ms for ms, _ in prof.values())
        row["tb_per_s_gpu"] = 28.0 * elements / (row["gpu_us"] * 1e-6) / 1e12          # (events around the step: includes the host's pace)
        row["tb_per_s_kernel"] = 28.0 * elements / (row["kernel_us"] * 1e-6) / 1e12    # (events around the launch alone)
        row["fraction_of_copy_rate"] = row["tb_per_s_kernel"] / COPY_TBS
    else:
        row["launches"] = count_launches(opt)
    return row, elements


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--timesteps", type=int, default=300)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for n in (int(s) for s in args.sizes.split(",")):
        row = {"splats": n, "timesteps": args.timesteps, "steps": args.steps, "warmup": args.warmup, "copy_tb_per_s": COPY_TBS}
        for leg in ("torch", "torch_fused", "gop"):
            row[leg], row["elements"] = time_leg(leg, n, args.timesteps, dev, args.steps, args.warmup)
            torch.cuda.empty_cache()
        row["bytes_per_step"] = 28 * row["elements"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
