"""Time per call of adaptive density control (include/gdc.h) at 10 k, 100 k and 1 M mesh-bound SH-3 splats with their twelve Adam moments:
about a sixth of the splats cloned, a third split, a quarter prune candidates.  Inputs are seeded and the same for both legs.

Legs, in one process:
    torch   densify.density_control_composed: the contract in composed torch fp32 on the same GPU (boolean-mask indexing, cat, its host reads)
    gdc     densify.density_control_fused: five launches, one host read

Two timings per leg, each the median of `--steps` calls after `--warmup`:
    gpu_us   device events around every single call
    wall_us  host wall time per call, each call closed by a synchronize (a call reads its row counts back, so it is synchronous anyway)
and for the gdc leg its kernels' own times (gdc_profile_*), the launches per call, and the gather's achieved bytes/s -- every output row read
once and written once, 4 B of row map read and the binding moved -- beside the 6.29 TB/s of a float4 copy on the MI355X.  One JSON line per
size; --out writes them all to a file.

    python tools/densify_timing.py [--steps 50] [--warmup 5] [--sizes 10000,100000,1000000] [--out profiles/densify_timing.json]
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

from gaussianavatars_amd import _lib, densify  # noqa: E402

COPY_TBS = 6.29
PARAMS = dict(max_grad=2e-4, min_opacity=5e-3, extent=5.0, percent_dense=0.01)
LEAVES = tuple(densify.SPLAT_GROUPS.values())
SHAPES = {"_xyz": (3,), "_features_dc": (1, 3), "_features_rest": (15, 3), "_opacity": (1,), "_scaling": (3,), "_rotation": (4,)}


def inputs(P, dev):
    rng = np.random.default_rng(0)
    F = max(1, P // 10)
    t = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    binding = rng.integers(0, F, P)
    fs = rng.uniform(0.5, 2.0, (F, 1))
    target = rng.choice([0.015, 0.15, 1.2], P, p=[0.5, 0.4, 0.1]) * rng.uniform(0.8, 1.2, P)
    scaling = np.log(target[:, None] * rng.uniform(0.3, 1.0, (P, 3)) / fs[binding])
    g = PARAMS["max_grad"] * rng.choice([0.2, 3.0], P) * rng.uniform(0.8, 1.2, P)
    denom = rng.integers(1, 40, P).astype(np.float64)
    o = np.where(rng.random(P) < 0.25, rng.uniform(0.001, 0.004, P), rng.uniform(0.1, 0.9, P))
    leaves = {k: t(rng.normal(0, 0.3, (P,) + s)) for k, s in SHAPES.items()}
    leaves["_scaling"], leaves["_opacity"] = t(scaling), t(np.log(o / (1 - o))[:, None])
    moments = {k: (t(rng.normal(0, 1e-3, (P,) + s)), t(rng.normal(0, 1e-3, (P,) + s) ** 2)) for k, s in SHAPES.items()}
    return (leaves, moments, t((g * denom)[:, None]), t(denom[:, None]), t(rng.normal(0, 1, (2, P, 3))), PARAMS["max_grad"], PARAMS["min_opacity"],
            PARAMS["extent"], PARAMS["percent_dense"], 20, t(binding, np.int32), t(fs), t(np.bincount(binding, minlength=F), np.int32))


def time_leg(leg, P, dev, steps, warmup):
    args = inputs(P, dev)
    fn = densify.density_control_fused if leg == "gdc" else densify.density_control_composed
    for _ in range(warmup):
        out = fn(*args)
    torch.cuda.synchronize()
    gpu, wall = [], []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        out = fn(*args)
        b.record()
        torch.cuda.synchronize()
        wall.append(1e6 * (time.perf_counter() - t0))
        gpu.append(1e3 * a.elapsed_time(b))
    row = {"gpu_us": statistics.median(gpu), "wall_us": statistics.median(wall), "gpu_us_min": min(gpu), "wall_us_min": min(wall),
           "rows_out": int(out["src"].shape[0]), "totals": [int(x) for x in out["totals"]]}
    if leg == "gdc":
        reps = 10
        _lib.gdc_profile_enable(True)
        for _ in range(reps):
            fn(*args)
        torch.cuda.synchronize()
        prof = _lib.gdc_profile_read()
        _lib.gdc_profile_enable(False)
        row["launches"] = sum(k for _, k in prof.values()) / reps
        row["host_reads"] = 1
        row["kernel_us"] = {name.split("::")[-1]: 1e3 * ms / k for name, (ms, k) in prof.items()}
        per_row = 4 * sum(int(np.prod(s)) for s in SHAPES.values()) * 3          # six leaves and twelve moments
        nbytes = row["rows_out"] * (2 * per_row + 4 + 2 * 4 + 3 * 4)                 # + row map, binding in and out, three statistics
        row["gather_bytes"] = nbytes
        row["gather_tb_per_s"] = nbytes / (row["kernel_us"]["k_dc_gather"] * 1e-6) / 1e12
        row["gather_fraction_of_copy_rate"] = row["gather_tb_per_s"] / COPY_TBS
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for n in (int(s) for s in args.sizes.split(",")):
        row = {"splats": n, "steps": args.steps, "warmup": args.warmup, "copy_tb_per_s": COPY_TBS}
        for leg in ("torch", "gdc"):
            row[leg] = time_leg(leg, n, dev, args.steps, args.warmup)
            torch.cuda.empty_cache()
        row["wall_ratio_torch_over_gdc"] = row["torch"]["wall_us"] / row["gdc"]["wall_us"]
        row["gpu_ratio_torch_over_gdc"] = row["torch"]["gpu_us"] / row["gdc"]["gpu_us"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
