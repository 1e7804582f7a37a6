"""Time per call of the 3-nearest-neighbour distances (knn.dist2_knn3, what create_from_pcd initialises the scales of an unbound model from) at
10 k, 100 k and 1 M uniform points and on one clustered cloud of 100 k (ten Gaussian blobs).  Protocol of tools/resort_timing.py; inputs are
seeded.

Legs, each in a child process of its own under its own time limit (a leg that runs into it is reported as "not finished in N s", is not
tried again, and nothing is started after it: the million points come last, the stand-in last among their legs):
    fused      include/gdc.h: gdc_knn3_dist2, the exact search on the spatial order (17 launches)
    composed   knn.dist2_knn3_composed: chunked torch in the difference form (GAA_FUSED_KNN=0)
    stand_in   the |a|^2 + |b|^2 - 2 a.b body the distCUDA2 stand-in had before (kept for CPU tensors), called directly on device tensors

Two timings per leg, each the median of `--steps` calls after `--warmup`:
    gpu_us   device events around every single call
    wall_us  host wall time per call, each call closed by a synchronize
For the fused leg also its kernels' own times (gdc_profile_*) and the launches per call.  One JSON line per cloud; --out writes them all.

    python tools/knn_timing.py [--steps 20] [--warmup 3] [--clouds uniform:10000,uniform:100000,blobs:100000,uniform:1000000] [--out profiles/knn_timing.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ("fused", "composed", "stand_in")


def cloud(kind, n):
    import numpy as np

    rng = np.random.default_rng(n % 9973 + len(kind))
    if kind == "uniform":
        return rng.random((n, 3)).astype(np.float32)
    centres = rng.uniform(-5, 5, (10, 3))
    return (centres[rng.integers(0, 10, n)] + rng.normal(0, 0.2, (n, 3))).astype(np.float32)


def stand_in(points):
    """shims/simple_knn/_C.py's CPU body, on whatever device the points live on."""
    import torch

    p = points.detach().float()
    n = p.shape[0]
    out = torch.empty(n, dtype=torch.float32, device=p.device)
    k = min(4, n)
    sq = (p * p).sum(1)
    chunk = max(1, min(n, (1 << 26) // max(n, 1)))
    for s in range(0, n, chunk):
        q = p[s: s + chunk]
        d2 = (sq[s: s + chunk, None] + sq[None, :] - 2.0 * (q @ p.t())).clamp_min_(0.0)
        d2[torch.arange(q.shape[0], device=p.device), torch.arange(s, s + q.shape[0], device=p.device)] = 0.0
        near = torch.topk(d2, k, dim=1, largest=False).values[:, 1:]
        out[s: s + chunk] = near.sum(1) / 3.0 if near.shape[1] == 3 else near.sum(1) / max(near.shape[1], 1)
    return out


def run_leg(leg, kind, n, steps, warmup):
    """The child: one leg on one cloud, one JSON line."""
    import torch

    from gaussianavatars_amd import _lib, knn

    dev = torch.device("cuda:0")
    x = torch.from_numpy(cloud(kind, n)).to(dev)
    fn = {"fused": lambda: knn.dist2_knn3(x, fused=True), "composed": lambda: knn.dist2_knn3_composed(x), "stand_in": lambda: stand_in(x)}[leg]
    gpu, wall = [], []
    for it in range(warmup + steps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        if it >= warmup:
            wall.append(1e6 * (time.perf_counter() - t0))
            gpu.append(1e3 * a.elapsed_time(b))
    row = {"gpu_us": statistics.median(gpu), "wall_us": statistics.median(wall), "gpu_us_min": min(gpu), "wall_us_min": min(wall),
           "zeros": int((out == 0).sum()), "mean": float(out.double().mean())}
    if leg == "fused":
        reps = 5
        _lib.gdc_profile_enable(True)
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        prof = _lib.gdc_profile_read()
        _lib.gdc_profile_enable(False)
        row["launches"] = sum(k for _, k in prof.values()) / reps
        row["kernel_us_per_call"] = {name.split("::")[-1]: 1e3 * ms / reps for name, (ms, k) in prof.items()}
        row["chunk"] = _lib.GDC_KNN_CHUNK
    print("LEG " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--clouds", default="uniform:10000,uniform:100000,blobs:100000,uniform:1000000")
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--limit", type=float, default=60.0, help="seconds per leg")
    ap.add_argument("--big-limit", type=float, default=180.0, help="seconds for a composed-torch leg at a million points or more")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)   # the child's own arguments
    ap.add_argument("--cloud", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        kind, n = args.cloud.split(":")
        return run_leg(args.leg, kind, int(n), args.steps, args.warmup)
    rows, cut_off = [], False
    for spec in args.clouds.split(","):
        kind, n = spec.split(":")
        n = int(n)
        row = {"cloud": kind, "points": n, "steps": args.steps, "warmup": args.warmup}
        for leg in args.legs.split(","):
            if cut_off:
                row[leg] = "not started: an earlier leg ran into its time limit"
                continue
            big = n >= 1000000 and leg != "fused"
            limit = args.big_limit if big else args.limit
            steps, warmup = (1, 1) if big else (args.steps, args.warmup)      # (seconds per call there)
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--cloud", spec, "--steps", str(steps), "--warmup", str(warmup)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
            except subprocess.TimeoutExpired:
                row[leg] = f"not finished in {limit:.0f} s"
                cut_off = True
                continue
            lines = [l for l in r.stdout.splitlines() if l.startswith("LEG ")]
            if r.returncode != 0 or not lines:
                row[leg] = f"failed with exit status {r.returncode}: {r.stderr.strip().splitlines()[-1] if r.stderr.strip() else ''}"
                print(json.dumps(row), flush=True)
                raise SystemExit(1)      # nothing more is started on the device after a leg that did not end cleanly
            row[leg] = json.loads(lines[-1][4:])
        for other in ("composed", "stand_in"):
            if isinstance(row.get(other), dict) and isinstance(row.get("fused"), dict):
                row[f"wall_ratio_{other}_over_fused"] = row[other]["wall_us"] / row["fused"]["wall_us"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
