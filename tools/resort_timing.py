"""Time per call of the spatial re-sort (gaussian_model.spatial_resort) at 10 k, 100 k and 1 M mesh-bound SH-3 splats with their twelve Adam
moments, on a model that has just been through one densify_and_prune -- the state patch._hook_spatial_order calls it in: the survivors in
their old order, the clones and children appended behind them.  Protocol of tools/densify_timing.py; inputs are seeded.

Legs, in one process, on copies of the same densified model:
    host     GAA_FUSED_RESORT=0: the host statement (copy to the host, float64 numpy codes, argsort, upload, ~22 index kernels)
    device   include/gdc.h ABI 2: gdc_morton_order + gdc_permute, nothing copied to the host

Two timings per leg, each the median of `--steps` calls after `--warmup`:
    gpu_us   device events around every single call
    wall_us  host wall time per call, each call closed by a synchronize
Every timed call starts from the densified, unsorted state: the model's tensors are put back (outside the timed window) before each call.
For the device leg also its kernels' own times (gdc_profile_*) and the launches per call.  One JSON line per size; --out writes them all.

    python tools/resort_timing.py [--steps 30] [--warmup 5] [--sizes 10000,100000,1000000] [--out profiles/resort_timing.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gaussianavatars_amd import _lib, densify  # noqa: E402
from gaussianavatars_amd.gaussian_model import GaussianModel, spatial_resort  # noqa: E402
from tools.densify_timing import PARAMS, inputs  # noqa: E402

LEAVES = tuple(densify.SPLAT_GROUPS.values())
ARGS = types.SimpleNamespace(percent_dense=PARAMS["percent_dense"], position_lr_init=1.6e-4, position_lr_final=1.6e-6, position_lr_delay_mult=0.01,
                             position_lr_max_steps=1000, feature_lr=2.5e-3, opacity_lr=5e-2, scaling_lr=5e-3, rotation_lr=1e-3)


def densified_model(P, dev):
    """A mirror model of P bound splats in Morton order, with optimizer state, after ONE densify_and_prune (no re-sort)."""
    leaves, moments, accum, denom, noise, max_grad, min_opacity, extent, _, mss, binding, fs, _ = inputs(P, dev)
    F = fs.shape[0]
    rng = np.random.default_rng(1)
    v = torch.from_numpy(rng.normal(0, 0.2, (F + 2, 3)).astype(np.float32)).to(dev)
    faces = torch.stack([torch.arange(F), torch.arange(F) + 1, torch.arange(F) + 2], 1).to(dev)
    m = GaussianModel(3)
    m.load_arrays({**{k: t.cpu().numpy() for k, t in leaves.items()}, "binding": binding.cpu().numpy()}, device=dev)
    m.flame_model = types.SimpleNamespace(v_template=v, faces=faces)
    m.face_scaling = fs
    m.training_setup(ARGS)
    for k in LEAVES:
        m.optimizer.state[getattr(m, k)] = {"step": torch.tensor(1.0), "exp_avg": moments[k][0].clone(), "exp_avg_sq": moments[k][1].clone()}
    os.environ["GAA_FUSED_RESORT"] = "1"
    spatial_resort(m)                                            # a loaded model is in order ...
    m.xyz_gradient_accum, m.denom = accum[m._gaa_order], denom[m._gaa_order]
    os.environ["GAA_SPATIAL_SORT"] = "0"
    m.densify_and_prune(max_grad, min_opacity, extent, mss, noise=noise[:, m._gaa_order].contiguous())   # ... and drifts out of it here
    torch.cuda.synchronize()
    return m


def state_of(m):
    s = {k: getattr(m, k).detach().clone() for k in LEAVES}
    s.update({("m", k): m.optimizer.state[getattr(m, k)]["exp_avg"].clone() for k in LEAVES})
    s.update({("v", k): m.optimizer.state[getattr(m, k)]["exp_avg_sq"].clone() for k in LEAVES})
    s.update({k: getattr(m, k).clone() for k in ("xyz_gradient_accum", "denom", "max_radii2D", "binding", "_gaa_order")})
    return s


def restore(m, s):
    """The model back in the densified, unsorted state: fresh copies, installed as densify._install does."""
    for k in LEAVES:
        old = getattr(m, k)
        p = torch.nn.Parameter(s[k].clone())
        state = m.optimizer.state.pop(old)
        state["exp_avg"], state["exp_avg_sq"] = s[("m", k)].clone(), s[("v", k)].clone()
        m.optimizer.state[p] = state
        [g for g in m.optimizer.param_groups if g["params"][0] is old][0]["params"][0] = p
        setattr(m, k, p)
    for k in ("xyz_gradient_accum", "denom", "max_radii2D", "binding", "_gaa_order"):
        setattr(m, k, s[k].clone())


def time_leg(leg, m, saved, steps, warmup):
    os.environ["GAA_FUSED_RESORT"] = "1" if leg == "device" else "0"
    gpu, wall, perm = [], [], None
    for it in range(warmup + steps):
        restore(m, saved)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        perm = spatial_resort(m)
        b.record()
        torch.cuda.synchronize()
        if it >= warmup:
            wall.append(1e6 * (time.perf_counter() - t0))
            gpu.append(1e3 * a.elapsed_time(b))
    row = {"gpu_us": statistics.median(gpu), "wall_us": statistics.median(wall), "gpu_us_min": min(gpu), "wall_us_min": min(wall)}
    if leg == "device":
        reps = 10
        _lib.gdc_profile_enable(True)
        for _ in range(reps):
            restore(m, saved)
            spatial_resort(m)
        torch.cuda.synchronize()
        prof = _lib.gdc_profile_read()
        _lib.gdc_profile_enable(False)
        row["launches"] = sum(k for _, k in prof.values()) / reps
        row["host_reads"] = 0
        row["kernel_us"] = {name.split("::")[-1]: 1e3 * ms / k for name, (ms, k) in prof.items()}
        row["kernel_us_per_call"] = {name.split("::")[-1]: 1e3 * ms / reps for name, (ms, k) in prof.items()}
    return row, perm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for n in (int(s) for s in args.sizes.split(",")):
        m = densified_model(n, dev)
        saved = state_of(m)
        N = m._xyz.shape[0]
        row = {"splats_before_densify": n, "splats": N, "rows_out_of_order": int((saved["_gaa_order"] < 0).sum()), "steps": args.steps,
               "warmup": args.warmup}
        perms = {}
        for leg in ("host", "device"):
            row[leg], perms[leg] = time_leg(leg, m, saved, args.steps, args.warmup)
        row["same_permutation"] = bool(torch.equal(perms["host"], perms["device"]))
        row["rows_moved"] = int((perms["device"] != torch.arange(N, device=dev)).sum())
        row["wall_ratio_host_over_device"] = row["host"]["wall_us"] / row["device"]["wall_us"]
        row["gpu_ratio_host_over_device"] = row["host"]["gpu_us"] / row["device"]["gpu_us"]
        print(json.dumps(row), flush=True)
        rows.append(row)
        del m, saved
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
