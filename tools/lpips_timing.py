#!/usr/bin/env python3
"""Times LPIPS of one 802x550 pair on the GPU, for both nets: the kernels of include/glp.h per kernel (the library's own event pairs) and as a
whole (HIP events around the call), against lpips_composed on the same GPU, which goes through torch's convolution.

    python tools/lpips_timing.py [--height 550 --width 802 --iters 20 --warmup 3 --out profiles/lpips_timing.json]

The weights are seeded random numbers of the right shapes (the time of a convolution does not depend on its values).  Nothing is asserted
on time; the JSON it prints is what DESIGN.md section 20 quotes once someone has run it on an MI355X."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gaussianavatars_amd import _lib  # noqa: E402
from gaussianavatars_amd import lpips as L  # noqa: E402


def random_weights(net, seed=0):
    g = np.random.default_rng(seed)
    backbone, lin = {}, {}
    for op in L.NETS[net]["ops"]:
        if op[0] == "conv":
            _, index, cin, cout, k = op[:5]
            backbone[f"features.{index}.weight"] = (g.standard_normal((cout, cin, k, k)) * np.sqrt(2.0 / (cin * k * k))).astype(np.float32)
            backbone[f"features.{index}.bias"] = (0.05 * g.standard_normal(cout)).astype(np.float32)
    for t, c in enumerate(L.NETS[net]["channels"]):
        lin[f"lin{t}.model.1.weight"] = g.uniform(0, 1, (1, c, 1, 1)).astype(np.float32)
    return L.Weights(net, backbone, lin)


def timed(fn, iters, warmup):
    """Mean milliseconds of fn() between two events on the current stream."""
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--height", type=int, default=550)
    ap.add_argument("--width", type=int, default=802)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(1)
    x = torch.rand((1, 3, args.height, args.width), generator=g).to(dev)
    y = (0.7 * x.cpu() + 0.3 * torch.rand(x.shape, generator=g)).to(dev)
    report = dict(height=args.height, width=args.width, iters=args.iters, device=torch.cuda.get_device_name(0), nets={})
    with torch.no_grad():
        for net in ("alex", "vgg"):
            w = random_weights(net)
            fused = lambda: L.terms(x, y, net, w)
            composed = lambda: L.lpips_composed(x, y, net, w)
            row = dict(hip_ms=timed(fused, args.iters, args.warmup), composed_torch_ms=timed(composed, args.iters, args.warmup))
            row["value_hip"], row["value_composed"] = float(fused()[5]), float(composed())
            _lib.glp_profile_enable(True)
            for _ in range(args.iters):
                fused()
            torch.cuda.synchronize()
            row["kernels_ms"] = {name: dict(ms_per_pair=ms / args.iters, launches_per_pair=k / args.iters) for name, (ms, k) in _lib.glp_profile_read().items()}
            _lib.glp_profile_enable(False)
            report["nets"][net] = row
    text = json.dumps(report, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(text + "\n")


if __name__ == "__main__":
    main()
