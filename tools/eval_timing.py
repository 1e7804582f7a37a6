"""Time per evaluated image pair and per exported frame at 802 x 550 (the reference's image size), on the kernels of include/gev.h and on the
composed torch they replace -- evaluate.py's own restatement of the reference's expressions, the path GAA_FUSED_EVAL=0 takes:

    pair      training_report's per-image body (two clamps, L1, PSNR, SSIM and the three fp64 running sums) : MetricAccumulator.update
    frame     render.py:41 (mul, add_, clamp_, permute, to uint8) on the device, without the copy to the host : to_u8
    frame2    the render and its ground truth                                                                  : to_u8(image, also=gt)

Both sides run in this one process and call, alternating, `rounds` times each; a round is `iters` back-to-back calls after `warmup` calls,
timed by device events and by the host clock around the same window ending in a synchronise.  The figure is the median over the rounds, the
spread its minimum and maximum.  One JSON line.

    python tools/eval_timing.py [--iters 200] [--warmup 20] [--rounds 5]
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
from gaussianavatars_amd import evaluate as E  # noqa: E402


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


def _ab(sides, iters, warmup, rounds):
    """{name: {device_ms, wall_ms: median over the rounds, ..._min, ..._max}} with the sides alternating inside every round."""
    got = {k: ([], []) for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            d, w = _ms(fn, iters, warmup)
            got[k][0].append(d)
            got[k][1].append(w)
    return {k: {"device_ms": statistics.median(d), "device_ms_min": min(d), "device_ms_max": max(d),
                "wall_ms": statistics.median(w), "wall_ms_min": min(w), "wall_ms_max": max(w)} for k, (d, w) in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--height", type=int, default=550)
    ap.add_argument("--width", type=int, default=802)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_timing.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    _lib.gev()
    g = torch.Generator(device="cpu").manual_seed(7)
    image = (torch.rand(3, args.height, args.width, generator=g) * 1.5 - 0.2).to(dev)
    gt = (0.7 * image.cpu() + 0.3 * torch.rand(3, args.height, args.width, generator=g)).clamp(0, 1).to(dev)
    N = args.iters + args.warmup

    def switch(fused, fn):
        """`fn` with GAA_FUSED_EVAL set for its side (evaluate.py reads it at every call)"""
        def run():
            os.environ["GAA_FUSED_EVAL"] = "1" if fused else "0"
            return fn()

        return run

    def pair_side():
        acc = E.MetricAccumulator(N, dev)

        def run():
            if acc.n == N:   # (a host counter: the table is simply written again)
                acc.n = 0
            acc.update(image, gt)

        return run

    fused_pair, composed_pair = pair_side(), pair_side()

    row = {"image": [args.height, args.width], "iters": args.iters, "warmup": args.warmup, "rounds": args.rounds}
    # the two sides compute the same figures and the same bytes (checked before anything is timed)
    os.environ["GAA_FUSED_EVAL"] = "1"
    f, fb = torch.stack(E.frame_metrics(image, gt)), E.to_u8(image)
    os.environ["GAA_FUSED_EVAL"] = "0"
    c, cb = torch.stack(E.frame_metrics(image, gt)), E.to_u8(image)
    row["figures_fused"], row["figures_composed"] = f.tolist(), c.tolist()
    row["bytes_equal"] = bool(torch.equal(fb, cb))
    row["pair"] = _ab({"fused": switch(True, fused_pair), "composed": switch(False, composed_pair)}, args.iters, args.warmup, args.rounds)
    row["frame"] = _ab({"fused": switch(True, lambda: E.to_u8(image)), "composed": switch(False, lambda: E.to_u8(image))},
                       args.iters, args.warmup, args.rounds)
    row["frame2"] = _ab({"fused": switch(True, lambda: E.to_u8(image, also=gt)), "composed": switch(False, lambda: E.to_u8(image, also=gt))},
                        args.iters, args.warmup, args.rounds)
    os.environ["GAA_FUSED_EVAL"] = "1"
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
