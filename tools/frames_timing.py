"""How a training frame reaches the GPU, at 802 x 550 (the reference's image size): the path the reference's train.py takes per iteration
against the resident frame store of include/gfs.h (gaussianavatars_amd/frames.py).

    a  upload     train.py:128 and gaussian_renderer._dev: a pageable host fp32 (3,H,W) tensor `.cuda()` plus the camera's three small host
                  tensors (two transposed 4x4 views made contiguous, one 3-vector), one `.to(device)` each
    b  resident   `FrameRef.cuda()` (one gfs_fetch launch) plus `store.camera(i)` (three views, nothing moves)
    c  fetch      gfs_fetch alone, by device events, and its rate over the bytes it has to move (the frame's stride in, 12 bytes per pixel out)
    d  ingest     FrameStore.from_cameras over PNG files on disk, per frame (decode on the thread pool, upload, gfs_compose), and gfs_compose
                  alone by device events

a and b run in this one process, alternating, `rounds` times each; a round is `iters` back-to-back calls over a rotation of `frames` different
frames after `warmup` calls, timed by the host clock around the window, which ends in a synchronise (an upload from pageable memory returns
when the copy is staged, a launch when it is enqueued: neither is the frame being there).  The figure is the median over the rounds, the spread
its minimum and maximum.  Both sides deliver the same bits (checked before anything is timed).  One JSON line.

What this does not measure: the DataLoader workers' decode and composite per frame and the worker-queue hop of the 5.3 MB tensor, which the
resident path also removes, and the effect on train.py's `iter_time` end to end.

    python tools/frames_timing.py [--iters 200] [--warmup 20] [--rounds 7] [--frames 8]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gaussianavatars_amd import _lib  # noqa: E402
from gaussianavatars_amd import frames as FR  # noqa: E402
from gaussianavatars_amd import synthetic as S  # noqa: E402
from gaussianavatars_amd.gaussian_renderer import _dev  # noqa: E402


def _wall_ms(fn, iters, warmup):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(iters):
        fn(i)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / iters


def _device_ms(fn, iters, warmup):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _spread(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--height", type=int, default=550)
    ap.add_argument("--width", type=int, default=802)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frames_timing.py measures on the GPU; there is none here")
    from PIL import Image

    dev = torch.device("cuda", 0)
    H, W, N = args.height, args.width, args.frames
    g = np.random.default_rng(11)
    row = {"image": [H, W], "iters": args.iters, "warmup": args.warmup, "rounds": args.rounds, "frames": N}
    with tempfile.TemporaryDirectory() as tmp:
        cams = []
        for i in range(N):
            c = S.orbit_camera(W, H, yaw_deg=10.0 * i)
            rgba = g.integers(0, 256, (H, W, 4), dtype=np.uint8)
            rgba[..., 3] = np.where(g.random((H, W)) < 0.7, 255, rgba[..., 3])   # mostly opaque, like a segmented portrait
            path = os.path.join(tmp, f"{i:05d}.png")
            Image.fromarray(rgba, "RGBA").save(path, compress_level=1)
            cams.append(argparse.Namespace(image=None, image_path=path, bg=np.array([1.0, 1.0, 1.0]), image_width=W, image_height=H, image_name=str(i),
                                           world_view_transform=torch.as_tensor(c.world_view_transform.T.copy()).transpose(0, 1),
                                           full_proj_transform=torch.as_tensor(c.full_proj_transform.T.copy()).transpose(0, 1),
                                           camera_center=torch.as_tensor(c.camera_center)))
        # d: ingest (the first build also maps the library and loads the code object: it is not the one timed)
        FR.FrameStore.from_cameras(cams[:1], dev).release()
        ingest = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            store = FR.FrameStore.from_cameras(cams, dev)
            torch.cuda.synchronize()
            ingest.append(1e3 * (time.perf_counter() - t0) / N)
            if len(ingest) < 3:
                store.release()
        row["d_ingest_per_frame"] = _spread(ingest)
        row["d_decode_threads"] = min(FR.MAX_DECODE_THREADS, N)
    assert all(store.resident(i) for i in range(N))
    grp = store.groups[(H, W)]
    rgba_dev = torch.from_numpy(g.integers(0, 256, (N, H, W, 4), dtype=np.uint8)).to(dev)
    row["d_compose_device_per_frame"] = _spread([_device_ms(lambda i: store.ingest((H, W), 0, rgba_dev, (1.0, 1.0, 1.0)), 20, 3) / N for _ in range(args.rounds)])
    refs = [store.ref(i) for i in range(N)]
    # the parent's side: what a DataLoader worker hands train.py -- a pageable fp32 tensor per frame and the camera's host tensors
    hosts = [store.image(i).cpu() for i in range(N)]
    assert not hosts[0].is_pinned()

    def upload(i):
        c = cams[i % N]
        return (hosts[i % N].cuda(), _dev(c.world_view_transform, dev), _dev(c.full_proj_transform, dev), _dev(c.camera_center, dev))

    def resident(i):
        return (refs[i % N].cuda(), *store.camera(i % N))

    same = all(all(torch.equal(x, y) for x, y in zip(upload(i), resident(i))) for i in range(N))
    row["same_bits"] = bool(same)
    a, b = [], []
    for _ in range(args.rounds):
        a.append(_wall_ms(upload, args.iters, args.warmup))
        b.append(_wall_ms(resident, args.iters, args.warmup))
    row["a_upload"], row["b_resident"] = _spread(a), _spread(b)
    row["b_median_below_a_min"] = bool(statistics.median(b) < min(a))
    # c: the kernel alone
    out = torch.empty((3, H, W), device=dev)
    lib, stream = _lib.gfs(), _lib.raw_stream(dev)

    def fetch(i):
        lib.gfs_fetch(H, W, grp.frames.data_ptr(), grp.capacity, i % N, store.table.data_ptr(), out.data_ptr(), stream)

    c = [_device_ms(fetch, args.iters, args.warmup) for _ in range(args.rounds)]
    row["c_fetch_device"] = _spread(c)
    moved = grp.stride + 12 * H * W
    row["c_fetch_bytes"] = moved
    row["c_fetch_GBps_at_median"] = moved / (statistics.median(c) * 1e-3) / 1e9
    row["c_note"] = "back-to-back launches by device events: the rate includes the launch gaps of a 6.6 MB pass"
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
