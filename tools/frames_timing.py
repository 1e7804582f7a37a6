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

    e  resize     a second JSON line (resize_row below): a store under `resample=True` over files of 3208 x 2200 for cameras of 802 x 550,
                  per frame, against the reference's worker `__getitem__` plus upload per iteration; the two resize kernels alone

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
    ap.add_argument("--resize-frames", type=int, default=4, help="frames of the resize line (0: leave it out)")
    ap.add_argument("--resize-from", type=int, nargs=2, default=(2200, 3208), metavar=("H", "W"), help="size of the files of the resize line")
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
    store.release()
    if args.resize_frames > 0:
        print(json.dumps(resize_row(args, dev)), flush=True)


def worker_getitem(camera):
    """What a DataLoader worker of the reference does for a camera whose size is not its file's (scene/__init__.py:41-63, PILtoTorch): decode,
    the fp64 composite on the host, bytes, `resize`, / 255, clamp -> the pageable fp32 tensor train.py:128 uploads."""
    from PIL import Image

    n = np.array(Image.open(camera.image_path).convert("RGBA")) / 255.0
    arr = n[:, :, :3] * n[:, :, 3:4] + camera.bg * (1 - n[:, :, 3:4])
    image = Image.fromarray(np.array(arr * 255.0, dtype=np.byte).view(np.uint8), "RGB").resize((camera.image_width, camera.image_height))
    return (torch.from_numpy(np.array(image)) / 255.0).permute(2, 0, 1).clamp(0.0, 1.0)


def resize_row(args, dev):
    """e  resize: files of --resize-from (3208 x 2200) for cameras of a quarter of that (802 x 550).  The build of a store over them under
    `resample=True` (decode on the thread pool, upload, gfs_compose at the file's size, gfs_resample), per frame and once; against what the
    path it replaces costs per ITERATION: worker_getitem in this process plus the `.cuda()` of its result (in training the first half runs in
    a DataLoader worker, beside the step rather than inside it, and crosses a queue, which is not timed here).  The two kernels alone by
    device events, with the bytes they have to move."""
    from PIL import Image

    Hs, Ws = args.resize_from
    H, W, N = Hs // 4, Ws // 4, args.resize_frames
    g = np.random.default_rng(12)
    row = {"resize": {"file": [Hs, Ws], "image": [H, W]}, "frames": N, "pillow": Image.__version__}
    with tempfile.TemporaryDirectory() as tmp:
        cams = []
        for i in range(N):
            c = S.orbit_camera(W, H, yaw_deg=10.0 * i)
            rgba = g.integers(0, 256, (Hs, Ws, 4), dtype=np.uint8)
            rgba[..., 3] = np.where(g.random((Hs, Ws)) < 0.7, 255, rgba[..., 3])
            path = os.path.join(tmp, f"{i:05d}.png")
            Image.fromarray(rgba, "RGBA").save(path, compress_level=1)
            cams.append(argparse.Namespace(image=None, image_path=path, bg=np.array([1.0, 1.0, 1.0]), image_width=W, image_height=H, image_name=str(i),
                                           world_view_transform=torch.as_tensor(c.world_view_transform.T.copy()).transpose(0, 1),
                                           full_proj_transform=torch.as_tensor(c.full_proj_transform.T.copy()).transpose(0, 1),
                                           camera_center=torch.as_tensor(c.camera_center)))
        FR.FrameStore.from_cameras(cams[:1], dev, resample=True).release()   # (maps the library, loads the code object, builds the tables)
        build = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            store = FR.FrameStore.from_cameras(cams, dev, resample=True)
            torch.cuda.synchronize()
            build.append(1e3 * (time.perf_counter() - t0) / N)
            if len(build) < 3:
                store.release()
        row["e_build_per_frame"] = _spread(build)
        row["e_decode_threads"] = min(FR.MAX_DECODE_THREADS, N)
        replaced, same = [], True
        for _ in range(3):
            for i, cam in enumerate(cams):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                gt = worker_getitem(cam).cuda()
                torch.cuda.synchronize()
                replaced.append(1e3 * (time.perf_counter() - t0))
                same = same and torch.equal(gt, store.image(i))
        row["e_replaced_per_iteration"] = _spread(replaced)
        row["e_same_bits"] = bool(same)
    assert all(store.resident(i) for i in range(N))
    # the two passes alone, over the N composited source-size frames
    staging = FR._Staging(dev)
    src, out = staging.group((Hs, Ws)), store.groups[(H, W)]
    src.frames.copy_(torch.from_numpy(g.integers(0, 256, src.frames.numel(), dtype=np.uint8)))
    kx, bx, ksx = staging.axis(Ws, W)
    ky, by, ksy = staging.axis(Hs, H)
    lib, stream = _lib.gfs(), _lib.raw_stream(dev)
    tmp_dev = staging.between(lib.gfs_resample_tmp_bytes(Hs, W, N))
    _lib.gfs_profile_enable(True)
    for _ in range(3 + args.rounds):
        rc = lib.gfs_resample(Hs, Ws, src.frames.data_ptr(), src.capacity, 0, H, W, kx, bx, ksx, ky, by, ksy, tmp_dev.data_ptr(), out.frames.data_ptr(),
                              out.capacity, 0, N, stream)
        assert rc == 0, _lib.gfs_error()
    prof = _lib.gfs_profile_read()
    _lib.gfs_profile_enable(False)
    moved = {"gfs::k_resample_h": N * (FR.frame_stride(Hs, Ws) + FR.frame_stride(Hs, W)), "gfs::k_resample_v": N * (FR.frame_stride(Hs, W) + FR.frame_stride(H, W))}
    for name, nbytes in moved.items():
        ms, launches = prof[name]
        row["e_" + name.split("::")[1]] = {"mean_ms_per_launch": ms / launches, "launches": launches, "frames_per_launch": N, "bytes": nbytes,
                                           "GBps": nbytes / (ms / launches * 1e-3) / 1e9}
    row["e_note"] = "kernel times: an event pair around each launch (the library's profile shim), code objects loaded by the builds before"
    store.release()
    return row


if __name__ == "__main__":
    main()
