"""Training frames resident in HBM, on the kernels of include/gfs.h: the ground truth of every frame as the 8-bit RGB image it is by
construction, the cameras' matrices beside it, and nothing uploaded per iteration.

    FrameStore.from_cameras(cameras, device)   decodes every camera's image once (PIL, a thread pool), uploads the RGBA bytes and composites
                                               them over the camera's background on the device (gfs_compose: scene/__init__.py:48-51, fp64)
    store.image(i)                             `original_image` of camera i, planar fp32 (3,H,W), from one launch (gfs_fetch)
    store.camera(i)                            (world_view_transform, full_proj_transform, camera_center) as views into one device block
    FrameRef                                   the picklable placeholder a resident camera carries as `original_image`
    ResidentCameraDataset                      scene.CameraDataset over a store: train.py's DataLoader line runs on it unchanged

The reference composes, quantises to bytes, divides by 255 and clamps for every frame of every epoch in a DataLoader worker
(scene/__init__.py:38-63), ships the 3xHxW fp32 result across a process boundary and uploads it from pageable memory (train.py:128).  Here a
worker's `__getitem__` copies the camera and attaches two small Python objects; the bytes never leave the device.

A frame is resident when its background is three numbers, its three camera tensors are fp32, the store's byte budget still has room and its
file decodes to the camera's own `image_width` x `image_height` -- or, under `from_cameras(..., resample=True)`, to any other size: the
composited bytes then go through PILtoTorch's `pil_image.resize(resolution)` (utils/general_utils.py:22) on the way in, restated exactly:
Pillow's bicubic resize of an 8-bit image is two integer passes over fixed-point coefficients (resample_tables, resample_composed,
gfs_resample), and the frame is stored at the camera's size like any other.  Without `resample` PIL's resampling is not restated and such a
frame is not resident.  Every frame that is not resident keeps the reference's path, frame by frame.

Device stores run on the kernels.  Host stores, and GAA_FRAME_STORE=0, evaluate the composed torch expressions below, which give the same
bits and are what the CPU tests hold to the pins.  A missing library is an error, never a reason to take the composed path.
"""
from __future__ import annotations

import ctypes as C
import functools
import itertools
import math
import os
from copy import deepcopy

import numpy as np
import torch

from . import _lib

MAX_DECODE_THREADS = 16   # a fixed ceiling: the machine's CPU count says nothing about the share of it this process may use
_CHUNK = 32               # frames decoded, uploaded and composited together


def fused_default() -> bool:
    """GAA_FRAME_STORE=0: no adoption by patch_reference(), and every call takes the composed-torch path (A/B runs)."""
    return os.environ.get("GAA_FRAME_STORE", "1") != "0"


def resize_default() -> bool:
    """GAA_FRAME_STORE_RESIZE=1: the stores patch.adopt_frame_store builds also hold the frames whose camera asks for another size than its
    file's (`from_cameras(..., resample=True)`).  Off unless set; read where GAA_FRAME_STORE is, when a store is built."""
    return os.environ.get("GAA_FRAME_STORE_RESIZE", "0") == "1"


def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {_lib.gfs_error()}")


def frame_stride(H: int, W: int) -> int:
    """include/gfs.h: gfs_frame_stride -- bytes from one stored frame to the next (whole groups of four pixels, a multiple of 16)."""
    return ((H * W + 3) // 4 * 12 + 15) // 16 * 16


def byte_table() -> torch.Tensor:
    """The 256 floats a byte of the ground truth can become: PILtoTorch's `torch.from_numpy(bytes) / 255.0` (utils/general_utils.py:23) on
    every byte value, computed by torch on the host, so that a fetched image holds torch's bits by construction."""
    return torch.arange(256, dtype=torch.uint8) / 255.0


# ---- the composed-torch restatement (host stores, GAA_FRAME_STORE=0) ---------------------------------------------------------------------
def compose_composed(rgba: torch.Tensor, bg) -> torch.Tensor:
    """scene/__init__.py:48-51 on a (..., H, W, 4) uint8 tensor: fp64 throughout, in the reference's order; truncation toward zero and the
    low 8 bits, which is what `np.array(arr * 255.0, dtype=np.byte)` read as "RGB" holds.  -> (..., H, W, 3) uint8."""
    # byte / 255.0 through a table numpy divides on the host: torch's device division by a host scalar multiplies by a reciprocal instead
    n = torch.from_numpy(np.arange(256) / 255.0).to(rgba.device)[rgba.to(torch.int64)]
    b = torch.as_tensor(np.asarray(bg, np.float64).reshape(3), device=rgba.device)
    arr = n[..., :3] * n[..., 3:4] + b * (1 - n[..., 3:4])
    return (arr * 255.0).to(torch.int32).to(torch.uint8)


def fetch_composed(rgb: torch.Tensor, table: torch.Tensor | None = None) -> torch.Tensor:
    """scene/__init__.py:54-62 at the file's own size on a (H, W, 3) uint8 tensor: PILtoTorch's division, the permute, the clamp.  On a device the
    division is a look-up in `table` (byte_table(), divided on the host), for the reason compose_composed gives."""
    f = rgb / 255.0 if table is None else table[rgb.to(torch.int64)]
    return f.permute(2, 0, 1).clamp(0.0, 1.0)


# ---- Pillow's bicubic resize of 8-bit images, restated (libImaging/Resample.c) -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def resample_tables(in_size: int, out_size: int):
    """One axis of `PIL.Image.resize` with its defaults (bicubic): -> (coefficients int32 (out, ksize), bounds int32 (out, 2)) as host tensors,
    bounds[i] = (first source index, taps) and coefficients[i, taps:] = 0; None when the size does not change (Pillow skips that axis).
    precompute_coeffs and normalize_coeffs_8bpc in IEEE doubles, operation by operation in Resample.c's order, on the host: the weights are
    summed tap by tap (no pairwise sum), divided by the sum, scaled by 2^22 and rounded half away from zero by a truncation.  Computed once per
    (in, out) and shared: the tensors are not to be written."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size <= 0 or out_size <= 0:
        raise ValueError(f"resample_tables({in_size}, {out_size}): sizes must be positive")
    if in_size == out_size:
        return None
    scale = np.float64(in_size) / np.float64(out_size)
    fs = max(scale, np.float64(1.0))
    support = np.float64(2.0) * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = np.float64(1.0) / fs
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    first = np.maximum((center - support + 0.5).astype(np.int64), 0)             # (a C cast: toward zero)
    taps = np.minimum((center + support + 0.5).astype(np.int64), in_size) - first
    tap = np.arange(ksize, dtype=np.int64)[None, :]
    t = np.abs(((tap + first[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss)
    a = np.float64(-0.5)
    near = ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    far = (((t - 5) * t + 8) * t - 4) * a
    w = np.where(tap < taps[:, None], np.where(t < 1.0, near, np.where(t < 2.0, far, 0.0)), 0.0)
    total = np.zeros(out_size, np.float64)
    for x in range(ksize):                                                        # in index order, as the C loop adds them
        total = total + w[:, x]
    w = np.where(total[:, None] != 0.0, w / np.where(total != 0.0, total, 1.0)[:, None], w)
    fixed = np.where(w < 0, -0.5 + w * float(1 << 22), 0.5 + w * float(1 << 22)).astype(np.int64).astype(np.int32)
    return torch.from_numpy(np.ascontiguousarray(fixed)), torch.from_numpy(np.ascontiguousarray(np.stack([first, taps], axis=1).astype(np.int32)))


def _resample_axis(x: torch.Tensor, dim: int, tables) -> torch.Tensor:
    """ImagingResampleHorizontal_8bpc / Vertical_8bpc along `dim` of a uint8 tensor: int32 products and sum, 2^21 added, an arithmetic shift by
    22, the clamp to a byte.  One gather per tap, so nothing larger than the output is ever held."""
    coef, bounds = (t.to(x.device) for t in tables)
    first, last = bounds[:, 0].to(torch.int64), (bounds[:, 1] - 1).to(torch.int64)
    shape = [1] * x.dim()
    shape[dim] = coef.shape[0]
    x = x.to(torch.int32)
    acc = None
    for t in range(coef.shape[1]):
        term = x.index_select(dim, first + torch.clamp(last, max=t)) * coef[:, t].view(shape)   # (behind its taps a coefficient is zero)
        acc = term + (1 << 21) if acc is None else acc + term
    return (acc >> 22).clamp(0, 255).to(torch.uint8)


def resample_composed(rgb, size):
    """`Image.fromarray(rgb, "RGB").resize(size)` on (..., H, W, 3) uint8, torch (any device) or numpy, `size` = (width, height) as PIL takes it:
    the horizontal axis first, bytes in between, the vertical axis second, an unchanged axis skipped.  -> (..., height, width, 3) uint8 of the
    same kind."""
    if isinstance(rgb, np.ndarray):
        return resample_composed(torch.from_numpy(np.ascontiguousarray(rgb)), size).numpy()
    if rgb.dtype is not torch.uint8 or rgb.dim() < 3 or rgb.shape[-1] != 3:
        raise ValueError(f"resample_composed takes (..., H, W, 3) uint8, got {tuple(rgb.shape)} {rgb.dtype}")
    W, H = int(size[0]), int(size[1])
    for dim, want in ((rgb.dim() - 2, W), (rgb.dim() - 3, H)):
        tables = resample_tables(rgb.shape[dim], want)
        if tables is not None:
            rgb = _resample_axis(rgb, dim, tables)
    return rgb.contiguous()


class _Staging:
    """What the resize needs while a store is built and not afterwards: a group of _CHUNK frames per source size, the image between the two
    passes, and the tables on the device."""

    def __init__(self, device):
        self.device, self.groups, self.tmp, self.tables = device, {}, None, {}

    def group(self, hw):
        if hw not in self.groups:
            self.groups[hw] = _Group(hw[0], hw[1], _CHUNK, self.device)
        return self.groups[hw]

    def axis(self, in_size, out_size):
        """(coefficients pointer, bounds pointer, ksize) of one axis on the device; (None, None, 0) when the size does not change."""
        if in_size == out_size:
            return None, None, 0
        if (in_size, out_size) not in self.tables:
            self.tables[(in_size, out_size)] = tuple(t.to(self.device) for t in resample_tables(in_size, out_size))
        coef, bounds = self.tables[(in_size, out_size)]
        return coef.data_ptr(), bounds.data_ptr(), coef.shape[1]

    def between(self, nbytes):
        if self.tmp is None or self.tmp.numel() < nbytes:
            self.tmp = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self.tmp


# ---- the process-local registry ------------------------------------------------------------------------------------------------------------
_STORES: dict = {}            # key -> FrameStore, in the process that built it
_counter = itertools.count()


def lookup(key) -> "FrameStore":
    """The store of `key` in THIS process.  A forked DataLoader worker inherits the parent's dictionary but must never touch the device: a store
    answers only to the process that built it."""
    store = _STORES.get(key)
    if store is None or store.pid != os.getpid():
        raise RuntimeError(f"frame store {key!r} is not held by this process (pid {os.getpid()}): a FrameRef materialises only in the process that "
                           "built its FrameStore -- DataLoader workers pass it on untouched")
    return store


def release(key) -> None:
    """Drops a store from the registry (its device memory goes when the last reference does)."""
    _STORES.pop(key, None)


class FrameRef:
    """What a resident camera carries as `original_image`: a store key, a frame index and the image's shape -- no tensor, so it crosses a
    DataLoader worker queue and `pin_memory` untouched.  `.cuda()`, `.to(...)` and `[...]` fetch the frame in the process that holds the
    store and return (or act on) that fresh (3,H,W) fp32 tensor on the store's device; `.shape`, `.dtype` and `.device` answer without
    fetching, `.device` with the device the fetched tensor will be on.  Any other attribute is forwarded to the fetched tensor."""
    __slots__ = ("key", "index", "_shape", "_device")

    def __init__(self, key, index, shape, device):
        self.key, self.index, self._shape, self._device = key, int(index), tuple(int(s) for s in shape), str(device)

    def __reduce__(self):
        return (FrameRef, (self.key, self.index, self._shape, self._device))

    def __repr__(self):
        return f"FrameRef(key={self.key!r}, index={self.index}, shape={self._shape}, device={self._device!r})"

    shape = property(lambda self: torch.Size(self._shape))
    dtype = property(lambda self: torch.float32)
    device = property(lambda self: torch.device(self._device))

    def size(self, dim=None):
        return self.shape if dim is None else self._shape[dim]

    def dim(self):
        return len(self._shape)

    def pin_memory(self, *a, **k):
        return self   # (there is nothing on the host to pin)

    def materialize(self) -> torch.Tensor:
        return lookup(self.key).image(self.index)

    def cuda(self, *a, **k):
        t = self.materialize()
        return t if t.is_cuda and not a and not k else t.cuda(*a, **k)

    def to(self, *a, **k):
        return self.materialize().to(*a, **k)

    def __getitem__(self, idx):
        return self.materialize()[idx]

    def __getattr__(self, name):
        if name.startswith("__"):   # (pickle and copy probe for protocol methods: those are not the tensor's to answer)
            raise AttributeError(name)
        return getattr(self.materialize(), name)


class _Group:
    """The frames of one (H, W): `capacity` frames of `stride` bytes in one uint8 tensor."""
    __slots__ = ("H", "W", "stride", "capacity", "frames", "count")

    def __init__(self, H, W, capacity, device):
        self.H, self.W, self.stride, self.capacity, self.count = H, W, frame_stride(H, W), capacity, 0
        self.frames = torch.empty(capacity * self.stride, dtype=torch.uint8, device=device)


def _image_size(camera):
    """(width, height) of the camera's image as PIL reports it, without decoding the pixels; None when it cannot be opened."""
    from PIL import Image

    try:
        if camera.image is not None:
            return tuple(camera.image.size)
        with Image.open(camera.image_path) as im:
            return tuple(im.size)
    except Exception:
        return None


def _decode(camera) -> np.ndarray:
    """scene/__init__.py:43-48: the camera's image, or its file, as (H, W, 4) uint8."""
    from PIL import Image

    image = Image.open(camera.image_path) if camera.image is None else camera.image
    return np.ascontiguousarray(np.array(image.convert("RGBA")))


def _camera_row(camera):
    """The 35 floats `gaussian_renderer._dev` would upload for this camera (contiguous copies of the two 4x4 matrices and the centre), or None
    when they are not three fp32 tensors of those shapes."""
    ts = [getattr(camera, n, None) for n in ("world_view_transform", "full_proj_transform", "camera_center")]
    shapes = ((4, 4), (4, 4), (3,))
    for t, s in zip(ts, shapes):
        if not isinstance(t, torch.Tensor) or t.dtype is not torch.float32 or tuple(t.shape) != s:
            return None
    return np.concatenate([np.ascontiguousarray(t.detach().cpu().numpy()).reshape(-1) for t in ts])


def _background(camera):
    try:
        bg = np.asarray(camera.bg, np.float64).reshape(-1)
    except (TypeError, ValueError, AttributeError):
        return None
    return bg if bg.shape == (3,) else None


def default_budget(device) -> int | None:
    """Bytes a store may take when the caller does not say: GAA_FRAME_STORE_GB (GiB) if set, else HALF of the device memory that is free when
    the store is built.  The half is a policy -- room for the model, its optimizer state and the rasterizer's buffers, none of which exist
    yet at that point -- not a measurement of what training needs.  A host store without the variable is not limited."""
    gb = os.environ.get("GAA_FRAME_STORE_GB")
    if gb is not None:
        return int(float(gb) * (1 << 30))
    if device.type == "cuda":
        return int(torch.cuda.mem_get_info(device)[0] // 2)
    return None


class FrameStore:
    """The resident frames of a list of cameras: one padded uint8 tensor per (H, W) group and one (N, 35) fp32 block of camera data, on
    `device`.  Indices are positions in the camera list the store was built from; `resident(i)` says whether frame i is held."""

    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.pid = os.getpid()
        self.key = f"{self.pid}-{next(_counter)}"
        self.groups: dict = {}      # (H, W) -> _Group
        self.where: list = []       # per camera: ((H, W), slot) or None
        self.cameras = None         # (N, 35) fp32 on the device; a row of zeros for a camera that is not resident
        self.table = byte_table().to(self.device)
        self.bytes = 0
        _STORES[self.key] = self

    # ---- building ---------------------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_cameras(cls, cameras, device, budget_bytes=None, resample=False) -> "FrameStore":
        """Decodes each camera's `image` or `image_path` with PIL `convert("RGBA")` on a pool of at most MAX_DECODE_THREADS threads, uploads
        the raw RGBA bytes and composites them over `camera.bg` on the device.  `budget_bytes`: what the frames may take (default_budget()
        when None); the cameras are admitted in order until it is spent, the rest stay non-resident.  `resample`: a camera whose file is
        not `image_width` x `image_height` is admitted too, and its composited bytes are resized to that size as PIL would (gfs_resample);
        the frame is stored, and counted against the budget, at the camera's size.  The source-size staging lives only during this call."""
        self = cls(device)
        cameras = list(cameras)
        budget = default_budget(self.device) if budget_bytes is None else int(budget_bytes)
        plan, rows, capacity, used = [], [], {}, 0   # plan: per camera (its group (H, W), slot, background, the file's (H, W)) or None
        for cam in cameras:
            size, bg, row = _image_size(cam), _background(cam), _camera_row(cam)
            ok = size is not None and bg is not None and row is not None and size[0] > 0 and size[1] > 0
            if ok:
                want = (int(cam.image_width), int(cam.image_height))
                ok = size == want or (resample and want[0] > 0 and want[1] > 0)
            if ok:
                need = frame_stride(want[1], want[0])
                ok = budget is None or used + need <= budget
            if ok:
                used += need
                hw = (want[1], want[0])
                plan.append((hw, capacity.get(hw, 0), bg, (size[1], size[0])))
                capacity[hw] = capacity.get(hw, 0) + 1
            else:
                plan.append(None)
            rows.append(row if ok else np.zeros(35, np.float32))
        self.bytes = used
        self.groups = {hw: _Group(hw[0], hw[1], n, self.device) for hw, n in capacity.items()}
        self.where = [None if p is None else (p[0], p[1]) for p in plan]
        self.cameras = torch.from_numpy(np.stack(rows).astype(np.float32) if rows else np.zeros((0, 35), np.float32)).to(self.device)
        todo = [i for i, p in enumerate(plan) if p is not None]
        if todo:
            from concurrent.futures import ThreadPoolExecutor

            staging = _Staging(self.device)
            with ThreadPoolExecutor(max_workers=min(MAX_DECODE_THREADS, len(todo))) as pool:
                for c0 in range(0, len(todo), _CHUNK):
                    chunk = todo[c0:c0 + _CHUNK]
                    images = list(pool.map(_decode, [cameras[i] for i in chunk]))
                    # runs of consecutive frames of one group, one file size and one background go up together: their slots are consecutive too
                    a = 0
                    while a < len(chunk):
                        hw, slot, bg, file_hw = plan[chunk[a]]
                        b = a + 1
                        while b < len(chunk) and plan[chunk[b]][0] == hw and plan[chunk[b]][3] == file_hw and np.array_equal(plan[chunk[b]][2], bg):
                            b += 1
                        if any(im.shape != (file_hw[0], file_hw[1], 4) for im in images[a:b]):
                            raise RuntimeError(f"an image of {cameras[chunk[a]].image_name!r} .. changed size between the header and the decode")
                        rgba = torch.from_numpy(np.stack(images[a:b]))
                        if file_hw == hw:
                            self.ingest(hw, slot, rgba, bg)
                        else:
                            self.ingest_resized(hw, slot, rgba, bg, staging)
                        a = b
        return self

    def ingest_resized(self, hw, first: int, rgba: torch.Tensor, bg, staging: "_Staging | None" = None) -> None:
        """Composites `rgba` ((n, Hs, Ws, 4) uint8 of any size, host or device) over `bg` at its own size and resizes the bytes to the group `hw`
        as `PIL.Image.resize` would, into frames first .. first + n - 1: the upload, gfs_compose into a staging group of the source size,
        gfs_resample from there into the slots, _CHUNK frames at a time.  `staging` is reused across calls by from_cameras and dropped with it."""
        g = self.groups[tuple(hw)]
        n, HW3 = rgba.shape[0], g.H * g.W * 3
        if rgba.dtype is not torch.uint8 or rgba.dim() != 4 or rgba.shape[3] != 4 or min(rgba.shape) < 1 or first < 0 or first + n > g.capacity:
            raise ValueError(f"ingest of {tuple(rgba.shape)} at {first} into a group of {g.capacity} frames of {(g.H, g.W)}")
        Hs, Ws = int(rgba.shape[1]), int(rgba.shape[2])
        if (Hs, Ws) == (g.H, g.W):
            return self.ingest(hw, first, rgba, bg)
        bg = np.asarray(bg, np.float64).reshape(3)
        if self.device.type == "cuda" and fused_default():
            staging = _Staging(self.device) if staging is None else staging
            src, lib, stream = staging.group((Hs, Ws)), _lib.gfs(), _lib.raw_stream(self.device)
            kx, bx, ksx = staging.axis(Ws, g.W)
            ky, by, ksy = staging.axis(Hs, g.H)
            tmp = staging.between(lib.gfs_resample_tmp_bytes(Hs, g.W, src.capacity)).data_ptr() if ksx and ksy else None
            with _lib.on_device(self.device):
                for a in range(0, n, src.capacity):
                    k = min(src.capacity, n - a)
                    part = rgba[a:a + k].to(self.device).contiguous()
                    _check(lib.gfs_compose(Hs, Ws, part.data_ptr(), (C.c_double * 3)(*bg), src.frames.data_ptr(), src.capacity, 0, k, stream), "gfs_compose")
                    _check(lib.gfs_resample(Hs, Ws, src.frames.data_ptr(), src.capacity, 0, g.H, g.W, kx, bx, ksx, ky, by, ksy, tmp, g.frames.data_ptr(),
                                            g.capacity, first + a, k, stream), "gfs_resample")
        else:
            for a in range(n):   # (a frame at a time: the fp64 composite of a source-size image is eight times its bytes)
                part = compose_composed(rgba[a].to(self.device), bg)
                g.frames.view(g.capacity, g.stride)[first + a, :HW3] = resample_composed(part, (g.W, g.H)).reshape(HW3)
        g.count = max(g.count, first + n)

    def ingest(self, hw, first: int, rgba: torch.Tensor, bg) -> None:
        """Composites `rgba` ((n, H, W, 4) uint8, host or device) over `bg` into frames first .. first + n - 1 of the group `hw`."""
        g = self.groups[tuple(hw)]
        n, HW3 = rgba.shape[0], g.H * g.W * 3
        if rgba.dtype is not torch.uint8 or tuple(rgba.shape[1:]) != (g.H, g.W, 4) or first < 0 or first + n > g.capacity:
            raise ValueError(f"ingest of {tuple(rgba.shape)} at {first} into a group of {g.capacity} frames of {(g.H, g.W)}")
        rgba = rgba.to(self.device).contiguous()
        bg = np.asarray(bg, np.float64).reshape(3)
        if self.device.type == "cuda" and fused_default():
            with _lib.on_device(self.device):
                for a in range(0, n, _lib.GFS_MAX_BATCH):
                    k = min(_lib.GFS_MAX_BATCH, n - a)
                    _check(_lib.gfs().gfs_compose(g.H, g.W, rgba[a:a + k].data_ptr(), (C.c_double * 3)(*bg), g.frames.data_ptr(), g.capacity,
                                                  first + a, k, _lib.raw_stream(self.device)), "gfs_compose")
        else:
            g.frames.view(g.capacity, g.stride)[first:first + n, :HW3] = compose_composed(rgba, bg).reshape(n, HW3)
        g.count = max(g.count, first + n)

    # ---- reading ----------------------------------------------------------------------------------------------------------------------------
    def __len__(self):
        return len(self.where)

    def resident(self, i: int) -> bool:
        return 0 <= i < len(self.where) and self.where[i] is not None

    def _slot(self, i):
        if not self.resident(i):
            raise IndexError(f"frame {i} is not resident in store {self.key!r}")
        hw, slot = self.where[i]
        return self.groups[hw], slot

    def shape(self, i: int):
        g, _ = self._slot(i)
        return (3, g.H, g.W)

    def ref(self, i: int) -> FrameRef:
        return FrameRef(self.key, i, self.shape(i), self.device)

    def rgb(self, i: int) -> torch.Tensor:
        """The stored bytes of frame i as a (H, W, 3) uint8 view."""
        g, slot = self._slot(i)
        return g.frames.view(g.capacity, g.stride)[slot, :g.H * g.W * 3].view(g.H, g.W, 3)

    def image(self, i: int) -> torch.Tensor:
        """`original_image` of camera i: a fresh planar fp32 (3, H, W) tensor on the store's device, the bits of scene/__init__.py:54-62."""
        g, slot = self._slot(i)
        if not (self.device.type == "cuda" and fused_default()):
            return fetch_composed(self.rgb(i), None if self.device.type == "cpu" else self.table).contiguous()
        out = torch.empty((3, g.H, g.W), dtype=torch.float32, device=self.device)
        with _lib.on_device(self.device):
            _check(_lib.gfs().gfs_fetch(g.H, g.W, g.frames.data_ptr(), g.capacity, slot, self.table.data_ptr(), out.data_ptr(),
                                        _lib.raw_stream(self.device)), "gfs_fetch")
        return out

    def camera(self, i: int):
        """(world_view_transform (4,4), full_proj_transform (4,4), camera_center (3,)) of camera i: contiguous fp32 views into the camera block,
        the values `gaussian_renderer._dev` would upload."""
        if not self.resident(i):
            raise IndexError(f"camera {i} is not resident in store {self.key!r}")
        row = self.cameras[i]
        return row[0:16].view(4, 4), row[16:32].view(4, 4), row[32:35]

    def release(self) -> None:
        release(self.key)


# ---- the device-indexed entries (one (H, W) group at a time; slots are positions inside the group) -------------------------------------------
def _group_of(store, hw):
    if store.device.type != "cuda":
        raise ValueError("the device-indexed fetches run on a device store only (there is no CPU implementation)")
    g = store.groups[tuple(hw)]
    return g


def fetch_indexed(store: FrameStore, hw, slot: torch.Tensor, out: torch.Tensor, flag: torch.Tensor) -> torch.Tensor:
    """gfs_fetch_indexed: the frame of group `hw` whose slot is the device int64 `slot` -> `out` ((3,H,W) fp32).  No host read: the call can
    be stream-captured and replayed after `slot` has been overwritten.  A slot outside the group writes nothing and sets bit
    GFS_FLAG_RANGE of `flag` (device int32, zeroed by the caller)."""
    g = _group_of(store, hw)
    if slot.dtype is not torch.int64 or slot.numel() != 1 or flag.dtype is not torch.int32 or tuple(out.shape) != (3, g.H, g.W) \
            or out.dtype is not torch.float32 or not out.is_contiguous() or not all(t.device == store.device for t in (slot, out, flag)):
        raise ValueError("fetch_indexed takes one device int64 slot, a contiguous fp32 (3,H,W) output and a device int32 flag")
    with _lib.on_device(store.device):
        _check(_lib.gfs().gfs_fetch_indexed(g.H, g.W, g.frames.data_ptr(), g.capacity, slot.data_ptr(), store.table.data_ptr(), out.data_ptr(),
                                            flag.data_ptr(), _lib.raw_stream(store.device)), "gfs_fetch_indexed")
    return out


def fetch_batch(store: FrameStore, hw, slots: torch.Tensor, flag: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """gfs_fetch_batch: K frames of group `hw` by a device int64 list of slots -> (K, 3, H, W) fp32, in one launch (frame_parallel and
    multi-lane callers)."""
    g = _group_of(store, hw)
    K = int(slots.numel())
    if slots.dtype is not torch.int64 or slots.device != store.device or not slots.is_contiguous() or not 1 <= K <= _lib.GFS_MAX_BATCH:
        raise ValueError(f"fetch_batch takes 1 .. {_lib.GFS_MAX_BATCH} contiguous device int64 slots")
    if flag is None:
        flag = torch.zeros(1, dtype=torch.int32, device=store.device)
    if out is None:
        out = torch.empty((K, 3, g.H, g.W), dtype=torch.float32, device=store.device)
    elif tuple(out.shape) != (K, 3, g.H, g.W) or out.dtype is not torch.float32 or not out.is_contiguous() or out.device != store.device:
        raise ValueError("`out` must be a contiguous fp32 (K,3,H,W) tensor on the store's device")
    with _lib.on_device(store.device):
        _check(_lib.gfs().gfs_fetch_batch(g.H, g.W, g.frames.data_ptr(), g.capacity, slots.data_ptr(), K, store.table.data_ptr(), out.data_ptr(),
                                          flag.data_ptr(), _lib.raw_stream(store.device)), "gfs_fetch_batch")
    return out


# ---- the dataset -----------------------------------------------------------------------------------------------------------------------------
class ResidentCameraDataset(torch.utils.data.Dataset):
    """scene.CameraDataset (scene/__init__.py:31-67) over a FrameStore: the same `__len__`, int and slice indexing and `deepcopy` of the camera.
    For a resident frame `__getitem__` only sets `original_image = FrameRef(...)` on the copy and tags it `_gaa_frame = (key, index)`; every
    other frame runs `fallback`'s own `__getitem__` (the reference's dataset over the same camera list)."""

    def __init__(self, cameras, store: FrameStore, fallback=None):
        self.cameras = cameras
        self.fallback = fallback
        self.key = store.key
        # what a worker needs, without the store: per frame its index in the store and, when resident, its shape
        self.indices = list(range(len(cameras)))
        self.shapes = [store.shape(i) if store.resident(i) else None for i in self.indices]
        self.device = str(store.device)

    def __len__(self):
        return len(self.cameras)

    def __getitem__(self, idx):
        if isinstance(idx, int):
            shape = self.shapes[idx]
            if shape is None:
                if self.fallback is None:
                    raise RuntimeError(f"frame {idx} is not resident and the dataset has no fallback")
                return self.fallback[idx]
            camera = deepcopy(self.cameras[idx])
            i = self.indices[idx]
            camera.original_image = FrameRef(self.key, i, shape, self.device)
            camera._gaa_frame = (self.key, i)
            return camera
        elif isinstance(idx, slice):
            sub = ResidentCameraDataset.__new__(ResidentCameraDataset)
            sub.cameras, sub.fallback = self.cameras[idx], (None if self.fallback is None else self.fallback[idx])
            sub.key, sub.indices, sub.shapes, sub.device = self.key, self.indices[idx], self.shapes[idx], self.device
            return sub
        else:
            raise TypeError("Invalid argument type")


def resident_camera(camera, device):
    """The three device tensors of a camera tagged `_gaa_frame` whose store this process holds on `device`; None for every other camera
    (gaussian_renderer then uploads the camera's own tensors, as before)."""
    tag = getattr(camera, "_gaa_frame", None)
    if tag is None:
        return None
    store = _STORES.get(tag[0])
    if store is None or store.pid != os.getpid() or store.device != device or not store.resident(tag[1]):
        return None
    return store.camera(tag[1])
