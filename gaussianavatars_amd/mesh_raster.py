"""The mesh overlay: nvdiffrast's `rasterize` and `antialias` as the reference's NVDiffRenderer.render_mesh calls them
(mesh_renderer/__init__.py), on the HIP kernels of include/gmr.h.  Forward only.

    rasterize(glctx, pos, tri, resolution)  ->  (rast (B,H,W,4) = (u, v, z/w, triangle_id + 1), rast_db (B,H,W,0))
    antialias(color, rast, pos, tri)        ->  color with analytic silhouette blending, same shape

The contract (pixel centres, the clip-space fragment test, depth order, the blend) is DESIGN.md section 10; it follows nvdiffrast's
published conventions, and bit parity with nvdiffrast is not claimed.  Every argument is checked here before any launch; a CUDA tensor
is required last, so the checks run on host tensors too.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

MAX_TRIANGLES = _lib.GMR_MAX_TRIANGLES


# ---- validation ----------------------------------------------------------------------------------------------------------------------
def _tensor(name, x, dtype, rank):
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(x).__name__}")
    if x.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {x.dtype}")
    if x.dim() != rank:
        raise ValueError(f"{name} must have rank {rank}, got shape {tuple(x.shape)}")


def _check_pos_tri(pos, tri):
    if isinstance(pos, torch.Tensor) and pos.dim() == 2:
        raise ValueError("pos of rank 2 is nvdiffrast's range mode, which is not supported: pass pos as (B, V, 4)")
    _tensor("pos", pos, torch.float32, 3)
    if pos.shape[2] != 4:
        raise ValueError(f"pos must be (B, V, 4), got {tuple(pos.shape)}")
    if pos.shape[0] < 1:
        raise ValueError("pos must hold at least one batch element")
    _tensor("tri", tri, torch.int32, 2)
    if tri.shape[1] != 3:
        raise ValueError(f"tri must be (F, 3), got {tuple(tri.shape)}")
    F, V = tri.shape[0], pos.shape[1]
    if F > MAX_TRIANGLES:
        raise ValueError(f"tri holds {F} triangles; at most {MAX_TRIANGLES} (2^24 - 1) are supported, the id is stored as an exact float")
    if F > 0:   # one host sync: an index outside [0, V) would be an out-of-bounds read on the device
        lo, hi = torch.aminmax(tri)
        lo, hi = int(lo), int(hi)
        if lo < 0 or hi >= V:
            raise ValueError(f"tri indexes vertices in [{lo}, {hi}], outside [0, {V}) of pos")


def _check_image(B, H, W):
    if H < 1 or W < 1:
        raise ValueError(f"resolution must be at least 1 x 1, got ({H}, {W})")
    if B * H * W >= 1 << 31:
        raise ValueError(f"B * H * W = {B * H * W} pixels: must be below 2^31")


def _check_device(**tensors):
    dev = None
    for name, x in tensors.items():
        if not x.is_cuda:
            raise ValueError(f"{name} must be a CUDA (HIP) tensor: the mesh rasterizer has no CPU path")
        if dev is None:
            dev = x.device
        elif x.device != dev:
            raise ValueError(f"{name} is on {x.device}, expected {dev}")
    return dev


def _check_rasterize(pos, tri, resolution, ranges):
    if ranges is not None:
        raise ValueError("ranges (nvdiffrast's range mode) is not supported: pass pos as (B, V, 4)")
    _check_pos_tri(pos, tri)
    try:
        H, W = (int(r) for r in resolution)
    except (TypeError, ValueError):
        raise TypeError(f"resolution must be (H, W), got {resolution!r}") from None
    _check_image(pos.shape[0], H, W)
    return H, W, _check_device(pos=pos, tri=tri)


def _check_antialias(color, rast, pos, tri, topology_hash):
    if topology_hash is not None:
        raise ValueError("topology_hash is not supported: pass None (the edge adjacency is built on every call)")
    _tensor("color", color, torch.float32, 4)
    _tensor("rast", rast, torch.float32, 4)
    _check_pos_tri(pos, tri)
    B, H, W, Cn = color.shape
    if Cn < 1:
        raise ValueError("color must have at least one channel")
    if tuple(rast.shape) != (B, H, W, 4):
        raise ValueError(f"rast {tuple(rast.shape)} does not match color {tuple(color.shape)}: expected {(B, H, W, 4)}")
    if pos.shape[0] != B:
        raise ValueError(f"pos holds {pos.shape[0]} batch elements, color {B}")
    _check_image(B, H, W)
    return _check_device(color=color, rast=rast, pos=pos, tri=tri)


# ---- edge adjacency ------------------------------------------------------------------------------------------------------------------
def edge_neighbours(tri: torch.Tensor, num_vertices: int) -> torch.Tensor:
    """(F, 3) int32: for edge k = (tri[f, k], tri[f, (k+1) % 3]) of triangle f, the other triangle on that edge, -1 for a boundary edge,
    -2 for an edge shared by more than two triangles.  Sort and unique on tri's device (any device); built on every call, never cached:
    the caller hands a fresh `faces.int()` each time and the allocator reuses addresses."""
    F = tri.shape[0]
    if F == 0:
        return torch.empty((0, 3), dtype=torch.int32, device=tri.device)
    t = tri.long()
    a = t
    b = t[:, [1, 2, 0]]
    key = (torch.minimum(a, b) * num_vertices + torch.maximum(a, b)).reshape(-1)   # one key per (triangle, edge)
    skey, order = torch.sort(key, stable=True)
    _, inv, counts = torch.unique_consecutive(skey, return_inverse=True, return_counts=True)
    start = torch.cumsum(counts, 0) - counts
    cnt = counts[inv]
    pos_in_group = torch.arange(key.numel(), device=tri.device) - start[inv]
    partner = (start[inv] + (1 - pos_in_group)).clamp(0, key.numel() - 1)
    nb_sorted = torch.where(cnt == 1, torch.full_like(cnt, -1), torch.where(cnt == 2, order[partner] // 3, torch.full_like(cnt, -2)))
    nb = torch.empty_like(nb_sorted)
    nb[order] = nb_sorted
    return nb.reshape(F, 3).to(torch.int32)


# ---- launches --------------------------------------------------------------------------------------------------------------------------
def _ptr(x):
    return C.c_void_p(x.data_ptr()) if x.numel() > 0 else None


def _rasterize(pos, tri, H, W, dev):
    lib = _lib.gmr()
    B, V, F = pos.shape[0], pos.shape[1], tri.shape[0]
    rast = torch.empty((B, H, W, 4), dtype=torch.float32, device=dev)
    nbytes = lib.gmr_workspace_bytes(B, F)
    ws = torch.empty((max(nbytes, 0),), dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        rc = lib.gmr_rasterize(B, V, F, H, W, _ptr(pos), _ptr(tri), _ptr(rast), _ptr(ws), C.c_void_p(_lib.raw_stream(dev)))
    if rc != 0:
        raise RuntimeError(f"gmr_rasterize failed: {_lib.gmr_error()}")
    return rast, torch.empty((B, H, W, 0), dtype=torch.float32, device=dev)


def _antialias(color, rast, pos, tri, dev):
    lib = _lib.gmr()
    B, H, W, Cn = color.shape
    V, F = pos.shape[1], tri.shape[0]
    nb = edge_neighbours(tri, V)
    out = torch.empty_like(color)
    with _lib.on_device(dev):
        rc = lib.gmr_antialias(B, V, F, H, W, Cn, _ptr(color), _ptr(rast), _ptr(pos), _ptr(tri), _ptr(nb), _ptr(out),
                               C.c_void_p(_lib.raw_stream(dev)))
    if rc != 0:
        raise RuntimeError(f"gmr_antialias failed: {_lib.gmr_error()}")
    return out


class _ForwardOnly(torch.autograd.Function):
    """Hangs the outputs off a node whose backward refuses: the overlay has no gradient, and it must never come back silently
    wrong or silently missing."""

    @staticmethod
    def forward(ctx, run, *inputs):
        out = run()
        return out

    @staticmethod
    def backward(ctx, *grads):
        raise NotImplementedError("the mesh overlay (gaussianavatars_amd.mesh_raster: rasterize / antialias) is forward-only: "
                                  "it has no gradient with respect to pos or color")


def _needs_node(*xs):
    return torch.is_grad_enabled() and any(x.requires_grad for x in xs)


# ---- public entry points -------------------------------------------------------------------------------------------------------------
def rasterize(glctx, pos, tri, resolution, ranges=None, grad_db=True):
    """nvdiffrast.torch.rasterize in instanced mode: pos (B, V, 4) float32 clip space, tri (F, 3) int32, resolution (H, W).

    Returns (rast, rast_db): rast (B, H, W, 4) = (u, v, z/w, triangle_id + 1), all zeros where nothing covers; rast_db is (B, H, W, 0),
    nvdiffrast's grad_db=False form, whatever grad_db says: image-space derivatives are not computed (no caller reads them).
    `glctx` is accepted and ignored.  Forward only: a backward through the outputs raises NotImplementedError."""
    H, W, dev = _check_rasterize(pos, tri, resolution, ranges)
    pos_c, tri_c = pos.detach().contiguous(), tri.contiguous()
    if _needs_node(pos):
        return _ForwardOnly.apply(lambda: _rasterize(pos_c, tri_c, H, W, dev), pos)
    return _rasterize(pos_c, tri_c, H, W, dev)


def antialias(color, rast, pos, tri, topology_hash=None, pos_gradient_boost=1.0):
    """nvdiffrast.torch.antialias: color (B, H, W, C) float32 blended across the silhouette edges found in rast (as rasterize wrote it)
    with pos (B, V, 4) and tri (F, 3).  Same shape as color.  pos_gradient_boost is accepted and ignored (no backward).
    Forward only: a backward through the output raises NotImplementedError."""
    dev = _check_antialias(color, rast, pos, tri, topology_hash)
    args = (color.detach().contiguous(), rast.detach().contiguous(), pos.detach().contiguous(), tri.contiguous(), dev)
    if _needs_node(color, pos):
        return _ForwardOnly.apply(lambda: _antialias(*args), color, pos)
    return _antialias(*args)
