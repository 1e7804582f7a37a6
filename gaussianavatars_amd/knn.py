"""The reference's `simple_knn._C.distCUDA2` (scene/gaussian_model.py:190-192): per point the mean SQUARED distance to its 3 nearest other
points, what `create_from_pcd` initialises the scales of an unbound model from.

    dist2_knn3(points, fused=None) -> (N,) fp32
        a device tensor goes to include/gdc.h's gdc_knn3_dist2 on the current stream: an exact search on the spatial order (17 launches, no host
        read, no allocation inside the library)
    dist2_knn3_composed(points) -> (N,) fp32
        the same contract in chunked torch on whatever device the points live on: the DIFFERENCE form (p_i - p_j)^2, summed (x + y) + z, the
        point itself masked by index, `topk`.  O(N^2): the CPU path and the opt-out (`fused=False`, GAA_FUSED_KNN=0).

Both detach their input and take any float dtype and any strides; the values are fp32.  With N - 1 < 3 neighbours the mean is over the
neighbours there are, N == 1 gives 0, N == 0 an empty tensor.

A CPU tensor, `fused=False` or GAA_FUSED_KNN=0 is the composed path.  That is a statement about the domain, not a substitute for a missing
kernel: for a device tensor a missing libgdc_hip.so is an error (the rule of densify.py).
"""
from __future__ import annotations

import os

import torch

from . import _lib

__all__ = ["dist2_knn3", "dist2_knn3_composed"]

_WS = {}   # (device index, raw stream) -> gdc_knn3_dist2's scratch, grown when a larger cloud arrives; never shared between two streams


def _points(points):
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3 or not points.is_floating_point():
        raise ValueError("points must be a floating-point tensor of shape (N, 3)")
    return points.detach().to(torch.float32).contiguous()


def _workspace(dev, stream, nbytes):
    """The (device, stream)'s scratch, as densify._order_workspace keeps its own.  Under stream capture nothing is cached: a scratch made there
    lives in that graph's private pool."""
    key = (dev.index, stream)
    held = _WS.get(key)
    if held is not None and held.numel() * 4 >= nbytes:
        return held
    held = torch.empty(max(nbytes // 4, 1024), dtype=torch.int32, device=dev)
    if not torch.cuda.is_current_stream_capturing():
        _WS[key] = held
    return held


@torch.no_grad()
def dist2_knn3_composed(points):
    """include/gdc.h's value in composed torch (see the module text)."""
    p = _points(points)
    n, dev = p.shape[0], p.device
    out = torch.zeros(n, dtype=torch.float32, device=dev)
    k = min(3, n - 1)
    if k <= 0:
        return out
    chunk = max(1, min(n, (1 << 24) // n))   # ~64 MB of fp32 per (chunk, N) plane
    cols = torch.arange(n, device=dev)
    count = torch.full((), float(k), dtype=torch.float32, device=dev)   # (a tensor: a device divides by a host scalar as a multiplication by 1 / k)
    for s in range(0, n, chunk):
        e = min(s + chunk, n)
        d = (p[s:e, None, :] - p[None, :, :]).square()
        d2 = (d[..., 0] + d[..., 1]) + d[..., 2]
        d2[cols[: e - s], cols[s:e]] = float("inf")   # the point itself, by index: a duplicate stays a neighbour at 0
        near = torch.topk(d2, k, dim=1, largest=False, sorted=True).values
        if k == 3:
            out[s:e] = ((near[:, 0] + near[:, 1]) + near[:, 2]) / count
        else:
            out[s:e] = near.sum(1) / count
    return out


@torch.no_grad()
def dist2_knn3(points, fused=None):
    """Mean squared distance of every row of `points` (N, 3) to its 3 nearest other rows, (N,) fp32 in the rows' order (see the module text)."""
    if fused is None:
        fused = os.environ.get("GAA_FUSED_KNN", "1") != "0"
    if not isinstance(points, torch.Tensor) or points.device.type != "cuda" or not fused:
        return dist2_knn3_composed(points)
    p = _points(points)
    dev, P = p.device, p.shape[0]
    lib = _lib.gdc()
    nbytes = lib.gdc_knn_workspace_bytes(P)
    if nbytes < 0:
        raise ValueError(f"N = {P} is outside [0, {_lib.GDC_MAX_SPLATS})")
    with _lib.on_device(dev):
        stream = _lib.raw_stream(dev)
        out = torch.empty(P, dtype=torch.float32, device=dev)
        ws = _workspace(dev, stream, nbytes)
        if lib.gdc_knn3_dist2(P, p.data_ptr(), out.data_ptr(), ws.data_ptr(), stream) != 0:
            raise RuntimeError(f"gdc_knn3_dist2 failed: {_lib.gdc_error()}")
    return out
