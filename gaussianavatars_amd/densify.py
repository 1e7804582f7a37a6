"""Adaptive density control (include/gdc.h): the reference's `densify_and_prune` (scene/gaussian_model.py:501-515 -- densify_and_clone,
densify_and_split and two prune_points, three passes of boolean-mask indexing and `cat` over six parameters and twelve Adam moments, a dozen
counts read back) as five launches and ONE host read.

    densify_and_prune(model, max_grad, min_opacity, extent, max_screen_size, noise=None)
        the whole call on a live model -- this package's mirror classes or the reference's own (same attribute names): the six leaves, their
        Adam moments inside `model.optimizer` (torch.optim.Adam or an adopted optim.FusedAdam; `step` is kept, non-splat groups are left
        alone), xyz_gradient_accum / denom / max_radii2D, binding / binding_counter and `_gaa_order`
    density_control_fused / density_control_composed
        the same contract on bare tensors: the kernels, and its composed-torch fp32 statement (what runs outside the kernels' domain for the
        mirror classes, the A/B leg of tools/densify_timing.py and the error bar of tests/test_densify_gpu.py)
    prune_points / reset_opacity / prune_optimizer / replace_tensor
        the remaining optimiser surgery of the training loop, composed torch, for classes that do not bring their own
    morton_permutation / permute_rows
        the spatial re-sort that follows a densification (gaussian_model.spatial_resort), on bare device tensors: io.morton_order's permutation
        bit for bit, and every per-splat tensor moved by it in one launch -- nothing is copied to the host and nothing synchronises

`noise` (2, P, 3) are the unit normals of the split's children, child c of splat i from noise[c, i].  None draws torch.randn(2, P, 3) on the
device: the same distribution as the reference's torch.normal(mean=0, std=scaling), NOT the same stream -- a seeded reference run and a seeded
run of this function place their children differently.

Outside the domain -- CPU tensors, a leaf or moment that is not contiguous fp32, a splat group without optimizer state, no optimizer, a stream
being captured, or GAA_FUSED_DENSIFY=0 -- the call is the original composed method, bit for bit: `fallback` (the reference's own
densify_and_prune, patch.py passes it) or, for the mirror classes, density_control_composed.  That is a statement about the domain, not a
substitute for a missing kernel: inside the domain a missing libgdc_hip.so is an error.
"""
from __future__ import annotations

import ctypes as C
import os

import torch
from torch import nn

from . import _lib

__all__ = ["densify_and_prune", "density_control_fused", "density_control_composed", "prune_points", "reset_opacity", "prune_optimizer",
           "replace_tensor", "morton_permutation", "permute_rows", "SPLAT_GROUPS"]

#: optimizer group name -> leaf attribute (scene/gaussian_model.py:213-220)
SPLAT_GROUPS = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
                "rotation": "_rotation"}
_KIND = {"_xyz": _lib.GDC_XYZ, "_scaling": _lib.GDC_SCALING}


def _dense(t, dev, dtype=torch.float32) -> bool:
    return isinstance(t, torch.Tensor) and t.dtype is dtype and t.device == dev and t.layout is torch.strided and t.is_contiguous()


def _row_floats(t) -> int:
    return t.numel() // t.shape[0] if t.shape[0] else int(torch.Size(t.shape[1:]).numel())


def _check_noise(noise, P, dev):
    if not (isinstance(noise, torch.Tensor) and tuple(noise.shape) == (2, P, 3) and noise.dtype is torch.float32 and noise.device == dev
            and noise.is_contiguous()):
        raise ValueError(f"noise must be a contiguous fp32 tensor of shape (2, {P}, 3) on {dev}")


# ------------------------------------------------------------------------------------------------
# the contract on bare tensors
# ------------------------------------------------------------------------------------------------
@torch.no_grad()
def density_control_fused(leaves, moments, accum, denom, noise, max_grad, min_opacity, extent, percent_dense, max_screen_size=None,
                          binding=None, face_scaling=None, binding_counter=None):
    """include/gdc.h on device tensors.  leaves: {attribute: (P, ...) fp32}; moments: {attribute: (exp_avg, exp_avg_sq)} or None.  Returns
    {"leaves", "moments", "src", "xyz_gradient_accum", "denom", "max_radii2D", "binding", "binding_counter", "totals"}; every output is a new
    tensor.  Arguments outside the kernels' domain raise: the callers decide about falling through."""
    xyz = leaves["_xyz"]
    dev, P = xyz.device, xyz.shape[0]
    if dev.type != "cuda":
        raise RuntimeError("density_control_fused needs device tensors: there is no CPU implementation")
    for k in SPLAT_GROUPS.values():
        if not _dense(leaves[k], dev) or leaves[k].shape[0] != P:
            raise ValueError(f"{k} must be a contiguous fp32 tensor of {P} rows on {dev}")
        if moments is not None and not all(_dense(m, dev) and m.shape == leaves[k].shape for m in moments[k]):
            raise ValueError(f"the moments of {k} must be contiguous fp32 tensors of its shape")
    if tuple(leaves["_xyz"].shape[1:]) != (3,) or tuple(leaves["_scaling"].shape[1:]) != (3,) or tuple(leaves["_rotation"].shape[1:]) != (4,) \
            or _row_floats(leaves["_opacity"]) != 1:
        raise ValueError("_xyz / _scaling are (P, 3), _rotation is (P, 4), _opacity is (P, 1)")
    if not (_dense(accum, dev) and _dense(denom, dev) and accum.numel() == P == denom.numel()):
        raise ValueError("xyz_gradient_accum / denom must be contiguous fp32 tensors of P elements")
    _check_noise(noise, P, dev)
    if not float(max_grad) > 0:
        raise ValueError("max_grad must be > 0")
    F, is64 = 0, 0
    if binding is not None:
        if binding.dtype not in (torch.int32, torch.int64) or not _dense(binding, dev, binding.dtype) or binding.shape != (P,):
            raise ValueError("binding must be a contiguous int32 / int64 tensor of P elements")
        if not _dense(binding_counter, dev, torch.int32) or binding_counter.dim() != 1:
            raise ValueError("binding_counter must be a contiguous int32 vector")
        F = binding_counter.shape[0]
        if not _dense(face_scaling, dev) or face_scaling.numel() < F:
            raise ValueError("face_scaling must be a contiguous fp32 tensor of at least F elements")
        is64 = 1 if binding.dtype is torch.int64 else 0
    lib = _lib.gdc()
    nbytes = lib.gdc_workspace_bytes(P, F)
    if nbytes < 0:
        raise ValueError(f"P = {P} is outside [0, {_lib.GDC_MAX_SPLATS})")
    ptr = lambda t: None if t is None else t.data_ptr()
    params = _lib.GdcParams(float(max_grad), float(min_opacity), float(extent), float(percent_dense), float(max_screen_size or 0))
    totals = (C.c_int32 * 4)()
    with _lib.on_device(dev):
        stream = _lib.raw_stream(dev)
        ws = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
        counter_out = None if binding is None else torch.empty_like(binding_counter)
        if lib.gdc_plan(P, F, C.byref(params), ptr(leaves["_scaling"]), ptr(leaves["_opacity"]), ptr(accum), ptr(denom), ptr(binding), is64,
                        ptr(face_scaling), ptr(binding_counter), ptr(counter_out), ptr(ws), totals, stream) != 0:
            raise RuntimeError(f"gdc_plan failed: {_lib.gdc_error()}")
        N = sum(totals)
        new = lambda t: torch.empty((N,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)
        out_leaves = {k: new(leaves[k]) for k in SPLAT_GROUPS.values()}
        out_moments = None if moments is None else {k: (new(moments[k][0]), new(moments[k][1])) for k in SPLAT_GROUPS.values()}
        stats = [torch.empty((N, 1), device=dev), torch.empty((N, 1), device=dev), torch.empty((N,), device=dev)]
        src = torch.empty(N, dtype=torch.int32, device=dev)
        binding_out = None if binding is None else torch.empty(N, dtype=binding.dtype, device=dev)
        rows = []
        for k in SPLAT_GROUPS.values():
            rf = _row_floats(leaves[k])
            rows.append((ptr(leaves[k]), ptr(out_leaves[k]), rf, _KIND.get(k, _lib.GDC_COPY)))
            if moments is not None:
                rows += [(ptr(m), ptr(o), rf, _lib.GDC_MOMENT) for m, o in zip(moments[k], out_moments[k])]
        rows += [(None, ptr(s), 1, _lib.GDC_ZERO) for s in stats]
        table = (_lib.GdcTensor * len(rows))(*rows)
        if lib.gdc_emit(P, F, totals, len(rows), table, ptr(xyz), ptr(leaves["_scaling"]), ptr(leaves["_rotation"]), ptr(noise), ptr(binding), is64,
                        ptr(face_scaling), ptr(src), ptr(binding_out), ptr(ws), stream) != 0:
            raise RuntimeError(f"gdc_emit failed: {_lib.gdc_error()}")
    return {"leaves": out_leaves, "moments": out_moments, "src": src, "xyz_gradient_accum": stats[0], "denom": stats[1], "max_radii2D": stats[2],
            "binding": binding_out, "binding_counter": counter_out, "totals": tuple(totals)}


@torch.no_grad()
def density_control_composed(leaves, moments, accum, denom, noise, max_grad, min_opacity, extent, percent_dense, max_screen_size=None,
                             binding=None, face_scaling=None, binding_counter=None):
    """The same contract, same arguments and same result dict, in composed torch at the tensors' own precision and device (CPU included):
    one decision per splat, boolean-mask indexing and `cat`."""
    xyz = leaves["_xyz"]
    dev, P = xyz.device, xyz.shape[0]
    if noise is not None and tuple(noise.shape) != (2, P, 3):
        raise ValueError(f"noise must have shape (2, {P}, 3)")
    g = accum.reshape(-1) / denom.reshape(-1)
    g[g.isnan()] = 0.0
    bound = binding is not None
    b = binding.long() if bound else None
    fs = face_scaling.reshape(-1)[b][:, None] if bound else None
    e = torch.exp(leaves["_scaling"])
    w = e * fs if bound else e
    S = w.max(dim=1).values if P else w.new_zeros(0)
    o = torch.sigmoid(leaves["_opacity"]).reshape(-1)
    dense, big = percent_dense * extent, 0.1 * extent
    clone = (g.abs() >= max_grad) & (S <= dense)
    split = (g >= max_grad) & (S > dense)
    c_scaling = torch.log((w / fs if bound else e) / 1.6)
    ce = torch.exp(c_scaling)
    S_child = (ce * fs if bound else ce).max(dim=1).values if P else S
    low = o < min_opacity
    cand_row = low | (S > big) if max_screen_size else low
    cand_child = low | (S_child > big) if max_screen_size else low
    counter = None
    if bound:
        nf = binding_counter.shape[0]
        cnt = binding_counter.long() + torch.bincount(b[clone | split], minlength=nf)
        n_cand = torch.where(split, 2 * cand_child.long(), cand_row.long() * (1 + clone.long()))
        cand = torch.zeros(nf, dtype=torch.long, device=dev).scatter_add_(0, b, n_cand)
        remove_f = cnt - cand > 0
        remove = remove_f[b]
        counter = (cnt - torch.where(remove_f, cand, torch.zeros_like(cand))).to(binding_counter.dtype)
    else:
        remove = torch.ones(P, dtype=torch.bool, device=dev)
    keep_row, keep_child = ~(cand_row & remove), ~(cand_child & remove)
    idx = torch.arange(P, device=dev)
    kids = idx[split & keep_child]
    seg = [idx[~split & keep_row], idx[clone & keep_row], kids, kids]
    source = torch.cat(seg)
    n0, n2, N = seg[0].shape[0], kids.shape[0], source.shape[0]
    out_leaves = {k: leaves[k][source] for k in SPLAT_GROUPS.values()}
    if n2:
        q = leaves["_rotation"][kids]
        q = q / q.norm(dim=1, keepdim=True)
        r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                         2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                         2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3).repeat(2, 1, 1)
        smp = torch.cat([noise[0][kids], noise[1][kids]]) * w[kids].repeat(2, 1)
        out_leaves["_xyz"][N - 2 * n2:] = torch.bmm(R, smp.unsqueeze(-1)).squeeze(-1) + xyz[kids].repeat(2, 1)
        out_leaves["_scaling"][N - 2 * n2:] = c_scaling[kids].repeat(2, 1)
    out_moments = None
    if moments is not None:
        out_moments = {}
        for k in SPLAT_GROUPS.values():
            pair = []
            for m in moments[k]:
                t = m[source]
                t[n0:] = 0
                pair.append(t)
            out_moments[k] = tuple(pair)
    src = torch.where(torch.arange(N, device=dev) < n0, source, -1 - source).to(torch.int32)
    return {"leaves": out_leaves, "moments": out_moments, "src": src, "xyz_gradient_accum": torch.zeros((N, 1), device=dev),
            "denom": torch.zeros((N, 1), device=dev), "max_radii2D": torch.zeros((N,), device=dev),
            "binding": binding[source] if bound else None, "binding_counter": counter,
            "totals": (n0, seg[1].shape[0], n2, n2)}


# ------------------------------------------------------------------------------------------------
# the spatial order on bare tensors (include/gdc.h, ABI 2)
# ------------------------------------------------------------------------------------------------
_ORDER_WS = {}   # (device index, raw stream) -> gdc_morton_order's scratch; never shared between two streams


def _order_workspace(dev, stream, nbytes):
    """The (device, stream)'s scratch, grown when a larger model arrives; the library clears what it needs on every call.  Under stream
    capture nothing is cached: a scratch made there lives in that graph's private pool."""
    key = (dev.index, stream)
    held = _ORDER_WS.get(key)
    if held is not None and held.numel() * 4 >= nbytes:
        return held
    held = torch.empty(max(nbytes // 4, 1024), dtype=torch.int32, device=dev)
    if not torch.cuda.is_current_stream_capturing():
        _ORDER_WS[key] = held
    return held


def _morton_i32(xyz, binding, face_centers):
    """morton_permutation as the int32 tensor the library writes."""
    if not isinstance(xyz, torch.Tensor) or xyz.device.type != "cuda":
        raise RuntimeError("morton_permutation needs device tensors: the host statement is io.morton_order")
    dev = xyz.device
    xyz = xyz.detach()
    if not _dense(xyz, dev) or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError("xyz must be a contiguous fp32 tensor of shape (P, 3)")
    P, F, is64 = xyz.shape[0], 0, 0
    if (binding is None) != (face_centers is None):
        raise ValueError("binding and face_centers are given together (a bound model) or not at all")
    if binding is not None:
        if binding.dtype not in (torch.int32, torch.int64) or not _dense(binding, dev, binding.dtype) or binding.shape != (P,):
            raise ValueError("binding must be a contiguous int32 / int64 tensor of P elements")
        if not _dense(face_centers, dev) or face_centers.dim() != 2 or face_centers.shape[1] != 3 or face_centers.shape[0] < 1:
            raise ValueError("face_centers must be a contiguous fp32 tensor of shape (F, 3), F > 0")
        F, is64 = face_centers.shape[0], 1 if binding.dtype is torch.int64 else 0
    lib = _lib.gdc()
    nbytes = lib.gdc_order_workspace_bytes(P)
    if nbytes < 0:
        raise ValueError(f"P = {P} is outside [0, {_lib.GDC_MAX_SPLATS})")
    with _lib.on_device(dev):
        stream = _lib.raw_stream(dev)
        perm = torch.empty(P, dtype=torch.int32, device=dev)
        ws = _order_workspace(dev, stream, nbytes)
        if lib.gdc_morton_order(P, F, xyz.data_ptr(), None if binding is None else binding.data_ptr(), is64,
                                None if face_centers is None else face_centers.data_ptr(), perm.data_ptr(), ws.data_ptr(), stream) != 0:
            raise RuntimeError(f"gdc_morton_order failed: {_lib.gdc_error()}")
    return perm


@torch.no_grad()
def morton_permutation(xyz, binding=None, face_centers=None, dtype=torch.int64):
    """io.morton_order of the positions the splats are ordered by, as a device tensor, bit for bit: `xyz` (P, 3) fp32 for an unbound model,
    `face_centers[binding] + 1e-3 * xyz` in fp32 for a bound one (face_centers (F, 3) fp32, binding int32 / int64).  The library's fifteen
    launches on the current stream; no host read, no synchronisation, so the call can be recorded into a graph.  `dtype`: torch.int64 (what
    indexing wants: one more element-wise kernel) or torch.int32, the tensor the library wrote, which permute_rows takes as it is."""
    if dtype not in (torch.int32, torch.int64):
        raise ValueError("dtype must be torch.int32 or torch.int64")
    perm = _morton_i32(xyz, binding, face_centers)
    return perm if dtype is torch.int32 else perm.long()


@torch.no_grad()
def permute_rows(tensors, perm):
    """[t[perm] for t in tensors] as new tensors, in ONE launch (one more for every further GDC_MAX_TENSORS tensors): contiguous device
    tensors of P rows and 4- or 8-byte elements (an int64 row moves as two 4-byte elements per entry), perm (P,) int32 -- used as it is --
    or int64, which costs one conversion kernel first."""
    tensors = [t.detach() for t in tensors]
    if not isinstance(perm, torch.Tensor) or perm.device.type != "cuda" or perm.dtype not in (torch.int32, torch.int64) or perm.dim() != 1:
        raise ValueError("perm must be an int32 / int64 device vector")
    dev, P = perm.device, perm.shape[0]
    perm = perm.to(torch.int32).contiguous()
    rows = []
    for k, t in enumerate(tensors):
        if not _dense(t, dev, t.dtype) or t.dim() < 1 or t.shape[0] != P or t.element_size() not in (4, 8):
            raise ValueError(f"tensor {k} must be a contiguous tensor of {P} rows of 4- or 8-byte elements on {dev}")
        rows.append(_row_floats(t) * (t.element_size() // 4))
    if P >= _lib.GDC_MAX_SPLATS:
        raise ValueError(f"P = {P} is outside [0, {_lib.GDC_MAX_SPLATS})")
    lib = _lib.gdc()
    out = [torch.empty_like(t) for t in tensors]
    with _lib.on_device(dev):
        stream = _lib.raw_stream(dev)
        for at in range(0, len(tensors), _lib.GDC_MAX_TENSORS):
            part = [(t.data_ptr(), o.data_ptr(), rf, _lib.GDC_COPY) for t, o, rf in
                    zip(tensors[at:at + _lib.GDC_MAX_TENSORS], out[at:at + _lib.GDC_MAX_TENSORS], rows[at:at + _lib.GDC_MAX_TENSORS])]
            table = (_lib.GdcTensor * len(part))(*part)
            if lib.gdc_permute(P, perm.data_ptr(), len(part), table, stream) != 0:
                raise RuntimeError(f"gdc_permute failed: {_lib.gdc_error()}")
    return out


# ------------------------------------------------------------------------------------------------
# a live model
# ------------------------------------------------------------------------------------------------
def _splat_groups(optimizer):
    """{attribute: param group} of the six splat groups; None when the optimizer does not have exactly one single-parameter group of each."""
    found = {}
    for group in optimizer.param_groups:
        name = group.get("name")
        if name in SPLAT_GROUPS:
            if len(group["params"]) != 1 or SPLAT_GROUPS[name] in found:
                return None
            found[SPLAT_GROUPS[name]] = group
    return found if len(found) == len(SPLAT_GROUPS) else None


def _fused_inputs(model):
    """(groups, moments) when the call is inside the kernels' domain, else None."""
    if os.environ.get("GAA_FUSED_DENSIFY", "1") == "0":
        return None
    xyz = getattr(model, "_xyz", None)
    if not isinstance(xyz, torch.Tensor) or xyz.device.type != "cuda" or xyz.shape[0] >= _lib.GDC_MAX_SPLATS:
        return None
    dev, P = xyz.device, xyz.shape[0]
    optimizer = getattr(model, "optimizer", None)
    groups = _splat_groups(optimizer) if optimizer is not None else None
    if groups is None or torch.cuda.is_current_stream_capturing():
        return None
    moments = {}
    for attr, group in groups.items():
        p = group["params"][0]
        state = optimizer.state.get(p)
        if p is not getattr(model, attr) or not _dense(p, dev) or p.shape[0] != P or not state or "exp_avg" not in state or "exp_avg_sq" not in state:
            return None
        m, v = state["exp_avg"], state["exp_avg_sq"]
        if not (_dense(m, dev) and _dense(v, dev) and m.shape == p.shape == v.shape):
            return None
        moments[attr] = (m, v)
    if tuple(model._xyz.shape[1:]) != (3,) or tuple(model._scaling.shape[1:]) != (3,) or tuple(model._rotation.shape[1:]) != (4,) \
            or tuple(model._opacity.shape[1:]) != (1,):
        return None
    for name in ("xyz_gradient_accum", "denom"):
        t = getattr(model, name, None)
        if not _dense(t, dev) or t.numel() != P:
            return None
    b = getattr(model, "binding", None)
    if b is not None:
        c = getattr(model, "binding_counter", None)
        if b.dtype not in (torch.int32, torch.int64) or not _dense(b, dev, b.dtype) or b.shape != (P,) or not _dense(c, dev, torch.int32) or c.dim() != 1:
            return None
    return groups, moments


def _face_scaling(model):
    if getattr(model, "binding", None) is None:
        return None
    if model.face_scaling is None:          # the reference's accessors initialise the mesh lazily (scene/gaussian_model.py:119-120)
        model.select_mesh_by_timestep(0)
    return model.face_scaling.detach()


def _install(model, out, P):
    """Puts the result of density_control_* into the model: parameters and moments into the optimizer (state re-keyed, `step` kept; groups that
    are not splat groups untouched), statistics, binding, binding_counter and `_gaa_order`."""
    optimizer = getattr(model, "optimizer", None)
    groups = _splat_groups(optimizer) if optimizer is not None else None
    for attr in SPLAT_GROUPS.values():
        old = getattr(model, attr)
        p = nn.Parameter(out["leaves"][attr].requires_grad_(True))
        group = None if groups is None else groups[attr]
        if group is not None and group["params"][0] is old:
            state = optimizer.state.get(old)
            if state is not None:
                del optimizer.state[old]
                if out["moments"] is not None and "exp_avg" in state:
                    state["exp_avg"], state["exp_avg_sq"] = out["moments"][attr]
                optimizer.state[p] = state
            group["params"][0] = p
        setattr(model, attr, p)
    model.xyz_gradient_accum, model.denom, model.max_radii2D = out["xyz_gradient_accum"], out["denom"], out["max_radii2D"]
    if out["binding"] is not None:
        model.binding, model.binding_counter = out["binding"], out["binding_counter"]
    # survivors keep their entry, new rows get -1 -- what patch._hook_spatial_order's wrappers of prune_points / densification_postfix produce
    order = getattr(model, "_gaa_order", None)
    if isinstance(order, torch.Tensor) and order.shape[0] == P:
        src = out["src"].to(order.device).long()
        model._gaa_order = torch.where(src >= 0, order[src.clamp(min=0)], torch.full_like(src, -1).to(order.dtype))
    else:
        model._gaa_order, model._gaa_order_lost = None, True


def _model_tensors(model, with_state):
    leaves = {attr: getattr(model, attr).detach() for attr in SPLAT_GROUPS.values()}
    moments = None
    optimizer = getattr(model, "optimizer", None)
    groups = _splat_groups(optimizer) if (with_state and optimizer is not None) else None
    if groups is not None:
        states = {a: optimizer.state.get(g["params"][0]) for a, g in groups.items()}
        if all(s and "exp_avg" in s and "exp_avg_sq" in s and g["params"][0] is getattr(model, a) for (a, g), s in zip(groups.items(), states.values())):
            moments = {a: (s["exp_avg"], s["exp_avg_sq"]) for a, s in states.items()}
    return leaves, moments


@torch.no_grad()
def densify_and_prune(model, max_grad, min_opacity, extent, max_screen_size, noise=None, fallback=None):
    """The reference's GaussianModel.densify_and_prune on `model` (see the module text).  Returns None, as the reference does."""
    P = model._xyz.shape[0]
    fused = _fused_inputs(model)
    if fused is None and fallback is not None:
        if noise is not None:
            raise ValueError("noise is only taken by the fused path: this call is outside its domain and runs the model's original method")
        return fallback(model, max_grad, min_opacity, extent, max_screen_size)
    dev = model._xyz.device
    if noise is None:
        noise = torch.randn(2, P, 3, device=dev)
    else:
        _check_noise(noise, P, dev)
    fs = _face_scaling(model)
    args = (model.xyz_gradient_accum, model.denom, noise, max_grad, min_opacity, extent, model.percent_dense, max_screen_size,
            getattr(model, "binding", None), None if fs is None else fs.contiguous(), getattr(model, "binding_counter", None))
    if fused is not None:
        leaves = {attr: getattr(model, attr).detach() for attr in SPLAT_GROUPS.values()}
        out = density_control_fused(leaves, fused[1], *args)
    else:
        out = density_control_composed(*_model_tensors(model, True), *args)
    _install(model, out, P)
    return None


def prune_optimizer(optimizer, index):
    """scene/gaussian_model.py:349-369 for any optimizer: every single-parameter group whose parameter has as many rows as `index` (a keep-mask
    or a permutation) is indexed with it, its moments too; returns {group name: new parameter}."""
    moved = {}
    for group in optimizer.param_groups:
        if len(group["params"]) != 1 or group["params"][0].shape[0] != index.shape[0]:
            continue
        old = group["params"][0]
        state = optimizer.state.get(old)
        p = nn.Parameter(old.detach()[index].requires_grad_(True))
        if state is not None:
            del optimizer.state[old]
            if "exp_avg" in state:
                state["exp_avg"], state["exp_avg_sq"] = state["exp_avg"][index], state["exp_avg_sq"][index]
            optimizer.state[p] = state
        group["params"][0] = p
        moved[group["name"]] = p
    return moved


def replace_tensor(optimizer, tensor, name):
    """scene/gaussian_model.py:334-347: the parameter of group `name` becomes `tensor`, its moments zero; `step` is kept."""
    moved = {}
    for group in optimizer.param_groups:
        if group.get("name") != name:
            continue
        old = group["params"][0]
        state = optimizer.state.get(old)
        p = nn.Parameter(tensor.requires_grad_(True))
        if state is not None:
            del optimizer.state[old]
            state["exp_avg"], state["exp_avg_sq"] = torch.zeros_like(tensor), torch.zeros_like(tensor)
            optimizer.state[p] = state
        group["params"][0] = p
        moved[name] = p
    return moved


@torch.no_grad()
def prune_points(model, mask):
    """scene/gaussian_model.py:371-398 in composed torch: removes the rows of `mask`, except that a face keeps its splats when the mask would
    take its last one (`mask` is narrowed IN PLACE to what is really removed, as the reference narrows it)."""
    if getattr(model, "binding", None) is not None:
        b = model.binding[mask].long()
        taken = torch.zeros_like(model.binding_counter).scatter_add_(0, b, torch.ones_like(b, dtype=model.binding_counter.dtype))
        mask[mask.clone()] = ((model.binding_counter - taken) > 0)[b]
    keep = ~mask
    optimizer = getattr(model, "optimizer", None)
    if optimizer is not None:
        moved = prune_optimizer(optimizer, keep)
        for name, attr in SPLAT_GROUPS.items():
            setattr(model, attr, moved[name])
    else:
        for attr in SPLAT_GROUPS.values():
            p = getattr(model, attr)
            setattr(model, attr, nn.Parameter(p.detach()[keep].requires_grad_(p.requires_grad)))
    model.xyz_gradient_accum, model.denom, model.max_radii2D = model.xyz_gradient_accum[keep], model.denom[keep], model.max_radii2D[keep]
    if getattr(model, "binding", None) is not None:
        b = model.binding[mask].long()
        model.binding_counter.scatter_add_(0, b, -torch.ones_like(b, dtype=model.binding_counter.dtype))
        model.binding = model.binding[keep]


@torch.no_grad()
def reset_opacity(model):
    """scene/gaussian_model.py:277-280: opacities above 0.01 are set to 0.01 (in logit space), the opacity moments to zero."""
    o = torch.sigmoid(model._opacity.detach()).clamp(max=0.01)
    logit = torch.log(o / (1 - o))
    optimizer = getattr(model, "optimizer", None)
    if optimizer is not None:
        model._opacity = replace_tensor(optimizer, logit, "opacity")["opacity"]
    else:
        model._opacity = nn.Parameter(logit.requires_grad_(True))
