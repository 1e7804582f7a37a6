"""Shared by tests/test_resort_cpu.py and tests/test_resort_gpu.py: seeded mirror models with a template mesh, an optimizer that has taken one
real step, statistics and a tracked `_gaa_order`, and the host statement of the positions the splats are ordered by."""
import types

import numpy as np
import torch

from gaussianavatars_amd import io as gio

LEAVES = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
STATS = ("xyz_gradient_accum", "denom", "max_radii2D")
ARGS = types.SimpleNamespace(percent_dense=0.01, position_lr_init=1.6e-4, position_lr_final=1.6e-6, position_lr_delay_mult=0.01,
                             position_lr_max_steps=1000, feature_lr=2.5e-3, opacity_lr=5e-2, scaling_lr=5e-3, rotation_lr=1e-3,
                             flame_pose_lr=1e-5, flame_trans_lr=1e-6, flame_expr_lr=1e-3)


def host_positions(xyz, binding=None, centers=None):
    """What gaussian_model.spatial_resort orders by, as numpy computes it there: fp32, `centers[binding] + 1e-3 * xyz` for a bound model."""
    xyz = np.asarray(xyz, np.float32)
    if binding is None or centers is None:
        return xyz
    return np.asarray(centers, np.float32)[np.asarray(binding).astype(np.int64)] + 1e-3 * xyz


def host_order(xyz, binding=None, centers=None):
    return torch.from_numpy(gio.morton_order(host_positions(xyz, binding, centers)))


def template(F, seed):
    """A template mesh of F faces as the stand-in for flame_model: (v_template (V, 3) fp32, faces (F, 3) long)."""
    rng = np.random.default_rng(seed)
    V = F + 2
    v = rng.normal(0, 0.2, (V, 3)).astype(np.float32)
    faces = np.stack([np.arange(F), np.arange(F) + 1, np.arange(F) + 2], 1)
    return torch.from_numpy(v), torch.from_numpy(faces)


def splat_arrays(P, F, sh, seed, i64=False):
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    K = (sh + 1) ** 2 - 1
    arrs = {"_xyz": f32(rng.normal(0, 0.3, (P, 3))), "_features_dc": f32(rng.normal(0, 1, (P, 1, 3))),
            "_features_rest": f32(rng.normal(0, 0.1, (P, K, 3))), "_opacity": f32(rng.normal(0, 1, (P, 1))),
            "_scaling": f32(rng.normal(-3, 0.5, (P, 3))), "_rotation": f32(rng.normal(0, 1, (P, 4))), "binding": None}
    if F:
        b = rng.integers(0, F, P)
        b[:min(P, F)] = np.arange(min(P, F))
        arrs["binding"] = b.astype(np.int64 if i64 else np.int32)
    return arrs


def make_model(P, F, sh, dev, seed=0, optimizer=True, step=True, i64=False, tracked=True):
    """A mirror GaussianModel on `dev`; the optimizer kind follows GAA_FUSED_ADAM (set it before the call)."""
    from gaussianavatars_amd.gaussian_model import GaussianModel

    m = GaussianModel(sh)
    m.load_arrays(splat_arrays(P, F, sh, seed, i64), device=dev)
    if F:
        v, faces = template(F, seed + 1)
        m.flame_model = types.SimpleNamespace(v_template=v.to(dev), faces=faces.to(dev))
    gen = torch.Generator().manual_seed(seed + 2)
    if optimizer:
        m.training_setup(ARGS)
        m.optimizer.add_param_group({"params": [torch.nn.Parameter(torch.zeros(4, 3, device=dev))], "lr": 1e-5, "name": "pose"})
        if step:
            for k in LEAVES:     # one real step: the optimizer's own state
                getattr(m, k).grad = (torch.randn(getattr(m, k).shape, generator=gen) * 1e-3).to(dev)
            m.optimizer.step()
            m.optimizer.zero_grad(set_to_none=True)
    m.xyz_gradient_accum = torch.rand((P, 1), generator=gen).to(dev)
    m.denom = torch.randint(0, 40, (P, 1), generator=gen).float().to(dev)
    m.max_radii2D = (torch.rand((P,), generator=gen) * 50).to(dev)
    if tracked:
        m._gaa_order = torch.arange(P, device=dev).flip(0)
    return m


def cpu_twin(m):
    """The model's tensors, optimizer state (`step` included) and bookkeeping copied to a new model on the CPU."""
    from gaussianavatars_amd.gaussian_model import GaussianModel

    t = GaussianModel(m.max_sh_degree)
    arrs = {k: getattr(m, k).detach().cpu().numpy().copy() for k in LEAVES}
    arrs["binding"] = None if m.binding is None else m.binding.cpu().numpy().copy()
    t.load_arrays(arrs, device="cpu")
    for k in LEAVES:
        getattr(t, k).requires_grad_(getattr(m, k).requires_grad)
    fm = getattr(m, "flame_model", None)
    if fm is not None:
        t.flame_model = types.SimpleNamespace(v_template=fm.v_template.cpu().clone(), faces=fm.faces.cpu().clone())
    if getattr(m, "optimizer", None) is not None:
        t.training_setup(ARGS)
        t.optimizer.add_param_group({"params": [torch.nn.Parameter(m.optimizer.param_groups[-1]["params"][0].detach().cpu().clone())], "lr": 1e-5,
                                     "name": "pose"})
        for k in LEAVES:
            s = m.optimizer.state.get(getattr(m, k))
            if s:
                t.optimizer.state[getattr(t, k)] = {"step": s["step"].clone(), "exp_avg": s["exp_avg"].cpu().clone(),
                                                    "exp_avg_sq": s["exp_avg_sq"].cpu().clone()}
    for k in STATS:
        setattr(t, k, getattr(m, k).cpu().clone())
    order = getattr(m, "_gaa_order", None)
    if order is not None:
        t._gaa_order = order.cpu().clone()
    return t


def snapshot(m):
    """Every per-splat tensor of the model as CPU clones: leaves, moments, statistics, binding and `_gaa_order`."""
    out = {k: getattr(m, k).detach().cpu().clone() for k in LEAVES + STATS}
    out["binding"] = None if m.binding is None else m.binding.cpu().clone()
    order = getattr(m, "_gaa_order", None)
    out["_gaa_order"] = None if order is None else order.cpu().clone()
    if getattr(m, "optimizer", None) is not None:
        for k in LEAVES:
            s = m.optimizer.state.get(getattr(m, k))
            if s:
                out["m" + k], out["v" + k] = s["exp_avg"].cpu().clone(), s["exp_avg_sq"].cpu().clone()
    return out


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype is torch.float32:
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)
