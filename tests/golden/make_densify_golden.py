#!/usr/bin/env python3
"""Generates tests/golden/densify_pins.npz by RUNNING THE REFERENCE's own `training_setup` + `densify_and_prune` (scene/gaussian_model.py, the
read-only checkout at /root/reference, as tests/golden/make_golden.py uses it) on the CPU, under tests/ref_cpu_env's device neutralisation.
Run by hand, once; the tests only read the file.  Arrays only: inputs, the unit normals the reference consumed, and its end state.

`torch.normal` is wrapped for the call: it draws z = randn and returns mean + z * std, and z is what is recorded, scattered into the
(2, P, 3) layout of include/gdc.h (child c of splat i reads noise[c, i]).

Cases (percent_dense 0.01, extent 5, max_grad 2e-4, min_opacity 5e-3):
    bound_sh3   F = 16, P = 257, SH 3, max_screen_size 20 with max_radii2D = 1000 everywhere (the term the reference never evaluates)
    bound_sh0   F = 16, P = 257, SH 0, max_screen_size None
    free_sh3    unbound, P = 64, SH 3, max_screen_size None
    free_sh0    unbound, P = 64, SH 0, max_screen_size 20, max_radii2D = 1000
every one with denom == 0 rows (accum 0 -> g = 0, accum > 0 -> g = +inf) and, when bound, face 5 made of prune candidates only and
face 9 with candidates and one healthy splat.  g, S and o keep at least 1 % away from their thresholds (asserted), so that one ulp of
expf cannot flip a decision.
"""
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

from tests import densify_ref as DR  # noqa: E402
from tests import ref_cpu_env  # noqa: E402

PARAMS = dict(max_grad=2e-4, min_opacity=5e-3, extent=5.0, percent_dense=0.01)
CASES = {"bound_sh3": dict(P=257, F=16, sh=3, mss=20), "bound_sh0": dict(P=257, F=16, sh=0, mss=None),
         "free_sh3": dict(P=64, F=0, sh=3, mss=None), "free_sh0": dict(P=64, F=0, sh=0, mss=20)}
LEAVES = DR.LEAVES


def inputs(name, P, F, sh, mss):
    rng = np.random.default_rng(sum(map(ord, name)))
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    binding = face_scaling = None
    fs = np.ones(P)
    if F:
        binding = rng.integers(0, F, P).astype(np.int32)
        binding[:F] = np.arange(F)                       # every face owns a splat
        face_scaling = f32(rng.uniform(0.5, 2.0, (F, 1)))
        fs = face_scaling[binding, 0].astype(np.float64)
    # world scale: small (clone side), medium (split side), large (split side and above 0.1 * extent, children too)
    target = rng.choice([0.015, 0.15, 1.2], P) * rng.uniform(0.8, 1.2, P)
    axes = rng.uniform(0.3, 1.0, (P, 3))
    axes[np.arange(P), rng.integers(0, 3, P)] = 1.0
    scaling = np.log(target[:, None] * axes / fs[:, None])
    g = PARAMS["max_grad"] * rng.choice([0.2, 3.0], P) * rng.uniform(0.8, 1.2, P)
    denom = rng.integers(1, 40, P).astype(np.float64)
    accum = g * denom
    denom[3::17] = 0                                     # never seen: accum 0 -> NaN -> 0
    accum[3::17] = 0
    denom[5::29] = 0                                     # (cannot happen in training; +inf must be kept)
    low = rng.random(P) < 0.25
    o = np.where(low, rng.uniform(0.001, 0.004, P), rng.uniform(0.1, 0.9, P))
    if F:
        on5, on9 = binding == 5, binding == 9
        o[on5] = rng.uniform(0.001, 0.004, on5.sum())    # face 5: candidates only -> all kept
        o[on9] = rng.uniform(0.001, 0.004, on9.sum())    # face 9: candidates and one healthy, quiet splat -> candidates go
        i9 = np.flatnonzero(on9)[0]
        o[i9], target_i9 = 0.5, 0.02
        scaling[i9] = np.log(target_i9 * axes[i9] / fs[i9])
        accum[i9], denom[i9] = 0.2 * PARAMS["max_grad"] * 7, 7
    K = (sh + 1) ** 2 - 1
    leaves = {"_xyz": f32(rng.normal(0, 0.3, (P, 3))), "_features_dc": f32(rng.normal(0, 1, (P, 1, 3))),
              "_features_rest": f32(rng.normal(0, 0.1, (P, K, 3))), "_opacity": f32(np.log(o / (1 - o)))[:, None],
              "_scaling": f32(scaling), "_rotation": f32(rng.normal(0, 1, (P, 4)))}
    return leaves, f32(accum)[:, None], f32(denom)[:, None], binding, face_scaling, rng


def run_case(name, RefGM, P, F, sh, mss):
    leaves, accum, denom, binding, face_scaling, rng = inputs(name, P, F, sh, mss)
    m = RefGM(sh)
    for k, v in leaves.items():
        setattr(m, k, torch.nn.Parameter(torch.tensor(v)))
    m.spatial_lr_scale = 1.0
    m.max_radii2D = torch.full((P,), 1000.0)
    if F:
        m.binding = torch.tensor(binding)
        m.binding_counter = torch.bincount(m.binding.long(), minlength=F).int()
        m.face_scaling = torch.tensor(face_scaling)
        # (training_setup and densification_postfix read get_xyz.shape[0]: a mesh has to be present, its frames do not enter the result)
        m.face_center, m.face_orien_mat = torch.zeros(F, 3), torch.eye(3).repeat(F, 1, 1)
        m.face_orien_quat = torch.tensor([1.0, 0, 0, 0]).repeat(F, 1)
    counter_in = None if not F else m.binding_counter.numpy().copy()
    args = types.SimpleNamespace(percent_dense=PARAMS["percent_dense"], position_lr_init=1.6e-4, position_lr_final=1.6e-6, position_lr_delay_mult=0.01,
                                 position_lr_max_steps=1000, feature_lr=2.5e-3, opacity_lr=5e-2, scaling_lr=5e-3, rotation_lr=1e-3)
    m.training_setup(args)
    gen = torch.Generator().manual_seed(7)
    for group in m.optimizer.param_groups:   # one step on random gradients: every group has moments, step == 1
        p = group["params"][0]
        p.grad = torch.randn(p.shape, generator=gen) * 1e-3
    m.optimizer.step()
    m.xyz_gradient_accum, m.denom = torch.tensor(accum), torch.tensor(denom)
    before = {k: getattr(m, k).detach().numpy().copy() for k in LEAVES}
    state = lambda: {k: m.optimizer.state[getattr(m, k)] for k in LEAVES}
    mom_in = {k: (s["exp_avg"].numpy().copy(), s["exp_avg_sq"].numpy().copy()) for k, s in state().items()}

    drawn = []
    real_normal = torch.normal

    def recording_normal(mean, std, **kw):
        z = torch.randn(std.shape, generator=gen)
        drawn.append(z.numpy().copy())
        return mean + z * std

    torch.normal = recording_normal
    try:
        m.densify_and_prune(PARAMS["max_grad"], PARAMS["min_opacity"], PARAMS["extent"], mss)
    finally:
        torch.normal = real_normal
    assert len(drawn) == 1
    noise = rng.normal(0, 1, (2, P, 3)).astype(np.float32)
    ref = DR.densify_ref(before, accum, denom, noise, max_screen_size=mss or 0, binding=binding, face_scaling=face_scaling,
                         binding_counter=counter_in, **PARAMS)
    assert ref["margin"] >= 0.01, (name, ref["margin"])
    sel = np.flatnonzero(ref["split"])
    assert drawn[0].shape == (2 * len(sel), 3), (drawn[0].shape, len(sel))
    noise[0, sel], noise[1, sel] = drawn[0][:len(sel)], drawn[0][len(sel):]
    assert ref["clone"].any() and ref["split"].any() and (ref["cand_row"] & ~ref["split"]).any()

    out = {"P": np.int64(P), "F": np.int64(F), "sh": np.int64(sh), "max_screen_size": np.float64(mss or 0), "noise": noise,
           "in_accum": accum, "in_denom": denom, "in_max_radii2D": np.full((P,), 1000.0, np.float32)}
    for k, v in PARAMS.items():
        out[k] = np.float64(v)
    for k in LEAVES:
        out["in" + k], out["in_m" + k], out["in_v" + k] = before[k], mom_in[k][0], mom_in[k][1]
        out["out" + k] = getattr(m, k).detach().numpy().copy()
        s = m.optimizer.state[getattr(m, k)]
        out["out_m" + k], out["out_v" + k] = s["exp_avg"].numpy().copy(), s["exp_avg_sq"].numpy().copy()
        assert float(s["step"]) == 1.0
    out["out_accum"], out["out_denom"], out["out_max_radii2D"] = m.xyz_gradient_accum.numpy().copy(), m.denom.numpy().copy(), m.max_radii2D.numpy().copy()
    if F:
        out["in_binding"], out["in_face_scaling"], out["in_binding_counter"] = binding, face_scaling, counter_in
        out["out_binding"], out["out_binding_counter"] = m.binding.numpy().copy(), m.binding_counter.numpy().copy()
        assert np.array_equal(out["out_binding_counter"], np.bincount(out["out_binding"], minlength=F))
    print(f"{name}: P {P} -> {out['out_xyz'].shape[0]} rows; clone {int(ref['clone'].sum())} split {int(ref['split'].sum())} "
          f"candidates {int(ref['cand_row'].sum())} margin {ref['margin']:.3f}")
    return {f"{name}/{k}": v for k, v in out.items()}


def main():
    ref_cpu_env._no_cuda()
    from gaussianavatars_amd import shims

    shims.install(stub_torchvision=True)   # the absent third-party imports of scene/*.py
    from scene.gaussian_model import GaussianModel as RefGM

    assert not getattr(RefGM, "_gaa_patched", False), "pins must come from the UNPATCHED reference class"
    arrays = {}
    for name, c in CASES.items():
        arrays.update(run_case(name, RefGM, **c))
    path = os.path.join(HERE, "densify_pins.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
