#!/usr/bin/env python3
"""Generates tests/golden/pcd_init_pins.npz by RUNNING THE REFERENCE's own `create_from_pcd` (scene/gaussian_model.py:172-206, the read-only
checkout at /root/reference, as tests/golden/make_densify_golden.py uses it) on the CPU, under tests/ref_cpu_env's device neutralisation.
Run by hand, once; the tests only read the file.  Arrays only: the inputs and the six leaves (plus max_radii2D).

    free/    GaussianModel(3).create_from_pcd(pcd, 2.5): 300 points of a cloud centred at (4, -2, 7) with 5e-2 spread, colours uniform in [0, 1)
    bound/   the `pcd=None` branch on a FlameGaussianModel (built without its licence-gated asset files: the base constructor, a binding of
             F = 37 faces and a unit mesh, as make_densify_golden.py does) after np.random.seed(1234): the colours are the global numpy stream's

In the generator `distCUDA2` -- the name scene/gaussian_model.py imported from simple_knn._C -- is replaced by the float64 brute force of
tests/knn_ref.py, rounded to fp32 once: the fixture's scales do not inherit any fp32 search's error.
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

from tests import knn_ref  # noqa: E402
from tests import ref_cpu_env  # noqa: E402

LEAVES = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
SEED, F, SH = 1234, 37, 3


def leaves_of(m):
    out = {k: getattr(m, k).detach().numpy().copy() for k in LEAVES}
    out["max_radii2D"] = m.max_radii2D.numpy().copy()
    return out


def main():
    ref_cpu_env._no_cuda()
    from gaussianavatars_amd import shims

    shims.install(stub_torchvision=True)   # the absent third-party imports of scene/*.py
    import scene.gaussian_model as ref_gm
    from scene.flame_gaussian_model import FlameGaussianModel as RefFGM

    RefGM = ref_gm.GaussianModel
    assert not getattr(RefGM, "_gaa_patched", False), "pins must come from the UNPATCHED reference class"
    ref_gm.distCUDA2 = lambda pts: torch.from_numpy(knn_ref.brute_force(pts.detach().numpy()).astype(np.float32))

    arrays = {}
    rng = np.random.default_rng(300)
    points = (rng.normal(0, 5e-2, (300, 3)) + np.array([4.0, -2.0, 7.0])).astype(np.float32)
    colors = rng.random((300, 3)).astype(np.float32)
    m = RefGM(SH)
    m.create_from_pcd(types.SimpleNamespace(points=points, colors=colors, normals=np.zeros_like(points)), 2.5)
    assert m.spatial_lr_scale == 2.5
    arrays.update({"free/in_points": points, "free/in_colors": colors, "free/spatial_lr_scale": np.float64(2.5), "free/sh": np.int64(SH)})
    arrays.update({"free/out" + k if k.startswith("_") else "free/out_" + k: v for k, v in leaves_of(m).items()})
    assert float(np.exp(arrays["free/out_scaling"]).min()) > 10 * np.sqrt(1e-7), "the clamp must not be what the fixture pins"

    b = RefFGM.__new__(RefFGM)
    RefGM.__init__(b, SH)
    b.binding = torch.arange(F)
    b.binding_counter = torch.ones(F, dtype=torch.int32)
    b.face_center, b.face_orien_mat = torch.zeros(F, 3), torch.eye(3).repeat(F, 1, 1)
    b.face_scaling, b.face_orien_quat = torch.ones(F, 1), torch.tensor([1.0, 0, 0, 0]).repeat(F, 1)
    np.random.seed(SEED)
    b.create_from_pcd(None, 1.0)
    arrays.update({"bound/seed": np.int64(SEED), "bound/F": np.int64(F), "bound/sh": np.int64(SH), "bound/spatial_lr_scale": np.float64(1.0)})
    arrays.update({"bound/out" + k if k.startswith("_") else "bound/out_" + k: v for k, v in leaves_of(b).items()})

    path = os.path.join(HERE, "pcd_init_pins.npz")
    np.savez_compressed(path, **arrays)
    for k, v in arrays.items():
        print(k, np.asarray(v).shape, np.asarray(v).dtype)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
