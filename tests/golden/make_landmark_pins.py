#!/usr/bin/env python3
"""Generates tests/golden/landmark_pins.npz by RUNNING THE REFERENCE's own `flame_model/lbs.py` (read-only checkout beside this repository) on
the CPU in float64 -- it does not travel to the GPU box, so what it produces is committed, as make_frame_pins.py's results are.

    python tests/golden/make_landmark_pins.py

The reference's FlameHead cannot be constructed here (the licensed flame2023.pkl is absent, and flame.py imports pytorch3d), so this calls what
`FlameHead.forward` calls (flame_model/flame.py:511-553) -- `lbs.blend_shapes`, `lbs.lbs`, `lbs.vertices2landmarks`, the reference's functions,
unmodified -- on the arrays of the synthetic full-size rig (gaussianavatars_amd.synthetic.flame_rig(4), the rig of model_pins.npz; V = 5143,
F = 10144), with the reference's own landmark embedding.  The lines of forward() between those calls (static offset, root centring,
translation, the `.repeat(bz, 1)` of the embedding) are restated below one to one.

Recorded (numeric arrays only):

    full_lmk_faces_idx (1,70) int64, full_lmk_bary_coords (1,70,3) float64
                          the two arrays of flame_model/assets/flame/landmark_embedding_with_eyes.npy that FlameHead registers, re-saved
    vert_rows             the vertex rows kept below (every tests/landmark_cases.VERT_STRIDE-th)
    for each pose of tests/landmark_cases.POSES (inputs: landmark_cases.pose_inputs, seeded, not stored):
    <pose>_verts          (rows,3)  vertices,              zero_centered_at_root_node=False
    <pose>_landmarks      (70,3)    landmarks of those
    <pose>_verts_rc       (rows,3)  vertices,              zero_centered_at_root_node=True
    <pose>_landmarks_rc   (70,3)    landmarks of those
    <pose>_root           (3,)      J[:, 0] as lbs returns it (the posed root joint, before the translation)

Also CHECKED here, on every pose: the posed root joint lbs returns equals row 0 of vertices2joints(J_regressor, v_shaped) bit for bit (the
identity include/gab_landmarks.h's gab_root_joint relies on: the root's transform has the rest joint as its translation column, lbs.py:283-296).
"""
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

from flame_model import lbs as ref_lbs  # noqa: E402  (the reference's)

from tests import landmark_cases as LC  # noqa: E402


def reference_forward(rig, p, lmk_idx, lmk_bary, zero_centered):
    """flame.py:509-553 in float64; every function called is the reference's."""
    t = lambda a: torch.as_tensor(a).double()
    faces = torch.as_tensor(rig["faces"]).long()
    shape, expr = t(p["shape"]), t(p["expr"])
    batch_size = shape.shape[0]
    betas = torch.cat([shape, expr], dim=1)
    full_pose = torch.cat([t(p["rotation"]), t(p["neck_pose"]), t(p["jaw_pose"]), t(p["eyes_pose"])], dim=1)
    template_vertices = t(rig["v_template"]).unsqueeze(0).expand(batch_size, -1, -1)
    v_shaped = template_vertices + ref_lbs.blend_shapes(betas, t(rig["shapedirs"]))
    v_shaped = v_shaped + t(p["static_offset"])
    vertices, J, _ = ref_lbs.lbs(full_pose, v_shaped, t(rig["posedirs"]), t(rig["J_regressor"]), torch.as_tensor(rig["parents"]).long(),
                                 t(rig["lbs_weights"]), dtype=torch.float64)
    rest_root = ref_lbs.vertices2joints(t(rig["J_regressor"]), v_shaped)[:, 0]
    assert torch.equal(J[:, 0], rest_root), "the posed root joint is not the rest root joint"
    root = J[0, 0].clone()
    if zero_centered:
        vertices = vertices - J[:, [0]]
    vertices = vertices + t(p["translation"])[:, None, :]
    bz = vertices.shape[0]
    landmarks = ref_lbs.vertices2landmarks(vertices, faces, torch.as_tensor(lmk_idx).long().repeat(bz, 1), t(lmk_bary).repeat(bz, 1, 1))
    return vertices[0].numpy(), landmarks[0].numpy(), root.numpy()


def main():
    emb = np.load(os.path.join(REF, "flame_model", "assets", "flame", "landmark_embedding_with_eyes.npy"), allow_pickle=True, encoding="latin1")[()]
    idx, bary = np.asarray(emb["full_lmk_faces_idx"]), np.asarray(emb["full_lmk_bary_coords"])
    assert idx.shape == (1, 70) and bary.shape == (1, 70, 3)
    bary32 = bary.astype(np.float32)   # what FlameHead registers (flame.py:140-143: dtype=self.dtype), widened exactly below
    rig = LC.rig()
    assert 0 <= idx.min() and idx.max() < rig["faces"].shape[0]
    rows = np.arange(0, rig["v_template"].shape[0], LC.VERT_STRIDE)
    out = dict(full_lmk_faces_idx=idx.astype(np.int64), full_lmk_bary_coords=bary.astype(np.float64), vert_rows=rows.astype(np.int64))
    for name in LC.POSES:
        p = LC.pose_inputs(name)
        v, lm, root = reference_forward(rig, p, idx, bary32, False)
        v_rc, lm_rc, root_rc = reference_forward(rig, p, idx, bary32, True)
        assert np.array_equal(root, root_rc)
        out.update({name + "_verts": v[rows], name + "_landmarks": lm, name + "_verts_rc": v_rc[rows], name + "_landmarks_rc": lm_rc, name + "_root": root})
        print(f"{name}: |verts| <= {np.abs(v).max():.3f}, root {root}, |landmarks - root-centred landmarks| = {np.abs(lm - lm_rc).max():.3f}")
    path = os.path.join(HERE, "landmark_pins.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
