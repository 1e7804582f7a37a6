"""Seeded inputs of tests/golden/landmark_pins.npz (written by tests/golden/make_landmark_pins.py from the reference's own lbs module; read by
tests/test_landmarks_cpu.py and tests/test_landmarks_gpu.py) and the hand-made embeddings of those tests.  TEST INFRASTRUCTURE: no reference
import here, this module travels to the GPU box.  The float64 / CPU-fp32 values come from gaussianavatars_amd/unfused.py, which the CPU test
pins to the recorded reference outputs."""
import functools
import os

import numpy as np
import torch

from gaussianavatars_amd import synthetic as S
from gaussianavatars_amd import unfused as U
from tests import binding_ref as BR

PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "landmark_pins.npz")
RIG_SEED = 4                      # synthetic.flame_rig(4): the full-size rig of model_pins (V = 5143, F = 10144 -- the embedding's faces reach 8905)
VERT_STRIDE = 8                   # the pins keep every 8th vertex row (643 of 5143): a few kB per array instead of 123
POSES = ("rest", "random", "jaw_neck", "still_translated")
LEAVES = ("shape", "expr", "rotation", "neck_pose", "jaw_pose", "eyes_pose", "translation", "static_offset")


@functools.lru_cache(maxsize=None)
def rig():
    return S.flame_rig(RIG_SEED)


@functools.lru_cache(maxsize=None)
def pose_inputs(name):
    """Batch-1 FLAME inputs (fp32, the reference's shapes).  rest: small rotations, zero translation; random: five rotations of 0.3 rad and a
    translation; jaw_neck: a jaw of 0.7 rad and a neck of 0.9 rad under a global rotation of 2 rad; still_translated: every rotation exactly
    zero (the 1e-8 convention of batch_rodrigues) and a translation of decimetres."""
    r = rig()
    V, nb = r["v_template"].shape[0], r["shapedirs"].shape[2]
    g = np.random.default_rng(5100 + POSES.index(name))
    unit = lambda n: (lambda x: x / np.linalg.norm(x))(g.normal(size=n))
    amp = dict(rest=0.02, random=0.3, jaw_neck=0.3, still_translated=0.0)[name]
    p = dict(shape=g.normal(0, 1.0, (1, S.N_SHAPE)), expr=g.normal(0, 0.7, (1, nb - S.N_SHAPE)), rotation=amp * unit(3)[None], neck_pose=amp * unit(3)[None],
             jaw_pose=amp * unit(3)[None], eyes_pose=np.concatenate([amp * unit(3), amp * unit(3)])[None], translation=g.normal(0, 0.01, (1, 3)),
             static_offset=g.normal(0, 2e-4, (1, V, 3)))
    if name == "rest":
        p["translation"] = np.zeros((1, 3))
    elif name == "jaw_neck":
        p["rotation"], p["neck_pose"] = 2.0 * unit(3)[None], 0.9 * unit(3)[None]
        p["jaw_pose"] = np.array([[0.66, 0.18, -0.15]])
    elif name == "still_translated":
        p["translation"] = np.array([[0.31, -0.22, 0.47]])
    return {k: np.ascontiguousarray(v, np.float32) for k, v in p.items()}


@functools.lru_cache(maxsize=None)
def pins():
    z = np.load(PINS)
    return {k: z[k] for k in z.files}


def embedding():
    """(full_lmk_faces_idx (L,) int64, full_lmk_bary_coords (L,3) fp32) of the reference's landmark_embedding_with_eyes.npy, from the pins
    (stored in the file's own (1,L) / (1,L,3) layout and dtype)."""
    z = pins()
    return z["full_lmk_faces_idx"][0].astype(np.int64), z["full_lmk_bary_coords"][0].astype(np.float32)


def torch_rig(r, dtype, dev="cpu"):
    out = {k: torch.as_tensor(r[k]).to(dtype).to(dev) for k in BR.RIG_BUFFERS}
    out["parents"] = torch.as_tensor(r["parents"])
    return out


def unfused_eval(r, p, faces, lmk_idx, lmk_bary, dtype, zero_centered=False, leaves=None):
    """unfused.flame_forward + unfused.landmarks in `dtype` on the CPU -> (verts (1,V,3), v_shaped, landmarks (1,L,3), leaves dict)."""
    if leaves is None:
        leaves = {k: torch.as_tensor(p[k]).to(dtype) for k in LEAVES}
    verts, vs = U.flame_forward(torch_rig(r, dtype), *[leaves[k] for k in LEAVES[:-1]], leaves["static_offset"], zero_centered_at_root_node=zero_centered)
    lm = U.landmarks(verts, torch.as_tensor(faces).long(), torch.as_tensor(lmk_idx).long(), torch.as_tensor(lmk_bary).to(dtype))
    return verts, vs, lm, leaves


# ---- hand-made embeddings ---------------------------------------------------------------------------------------------------------------
SHARED_V = 7
SHARED_FACES = np.array([[0, 1, 2], [2, 3, 4], [4, 2, 5], [5, 6, 0]], np.int64)
# landmarks 0, 1, 2 (and 4, on face 1 again) meet in vertex 2 -- as corners k = 2, 0, 1 (and 0); landmark 3 sits ON vertex 5: bary (1, 0, 0)
SHARED_LMK_FACE = np.array([0, 1, 2, 3, 1], np.int64)
SHARED_LMK_BARY = np.array([[0.2, 0.3, 0.5], [0.6, 0.1, 0.3], [0.25, 0.5, 0.25], [1.0, 0.0, 0.0], [0.1, 0.7, 0.2]], np.float32)


@functools.lru_cache(maxsize=None)
def small_case():
    """The 257-vertex rig of tests/binding_ref.py (10 shape, 100 expression coefficients, 514 faces; two blocks of the per-vertex kernels) with
    the real embedding's barycentric coordinates on its faces folded into the small mesh (index mod 514: landmarks that share a face and
    faces that share vertices remain), and the random pose of binding_ref.flame_case."""
    r, p, _ = BR.flame_case(257, 10, 100, "random")
    idx, bary = embedding()
    return r, p, idx % r["faces"].shape[0], bary
