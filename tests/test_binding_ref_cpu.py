"""Anchors of the float64 binding reference (tests/binding_ref.py) that tests/test_binding_parity_gpu.py holds the kernels to; no GPU needed.

  pins ......... unfused.py in float64 reproduces the vectors generated from the reference's own lbs / compute_face_orientation code
                 (tests/golden/binding_pins.npz) within the bars tests/test_binding_gpu.py::test_flame_forward_matches_reference_golden uses;
  gradcheck .... its float64 autograd gradients are the derivatives of what it computes (finite differences);
  conditions ... every face set the GPU tests run is far from a switch of rotmat_to_unitquat's branch (so fp32 and float64 take the same one)
                 and reaches all four branches."""
import os

import numpy as np
import pytest
import torch

from gaussianavatars_amd import unfused as U
from tests import binding_ref as BR
from tests.test_binding_gpu import _close

G = os.path.join(os.path.dirname(__file__), "golden")


def test_float64_reference_reproduces_the_reference_projects_pins():
    pins = np.load(os.path.join(G, "binding_pins.npz"))
    d = lambda a: torch.as_tensor(a).double()
    rig = {k[4:]: (d(pins[k]) if pins[k].dtype.kind == "f" else torch.as_tensor(pins[k])) for k in pins.files if k.startswith("rig_")}
    betas, pose = d(pins["betas"]), d(pins["pose"])
    verts, v_shaped = U.flame_forward(rig, betas[:, :30], betas[:, 30:], pose[:, 0:3], pose[:, 3:6], pose[:, 6:9], pose[:, 9:15], d(pins["trans"]),
                                      d(pins["static_offset"]))
    assert verts.dtype == torch.float64
    t = torch.as_tensor
    _close(v_shaped, t(pins["v_shaped"]), 2e-5, "v_shaped vs reference")
    _close(verts, t(pins["verts"]), 2e-5, "verts vs reference lbs")
    c, R, s, q = U.face_frames(verts[0], t(pins["faces"]).long())
    _close(c, t(pins["face_center"]), 2e-5, "face_center")
    _close(R, t(pins["face_R"]), 5e-5, "face_orien_mat vs compute_face_orientation")
    _close(s, t(pins["face_scale"]), 2e-5, "face_scaling")
    qs = t(pins["face_quat_xyzw_scipy"]).double()
    qx = torch.roll(q, -1, dims=-1)
    _close(qx * torch.sign((qx * qs).sum(1, keepdim=True)), qs, 1e-4, "face_orien_quat vs SciPy")


def _leaf(a):
    return torch.as_tensor(a).double().requires_grad_(True)


def test_gradcheck_flame_forward():
    rig, p, _ = BR.flame_case(37, 3, 5)
    R = BR._torch_rig(rig, torch.float64)
    ins = [_leaf(p[k]) for k in BR.FLAME_LEAVES]
    assert torch.autograd.gradcheck(lambda *a: U.flame_forward(R, *a), ins, eps=1e-6, atol=1e-7, rtol=1e-5)


def test_gradcheck_flame_forward_at_zero_pose():
    """unfused.rodrigues adds 1e-8 to the vector before the norm: well defined, and differentiable, at r == 0 (angle 1.7e-8)."""
    rig, p, _ = BR.flame_case(37, 3, 5, "zero")
    R = BR._torch_rig(rig, torch.float64)
    ins = [_leaf(p[k]) for k in BR.FLAME_LEAVES]
    out = U.flame_forward(R, *ins)
    assert all(bool(torch.isfinite(o).all()) for o in out)
    g = torch.autograd.grad(out[0].sum() + out[0][0, :, 0].square().sum(), ins)
    assert all(bool(torch.isfinite(x).all()) for x in g)


def test_gradcheck_face_frames_on_non_degenerate_faces():
    rig = BR.small_rig(37, 3, 5)
    verts, faces = rig["v_template"], rig["faces"][:60]
    assert not BR.degenerate(verts, faces).any()
    R = U.face_frames(torch.as_tensor(verts).double(), torch.as_tensor(faces))[1].numpy()
    assert BR.quat_branches(R)[1].min() > 1e-3   # (finite differences of 1e-6 stay inside one branch)
    assert torch.autograd.gradcheck(lambda v: U.face_frames(v, torch.as_tensor(faces)), [_leaf(verts)], eps=1e-7, atol=1e-5, rtol=1e-4)


def test_gradcheck_bind_functions():
    leaves, binding, _ = BR.bind_case(65, True)
    b = torch.as_tensor(binding)
    L = {k: _leaf(leaves[k]) for k in BR.BIND_LEAVES}
    L["_scaling"] = _leaf(np.clip(leaves["_scaling"], -3.0, 2.0))   # (exp(-8) outputs are below gradcheck's absolute tolerance)
    assert torch.autograd.gradcheck(lambda x, R, s, c: U.bind_xyz(x, b, R, s, c), [L["_xyz"], L["face_R"], L["face_scale"], L["face_center"]],
                                    eps=1e-6, atol=1e-7, rtol=1e-5)
    assert torch.autograd.gradcheck(lambda ls, s: U.bind_scaling(ls, b, s), [L["_scaling"], L["face_scale"]], eps=1e-6, atol=1e-8, rtol=1e-5)
    assert torch.autograd.gradcheck(lambda q, fq: U.bind_rotation(q, b, fq), [L["_rotation"], L["face_quat"]], eps=1e-6, atol=1e-7, rtol=1e-5)


def test_face_sets_of_the_gpu_tests_are_well_conditioned():
    """(a) on each non-degenerate face the largest and second largest of (R00, R11, R22, trace) differ by more than 1e-3: a fp32 evaluation
    (error ~1e-6) picks the branch float64 picks; (b) all four branches occur.  (b) cannot hold for fewer than four faces: the one-face set
    is the first face of the 257-face set, which is held to it; the hand-built degenerate set (two regular faces) is held to (a) only."""
    for name, (verts, faces) in BR.face_sets().items():
        deg = BR.degenerate(verts, faces)
        R = U.face_frames(torch.as_tensor(verts).double(), torch.as_tensor(faces))[1].numpy()
        branch, margin = BR.quat_branches(R)
        counts = np.bincount(branch[~deg], minlength=4)
        print(f"{name}: {len(faces)} faces, {int(deg.sum())} degenerate; branches (R00, R11, R22, trace) = {counts.tolist()}; "
              f"smallest margin {margin[~deg].min():.3e}")
        assert margin[~deg].min() > 1e-3, f"{name}: a face within 1e-3 of a branch switch (change the seed of the set)"
        if len(faces) >= 40:
            assert (counts >= 1).all(), f"{name}: branch counts {counts.tolist()}"
    assert np.array_equal(BR.face_case(1)[1], BR.face_case(257)[1][:1]) and np.array_equal(BR.face_case(1)[0], BR.face_case(257)[0])
    assert BR.degenerate(*BR.degenerate_case()[:2]).tolist() == [True, True, True, True, False, False]


def test_bind_sets_have_empty_and_crowded_faces():
    for N in (1, 63, 64, 65, 1000):
        _, binding, _ = BR.bind_case(N, False)
        counts = np.bincount(binding, minlength=BR.BIND_F)
        assert len(counts) == BR.BIND_F and all(counts[f] == 0 for f in BR.BIND_EMPTY)
        if N == 1000:
            assert counts[BR.BIND_HEAVY] > 300
            assert (counts > 0).sum() == BR.BIND_F - len(BR.BIND_EMPTY)
    leaves = BR.bind_case(1000, True)[0]
    n = np.linalg.norm(leaves["_rotation"], axis=1)
    assert 0.2 <= n.min() < 0.3 and 4.0 < n.max() <= 5.0001
    fn = np.linalg.norm(leaves["face_quat"], axis=1)
    assert 0.5 <= fn.min() < 0.7 and 1.5 < fn.max() <= 2.0001
    assert np.allclose(np.linalg.norm(BR.bind_case(1000, False)[0]["face_quat"], axis=1), 1.0, atol=1e-6)


def test_row_err_sees_a_small_wrong_row_that_a_whole_tensor_error_does_not():
    ref = np.ones((4, 3))
    ref[2] = 1e-3
    got = ref.copy()
    got[2, 0] *= 1.01                    # 1 % of a row a thousand times smaller than the largest: 1e-5 of the tensor's max
    assert abs(got - ref).max() / abs(ref).max() < 2e-5
    assert BR.row_err(got, ref) > 4e-3
    assert BR.row_err(ref, ref) == 0.0 and BR.row_err(np.zeros((2, 3)), np.zeros((2, 3))) == 0.0
    assert BR.row_err(np.full((2, 3), 1e-30), np.zeros((2, 3))) == float("inf")      # a row that must be exactly zero
    assert BR.row_err(np.array([[np.nan, 1.0]]), np.ones((1, 2))) == float("inf")
    assert BR.bar("x", 0.0) == BR.FLOOR and BR.bar("x", 1e-3) == BR.FACTOR * 1e-3
